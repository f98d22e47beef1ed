// step_body.hpp — the part of a timestep that the single-rank loop (shstep_run_device) and the loop over all ranks
// (shhalo_run_device) share: what is enqueued before the forward exchange and after the reverse exchange.  The
// functions only enqueue on the given stream (shstep_run.cpp): nothing is allocated, synchronised or read back, so
// they may be captured into a graph.  Internal: nothing here is part of the boundary.
#pragma once
#include "../../include/shhalo.h"
#include "../../include/shstep.h"

namespace shp {

struct StepView {
  int nlocal;
  double *x, *v, *quat, *angmom, *f, *torque;
  const int *shtype, *mask;
  int groupbit;
  double dt;
  const double* gravity;   // [3]
  double gamma_t, gamma_r;
};

inline StepView step_view(const shstep_arrays* a)
{
  return {a->nlocal, a->x, a->v, a->quat, a->angmom, a->f, a->torque, a->shtype, a->mask, a->groupbit, a->dt, a->gravity,
          a->gamma_t, a->gamma_r};
}

inline StepView step_view(const shhalo_arrays* a, const shhalo_run_params* p)
{
  return {a->nlocal, a->x, a->v, a->quat, a->angmom, a->f, a->torque, a->shtype, a->mask, p->groupbit, p->dt, p->gravity,
          p->gamma_t, p->gamma_r};
}

// gravity or viscous drag: all zero, and the loops enqueue no post_force pass
inline bool step_has_body_forces(const StepView& s)
{
  return s.gravity[0] != 0.0 || s.gravity[1] != 0.0 || s.gravity[2] != 0.0 || s.gamma_t != 0.0 || s.gamma_r != 0.0;
}

int step_first_half(shpair_ctx* c, const StepView& s, void* stream);      // initial_integrate: half kick + drift
int step_after_reverse(shpair_ctx* c, const StepView& s, void* stream);   // walls, body forces, final_integrate
// Contact dissipation (SPEC §2.10, §2.11) in two halves, both between the first half kick and the reverse exchange.
// Nothing is enqueued by either while the coefficients it serves are 0.
//  step_twists: (w, omega) of the owned rows and `nghost` ghost rows of the rank's own borders into the step state's
//   twist buffer, from the half-step v, angmom and the drifted quat (also what a damped wall pass reads).  The
//   single-rank loop passes its ghosts (periodic images: they take their owners' rows); the loop over all ranks passes 0
//   and lets the forward exchange bring the ghost rows' twists from their owners.
//  step_dissipation_pass: the pair damping and friction wrench of the last compute's integrals on those twists, over owned +
//   ghost rows (shstep_pair_dissipation_device; s.shtype holds the ghost rows too);
//   behind it, while a rolling or twisting coefficient is set (SPEC §2.16), shstep_pair_rolling_device on the same
//   integrals and twists; the ghost rows' shares go home with the reverse exchange.
int step_twists(shpair_ctx* c, const StepView& s, int nghost, void* stream);
int step_dissipation_pass(shpair_ctx* c, const StepView& s, int nghost, const double* x, const int* type, void* stream);

}  // namespace shp
