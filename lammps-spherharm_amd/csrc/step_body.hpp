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
// twists and pair damping (SPEC §2.10), after the pair compute and before the reverse exchange; one rank's loop only
int step_pair_damping(shpair_ctx* c, const StepView& s, int nghost, const double* x, const int* type, void* stream);

}  // namespace shp
