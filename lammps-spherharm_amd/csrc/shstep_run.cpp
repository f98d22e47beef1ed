// shstep_run.cpp — shstep_run_device of include/shstep.h: Verlet::run for one rank, enqueued call by call or replayed
// from captured graphs, and the step body it shares with the loop over all ranks (step_body.hpp).  One step is
//   segment A: first half kick, and on a checking step the displacement test with its flag read-back
//   (the host reads the flags; ghosts and list are rebuilt, and the graphs captured again, when an atom moved)
//   segment B: forward ghosts, clear, pair forces, [twists, pair damping and friction, SPEC §2.10-11, rolling and twisting resistance, §2.16], reverse ghosts, [wall advance, SPEC §2.12], walls, [cylinders, SPEC §2.18], [cones, SPEC §2.22, §2.23], gravity
//   and drag, second half kick
// Host code only: the kernels are launched by the entry points of the shstep_*.hip files and shpair_api.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/shstep.h"
#include "shstep_state.hpp"
#include "step_body.hpp"

using namespace shp;

// The step body both run loops share (step_body.hpp).
int shp::step_first_half(shpair_ctx* c, const StepView& v, void* st)
{
  return shstep_nve_device(c, 0, v.nlocal, v.dt, v.x, v.v, v.quat, v.angmom, v.f, v.torque, v.shtype, v.mask, v.groupbit, st);
}

// Planar walls act on owned particles only, so they come once the reverse exchange has brought the ghost rows'
// contributions home (f and torque of the owned rows are complete pair sums); the body forces read those rows and the
// second half kick consumes them.
int shp::step_after_reverse(shpair_ctx* c, const StepView& v, void* st)
{
  // Translating walls (SPEC §2.12): x is x(t + dt) here, so the planes go to c(t + dt) first — one kernel that updates the
  // wall table in place (a captured one does the same at every replay); nothing while no wall has a normal velocity.
  if (step_walls_advance(c)) RC(shstep_advance_walls_device(c, v.dt, st));
  // (with a wall coefficient set: the twist form, on the twists step_twists left in the step state)
  // (SPEC §2.15, a wall tangential spring: the form with the step's dt; x is x(t + dt) and the twists are the half-step
  // ones, so xi advances by the midpoint rule, as the pair springs do)
  if (step_wall_history(c))
    RC(shstep_wall_contact_device(c, v.nlocal, v.x, v.quat, v.shtype, v.mask, v.groupbit, v.f, v.torque, nullptr, c->step->d_twist.p,
                                  v.dt, st));
  else if (c->step && c->step->walls.nwalls > 0)
    RC(shstep_wall_force_damped_device(c, v.nlocal, v.x, v.quat, v.shtype, v.mask, v.groupbit, v.f, v.torque, nullptr,
                                       step_wall_reads_twists(c) ? c->step->d_twist.p : nullptr, st));
  // Cylindrical container walls (SPEC §2.18), directly behind the planar pass: owned rows only, the twists while a
  // cylinder coefficient is set, rolling and twisting resistance (SPEC §2.21) among them: its kernel runs inside the pass.
  // (The loop over all ranks refuses to run while a cylinder is set.)
  // (SPEC §2.19, a cylinder tangential spring: the form with the step's dt, on the same midpoint twists as §2.15)
  if (step_cyl_history(c))
    RC(shstep_cyl_contact_device(c, v.nlocal, v.x, v.quat, v.shtype, v.mask, v.groupbit, v.f, v.torque, nullptr, c->step->d_twist.p,
                                 v.dt, st));
  else if (step_has_cylinders(c))
    RC(shstep_cylinder_force_device(c, v.nlocal, v.x, v.quat, v.shtype, v.mask, v.groupbit, v.f, v.torque, nullptr,
                                    step_cyl_reads_twists(c) ? c->step->d_twist.p : nullptr, st));
  // Conical container walls (SPEC §2.22), directly behind the cylinder pass: owned rows only, the twists while a cone
  // coefficient is set, rolling and twisting resistance (SPEC §2.24) among them: its kernel runs inside the pass.
  // (The loop over all ranks refuses to run while a cone is set.)
  // (SPEC §2.23, a cone tangential spring: the form with the step's dt, on the same midpoint twists as §2.15 and §2.19)
  if (step_cone_history(c))
    RC(shstep_conic_contact_device(c, v.nlocal, v.x, v.quat, v.shtype, v.mask, v.groupbit, v.f, v.torque, nullptr, c->step->d_twist.p,
                                   v.dt, st));
  else if (step_has_cones(c))
    RC(shstep_cone_force_device(c, v.nlocal, v.x, v.quat, v.shtype, v.mask, v.groupbit, v.f, v.torque, nullptr,
                                step_cone_reads_twists(c) ? c->step->d_twist.p : nullptr, st));
  // Energy ledger (SPEC §2.13): dt times the powers this step's pair dissipation pass and wall pass left, once per step;
  // with the shell ledger on (SPEC §2.20) also the cylinder pass', into the shell accumulator
  if (c->ledger_on) RC(shstep_ledger_fold_device(c, v.dt, st));
  if (step_has_body_forces(v))
    RC(shstep_post_force_device(c, v.nlocal, v.gravity, v.gamma_t, v.gamma_r, v.v, v.quat, v.angmom, v.shtype, v.mask, v.groupbit,
                                v.f, v.torque, st));
  return shstep_nve_device(c, 1, v.nlocal, v.dt, v.x, v.v, v.quat, v.angmom, v.f, v.torque, v.shtype, v.mask, v.groupbit, st);
}

// SPEC §2.10, §2.11: the twists of the rows from the half-step velocities (also what a damped wall pass reads) ...
// Nothing is enqueued while every coefficient is 0.
int shp::step_twists(shpair_ctx* c, const StepView& v, int nghost, void* st)
{
  if (!step_has_dissipation(c)) return SHPAIR_OK;
  return shstep_twist_device(c, v.nlocal, nghost, v.v, v.quat, v.angmom, v.shtype, c->step->d_twist.p, st);
}

// ... and, between the pair compute and the reverse exchange, the pair wrench of damping and friction, whose ghost rows
// go home with the reverse.  Nothing is enqueued while every pair coefficient is 0.  Behind it, while a rolling or
// twisting coefficient is set (SPEC §2.16), the pass of the two resisting couples: on the same integrals and twists,
// torques only, alone or beside whichever pair pass ran.
int shp::step_dissipation_pass(shpair_ctx* c, const StepView& v, int nghost, const double* x, const int* type, void* st)
{
  if (shp_has_pair_pass(c)) {
    // SPEC §2.14: x is x(t + dt) and the twists are the half-step ones, so xi advances by the midpoint rule
    if (c->hist_on)
      RC(shstep_pair_contact_device(c, v.nlocal, nghost, x, type, v.shtype, c->step->d_twist.p, 1, v.dt, v.f, v.torque, st));
    else
      RC(shstep_pair_dissipation_device(c, v.nlocal, nghost, x, type, v.shtype, c->step->d_twist.p, 1, v.f, v.torque, st));
  }
  if (shp_has_rolling(c)) RC(shstep_pair_rolling_device(c, v.nlocal, nghost, x, type, c->step->d_twist.p, 1, v.torque, st));
  return SHPAIR_OK;
}

namespace {

// The graph executables of a replayed run, and the one place that destroys them.  They hold kernel arguments (ghost
// and pair counts, the context's list and x-hold buffers): captured once and again after every rebuild.
struct StepGraphs {
  hipGraphExec_t a = nullptr, a_nocheck = nullptr, b = nullptr;   // segment A with / without the displacement test, segment B
  void reset()
  {
    for (hipGraphExec_t* g : {&a, &a_nocheck, &b}) {
      if (*g) (void)hipGraphExecDestroy(*g);
      *g = nullptr;
    }
  }
  ~StepGraphs() { reset(); }
};

struct Run {
  shpair_ctx* c;
  shstep_state* s;
  const shstep_arrays* a;
  hipStream_t st;
  bool use_graph;
  int nghost, nreb;
  StepGraphs g;
};

int enqueue_a(Run& r, bool with_check)
{
  RC(step_first_half(r.c, step_view(r.a), r.st));
  if (with_check) RC(step_enqueue_displacement(r.c, r.s, r.a->nlocal, r.a->x, true, r.st));
  return SHPAIR_OK;
}

int enqueue_b(Run& r)
{
  shpair_ctx* c = r.c;
  const shstep_arrays* a = r.a;
  const size_t nall = (size_t)a->nlocal + r.nghost;
  RC(shstep_forward_device(c, a->x, a->quat, r.st));
  RC(shstep_force_clear_device(c, (int)nall, a->f, a->torque, r.st));
  RC(shpair_compute_device(c, a->nlocal, r.nghost, a->x, a->quat, a->type, a->shtype, 1, 0, 0, a->f, a->torque, nullptr, r.st));
  RC(step_twists(c, step_view(a), r.nghost, r.st));
  RC(step_dissipation_pass(c, step_view(a), r.nghost, a->x, a->type, r.st));
  RC(shstep_reverse_device(c, a->f, a->torque, r.st));
  return step_after_reverse(c, step_view(a), r.st);
}

template <typename F>
int capture(shpair_ctx* c, hipStream_t st, hipGraphExec_t* out, F&& body)
{
  hipGraph_t g = nullptr;
  HIPCHK(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = body();
  const hipError_t e = hipStreamEndCapture(st, &g);
  if (rc) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  if (e != hipSuccess) CTX_FAIL(c, SHPAIR_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
  const hipError_t e2 = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e2 != hipSuccess) CTX_FAIL(c, SHPAIR_EHIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e2));
  return SHPAIR_OK;
}

int recapture(Run& r)
{
  r.g.reset();
  RC(capture(r.c, r.st, &r.g.a, [&] { return enqueue_a(r, true); }));
  if (r.a->check_every > 1) RC(capture(r.c, r.st, &r.g.a_nocheck, [&] { return enqueue_a(r, false); }));
  return capture(r.c, r.st, &r.g.b, [&] { return enqueue_b(r); });
}

int launch(Run& r, hipGraphExec_t g)
{
  const hipError_t e = hipGraphLaunch(g, r.st);
  if (e != hipSuccess) CTX_FAIL(r.c, SHPAIR_EHIP, "hipGraphLaunch failed: %s", hipGetErrorString(e));
  return SHPAIR_OK;
}

// an atom moved more than skin / 2: ghosts and list again, and the graphs with their new arguments
int rebuild(Run& r)
{
  const shstep_arrays* a = r.a;
  int np = 0;
  RC(shstep_borders_device(r.c, a->nlocal, a->nmax, a->x, a->quat, a->type, a->shtype, nullptr, &r.nghost, r.st));
  RC(shstep_neighbor_build_device(r.c, a->nlocal, r.nghost, a->x, a->shtype, nullptr, &np, r.st));
  ++r.nreb;
  return r.use_graph ? recapture(r) : SHPAIR_OK;
}

int one_step(Run& r, int step)
{
  const bool check = ((step + 1) % r.a->check_every) == 0;
  RC(r.use_graph ? launch(r, check ? r.g.a : r.g.a_nocheck) : enqueue_a(r, check));
  if (check) {
    const hipError_t e = hipStreamSynchronize(r.st);
    if (e != hipSuccess) CTX_FAIL(r.c, SHPAIR_EHIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    RC(step_decode_flags(r.c, r.s, r.st));
    if (r.s->h_flags[1]) RC(rebuild(r));
  }
  return r.use_graph ? launch(r, r.g.b) : enqueue_b(r);
}

}  // namespace

extern "C" int shstep_run_device(shpair_ctx* c, const shstep_arrays* a, int nsteps, int use_graph, int* nghost_io, int* rebuilds,
                                 void* stream)
{
  STEP_PROLOGUE(c);
  if (rebuilds) *rebuilds = 0;
  if (!a || !nghost_io || nsteps < 0) CTX_FAIL(c, SHPAIR_EINVAL, "null arguments or nsteps < 0");
  if (a->nlocal < 0 || a->nmax < a->nlocal || a->check_every < 1 || !std::isfinite(a->dt))
    CTX_FAIL(c, SHPAIR_EINVAL, "bad nlocal (%d) / nmax (%d) / check_every (%d) / dt", a->nlocal, a->nmax, a->check_every);
  if (nsteps == 0 || a->nlocal == 0) return SHPAIR_OK;
  if (!a->x || !a->v || !a->quat || !a->angmom || !a->f || !a->torque || !a->type || !a->shtype || !a->mask)
    CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  if (s->l_nlocal != a->nlocal || !c->have_neighbors || s->b_nlocal != a->nlocal || *nghost_io != s->nghost)
    CTX_FAIL(c, SHPAIR_ESTATE, "run: ghosts and neighbour list of the current particles must be built first "
             "(shstep_borders_device + shstep_neighbor_build_device)");
  hipStream_t st = (hipStream_t)stream;
  if (use_graph && !st) CTX_FAIL(c, SHPAIR_EINVAL, "run: graph replay needs an explicit stream (the null stream cannot be captured)");
  if (use_graph && (c->opt_timing || c->opt_count)) CTX_FAIL(c, SHPAIR_ESTATE, "run: switch the timing / count options off for graph replay");
  // nothing may be allocated or copied inside a capture: tables and buffers first
  RC(step_refresh_mass(c, s));
  RC(step_refresh_box(c, s));
  RC(shpair_prepare_tables(c));
  if (s->walls.nwalls > 0) RC(step_size_wall_buffers(c, s, a->nlocal, c->ledger_on || step_wall_rolling(c)));   // (the ledger keeps the rows, and so does SPEC §2.17)
  if (s->cyl.n > 0) RC(step_size_cyl_buffers(c, s, a->nlocal, step_cyl_rolling(c)));   // SPEC §2.18 (the power rows of §2.20 while both ledgers are on, the rows §2.21 keeps)
  if (s->cone.n > 0) RC(step_size_cone_buffers(c, s, a->nlocal, step_cone_rolling(c)));   // SPEC §2.22 (and the rows §2.24 keeps)
  // SPEC §2.15: xi_iw is keyed by the row index.  Neither this loop nor the rebuild it calls reorders, adds or removes
  // owned rows (shstep_borders_device wraps them in place and appends ghosts behind them), so the key holds for the run;
  // rows of another nlocal than the state's start from nothing live here, not inside a capture.
  RC(step_bind_wall_history(c, s, a->nlocal));
  RC(step_bind_cyl_history(c, s, a->nlocal));   // SPEC §2.19: the same for (xi_a, xi_theta) of the cylinders
  RC(step_bind_conic_history(c, s, a->nlocal));   // SPEC §2.23: ... and for (xi_g, xi_theta, phi_c) of the cones
  if (step_has_dissipation(c)) {
    HIPCHK(c, s->d_twist.ensure(6 * (size_t)a->nmax));
    HIPCHK(c, shp_size_dissipation_buffers(c, (size_t)c->npairs));
  }
  Run r{c, s, a, st, use_graph != 0, *nghost_io, 0};
  int rc = use_graph ? recapture(r) : SHPAIR_OK;
  for (int step = 0; step < nsteps && rc == SHPAIR_OK; ++step) rc = one_step(r, step);
  const hipError_t es = hipStreamSynchronize(st);
  *nghost_io = r.nghost;
  if (rebuilds) *rebuilds = r.nreb;
  if (rc) return rc;
  if (es != hipSuccess) CTX_FAIL(c, SHPAIR_EHIP, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
  if (s->walls.nwalls > 0 || s->cyl.n > 0 || s->cone.n > 0) return shpair_check_device_errors(c, st);   // a centre that went behind a wall, or out of a cylinder or a cone, during the run
  return SHPAIR_OK;
}
