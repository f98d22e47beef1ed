// shstep_ledger.hip — the energy ledger of include/shstep.h (docs/SPEC.md §2.13) on top of ledger_kernels.hpp, of which
// this is the only includer: the switch, the fold, the read-back and the reset.  The accumulator is the step state's
// d_ledger; the rows the fold reads are the pair pass' (shpair_ctx::d_slot_pow, shstep_dissipation.hip) and the wall
// pass' (WallState::work.rows / d_wprows, shstep_walls.hip), which also say whether they are fresh.
// The cylinder entries (SPEC §2.20) have an accumulator, a switch and fold kernels of their own in shstep_cylinders.hip;
// the fold here hands them their turn and the reset zeroes them.
// Nothing is allocated, zeroed or launched while the ledger is off.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/shstep.h"
#include "ledger_kernels.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"

using namespace shp;

static_assert(SHSTEP_MAX_WALLS == 32 && kLedgerDoubles == 5 + 3 * SHSTEP_MAX_WALLS, "the accumulator holds 5 totals and 3 per wall");

extern "C" {

int shstep_set_energy_ledger(shpair_ctx* c, int on)
{
  STEP_PROLOGUE(c);
  if ((on != 0) == c->ledger_on) return SHPAIR_OK;
  // SPEC §2.18: the ledger keeps no cylinder entries; what a cylinder dissipates would go missing from the balance,
  // unless the shell ledger is on and keeps them (SPEC §2.20)
  const bool shell = step_shell_ledger(c);
  const shp::SurfaceSwitches& cyl = s->cyl.on;
  if (on && !shell && cyl.roll && !cyl.damp && !cyl.fric && !cyl.hist)   // SPEC §2.21: the same for what the two couples dissipate
    CTX_FAIL(c, SHPAIR_ESTATE, "energy ledger: cylinder rolling or twisting resistance is set and the ledger keeps no cylinder "
             "entries (docs/SPEC.md 2.21); set every cylinder rolling and twisting coefficient to 0 first");
  if (on && !shell && step_cyl_reads_twists(c) && !step_cyl_history(c))
    CTX_FAIL(c, SHPAIR_ESTATE, "energy ledger: a cylinder damping or friction coefficient is set and the ledger keeps no cylinder "
             "entries (docs/SPEC.md 2.18); set every cylinder coefficient to 0 first");
  if (on && !shell && step_cyl_history(c))   // SPEC §2.19: the same for what a sliding spring dissipates
    CTX_FAIL(c, SHPAIR_ESTATE, "energy ledger: a cylinder tangential spring is set and the ledger keeps no cylinder entries "
             "(docs/SPEC.md 2.19); set every cylinder k_t to 0 first");
  if (on && step_cone_history(c))   // SPEC §2.23: the same for what a sliding cone spring dissipates
    CTX_FAIL(c, SHPAIR_ESTATE, "energy ledger: a cone tangential spring is set and the ledger keeps no cone entries "
             "(docs/SPEC.md 2.23); set every cone k_t to 0 first");
  if (on && step_cone_dissipates(c))   // SPEC §2.22: the ledger keeps no cone entries either, and cones have no ledger of their own
    CTX_FAIL(c, SHPAIR_ESTATE, "energy ledger: a cone damping or friction coefficient or a cone rotation is set and the ledger keeps "
             "no cone entries (docs/SPEC.md 2.22); set every cone coefficient and Omega to 0 first");
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass or fold may still use the buffers
  c->ledger_pair_fresh = false;        // rows of the other setting are not folded
  c->ledger_rows_pair = false;
  s->walls.ledger_fresh = false;
  s->cyl.shell_fresh = false;
  if (!on) {
    c->ledger_on = false;   // frees nothing: the accumulator can still be read
    return SHPAIR_OK;
  }
  HIPCHK(c, s->d_ledger.ensure(kLedgerDoubles));
  HIPCHK(c, hipMemset(s->d_ledger.p, 0, kLedgerDoubles * sizeof(double)));
  c->ledger_on = true;
  // the pair pass' power rows are sized with the list (here for the installed one); the wall pass' with its buffers
  if (c->have_neighbors) HIPCHK(c, shp_size_dissipation_buffers(c, (size_t)c->npairs));
  return SHPAIR_OK;
}

int shstep_ledger_fold_device(shpair_ctx* c, double dt, void* stream)
{
  STEP_PROLOGUE(c);
  if (!std::isfinite(dt)) CTX_FAIL(c, SHPAIR_EINVAL, "ledger fold: dt is not finite");
  if (!c->ledger_on) CTX_FAIL(c, SHPAIR_ESTATE, "ledger fold: the energy ledger is off (shstep_set_energy_ledger)");
  const bool pair = c->ledger_pair_fresh, wall = s->walls.ledger_fresh && s->walls.nwalls > 0;
  const bool shell = s->cyl.shell_fresh && s->cyl.n > 0;   // SPEC §2.20: the cylinder pass' power rows
  if (!pair && !wall && !shell) return SHPAIR_OK;   // every pass is folded once
  hipStream_t st = (hipStream_t)stream;
  if (shell) RC(step_fold_shell_rows(c, s, dt, st));   // into an accumulator of its own: the launches below stay what they were
  if (!pair && !wall) return SHPAIR_OK;
  int nbp = 0, nbw = 0, nw = 0;
  const double* ppart = nullptr;
  if (pair) {
    const int np = c->ledger_pair_np;
    nbp = (int)nblk(np, kLedgerChunk);
    double* part = c->d_slot_pow.p + 2 * (size_t)np;
    hipLaunchKernelGGL(ledger_pair_partial_kernel, dim3(nbp), dim3(kLedgerBlock), 0, st, np, (const double*)c->d_slot_pow.p, part);
    ppart = part;
  }
  if (wall) {
    const int nlocal = s->walls.ledger_nlocal;
    nw = s->walls.nwalls;
    nbw = (int)nblk(nlocal, kLedgerBlock);
    hipLaunchKernelGGL(ledger_wall_partial_kernel, dim3(nbw, nw), dim3(kLedgerBlock), 0, st, nlocal, nw,
                       (const unsigned*)s->walls.work.mask.p, (const double*)s->walls.work.rows.p,
                       s->walls.ledger_power ? (const double*)s->walls.d_wprows.p : (const double*)nullptr, s->walls.d_wlpart.p);
  }
  // (the velocity table is allocated by the first shstep_set_wall_velocity that sets one: no wall has moved without it)
  hipLaunchKernelGGL(ledger_final_kernel, dim3(1), dim3(kLedgerBlock), 0, st, nbp, ppart, nw, nbw, (const double*)s->walls.d_wlpart.p,
                     s->walls.wall_move_on ? (const double*)s->walls.d_wvel.p : (const double*)nullptr, dt, s->d_ledger.p);
  HIPCHK(c, hipGetLastError());
  c->ledger_pair_fresh = false;
  c->ledger_rows_pair = false;   // folded rows take no further share (SPEC §2.16)
  s->walls.ledger_fresh = false;
  return SHPAIR_OK;
}

int shstep_get_energy_ledger(shpair_ctx* c, double* totals5, int nwalls, double* per_wall3)
{
  STEP_PROLOGUE(c);
  if (!totals5) CTX_FAIL(c, SHPAIR_EINVAL, "get energy ledger: null output pointer");
  if (per_wall3 && nwalls != s->walls.nwalls)
    CTX_FAIL(c, SHPAIR_EINVAL, "get energy ledger: room for %d walls, %d are set", nwalls, s->walls.nwalls);
  if (!s->d_ledger.p) CTX_FAIL(c, SHPAIR_ESTATE, "get energy ledger: the energy ledger was never switched on");
  double h[kLedgerDoubles];
  HIPCHK(c, hipDeviceSynchronize());   // a fold may still be in flight
  HIPCHK(c, hipMemcpy(h, s->d_ledger.p, sizeof(h), hipMemcpyDeviceToHost));
  for (int k = 0; k < kLedgerTotals; ++k) totals5[k] = h[k];
  if (per_wall3)
    for (int k = 0; k < kLedgerPerWall * nwalls; ++k) per_wall3[k] = h[kLedgerTotals + k];
  return SHPAIR_OK;
}

int shstep_reset_energy_ledger(shpair_ctx* c)
{
  STEP_PROLOGUE(c);
  if (!s->d_ledger.p) CTX_FAIL(c, SHPAIR_ESTATE, "reset energy ledger: the energy ledger was never switched on");
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemset(s->d_ledger.p, 0, kLedgerDoubles * sizeof(double)));
  if (s->cyl.d_shell.p)   // SPEC §2.20: the shell entries are part of the same balance
    HIPCHK(c, hipMemset(s->cyl.d_shell.p, 0, kShellDoubles * sizeof(double)));
  return SHPAIR_OK;
}

}  // extern "C"
