// shstep_rolling.hip — rolling and twisting resistance of SH pairs (docs/SPEC.md §2.16) behind include/shstep.h, on top
// of rolling_kernels.hpp: the two setters and the pass.  The pass is one of its own, enqueued behind the pair pass of
// shstep_dissipation.hip (whichever of its forms the other coefficients ask for, or none), so those kernels are what they
// are without it.
// Nothing is allocated, zeroed or launched while every coefficient of both kinds is 0.
#include <hip/hip_runtime.h>

#include "../../include/shstep.h"
#include "rolling_kernels.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"

using namespace shp;

extern "C" {

int shstep_set_pair_rolling(shpair_ctx* c, int itype, int jtype, double mu_r, double gamma_r)
{
  STEP_PROLOGUE(c);
  const double vals[2] = {mu_r, gamma_r};
  const char* names[2] = {"mu_r", "gamma_r"};
  return set_pair_coefficients(c, "rolling", itype, jtype, 2, vals, names, c->roll_coef, c->d_roll_coef, c->roll_on);
}

int shstep_set_pair_twisting(shpair_ctx* c, int itype, int jtype, double mu_tw, double gamma_tw)
{
  STEP_PROLOGUE(c);
  const double vals[2] = {mu_tw, gamma_tw};
  const char* names[2] = {"mu_tw", "gamma_tw"};
  return set_pair_coefficients(c, "twisting", itype, jtype, 2, vals, names, c->twist_coef, c->d_twist_coef, c->twistres_on);
}

int shstep_pair_rolling_device(shpair_ctx* c, int nlocal, int nghost, const double* x, const int* type, const double* twist,
                               int newton_pair, double* torque, void* stream)
{
  STEP_PROLOGUE(c);
  if (nlocal < 0 || nghost < 0) CTX_FAIL(c, SHPAIR_EINVAL, "negative atom counts");
  if (!shp_has_rolling(c)) return SHPAIR_OK;   // no pair has rolling or twisting resistance: nothing is launched
  if (!c->have_neighbors) CTX_FAIL(c, SHPAIR_ESTATE, "no neighbour list");
  if (c->npairs == 0) return SHPAIR_OK;
  if (!c->integrals_src)
    CTX_FAIL(c, SHPAIR_EINVAL, "pair rolling: no compute has run on the installed list since the resistance was switched on");
  if (!x || !type || !twist || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  if ((long long)c->max_atom_index >= (long long)nlocal + nghost)
    CTX_FAIL(c, SHPAIR_EINVAL, "the neighbour list refers to atom %d but nlocal + nghost = %lld (stale list?)", c->max_atom_index,
             (long long)nlocal + nghost);
  if (c->tables_dirty) CTX_FAIL(c, SHPAIR_ESTATE, "pair rolling: the coefficients changed since the last compute");
  hipStream_t st = (hipStream_t)stream;
  const size_t n2 = ((size_t)c->ntypes + 1) * ((size_t)c->ntypes + 1);
  RollingParams P{};
  P.npairs = c->npairs; P.nlocal = nlocal; P.nall = nlocal + nghost; P.newton_pair = newton_pair ? 1 : 0; P.ntypes = c->ntypes;
  P.needv = c->integrals_needv ? 1 : 0;
  P.pair_i = c->d_pair_i.p; P.pair_j = c->d_pair_j.p; P.integrals = c->integrals_src; P.x = x; P.type = type; P.twist = twist;
  P.gamma = c->damp_on ? c->d_damp_gamma.p : nullptr;   // (the table may never have been allocated)
  P.kn = c->d_kn.p; P.expo = c->d_expo.p; P.torque = torque;
  if (c->roll_on) {   // a kind that is off is not read: its table may never have been allocated
    P.mu_r = c->d_roll_coef.p;
    P.gamma_r = c->d_roll_coef.p + n2;
  }
  if (c->twistres_on) {
    P.mu_tw = c->d_twist_coef.p;
    P.gamma_tw = c->d_twist_coef.p + n2;
  }
  const bool ledger = c->ledger_on;   // SPEC §2.13: the instance that also leaves its power in the friction entry
  if (ledger) {
    HIPCHK(c, shp_size_dissipation_buffers(c, (size_t)c->npairs));   // sized with the list; grows only if the ledger was switched on since
    P.power = c->d_slot_pow.p;
    // The PAIR pass has written the rows from the integrals of the last compute, and no fold has taken them: this
    // pass' share joins them.  Otherwise (no pair pass exists or ran on this compute; rows an earlier rolling pass
    // left do not count) it writes them, as the pair kernels do: the fold sees the last pass, once.  The flag is the
    // pair pass' alone and every compute clears it, so what a captured pass does never depends on an earlier step.
    P.add_power = (shp_has_pair_pass(c) && c->ledger_rows_pair && c->ledger_pair_fresh && c->ledger_pair_np == c->npairs) ? 1 : 0;
  }
  if (c->opt_deterministic) {
    if (c->rev_dirty) CTX_FAIL(c, SHPAIR_ESTATE, "pair rolling: the deterministic option was set after the last compute");
    HIPCHK(c, shp_size_dissipation_buffers(c, (size_t)c->npairs));   // sized with the list; grows only if an option changed since
    P.rows = c->d_slot_ft.p;   // the pair pass' row buffer: its gather is ahead of this pass on the stream
  }
  hipLaunchKernelGGL(ledger ? rolling_pair_ledger_kernel : rolling_pair_kernel, dim3(nblk(c->npairs, kRollBlock)), dim3(kRollBlock), 0,
                     st, P);
  HIPCHK(c, hipGetLastError());
  if (ledger) {
    c->ledger_pair_fresh = true;
    c->ledger_pair_np = c->npairs;
  }
  if (P.rows) {
    const int nall_idx = c->max_atom_index + 1;
    hipLaunchKernelGGL(rolling_gather_kernel, dim3(nblk(3LL * nall_idx, kRollBlock)), dim3(kRollBlock), 0, st, nall_idx,
                       (const int*)c->d_rev_start.p, (const int*)c->d_rev_ent.p, (const double*)P.rows, torque);
    HIPCHK(c, hipGetLastError());
  }
  return SHPAIR_OK;
}

}  // extern "C"
