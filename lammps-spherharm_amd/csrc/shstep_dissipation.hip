// shstep_dissipation.hip — the contact-dissipation entry points of include/shstep.h for pairs (docs/SPEC.md §2.10
// volume-rate damping, §2.11 Coulomb-capped friction) on top of dissipation_kernels.hpp: the two pair setters, the twists
// and the pair pass.  The wall coefficients and the wall pass that reads them are in shstep_walls.hip.
// Nothing is allocated, zeroed or launched while every coefficient is 0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/shstep.h"
#include "dissipation_kernels.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"

using namespace shp;

// The pair setters' common part.  `host` holds ntab tables of (ntypes+1)^2 like kn, one per coefficient of the kind
// `what`; vals[k] (named names[k] in messages) goes into table k, symmetrically.  A type pair counts iff all of its
// coefficients are non-zero, and `on` says whether one does.  Tables that were never needed stay unallocated.
static int set_pair_coefficients(shpair_ctx* c, const char* what, int itype, int jtype, int ntab, const double* vals,
                                 const char* const* names, std::vector<double>& host, DevBuf<double>& dev, bool& on)
{
  if (c->ntypes <= 0) CTX_FAIL(c, SHPAIR_ESTATE, "shpair_set_ntypes() must come first");
  if (itype < 1 || itype > c->ntypes || jtype < 1 || jtype > c->ntypes)
    CTX_FAIL(c, SHPAIR_EINVAL, "pair %s: types %d %d outside [1,%d]", what, itype, jtype, c->ntypes);
  bool zero = true;
  for (int k = 0; k < ntab; ++k) {
    if (!(vals[k] >= 0.0) || !std::isfinite(vals[k]))
      CTX_FAIL(c, SHPAIR_EINVAL, "pair %s: %s %g must be finite and >= 0", what, names[k], vals[k]);
    zero = zero && vals[k] == 0.0;
  }
  const size_t nt = (size_t)c->ntypes + 1, n2 = nt * nt;
  if (host.size() != ntab * n2) {
    if (zero) return SHPAIR_OK;   // all zero already: nothing is allocated
    host.assign(ntab * n2, 0.0);
  }
  for (int k = 0; k < ntab; ++k) host[k * n2 + itype * nt + jtype] = host[k * n2 + jtype * nt + itype] = vals[k];
  bool any = false;
  for (size_t e = 0; e < n2 && !any; ++e) {
    any = true;
    for (int k = 0; k < ntab; ++k) any = any && host[k * n2 + e] != 0.0;
  }
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still read the old table
  HIPCHK(c, dev.ensure(host.size()));
  HIPCHK(c, hipMemcpy(dev.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
  if (any && !shp_keeps_integrals(c)) c->integrals_src = nullptr;   // switched on: no compute has left its integrals yet
  on = any;
  if (any && c->have_neighbors) HIPCHK(c, shp_size_dissipation_buffers(c, (size_t)c->npairs));
  return SHPAIR_OK;
}

extern "C" {

int shstep_set_pair_damping(shpair_ctx* c, int itype, int jtype, double gamma)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"gamma"};
  return set_pair_coefficients(c, "damping", itype, jtype, 1, &gamma, names, c->damp_gamma, c->d_damp_gamma, c->damp_on);
}

int shstep_set_pair_friction(shpair_ctx* c, int itype, int jtype, double mu, double gamma_t)
{
  STEP_PROLOGUE(c);
  const double vals[2] = {mu, gamma_t};
  const char* names[2] = {"mu", "gamma_t"};
  return set_pair_coefficients(c, "friction", itype, jtype, 2, vals, names, c->fric_coef, c->d_fric_coef, c->fric_on);
}

int shstep_twist_device(shpair_ctx* c, int nlocal, int nghost, const double* v, const double* quat, const double* angmom,
                        const int* shtype, double* twist, void* stream)
{
  STEP_PROLOGUE(c);
  if (nlocal < 0 || nghost < 0) CTX_FAIL(c, SHPAIR_EINVAL, "bad nlocal (%d) / nghost (%d)", nlocal, nghost);
  if (nghost > 0 && (nghost != s->nghost || nlocal != s->b_nlocal))
    CTX_FAIL(c, SHPAIR_ESTATE, "twist: the ghost rows must be those of the last shstep_borders_device() (%d owned, %d ghosts); "
             "pass nghost = 0 and fill other ghosts' rows yourself", s->b_nlocal, s->nghost);
  if (nlocal == 0) return SHPAIR_OK;
  if (!v || !quat || !angmom || !shtype || !twist) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  RC(step_refresh_mass(c, s));
  hipLaunchKernelGGL(twist_kernel, dim3(nblk((long long)nlocal + nghost, kDampBlock)), dim3(kDampBlock), 0, (hipStream_t)stream, nlocal,
                     nghost, (const double*)s->d_mass.p, c->nshapes, v, quat, angmom, shtype, (const int*)s->d_gowner.p, twist,
                     s->d_flags.p);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shstep_pair_damping_device(shpair_ctx* c, int nlocal, int nghost, const double* x, const int* type, const double* twist,
                               int newton_pair, double* f, double* torque, void* stream)
{
  if (!c) return SHPAIR_EINVAL;
  if (c->fric_on) CTX_FAIL(c, SHPAIR_EINVAL, "pair friction needs the form with shape indices (shstep_pair_dissipation_device)");
  return shstep_pair_dissipation_device(c, nlocal, nghost, x, type, nullptr, twist, newton_pair, f, torque, stream);
}

int shstep_pair_dissipation_device(shpair_ctx* c, int nlocal, int nghost, const double* x, const int* type, const int* shtype,
                                   const double* twist, int newton_pair, double* f, double* torque, void* stream)
{
  STEP_PROLOGUE(c);
  if (nlocal < 0 || nghost < 0) CTX_FAIL(c, SHPAIR_EINVAL, "negative atom counts");
  if (!shp_keeps_integrals(c)) return SHPAIR_OK;   // every gamma_ij and every friction pair is 0: nothing is launched
  if (!c->have_neighbors) CTX_FAIL(c, SHPAIR_ESTATE, "no neighbour list");
  if (c->npairs == 0) return SHPAIR_OK;
  if (!c->integrals_src)
    CTX_FAIL(c, SHPAIR_EINVAL, "pair damping: no compute has run on the installed list since damping was switched on");
  if (!x || !type || !twist || !f || !torque || (c->fric_on && !shtype)) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  if ((long long)c->max_atom_index >= (long long)nlocal + nghost)
    CTX_FAIL(c, SHPAIR_EINVAL, "the neighbour list refers to atom %d but nlocal + nghost = %lld (stale list?)", c->max_atom_index,
             (long long)nlocal + nghost);
  if (c->tables_dirty) CTX_FAIL(c, SHPAIR_ESTATE, "pair damping: the coefficients changed since the last compute");
  hipStream_t st = (hipStream_t)stream;
  DampParams P{};
  P.npairs = c->npairs; P.nlocal = nlocal; P.nall = nlocal + nghost; P.newton_pair = newton_pair ? 1 : 0; P.ntypes = c->ntypes;
  P.needv = c->integrals_needv ? 1 : 0;
  P.pair_i = c->d_pair_i.p; P.pair_j = c->d_pair_j.p; P.integrals = c->integrals_src; P.x = x; P.type = type; P.twist = twist;
  P.gamma = c->d_damp_gamma.p; P.kn = c->d_kn.p; P.expo = c->d_expo.p; P.f = f; P.torque = torque;
  const bool ledger = c->ledger_on;   // SPEC §2.13: the instances that also leave the power rows
  if (ledger) {
    HIPCHK(c, shp_size_dissipation_buffers(c, (size_t)c->npairs));   // sized with the list; grows only if the ledger was switched on since
    P.power = c->d_slot_pow.p;
  }
  if (c->opt_deterministic) {
    if (c->rev_dirty) CTX_FAIL(c, SHPAIR_ESTATE, "pair damping: the deterministic option was set after the last compute");
    HIPCHK(c, shp_size_dissipation_buffers(c, (size_t)c->npairs));   // sized with the list; grows only if an option changed since
    P.pair_ft = c->d_slot_ft.p;
  }
  if (c->fric_on) {   // damping and friction in one pass (SPEC §2.11)
    const size_t n2 = ((size_t)c->ntypes + 1) * ((size_t)c->ntypes + 1);
    FrictionParams Q{};
    Q.d = P;
    if (!c->damp_on) Q.d.gamma = nullptr;   // (the table may never have been allocated)
    Q.nshapes = c->nshapes; Q.shtype = shtype; Q.rmax = c->d_rmax.p;
    Q.mu = c->d_fric_coef.p; Q.gamma_t = c->d_fric_coef.p + n2;
    hipLaunchKernelGGL(ledger ? pair_dissipation_ledger_kernel : pair_dissipation_kernel, dim3(nblk(c->npairs, kDampBlock)),
                       dim3(kDampBlock), 0, st, Q);
  } else {
    hipLaunchKernelGGL(ledger ? pair_damp_ledger_kernel : pair_damp_kernel, dim3(nblk(c->npairs, kDampBlock)), dim3(kDampBlock), 0,
                       st, P);
  }
  HIPCHK(c, hipGetLastError());
  if (ledger) {
    c->ledger_pair_fresh = true;
    c->ledger_pair_np = c->npairs;
  }
  if (P.pair_ft) RC(shp_det_gather(c, P.pair_ft, f, torque, st));
  return SHPAIR_OK;
}

}  // extern "C"
