// shstep_dissipation.hip — the contact-dissipation entry points of include/shstep.h for pairs (docs/SPEC.md §2.10
// volume-rate damping, §2.11 Coulomb-capped friction, §2.14 tangential springs with history) on top of
// dissipation_kernels.hpp and history_kernels.hpp: the three pair setters, the twists, the pair pass in its two forms,
// and what a device build does for the contact history.  The wall coefficients and the wall pass that reads them are in
// shstep_walls.hip.
// Nothing is allocated, zeroed or launched while every coefficient is 0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/shstep.h"
#include "dissipation_kernels.hpp"
#include "history_kernels.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"

using namespace shp;

// The pair setters' common part.  `host` holds ntab tables of (ntypes+1)^2 like kn, one per coefficient of the kind
// `what`; vals[k] (named names[k] in messages) goes into table k, symmetrically.  A type pair counts iff all of its
// coefficients are non-zero, and `on` says whether one does.  Tables that were never needed stay unallocated.
// (Shared with the setters of shstep_rolling.hip through shstep_state.hpp.)
int shp::set_pair_coefficients(shpair_ctx* c, const char* what, int itype, int jtype, int ntab, const double* vals,
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

// The pair pass in its two forms: shstep_pair_dissipation_device (history = false, dt unused) and, while a tangential
// spring is set, shstep_pair_contact_device (SPEC §2.14).
static int pair_pass(shpair_ctx* c, shstep_state* s, int nlocal, int nghost, const double* x, const int* type, const int* shtype,
                     const double* twist, int newton_pair, double* f, double* torque, void* stream, const bool history, const double dt)
{
  if (nlocal < 0 || nghost < 0) CTX_FAIL(c, SHPAIR_EINVAL, "negative atom counts");
  // every gamma_ij, friction pair and spring is 0: nothing is launched.  (Not shp_keeps_integrals: with a rolling or
  // twisting coefficient alone, SPEC §2.16, the integrals are kept but none of this pass' tables need exist.)
  if (!shp_has_pair_pass(c)) return SHPAIR_OK;
  if (!c->have_neighbors) CTX_FAIL(c, SHPAIR_ESTATE, "no neighbour list");
  if (history) {
    if (s->l_nlocal < 0)
      CTX_FAIL(c, SHPAIR_ESTATE, "pair contact: tangential history needs a list built by shstep_neighbor_build_device");
    if (s->partitioned)
      CTX_FAIL(c, SHPAIR_ESTATE, "pair contact: tangential history does not follow a list partitioned by option halo_overlap");
  }
  if (c->npairs == 0) return SHPAIR_OK;
  if (history) {
    if (!c->integrals_src) CTX_FAIL(c, SHPAIR_ESTATE, "pair contact: no compute has run on the installed list");
    if (c->hist_np != c->npairs)
      CTX_FAIL(c, SHPAIR_ESTATE, "pair contact: the installed list was built before a tangential spring was set; build it again");
  }
  if (!c->integrals_src)
    CTX_FAIL(c, SHPAIR_EINVAL, "pair damping: no compute has run on the installed list since damping was switched on");
  if (!x || !type || !twist || !f || !torque || ((c->fric_on || history) && !shtype)) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
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
  if (c->fric_on || history) {   // damping and friction in one pass (SPEC §2.11)
    const size_t n2 = ((size_t)c->ntypes + 1) * ((size_t)c->ntypes + 1);
    FrictionParams Q{};
    Q.d = P;
    if (!c->damp_on) Q.d.gamma = nullptr;   // (the table may never have been allocated)
    Q.nshapes = c->nshapes; Q.shtype = shtype; Q.rmax = c->d_rmax.p;
    Q.mu = c->d_fric_coef.p; Q.gamma_t = c->d_fric_coef.p ? c->d_fric_coef.p + n2 : nullptr;
    if (history) {   // ... and the tangential springs (SPEC §2.14); xi and the keys were sized and filled by the build
      HistoryParams H{};
      H.q = Q; H.kt = c->d_spring_kt.p; H.xi = c->d_xi.p; H.stride = (size_t)c->npairs; H.dt = dt;
      hipLaunchKernelGGL(ledger ? pair_history_ledger_kernel : pair_history_kernel, dim3(nblk(c->npairs, kDampBlock)),
                         dim3(kDampBlock), 0, st, H);
    } else {
      hipLaunchKernelGGL(ledger ? pair_dissipation_ledger_kernel : pair_dissipation_kernel, dim3(nblk(c->npairs, kDampBlock)),
                         dim3(kDampBlock), 0, st, Q);
    }
  } else {
    hipLaunchKernelGGL(ledger ? pair_damp_ledger_kernel : pair_damp_kernel, dim3(nblk(c->npairs, kDampBlock)), dim3(kDampBlock), 0,
                       st, P);
  }
  HIPCHK(c, hipGetLastError());
  if (ledger) {
    c->ledger_pair_fresh = true;
    c->ledger_pair_np = c->npairs;
    c->ledger_rows_pair = true;   // a rolling pass behind this one (SPEC §2.16) adds its share to these rows
  }
  if (P.pair_ft) RC(shp_det_gather(c, P.pair_ft, f, torque, st));
  return SHPAIR_OK;
}

// ---- the contact history around a device build (shstep_state.hpp) ------------------------------------------------------

int shp::step_history_put_aside(shpair_ctx* c, shstep_state* s, int nlocal)
{
  const bool live = c->have_neighbors && s->l_nlocal == nlocal && !s->partitioned && c->hist_np >= 0 && c->hist_np == c->npairs;
  const int old_np = live ? c->hist_np : -1;
  c->hist_np = -1;
  if (!live) return -1;
  std::swap(c->d_xi, c->d_xi_old);
  std::swap(c->d_hkey, c->d_hkey_old);
  std::swap(s->d_offs, c->d_hoffs_old);
  return old_np;
}

int shp::step_history_carry(shpair_ctx* c, shstep_state* s, int nlocal, int np, const int* tag, int old_np, hipStream_t st)
{
  if (np == 0) {
    c->hist_np = 0;
    return SHPAIR_OK;
  }
  // (sized by shp_size_pair_buffers for this list; here in case the spring was set between two builds of one size)
  HIPCHK(c, c->d_xi.ensure(3 * (size_t)np));
  HIPCHK(c, c->d_hkey.ensure((size_t)np));
  const dim3 grid(nblk(np, kDampBlock)), block(kDampBlock);
  hipLaunchKernelGGL(history_key_kernel, grid, block, 0, st, np, nlocal, (const int*)c->d_pair_j.p, tag, (const int*)s->d_gowner.p,
                     c->d_hkey.p);
  if (old_np > 0)
    hipLaunchKernelGGL(history_carry_kernel, grid, block, 0, st, np, (const int*)c->d_pair_i.p, (const int*)c->d_hkey.p,
                       (const int*)c->d_hoffs_old.p, (const int*)c->d_hkey_old.p, (const double*)c->d_xi_old.p, (size_t)old_np,
                       c->d_xi.p, (size_t)np);
  else
    HIPCHK(c, hipMemsetAsync(c->d_xi.p, 0, 3 * (size_t)np * sizeof(double), st));
  HIPCHK(c, hipGetLastError());
  c->hist_np = np;
  return SHPAIR_OK;
}

// xi of the installed list for the three blocking calls below: refuses unless a spring is set and a device build has
// filled it
static int history_ready(shpair_ctx* c, shstep_state* s, const char* what)
{
  if (s->l_nlocal < 0 || !c->have_neighbors || s->partitioned)
    CTX_FAIL(c, SHPAIR_ESTATE, "%s: no unpartitioned list built by shstep_neighbor_build_device", what);
  if (!c->hist_on) CTX_FAIL(c, SHPAIR_ESTATE, "%s: no tangential spring is set (shstep_set_pair_tangential_spring)", what);
  if (c->hist_np != c->npairs)
    CTX_FAIL(c, SHPAIR_ESTATE, "%s: the installed list was built before a tangential spring was set; build it again", what);
  HIPCHK(c, hipDeviceSynchronize());   // a pass may still be writing xi
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
  if (c->hist_on)
    CTX_FAIL(c, SHPAIR_EINVAL, "a tangential spring is set: the pair pass needs the form with a time step (shstep_pair_contact_device)");
  return pair_pass(c, s, nlocal, nghost, x, type, shtype, twist, newton_pair, f, torque, stream, false, 0.0);
}

int shstep_set_pair_tangential_spring(shpair_ctx* c, int itype, int jtype, double kt)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"kt"};
  const bool was_on = c->hist_on;
  const int rc = set_pair_coefficients(c, "tangential spring", itype, jtype, 1, &kt, names, c->spring_kt, c->d_spring_kt, c->hist_on);
  // switched on or off: what xi and the keys hold is no list's history any more.  A list installed now was (or, after
  // builds without a spring, may have been) built without keys, and the next build starts from zero.
  if (c->hist_on != was_on) c->hist_np = -1;
  return rc;
}

int shstep_pair_contact_device(shpair_ctx* c, int nlocal, int nghost, const double* x, const int* type, const int* shtype,
                               const double* twist, int newton_pair, double dt, double* f, double* torque, void* stream)
{
  STEP_PROLOGUE(c);
  if (!(dt >= 0.0) || !std::isfinite(dt)) CTX_FAIL(c, SHPAIR_EINVAL, "pair contact: dt %g must be finite and >= 0", dt);
  return pair_pass(c, s, nlocal, nghost, x, type, shtype, twist, newton_pair, f, torque, stream, c->hist_on, dt);
}

int shstep_copy_contact_history(shpair_ctx* c, double* xi3)
{
  STEP_PROLOGUE(c);
  RC(history_ready(c, s, "copy contact history"));
  const size_t np = (size_t)c->npairs;
  if (np == 0) return SHPAIR_OK;
  if (!xi3) CTX_FAIL(c, SHPAIR_EINVAL, "copy contact history: null output pointer");
  std::vector<double> h(3 * np);
  HIPCHK(c, hipMemcpy(h.data(), c->d_xi.p, 3 * np * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t w = 0; w < np; ++w)
    for (int k = 0; k < 3; ++k) xi3[3 * w + k] = h[k * np + w];   // planes -> one triple per slot
  return SHPAIR_OK;
}

int shstep_set_contact_history(shpair_ctx* c, const double* xi3)
{
  STEP_PROLOGUE(c);
  RC(history_ready(c, s, "set contact history"));
  const size_t np = (size_t)c->npairs;
  if (np == 0) return SHPAIR_OK;
  if (!xi3) CTX_FAIL(c, SHPAIR_EINVAL, "set contact history: null input pointer");
  std::vector<double> h(3 * np);
  for (size_t w = 0; w < np; ++w)
    for (int k = 0; k < 3; ++k) h[k * np + w] = xi3[3 * w + k];
  HIPCHK(c, hipMemcpy(c->d_xi.p, h.data(), 3 * np * sizeof(double), hipMemcpyHostToDevice));
  return SHPAIR_OK;
}

int shstep_reset_contact_history(shpair_ctx* c)
{
  STEP_PROLOGUE(c);
  if (c->hist_np <= 0) return SHPAIR_OK;   // no list holds a history: nothing to zero
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemset(c->d_xi.p, 0, 3 * (size_t)c->hist_np * sizeof(double)));
  return SHPAIR_OK;
}

}  // extern "C"
