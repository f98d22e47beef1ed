// shstep_cylinders.hip — the cylindrical container walls of include/shstep.h (docs/SPEC.md §2.18) on top of
// cylinder_kernels.hpp, of which this is the only includer: the cylinders and their coefficients (damping, friction,
// rotation about the axis), the cylinder pass, its statistics and the read-back for restarts.  The state is CylState
// (shstep_state.hpp); cyl_damp_on and cyl_fric_on choose the dissipative instance and tell the run loops that the pass
// reads twists (step_cyl_reads_twists).  The argument checks are cylinder_check.hpp's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/shstep.h"
#include "cylinder_check.hpp"
#include "cylinder_kernels.hpp"
#include "ring_tables.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"

using namespace shp;

static_assert(kMaxCylinders == SHSTEP_MAX_CYLINDERS && kCylinderLimit == SHSTEP_MAX_CYLINDERS, "one limit");

// buffers of a cylinder pass over nlocal particles; they only grow, so a caller that captures the pass sizes them first
int shp::step_size_cyl_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out)
{
  const size_t n = nlocal > 0 ? (size_t)nlocal : 1;
  HIPCHK(c, s->cyl.d_cmask.ensure(n));
  HIPCHK(c, s->cyl.d_cqueue.ensure(n));
  HIPCHK(c, s->cyl.d_ccnt.ensure(2));
  if (want_out) {
    HIPCHK(c, s->cyl.d_crows.ensure(kCylRow * n * (size_t)s->cyl.ncyl));
    HIPCHK(c, s->cyl.d_cpart.ensure(kCylRow * (size_t)nblk(nlocal, kCylBlock) * (size_t)s->cyl.ncyl));
  }
  return SHPAIR_OK;
}

// the kernel arguments of a cylinder pass: the caller's arrays, the cylinders, the pair context's shape and quadrature tables
static CylParams cyl_params(const shpair_ctx* c, const shstep_state* s, int nlocal, const double* x, const double* quat,
                            const int* shtype, const int* mask, int groupbit, double* f, double* torque, bool want_rows,
                            const double* twist)
{
  CylParams P{};
  P.nlocal = nlocal; P.ncyl = s->cyl.ncyl; P.cyls = s->cyl.d_cyl.p;
  P.x = x; P.quat = quat; P.shtype = shtype; P.mask = mask; P.groupbit = groupbit; P.f = f; P.torque = torque;
  P.rc = c->d_rc.p; P.cw = c->d_coef.p; P.rmax = c->d_rmax.p; P.cstride = c->cstride; P.lmax = c->lmax; P.nshapes = c->nshapes;
  const QuadLayout lay(c->lmax, c->nq);
  const double* q = c->d_quad.p;
  P.nq = c->nq; P.glt = q + lay.glt; P.glw = q + lay.glw; P.cpsi = q + lay.cpsi; P.spsi = q + lay.spsi;
  P.cmask = s->cyl.d_cmask.p; P.queue = s->cyl.d_cqueue.p; P.count = s->cyl.d_ccnt.p; P.err = c->d_err.p;
  P.rows = want_rows ? s->cyl.d_crows.p : nullptr;
  P.coef = s->cyl.d_ccoef.p; P.twist = twist;
  return P;
}

// The one place that turns the host copy of the coefficients ([kCylCoefRows][ncyl]: gamma_c, mu_c, gamma_t,c, Omega)
// into the device table and the two flags.  A cylinder is damped iff gamma_c != 0 and has friction iff mu_c and
// gamma_t,c are non-zero; Omega alone is no coefficient (it enters through the friction only).  The energy ledger has no
// cylinder entries: a coefficient while it is on is refused, and the state stays what it was.
static int install_cyl_coefficients(shpair_ctx* c, shstep_state* s, const char* what, const std::vector<double>& h)
{
  CylState& cs = s->cyl;
  const size_t nc = (size_t)cs.ncyl;
  bool damp = false, fric = false;
  for (size_t k = 0; k < nc; ++k) {
    damp = damp || h[k] != 0.0;
    fric = fric || (h[nc + k] != 0.0 && h[2 * nc + k] != 0.0);
  }
  if ((damp || fric) && c->ledger_on)
    CTX_FAIL(c, SHPAIR_ESTATE, "cylinder %s: the energy ledger is on and keeps no cylinder entries (docs/SPEC.md 2.18); switch it off "
             "(shstep_set_energy_ledger) or leave every cylinder coefficient 0", what);
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still read the old table
  HIPCHK(c, hipMemcpy(cs.d_ccoef.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));   // (shstep_set_cylinders sized it)
  cs.h_coef = h;
  cs.cyl_damp_on = damp;
  cs.cyl_fric_on = fric;
  return SHPAIR_OK;
}

extern "C" {

int shstep_set_cylinders(shpair_ctx* c, int ncyl, const double* cyl7, const double* kn, const double* exponent)
{
  STEP_PROLOGUE(c);
  const std::string bad = check_cylinders(ncyl, cyl7, kn, exponent);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  CylState& cs = s->cyl;
  std::vector<double> h((size_t)kCylStride * (size_t)ncyl);
  for (int k = 0; k < ncyl; ++k) {
    double* r = &h[(size_t)kCylStride * k];
    for (int j = 0; j < 7; ++j) r[j] = cyl7[7 * k + j];
    r[7] = kn[k]; r[8] = exponent[k];
  }
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still read the old tables
  if (ncyl > 0) {   // (no cylinder: nothing is allocated)
    HIPCHK(c, cs.d_cyl.ensure(h.size()));
    HIPCHK(c, hipMemcpy(cs.d_cyl.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, cs.d_ccoef.ensure((size_t)kCylCoefRows * ncyl));
    HIPCHK(c, hipMemset(cs.d_ccoef.p, 0, (size_t)kCylCoefRows * ncyl * sizeof(double)));
  }
  cs.h_cyl = h;
  cs.h_coef.assign((size_t)kCylCoefRows * ncyl, 0.0);   // every gamma_c, mu_c, gamma_t,c and Omega is 0 again
  cs.cyl_damp_on = false;
  cs.cyl_fric_on = false;
  cs.ncyl = ncyl;
  cs.cyl_called = false;
  return SHPAIR_OK;
}

int shstep_set_cylinder_damping(shpair_ctx* c, int ncyl, const double* gamma)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"damping coefficient"};
  const std::string bad = check_cylinder_coefficients("damping", ncyl, s->cyl.ncyl, 1, &gamma, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  std::vector<double> h = s->cyl.h_coef;
  for (int k = 0; k < ncyl; ++k) h[k] = gamma[k];
  return install_cyl_coefficients(c, s, "damping", h);
}

int shstep_set_cylinder_friction(shpair_ctx* c, int ncyl, const double* mu, const double* gamma_t)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu, gamma_t};
  const char* names[2] = {"friction coefficient mu", "friction coefficient gamma_t"};
  const std::string bad = check_cylinder_coefficients("friction", ncyl, s->cyl.ncyl, 2, tabs, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  std::vector<double> h = s->cyl.h_coef;
  for (int k = 0; k < ncyl; ++k) {
    h[(size_t)ncyl + k] = mu[k];
    h[2 * (size_t)ncyl + k] = gamma_t[k];
  }
  return install_cyl_coefficients(c, s, "friction", h);
}

int shstep_set_cylinder_rotation(shpair_ctx* c, int ncyl, const double* omega)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"angular velocity"};
  const std::string bad = check_cylinder_coefficients("rotation", ncyl, s->cyl.ncyl, 1, &omega, names, true);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  std::vector<double> h = s->cyl.h_coef;
  for (int k = 0; k < ncyl; ++k) h[3 * (size_t)ncyl + k] = omega[k];
  return install_cyl_coefficients(c, s, "rotation", h);
}

// The geometry never moves: the host copy is what the device holds.
int shstep_get_cylinders(shpair_ctx* c, int ncyl, double* cyl7_out)
{
  STEP_PROLOGUE(c);
  if (ncyl != s->cyl.ncyl) CTX_FAIL(c, SHPAIR_EINVAL, "get cylinders: room for %d cylinders, %d are set", ncyl, s->cyl.ncyl);
  if (ncyl == 0) return SHPAIR_OK;
  if (!cyl7_out) CTX_FAIL(c, SHPAIR_EINVAL, "get cylinders: null output pointer");
  for (int k = 0; k < ncyl; ++k)
    for (int j = 0; j < 7; ++j) cyl7_out[7 * k + j] = s->cyl.h_cyl[(size_t)kCylStride * k + j];
  return SHPAIR_OK;
}

int shstep_cylinder_force_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                                 int groupbit, double* f, double* torque, double* cyl_out, const double* twist, void* stream)
{
  STEP_PROLOGUE(c);
  if (nlocal < 0) CTX_FAIL(c, SHPAIR_EINVAL, "nlocal %d < 0", nlocal);
  CylState& cs = s->cyl;
  if (cs.ncyl == 0 || nlocal == 0) return SHPAIR_OK;   // no cylinder: nothing is allocated, zeroed or launched
  if (!x || !quat || !shtype || !mask || !f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  const bool diss = cs.cyl_damp_on || cs.cyl_fric_on;   // every coefficient 0: the elastic instance, whatever twist is
  if (diss && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "cylinder %s: null twist pointer", cs.cyl_damp_on ? "damping" : "friction");
  if (c->tables_dirty || c->quad_dirty) RC(shpair_prepare_tables(c));
  const bool want_rows = cyl_out != nullptr;
  RC(step_size_cyl_buffers(c, s, nlocal, want_rows));
  hipStream_t st = (hipStream_t)stream;
  const CylParams P = cyl_params(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, want_rows, twist);
  HIPCHK(c, hipMemsetAsync(cs.d_ccnt.p, 0, 2 * sizeof(int), st));
  const unsigned nb = nblk(nlocal, kCylBlock);
  hipLaunchKernelGGL(cyl_candidates_kernel, dim3(nb), dim3(kCylBlock), 0, st, P);
  // one wave per queued particle: a grid that covers nlocal, capped; the waves stride over the device-side count
  const unsigned ncb = nblk(nlocal, kCylBlock / 64);
  const dim3 grid(ncb < (unsigned)kCylMaxBlocks ? ncb : (unsigned)kCylMaxBlocks);
  hipLaunchKernelGGL(diss ? cyl_contact_dissipative_kernel : cyl_contact_kernel, grid, dim3(kCylBlock), 0, st, P);
  if (cyl_out) {
    hipLaunchKernelGGL(cyl_rows_partial_kernel, dim3(nb, cs.ncyl), dim3(kCylBlock), 0, st, nlocal, cs.ncyl,
                       (const unsigned char*)cs.d_cmask.p, (const double*)cs.d_crows.p, cs.d_cpart.p);
    hipLaunchKernelGGL(cyl_rows_final_kernel, dim3(cs.ncyl), dim3(kCylBlock), 0, st, (int)nb, (const double*)cs.d_cpart.p, cyl_out);
  }
  HIPCHK(c, hipGetLastError());
  cs.cyl_called = true;
  return SHPAIR_OK;
}

int shstep_get_cylinder_stats(shpair_ctx* c, int* ncontacts)
{
  STEP_PROLOGUE(c);
  if (!ncontacts) CTX_FAIL(c, SHPAIR_EINVAL, "null output pointer");
  *ncontacts = 0;
  if (!s->cyl.cyl_called) return SHPAIR_OK;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(ncontacts, s->cyl.d_ccnt.p + 1, sizeof(int), hipMemcpyDeviceToHost));
  return shpair_check_device_errors(c, c->stream);
}

}  // extern "C"
