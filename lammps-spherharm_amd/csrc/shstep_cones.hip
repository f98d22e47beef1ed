// shstep_cones.hip — the conical container walls of include/shstep.h (docs/SPEC.md §2.22) on top of cone_kernels.hpp, of
// which this is the only includer: the cones and their coefficients (damping, friction, rotation about the axis), the
// cone pass, its statistics and the read-back for restarts.  The state is ConeState (shstep_state.hpp).  The coefficient
// setters check, keep and derive through surface_coefficients.hpp, as the planar walls and the cylinders do: each writes
// its tables into a copy of the record, and install_cone_coefficients refuses, uploads and commits it with its switches;
// on.damp and on.fric choose the dissipative instance and tell the run loops that the pass reads twists
// (step_cone_reads_twists).  The geometry's argument check is cone_check.hpp's; the work buffers and the common kernel
// arguments are surface_state.hpp's, and so is the spring history of §2.23.  What is here of §2.23: the spring setter, the
// pass with a time step and the three restart calls; on.hist chooses the HIST instance and tells the loops to hand the
// pass their dt (step_cone_history).  What is here of §2.24 (conic_roll_kernels.hpp, of which this is the only includer too): the two
// setters of rolling and twisting resistance and the launch of conic_roll_kernel behind the contact kernel; on.roll keeps
// the rows whoever asks for cone_out.  Cones have no ledger entries: the energy ledger and a cone that dissipates, holds a
// spring, resists rolling or twisting or is driven refuse each other.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/shstep.h"
#include "cone_check.hpp"
#include "cone_kernels.hpp"
#include "conic_roll_kernels.hpp"
#include "ring_tables.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"

using namespace shp;

static_assert(kMaxCones == SHSTEP_MAX_CONES && kConeLimit == SHSTEP_MAX_CONES, "one limit");
static_assert(kConeCoefRows == 4, "d_kcoef holds gamma_k, mu_k, gamma_t,k, Omega");
static_assert(kConeStride == 10, "a cone is the 8 doubles of shstep_set_cones, kn and the exponent");

static_assert(kConicXi == 3, "ConeState::hist holds (xi_g, xi_theta, phi_c)");
static_assert(kConicRollRows == 4, "d_kroll holds mu_r,k, gamma_r,k, mu_tw,k, gamma_tw,k");

int shp::step_size_cone_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out)
{
  // (SPEC §2.24 takes its normal load from the rows: they are kept whoever asks for cone_out)
  HIPCHK(c, s->cone.work.ensure(nlocal, s->cone.ncone, kConeRow, want_out || s->cone.on.roll, kConeBlock));
  if (s->cone.on.hist) HIPCHK(c, s->cone.hist.size(nlocal, s->cone.ncone));   // SPEC §2.23: 24 ncone + 1 B per owned particle
  return SHPAIR_OK;
}

int shp::step_bind_conic_history(shpair_ctx* c, shstep_state* s, int nlocal)
{
  if (!s->cone.on.hist || nlocal <= 0 || s->cone.hist.nlocal == nlocal) return SHPAIR_OK;
  RC(step_size_cone_buffers(c, s, nlocal, false));
  return s->cone.hist.bind(c, nlocal);
}

// The one place that turns a record of the cone coefficients, a copy of the state's with a setter's tables written into
// it, into the device tables ([kConeCoefRows][ncone]: gamma_k, mu_k, gamma_t,k, Omega; [ncone]: k_t,k) and the switches.
// Neither the energy ledger nor the shell ledger keeps cone entries: a coefficient, a spring, or a non-zero Omega (the
// work of the drive would go missing), while either is on is refused, and the state stays what it was.  Nothing is
// allocated for the springs while no cone has one and none had, nor for the rolling table ([kConicRollRows][ncone]:
// mu_r,k, gamma_r,k, mu_tw,k, gamma_tw,k; SPEC §2.24; conic_roll_kernel is the only reader); a change of hist drops the
// history.
static int install_cone_coefficients(shpair_ctx* c, shstep_state* s, const char* what, const SurfaceCoefficients& r)
{
  ConeState& ks = s->cone;
  const SurfaceSwitches on = derive_surface_switches(r), was = ks.on;
  bool driven = false;
  for (const double o : r.Omega) driven = driven || o != 0.0;
  if ((on.any() || driven) && (c->ledger_on || s->cyl.shell_ledger_on))
    CTX_FAIL(c, SHPAIR_ESTATE, "cone %s: the %s ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
             "(%s) or leave every cone coefficient and Omega 0", what, c->ledger_on ? "energy" : "shell",
             c->ledger_on ? "shstep_set_energy_ledger" : "shstep_set_shell_ledger");
  const std::vector<double> h = pack_surface_tables({&r.gamma, &r.mu, &r.gamma_t, &r.Omega});
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still read the old table
  HIPCHK(c, hipMemcpy(ks.d_kcoef.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));   // (shstep_set_cones sized it)
  if (on.hist || was.hist) {   // (the HIST instance is the only reader)
    HIPCHK(c, ks.d_kkt.ensure(r.k_t.size()));
    HIPCHK(c, hipMemcpy(ks.d_kkt.p, r.k_t.data(), r.k_t.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (on.roll || was.roll) {
    const std::vector<double> hr = pack_surface_tables({&r.mu_r, &r.gamma_r, &r.mu_tw, &r.gamma_tw});
    HIPCHK(c, ks.d_kroll.ensure(hr.size()));
    HIPCHK(c, hipMemcpy(ks.d_kroll.p, hr.data(), hr.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  ks.coef = r;
  ks.on = on;
  if (on.hist != was.hist) ks.hist.nlocal = -1;
  return SHPAIR_OK;
}

extern "C" {

int shstep_set_cones(shpair_ctx* c, int ncone, const double* cone8, const double* kn, const double* exponent)
{
  STEP_PROLOGUE(c);
  const std::string bad = check_cones(ncone, cone8, kn, exponent);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  ConeState& ks = s->cone;
  std::vector<double> h((size_t)kConeStride * (size_t)ncone);
  for (int k = 0; k < ncone; ++k) {
    double* r = &h[(size_t)kConeStride * k];
    for (int j = 0; j < 8; ++j) r[j] = cone8[8 * k + j];
    r[8] = kn[k]; r[9] = exponent[k];
  }
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still read the old tables
  if (ncone > 0) {   // (no cone: nothing is allocated)
    HIPCHK(c, ks.d_cone.ensure(h.size()));
    HIPCHK(c, hipMemcpy(ks.d_cone.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, ks.d_kcoef.ensure((size_t)kConeCoefRows * ncone));
    HIPCHK(c, hipMemset(ks.d_kcoef.p, 0, (size_t)kConeCoefRows * ncone * sizeof(double)));
  }
  ks.h_cone = h;
  ks.coef.reset(ncone);   // every coefficient and Omega is 0 again, and the history goes with k_t,k (SPEC §2.23)
  ks.on = SurfaceSwitches{};
  ks.hist.nlocal = -1;
  ks.ncone = ncone;
  ks.cone_called = false;
  return SHPAIR_OK;
}

int shstep_set_cone_damping(shpair_ctx* c, int ncone, const double* gamma)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"damping coefficient"};
  const std::string bad = check_surface_coefficients(kConeSurface, "damping", ncone, s->cone.ncone, 1, &gamma, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncone == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cone.coef;
  r.gamma.assign(gamma, gamma + ncone);
  return install_cone_coefficients(c, s, "damping", r);
}

int shstep_set_cone_friction(shpair_ctx* c, int ncone, const double* mu, const double* gamma_t)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu, gamma_t};
  const char* names[2] = {"friction coefficient mu", "friction coefficient gamma_t"};
  const std::string bad = check_surface_coefficients(kConeSurface, "friction", ncone, s->cone.ncone, 2, tabs, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncone == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cone.coef;
  r.mu.assign(mu, mu + ncone);
  r.gamma_t.assign(gamma_t, gamma_t + ncone);
  return install_cone_coefficients(c, s, "friction", r);
}

int shstep_set_cone_rotation(shpair_ctx* c, int ncone, const double* omega)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"angular velocity"};
  const std::string bad = check_surface_coefficients(kConeSurface, "rotation", ncone, s->cone.ncone, 1, &omega, names, true);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncone == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cone.coef;
  r.Omega.assign(omega, omega + ncone);
  return install_cone_coefficients(c, s, "rotation", r);
}

// k_t,k per cone (SPEC §2.23); a mu_k set earlier, or later, makes it a history cone
int shstep_set_conic_tangential_spring(shpair_ctx* c, int ncone, const double* kt)
{
  STEP_PROLOGUE(c);
  const std::string bad = check_conic_spring(ncone, s->cone.ncone, kt);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncone == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cone.coef;
  r.k_t.assign(kt, kt + ncone);
  return install_cone_coefficients(c, s, "tangential spring", r);
}

// mu_r,k (a length) and gamma_r,k per cone (SPEC §2.24); a cone has rolling resistance iff both are non-zero
int shstep_set_rolling_con(shpair_ctx* c, int ncone, const double* mu_r, const double* gamma_r)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu_r, gamma_r};
  const std::string bad = check_conic_resistance("rolling", ncone, s->cone.ncone, tabs);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncone == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cone.coef;
  r.mu_r.assign(mu_r, mu_r + ncone);
  r.gamma_r.assign(gamma_r, gamma_r + ncone);
  return install_cone_coefficients(c, s, "rolling resistance", r);
}

// ... and mu_tw,k, gamma_tw,k: twisting resistance, alike
int shstep_set_twisting_con(shpair_ctx* c, int ncone, const double* mu_tw, const double* gamma_tw)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu_tw, gamma_tw};
  const std::string bad = check_conic_resistance("twisting", ncone, s->cone.ncone, tabs);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncone == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cone.coef;
  r.mu_tw.assign(mu_tw, mu_tw + ncone);
  r.gamma_tw.assign(gamma_tw, gamma_tw + ncone);
  return install_cone_coefficients(c, s, "twisting resistance", r);
}

// The geometry never moves: the host copy is what the device holds.
int shstep_get_cones(shpair_ctx* c, int ncone, double* cone8_out)
{
  STEP_PROLOGUE(c);
  if (ncone != s->cone.ncone) CTX_FAIL(c, SHPAIR_EINVAL, "get cones: room for %d cones, %d are set", ncone, s->cone.ncone);
  if (ncone == 0) return SHPAIR_OK;
  if (!cone8_out) CTX_FAIL(c, SHPAIR_EINVAL, "get cones: null output pointer");
  for (int k = 0; k < ncone; ++k)
    for (int j = 0; j < 8; ++j) cone8_out[8 * k + j] = s->cone.h_cone[(size_t)kConeStride * k + j];
  return SHPAIR_OK;
}

}  // extern "C"

// The cone pass behind shstep_cone_force_device (no spring set: dt is not looked at) and shstep_conic_contact_device.
static int cone_pass(shpair_ctx* c, shstep_state* s, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                     int groupbit, double* f, double* torque, double* cone_out, const double* twist, double dt, void* stream)
{
  if (nlocal < 0) CTX_FAIL(c, SHPAIR_EINVAL, "nlocal %d < 0", nlocal);
  ConeState& ks = s->cone;
  if (ks.ncone == 0 || nlocal == 0) return SHPAIR_OK;   // no cone: nothing is allocated, zeroed or launched
  if (!x || !quat || !shtype || !mask || !f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  const bool diss = ks.on.damp || ks.on.fric;   // every coefficient 0: the elastic instance, whatever twist and Omega are
  if (diss && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "cone %s: null twist pointer", ks.on.damp ? "damping" : "friction");
  const bool hist = ks.on.hist;   // SPEC §2.23
  if (hist && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "cone tangential spring: null twist pointer");
  const bool roll = ks.on.roll;   // SPEC §2.24
  if (roll && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "%s", conic_resistance_null_twist());
  if (c->tables_dirty || c->quad_dirty) RC(shpair_prepare_tables(c));
  const bool want_rows = cone_out != nullptr || roll;   // (§2.24 takes its normal load from them)
  RC(step_size_cone_buffers(c, s, nlocal, want_rows));
  hipStream_t st = (hipStream_t)stream;
  ConeParams P{};   // the common kernel arguments, and the coefficient table
  fill_surface_params(P, c, QuadLayout(c->lmax, c->nq), nlocal, ks.ncone, ks.d_cone.p, x, quat, shtype, mask, groupbit, f, torque, ks.work, want_rows);
  P.coef = ks.d_kcoef.p; P.twist = twist;
  ConicSpringParams H{};   // (the HIST instance only)
  const bool advance = hist && dt > 0.0;
  if (hist) {
    static_cast<ConeParams&>(H) = P;
    H.kt = ks.d_kkt.p; H.xi = ks.hist.xi.p; H.live = ks.hist.live.p; H.dt = dt;
    RC(ks.hist.begin_pass(c, nlocal, advance, st, &H.live_dead));
  }
  HIPCHK(c, hipMemsetAsync(ks.work.count.p, 0, 2 * sizeof(int), st));
  const unsigned nb = nblk(nlocal, kConeBlock);
  hipLaunchKernelGGL(cone_candidates_kernel, dim3(nb), dim3(kConeBlock), 0, st, P);
  if (advance)   // the bits of the cones a particle no longer reaches die, whether or not the contact kernel visits it
    hipLaunchKernelGGL(conic_live_sweep_kernel, dim3(nb), dim3(kConeBlock), 0, st, nlocal, (const unsigned char*)ks.work.mask.p, ks.hist.live.p);
  // one wave per queued particle: a grid that covers nlocal, capped; the waves stride over the device-side count
  const unsigned ncb = nblk(nlocal, kConeBlock / 64);
  const dim3 grid(ncb < (unsigned)kConeMaxBlocks ? ncb : (unsigned)kConeMaxBlocks);
  if (hist)
    hipLaunchKernelGGL(conic_spring_kernel, grid, dim3(kConeBlock), 0, st, H);
  else
    hipLaunchKernelGGL(diss ? cone_contact_dissipative_kernel : cone_contact_kernel, grid, dim3(kConeBlock), 0, st, P);
  if (roll) {   // SPEC §2.24: the two couples from the rows the contact kernel just left, one lane per owned row; a look adds them too
    ConicRollParams Q{};
    Q.nlocal = nlocal; Q.ncone = ks.ncone;
    Q.kmask = ks.work.mask.p; Q.x = x; Q.cones = ks.d_cone.p; Q.coef = ks.d_kcoef.p; Q.twist = twist; Q.kroll = ks.d_kroll.p;
    Q.rows = ks.work.rows.p; Q.torque = torque;
    hipLaunchKernelGGL(conic_roll_kernel, dim3(nb), dim3(kConeBlock), 0, st, Q);
  }
  if (cone_out) {
    hipLaunchKernelGGL(cone_rows_partial_kernel, dim3(nb, ks.ncone), dim3(kConeBlock), 0, st, nlocal, ks.ncone,
                       (const unsigned char*)ks.work.mask.p, (const double*)ks.work.rows.p, ks.work.part.p);
    hipLaunchKernelGGL(cone_rows_final_kernel, dim3(ks.ncone), dim3(kConeBlock), 0, st, (int)nb, (const double*)ks.work.part.p, cone_out);
  }
  HIPCHK(c, hipGetLastError());
  ks.cone_called = true;
  return SHPAIR_OK;
}

extern "C" {

int shstep_cone_force_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                             int groupbit, double* f, double* torque, double* cone_out, const double* twist, void* stream)
{
  STEP_PROLOGUE(c);
  if (s->cone.on.hist)
    CTX_FAIL(c, SHPAIR_EINVAL, "a cone tangential spring is set: the cone pass needs the form with a time step (shstep_conic_contact_device)");
  return cone_pass(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, cone_out, twist, 0.0, stream);
}

int shstep_conic_contact_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                                int groupbit, double* f, double* torque, double* cone_out, const double* twist, double dt, void* stream)
{
  STEP_PROLOGUE(c);
  if (!(dt >= 0.0) || !std::isfinite(dt)) CTX_FAIL(c, SHPAIR_EINVAL, "cone contact: dt %g must be finite and >= 0", dt);
  return cone_pass(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, cone_out, twist, dt, stream);
}

// (xi_g, xi_theta, phi_c) of the cones to / from the host (SPEC §2.23): [nlocal][ncone][3], 0 where the bit is dead
int shstep_copy_conic_history(shpair_ctx* c, int nlocal, double* xi_out)
{
  STEP_PROLOGUE(c);
  return s->cone.hist.copy_out(c, "cone", "shstep_set_conic_tangential_spring", s->cone.on.hist, nlocal, s->cone.ncone, xi_out);
}

int shstep_set_conic_history(shpair_ctx* c, int nlocal, const double* xi)
{
  STEP_PROLOGUE(c);
  return s->cone.hist.set_from_host(c, s, "cone", "shstep_set_conic_tangential_spring", s->cone.on.hist, nlocal, s->cone.ncone, xi,
                                    step_size_cone_buffers);
}

int shstep_reset_conic_history(shpair_ctx* c)
{
  STEP_PROLOGUE(c);
  return s->cone.hist.reset(c);
}

int shstep_get_cone_stats(shpair_ctx* c, int* ncontacts)
{
  STEP_PROLOGUE(c);
  if (!ncontacts) CTX_FAIL(c, SHPAIR_EINVAL, "null output pointer");
  *ncontacts = 0;
  if (!s->cone.cone_called) return SHPAIR_OK;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(ncontacts, s->cone.work.count.p + 1, sizeof(int), hipMemcpyDeviceToHost));
  return shpair_check_device_errors(c, c->stream);
}

}  // extern "C"
