// shstep_cylinders.hip — the cylindrical container walls of include/shstep.h (docs/SPEC.md §2.18) on top of
// cylinder_kernels.hpp, of which this is the only includer: the cylinders and their coefficients (damping, friction,
// rotation about the axis), the cylinder pass, its statistics and the read-back for restarts.  The state is CylState
// (shstep_state.hpp).  The coefficient setters check, keep and derive through surface_coefficients.hpp, as the planar
// walls do: each writes its tables into a copy of the record, and install_cyl_coefficients refuses, uploads and commits it
// with its switches; on.damp and on.fric choose the dissipative instance and tell the run loops that the pass reads twists
// (step_cyl_reads_twists).  The geometry's argument check is cylinder_check.hpp's; the work buffers, the spring
// history of §2.19 and the common kernel arguments are surface_state.hpp's.  What is here of §2.19: the pass with a time
// step and the three restart calls; on.hist chooses the HIST instance and tells the loops to hand the pass their dt
// (step_cyl_history).  What is here of §2.20 (cyl_power_kernels.hpp, of which this is the only includer too): the shell
// ledger's switch and read-back, the choice of the LEDGER twin of an instance while both ledgers are on, and the fold of
// its power rows, which shstep_ledger_fold_device (shstep_ledger.hip) calls.  What is here of §2.21 (cyl_roll_kernels.hpp, the
// same): the two setters of rolling and twisting resistance and the launch of cyl_roll_kernel behind the contact kernel;
// on.roll keeps the rows whoever asks for cyl_out.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/shstep.h"
#include "cylinder_check.hpp"
#include "cyl_power_kernels.hpp"
#include "cyl_roll_kernels.hpp"
#include "cylinder_kernels.hpp"
#include "ring_tables.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"

using namespace shp;

static_assert(kMaxCylinders == SHSTEP_MAX_CYLINDERS && kCylinderLimit == SHSTEP_MAX_CYLINDERS, "one limit");
static_assert(kShellDoubles == 3 + 3 * SHSTEP_MAX_CYLINDERS && kShellDoubles == kShellTotals + kCylPowerRow * kMaxCylinders,
              "the shell accumulator holds 3 totals and 3 per cylinder");
static_assert(kCylCoefRows == 4, "d_ccoef holds gamma_c, mu_c, gamma_t,c, Omega");
static_assert(kCylRollRows == 4, "d_croll holds mu_r,c, gamma_r,c, mu_tw,c, gamma_tw,c");

int shp::step_size_cyl_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out)
{
  // (SPEC §2.21 takes its normal load from the rows: they are kept whoever asks for cyl_out)
  HIPCHK(c, s->cyl.work.ensure(nlocal, s->cyl.ncyl, kCylRow, want_out || s->cyl.on.roll, kCylBlock));
  if (s->cyl.on.hist) HIPCHK(c, s->cyl.hist.size(nlocal, s->cyl.ncyl));   // SPEC §2.19: 16 ncyl + 1 B per owned particle
  if (s->cyl.shell_ledger_on && c->ledger_on) {   // SPEC §2.20: the power rows and the block sums of their fold
    const size_t n = nlocal > 0 ? (size_t)nlocal : 1;
    HIPCHK(c, s->cyl.d_cprows.ensure((size_t)kCylPowerRow * n * (size_t)s->cyl.ncyl));
    HIPCHK(c, s->cyl.d_cppart.ensure((size_t)kCylPowerRow * nblk(nlocal, kCylBlock) * (size_t)s->cyl.ncyl));
  }
  return SHPAIR_OK;
}

int shp::step_bind_cyl_history(shpair_ctx* c, shstep_state* s, int nlocal)
{
  if (!s->cyl.on.hist || nlocal <= 0 || s->cyl.hist.nlocal == nlocal) return SHPAIR_OK;
  RC(step_size_cyl_buffers(c, s, nlocal, false));
  return s->cyl.hist.bind(c, nlocal);
}

// The one place that turns a record of the cylinder coefficients, a copy of the state's with a setter's tables written
// into it, into the device tables ([kCylCoefRows][ncyl]: gamma_c, mu_c, gamma_t,c, Omega; [ncyl]: k_t,c) and the switches
// (derive_surface_switches has the rules).  The energy ledger itself has no cylinder entries: a coefficient while it is on
// is refused unless the shell ledger is on (SPEC §2.20), and the state stays what it was.  Nothing is allocated for the
// springs while no cylinder has one and none had, nor for the rolling table ([kCylRollRows][ncyl]: mu_r,c, gamma_r,c,
// mu_tw,c, gamma_tw,c; SPEC §2.21; cyl_roll_kernel and its ledger twin are the only readers); a change of hist drops
// the history.
static int install_cyl_coefficients(shpair_ctx* c, shstep_state* s, const char* what, const SurfaceCoefficients& r)
{
  CylState& cs = s->cyl;
  const SurfaceSwitches on = derive_surface_switches(r), was = cs.on;
  if (on.any() && c->ledger_on && !cs.shell_ledger_on)
    CTX_FAIL(c, SHPAIR_ESTATE, "cylinder %s: the energy ledger is on and keeps no cylinder entries (docs/SPEC.md 2.18); switch it off "
             "(shstep_set_energy_ledger) or leave every cylinder coefficient 0", what);
  const std::vector<double> h = pack_surface_tables({&r.gamma, &r.mu, &r.gamma_t, &r.Omega});
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still read the old table
  HIPCHK(c, hipMemcpy(cs.d_ccoef.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));   // (shstep_set_cylinders sized it)
  if (on.hist || was.hist) {   // (the HIST instance is the only reader)
    HIPCHK(c, cs.d_ckt.ensure(r.k_t.size()));
    HIPCHK(c, hipMemcpy(cs.d_ckt.p, r.k_t.data(), r.k_t.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (on.roll || was.roll) {
    const std::vector<double> hr = pack_surface_tables({&r.mu_r, &r.gamma_r, &r.mu_tw, &r.gamma_tw});
    HIPCHK(c, cs.d_croll.ensure(hr.size()));
    HIPCHK(c, hipMemcpy(cs.d_croll.p, hr.data(), hr.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  cs.coef = r;
  cs.on = on;
  if (on.hist != was.hist) cs.hist.nlocal = -1;
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
  cs.coef.reset(ncyl);   // every coefficient and Omega is 0 again, and the history goes with k_t,c (SPEC §2.19)
  cs.on = SurfaceSwitches{};
  cs.hist.nlocal = -1;
  cs.ncyl = ncyl;
  cs.cyl_called = false;
  // the shell ledger's entries go with the cylinders (SPEC §2.20), as the wall entries go with the walls
  cs.shell_fresh = false;
  if (cs.d_shell.p) HIPCHK(c, hipMemset(cs.d_shell.p, 0, kShellDoubles * sizeof(double)));
  return SHPAIR_OK;
}

int shstep_set_cylinder_damping(shpair_ctx* c, int ncyl, const double* gamma)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"damping coefficient"};
  const std::string bad = check_surface_coefficients(kCylinderSurface, "damping", ncyl, s->cyl.ncyl, 1, &gamma, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cyl.coef;
  r.gamma.assign(gamma, gamma + ncyl);
  return install_cyl_coefficients(c, s, "damping", r);
}

int shstep_set_cylinder_friction(shpair_ctx* c, int ncyl, const double* mu, const double* gamma_t)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu, gamma_t};
  const char* names[2] = {"friction coefficient mu", "friction coefficient gamma_t"};
  const std::string bad = check_surface_coefficients(kCylinderSurface, "friction", ncyl, s->cyl.ncyl, 2, tabs, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cyl.coef;
  r.mu.assign(mu, mu + ncyl);
  r.gamma_t.assign(gamma_t, gamma_t + ncyl);
  return install_cyl_coefficients(c, s, "friction", r);
}

int shstep_set_cylinder_rotation(shpair_ctx* c, int ncyl, const double* omega)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"angular velocity"};
  const std::string bad = check_surface_coefficients(kCylinderSurface, "rotation", ncyl, s->cyl.ncyl, 1, &omega, names, true);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cyl.coef;
  r.Omega.assign(omega, omega + ncyl);
  return install_cyl_coefficients(c, s, "rotation", r);
}

// k_t,c per cylinder (SPEC §2.19); a mu_c set earlier, or later, makes it a history cylinder
int shstep_set_cyl_tangential_spring(shpair_ctx* c, int ncyl, const double* kt)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"tangential spring k_t"};
  const std::string bad = check_surface_coefficients(kCylinderSurface, "tangential spring", ncyl, s->cyl.ncyl, 1, &kt, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cyl.coef;
  r.k_t.assign(kt, kt + ncyl);
  return install_cyl_coefficients(c, s, "tangential spring", r);
}

// mu_r,c (a length) and gamma_r,c per cylinder (SPEC §2.21); a cylinder has rolling resistance iff both are non-zero
int shstep_set_rolling_cyl(shpair_ctx* c, int ncyl, const double* mu_r, const double* gamma_r)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu_r, gamma_r};
  const char* names[2] = {"rolling coefficient mu_r", "rolling coefficient gamma_r"};
  const std::string bad = check_surface_coefficients(kCylinderSurface, "rolling resistance", ncyl, s->cyl.ncyl, 2, tabs, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cyl.coef;
  r.mu_r.assign(mu_r, mu_r + ncyl);
  r.gamma_r.assign(gamma_r, gamma_r + ncyl);
  return install_cyl_coefficients(c, s, "rolling resistance", r);
}

// ... and mu_tw,c, gamma_tw,c: twisting resistance, alike
int shstep_set_twisting_cyl(shpair_ctx* c, int ncyl, const double* mu_tw, const double* gamma_tw)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu_tw, gamma_tw};
  const char* names[2] = {"twisting coefficient mu_tw", "twisting coefficient gamma_tw"};
  const std::string bad = check_surface_coefficients(kCylinderSurface, "twisting resistance", ncyl, s->cyl.ncyl, 2, tabs, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (ncyl == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->cyl.coef;
  r.mu_tw.assign(mu_tw, mu_tw + ncyl);
  r.gamma_tw.assign(gamma_tw, gamma_tw + ncyl);
  return install_cyl_coefficients(c, s, "twisting resistance", r);
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

}  // extern "C"

// The cylinder pass behind shstep_cylinder_force_device (no spring set: dt is not looked at) and shstep_cyl_contact_device.
static int cyl_pass(shpair_ctx* c, shstep_state* s, int nlocal, const double* x, const double* quat, const int* shtype,
                    const int* mask, int groupbit, double* f, double* torque, double* cyl_out, const double* twist, double dt,
                    void* stream)
{
  if (nlocal < 0) CTX_FAIL(c, SHPAIR_EINVAL, "nlocal %d < 0", nlocal);
  CylState& cs = s->cyl;
  if (cs.ncyl == 0 || nlocal == 0) return SHPAIR_OK;   // no cylinder: nothing is allocated, zeroed or launched
  if (!x || !quat || !shtype || !mask || !f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  const bool diss = cs.on.damp || cs.on.fric;   // every coefficient 0: the elastic instance, whatever twist is
  if (diss && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "cylinder %s: null twist pointer", cs.on.damp ? "damping" : "friction");
  const bool hist = cs.on.hist;   // SPEC §2.19
  if (hist && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "cylinder tangential spring: null twist pointer");
  const bool roll = cs.on.roll;   // SPEC §2.21
  if (roll && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "cylinder rolling or twisting resistance: null twist pointer");
  if (c->tables_dirty || c->quad_dirty) RC(shpair_prepare_tables(c));
  const bool want_rows = cyl_out != nullptr || roll;   // (§2.21 takes its normal load from them)
  RC(step_size_cyl_buffers(c, s, nlocal, want_rows));
  hipStream_t st = (hipStream_t)stream;
  CylParams P{};   // the common kernel arguments, and the coefficient table
  fill_surface_params(P, c, QuadLayout(c->lmax, c->nq), nlocal, cs.ncyl, cs.d_cyl.p, x, quat, shtype, mask, groupbit, f, torque, cs.work, want_rows);
  P.coef = cs.d_ccoef.p; P.twist = twist;
  CylSpringParams H{};   // (the HIST instance only)
  const bool advance = hist && dt > 0.0;
  if (hist) {
    static_cast<CylParams&>(H) = P;
    H.kt = cs.d_ckt.p; H.xi = cs.hist.xi.p; H.live = cs.hist.live.p; H.dt = dt;
    RC(cs.hist.begin_pass(c, nlocal, advance, st, &H.live_dead));
  }
  // SPEC §2.20: both ledgers on and a coefficient set: the LEDGER twin of the instance, which also leaves the power rows
  // (the elastic contact dissipates nothing and the drive does no work on it: it keeps its one instance)
  const bool ledger = cs.shell_ledger_on && c->ledger_on;
  const bool power = ledger && (diss || hist);
  HIPCHK(c, hipMemsetAsync(cs.work.count.p, 0, 2 * sizeof(int), st));
  const unsigned nb = nblk(nlocal, kCylBlock);
  hipLaunchKernelGGL(cyl_candidates_kernel, dim3(nb), dim3(kCylBlock), 0, st, P);
  if (advance)   // the bits of the cylinders a particle no longer reaches die, whether or not the contact kernel visits it
    hipLaunchKernelGGL(cyl_live_sweep_kernel, dim3(nb), dim3(kCylBlock), 0, st, nlocal, (const unsigned char*)cs.work.mask.p, cs.hist.live.p);
  // one wave per queued particle: a grid that covers nlocal, capped; the waves stride over the device-side count
  const unsigned ncb = nblk(nlocal, kCylBlock / 64);
  const dim3 grid(ncb < (unsigned)kCylMaxBlocks ? ncb : (unsigned)kCylMaxBlocks);
  if (power && hist) {
    CylPowerSpringParams L{};
    static_cast<CylSpringParams&>(L) = H;
    L.prows = cs.d_cprows.p;
    hipLaunchKernelGGL(cyl_power_spring_kernel, grid, dim3(kCylBlock), 0, st, L);
  } else if (power) {
    CylPowerParams L{};
    static_cast<CylParams&>(L) = P;
    L.prows = cs.d_cprows.p;
    hipLaunchKernelGGL(cyl_power_dissipative_kernel, grid, dim3(kCylBlock), 0, st, L);
  } else if (hist)
    hipLaunchKernelGGL(cyl_spring_kernel, grid, dim3(kCylBlock), 0, st, H);
  else
    hipLaunchKernelGGL(diss ? cyl_contact_dissipative_kernel : cyl_contact_kernel, grid, dim3(kCylBlock), 0, st, P);
  if (roll) {   // SPEC §2.21: the two couples from the rows the contact kernel just left, one lane per owned row; a look adds them too
    CylRollParams Q{};
    Q.nlocal = nlocal; Q.ncyl = cs.ncyl; Q.add_power = power ? 1 : 0;
    Q.cmask = cs.work.mask.p; Q.x = x; Q.cyls = cs.d_cyl.p; Q.coef = cs.d_ccoef.p; Q.twist = twist; Q.croll = cs.d_croll.p;
    Q.rows = cs.work.rows.p; Q.torque = torque; Q.prows = ledger ? cs.d_cprows.p : nullptr;
    hipLaunchKernelGGL(ledger ? cyl_roll_ledger_kernel : cyl_roll_kernel, dim3(nb), dim3(kCylBlock), 0, st, Q);
  }
  if (cyl_out) {
    hipLaunchKernelGGL(cyl_rows_partial_kernel, dim3(nb, cs.ncyl), dim3(kCylBlock), 0, st, nlocal, cs.ncyl,
                       (const unsigned char*)cs.work.mask.p, (const double*)cs.work.rows.p, cs.work.part.p);
    hipLaunchKernelGGL(cyl_rows_final_kernel, dim3(cs.ncyl), dim3(kCylBlock), 0, st, (int)nb, (const double*)cs.work.part.p, cyl_out);
  }
  HIPCHK(c, hipGetLastError());
  cs.cyl_called = true;
  if (power || (ledger && roll)) {   // the rows are fresh (§2.21 writes them where the elastic instance left none): the next fold adds them, once
    cs.shell_fresh = true;
    cs.shell_nlocal = nlocal;
  }
  return SHPAIR_OK;
}

// SPEC §2.20, called by shstep_ledger_fold_device: the rows of the last LEDGER pass, dt times their ordered sums into the
// shell accumulator; the buffers are the pass'.
int shp::step_fold_shell_rows(shpair_ctx* c, shstep_state* s, double dt, hipStream_t st)
{
  CylState& cs = s->cyl;
  if (!cs.shell_fresh || cs.ncyl == 0) return SHPAIR_OK;
  const int nb = (int)nblk(cs.shell_nlocal, kCylBlock);
  hipLaunchKernelGGL(cyl_power_partial_kernel, dim3(nb, cs.ncyl), dim3(kCylBlock), 0, st, cs.shell_nlocal, cs.ncyl,
                     (const unsigned char*)cs.work.mask.p, (const double*)cs.d_cprows.p, cs.d_cppart.p);
  hipLaunchKernelGGL(cyl_power_final_kernel, dim3(1), dim3(kCylBlock), 0, st, cs.ncyl, nb, (const double*)cs.d_cppart.p, dt, cs.d_shell.p);
  HIPCHK(c, hipGetLastError());
  cs.shell_fresh = false;
  return SHPAIR_OK;
}

extern "C" {

int shstep_cylinder_force_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                                 int groupbit, double* f, double* torque, double* cyl_out, const double* twist, void* stream)
{
  STEP_PROLOGUE(c);
  if (s->cyl.on.hist)
    CTX_FAIL(c, SHPAIR_EINVAL, "a cylinder tangential spring is set: the cylinder pass needs the form with a time step (shstep_cyl_contact_device)");
  return cyl_pass(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, cyl_out, twist, 0.0, stream);
}

int shstep_cyl_contact_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                              int groupbit, double* f, double* torque, double* cyl_out, const double* twist, double dt, void* stream)
{
  STEP_PROLOGUE(c);
  if (!(dt >= 0.0) || !std::isfinite(dt)) CTX_FAIL(c, SHPAIR_EINVAL, "cylinder contact: dt %g must be finite and >= 0", dt);
  return cyl_pass(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, cyl_out, twist, dt, stream);
}

// (xi_a, xi_theta) of the cylinders to / from the host (SPEC §2.19): [nlocal][ncyl][2], 0 where the bit is dead
int shstep_copy_cyl_history(shpair_ctx* c, int nlocal, double* xi_out)
{
  STEP_PROLOGUE(c);
  return s->cyl.hist.copy_out(c, "cylinder", "shstep_set_cyl_tangential_spring", s->cyl.on.hist, nlocal, s->cyl.ncyl, xi_out);
}

int shstep_set_cyl_history(shpair_ctx* c, int nlocal, const double* xi)
{
  STEP_PROLOGUE(c);
  return s->cyl.hist.set_from_host(c, s, "cylinder", "shstep_set_cyl_tangential_spring", s->cyl.on.hist, nlocal, s->cyl.ncyl, xi,
                                   step_size_cyl_buffers);
}

int shstep_reset_cyl_history(shpair_ctx* c)
{
  STEP_PROLOGUE(c);
  return s->cyl.hist.reset(c);
}

// ---- the cylinder entries of the energy ledger (SPEC §2.20)
int shstep_set_shell_ledger(shpair_ctx* c, int on)
{
  STEP_PROLOGUE(c);
  CylState& cs = s->cyl;
  if ((on != 0) == cs.shell_ledger_on) return SHPAIR_OK;
  // switching off under the energy ledger with a coefficient set would recreate the state the two refusals keep out
  if (!on && c->ledger_on && cs.on.any())
    CTX_FAIL(c, SHPAIR_ESTATE, "shell ledger: the energy ledger is on and a cylinder coefficient or tangential spring is set "
             "(docs/SPEC.md 2.20); switch the energy ledger off or set every cylinder coefficient to 0 first");
  if (on && step_cone_history(c))   // SPEC §2.23: nor for what a sliding cone spring dissipates
    CTX_FAIL(c, SHPAIR_ESTATE, "shell ledger: a cone tangential spring is set and the ledger keeps no cone entries "
             "(docs/SPEC.md 2.23); set every cone k_t to 0 first");
  if (on && step_cone_dissipates(c))   // SPEC §2.22: the shell entries are the cylinders'; a cone has none
    CTX_FAIL(c, SHPAIR_ESTATE, "shell ledger: a cone damping or friction coefficient or a cone rotation is set and the ledger keeps "
             "no cone entries (docs/SPEC.md 2.22); set every cone coefficient and Omega to 0 first");
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass or fold may still use the buffers
  cs.shell_fresh = false;              // rows of the other setting are not folded
  if (!on) {
    cs.shell_ledger_on = false;   // frees nothing: the accumulator can still be read
    return SHPAIR_OK;
  }
  HIPCHK(c, cs.d_shell.ensure(kShellDoubles));
  HIPCHK(c, hipMemset(cs.d_shell.p, 0, kShellDoubles * sizeof(double)));
  cs.shell_ledger_on = true;
  return SHPAIR_OK;
}

int shstep_get_shell_ledger(shpair_ctx* c, double* totals3, int ncyl, double* per_shell3)
{
  STEP_PROLOGUE(c);
  CylState& cs = s->cyl;
  if (!totals3) CTX_FAIL(c, SHPAIR_EINVAL, "get shell ledger: null output pointer");
  if (per_shell3 && ncyl != cs.ncyl) CTX_FAIL(c, SHPAIR_EINVAL, "get shell ledger: room for %d cylinders, %d are set", ncyl, cs.ncyl);
  if (!cs.d_shell.p) CTX_FAIL(c, SHPAIR_ESTATE, "get shell ledger: the shell ledger was never switched on (shstep_set_shell_ledger)");
  double h[kShellDoubles];
  HIPCHK(c, hipDeviceSynchronize());   // a fold may still be in flight
  HIPCHK(c, hipMemcpy(h, cs.d_shell.p, sizeof(h), hipMemcpyDeviceToHost));
  for (int k = 0; k < kShellTotals; ++k) totals3[k] = h[k];
  if (per_shell3)
    for (int k = 0; k < kCylPowerRow * ncyl; ++k) per_shell3[k] = h[kShellTotals + k];
  return SHPAIR_OK;
}

int shstep_get_cylinder_stats(shpair_ctx* c, int* ncontacts)
{
  STEP_PROLOGUE(c);
  if (!ncontacts) CTX_FAIL(c, SHPAIR_EINVAL, "null output pointer");
  *ncontacts = 0;
  if (!s->cyl.cyl_called) return SHPAIR_OK;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(ncontacts, s->cyl.work.count.p + 1, sizeof(int), hipMemcpyDeviceToHost));
  return shpair_check_device_errors(c, c->stream);
}

}  // extern "C"
