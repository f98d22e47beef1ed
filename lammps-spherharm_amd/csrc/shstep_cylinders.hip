// shstep_cylinders.hip — the cylindrical container walls of include/shstep.h (docs/SPEC.md §2.18) on top of
// cylinder_kernels.hpp, cyl_power_kernels.hpp (§2.20) and cyl_roll_kernels.hpp (§2.21), of which this is the only includer.
// The host layer is shell_host.hpp's, shared with the cones: the state (CylState of shstep_state.hpp), the coefficient
// setters and the one place that installs a record, the pass in both forms, the statistics, the read-back for restarts and
// the three history calls of §2.19.  Here: what the family is (CylHost), its two hooks, the entry points, and the shell
// ledger of §2.20: its switch and read-back, the sizing of its power rows, the choice of the LEDGER twin of an instance
// while both ledgers are on, and the fold of the rows, which shstep_ledger_fold_device (shstep_ledger.hip) calls.  The
// geometry's argument check is cylinder_check.hpp's.
#include <hip/hip_runtime.h>

#include "../../include/shstep.h"
#include "cylinder_check.hpp"
#include "cyl_power_kernels.hpp"
#include "cyl_roll_kernels.hpp"
#include "cylinder_kernels.hpp"
#include "shell_host.hpp"

using namespace shp;

static_assert(kMaxCylinders == SHSTEP_MAX_CYLINDERS && kCylinderLimit == SHSTEP_MAX_CYLINDERS, "one limit");
static_assert(kShellDoubles == 3 + 3 * SHSTEP_MAX_CYLINDERS && kShellDoubles == kShellTotals + kCylPowerRow * kMaxCylinders,
              "the shell accumulator holds 3 totals and 3 per cylinder");
static_assert(kCylCoefRows == 4, "d_coef holds gamma_c, mu_c, gamma_t,c, Omega");
static_assert(kCylRollRows == 4, "d_roll holds mu_r,c, gamma_r,c, mu_tw,c, gamma_tw,c");

namespace {
struct CylHost {
  using State = CylState;
  using Params = CylParams;
  using SpringParams = CylSpringParams;
  using RollParams = CylRollParams;
  static State& state(shstep_state* s) { return s->cyl; }
  static constexpr SurfaceKind kind = kCylinderSurface;
  static constexpr int kIn = 7, kStride = kCylStride, kRow = kCylRow, kBlock = kCylBlock, kMaxBlocks = kCylMaxBlocks;
  static constexpr const char* spring_setter = "shstep_set_cyl_tangential_spring";
  static constexpr const char* contact_call = "shstep_cyl_contact_device";
  static const char* roll_null_twist() { return "cylinder rolling or twisting resistance: null twist pointer"; }
  static constexpr auto candidates = cyl_candidates_kernel;
  static constexpr auto live_sweep = cyl_live_sweep_kernel;
  static constexpr auto rows_partial = cyl_rows_partial_kernel;
  static constexpr auto rows_final = cyl_rows_final_kernel;
  static int size_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out) { return step_size_cyl_buffers(c, s, nlocal, want_out); }

  // The energy ledger itself has no cylinder entries: a coefficient while it is on is refused unless the shell ledger is on
  // (SPEC §2.20).
  static int refuse(shpair_ctx* c, shstep_state* s, const char* what, const SurfaceCoefficients&, const SurfaceSwitches& on)
  {
    if (on.any() && c->ledger_on && !s->cyl.shell_ledger_on)
      CTX_FAIL(c, SHPAIR_ESTATE, "cylinder %s: the energy ledger is on and keeps no cylinder entries (docs/SPEC.md 2.18); switch it off "
               "(shstep_set_energy_ledger) or leave every cylinder coefficient 0", what);
    return SHPAIR_OK;
  }
  // five instances: elastic, dissipative, the one with springs, and, while both ledgers are on and a coefficient is set, the
  // LEDGER twins of the last two, which also leave the power rows (SPEC §2.20; the elastic contact dissipates nothing and
  // the drive does no work on it: it keeps its one instance)
  static ShellLedgerUse launch_contact(shpair_ctx* c, State& cs, const Params& P, const SpringParams& H, bool diss, bool hist, dim3 grid,
                                       hipStream_t st)
  {
    ShellLedgerUse use;
    use.ledger = cs.shell_ledger_on && c->ledger_on;
    use.power = use.ledger && (diss || hist);
    if (use.power && hist) {
      CylPowerSpringParams L{};
      static_cast<CylSpringParams&>(L) = H;
      L.prows = cs.d_cprows.p;
      hipLaunchKernelGGL(cyl_power_spring_kernel, grid, dim3(kCylBlock), 0, st, L);
    } else if (use.power) {
      CylPowerParams L{};
      static_cast<CylParams&>(L) = P;
      L.prows = cs.d_cprows.p;
      hipLaunchKernelGGL(cyl_power_dissipative_kernel, grid, dim3(kCylBlock), 0, st, L);
    } else if (hist)
      hipLaunchKernelGGL(cyl_spring_kernel, grid, dim3(kCylBlock), 0, st, H);
    else
      hipLaunchKernelGGL(diss ? cyl_contact_dissipative_kernel : cyl_contact_kernel, grid, dim3(kCylBlock), 0, st, P);
    return use;
  }
  static void launch_roll(State& cs, RollParams Q, const ShellLedgerUse& use, unsigned nb, hipStream_t st)
  {
    Q.add_power = use.power ? 1 : 0;
    Q.prows = use.ledger ? cs.d_cprows.p : nullptr;
    hipLaunchKernelGGL(use.ledger ? cyl_roll_ledger_kernel : cyl_roll_kernel, dim3(nb), dim3(kCylBlock), 0, st, Q);
  }
};

// a pass has run: the power rows are fresh (§2.21 writes them where the elastic instance left none), and the next fold adds
// them, once
int note_fresh_rows(shstep_state* s, int rc, const ShellLedgerUse& use, int nlocal)
{
  if (rc == SHPAIR_OK && (use.power || (use.ledger && s->cyl.on.roll))) {
    s->cyl.shell_fresh = true;
    s->cyl.shell_nlocal = nlocal;
  }
  return rc;
}
}  // namespace

// (SPEC §2.21 takes its normal load from the rows: they are kept whoever asks for cyl_out; §2.19: 16 ncyl + 1 B of history per owned particle)
int shp::step_size_cyl_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out)
{
  RC(size_shell_buffers<CylHost>(c, s, nlocal, want_out));
  if (s->cyl.shell_ledger_on && c->ledger_on) {   // SPEC §2.20: the power rows and the block sums of their fold
    const size_t n = nlocal > 0 ? (size_t)nlocal : 1;
    HIPCHK(c, s->cyl.d_cprows.ensure((size_t)kCylPowerRow * n * (size_t)s->cyl.n));
    HIPCHK(c, s->cyl.d_cppart.ensure((size_t)kCylPowerRow * nblk(nlocal, kCylBlock) * (size_t)s->cyl.n));
  }
  return SHPAIR_OK;
}

int shp::step_bind_cyl_history(shpair_ctx* c, shstep_state* s, int nlocal) { return bind_shell_history<CylHost>(c, s, nlocal); }

// SPEC §2.20, called by shstep_ledger_fold_device: the rows of the last LEDGER pass, dt times their ordered sums into the
// shell accumulator; the buffers are the pass'.
int shp::step_fold_shell_rows(shpair_ctx* c, shstep_state* s, double dt, hipStream_t st)
{
  CylState& cs = s->cyl;
  if (!cs.shell_fresh || cs.n == 0) return SHPAIR_OK;
  const int nb = (int)nblk(cs.shell_nlocal, kCylBlock);
  hipLaunchKernelGGL(cyl_power_partial_kernel, dim3(nb, cs.n), dim3(kCylBlock), 0, st, cs.shell_nlocal, cs.n,
                     (const unsigned char*)cs.work.mask.p, (const double*)cs.d_cprows.p, cs.d_cppart.p);
  hipLaunchKernelGGL(cyl_power_final_kernel, dim3(1), dim3(kCylBlock), 0, st, cs.n, nb, (const double*)cs.d_cppart.p, dt, cs.d_shell.p);
  HIPCHK(c, hipGetLastError());
  cs.shell_fresh = false;
  return SHPAIR_OK;
}

extern "C" {

int shstep_set_cylinders(shpair_ctx* c, int ncyl, const double* cyl7, const double* kn, const double* exponent)
{
  STEP_PROLOGUE(c);
  const std::string bad = check_cylinders(ncyl, cyl7, kn, exponent);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  RC(set_shell_geometry<CylHost>(c, s, ncyl, cyl7, kn, exponent));
  // the shell ledger's entries go with the cylinders (SPEC §2.20), as the wall entries go with the walls
  CylState& cs = s->cyl;
  cs.shell_fresh = false;
  if (cs.d_shell.p) HIPCHK(c, hipMemset(cs.d_shell.p, 0, kShellDoubles * sizeof(double)));
  return SHPAIR_OK;
}

int shstep_set_cylinder_damping(shpair_ctx* c, int ncyl, const double* gamma)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<CylHost>(c, s, kSetDamping, ncyl, gamma);
}

int shstep_set_cylinder_friction(shpair_ctx* c, int ncyl, const double* mu, const double* gamma_t)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<CylHost>(c, s, kSetFriction, ncyl, mu, gamma_t);
}

int shstep_set_cylinder_rotation(shpair_ctx* c, int ncyl, const double* omega)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<CylHost>(c, s, kSetRotation, ncyl, omega);
}

// k_t,c per cylinder (SPEC §2.19); a mu_c set earlier, or later, makes it a history cylinder
int shstep_set_cyl_tangential_spring(shpair_ctx* c, int ncyl, const double* kt)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<CylHost>(c, s, kSetSpring, ncyl, kt);
}

// mu_r,c (a length) and gamma_r,c per cylinder (SPEC §2.21); a cylinder has rolling resistance iff both are non-zero
int shstep_set_rolling_cyl(shpair_ctx* c, int ncyl, const double* mu_r, const double* gamma_r)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<CylHost>(c, s, kSetRolling, ncyl, mu_r, gamma_r);
}

// ... and mu_tw,c, gamma_tw,c: twisting resistance, alike
int shstep_set_twisting_cyl(shpair_ctx* c, int ncyl, const double* mu_tw, const double* gamma_tw)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<CylHost>(c, s, kSetTwisting, ncyl, mu_tw, gamma_tw);
}

int shstep_get_cylinders(shpair_ctx* c, int ncyl, double* cyl7_out)
{
  STEP_PROLOGUE(c);
  return get_shell_geometry<CylHost>(c, s, ncyl, cyl7_out);
}

int shstep_cylinder_force_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                                 int groupbit, double* f, double* torque, double* cyl_out, const double* twist, void* stream)
{
  STEP_PROLOGUE(c);
  ShellLedgerUse use;
  return note_fresh_rows(s, shell_force_call<CylHost>(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, cyl_out, twist, stream, &use),
                         use, nlocal);
}

int shstep_cyl_contact_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                              int groupbit, double* f, double* torque, double* cyl_out, const double* twist, double dt, void* stream)
{
  STEP_PROLOGUE(c);
  ShellLedgerUse use;
  return note_fresh_rows(s, shell_contact_call<CylHost>(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, cyl_out, twist, dt, stream, &use),
                         use, nlocal);
}

// (xi_a, xi_theta) of the cylinders to / from the host (SPEC §2.19): [nlocal][ncyl][2], 0 where the bit is dead
int shstep_copy_cyl_history(shpair_ctx* c, int nlocal, double* xi_out)
{
  STEP_PROLOGUE(c);
  return copy_shell_history<CylHost>(c, s, nlocal, xi_out);
}

int shstep_set_cyl_history(shpair_ctx* c, int nlocal, const double* xi)
{
  STEP_PROLOGUE(c);
  return set_shell_history<CylHost>(c, s, nlocal, xi);
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
  if (per_shell3 && ncyl != cs.n) CTX_FAIL(c, SHPAIR_EINVAL, "get shell ledger: room for %d cylinders, %d are set", ncyl, cs.n);
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
  return get_shell_stats<CylHost>(c, s, ncontacts);
}

}  // extern "C"
