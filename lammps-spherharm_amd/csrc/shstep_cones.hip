// shstep_cones.hip — the conical container walls of include/shstep.h (docs/SPEC.md §2.22) on top of cone_kernels.hpp and
// conic_roll_kernels.hpp (§2.24), of which this is the only includer.  The host layer is shell_host.hpp's, shared with the
// cylinders: the state (ConeState of shstep_state.hpp), the coefficient setters and the one place that installs a record,
// the pass in both forms, the statistics, the read-back for restarts and the three history calls of §2.23.  Here: what
// the family is (ConeHost), its two hooks, and the entry points.  The geometry's argument check is cone_check.hpp's.
// Cones have no ledger entries: either ledger and a cone that dissipates, holds a spring, resists rolling or twisting or is
// driven refuse each other.
#include <hip/hip_runtime.h>

#include "../../include/shstep.h"
#include "cone_check.hpp"
#include "cone_kernels.hpp"
#include "conic_roll_kernels.hpp"
#include "shell_host.hpp"

using namespace shp;

static_assert(kMaxCones == SHSTEP_MAX_CONES && kConeLimit == SHSTEP_MAX_CONES, "one limit");
static_assert(kConeCoefRows == 4, "d_coef holds gamma_k, mu_k, gamma_t,k, Omega");
static_assert(kConeStride == 10, "a cone is the 8 doubles of shstep_set_cones, kn and the exponent");

static_assert(kConicXi == 3, "ConeState::hist holds (xi_g, xi_theta, phi_c)");
static_assert(kConicRollRows == 4, "d_roll holds mu_r,k, gamma_r,k, mu_tw,k, gamma_tw,k");

namespace {
struct ConeHost {
  using State = ConeState;
  using Params = ConeParams;
  using SpringParams = ConicSpringParams;
  using RollParams = ConicRollParams;
  static State& state(shstep_state* s) { return s->cone; }
  static constexpr SurfaceKind kind = kConeSurface;
  static constexpr int kIn = 8, kStride = kConeStride, kRow = kConeRow, kBlock = kConeBlock, kMaxBlocks = kConeMaxBlocks;
  static constexpr const char* spring_setter = "shstep_set_conic_tangential_spring";
  static constexpr const char* contact_call = "shstep_conic_contact_device";
  static const char* roll_null_twist() { return conic_resistance_null_twist(); }
  static constexpr auto candidates = cone_candidates_kernel;
  static constexpr auto live_sweep = conic_live_sweep_kernel;
  static constexpr auto rows_partial = cone_rows_partial_kernel;
  static constexpr auto rows_final = cone_rows_final_kernel;
  static int size_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out) { return step_size_cone_buffers(c, s, nlocal, want_out); }

  // Neither the energy ledger nor the shell ledger keeps cone entries: a coefficient, a spring, or a non-zero Omega (the
  // work of the drive would go missing), while either is on is refused.
  static int refuse(shpair_ctx* c, shstep_state* s, const char* what, const SurfaceCoefficients& r, const SurfaceSwitches& on)
  {
    bool driven = false;
    for (const double o : r.Omega) driven = driven || o != 0.0;
    if ((on.any() || driven) && (c->ledger_on || s->cyl.shell_ledger_on))
      CTX_FAIL(c, SHPAIR_ESTATE, "cone %s: the %s ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
               "(%s) or leave every cone coefficient and Omega 0", what, c->ledger_on ? "energy" : "shell",
               c->ledger_on ? "shstep_set_energy_ledger" : "shstep_set_shell_ledger");
    return SHPAIR_OK;
  }
  // three instances: elastic, dissipative, and the one with springs
  static ShellLedgerUse launch_contact(shpair_ctx*, State&, const Params& P, const SpringParams& H, bool diss, bool hist, dim3 grid,
                                       hipStream_t st)
  {
    if (hist)
      hipLaunchKernelGGL(conic_spring_kernel, grid, dim3(kConeBlock), 0, st, H);
    else
      hipLaunchKernelGGL(diss ? cone_contact_dissipative_kernel : cone_contact_kernel, grid, dim3(kConeBlock), 0, st, P);
    return {};
  }
  static void launch_roll(State&, const RollParams& Q, const ShellLedgerUse&, unsigned nb, hipStream_t st)
  {
    hipLaunchKernelGGL(conic_roll_kernel, dim3(nb), dim3(kConeBlock), 0, st, Q);
  }
};
}  // namespace

// (SPEC §2.24 takes its normal load from the rows: they are kept whoever asks for cone_out; §2.23: 24 ncone + 1 B of history per owned particle)
int shp::step_size_cone_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out)
{
  return size_shell_buffers<ConeHost>(c, s, nlocal, want_out);
}

int shp::step_bind_conic_history(shpair_ctx* c, shstep_state* s, int nlocal) { return bind_shell_history<ConeHost>(c, s, nlocal); }

extern "C" {

int shstep_set_cones(shpair_ctx* c, int ncone, const double* cone8, const double* kn, const double* exponent)
{
  STEP_PROLOGUE(c);
  const std::string bad = check_cones(ncone, cone8, kn, exponent);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  return set_shell_geometry<ConeHost>(c, s, ncone, cone8, kn, exponent);
}

int shstep_set_cone_damping(shpair_ctx* c, int ncone, const double* gamma)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<ConeHost>(c, s, kSetDamping, ncone, gamma);
}

int shstep_set_cone_friction(shpair_ctx* c, int ncone, const double* mu, const double* gamma_t)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<ConeHost>(c, s, kSetFriction, ncone, mu, gamma_t);
}

int shstep_set_cone_rotation(shpair_ctx* c, int ncone, const double* omega)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<ConeHost>(c, s, kSetRotation, ncone, omega);
}

// k_t,k per cone (SPEC §2.23); a mu_k set earlier, or later, makes it a history cone
int shstep_set_conic_tangential_spring(shpair_ctx* c, int ncone, const double* kt)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<ConeHost>(c, s, kSetSpring, ncone, kt);
}

// mu_r,k (a length) and gamma_r,k per cone (SPEC §2.24); a cone has rolling resistance iff both are non-zero
int shstep_set_rolling_con(shpair_ctx* c, int ncone, const double* mu_r, const double* gamma_r)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<ConeHost>(c, s, kSetRolling, ncone, mu_r, gamma_r);
}

// ... and mu_tw,k, gamma_tw,k: twisting resistance, alike
int shstep_set_twisting_con(shpair_ctx* c, int ncone, const double* mu_tw, const double* gamma_tw)
{
  STEP_PROLOGUE(c);
  return set_shell_coefficients<ConeHost>(c, s, kSetTwisting, ncone, mu_tw, gamma_tw);
}

int shstep_get_cones(shpair_ctx* c, int ncone, double* cone8_out)
{
  STEP_PROLOGUE(c);
  return get_shell_geometry<ConeHost>(c, s, ncone, cone8_out);
}

int shstep_cone_force_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                             int groupbit, double* f, double* torque, double* cone_out, const double* twist, void* stream)
{
  STEP_PROLOGUE(c);
  return shell_force_call<ConeHost>(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, cone_out, twist, stream);
}

int shstep_conic_contact_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                                int groupbit, double* f, double* torque, double* cone_out, const double* twist, double dt, void* stream)
{
  STEP_PROLOGUE(c);
  return shell_contact_call<ConeHost>(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, cone_out, twist, dt, stream);
}

// (xi_g, xi_theta, phi_c) of the cones to / from the host (SPEC §2.23): [nlocal][ncone][3], 0 where the bit is dead
int shstep_copy_conic_history(shpair_ctx* c, int nlocal, double* xi_out)
{
  STEP_PROLOGUE(c);
  return copy_shell_history<ConeHost>(c, s, nlocal, xi_out);
}

int shstep_set_conic_history(shpair_ctx* c, int nlocal, const double* xi)
{
  STEP_PROLOGUE(c);
  return set_shell_history<ConeHost>(c, s, nlocal, xi);
}

int shstep_reset_conic_history(shpair_ctx* c)
{
  STEP_PROLOGUE(c);
  return s->cone.hist.reset(c);
}

int shstep_get_cone_stats(shpair_ctx* c, int* ncontacts)
{
  STEP_PROLOGUE(c);
  return get_shell_stats<ConeHost>(c, s, ncontacts);
}

}  // extern "C"
