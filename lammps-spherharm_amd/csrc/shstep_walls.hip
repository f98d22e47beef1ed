// shstep_walls.hip — the planar walls of include/shstep.h (docs/SPEC.md §2.9, with the wall share of §2.10 damping and
// §2.11 friction) on top of wall_kernels.hpp, of which this is the only includer: the walls and their coefficients, the
// wall pass in its three forms, its statistics, and the translation of the planes (§2.12): their velocities, the advance,
// the read-back.  The state is WallState (shstep_state.hpp).  The coefficient setters check, keep and derive through
// surface_coefficients.hpp: each writes its tables into a copy of the record, and install_wall_coefficients uploads and
// commits it with its switches.  The switches on.damp and on.fric, with wall_move_on, choose the kernel instance and tell
// the run loops that the pass reads twists (step_wall_reads_twists); wall_advance_on tells them to advance the planes
// (step_walls_advance).  The tangential springs with history of §2.15 are here too: the pass with a time step and the
// three restart calls, on the history of surface_state.hpp; on.hist chooses the HIST instances and tells the loops to hand
// the pass their dt (step_wall_history).  And the rolling and twisting resistance of §2.17 (wall_roll_kernels.hpp, of
// which this is the only includer too): its two setters and its launch behind the contact kernel; on.roll makes the pass
// keep its rows and read twists.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/shstep.h"
#include "ring_tables.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"
#include "wall_kernels.hpp"
#include "wall_roll_kernels.hpp"

using namespace shp;

static_assert(kWallBlock == kLedgerBlock, "the ledger's fold partitions the wall rows as wall_rows_partial_kernel does");

int shp::step_size_wall_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out)
{
  const size_t n = nlocal > 0 ? (size_t)nlocal : 1;
  HIPCHK(c, s->walls.work.ensure(nlocal, s->walls.nwalls, 4, want_out, kWallBlock));
  if (c->ledger_on) {   // SPEC §2.13: the power rows and the block sums of the fold (the caller asked for the rows: want_out)
    HIPCHK(c, s->walls.d_wprows.ensure(2 * n * (size_t)s->walls.nwalls));
    HIPCHK(c, s->walls.d_wlpart.ensure((size_t)kLedgerWallTerms * nblk(nlocal, kLedgerBlock) * (size_t)s->walls.nwalls));
  }
  if (s->walls.on.hist) HIPCHK(c, s->walls.hist.size(nlocal, s->walls.nwalls));   // SPEC §2.15: 24 nwalls + 4 B per owned particle
  return SHPAIR_OK;
}

int shp::step_bind_wall_history(shpair_ctx* c, shstep_state* s, int nlocal)
{
  if (!s->walls.on.hist || nlocal <= 0 || s->walls.hist.nlocal == nlocal) return SHPAIR_OK;
  RC(step_size_wall_buffers(c, s, nlocal, false));
  return s->walls.hist.bind(c, nlocal);
}

// An enqueued wall pass may still read the old table: waits for the device, then sizes `dev` for the image and fills it.
static int upload_wall_table(shpair_ctx* c, DevBuf<double>& dev, const std::vector<double>& h)
{
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, dev.ensure(h.size()));
  HIPCHK(c, hipMemcpy(dev.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  return SHPAIR_OK;
}

// The one place that turns a record of the wall coefficients, a copy of the state's with a setter's tables written into
// it, into the device tables and the switches (derive_surface_switches has the rules); the state changes only once every
// upload has passed.  d_wgamma is shstep_set_walls'; nothing else is allocated while no wall has the thing and none had
// (the friction and the history instances are the only readers of d_wfric, the history instances of d_wkt,
// wall_roll_kernel and its ledger twin of d_wroll).  A change of hist drops the history.
static int install_wall_coefficients(shpair_ctx* c, shstep_state* s, const SurfaceCoefficients& r)
{
  WallState& ws = s->walls;
  const SurfaceSwitches on = derive_surface_switches(r), was = ws.on;
  RC(upload_wall_table(c, ws.d_wgamma, r.gamma));
  if (on.fric || on.hist || was.fric || was.hist) RC(upload_wall_table(c, ws.d_wfric, pack_surface_tables({&r.mu, &r.gamma_t})));
  if (on.hist || was.hist) RC(upload_wall_table(c, ws.d_wkt, r.k_t));
  if (on.roll || was.roll) RC(upload_wall_table(c, ws.d_wroll, pack_surface_tables({&r.mu_r, &r.gamma_r, &r.mu_tw, &r.gamma_tw})));
  ws.coef = r;
  ws.on = on;
  if (on.hist != was.hist) ws.hist.nlocal = -1;
  return SHPAIR_OK;
}

extern "C" {

int shstep_set_walls(shpair_ctx* c, int nwalls, const double* plane4, const double* kn, const double* exponent)
{
  STEP_PROLOGUE(c);
  if (nwalls < 0 || nwalls > SHSTEP_MAX_WALLS) CTX_FAIL(c, SHPAIR_EINVAL, "walls: %d walls, 0..%d are accepted", nwalls, SHSTEP_MAX_WALLS);
  if (nwalls > 0 && (!plane4 || !kn || !exponent)) CTX_FAIL(c, SHPAIR_EINVAL, "walls: null array pointer");
  std::vector<double> h((size_t)kWallStride * (nwalls > 0 ? nwalls : 1), 0.0);
  for (int w = 0; w < nwalls; ++w) {
    const double* p = plane4 + 4 * w;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(p[3]) || !std::isfinite(kn[w]) ||
        !std::isfinite(exponent[w]))
      CTX_FAIL(c, SHPAIR_EINVAL, "wall %d: a number that is not finite", w);
    const double nn = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    if (!(std::fabs(nn - 1.0) <= 1e-12)) CTX_FAIL(c, SHPAIR_EINVAL, "wall %d: the normal has length %.17g, not 1", w, nn);
    if (kn[w] < 0.0) CTX_FAIL(c, SHPAIR_EINVAL, "wall %d: kn %g < 0", w, kn[w]);
    if (exponent[w] < 1.0) CTX_FAIL(c, SHPAIR_EINVAL, "wall %d: exponent %g < 1", w, exponent[w]);
    double* r = &h[(size_t)kWallStride * w];
    r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3]; r[4] = kn[w]; r[5] = exponent[w];
  }
  RC(upload_wall_table(c, s->walls.d_walls, h));
  HIPCHK(c, s->walls.d_wgamma.ensure(nwalls > 0 ? (size_t)nwalls : 1));
  HIPCHK(c, hipMemset(s->walls.d_wgamma.p, 0, (nwalls > 0 ? (size_t)nwalls : 1) * sizeof(double)));
  s->walls.coef.reset(nwalls);        // every coefficient is 0 again, and the history goes with k_t,w
  s->walls.on = SurfaceSwitches{};
  s->walls.hist.nlocal = -1;
  s->walls.wall_move_on = false;      // every u_w is 0 again
  s->walls.wall_advance_on = false;
  s->walls.h_normals.assign(3 * (size_t)(nwalls > 0 ? nwalls : 0), 0.0);
  for (int w = 0; w < nwalls; ++w)
    for (int k = 0; k < 3; ++k) s->walls.h_normals[3 * (size_t)w + k] = plane4[4 * w + k];
  s->walls.nwalls = nwalls;
  s->walls.wall_called = false;
  // the energy ledger's wall entries go with the walls (SPEC §2.13): the three wall totals and every per-wall triple
  s->walls.ledger_fresh = false;
  if (s->d_ledger.p) HIPCHK(c, hipMemset(s->d_ledger.p + 2, 0, (kLedgerDoubles - 2) * sizeof(double)));
  return SHPAIR_OK;
}

int shstep_set_wall_damping(shpair_ctx* c, int nwalls, const double* gamma)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"damping coefficient"};
  const std::string bad = check_surface_coefficients(kWallSurface, "damping", nwalls, s->walls.nwalls, 1, &gamma, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (nwalls == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->walls.coef;
  r.gamma.assign(gamma, gamma + nwalls);
  return install_wall_coefficients(c, s, r);
}

int shstep_set_wall_friction(shpair_ctx* c, int nwalls, const double* mu, const double* gamma_t)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu, gamma_t};
  const char* names[2] = {"friction coefficient mu", "friction coefficient gamma_t"};
  const std::string bad = check_surface_coefficients(kWallSurface, "friction", nwalls, s->walls.nwalls, 2, tabs, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (nwalls == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->walls.coef;
  r.mu.assign(mu, mu + nwalls);   // (a mu without a gamma_t is kept: a spring set later, or earlier, makes it a history wall)
  r.gamma_t.assign(gamma_t, gamma_t + nwalls);
  return install_wall_coefficients(c, s, r);
}

int shstep_set_wall_tangential_spring(shpair_ctx* c, int nwalls, const double* kt)
{
  STEP_PROLOGUE(c);
  const char* names[1] = {"tangential spring k_t"};
  const std::string bad = check_surface_coefficients(kWallSurface, "tangential spring", nwalls, s->walls.nwalls, 1, &kt, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (nwalls == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->walls.coef;
  r.k_t.assign(kt, kt + nwalls);
  return install_wall_coefficients(c, s, r);
}

int shstep_set_wall_rolling(shpair_ctx* c, int nwalls, const double* mu_r, const double* gamma_r)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu_r, gamma_r};
  const char* names[2] = {"rolling coefficient mu_r", "rolling coefficient gamma_r"};
  const std::string bad = check_surface_coefficients(kWallSurface, "rolling resistance", nwalls, s->walls.nwalls, 2, tabs, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (nwalls == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->walls.coef;
  r.mu_r.assign(mu_r, mu_r + nwalls);
  r.gamma_r.assign(gamma_r, gamma_r + nwalls);
  return install_wall_coefficients(c, s, r);
}

int shstep_set_wall_twisting(shpair_ctx* c, int nwalls, const double* mu_tw, const double* gamma_tw)
{
  STEP_PROLOGUE(c);
  const double* tabs[2] = {mu_tw, gamma_tw};
  const char* names[2] = {"twisting coefficient mu_tw", "twisting coefficient gamma_tw"};
  const std::string bad = check_surface_coefficients(kWallSurface, "twisting resistance", nwalls, s->walls.nwalls, 2, tabs, names, false);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (nwalls == 0) return SHPAIR_OK;
  SurfaceCoefficients r = s->walls.coef;
  r.mu_tw.assign(mu_tw, mu_tw + nwalls);
  r.gamma_tw.assign(gamma_tw, gamma_tw + nwalls);
  return install_wall_coefficients(c, s, r);
}

int shstep_set_wall_velocity(shpair_ctx* c, int nwalls, const double* vel3)
{
  STEP_PROLOGUE(c);
  if (nwalls != s->walls.nwalls)
    CTX_FAIL(c, SHPAIR_EINVAL, "wall velocity: %d velocities for %d walls (call it after shstep_set_walls)", nwalls, s->walls.nwalls);
  if (nwalls == 0) return SHPAIR_OK;
  if (!vel3) CTX_FAIL(c, SHPAIR_EINVAL, "wall velocity: null array pointer");
  std::vector<double> h((size_t)kWallVelStride * nwalls);
  bool any = false, normal = false;
  for (int w = 0; w < nwalls; ++w) {
    const double* u = vel3 + 3 * w;
    if (!std::isfinite(u[0]) || !std::isfinite(u[1]) || !std::isfinite(u[2]))
      CTX_FAIL(c, SHPAIR_EINVAL, "wall %d: a velocity component that is not finite", w);
    const double* n = &s->walls.h_normals[3 * (size_t)w];
    const double nu = n[0] * u[0] + n[1] * u[1] + n[2] * u[2];   // once, here: the advance adds dt times this number
    if (!std::isfinite(nu)) CTX_FAIL(c, SHPAIR_EINVAL, "wall %d: the normal velocity is not finite", w);
    double* r = &h[(size_t)kWallVelStride * w];
    r[0] = u[0]; r[1] = u[1]; r[2] = u[2]; r[3] = nu;
    any = any || u[0] != 0.0 || u[1] != 0.0 || u[2] != 0.0;
    normal = normal || nu != 0.0;
  }
  if (!any && !s->walls.wall_move_on) return SHPAIR_OK;   // no wall moves and none did: nothing is allocated
  RC(upload_wall_table(c, s->walls.d_wvel, h));   // (read only while one of the two flags below is set)
  s->walls.wall_move_on = any;
  s->walls.wall_advance_on = normal;
  return SHPAIR_OK;
}

int shstep_advance_walls_device(shpair_ctx* c, double dt, void* stream)
{
  STEP_PROLOGUE(c);
  if (!std::isfinite(dt)) CTX_FAIL(c, SHPAIR_EINVAL, "advance walls: dt is not finite");
  if (s->walls.nwalls == 0 || !s->walls.wall_advance_on) return SHPAIR_OK;   // belts and fixed walls: the planes stay
  hipLaunchKernelGGL(wall_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, s->walls.nwalls, s->walls.d_walls.p,
                     (const double*)s->walls.d_wvel.p, dt);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shstep_get_walls(shpair_ctx* c, int nwalls, double* plane4_out)
{
  STEP_PROLOGUE(c);
  if (nwalls != s->walls.nwalls) CTX_FAIL(c, SHPAIR_EINVAL, "get walls: room for %d walls, %d are set", nwalls, s->walls.nwalls);
  if (nwalls == 0) return SHPAIR_OK;
  if (!plane4_out) CTX_FAIL(c, SHPAIR_EINVAL, "get walls: null output pointer");
  std::vector<double> h((size_t)kWallStride * nwalls);
  HIPCHK(c, hipDeviceSynchronize());   // an advance may still be in flight
  HIPCHK(c, hipMemcpy(h.data(), s->walls.d_walls.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int w = 0; w < nwalls; ++w)
    for (int k = 0; k < 4; ++k) plane4_out[4 * w + k] = h[(size_t)kWallStride * w + k];
  return SHPAIR_OK;
}

int shstep_wall_force_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                             int groupbit, double* f, double* torque, double* wall_out, void* stream)
{
  if (!c) return SHPAIR_EINVAL;
  // (no step state yet: no wall coefficient either)
  if (c->step && c->step->walls.on.damp) CTX_FAIL(c, SHPAIR_EINVAL, "wall damping needs the twist form (shstep_wall_force_damped_device)");
  if (c->step && c->step->walls.on.fric) CTX_FAIL(c, SHPAIR_EINVAL, "wall friction needs the twist form (shstep_wall_force_damped_device)");
  if (step_wall_history(c))
    CTX_FAIL(c, SHPAIR_EINVAL, "a wall tangential spring is set: the wall pass needs the form with a time step (shstep_wall_contact_device)");
  if (step_wall_rolling(c))
    CTX_FAIL(c, SHPAIR_ESTATE, "wall rolling or twisting resistance is set: the wall pass needs the twist form (shstep_wall_force_damped_device)");
  return shstep_wall_force_damped_device(c, nlocal, x, quat, shtype, mask, groupbit, f, torque, wall_out, nullptr, stream);
}

}  // extern "C"

// The wall pass behind shstep_wall_force_damped_device (no spring set: dt is not looked at) and shstep_wall_contact_device.
static int wall_pass(shpair_ctx* c, shstep_state* s, int nlocal, const double* x, const double* quat, const int* shtype,
                     const int* mask, int groupbit, double* f, double* torque, double* wall_out, const double* twist, double dt,
                     void* stream)
{
  if (nlocal < 0) CTX_FAIL(c, SHPAIR_EINVAL, "nlocal %d < 0", nlocal);
  if (s->walls.nwalls == 0 || nlocal == 0) return SHPAIR_OK;
  if (!x || !quat || !shtype || !mask || !f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  const bool damp = s->walls.on.damp, fric = s->walls.on.fric;   // every coefficient 0: the elastic instance, whatever twist is
  if (damp && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "wall damping: null twist pointer");
  if (fric && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "wall friction: null twist pointer");
  const bool hist = s->walls.on.hist;   // SPEC §2.15
  if (hist && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "wall tangential spring: null twist pointer");
  const bool roll = s->walls.on.roll;   // SPEC §2.17
  if (roll && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "wall rolling or twisting resistance: null twist pointer");
  if (c->tables_dirty || c->quad_dirty) RC(shpair_prepare_tables(c));
  const bool ledger = c->ledger_on;   // SPEC §2.13: the rows are kept whether or not the caller asks for the totals
  const bool want_rows = wall_out != nullptr || ledger || roll;   // (§2.17 takes its normal load from them)
  RC(step_size_wall_buffers(c, s, nlocal, want_rows));
  hipStream_t st = (hipStream_t)stream;
  WallParams P{};   // the common kernel arguments, and the tables of the wall coefficients
  fill_surface_params(P, c, QuadLayout(c->lmax, c->nq), nlocal, s->walls.nwalls, s->walls.d_walls.p, x, quat, shtype, mask, groupbit, f,
                      torque, s->walls.work, want_rows);
  P.wgamma = s->walls.d_wgamma.p; P.twist = twist; P.wfric = s->walls.d_wfric.p; P.wvel = s->walls.d_wvel.p;
  P.prows = s->walls.d_wprows.p;   // (written by the LEDGER instances only, which run only while the ledger is on)
  WallHistParams H{};   // (the HIST instances only)
  const bool advance = hist && dt > 0.0;
  if (hist) {
    static_cast<WallParams&>(H) = P;
    H.kt = s->walls.d_wkt.p; H.xi = s->walls.hist.xi.p; H.live = s->walls.hist.live.p; H.dt = dt;
    RC(s->walls.hist.begin_pass(c, nlocal, advance, st, &H.live_dead));
  }
  HIPCHK(c, hipMemsetAsync(s->walls.work.count.p, 0, 2 * sizeof(int), st));
  const unsigned nb = nblk(nlocal, kWallBlock);
  hipLaunchKernelGGL(wall_candidates_kernel, dim3(nb), dim3(kWallBlock), 0, st, P);
  if (advance)   // the bits of the walls a particle no longer reaches die, whether or not the contact kernel visits it
    hipLaunchKernelGGL(wall_spring_sweep_kernel, dim3(nb), dim3(kWallBlock), 0, st, nlocal, (const unsigned*)s->walls.work.mask.p, s->walls.hist.live.p);
  // one wave per queued particle: a grid that covers nlocal, capped; the waves stride over the device-side count
  const unsigned ncb = nblk(nlocal, kWallBlock / 64);
  // a u_w enters the force through the twists only: with every coefficient 0 the elastic instance runs untouched
  const bool move = s->walls.wall_move_on && (damp || fric || hist);
  // (the elastic contact dissipates nothing: with the ledger on it keeps its one instance and leaves F_w for the work)
  const bool power = ledger && (damp || fric || hist);
  const auto contact =
      power ? (move ? (fric ? wall_ledger_moving_friction_kernel : wall_ledger_moving_damped_kernel)
                    : (fric ? wall_ledger_friction_kernel : wall_ledger_damped_kernel))
            : (move ? (fric ? wall_moving_friction_kernel : wall_moving_damped_kernel)
                    : (fric ? wall_contact_friction_kernel : (damp ? wall_contact_damped_kernel : wall_contact_kernel)));
  const dim3 grid(ncb < (unsigned)kWallMaxBlocks ? ncb : (unsigned)kWallMaxBlocks);
  if (hist) {
    const auto sprung = power ? (move ? wall_spring_moving_ledger_kernel : wall_spring_ledger_kernel)
                              : (move ? wall_spring_moving_kernel : wall_spring_kernel);
    hipLaunchKernelGGL(sprung, grid, dim3(kWallBlock), 0, st, H);
  } else {
    hipLaunchKernelGGL(contact, grid, dim3(kWallBlock), 0, st, P);
  }
  if (roll) {   // SPEC §2.17: the two couples from the rows the contact kernel just left, one lane per owned row
    WallRollParams Q{};
    Q.nlocal = nlocal; Q.nwalls = s->walls.nwalls; Q.add_power = power ? 1 : 0;
    Q.wmask = s->walls.work.mask.p; Q.walls = s->walls.d_walls.p; Q.rows = s->walls.work.rows.p; Q.twist = twist;
    Q.wroll = s->walls.d_wroll.p; Q.torque = torque; Q.prows = ledger ? s->walls.d_wprows.p : nullptr;
    hipLaunchKernelGGL(ledger ? wall_roll_ledger_kernel : wall_roll_kernel, dim3(nb), dim3(kWallBlock), 0, st, Q);
  }
  if (wall_out) {
    hipLaunchKernelGGL(wall_rows_partial_kernel, dim3(nb, s->walls.nwalls), dim3(kWallBlock), 0, st, nlocal, s->walls.nwalls,
                       (const unsigned*)s->walls.work.mask.p, (const double*)s->walls.work.rows.p, s->walls.work.part.p);
    hipLaunchKernelGGL(wall_rows_final_kernel, dim3(s->walls.nwalls), dim3(kWallBlock), 0, st, (int)nb, (const double*)s->walls.work.part.p, wall_out);
  }
  HIPCHK(c, hipGetLastError());
  s->walls.wall_called = true;
  if (ledger) {
    s->walls.ledger_fresh = true;
    s->walls.ledger_nlocal = nlocal;
    s->walls.ledger_power = power || roll;   // (§2.17 writes the power rows where the elastic instance left none)
  }
  return SHPAIR_OK;
}

extern "C" {

int shstep_wall_force_damped_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype,
                                    const int* mask, int groupbit, double* f, double* torque, double* wall_out,
                                    const double* twist, void* stream)
{
  STEP_PROLOGUE(c);
  if (s->walls.on.hist)
    CTX_FAIL(c, SHPAIR_EINVAL, "a wall tangential spring is set: the wall pass needs the form with a time step (shstep_wall_contact_device)");
  return wall_pass(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, wall_out, twist, 0.0, stream);
}

int shstep_wall_contact_device(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                               int groupbit, double* f, double* torque, double* wall_out, const double* twist, double dt,
                               void* stream)
{
  STEP_PROLOGUE(c);
  if (!(dt >= 0.0) || !std::isfinite(dt)) CTX_FAIL(c, SHPAIR_EINVAL, "wall contact: dt %g must be finite and >= 0", dt);
  return wall_pass(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, wall_out, twist, dt, stream);
}

// xi of the walls to / from the host (SPEC §2.15): [nlocal][nwalls][3], 0 where the bit is dead
int shstep_copy_wall_history(shpair_ctx* c, int nlocal, double* xi_out)
{
  STEP_PROLOGUE(c);
  return s->walls.hist.copy_out(c, "wall", "shstep_set_wall_tangential_spring", s->walls.on.hist, nlocal, s->walls.nwalls, xi_out);
}

int shstep_set_wall_history(shpair_ctx* c, int nlocal, const double* xi)
{
  STEP_PROLOGUE(c);
  return s->walls.hist.set_from_host(c, s, "wall", "shstep_set_wall_tangential_spring", s->walls.on.hist, nlocal, s->walls.nwalls, xi,
                                     step_size_wall_buffers);
}

int shstep_reset_wall_history(shpair_ctx* c)
{
  STEP_PROLOGUE(c);
  return s->walls.hist.reset(c);
}

int shstep_wall_force(shpair_ctx* c, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                      int groupbit, double* f, double* torque, double* wall_out)
{
  STEP_PROLOGUE(c);
  if (nlocal < 0) CTX_FAIL(c, SHPAIR_EINVAL, "nlocal %d < 0", nlocal);
  if (s->walls.nwalls == 0 || nlocal == 0) return SHPAIR_OK;
  if (!x || !quat || !shtype || !mask || !f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  if (s->walls.on.hist)   // (ahead of the staging; shstep_wall_force_device would refuse behind it)
    CTX_FAIL(c, SHPAIR_EINVAL, "a wall tangential spring is set: the wall pass needs the form with a time step (shstep_wall_contact_device)");
  if (s->walls.on.roll)   // (the same: this form has no twists to hand on)
    CTX_FAIL(c, SHPAIR_ESTATE, "wall rolling or twisting resistance is set: the wall pass needs the twist form (shstep_wall_force_damped_device)");
  const size_t n = (size_t)nlocal, nw = (size_t)s->walls.nwalls;
  HIPCHK(c, s->s_x.ensure(3 * n)); HIPCHK(c, s->s_q.ensure(4 * n)); HIPCHK(c, s->s_f.ensure(3 * n));
  HIPCHK(c, s->s_t.ensure(3 * n)); HIPCHK(c, s->s_sh.ensure(n)); HIPCHK(c, s->s_mask.ensure(n));
  HIPCHK(c, s->walls.d_wout.ensure(4 * nw));
  hipStream_t st = c->stream;
  HIPCHK(c, upload(s->s_x, x, 3 * n, st));
  HIPCHK(c, upload(s->s_q, quat, 4 * n, st));
  HIPCHK(c, upload(s->s_sh, shtype, n, st));
  HIPCHK(c, upload(s->s_mask, mask, n, st));
  HIPCHK(c, hipMemsetAsync(s->s_f.p, 0, 3 * n * sizeof(double), st));
  HIPCHK(c, hipMemsetAsync(s->s_t.p, 0, 3 * n * sizeof(double), st));
  HIPCHK(c, hipMemsetAsync(s->walls.d_wout.p, 0, 4 * nw * sizeof(double), st));
  RC(shstep_wall_force_device(c, nlocal, s->s_x.p, s->s_q.p, s->s_sh.p, s->s_mask.p, groupbit, s->s_f.p, s->s_t.p,
                              wall_out ? s->walls.d_wout.p : nullptr, st));
  std::vector<double> hf(3 * n), ht(3 * n), hw(4 * nw, 0.0);
  HIPCHK(c, download(hf.data(), s->s_f, 3 * n, st));
  HIPCHK(c, download(ht.data(), s->s_t, 3 * n, st));
  if (wall_out) HIPCHK(c, download(hw.data(), s->walls.d_wout, 4 * nw, st));
  HIPCHK(c, hipStreamSynchronize(st));
  for (size_t k = 0; k < 3 * n; ++k) {
    f[k] += hf[k];
    torque[k] += ht[k];
  }
  if (wall_out)
    for (size_t k = 0; k < 4 * nw; ++k) wall_out[k] += hw[k];
  return shpair_check_device_errors(c, st);
}

int shstep_get_wall_stats(shpair_ctx* c, int* ncontacts)
{
  STEP_PROLOGUE(c);
  if (!ncontacts) CTX_FAIL(c, SHPAIR_EINVAL, "null output pointer");
  *ncontacts = 0;
  if (!s->walls.wall_called) return SHPAIR_OK;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(s->h_flags + 3, s->walls.work.count.p + 1, sizeof(int), hipMemcpyDeviceToHost));
  *ncontacts = s->h_flags[3];
  return shpair_check_device_errors(c, c->stream);
}

}  // extern "C"
