// shell_host.hpp — the host layer of the two axial shell families, cylindrical (docs/SPEC.md §2.18–§2.21) and conical
// (§2.22–§2.24) container walls, once for both: the geometry setter's upload, the one place that installs a record of
// coefficients, the one body of the seven coefficient setters, the read-backs, the history calls and the pass.  The state is
// ShellState (shstep_state.hpp); the check of a setter, the record and its switches are surface_coefficients.hpp's; the
// work buffers, the spring history and the common kernel arguments are surface_state.hpp's.
//
// Function templates over a family description F, which each of the two .hip files writes for itself:
//   State, state(s)            CylState / ConeState, and where it hangs in the step state
//   kind                       the SurfaceKind: the family's noun, plural and geometry setter in a message
//   kIn, kStride               doubles per surface as the caller passes them (7 or 8), and as the device holds them (kn and
//                              the exponent behind them)
//   kRow, kBlock, kMaxBlocks   the row width, the block of every kernel of the pass, the cap of the contact kernel's grid
//   spring_setter, contact_call, roll_null_twist()   the other words of its messages
//   Params, SpringParams, RollParams                 its kernel-argument structs
//   candidates, live_sweep, rows_partial, rows_final  its kernels of the pass that have one instance
//   size_buffers               its step_size_*_buffers (the cylinders size the power rows of §2.20 on top of size_shell_buffers)
// and the two hooks, the only code of a family inside the shared bodies:
//   refuse(c, s, what, r, on)  what the ledgers forbid of a record about to be installed: called before anything is
//                              uploaded, so that a refusal leaves the state as it was
//   launch_contact(...), launch_roll(...)   the choice among the family's instances of the contact kernel, and of the
//                              roll kernel behind it; ShellLedgerUse is what the first tells the second (and the caller)
//                              of the LEDGER twins, which only the cylinders have
// Per pass the stream sees what it always saw: the count's memset, candidates, the live sweep of an advancing pass, the
// contact instance, the roll kernel while a surface has a kind, the two row-total kernels when totals are asked for.
//
// Included by shstep_cylinders.hip and shstep_cones.hip only, behind their kernel headers.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "ring_tables.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"

namespace shp {

struct ShellLedgerUse {
  bool ledger = false;   // both ledgers are on: the roll kernel is its LEDGER twin
  bool power = false;    // ... and a LEDGER instance of the contact kernel wrote the power rows of this pass
};

// the work buffers and the history of a pass over nlocal particles (a law that takes its normal load from the rows keeps
// them whoever asks for totals)
template <typename F>
int size_shell_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out)
{
  typename F::State& st = F::state(s);
  HIPCHK(c, st.work.ensure(nlocal, st.n, F::kRow, want_out || st.on.roll, F::kBlock));
  if (st.on.hist) HIPCHK(c, st.hist.size(nlocal, st.n));
  return SHPAIR_OK;
}

template <typename F>
int bind_shell_history(shpair_ctx* c, shstep_state* s, int nlocal)
{
  typename F::State& st = F::state(s);
  if (!st.on.hist || nlocal <= 0 || st.hist.nlocal == nlocal) return SHPAIR_OK;
  RC(F::size_buffers(c, s, nlocal, false));
  return st.hist.bind(c, nlocal);
}

// The geometry setter behind the family's argument check: the device's image of the surfaces, every coefficient and Omega
// 0 again, and the history gone with k_t.
template <typename F>
int set_shell_geometry(shpair_ctx* c, shstep_state* s, int n, const double* in, const double* kn, const double* exponent)
{
  static_assert(F::kStride == F::kIn + 2, "a surface is the doubles of its setter, kn and the exponent");
  typename F::State& st = F::state(s);
  std::vector<double> h((size_t)F::kStride * (size_t)n);
  for (int k = 0; k < n; ++k) {
    double* r = &h[(size_t)F::kStride * k];
    for (int j = 0; j < F::kIn; ++j) r[j] = in[F::kIn * k + j];
    r[F::kIn] = kn[k]; r[F::kIn + 1] = exponent[k];
  }
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still read the old tables
  if (n > 0) {   // (no surface: nothing is allocated)
    HIPCHK(c, st.d_surf.ensure(h.size()));
    HIPCHK(c, hipMemcpy(st.d_surf.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, st.d_coef.ensure((size_t)4 * n));
    HIPCHK(c, hipMemset(st.d_coef.p, 0, (size_t)4 * n * sizeof(double)));
  }
  st.h_surf = h;
  st.coef.reset(n);
  st.on = SurfaceSwitches{};
  st.hist.nlocal = -1;
  st.n = n;
  st.called = false;
  return SHPAIR_OK;
}

// The one place that turns a record of a family's coefficients, a copy of the state's with a setter's tables written into
// it, into the device tables ([4][n]: gamma, mu, gamma_t, Omega; [n]: k_t; [4][n]: mu_r, gamma_r, mu_tw, gamma_tw, which
// the roll kernels alone read) and the switches (derive_surface_switches has the rules).  Nothing is allocated for the
// springs while no surface has one and none had, nor for the rolling table; a change of hist drops the history.
template <typename F>
int install_shell_coefficients(shpair_ctx* c, shstep_state* s, const char* what, const SurfaceCoefficients& r)
{
  typename F::State& st = F::state(s);
  const SurfaceSwitches on = derive_surface_switches(r), was = st.on;
  RC(F::refuse(c, s, what, r, on));
  const std::vector<double> h = pack_surface_tables({&r.gamma, &r.mu, &r.gamma_t, &r.Omega});
  HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still read the old table
  HIPCHK(c, hipMemcpy(st.d_coef.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));   // (the geometry setter sized it)
  if (on.hist || was.hist) {   // (the HIST instance is the only reader)
    HIPCHK(c, st.d_kt.ensure(r.k_t.size()));
    HIPCHK(c, hipMemcpy(st.d_kt.p, r.k_t.data(), r.k_t.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (on.roll || was.roll) {
    const std::vector<double> hr = pack_surface_tables({&r.mu_r, &r.gamma_r, &r.mu_tw, &r.gamma_tw});
    HIPCHK(c, st.d_roll.ensure(hr.size()));
    HIPCHK(c, hipMemcpy(st.d_roll.p, hr.data(), hr.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  st.coef = r;
  st.on = on;
  if (on.hist != was.hist) st.hist.nlocal = -1;
  return SHPAIR_OK;
}

// The one body of the coefficient setters: t says which (surface_coefficients.hpp), t0 and t1 are its tables as passed.
template <typename F>
int set_shell_coefficients(shpair_ctx* c, shstep_state* s, const SurfaceSetter& t, int n, const double* t0, const double* t1 = nullptr)
{
  typename F::State& st = F::state(s);
  const double* tabs[2] = {t0, t1};
  const std::string bad = check_surface_setter(F::kind, t, n, st.n, tabs);
  if (!bad.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "%s", bad.c_str());
  if (n == 0) return SHPAIR_OK;
  SurfaceCoefficients r = st.coef;
  for (int k = 0; k < t.ntab; ++k) (r.*t.tabs[k]).assign(tabs[k], tabs[k] + n);
  return install_shell_coefficients<F>(c, s, t.what, r);
}

// The geometry never moves: the host copy is what the device holds.
template <typename F>
int get_shell_geometry(shpair_ctx* c, shstep_state* s, int n, double* out)
{
  typename F::State& st = F::state(s);
  if (n != st.n) CTX_FAIL(c, SHPAIR_EINVAL, "get %s: room for %d %s, %d are set", F::kind.plural, n, F::kind.plural, st.n);
  if (n == 0) return SHPAIR_OK;
  if (!out) CTX_FAIL(c, SHPAIR_EINVAL, "get %s: null output pointer", F::kind.plural);
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < F::kIn; ++j) out[F::kIn * k + j] = st.h_surf[(size_t)F::kStride * k + j];
  return SHPAIR_OK;
}

template <typename F>
int get_shell_stats(shpair_ctx* c, shstep_state* s, int* ncontacts)
{
  typename F::State& st = F::state(s);
  if (!ncontacts) CTX_FAIL(c, SHPAIR_EINVAL, "null output pointer");
  *ncontacts = 0;
  if (!st.called) return SHPAIR_OK;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(ncontacts, st.work.count.p + 1, sizeof(int), hipMemcpyDeviceToHost));
  return shpair_check_device_errors(c, c->stream);
}

// xi of the family's springs to / from the host, [nlocal][n][W], 0 where the bit is dead
template <typename F>
int copy_shell_history(shpair_ctx* c, shstep_state* s, int nlocal, double* xi_out)
{
  typename F::State& st = F::state(s);
  return st.hist.copy_out(c, F::kind.noun, F::spring_setter, st.on.hist, nlocal, st.n, xi_out);
}

template <typename F>
int set_shell_history(shpair_ctx* c, shstep_state* s, int nlocal, const double* xi)
{
  typename F::State& st = F::state(s);
  return st.hist.set_from_host(c, s, F::kind.noun, F::spring_setter, st.on.hist, nlocal, st.n, xi, F::size_buffers);
}

// The pass behind both forms of a family's call: without a time step (no spring set: refused otherwise, dt is not looked
// at) and with one.  use: what the contact-launch hook chose of the LEDGER twins (nothing where nothing was launched).
template <typename F>
int shell_pass(shpair_ctx* c, shstep_state* s, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
               int groupbit, double* f, double* torque, double* out, const double* twist, double dt, void* stream,
               ShellLedgerUse* use = nullptr)
{
  if (nlocal < 0) CTX_FAIL(c, SHPAIR_EINVAL, "nlocal %d < 0", nlocal);
  typename F::State& st = F::state(s);
  if (st.n == 0 || nlocal == 0) return SHPAIR_OK;   // no surface: nothing is allocated, zeroed or launched
  if (!x || !quat || !shtype || !mask || !f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  const bool diss = st.on.damp || st.on.fric;   // every coefficient 0: the elastic instance, whatever twist and Omega are
  if (diss && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "%s %s: null twist pointer", F::kind.noun, st.on.damp ? "damping" : "friction");
  const bool hist = st.on.hist;
  if (hist && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "%s tangential spring: null twist pointer", F::kind.noun);
  const bool roll = st.on.roll;
  if (roll && !twist) CTX_FAIL(c, SHPAIR_EINVAL, "%s", F::roll_null_twist());
  if (c->tables_dirty || c->quad_dirty) RC(shpair_prepare_tables(c));
  const bool want_rows = out != nullptr || roll;   // (the roll kernel takes its normal load from them)
  RC(F::size_buffers(c, s, nlocal, want_rows));
  hipStream_t sm = (hipStream_t)stream;
  typename F::Params P{};   // the common kernel arguments, and the coefficient table
  fill_surface_params(P, c, QuadLayout(c->lmax, c->nq), nlocal, st.n, st.d_surf.p, x, quat, shtype, mask, groupbit, f, torque, st.work, want_rows);
  P.coef = st.d_coef.p; P.twist = twist;
  typename F::SpringParams H{};   // (the HIST instance only)
  const bool advance = hist && dt > 0.0;
  if (hist) {
    static_cast<typename F::Params&>(H) = P;
    H.kt = st.d_kt.p; H.xi = st.hist.xi.p; H.live = st.hist.live.p; H.dt = dt;
    RC(st.hist.begin_pass(c, nlocal, advance, sm, &H.live_dead));
  }
  HIPCHK(c, hipMemsetAsync(st.work.count.p, 0, 2 * sizeof(int), sm));
  const unsigned nb = nblk(nlocal, F::kBlock);
  hipLaunchKernelGGL(F::candidates, dim3(nb), dim3(F::kBlock), 0, sm, P);
  if (advance)   // the bits of the surfaces a particle no longer reaches die, whether or not the contact kernel visits it
    hipLaunchKernelGGL(F::live_sweep, dim3(nb), dim3(F::kBlock), 0, sm, nlocal, (const unsigned char*)st.work.mask.p, st.hist.live.p);
  // one wave per queued particle: a grid that covers nlocal, capped; the waves stride over the device-side count
  const unsigned ncb = nblk(nlocal, F::kBlock / 64);
  const dim3 grid(ncb < (unsigned)F::kMaxBlocks ? ncb : (unsigned)F::kMaxBlocks);
  const ShellLedgerUse lu = F::launch_contact(c, st, P, H, diss, hist, grid, sm);
  if (roll) {   // the two couples from the rows the contact kernel just left, one lane per owned row; a look adds them too
    typename F::RollParams Q{};
    Q.nlocal = nlocal; Q.nsurf = st.n;
    Q.smask = st.work.mask.p; Q.x = x; Q.surf = st.d_surf.p; Q.coef = st.d_coef.p; Q.twist = twist; Q.roll = st.d_roll.p;
    Q.rows = st.work.rows.p; Q.torque = torque;
    F::launch_roll(st, Q, lu, nb, sm);
  }
  if (out) {
    hipLaunchKernelGGL(F::rows_partial, dim3(nb, st.n), dim3(F::kBlock), 0, sm, nlocal, st.n, (const unsigned char*)st.work.mask.p,
                       (const double*)st.work.rows.p, st.work.part.p);
    hipLaunchKernelGGL(F::rows_final, dim3(st.n), dim3(F::kBlock), 0, sm, (int)nb, (const double*)st.work.part.p, out);
  }
  HIPCHK(c, hipGetLastError());
  st.called = true;
  if (use) *use = lu;
  return SHPAIR_OK;
}

// the form without a time step, and the one with
template <typename F>
int shell_force_call(shpair_ctx* c, shstep_state* s, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                     int groupbit, double* f, double* torque, double* out, const double* twist, void* stream, ShellLedgerUse* use = nullptr)
{
  if (F::state(s).on.hist)
    CTX_FAIL(c, SHPAIR_EINVAL, "a %s tangential spring is set: the %s pass needs the form with a time step (%s)", F::kind.noun,
             F::kind.noun, F::contact_call);
  return shell_pass<F>(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, out, twist, 0.0, stream, use);
}

template <typename F>
int shell_contact_call(shpair_ctx* c, shstep_state* s, int nlocal, const double* x, const double* quat, const int* shtype, const int* mask,
                       int groupbit, double* f, double* torque, double* out, const double* twist, double dt, void* stream,
                       ShellLedgerUse* use = nullptr)
{
  if (!(dt >= 0.0) || !std::isfinite(dt)) CTX_FAIL(c, SHPAIR_EINVAL, "%s contact: dt %g must be finite and >= 0", F::kind.noun, dt);
  return shell_pass<F>(c, s, nlocal, x, quat, shtype, mask, groupbit, f, torque, out, twist, dt, stream, use);
}

}  // namespace shp
