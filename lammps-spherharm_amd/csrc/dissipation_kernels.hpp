// dissipation_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.10 and §2.11: volume-rate contact damping and
// Coulomb-capped viscous friction of SH pairs.
//
// Both wrenches need nothing the contact kernels do not already leave behind: the per-slot integrals V, S_n[3], T_n[3]
// (space frame, the `pair_out` rows their epilogues store), the two atoms' twists, d = x_j - x_i and, for friction, the
// bounding radii.  Streaming passes, one lane per row / per list slot, bound by HBM:
//   twist_kernel      (w, omega) of every row: w = v - omega x s is the velocity of the SH origin (what x moves with),
//                     omega = R Iinv R^T L.  A ghost row of a device-built border takes its OWNER's inputs (images move
//                     with their owners and a twist is translation-invariant), so one launch serves owned and ghost rows
//                     and a ghost's six numbers are its owner's bit for bit.
//   pair_damp_kernel  Vdot = S_n.(w_i - w_j) + T_n.omega_i - (T_n - d x S_n).omega_j,  delta = max(-p, gamma_ij Vdot)
//                     (p_tot = max(0, p + gamma Vdot), delta = p_tot - p),  F_i -= delta S_n, tau_i -= delta T_n,
//                     F_j += delta S_n, tau_j += delta (T_n - d x S_n).  No contact point, normalisation, sqrt or
//                     division; pow only where the exponent is not 1 (the clamp needs p).
//   pair_dissipation_kernel   the same delta (0 where gamma_ij is 0), then the history-free friction of LAMMPS
//                     gran/hooke: F_t = -kappa v_t with kappa = gamma_t while gamma_t |v_t| <= mu N, mu N / |v_t|
//                     beyond.  The contact point is the point of the normal wrench's line of action (through
//                     r_perp = S_n x T_n / |S_n|^2, along S_n) nearest the radical plane of the two bounding spheres;
//                     both bodies take the force there, so momentum and angular momentum are conserved exactly.  One
//                     division by q = |S_n|^2, one square root for N = p_tot |S_n|, one for |v_t|; no unit vector is
//                     formed, so v_t = 0 gives exactly zero.  F_i = -delta S_n + F_t, tau_i = -delta T_n + r_i x F_t,
//                     F_j = -F_i, tau_j = delta (T_n - d x S_n) - r_j x F_t.
// The two pair kernels are one slot body (pair_slot) with friction as a compile-time switch; the library launches the
// second only while a friction coefficient is set.  Scatter: the FP64 hardware atomics of the pair path, or —
// deterministic mode — one 12-double row per slot (zeros for a slot that adds nothing) for det_gather_kernel, which adds
// every atom's rows in list order.  The tangential spring of §2.14 is the body's HIST switch, for the two entry points
// of history_kernels.hpp.  p, the capped coefficient and the ledger share are contact_laws.hpp's, shared with the
// rolling pass.
// Included by shstep_dissipation.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "contact_laws.hpp"
#include "rigid_body.hpp"

namespace shp {

constexpr int kDampBlock = 256;

__global__ __launch_bounds__(kDampBlock) void twist_kernel(const int nlocal, const int nghost, const double* __restrict__ mass,
                                                           const int nshapes, const double* __restrict__ v,
                                                           const double* __restrict__ quat, const double* __restrict__ angmom,
                                                           const int* __restrict__ shtype, const int* __restrict__ gowner,
                                                           double* __restrict__ twist, int* __restrict__ flags)
{
  const int row = blockIdx.x * kDampBlock + threadIdx.x;
  if (row >= nlocal + nghost) return;
  const int i = row < nlocal ? row : gowner[row - nlocal];   // an owned row: v and angmom have nlocal rows
  double* __restrict__ o = twist + 6 * (size_t)row;
  const int st = (unsigned)i < (unsigned)nlocal ? shtype[i] : -1;
  if ((unsigned)st >= (unsigned)nshapes) {
    atomicOr(flags, kErrShape);
    for (int k = 0; k < 6; ++k) o[k] = 0.0;
    return;
  }
  const double* __restrict__ mr = mass + (size_t)kMassStride * st;
  const Mat3 R = rot_of(quat[4 * i], quat[4 * i + 1], quat[4 * i + 2], quat[4 * i + 3]);
  const double L[3] = {angmom[3 * i], angmom[3 * i + 1], angmom[3 * i + 2]};
  double w[3], s[3];
  omega_of(R, mr, L, w);
  for (int k = 0; k < 3; ++k) s[k] = R.m[k][0] * mr[2] + R.m[k][1] * mr[3] + R.m[k][2] * mr[4];
  o[0] = v[3 * i] - (w[1] * s[2] - w[2] * s[1]);
  o[1] = v[3 * i + 1] - (w[2] * s[0] - w[0] * s[2]);
  o[2] = v[3 * i + 2] - (w[0] * s[1] - w[1] * s[0]);
  o[3] = w[0]; o[4] = w[1]; o[5] = w[2];
}

struct DampParams {
  int npairs, nlocal, nall, newton_pair, ntypes;
  int needv;               // the contact kernel of these integrals had the volume path: V > 0 decides "touched"
  const int* pair_i;
  const int* pair_j;
  const double* integrals;   // 7 doubles per slot: V, S_n, T_n
  const double* x;
  const int* type;
  const double* twist;       // 6 doubles per row
  const double* gamma;       // (ntypes+1)^2, like kn / expo
  const double* kn;
  const double* expo;
  double* f;
  double* torque;
  double* pair_ft;           // deterministic mode: 12 doubles per slot, written instead of the atomics; else null
  double* power;             // the LEDGER instances only (SPEC §2.13): 2 doubles per slot, share P_d, share P_f
};

struct FrictionParams {
  DampParams d;            // gamma may be null: no damping coefficient was ever set
  int nshapes;
  const int* shtype;
  const double* rmax;      // [nshapes] bounding radii
  const double* mu;        // (ntypes+1)^2, like gamma
  const double* gamma_t;
};

// One list slot of the pair pass; p, the capped coefficient and the ledger share are contact_laws.hpp's.  FRIC: the
// friction block is compiled in and reads Q's tables; else Q is not read.
// (Both structs by value: their fields stay kernel arguments to the optimiser, as in a kernel that holds this text.)
// LEDGER (SPEC §2.13): every slot also leaves its dissipated power, P_d = delta Vdot and P_f = kappa |v_t|^2 from the
// numbers the wrench was formed with, times the slot's share of the energy tally; zeros for a slot that adds nothing.
// Instances of their own, launched only while the energy ledger is on.
// HIST (with FRIC; SPEC §2.14, history_kernels.hpp): H is that header's HistoryParams, and a type pair with mu != 0 and
// k_t != 0 takes the tangential spring in place of kappa.  mu and gamma_t may then be null tables, and the slot index
// is a size_t where the other instances count in int.  Without HIST, H is the empty NoHistory and is not read.
struct NoHistory {};

template <bool FRIC, bool LEDGER = false, bool HIST = false, typename History = NoHistory>
__device__ __forceinline__ void pair_slot(const DampParams P, const FrictionParams Q, const History H = History{})
{
  using index_t = std::conditional_t<HIST, size_t, int>;
  const index_t w = (index_t)blockIdx.x * kDampBlock + threadIdx.x;
  if (w >= (index_t)P.npairs) return;
  double Fi[3] = {0.0, 0.0, 0.0}, Ti[3] = {0.0, 0.0, 0.0}, Tj[3] = {0.0, 0.0, 0.0};
  double xn[3] = {0.0, 0.0, 0.0};   // HIST only: what xi becomes, zero unless the slot advances its spring below
  double Pd = 0.0, Pf = 0.0;        // LEDGER only
  bool act = false, applyj = false;
  const int i = P.pair_i[w], j = P.pair_j[w];
  const double* __restrict__ io = P.integrals + 7 * (size_t)w;
  const double V = io[0];
  const double S[3] = {io[1], io[2], io[3]};
  const bool touched = V > 0.0 || (!P.needv && (S[0] != 0.0 || S[1] != 0.0 || S[2] != 0.0));
  if (touched && (unsigned)i < (unsigned)P.nall && (unsigned)j < (unsigned)P.nall) {
    const int ti = P.type[i], tj = P.type[j];
    if (ti >= 1 && ti <= P.ntypes && tj >= 1 && tj <= P.ntypes) {   // (the set-up kernel reported a type out of range)
      const int tt = ti * (P.ntypes + 1) + tj;
      double g, mu = 0.0, gt = 0.0, kt = 0.0;
      if constexpr (HIST) {
        g = P.gamma ? P.gamma[tt] : 0.0;
        mu = Q.mu ? Q.mu[tt] : 0.0;
        gt = Q.gamma_t ? Q.gamma_t[tt] : 0.0;
        kt = H.kt[tt];
      } else if constexpr (FRIC) {
        g = P.gamma ? P.gamma[tt] : 0.0;
        mu = Q.mu[tt];
        gt = Q.gamma_t[tt];
      } else {
        g = P.gamma[tt];
      }
      const bool hist = HIST && mu != 0.0 && kt != 0.0;   // gamma_t may then be 0
      const bool fric = hist || (mu != 0.0 && gt != 0.0);
      if (g != 0.0 || fric) {
        const double T[3] = {io[4], io[5], io[6]};
        const double p = pair_pressure(P.kn[tt], P.expo[tt], V);
        const double d[3] = {P.x[3 * (index_t)j] - P.x[3 * (index_t)i], P.x[3 * (index_t)j + 1] - P.x[3 * (index_t)i + 1],
                             P.x[3 * (index_t)j + 2] - P.x[3 * (index_t)i + 2]};
        // (the arm and Vdot below are also rolling_slot's text, rolling_kernels.hpp: change both)
        const double A[3] = {T[0] - (d[1] * S[2] - d[2] * S[1]), T[1] - (d[2] * S[0] - d[0] * S[2]),
                             T[2] - (d[0] * S[1] - d[1] * S[0])};
        const double* __restrict__ ti6 = P.twist + 6 * (size_t)i;
        const double* __restrict__ tj6 = P.twist + 6 * (size_t)j;
        double delta = 0.0;
        if (g != 0.0) {
          double vd = 0.0;
          for (int k = 0; k < 3; ++k) vd = fma(S[k], ti6[k] - tj6[k], vd);
          for (int k = 0; k < 3; ++k) vd = fma(T[k], ti6[3 + k], vd);
          for (int k = 0; k < 3; ++k) vd = fma(-A[k], tj6[3 + k], vd);
          delta = fmax(-p, g * vd);   // p_tot - p with p_tot = max(0, p + gamma Vdot): a contact never pulls
          if constexpr (LEDGER) Pd = delta * vd;   // gamma Vdot^2, or p |Vdot| for a clamped contact
        }
        for (int k = 0; k < 3; ++k) {
          Fi[k] = -delta * S[k];
          Ti[k] = -delta * T[k];
          Tj[k] = delta * A[k];
        }
        act = delta != 0.0;
        if constexpr (FRIC) {
          const double q = S[0] * S[0] + S[1] * S[1] + S[2] * S[2];
          const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
          const double N = (p + delta) * sqrt(q);   // p_tot |S_n|: 0 for a clamped contact
          const int si = Q.shtype[i], sj = Q.shtype[j];
          // (a shape index out of range was reported by the set-up kernel of the compute)
          // N > 0: a clamped contact has no friction and loses its spring (§2.14).  The HIST instances ask it of a history
          // slot only: their slot without history goes on with cap = 0, which gives F_t = 0, and then issues atomics of
          // zeros where the FRIC instances issue none.  Kept as it is: one guard for both would change what they do.
          if (fric && q > 0.0 && dd > 0.0 && (HIST ? (!hist || N > 0.0) : N > 0.0) && (unsigned)si < (unsigned)Q.nshapes &&
              (unsigned)sj < (unsigned)Q.nshapes) {
            const double qi = 1.0 / q;
            const double Ri = Q.rmax[si], Rj = Q.rmax[sj];
            const double t = 0.5 * (1.0 + (Ri * Ri - Rj * Rj) / dd);
            const double ds = t * (d[0] * S[0] + d[1] * S[1] + d[2] * S[2]);
            // r_i = (S x T + t (d.S) S) / q: the contact point from x_i;  r_j = r_i - d
            const double ri[3] = {(S[1] * T[2] - S[2] * T[1] + ds * S[0]) * qi, (S[2] * T[0] - S[0] * T[2] + ds * S[1]) * qi,
                                  (S[0] * T[1] - S[1] * T[0] + ds * S[2]) * qi};
            const double rj[3] = {ri[0] - d[0], ri[1] - d[1], ri[2] - d[2]};
            const double* oi = ti6 + 3;
            const double* oj = tj6 + 3;
            const double vr[3] = {(ti6[0] + (oi[1] * ri[2] - oi[2] * ri[1])) - (tj6[0] + (oj[1] * rj[2] - oj[2] * rj[1])),
                                  (ti6[1] + (oi[2] * ri[0] - oi[0] * ri[2])) - (tj6[1] + (oj[2] * rj[0] - oj[0] * rj[2])),
                                  (ti6[2] + (oi[0] * ri[1] - oi[1] * ri[0])) - (tj6[2] + (oj[0] * rj[1] - oj[1] * rj[0]))};
            const double vn = (vr[0] * S[0] + vr[1] * S[1] + vr[2] * S[2]) * qi;
            const double vt[3] = {vr[0] - vn * S[0], vr[1] - vn * S[1], vr[2] - vn * S[2]};
            double Ft[3];
            double vtn = 0.0, kappa = 0.0;   // of the viscous branch
            if (hist) {
              if constexpr (HIST) {
                const double cap = mu * N;
                // advance, then take off what the turning normal has put along S_n
                double xp[3] = {H.xi[w] + H.dt * vt[0], H.xi[H.stride + w] + H.dt * vt[1], H.xi[2 * H.stride + w] + H.dt * vt[2]};
                const double xs = (xp[0] * S[0] + xp[1] * S[1] + xp[2] * S[2]) * qi;
                for (int k = 0; k < 3; ++k) xp[k] -= xs * S[k];
                const double Fs[3] = {-kt * xp[0] - gt * vt[0], -kt * xp[1] - gt * vt[1], -kt * xp[2] - gt * vt[2]};
                const double fn = sqrt(Fs[0] * Fs[0] + Fs[1] * Fs[1] + Fs[2] * Fs[2]);
                if (fn <= cap) {   // sticks
                  for (int k = 0; k < 3; ++k) {
                    Ft[k] = Fs[k];
                    xn[k] = xp[k];
                  }
                } else {           // slides: the spring keeps what the capped force can hold
                  const double sc = cap / fn;
                  for (int k = 0; k < 3; ++k) {
                    Ft[k] = Fs[k] * sc;
                    xn[k] = -(Ft[k] + gt * vt[k]) / kt;
                  }
                }
                act = act || Ft[0] != 0.0 || Ft[1] != 0.0 || Ft[2] != 0.0;   // a spring at rest still pushes
                if constexpr (LEDGER) Pf = -(Ft[0] * vt[0] + Ft[1] * vt[1] + Ft[2] * vt[2]);   // negative while it unloads
              }
            } else {
              vtn = sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
              kappa = capped_coefficient(gt, vtn, mu * N);
              Ft[0] = -kappa * vt[0]; Ft[1] = -kappa * vt[1]; Ft[2] = -kappa * vt[2];
              // The tally of the viscous branch stands here in the HIST instances and behind the wrench in the others,
              // as in the two bodies this one replaces: the order decides the instruction schedule of either family.
              if constexpr (HIST) {
                act = act || vtn != 0.0;
                if constexpr (LEDGER) Pf = kappa * (vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
              }
            }
            Fi[0] += Ft[0]; Fi[1] += Ft[1]; Fi[2] += Ft[2];
            Ti[0] += ri[1] * Ft[2] - ri[2] * Ft[1];
            Ti[1] += ri[2] * Ft[0] - ri[0] * Ft[2];
            Ti[2] += ri[0] * Ft[1] - ri[1] * Ft[0];
            Tj[0] -= rj[1] * Ft[2] - rj[2] * Ft[1];
            Tj[1] -= rj[2] * Ft[0] - rj[0] * Ft[2];
            Tj[2] -= rj[0] * Ft[1] - rj[1] * Ft[0];
            if constexpr (!HIST) {
              act = act || vtn != 0.0;
              if constexpr (LEDGER) Pf = kappa * (vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
            }
          }
        }
        applyj = P.newton_pair || j < P.nlocal;
      }
    }
  }
  if constexpr (HIST) {
    if (H.dt > 0.0) {   // a step: every slot writes its xi (zero for one without a live spring)
      H.xi[w] = xn[0];
      H.xi[H.stride + w] = xn[1];
      H.xi[2 * H.stride + w] = xn[2];
    }
  }
  if constexpr (LEDGER) {   // every slot writes its row: the fold reads all of them
    const double share = ledger_share(P.newton_pair, j, P.nlocal);
    P.power[2 * (size_t)w] = share * Pd;
    P.power[2 * (size_t)w + 1] = share * Pf;
  }
  if (P.pair_ft) {   // every slot writes its row: the gather reads all of them
    double* __restrict__ o = P.pair_ft + 12 * (size_t)w;
    for (int k = 0; k < 3; ++k) {
      o[k] = Fi[k];
      o[3 + k] = Ti[k];
      o[6 + k] = applyj ? -Fi[k] : 0.0;
      o[9 + k] = applyj ? Tj[k] : 0.0;
    }
    return;
  }
  if (!act) return;
  for (int k = 0; k < 3; ++k) {
    atomicAdd(P.f + 3 * (size_t)i + k, Fi[k]);
    atomicAdd(P.torque + 3 * (size_t)i + k, Ti[k]);
  }
  if (applyj)
    for (int k = 0; k < 3; ++k) {
      atomicAdd(P.f + 3 * (size_t)j + k, -Fi[k]);
      atomicAdd(P.torque + 3 * (size_t)j + k, Tj[k]);
    }
}

__global__ __launch_bounds__(kDampBlock) void pair_damp_kernel(const DampParams P)
{
  pair_slot<false>(P, FrictionParams{});
}

__global__ __launch_bounds__(kDampBlock) void pair_dissipation_kernel(const FrictionParams Q)
{
  pair_slot<true>(Q.d, Q);
}

// ... and the two that also leave the power rows of the energy ledger (SPEC §2.13), launched only while it is on
__global__ __launch_bounds__(kDampBlock) void pair_damp_ledger_kernel(const DampParams P)
{
  pair_slot<false, true>(P, FrictionParams{});
}

__global__ __launch_bounds__(kDampBlock) void pair_dissipation_ledger_kernel(const FrictionParams Q)
{
  pair_slot<true, true>(Q.d, Q);
}

}  // namespace shp
