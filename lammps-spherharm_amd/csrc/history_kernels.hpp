// history_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.14: tangential contact springs with history for SH pairs.
//
// Every slot of a device-built list owns xi, the accumulated tangential displacement of i's contact point relative to
// j's (space frame).  Three kernels:
//   pair_history_kernel        the pair pass of dissipation_kernels.hpp (pair_slot with friction) with the spring: a
//   pair_history_ledger_kernel sibling body, history_slot, so that the four kernels there stay what they are.  A type
//                              pair has history iff mu_ij != 0 and k_t,ij != 0; the other type pairs take §2.11's
//                              friction as pair_slot forms it.  For a history slot that passes §2.11's guards:
//                                xi' = xi + dt v_t, less its part along S_n;  F* = -k_t xi' - gamma_t v_t;
//                                |F*| <= mu N: F_t = F*, xi <- xi';  else F_t = F* mu N / |F*|, xi <- -(F_t + gamma_t v_t) / k_t
//                              and the wrench of F_t at r_i on both bodies, as §2.11's.  Every other slot gets xi <- 0.
//                              dt = 0 forms the force from the stored xi and writes nothing back.  One lane per slot,
//                              one owner per xi: no atomics on it.
//   history_key_kernel         after a build: one int per slot, the tag of j's owner (what survives a rebuild; the
//                              list is built with tag_i < tag_j, so i never swaps with j)
//   history_carry_kernel       one lane per NEW slot (i, key): scans the OLD row i for the key, copies its xi or writes 0
// xi is three planes of `stride` doubles (stride = the list's slot count): the 64 lanes of a wave load 64 consecutive
// doubles of a plane, one 512 B request each, where [slot][3] would stride the lanes by 24 B.
// Streaming kernels bound by HBM.  Included by shstep_dissipation.hip only, behind dissipation_kernels.hpp (the
// kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "dissipation_kernels.hpp"

namespace shp {

struct HistoryParams {
  FrictionParams q;        // q.d.gamma, q.mu and q.gamma_t may be null: no coefficient of the kind was ever set
  const double* kt;        // (ntypes+1)^2, like mu
  double* xi;              // [3][stride]
  size_t stride;
  double dt;               // 0: a look, xi is not written
};

template <bool LEDGER>
__device__ __forceinline__ void history_slot(const HistoryParams H)
{
  const DampParams& P = H.q.d;
  const FrictionParams& Q = H.q;
  const size_t w = (size_t)blockIdx.x * kDampBlock + threadIdx.x;
  if (w >= (size_t)P.npairs) return;
  double Fi[3] = {0.0, 0.0, 0.0}, Ti[3] = {0.0, 0.0, 0.0}, Tj[3] = {0.0, 0.0, 0.0};
  double xn[3] = {0.0, 0.0, 0.0};   // what xi becomes: zero unless the slot advances its spring below
  double Pd = 0.0, Pf = 0.0;        // LEDGER only
  bool act = false, applyj = false;
  const int i = P.pair_i[w], j = P.pair_j[w];
  const double* __restrict__ io = P.integrals + 7 * w;
  const double V = io[0];
  const double S[3] = {io[1], io[2], io[3]};
  // touched, as the contact kernels' epilogue decides it
  const bool touched = V > 0.0 || (!P.needv && (S[0] != 0.0 || S[1] != 0.0 || S[2] != 0.0));
  if (touched && (unsigned)i < (unsigned)P.nall && (unsigned)j < (unsigned)P.nall) {
    const int ti = P.type[i], tj = P.type[j];
    if (ti >= 1 && ti <= P.ntypes && tj >= 1 && tj <= P.ntypes) {   // (the set-up kernel reported a type out of range)
      const int tt = ti * (P.ntypes + 1) + tj;
      const double g = P.gamma ? P.gamma[tt] : 0.0;
      const double mu = Q.mu ? Q.mu[tt] : 0.0;
      const double gt = Q.gamma_t ? Q.gamma_t[tt] : 0.0;
      const double kt = H.kt[tt];
      const bool hist = mu != 0.0 && kt != 0.0;          // gamma_t may then be 0
      const bool fric = hist || (mu != 0.0 && gt != 0.0);
      if (g != 0.0 || fric) {
        const double T[3] = {io[4], io[5], io[6]};
        const double kn = P.kn[tt], m = P.expo[tt];
        const double p = (m == 1.0 || !(V > 0.0)) ? kn : kn * m * pow(V, m - 1.0);
        const double d[3] = {P.x[3 * (size_t)j] - P.x[3 * (size_t)i], P.x[3 * (size_t)j + 1] - P.x[3 * (size_t)i + 1],
                             P.x[3 * (size_t)j + 2] - P.x[3 * (size_t)i + 2]};
        // the arm of particle j: A = T_n - d x S_n
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
          if constexpr (LEDGER) Pd = delta * vd;
        }
        for (int k = 0; k < 3; ++k) {
          Fi[k] = -delta * S[k];
          Ti[k] = -delta * T[k];
          Tj[k] = delta * A[k];
        }
        act = delta != 0.0;
        const double q = S[0] * S[0] + S[1] * S[1] + S[2] * S[2];
        const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const double N = (p + delta) * sqrt(q);   // p_tot |S_n|: 0 for a clamped contact
        const int si = Q.shtype[i], sj = Q.shtype[j];
        // §2.11's guards, and for a history slot N > 0 (§2.14: a clamped contact loses its spring; without history the
        // slot goes on as in pair_slot, where cap = 0 gives F_t = 0); a history slot that fails one keeps xn = 0
        if (fric && q > 0.0 && dd > 0.0 && (!hist || N > 0.0) && (unsigned)si < (unsigned)Q.nshapes &&
            (unsigned)sj < (unsigned)Q.nshapes) {
          const double Ri = Q.rmax[si], Rj = Q.rmax[sj];
          const double qi = 1.0 / q;
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
          const double cap = mu * N;
          double Ft[3];
          if (hist) {
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
          } else {
            const double vtn = sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
            const double kappa = gt * vtn <= cap ? gt : cap / vtn;   // vtn = 0 takes the first branch
            Ft[0] = -kappa * vt[0]; Ft[1] = -kappa * vt[1]; Ft[2] = -kappa * vt[2];
            act = act || vtn != 0.0;
            if constexpr (LEDGER) Pf = kappa * (vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
          }
          Fi[0] += Ft[0]; Fi[1] += Ft[1]; Fi[2] += Ft[2];
          Ti[0] += ri[1] * Ft[2] - ri[2] * Ft[1];
          Ti[1] += ri[2] * Ft[0] - ri[0] * Ft[2];
          Ti[2] += ri[0] * Ft[1] - ri[1] * Ft[0];
          Tj[0] -= rj[1] * Ft[2] - rj[2] * Ft[1];
          Tj[1] -= rj[2] * Ft[0] - rj[0] * Ft[2];
          Tj[2] -= rj[0] * Ft[1] - rj[1] * Ft[0];
        }
        applyj = P.newton_pair || j < P.nlocal;
      }
    }
  }
  if (H.dt > 0.0) {   // a step: every slot writes its xi (zero for one without a live spring)
    H.xi[w] = xn[0];
    H.xi[H.stride + w] = xn[1];
    H.xi[2 * H.stride + w] = xn[2];
  }
  if constexpr (LEDGER) {   // every slot writes its row: the fold reads all of them
    const double share = P.newton_pair ? 1.0 : (0.5 + (j < P.nlocal ? 0.5 : 0.0));
    P.power[2 * w] = share * Pd;
    P.power[2 * w + 1] = share * Pf;
  }
  if (P.pair_ft) {   // every slot writes its row: the gather reads all of them
    double* __restrict__ o = P.pair_ft + 12 * w;
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

__global__ __launch_bounds__(kDampBlock) void pair_history_kernel(const HistoryParams H)
{
  history_slot<false>(H);
}

__global__ __launch_bounds__(kDampBlock) void pair_history_ledger_kernel(const HistoryParams H)
{
  history_slot<true>(H);
}

// key[w] = the tag of j's owner.  With tags, a ghost row holds its owner's (shstep_borders_device copies it, and a
// host's own ghost rows carry theirs); without, the tag is the row index and a ghost's owner is in gowner — the two
// cases of half_list_kernel, which built the list from the same arrays.
__global__ __launch_bounds__(kDampBlock) void history_key_kernel(const int np, const int nlocal, const int* __restrict__ pair_j,
                                                                 const int* __restrict__ tag, const int* __restrict__ gowner,
                                                                 int* __restrict__ key)
{
  const size_t w = (size_t)blockIdx.x * kDampBlock + threadIdx.x;
  if (w >= (size_t)np) return;
  const int j = pair_j[w];
  key[w] = tag ? tag[j] : (j < nlocal ? j : gowner[j - nlocal]);
}

// Rows are a dozen entries: a linear scan of the old row.  A periodic edge is at least twice the ghost cutoff (SPEC
// §7), so a row holds an owner's tag at most once.
__global__ __launch_bounds__(kDampBlock) void history_carry_kernel(const int np, const int* __restrict__ pair_i,
                                                                   const int* __restrict__ key, const int* __restrict__ old_offs,
                                                                   const int* __restrict__ old_key, const double* __restrict__ old_xi,
                                                                   const size_t old_stride, double* __restrict__ xi, const size_t stride)
{
  const size_t w = (size_t)blockIdx.x * kDampBlock + threadIdx.x;
  if (w >= (size_t)np) return;
  const int i = pair_i[w], k = key[w];
  double a[3] = {0.0, 0.0, 0.0};
  for (int p = old_offs[i], e = old_offs[i + 1]; p < e; ++p)
    if (old_key[p] == k) {
      a[0] = old_xi[p];
      a[1] = old_xi[old_stride + p];
      a[2] = old_xi[2 * old_stride + p];
      break;
    }
  xi[w] = a[0];
  xi[stride + w] = a[1];
  xi[2 * stride + w] = a[2];
}

}  // namespace shp
