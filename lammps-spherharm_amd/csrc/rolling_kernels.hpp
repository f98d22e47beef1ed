// rolling_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.16: rolling and twisting resistance of SH pairs.
//
// The two resisting couples act on the relative ANGULAR velocity of a contact, as damping (§2.10) and friction (§2.11)
// act on the relative velocity, and need nothing those do not: the per-slot integrals V, S_n[3], T_n[3] of the last
// compute, the two atoms' twists, d = x_j - x_i (for Vdot only) and the type tables.  One streaming pass of its own over
// the list slots, one lane per slot, bound by HBM, behind whichever pair pass the coefficients ask for (none, damping,
// dissipation, history), which it shares its laws with through contact_laws.hpp and nothing else.
//   rolling_pair_kernel   Omega = omega_i - omega_j,  Omega_n = (Omega.S_n) S_n / q,  Omega_r = Omega - Omega_n  (q = |S_n|^2:
//                     one division, no unit vector, so Omega = 0 gives exactly zero),  N = p_tot |S_n| with the p_tot
//                     of pair_slot (dissipation_kernels.hpp), formed by the same helpers (contact_laws.hpp),
//                     kappa_r = gamma_r while gamma_r |Omega_r| <= mu_r N, mu_r N / |Omega_r| beyond; kappa_tw alike from
//                     gamma_tw, mu_tw, |Omega_n|;  M = -kappa_r Omega_r - kappa_tw Omega_n,  tau_i += M, tau_j -= M.
//                     A pure couple: no force, and no contact point enters.
//   rolling_pair_ledger_kernel   the same, and the power kappa_r |Omega_r|^2 + kappa_tw |Omega_n|^2 times the slot's share
//                     into the friction entry of the slot's power row (SPEC §2.13): added to the row a pair pass of this
//                     step wrote, or written as (0, share P) where none ran.
//   rolling_gather_kernel   deterministic mode: the slots leave one 6-double row each (tau_i, tau_j; zeros for a slot that
//                     adds nothing) instead of the atomics, and this adds every atom's rows in list order through the
//                     reverse index of det_kernels.hpp.  It touches torque only, and only where the sum is not zero, so
//                     f and every zero of torque keep their bits.
// Included by shstep_rolling.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "contact_laws.hpp"

namespace shp {

constexpr int kRollBlock = 256;   // as kDampBlock of the pair pass

struct RollingParams {
  int npairs, nlocal, nall, newton_pair, ntypes;
  int needv;               // the contact kernel of these integrals had the volume path: V > 0 decides "touched"
  int add_power;           // LEDGER: the pair pass has written the power rows from these integrals: add to the friction entry
  const int* pair_i;
  const int* pair_j;
  const double* integrals;   // 7 doubles per slot: V, S_n, T_n
  const double* x;
  const int* type;
  const double* twist;       // 6 doubles per row
  const double* gamma;       // (ntypes+1)^2 like kn / expo; null: no damping coefficient was ever set
  const double* kn;
  const double* expo;
  const double* mu_r;        // the four tables of §2.16, (ntypes+1)^2 each; a kind that was never set: both null
  const double* gamma_r;
  const double* mu_tw;
  const double* gamma_tw;
  double* torque;
  double* rows;              // deterministic mode: 6 doubles per slot, written instead of the atomics; else null
  double* power;             // LEDGER only: 2 doubles per slot, share P_d, share P_f
};

// One list slot.  Touched, the index and type guards, the arm and Vdot are pair_slot's text; p, the two couples and the
// ledger share are contact_laws.hpp's.
template <bool LEDGER>
__device__ __forceinline__ void rolling_slot(const RollingParams P)
{
  const int w = blockIdx.x * kRollBlock + threadIdx.x;
  if (w >= P.npairs) return;
  double M[3] = {0.0, 0.0, 0.0};
  double Pw = 0.0;   // LEDGER only
  bool applyj = false;
  const int i = P.pair_i[w], j = P.pair_j[w];
  const double* __restrict__ io = P.integrals + 7 * (size_t)w;
  const double V = io[0];
  const double S[3] = {io[1], io[2], io[3]};
  const bool touched = V > 0.0 || (!P.needv && (S[0] != 0.0 || S[1] != 0.0 || S[2] != 0.0));
  if (touched && (unsigned)i < (unsigned)P.nall && (unsigned)j < (unsigned)P.nall) {
    const int ti = P.type[i], tj = P.type[j];
    if (ti >= 1 && ti <= P.ntypes && tj >= 1 && tj <= P.ntypes) {
      const int tt = ti * (P.ntypes + 1) + tj;
      const double mur = P.mu_r ? P.mu_r[tt] : 0.0, gr = P.mu_r ? P.gamma_r[tt] : 0.0;
      const double mutw = P.mu_tw ? P.mu_tw[tt] : 0.0, gtw = P.mu_tw ? P.gamma_tw[tt] : 0.0;
      const bool roll = mur != 0.0 && gr != 0.0, twst = mutw != 0.0 && gtw != 0.0;
      const double q = S[0] * S[0] + S[1] * S[1] + S[2] * S[2];
      if ((roll || twst) && q > 0.0) {
        const double g = P.gamma ? P.gamma[tt] : 0.0;
        const double p = pair_pressure(P.kn[tt], P.expo[tt], V);
        const double* __restrict__ ti6 = P.twist + 6 * (size_t)i;
        const double* __restrict__ tj6 = P.twist + 6 * (size_t)j;
        double delta = 0.0;
        if (g != 0.0) {   // x and T_n enter here only
          const double T[3] = {io[4], io[5], io[6]};
          const double d[3] = {P.x[3 * j] - P.x[3 * i], P.x[3 * j + 1] - P.x[3 * i + 1], P.x[3 * j + 2] - P.x[3 * i + 2]};
          // the arm and Vdot of pair_slot (dissipation_kernels.hpp), word for word: N here is N there only while both agree
          const double A[3] = {T[0] - (d[1] * S[2] - d[2] * S[1]), T[1] - (d[2] * S[0] - d[0] * S[2]),
                               T[2] - (d[0] * S[1] - d[1] * S[0])};
          double vd = 0.0;
          for (int k = 0; k < 3; ++k) vd = fma(S[k], ti6[k] - tj6[k], vd);
          for (int k = 0; k < 3; ++k) vd = fma(T[k], ti6[3 + k], vd);
          for (int k = 0; k < 3; ++k) vd = fma(-A[k], tj6[3 + k], vd);
          delta = fmax(-p, g * vd);
        }
        const double N = (p + delta) * sqrt(q);   // p_tot |S_n|: 0 for a clamped contact
        if (N > 0.0) {
          const double Om[3] = {ti6[3] - tj6[3], ti6[4] - tj6[4], ti6[5] - tj6[5]};
          const double on = (Om[0] * S[0] + Om[1] * S[1] + Om[2] * S[2]) / q;
          const double On[3] = {on * S[0], on * S[1], on * S[2]};
          const double Pc = resisting_couples<false>(Om, On, N, roll, mur, gr, twst, mutw, gtw, M);
          if constexpr (LEDGER) Pw = Pc;
          applyj = P.newton_pair || j < P.nlocal;
        }
      }
    }
  }
  if constexpr (LEDGER) {   // every slot leaves a fresh row: the fold reads all of them
    const double share = ledger_share(P.newton_pair, j, P.nlocal);
    double* __restrict__ o = P.power + 2 * (size_t)w;
    if (P.add_power) {
      if (Pw != 0.0) o[1] += share * Pw;
    } else {
      o[0] = 0.0;
      o[1] = share * Pw;
    }
  }
  if (P.rows) {   // every slot writes its row: the gather reads all of them
    double* __restrict__ o = P.rows + 6 * (size_t)w;
    for (int k = 0; k < 3; ++k) {
      o[k] = M[k];
      o[3 + k] = applyj ? -M[k] : 0.0;
    }
    return;
  }
  if (M[0] == 0.0 && M[1] == 0.0 && M[2] == 0.0) return;   // a slot that adds nothing issues no atomic
  for (int k = 0; k < 3; ++k) atomicAdd(P.torque + 3 * (size_t)i + k, M[k]);
  if (applyj)
    for (int k = 0; k < 3; ++k) atomicAdd(P.torque + 3 * (size_t)j + k, -M[k]);
}

__global__ __launch_bounds__(kRollBlock) void rolling_pair_kernel(const RollingParams P)
{
  rolling_slot<false>(P);
}

// ... and the one that also leaves the power of the energy ledger (SPEC §2.13), launched only while it is on
__global__ __launch_bounds__(kRollBlock) void rolling_pair_ledger_kernel(const RollingParams P)
{
  rolling_slot<true>(P);
}

// one lane per (atom, torque component): the atom's rows in ascending (list slot, side), as det_gather_kernel adds them
__global__ __launch_bounds__(kRollBlock) void rolling_gather_kernel(const int nall, const int* __restrict__ start,
                                                                  const int* __restrict__ ent, const double* __restrict__ rows,
                                                                  double* __restrict__ torque)
{
  const int t = blockIdx.x * kRollBlock + threadIdx.x;
  if (t >= 3 * nall) return;
  const int a = t / 3, c = t - 3 * a;
  const int b = start[a], e = start[a + 1];
  double s = 0.0;
  for (int k = b; k < e; ++k) {
    const int v = ent[k];
    s += rows[(size_t)6 * (v >> 1) + 3 * (v & 1) + c];
  }
  if (s != 0.0) torque[3 * (size_t)a + c] += s;
}

}  // namespace shp
