// friction_kernels.hpp — gfx950 kernel of docs/SPEC.md §2.11: Coulomb-capped viscous friction of SH pairs, together
// with the volume-rate damping of §2.10 (damp_kernels.hpp) in one pass.
//
// History-free (LAMMPS gran/hooke): F_t = -kappa v_t with kappa = gamma_t while gamma_t |v_t| <= mu N, mu N / |v_t|
// beyond.  Everything comes from what a list slot already holds: the integrals V, S_n, T_n of the last compute, the two
// twists, d = x_j - x_i and the bounding radii.  The contact point is the point of the normal wrench's line of action
// (through r_perp = S_n x T_n / |S_n|^2, along S_n) nearest the radical plane of the two bounding spheres; both bodies
// take the force there, so momentum and angular momentum are conserved exactly.  One division by q = |S_n|^2, one
// square root for N = p_tot |S_n|, one for |v_t|; no unit vector is formed, so v_t = 0 gives exactly zero.
//   pair_dissipation_kernel   one lane per list slot: delta = p_tot - p as pair_damp_kernel forms it (0 where gamma_ij
//                             is 0), then F_t; F_i = -delta S_n + F_t, tau_i = -delta T_n + r_i x F_t, F_j = -F_i,
//                             tau_j = delta (T_n - d x S_n) - r_j x F_t.  Scatter as in pair_damp_kernel: FP64 atomics,
//                             or the 12-double row per slot of the deterministic mode.
// The library launches it only while a friction coefficient is set; pair_damp_kernel keeps serving damping alone.
// Included by shstep_api.hip only (the kernel is not a template: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "damp_kernels.hpp"

namespace shp {

struct FrictionParams {
  DampParams d;            // gamma may be null: no damping coefficient was ever set
  int nshapes;
  const int* shtype;
  const double* rmax;      // [nshapes] bounding radii
  const double* mu;        // (ntypes+1)^2, like gamma
  const double* gamma_t;
};

__global__ __launch_bounds__(kDampBlock) void pair_dissipation_kernel(const FrictionParams Q)
{
  const DampParams& P = Q.d;
  const int w = blockIdx.x * kDampBlock + threadIdx.x;
  if (w >= P.npairs) return;
  double Fi[3] = {0.0, 0.0, 0.0}, Ti[3] = {0.0, 0.0, 0.0}, Tj[3] = {0.0, 0.0, 0.0};
  bool act = false, applyj = false;
  const int i = P.pair_i[w], j = P.pair_j[w];
  const double* __restrict__ io = P.integrals + 7 * (size_t)w;
  const double V = io[0];
  const double S[3] = {io[1], io[2], io[3]};
  // touched, as the contact kernels' epilogue decides it
  const bool touched = V > 0.0 || (!P.needv && (S[0] != 0.0 || S[1] != 0.0 || S[2] != 0.0));
  if (touched && (unsigned)i < (unsigned)P.nall && (unsigned)j < (unsigned)P.nall) {
    const int ti = P.type[i], tj = P.type[j];
    if (ti >= 1 && ti <= P.ntypes && tj >= 1 && tj <= P.ntypes) {   // (the set-up kernel reported a type out of range)
      const int tt = ti * (P.ntypes + 1) + tj;
      const double g = P.gamma ? P.gamma[tt] : 0.0;
      const double mu = Q.mu[tt], gt = Q.gamma_t[tt];
      const bool fric = mu != 0.0 && gt != 0.0;
      if (g != 0.0 || fric) {
        const double T[3] = {io[4], io[5], io[6]};
        const double kn = P.kn[tt], m = P.expo[tt];
        const double p = (m == 1.0 || !(V > 0.0)) ? kn : kn * m * pow(V, m - 1.0);
        const double d[3] = {P.x[3 * j] - P.x[3 * i], P.x[3 * j + 1] - P.x[3 * i + 1], P.x[3 * j + 2] - P.x[3 * i + 2]};
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
        // (a shape index out of range was reported by the set-up kernel of the compute)
        if (fric && q > 0.0 && dd > 0.0 && N > 0.0 && (unsigned)si < (unsigned)Q.nshapes && (unsigned)sj < (unsigned)Q.nshapes) {
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
          const double vtn = sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
          const double cap = mu * N;
          const double kappa = gt * vtn <= cap ? gt : cap / vtn;   // vtn = 0 takes the first branch
          const double Ft[3] = {-kappa * vt[0], -kappa * vt[1], -kappa * vt[2]};
          Fi[0] += Ft[0]; Fi[1] += Ft[1]; Fi[2] += Ft[2];
          Ti[0] += ri[1] * Ft[2] - ri[2] * Ft[1];
          Ti[1] += ri[2] * Ft[0] - ri[0] * Ft[2];
          Ti[2] += ri[0] * Ft[1] - ri[1] * Ft[0];
          Tj[0] -= rj[1] * Ft[2] - rj[2] * Ft[1];
          Tj[1] -= rj[2] * Ft[0] - rj[0] * Ft[2];
          Tj[2] -= rj[0] * Ft[1] - rj[1] * Ft[0];
          act = act || vtn != 0.0;
        }
        applyj = P.newton_pair || j < P.nlocal;
      }
    }
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

}  // namespace shp
