// wall_roll_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.17: rolling and twisting resistance at planar walls.
//
// The two resisting couples of §2.16 with the wall in the place of particle j: a wall does not rotate, so they act on the
// particle's own angular velocity, split along the exact wall normal.  The wall contact kernel forms its integrals in
// flight and keeps none (wall_kernels.hpp), but it leaves one (E, F_w) row per (particle, wall in its mask): minus the
// whole force on the particle from that wall.  Friction and the tangential spring lie in the plane by construction, so
// the row's part along n_w is the normal load, and a streaming pass of its own behind the contact kernel needs nothing
// else: the contact kernel is not touched.  The couples themselves are resisting_couples of contact_laws.hpp, the law
// the pair pass of rolling_kernels.hpp applies; only the normal part of Omega is formed here, with the exact n_w.
//   wall_roll_kernel  one lane per owned row.  The lane walks the bits of wmask[i] in index order; per wall
//                     N = max(0, -n_w.F_w),  Omega = omega_i (twist row; u_w of §2.12 does not enter),
//                     Omega_n = (Omega.n_w) n_w,  Omega_r = Omega - Omega_n,
//                     kappa_r = gamma_r while gamma_r |Omega_r| <= mu_r N, mu_r N / |Omega_r| beyond; kappa_tw alike from
//                     gamma_tw, mu_tw, |Omega_n|;  M = -kappa_r Omega_r - kappa_tw Omega_n.
//                     The particle's sum over its walls goes to torque[i] with one plain read-add-write, and only where
//                     a component is not zero: no atomics, no force, every zero of torque keeps its bits, and the same
//                     bits with and without the "deterministic" option.
//   wall_roll_ledger_kernel   the same, and the power kappa_r |Omega_r|^2 + kappa_tw |Omega_n|^2 into the friction entry
//                     of the (particle, wall) power row (SPEC §2.13): added to the row the contact kernel's LEDGER
//                     instance wrote, or written as (0, P) for every wall in the mask where the elastic instance ran.
// A row of either kind is valid only for a wall in the CURRENT mask (rows of an earlier call or of another nlocal are
// stale): no row of a wall outside it is read.  Bound by HBM: 4 + 24 B per particle and 32 B per (particle, wall).
// Included by shstep_walls.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "contact_laws.hpp"
#include "wall_kernels.hpp"

namespace shp {

struct WallRollParams {
  int nlocal, nwalls;
  int add_power;           // LEDGER: the contact kernel's instance has written the power rows of this pass: add to the friction entry
  const unsigned* wmask;   // [nlocal] of the candidate pass: 0 for a particle outside the group
  const double* walls;     // kWallStride doubles per wall, the normal first
  const double* rows;      // [nlocal][nwalls][4] E, F_w of this pass
  const double* twist;     // [nlocal][6]: velocity of the SH origin and angular velocity, space frame
  const double* wroll;     // [4][nwalls] mu_r,w, gamma_r,w, mu_tw,w, gamma_tw,w
  double* torque;
  double* prows;           // LEDGER only: [nlocal][nwalls][2] P_d, P_f
};

template <bool LEDGER>
__device__ __forceinline__ void wall_roll_row(const WallRollParams P)
{
  const int i = blockIdx.x * kWallBlock + threadIdx.x;
  if (i >= P.nlocal) return;
  unsigned wm = P.wmask[i];
  if (!wm) return;   // no wall within reach: no row of this particle is read by anyone
  const double* __restrict__ tw = P.twist + 6 * (size_t)i;
  const double Om[3] = {tw[3], tw[4], tw[5]};
  double M[3] = {0.0, 0.0, 0.0};
  while (wm) {
    const int w = __builtin_ctz(wm);
    wm &= wm - 1;
    const double* __restrict__ W = P.walls + kWallStride * w;
    const double* __restrict__ row = P.rows + ((size_t)i * P.nwalls + w) * 4;
    const double mur = P.wroll[w], gr = P.wroll[P.nwalls + w];
    const double mutw = P.wroll[2 * P.nwalls + w], gtw = P.wroll[3 * P.nwalls + w];
    const bool roll = mur != 0.0 && gr != 0.0, twst = mutw != 0.0 && gtw != 0.0;
    const double N = fmax(0.0, -(W[0] * row[1] + W[1] * row[2] + W[2] * row[3]));   // 0 for V <= 0 and for a clamped contact
    double Pw = 0.0;   // LEDGER only
    if ((roll || twst) && N > 0.0) {
      const double on = Om[0] * W[0] + Om[1] * W[1] + Om[2] * W[2];
      const double On[3] = {on * W[0], on * W[1], on * W[2]};
      const double Pc = resisting_couples<true>(Om, On, N, roll, mur, gr, twst, mutw, gtw, M);
      if constexpr (LEDGER) Pw = Pc;
    }
    if constexpr (LEDGER) {   // every wall in the mask leaves a fresh row: the fold reads all of them
      double* __restrict__ prow = P.prows + ((size_t)i * P.nwalls + w) * 2;
      if (P.add_power) {
        if (Pw != 0.0) prow[1] += Pw;
      } else {
        prow[0] = 0.0;
        prow[1] = Pw;
      }
    }
  }
  for (int k = 0; k < 3; ++k)   // the only writer of row i at this point of the stream
    if (M[k] != 0.0) P.torque[3 * (size_t)i + k] += M[k];
}

__global__ __launch_bounds__(kWallBlock) void wall_roll_kernel(const WallRollParams P) { wall_roll_row<false>(P); }

// ... and the one that also leaves the power of the energy ledger (SPEC §2.13), launched only while it is on
__global__ __launch_bounds__(kWallBlock) void wall_roll_ledger_kernel(const WallRollParams P) { wall_roll_row<true>(P); }

}  // namespace shp
