// conic_roll_kernels.hpp — gfx950 kernel of docs/SPEC.md §2.24: rolling and twisting resistance at conical walls.
//
// The two resisting couples of §2.16 with the cone in the place of particle j, the twin of cyl_roll_kernels.hpp.  The
// cone contact kernel forms its integrals in flight and keeps none (cone_kernels.hpp), but it leaves one row
// (E_k, F_w, M_ax) per (particle, cone in its mask): F_w is minus the whole force on the particle from that cone,
// whichever of the three instances wrote it.  The normal is the wall's geometric outward one at the nearest generator,
// n = c c^ - s a^ with c^ = rho / d from cone_foot, the operations of the candidate and the contact kernel (c, s the
// cosine and sine of the half-angle), never S^; the load is the row's part along it (what that costs: SPEC §2.24).  A
// streaming pass of its own behind the contact kernel needs nothing else: the contact kernel is not touched.  The
// couples are resisting_couples of contact_laws.hpp.
//   conic_roll_kernel   one lane per owned row.  The lane walks the bits of the cone mask of row i in index order; per cone
//                     N = max(0, n.F_w),  Omega_rel = omega_i - Omega_k a (twist row; the product rounded on its own, so a
//                     particle carried rigidly round by the cone, omega_i = Omega_k a, has exactly 0),
//                     Omega_n = (Omega_rel.n) n,  Omega_r = Omega_rel - Omega_n  (a.n = -s: unlike a drum's, the cone's
//                     rotation twists, by -Omega_k s n, and rolls, by Omega_k c g^),
//                     M_k = -kappa_r Omega_r - kappa_tw Omega_n with the caps mu N / |.|.
//                     The particle's sum over its cones goes to torque[i] with one plain read-add-write, and only where
//                     a component is not zero; the couple on the wall is -M_k, so the row's M_ax gains -a.M_k under the
//                     same rule.  No atomics, no force, entries 0..3 of a row keep their bits, and the same bits with
//                     and without the "deterministic" option.
// There is no ledger twin: cones keep no ledger entries.
// A row is valid only for a cone in the CURRENT mask (rows of an earlier call or of another nlocal are stale): no row of
// a cone outside it is read.  Bound by HBM: 1 + 48 B per particle (mask, twist's omega, x) and about 88 B per (particle,
// cone) (the row read, M_ax written, the torque's read-add-write shared).
// Included by shstep_cones.hip only (the kernel is not a template: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "cone_kernels.hpp"
#include "contact_laws.hpp"

namespace shp {

constexpr int kConicRollRows = 4;   // the table is [4][ncone]: mu_r,k, gamma_r,k, mu_tw,k, gamma_tw,k

struct ConicRollParams {
  int nlocal, ncone;
  const unsigned char* kmask;   // [nlocal] of the candidate pass: 0 for a particle outside the group
  const double* x;              // [nlocal][3]
  const double* cones;          // kConeStride doubles per cone
  const double* coef;           // [kConeCoefRows][ncone]: row 3 is Omega_k
  const double* twist;          // [nlocal][6]: velocity of the SH origin and angular velocity, space frame
  const double* kroll;          // [kConicRollRows][ncone]
  double* rows;                 // [nlocal][ncone][kConeRow] of this pass: entries 1..3 are read, entry 4 gains -a.M_k
  double* torque;
};

// omega_i - Omega_k a with the product rounded before the difference: no fma, so that omega_i = Omega_k a gives 0
__device__ __forceinline__ double conic_relative_spin(const double om, const double Ok, const double a)
{
#pragma clang fp contract(off)
  const double carried = Ok * a;
  return om - carried;
}

__global__ __launch_bounds__(kConeBlock) void conic_roll_kernel(const ConicRollParams P)
{
  const int i = blockIdx.x * kConeBlock + threadIdx.x;
  if (i >= P.nlocal) return;
  unsigned cm = P.kmask[i];
  if (!cm) return;   // no cone within reach: no row of this particle is read by anyone
  const double px = P.x[3 * (size_t)i], py = P.x[3 * (size_t)i + 1], pz = P.x[3 * (size_t)i + 2];
  const double* __restrict__ tw = P.twist + 6 * (size_t)i;
  const double Om[3] = {tw[3], tw[4], tw[5]};
  double M[3] = {0.0, 0.0, 0.0};
  while (cm) {
    const int c = __builtin_ctz(cm);
    cm &= cm - 1;
    const double mur = P.kroll[c], gr = P.kroll[P.ncone + c];
    const double mutw = P.kroll[2 * P.ncone + c], gtw = P.kroll[3 * P.ncone + c];
    const bool roll = mur != 0.0 && gr != 0.0, twst = mutw != 0.0 && gtw != 0.0;
    if (!(roll || twst)) continue;
    const double* __restrict__ C = P.cones + kConeStride * c;
    double* __restrict__ row = P.rows + ((size_t)i * P.ncone + c) * kConeRow;
    const double ax[3] = {C[3], C[4], C[5]};
    const double ct = C[6], sn = C[7];
    const ConeFoot ft = cone_foot(C, px, py, pz);
    // c^ = rho / d; on the axis (d = 0 as computed) the e1 of the frame rule about the axis, as cone_contact_body
    double cc[3];
    if (ft.d > 0.0) {
      const double di = 1.0 / ft.d;
      cc[0] = ft.r0 * di; cc[1] = ft.r1 * di; cc[2] = ft.r2 * di;
    } else {
      const double s = copysign(1.0, ax[2]), a = -1.0 / (s + ax[2]);
      cc[0] = 1.0 + s * ax[0] * ax[0] * a; cc[1] = s * (ax[0] * ax[1] * a); cc[2] = -s * ax[0];
    }
    // n^ = c c^ - s a^, the outward wall normal at the nearest generator, with the operations of cone_contact_body
    const double nn[3] = {fma(ct, cc[0], -(sn * ax[0])), fma(ct, cc[1], -(sn * ax[1])), fma(ct, cc[2], -(sn * ax[2]))};
    const double N = fmax(0.0, nn[0] * row[1] + nn[1] * row[2] + nn[2] * row[3]);   // 0 for V <= 0 and for a clamped contact
    if (N > 0.0) {
      const double Ok = P.coef[3 * P.ncone + c];
      const double Orel[3] = {conic_relative_spin(Om[0], Ok, ax[0]), conic_relative_spin(Om[1], Ok, ax[1]),
                              conic_relative_spin(Om[2], Ok, ax[2])};
      const double on = Orel[0] * nn[0] + Orel[1] * nn[1] + Orel[2] * nn[2];
      const double On[3] = {on * nn[0], on * nn[1], on * nn[2]};
      double Mk[3];
      resisting_couples<false>(Orel, On, N, roll, mur, gr, twst, mutw, gtw, Mk);
      M[0] += Mk[0]; M[1] += Mk[1]; M[2] += Mk[2];
      const double am = ax[0] * Mk[0] + ax[1] * Mk[1] + ax[2] * Mk[2];
      if (am != 0.0) row[4] -= am;   // the couple on the wall is -M_k: M_ax stays what the drive works against
    }
  }
  for (int k = 0; k < 3; ++k)   // the only writer of row i at this point of the stream
    if (M[k] != 0.0) P.torque[3 * (size_t)i + k] += M[k];
}

}  // namespace shp
