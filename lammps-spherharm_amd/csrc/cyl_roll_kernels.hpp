// cyl_roll_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.21: rolling and twisting resistance at cylindrical walls.
//
// The two resisting couples of §2.16 with the shell in the place of particle j, the twin of wall_roll_kernels.hpp.  The
// cylinder contact kernel forms its integrals in flight and keeps none (cylinder_kernels.hpp), but it leaves one row
// (E_c, F_w, M_ax) per (particle, cylinder in its mask): F_w is minus the whole force on the particle from that
// cylinder, whichever of the five instances wrote it.  The normal is the shell's exact inward one on the radial line
// through the centre, n = -c with c = rho / d from cyl_foot, the operations of the candidate and the contact kernel; the
// load is the row's radial part (what that costs: SPEC §2.21).  A streaming pass of its own behind the contact kernel
// needs nothing else: the contact kernel is not touched.  The couples are resisting_couples of contact_laws.hpp.
//   cyl_roll_kernel   one lane per owned row.  The lane walks the bits of cmask[i] in index order; per cylinder
//                     N = max(0, c.F_w),  Omega_rel = omega_i - Omega_c a (twist row; the product rounded on its own, so a
//                     particle carried rigidly round by the drum, omega_i = Omega_c a, has exactly 0),
//                     Omega_n = (Omega_rel.c) c,  Omega_r = Omega_rel - Omega_n  (a is normal to c: the drum's rotation
//                     only rolls),  M_c = -kappa_r Omega_r - kappa_tw Omega_n with the caps mu N / |.|.
//                     The particle's sum over its cylinders goes to torque[i] with one plain read-add-write, and only
//                     where a component is not zero; the couple on the shell is -M_c, so the row's M_ax gains -a.M_c
//                     under the same rule.  No atomics, no force, entries 0..3 of a row keep their bits, and the same
//                     bits with and without the "deterministic" option.
//   cyl_roll_ledger_kernel   the same, and of M.omega_i = -P_roll + Wdot_roll the power P_roll = kappa_r |Omega_r|^2 +
//                     kappa_tw |Omega_n|^2 into the friction entry and Wdot_roll = Omega_c (a.M_c) into the work entry of
//                     the (particle, cylinder) power row (SPEC §2.20): added to the row the contact kernel's LEDGER
//                     instance wrote, or written as (0, P, Wdot) for every cylinder in the mask where the elastic
//                     instance ran.
// A row of either kind is valid only for a cylinder in the CURRENT mask (rows of an earlier call or of another nlocal
// are stale): no row of a cylinder outside it is read.  Bound by HBM: 1 + 48 B per particle (mask, twist's omega, x) and
// about 88 B per (particle, cylinder) (the row read, M_ax written, the torque's read-add-write shared).
// Included by shstep_cylinders.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "contact_laws.hpp"
#include "cylinder_kernels.hpp"

namespace shp {

constexpr int kCylRollRows = 4;   // the table is [4][ncyl]: mu_r,c, gamma_r,c, mu_tw,c, gamma_tw,c

struct CylRollParams {
  int nlocal, ncyl;
  int add_power;                // LEDGER: a LEDGER instance of the contact body has written the power rows of this pass: add to them
  const unsigned char* cmask;   // [nlocal] of the candidate pass: 0 for a particle outside the group
  const double* x;              // [nlocal][3]
  const double* cyls;           // kCylStride doubles per cylinder
  const double* coef;           // [kCylCoefRows][ncyl]: row 3 is Omega_c
  const double* twist;          // [nlocal][6]: velocity of the SH origin and angular velocity, space frame
  const double* croll;          // [kCylRollRows][ncyl]
  double* rows;                 // [nlocal][ncyl][kCylRow] of this pass: entries 1..3 are read, entry 4 gains -a.M_c
  double* torque;
  double* prows;                // LEDGER only: [nlocal][ncyl][kCylPowerRow] P_d, P_f, Wdot_c
};

// omega_i - Omega_c a with the product rounded before the difference: no fma, so that omega_i = Omega_c a gives 0
__device__ __forceinline__ double cyl_relative_spin(const double om, const double Oc, const double a)
{
#pragma clang fp contract(off)
  const double carried = Oc * a;
  return om - carried;
}

template <bool LEDGER>
__device__ __forceinline__ void cyl_roll_row(const CylRollParams P)
{
  const int i = blockIdx.x * kCylBlock + threadIdx.x;
  if (i >= P.nlocal) return;
  unsigned cm = P.cmask[i];
  if (!cm) return;   // no cylinder within reach: no row of this particle is read by anyone
  const double px = P.x[3 * (size_t)i], py = P.x[3 * (size_t)i + 1], pz = P.x[3 * (size_t)i + 2];
  const double* __restrict__ tw = P.twist + 6 * (size_t)i;
  const double Om[3] = {tw[3], tw[4], tw[5]};
  double M[3] = {0.0, 0.0, 0.0};
  while (cm) {
    const int c = __builtin_ctz(cm);
    cm &= cm - 1;
    const double* __restrict__ C = P.cyls + kCylStride * c;
    double* __restrict__ row = P.rows + ((size_t)i * P.ncyl + c) * kCylRow;
    const double mur = P.croll[c], gr = P.croll[P.ncyl + c];
    const double mutw = P.croll[2 * P.ncyl + c], gtw = P.croll[3 * P.ncyl + c];
    const bool roll = mur != 0.0 && gr != 0.0, twst = mutw != 0.0 && gtw != 0.0;
    double Pc = 0.0, Wc = 0.0;   // LEDGER only
    if (roll || twst) {
      const double ax[3] = {C[3], C[4], C[5]};
      const CylFoot ft = cyl_foot(C, px, py, pz);
      // c = rho / d; on the axis (d = 0 as computed) the e1 of the frame rule about the axis, as cyl_contact_body
      double cc[3];
      if (ft.d > 0.0) {
        const double di = 1.0 / ft.d;
        cc[0] = ft.r0 * di; cc[1] = ft.r1 * di; cc[2] = ft.r2 * di;
      } else {
        const double s = copysign(1.0, ax[2]), a = -1.0 / (s + ax[2]);
        cc[0] = 1.0 + s * ax[0] * ax[0] * a; cc[1] = s * (ax[0] * ax[1] * a); cc[2] = -s * ax[0];
      }
      const double N = fmax(0.0, cc[0] * row[1] + cc[1] * row[2] + cc[2] * row[3]);   // 0 for V <= 0 and for a clamped contact
      if (N > 0.0) {
        const double Oc = P.coef[3 * P.ncyl + c];
        const double Orel[3] = {cyl_relative_spin(Om[0], Oc, ax[0]), cyl_relative_spin(Om[1], Oc, ax[1]),
                                cyl_relative_spin(Om[2], Oc, ax[2])};
        const double on = Orel[0] * cc[0] + Orel[1] * cc[1] + Orel[2] * cc[2];
        const double On[3] = {on * cc[0], on * cc[1], on * cc[2]};
        double Mc[3];
        const double Pr = resisting_couples<false>(Orel, On, N, roll, mur, gr, twst, mutw, gtw, Mc);
        M[0] += Mc[0]; M[1] += Mc[1]; M[2] += Mc[2];
        const double am = ax[0] * Mc[0] + ax[1] * Mc[1] + ax[2] * Mc[2];
        if (am != 0.0) row[4] -= am;   // the couple on the shell is -M_c: M_ax stays what the drive works against
        if constexpr (LEDGER) {
          Pc = Pr;
          Wc = Oc * am;
        }
      }
    }
    if constexpr (LEDGER) {   // every cylinder in the mask leaves a fresh row: the fold reads all of them
      double* __restrict__ prow = P.prows + ((size_t)i * P.ncyl + c) * kCylPowerRow;
      if (P.add_power) {
        if (Pc != 0.0) prow[1] += Pc;
        if (Wc != 0.0) prow[2] += Wc;
      } else {
        prow[0] = 0.0;
        prow[1] = Pc;
        prow[2] = Wc;
      }
    }
  }
  for (int k = 0; k < 3; ++k)   // the only writer of row i at this point of the stream
    if (M[k] != 0.0) P.torque[3 * (size_t)i + k] += M[k];
}

__global__ __launch_bounds__(kCylBlock) void cyl_roll_kernel(const CylRollParams P) { cyl_roll_row<false>(P); }

// ... and the one that also leaves the powers of the shell ledger (SPEC §2.20), launched only while both ledgers are on
__global__ __launch_bounds__(kCylBlock) void cyl_roll_ledger_kernel(const CylRollParams P) { cyl_roll_row<true>(P); }

}  // namespace shp
