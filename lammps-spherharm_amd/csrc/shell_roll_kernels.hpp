// shell_roll_kernels.hpp — the one body of the roll row of the two axial families: rolling and twisting resistance at
// cylindrical (docs/SPEC.md §2.21) and conical (§2.24) walls.
//
// The two resisting couples of §2.16 with the shell in the place of particle j, the twin of wall_roll_kernels.hpp.  An
// axial contact kernel forms its integrals in flight and keeps none (cylinder_kernels.hpp, cone_kernels.hpp), but it leaves
// one row (E, F_w, M_ax) per (particle, surface in its mask): F_w is minus the whole force on the particle from that
// surface, whichever instance wrote it.  The load is the row's part along the family's normal n (what that costs: SPEC
// §2.21, §2.24).  A streaming pass of its own behind the contact kernel needs nothing else: the contact kernel is not
// touched.  The couples are resisting_couples of contact_laws.hpp.
//   shell_roll_row    one lane per owned row.  The lane walks the bits of smask[i] in index order; per surface
//                     N = max(0, n.F_w),  Omega_rel = omega_i - Omega a (twist row; relative_spin: the product rounded on
//                     its own),  Omega_n = (Omega_rel.n) n,  Omega_r = Omega_rel - Omega_n,
//                     M = -kappa_r Omega_r - kappa_tw Omega_n with the caps mu N / |.|.
//                     The particle's sum over its surfaces goes to torque[i] with one plain read-add-write, and only
//                     where a component is not zero; the couple on the shell is -M, so the row's M_ax gains -a.M under
//                     the same rule.  No atomics, no force, entries 0..3 of a row keep their bits, and the same bits
//                     with and without the "deterministic" option.
//   LEDGER            (cylinders only) also, of M.omega_i = -P_roll + Wdot_roll, the power P_roll = kappa_r |Omega_r|^2 +
//                     kappa_tw |Omega_n|^2 into the friction entry and Wdot_roll = Omega (a.M) into the work entry of the
//                     (particle, surface) power row (SPEC §2.20): added to the row the contact kernel's LEDGER instance
//                     wrote, or written as (0, P, Wdot) for every surface in the mask where the elastic instance ran.
// A row of either kind is valid only for a surface in the CURRENT mask (rows of an earlier call or of another nlocal are
// stale): no row of a surface outside it is read.  Bound by HBM: 1 + 48 B per particle (mask, twist's omega, x) and about
// 88 B per (particle, surface) (the row read, M_ax written, the torque's read-add-write shared).
//
// A Family (cyl_roll_kernels.hpp, conic_roll_kernels.hpp) supplies Params, kStride, kRow, kPowerRow, kBlock, kOmegaRow (the
// row of Omega in the coefficient table), normal(): the foot of the centre and the unit normal the load is taken along,
// and kEarly.  The kernels are non-template one-liners in the two family headers, each in its own translation unit, and
// each keeps the machine code it had with the body written out (shpair/codeobj.kernel_hashes).  kEarly is there for that:
// the cylinder's kernels always formed the surface's and the row's address ahead of the table loads and the cone's behind
// the test, and with one order for both the other family's code moves.
#pragma once
#include <hip/hip_runtime.h>

#include "contact_laws.hpp"
#include "surface_pass.hpp"

namespace shp {

constexpr int kShellRollRows = 4;   // the table is [4][nsurf]: mu_r, gamma_r, mu_tw, gamma_tw

// Family::Params holds nlocal, nsurf, smask [nlocal], x, surf, coef, twist, roll [kShellRollRows][nsurf], rows, torque and,
// for a family with a LEDGER twin, add_power and prows: each family lays them out as its kernels always took them.
template <typename Family, bool LEDGER>
__device__ __forceinline__ void shell_roll_row(const typename Family::Params P)
{
  const int i = blockIdx.x * Family::kBlock + threadIdx.x;
  if (i >= P.nlocal) return;
  unsigned cm = P.smask[i];
  if (!cm) return;   // no surface within reach: no row of this particle is read by anyone
  const double px = P.x[3 * (size_t)i], py = P.x[3 * (size_t)i + 1], pz = P.x[3 * (size_t)i + 2];
  const double* __restrict__ tw = P.twist + 6 * (size_t)i;
  const double Om[3] = {tw[3], tw[4], tw[5]};
  double M[3] = {0.0, 0.0, 0.0};
  while (cm) {
    const int c = __builtin_ctz(cm);
    cm &= cm - 1;
    // (kEarly: the two addresses formed ahead of the table loads, as the cylinder's kernels always did; else behind the test)
    const double* __restrict__ C0 = Family::kEarly ? P.surf + Family::kStride * c : nullptr;
    double* __restrict__ row0 = Family::kEarly ? P.rows + ((size_t)i * P.nsurf + c) * Family::kRow : nullptr;
    const double mur = P.roll[c], gr = P.roll[P.nsurf + c];
    const double mutw = P.roll[2 * P.nsurf + c], gtw = P.roll[3 * P.nsurf + c];
    const bool roll = mur != 0.0 && gr != 0.0, twst = mutw != 0.0 && gtw != 0.0;
    double Pc = 0.0, Wc = 0.0;   // LEDGER only
    if (roll || twst) {
      const double* __restrict__ C = Family::kEarly ? C0 : P.surf + Family::kStride * c;
      double* __restrict__ row = Family::kEarly ? row0 : P.rows + ((size_t)i * P.nsurf + c) * Family::kRow;
      const double ax[3] = {C[3], C[4], C[5]};
      const AxialUnit nu = Family::normal(C, px, py, pz, ax[0], ax[1], ax[2]);
      const double nn[3] = {nu.c0, nu.c1, nu.c2};
      const double N = fmax(0.0, nn[0] * row[1] + nn[1] * row[2] + nn[2] * row[3]);   // 0 for V <= 0 and for a clamped contact
      if (N > 0.0) {
        const double Oc = P.coef[Family::kOmegaRow * P.nsurf + c];
        const double Orel[3] = {relative_spin(Om[0], Oc, ax[0]), relative_spin(Om[1], Oc, ax[1]), relative_spin(Om[2], Oc, ax[2])};
        const double on = Orel[0] * nn[0] + Orel[1] * nn[1] + Orel[2] * nn[2];
        const double On[3] = {on * nn[0], on * nn[1], on * nn[2]};
        double Mc[3];
        const double Pr = resisting_couples<false>(Orel, On, N, roll, mur, gr, twst, mutw, gtw, Mc);
        M[0] += Mc[0]; M[1] += Mc[1]; M[2] += Mc[2];
        const double am = ax[0] * Mc[0] + ax[1] * Mc[1] + ax[2] * Mc[2];
        if (am != 0.0) row[4] -= am;   // the couple on the shell is -M: M_ax stays what the drive works against
        if constexpr (LEDGER) {
          Pc = Pr;
          Wc = Oc * am;
        }
      }
    }
    if constexpr (LEDGER) {   // every surface in the mask leaves a fresh row: the fold reads all of them
      double* __restrict__ prow = P.prows + ((size_t)i * P.nsurf + c) * Family::kPowerRow;
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

}  // namespace shp
