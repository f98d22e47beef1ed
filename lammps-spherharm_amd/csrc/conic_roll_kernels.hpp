// conic_roll_kernels.hpp — gfx950 kernel of docs/SPEC.md §2.24: rolling and twisting resistance at conical walls.
//
// The row is shell_roll_row of shell_roll_kernels.hpp, which describes it; here are what the cone supplies and the
// kernel.  The normal is the wall's geometric outward one at the nearest generator, n = c c^ - s a^ with c^ = rho / d from
// cone_foot, the operations of the candidate and the contact kernel (c, s the cosine and sine of the half-angle), never S^:
// the load is N = max(0, n.F_w).  a.n = -s: unlike a drum's, the cone's rotation twists, by -Omega_k s n, and rolls, by
// Omega_k c g^.
//   conic_roll_kernel   the row behind any of the three instances of the contact kernel
// There is no ledger twin: cones keep no ledger entries.
// Included by shstep_cones.hip only (the kernel is not a template: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "cone_kernels.hpp"
#include "shell_roll_kernels.hpp"

namespace shp {

constexpr int kConicRollRows = kShellRollRows;   // the table is [4][ncone]: mu_r,k, gamma_r,k, mu_tw,k, gamma_tw,k

struct ConicRollParams {
  int nlocal, nsurf;
  const unsigned char* smask;   // [nlocal] of the candidate pass: 0 for a particle outside the group
  const double* x;              // [nlocal][3]
  const double* surf;           // kConeStride doubles per cone
  const double* coef;           // [kConeCoefRows][ncone]: row 3 is Omega_k
  const double* twist;          // [nlocal][6]: velocity of the SH origin and angular velocity, space frame
  const double* roll;           // [kConicRollRows][ncone]
  double* rows;                 // [nlocal][ncone][kConeRow] of this pass: entries 1..3 are read, entry 4 gains -a.M_k
  double* torque;
};

struct ConicRollFamily {
  using Params = ConicRollParams;
  static constexpr int kStride = kConeStride, kRow = kConeRow, kPowerRow = 0, kBlock = kConeBlock, kOmegaRow = 3;
  static constexpr bool kEarly = false;   // where the row forms its addresses: shell_roll_kernels.hpp
  // n^ = c c^ - s a^, the outward wall normal at the nearest generator, with the operations of cone_contact_body
  static __device__ __forceinline__ AxialUnit normal(const double* C, const double px, const double py, const double pz, const double a0,
                                                     const double a1, const double a2)
  {
    const double ct = C[6], sn = C[7];
    const ConeFoot ft = cone_foot(C, px, py, pz);
    const AxialUnit cu = axial_radial_unit(ft.d, ft.r0, ft.r1, ft.r2, a0, a1, a2);
    AxialUnit n;
    n.c0 = fma(ct, cu.c0, -(sn * a0)); n.c1 = fma(ct, cu.c1, -(sn * a1)); n.c2 = fma(ct, cu.c2, -(sn * a2));
    return n;
  }
};

__global__ __launch_bounds__(kConeBlock) void conic_roll_kernel(const ConicRollParams P) { shell_roll_row<ConicRollFamily, false>(P); }

}  // namespace shp
