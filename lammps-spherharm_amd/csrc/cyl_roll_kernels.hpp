// cyl_roll_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.21: rolling and twisting resistance at cylindrical walls.
//
// The row is shell_roll_row of shell_roll_kernels.hpp, which describes it; here are what the cylinder supplies and the two
// kernels.  The normal is the shell's exact inward one on the radial line through the centre, n = -c with c = rho / d
// from cyl_foot, the operations of the candidate and the contact kernel: the load is N = max(0, c.F_w), the row's radial
// part.  a is normal to c: the drum's rotation only rolls.
//   cyl_roll_kernel          the row behind any of the five instances of the contact kernel
//   cyl_roll_ledger_kernel   the LEDGER twin, launched only while both ledgers are on (SPEC §2.20)
// Included by shstep_cylinders.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "cylinder_kernels.hpp"
#include "shell_roll_kernels.hpp"

namespace shp {

constexpr int kCylRollRows = kShellRollRows;   // the table is [4][ncyl]: mu_r,c, gamma_r,c, mu_tw,c, gamma_tw,c

struct CylRollParams {
  int nlocal, nsurf;
  int add_power;                // LEDGER: a LEDGER instance of the contact body has written the power rows of this pass: add to them
  const unsigned char* smask;   // [nlocal] of the candidate pass: 0 for a particle outside the group
  const double* x;              // [nlocal][3]
  const double* surf;           // kCylStride doubles per cylinder
  const double* coef;           // [kCylCoefRows][ncyl]: row 3 is Omega_c
  const double* twist;          // [nlocal][6]: velocity of the SH origin and angular velocity, space frame
  const double* roll;           // [kCylRollRows][ncyl]
  double* rows;                 // [nlocal][ncyl][kCylRow] of this pass: entries 1..3 are read, entry 4 gains -a.M_c
  double* torque;
  double* prows;                // LEDGER only: [nlocal][ncyl][kCylPowerRow] P_d, P_f, Wdot_c
};

struct CylRollFamily {
  using Params = CylRollParams;
  static constexpr int kStride = kCylStride, kRow = kCylRow, kPowerRow = kCylPowerRow, kBlock = kCylBlock, kOmegaRow = 3;
  static constexpr bool kEarly = true;   // where the row forms its addresses: shell_roll_kernels.hpp
  // c = rho / d, as cyl_contact_body
  static __device__ __forceinline__ AxialUnit normal(const double* C, const double px, const double py, const double pz, const double a0,
                                                     const double a1, const double a2)
  {
    const CylFoot ft = cyl_foot(C, px, py, pz);
    return axial_radial_unit(ft.d, ft.r0, ft.r1, ft.r2, a0, a1, a2);
  }
};

__global__ __launch_bounds__(kCylBlock) void cyl_roll_kernel(const CylRollParams P) { shell_roll_row<CylRollFamily, false>(P); }

// ... and the one that also leaves the powers of the shell ledger (SPEC §2.20), launched only while both ledgers are on
__global__ __launch_bounds__(kCylBlock) void cyl_roll_ledger_kernel(const CylRollParams P) { shell_roll_row<CylRollFamily, true>(P); }

}  // namespace shp
