// cyl_power_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.20: the cylinder entries of the energy ledger.
//
// While the energy ledger and the shell ledger are on, a cylinder pass with a coefficient launches one of the two LEDGER
// instances of cyl_contact_body (cylinder_kernels.hpp) in place of the ordinary one; it leaves a power row
// (P_d, P_f, Wdot_c) per (particle, cylinder in its mask) beside everything the ordinary instance writes, with the same
// bits.  The fold adds dt times the sums of the rows into the shell accumulator, 3 totals then 3 per cylinder:
//   cyl_power_partial_kernel   block (b, c) adds the rows of particles [256 b, 256 b + 256) for cylinder c through the
//                              mask: the partition and the tree of cyl_rows_partial_kernel (surface_pass.hpp)
//   cyl_power_final_kernel     one block: per cylinder the block sums in ascending order through the same tree; thread 0
//                              multiplies by dt and adds into the accumulator, the cylinders one after the other
// Nothing is added with an atomic and the partition depends on the particle count only: the sums are bitwise reproducible,
// with or without the "deterministic" option.  Each instance takes a parameter struct of its own, the common one with
// prows behind it, so the kernel arguments of the other instances stay what they were.
//
// Included by shstep_cylinders.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "cylinder_kernels.hpp"
#include "shpair_ctx.hpp"   // kShellTotals, kShellDoubles: the accumulator, totals then 3 per cylinder

namespace shp {

struct CylPowerParams : CylParams {
  double* prows;   // [nlocal][ncyl][kCylPowerRow] P_d, P_f, Wdot_c
};

struct CylPowerSpringParams : CylSpringParams {
  double* prows;
};

static_assert(offsetof(CylPowerParams, prows) == sizeof(CylParams) && offsetof(CylPowerSpringParams, prows) == sizeof(CylSpringParams),
              "the LEDGER instances' arguments: the common ones, then prows");

__global__ __launch_bounds__(kCylBlock) void cyl_power_dissipative_kernel(const CylPowerParams P)
{
  cyl_contact_body<true, false, CylPowerParams, true>(P);
}

__global__ __launch_bounds__(kCylBlock) void cyl_power_spring_kernel(const CylPowerSpringParams P)
{
  cyl_contact_body<true, true, CylPowerSpringParams, true>(P);
}

// part: [ncyl][gridDim.x][kCylPowerRow]
__global__ __launch_bounds__(kCylBlock) void cyl_power_partial_kernel(int nlocal, int ncyl, const unsigned char* __restrict__ cmask,
                                                                       const double* __restrict__ prows, double* __restrict__ part)
{
  surface_rows_partial<kCylPowerRow>(nlocal, ncyl, cmask, prows, part);
}

// acc: kShellDoubles time integrals
__global__ __launch_bounds__(kCylBlock) void cyl_power_final_kernel(const int ncyl, const int nb, const double* __restrict__ part,
                                                                     const double dt, double* __restrict__ acc)
{
  __shared__ double sh[kCylPowerRow][kCylBlock];
  double tot[kCylPowerRow] = {0.0, 0.0, 0.0};   // thread 0: this fold's totals over the cylinders, in cylinder order
  for (int c = 0; c < ncyl; ++c) {
    double v[kCylPowerRow] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += kCylBlock)
      for (int k = 0; k < kCylPowerRow; ++k) v[k] += part[((size_t)c * nb + b) * kCylPowerRow + k];
    surface_block_sum<kCylPowerRow>(v, sh);
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)   // dt times the sum is rounded once, not fused into either addition: one cylinder's totals are its entry
      double* a = acc + kShellTotals + kCylPowerRow * c;
      for (int k = 0; k < kCylPowerRow; ++k) {
        const double e = dt * sh[k][0];
        a[k] += e;
        tot[k] += e;
      }
    }
    __syncthreads();   // the next cylinder writes sh again
  }
  if (threadIdx.x == 0)
    for (int k = 0; k < kShellTotals; ++k) acc[k] += tot[k];
}

}  // namespace shp
