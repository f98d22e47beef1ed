// ledger_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.13: the fold of the energy ledger.
//
// The pair dissipation pass leaves one power row per list slot (dissipation_kernels.hpp, the LEDGER instances), the wall
// pass one (E, F_w) row and one power row per (particle, wall in its mask) (wall_kernels.hpp).  The fold adds dt times
// their sums, and dt times the work rate -F_w.u_w of every wall, into the context's accumulator:
//   ledger_pair_partial_kernel   block b adds the rows of slots [b kLedgerChunk, (b + 1) kLedgerChunk): each thread a
//                                fixed strided subset in ascending order, then a fixed LDS tree (tally_partial_kernel's
//                                scheme, det_kernels.hpp)
//   ledger_wall_partial_kernel   block (b, w) adds F_w, P_d, P_f of particles [256 b, 256 b + 256) for wall w: the
//                                partition and the tree of wall_rows_partial_kernel, so the F_w it arrives at has the bits
//                                of the force in a wall_out that started from zero
//   ledger_final_kernel          one block: the block sums in ascending order through the same tree, the walls one after
//                                the other; thread 0 forms -F_w.u_w, multiplies by dt and adds into the accumulator
// The partition depends on the slot count and the particle count only, and nothing is added with an atomic: the sums are
// bitwise reproducible, with or without the "deterministic" option.  Streaming passes over 16 B per slot and 48 B per
// (particle, wall); included by shstep_ledger.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "shpair_ctx.hpp"

namespace shp {

// sh[c][t] over t in a fixed tree, C components; the result is in sh[c][0]
template <int C>
__device__ __forceinline__ void ledger_block_tree(double (*sh)[kLedgerBlock], const int t)
{
  for (int half = kLedgerBlock / 2; half > 0; half >>= 1) {
    __syncthreads();
    if (t < half)
      for (int c = 0; c < C; ++c) sh[c][t] += sh[c][t + half];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kLedgerBlock) void ledger_pair_partial_kernel(const int np, const double* __restrict__ power,
                                                                          double* __restrict__ part)
{
  __shared__ double sh[2][kLedgerBlock];
  const int t = threadIdx.x;
  const int lo = blockIdx.x * kLedgerChunk;
  const int hi = (lo + kLedgerChunk < np) ? lo + kLedgerChunk : np;
  double s0 = 0.0, s1 = 0.0;
  for (int w = lo + t; w < hi; w += kLedgerBlock) {
    const double2 r = *(const double2*)(power + 2 * (size_t)w);
    s0 += r.x;
    s1 += r.y;
  }
  sh[0][t] = s0;
  sh[1][t] = s1;
  ledger_block_tree<2>(sh, t);
  if (t < 2) part[2 * (size_t)blockIdx.x + t] = sh[t][0];
}

// rows: [nlocal][nwalls][4] E, F_w; prows: [nlocal][nwalls][2] P_d, P_f, or null after the elastic instance (which
// dissipates nothing).  part: [nwalls][gridDim.x][kLedgerWallTerms].
__global__ __launch_bounds__(kLedgerBlock) void ledger_wall_partial_kernel(const int nlocal, const int nwalls,
                                                                          const unsigned* __restrict__ wmask,
                                                                          const double* __restrict__ rows,
                                                                          const double* __restrict__ prows, double* __restrict__ part)
{
  __shared__ double sh[kLedgerWallTerms][kLedgerBlock];
  const int t = threadIdx.x;
  const int i = blockIdx.x * kLedgerBlock + t, w = blockIdx.y;
  double v[kLedgerWallTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < nlocal && ((wmask[i] >> w) & 1u)) {
    const double* row = rows + ((size_t)i * nwalls + w) * 4;
    v[0] = row[1]; v[1] = row[2]; v[2] = row[3];
    if (prows) {
      const double* prow = prows + ((size_t)i * nwalls + w) * 2;
      v[3] = prow[0]; v[4] = prow[1];
    }
  }
  for (int k = 0; k < kLedgerWallTerms; ++k) sh[k][t] = v[k];
  ledger_block_tree<kLedgerWallTerms>(sh, t);
  if (t < kLedgerWallTerms) part[((size_t)w * gridDim.x + blockIdx.x) * kLedgerWallTerms + t] = sh[t][0];
}

// nbp block sums of the pair rows (0: no fresh pair pass), nbw per wall of the wall rows (nwalls = 0: no fresh wall
// pass); wvel: kWallVelStride (4) doubles per wall, u_w first, or null while no wall moves.  acc: kLedgerDoubles.
__global__ __launch_bounds__(kLedgerBlock) void ledger_final_kernel(const int nbp, const double* __restrict__ ppart, const int nwalls,
                                                                   const int nbw, const double* __restrict__ wpart,
                                                                   const double* __restrict__ wvel, const double dt,
                                                                   double* __restrict__ acc)
{
  __shared__ double sh[kLedgerWallTerms][kLedgerBlock];
  const int t = threadIdx.x;
  if (nbp > 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int b = t; b < nbp; b += kLedgerBlock) {
      s0 += ppart[2 * (size_t)b];
      s1 += ppart[2 * (size_t)b + 1];
    }
    sh[0][t] = s0;
    sh[1][t] = s1;
    ledger_block_tree<2>(sh, t);
    if (t == 0) {
      acc[0] += dt * sh[0][0];
      acc[1] += dt * sh[1][0];
    }
    __syncthreads();   // sh is written again below
  }
  double td = 0.0, tf = 0.0, tw = 0.0;   // thread 0: this fold's totals over the walls, in wall order
  for (int w = 0; w < nwalls; ++w) {
    double v[kLedgerWallTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = t; b < nbw; b += kLedgerBlock)
      for (int k = 0; k < kLedgerWallTerms; ++k) v[k] += wpart[((size_t)w * nbw + b) * kLedgerWallTerms + k];
    for (int k = 0; k < kLedgerWallTerms; ++k) sh[k][t] = v[k];
    ledger_block_tree<kLedgerWallTerms>(sh, t);
    if (t == 0) {
      double rate = 0.0;   // -F_w.u_w: the power the wall delivers to the bed
      if (wvel) rate = -(sh[0][0] * wvel[4 * w] + sh[1][0] * wvel[4 * w + 1] + sh[2][0] * wvel[4 * w + 2]);
      const double ed = dt * sh[3][0], ef = dt * sh[4][0], ew = dt * rate;
      double* a = acc + kLedgerTotals + kLedgerPerWall * w;
      a[0] += ed; a[1] += ef; a[2] += ew;
      td += ed; tf += ef; tw += ew;
    }
    __syncthreads();   // the next wall writes sh again
  }
  if (t == 0 && nwalls > 0) {
    acc[2] += td;
    acc[3] += tf;
    acc[4] += tw;
  }
}

}  // namespace shp
