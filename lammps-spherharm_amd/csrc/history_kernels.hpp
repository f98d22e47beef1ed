// history_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.14: tangential contact springs with history for SH pairs.
//
// Every slot of a device-built list owns xi, the accumulated tangential displacement of i's contact point relative to
// j's (space frame).  Three kernels:
//   pair_history_kernel        the pair pass of dissipation_kernels.hpp with the spring: pair_slot with friction and its
//   pair_history_ledger_kernel HIST switch, which reads the HistoryParams below; the body is there.  A type
//                              pair has history iff mu_ij != 0 and k_t,ij != 0; the other type pairs take §2.11's
//                              friction as pair_slot forms it.  For a history slot that passes §2.11's guards:
//                                xi' = xi + dt v_t, less its part along S_n;  F* = -k_t xi' - gamma_t v_t;
//                                |F*| <= mu N: F_t = F*, xi <- xi';  else F_t = F* mu N / |F*|, xi <- -(F_t + gamma_t v_t) / k_t
//                              and the wrench of F_t at r_i on both bodies, as §2.11's.  Every other slot gets xi <- 0.
//                              dt = 0 forms the force from the stored xi and writes nothing back.  One lane per slot,
//                              one owner per xi: no atomics on it.
//   history_key_kernel         after a build: one int per slot, the tag of j's owner (what survives a rebuild; the
//                              list is built with tag_i < tag_j, so i never swaps with j)
//   history_carry_kernel       one lane per NEW slot (i, key): scans the OLD row i for the key, copies its xi or writes 0
// xi is three planes of `stride` doubles (stride = the list's slot count): the 64 lanes of a wave load 64 consecutive
// doubles of a plane, one 512 B request each, where [slot][3] would stride the lanes by 24 B.
// Streaming kernels bound by HBM.  Included by shstep_dissipation.hip only, behind dissipation_kernels.hpp (the
// kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "dissipation_kernels.hpp"

namespace shp {

struct HistoryParams {
  FrictionParams q;        // q.d.gamma, q.mu and q.gamma_t may be null: no coefficient of the kind was ever set
  const double* kt;        // (ntypes+1)^2, like mu
  double* xi;              // [3][stride]
  size_t stride;
  double dt;               // 0: a look, xi is not written
};

__global__ __launch_bounds__(kDampBlock) void pair_history_kernel(const HistoryParams H)
{
  pair_slot<true, false, true>(H.q.d, H.q, H);
}

__global__ __launch_bounds__(kDampBlock) void pair_history_ledger_kernel(const HistoryParams H)
{
  pair_slot<true, true, true>(H.q.d, H.q, H);
}

// key[w] = the tag of j's owner.  With tags, a ghost row holds its owner's (shstep_borders_device copies it, and a
// host's own ghost rows carry theirs); without, the tag is the row index and a ghost's owner is in gowner — the two
// cases of half_list_kernel, which built the list from the same arrays.
__global__ __launch_bounds__(kDampBlock) void history_key_kernel(const int np, const int nlocal, const int* __restrict__ pair_j,
                                                                 const int* __restrict__ tag, const int* __restrict__ gowner,
                                                                 int* __restrict__ key)
{
  const size_t w = (size_t)blockIdx.x * kDampBlock + threadIdx.x;
  if (w >= (size_t)np) return;
  const int j = pair_j[w];
  key[w] = tag ? tag[j] : (j < nlocal ? j : gowner[j - nlocal]);
}

// Rows are a dozen entries: a linear scan of the old row.  A periodic edge is at least twice the ghost cutoff (SPEC
// §7), so a row holds an owner's tag at most once.
__global__ __launch_bounds__(kDampBlock) void history_carry_kernel(const int np, const int* __restrict__ pair_i,
                                                                   const int* __restrict__ key, const int* __restrict__ old_offs,
                                                                   const int* __restrict__ old_key, const double* __restrict__ old_xi,
                                                                   const size_t old_stride, double* __restrict__ xi, const size_t stride)
{
  const size_t w = (size_t)blockIdx.x * kDampBlock + threadIdx.x;
  if (w >= (size_t)np) return;
  const int i = pair_i[w], k = key[w];
  double a[3] = {0.0, 0.0, 0.0};
  for (int p = old_offs[i], e = old_offs[i + 1]; p < e; ++p)
    if (old_key[p] == k) {
      a[0] = old_xi[p];
      a[1] = old_xi[old_stride + p];
      a[2] = old_xi[2 * old_stride + p];
      break;
    }
  xi[w] = a[0];
  xi[stride + w] = a[1];
  xi[2 * stride + w] = a[2];
}

}  // namespace shp
