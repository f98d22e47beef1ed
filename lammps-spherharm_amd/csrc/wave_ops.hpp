// wave_ops.hpp — wave and LDS primitives of the pair kernels (16-byte LDS reads, scalar wave votes, laundered
// values, late kernel arguments, wave / pair synchronisation) and the Newton-Raphson maths (rsqrt, sqrt, rcp, pow).
#pragma once
#include "pair_params.hpp"

namespace shp {

// 16-byte LDS reads.  Rows of the ring tables and of particle j's table are 16-byte aligned (wave_lds_layout), but the
// compiler only knows that a double* is 8-byte aligned and reads adjacent doubles with ds_read2_b64 — two 8-byte
// accesses per lane, serviced at HALF the rate of ds_read_b128 (128 against 256 B/clk/CU) and banked modulo 32 instead
// of 64 dwords, where the 36-dword row stride of particle j's table (chosen for ds_read_b128) puts rows l and l + 8 on
// the same banks.  Measured on the round-2 kernel (profiles/r03_b_lds_sites.txt): 9 LDS-array cycles per LDS
// instruction in the node loops, 27 % of them bank conflicts, the LDS pipe 83 % busy beside an 80 % busy VALU.
typedef double v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2d lds2(const double* p) { return *(const v2d*)__builtin_assume_aligned(p, 16); }

// Integer products of the node loops through the 24-bit multiplier (v_mul_u32_u24 / v_mul_i32_i24: full rate;
// v_mul_lo_u32 is a quarter-rate instruction).  Operands are node, ring and azimuth indices (< 2^15) and the
// multiply-shift constants (< 2^24).  Only the JPT kernels take it: in four forces-only body-frame kernels the changed
// instruction mix tips the register allocator into 2-4 spills.
template <bool ON>
__device__ __forceinline__ unsigned umul_sel(const unsigned a, const unsigned b) { return ON ? __umul24(a, b) : a * b; }
template <bool ON>
__device__ __forceinline__ int mul_sel(const int a, const int b) { return ON ? __mul24(a, b) : a * b; }

// Wave votes as SCALAR mask arithmetic.  HIP's __any() goes through a 0 / 1 value per lane (v_cndmask + v_cmp, two
// vector instructions per vote) and boolean algebra on lane predicates is materialised the same way; a ballot is the
// compare's own SGPR pair, masks combine on the scalar unit, and lane_of() hands a mask back as a lane predicate
// (s_and_saveexec on the mask itself).
// (the HIP wrappers __ballot / __any take an int: the predicate is first turned into 0 / 1 per lane and compared again)
__device__ __forceinline__ unsigned long long wave_ballot(const bool p) { return __builtin_amdgcn_ballot_w64(p); }
// wave_any: the mask passes through an (empty) scalar asm operand — compared directly, LLVM turns `ballot != 0` back into
// the 0 / 1-per-lane idiom (v_cndmask + v_cmp + branch on vccz); through the operand it is s_cmp_lg_u64 + a scalar branch
// (SCALAR = false, the plain comparison: the body-frame kernels, which have no scalar register to spare for it)
template <bool SCALAR = true>
__device__ __forceinline__ bool mask_any(unsigned long long m)
{
  if constexpr (SCALAR) asm("" : "+s"(m));
  return m != 0ULL;
}
template <bool SCALAR = true>
__device__ __forceinline__ bool wave_any(const bool p) { return mask_any<SCALAR>(__builtin_amdgcn_ballot_w64(p)); }
__device__ __forceinline__ bool lane_of(const unsigned long long mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }

__device__ __forceinline__ unsigned launder_s32(unsigned v)   // ... of a wave-uniform value: it stays in a scalar register
{
  asm volatile("" : "+s"(v));
  return v;
}
__device__ __forceinline__ unsigned launder_u32(unsigned v)
{
  asm volatile("" : "+v"(v));
  return v;
}

// The lane index, made where it is asked for.  Anything derived from threadIdx is invariant everywhere: addresses the
// epilogue computes from it (lane * 8 as a 64-bit offset, ...) are merged with the prologue's and then carried —
// or spilled — through the node loops, where registers are scarcest.  Two instructions.
__device__ __forceinline__ int fresh_lane()
{
  int v;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(v));
  return v;
}

// The kernel's arguments, read where they are used.  A by-value argument struct is loaded from the kernarg segment in
// the entry block; the epilogue's sixteen pointers and flags (f, torque, pair_i, pair_j, type, kn, ...) would then sit
// in ~30 scalar registers through the node loops, where the coefficient windows of sh_eval need them: the allocator
// parks them in lanes of a vector register and restores eight of them in EVERY iteration of the root loop and of the
// slab loop (v_readlane, ~330 vector instructions per pair at L = 6).  Reading them through a kernarg pointer the
// compiler cannot see through makes them plain scalar loads at the point of use.
typedef const PairParams __attribute__((address_space(4))) LateParams;
__device__ __forceinline__ LateParams* late_params()
{
  unsigned long long a = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return (LateParams*)a;
}

__device__ __forceinline__ void wave_lds_sync()
{
  // LDS written by some lanes of the wave, read by others: DS operations of one
  // wave execute in order, so only the compiler has to be kept from reordering.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ... and between the waves of a pair (WPP = 2): a workgroup barrier
template <int WPP>
__device__ __forceinline__ void pair_sync()
{
  if constexpr (WPP == 1) wave_lds_sync();
  else __syncthreads();
}

// 1/sqrt(x) to the last ulp or two: v_rsq_f64 (2^-26) + two Newton steps.
// Half the VALU work of sqrt() followed by a division.
__device__ __forceinline__ double rsqrt_nr(const double x)
{
  double y = __builtin_amdgcn_rsq(x);
  double h = fma(-x * y, y, 1.0);
  y = fma(y * 0.5, h, y);
  h = fma(-x * y, y, 1.0);
  y = fma(y * 0.5, h, y);
  return y;
}

// The same with ONE Newton step: from v_rsq_f64's 2^-26 the step leaves 3/2 (2^-26)^2 = 3.3e-16 plus its own
// rounding, i.e. 2-3 ulp.  Used where the root only normalises a direction or feeds a residual that is compared
// with tolerances of 1e-7 and more (node loops: 4 VALU instructions fewer per radius evaluation).
__device__ __forceinline__ double rsqrt_nr1(const double x)
{
  double y = __builtin_amdgcn_rsq(x);
  const double h = fma(-x * y, y, 1.0);
  y = fma(y * 0.5, h, y);
  return y;
}

// sqrt(x) for x >= 0 as x * rsqrt(x): a third of the VALU work of the IEEE sqrt() expansion
// (which rescales, iterates and fixes up special cases), accurate to the last ulp or two.
__device__ __forceinline__ double sqrt_nr(const double x) { return (x > 0.0) ? x * rsqrt_nr(x) : 0.0; }

// sqrt(x) with the one-step root: 2-3 ulp.  For the brackets, first iterate and end-point residual of the inner-radius
// search and wherever else 1e-15 relative is far inside what the value is used for.
// (x <= 0 and NaN give 1e-150 for 0: one v_max_f64 — written as such, fmax() adds a canonicalising v_max_f64 under IEEE
// mode — instead of a compare and two selects)
__device__ __forceinline__ double max_raw(const double x, const double c)
{
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(c));
  return r;
}
template <bool CLAMP = false>
__device__ __forceinline__ double sqrt_nr1(const double x)
{
  if constexpr (CLAMP) {
    const double t = max_raw(x, 1e-300);
    return t * rsqrt_nr1(t);
  } else {
    return (x > 0.0) ? x * rsqrt_nr1(x) : 0.0;   // (the body-frame kernels have no register for the constant)
  }
}

// 1/d to the last ulp or two: v_rcp_f64 + two Newton steps (5 VALU ops instead of
// the ~12 of an IEEE division); 0 and denormals give inf/NaN, which the callers test.
__device__ __forceinline__ double rcp_nr(const double d)
{
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  return r;
}

// 1/d with ONE Newton step: v_rcp_f64's 2^-26 squared is 2^-52, plus the step's own rounding: 2-3 ulp.
__device__ __forceinline__ double rcp_nr1(const double d)
{
  const double r = __builtin_amdgcn_rcp(d);
  return fma(fma(-d, r, 1.0), r, r);
}

// V^e for the exponents the force law usually asks for (m - 1 or m a multiple of 1/4) by square
// roots: ~25 VALU instructions instead of the ~150 of pow(); the whole wave issues them for lane 0.
__device__ __forceinline__ double pow_quarter(const double v, const double e)
{
  if (e == 0.25) return sqrt_nr(sqrt_nr(v));
  if (e == 0.5) return sqrt_nr(v);
  if (e == 0.75) { const double s = sqrt_nr(v); return s * sqrt_nr(s); }
  if (e == 1.0) return v;
  if (e == 1.25) return v * sqrt_nr(sqrt_nr(v));
  if (e == 1.5) return v * sqrt_nr(v);
  if (e == 2.0) return v * v;
  return pow(v, e);
}

}  // namespace shp
