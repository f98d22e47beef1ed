// pair_rotate.hpp — particle i's (and, for the compiled orders, particle j's) real-SH coefficients rotated into the
// pair's cap frame: in the contact kernel (cap_frame_rotate, body-frame family) or one lane per rotation in a kernel
// of its own (pair_rotate_lane_kernel), with the layout of the rotated vectors it writes (rot_*).
#pragma once
#include "contact_plan.hpp"
#include "sh_device.hpp"
#include "wave_ops.hpp"

namespace shp {

// ---- set-up: particle i's expansion in the cap frame ------------------------
// M = [b1 b2 bc]: the cap axes (e1, e2, c) in i's body frame, so that
// r_cap(u') = r_body(M u').  M = Rz(alpha) Ry(beta) Rz(gamma), Ry(beta) =
// Rx(-90) Rz(beta) Rx(90); with (O_A f)(u) = f(A u), O_{AB} = O_B O_A, hence
//   c' = Z(gamma) X Z(beta) X^T Z(alpha) c ,  X = T(Rx(+90)) (constant).
// alpha is read off the third column of M; gamma follows from the WELL
// CONDITIONED sum (cos beta >= 0) or difference (cos beta < 0) of the two
// angles, so that the 1/sin(beta) error of alpha near the poles only moves the
// axis of a vanishing tilt.
template <int L>
__device__ __forceinline__ void cap_frame_rotate(const PairParams& P, double* __restrict__ lw, const WaveLdsLayout& W,
                                                 const int LL, const int si, const int lane, const int fr_euler = FR_EULER)
{
  const int ns = (LL + 1) * (LL + 1);
  double* trig = lw + W.trig;
  double* v0 = lw + W.v0;
  double* v1 = lw + W.v1;
  // Euler angles (computed per pair by pair_setup_kernel): lanes 0,1,2 tabulate cos/sin(m angle) for alpha, beta, gamma
  if (lane < 3) {
    const double c1 = lw[fr_euler + 2 * lane], s1 = lw[fr_euler + 2 * lane + 1];
    double* t = trig + 2 * (LL + 1) * lane;
    double cm = 1.0, sm = 0.0;
    for (int m = 0; m <= LL; ++m) {
      t[2 * m] = cm;
      t[2 * m + 1] = sm;
      const double c = fma(cm, c1, -(sm * s1)), s = fma(cm, s1, sm * c1);
      cm = c;
      sm = s;
    }
  }
  wave_lds_sync();
  const double* creal = P.creal + (size_t)si * ns;
  const int XW = LL / 2 + 1;
  // five steps; step s reads `src`, writes `dst`; element e = row (l, m) of the vector
  for (int step = 0; step < 5; ++step) {
    const double* src = (step == 0) ? creal : ((step & 1) ? v0 : v1);
    double* dst = (step & 1) ? v1 : v0;
    for (int e = lane; e < ns; e += 64) {
      double out;
      if ((step & 1) == 0) {  // Z(angle): 0 alpha, 2 beta, 4 gamma
        const int inf = P.xinfo[e];
        const int l = inf & 255, mm = (inf >> 8) - l;
        const double* t = trig + 2 * (LL + 1) * (step >> 1);
        const int m = mm < 0 ? -mm : mm;
        const double self = src[e], other = src[l * l + l - mm];
        const double cm = t[2 * m], sm = t[2 * m + 1];
        out = (mm == 0) ? self : fma(cm, self, (mm > 0 ? sm : -sm) * other);
        if (step == 4) out *= P.gscale[e];
      } else {  // X^T (step 1) or X (step 3), ELL rows
        const size_t rowoff = ((size_t)(step == 1 ? ns : 0) + e) * XW;
        const double* val = P.xval + rowoff;
        const int* col = P.xcol + rowoff;
        out = 0.0;
#pragma unroll
        for (int t = 0; t < ((L >= 0) ? L / 2 + 1 : XW); ++t) out = fma(val[t], src[col[t]], out);
      }
      dst[e] = out;
    }
    wave_lds_sync();
  }
  // the rotated, scaled coefficients are now in v0
}

// The rotations as a kernel of their own (compiled orders), ONE LANE PER ROTATION.  Inside the contact kernel a
// rotation is a chain of five dependent table-load / LDS steps, ~10 000 cycles of latency for 85 instructions during
// which the wave holds its registers and LDS (a wave-per-rotation kernel measured 0.6 ms per launch at the headline
// however many waves were resident: round 2, profiles/r02_w_*).  Here a wave carries 64 rotations through the same five steps; the
// rotation is block diagonal in l, so a lane's block of 2l + 1 values lives in LDS as [element][lane] (conflict
// free) between the steps that gather (X^T, X) and in registers for those that do not (the Z turns; cos/sin(m angle) of
// the three angles sit in registers too), the X matrices are wave-uniform (scalar loads, SGPR operands) and every
// loop is wave-uniform: ~20 instructions per rotation.  The arithmetic and its order are those of cap_frame_rotate.
// Layout of the rotated vectors: TILES of 64 rotations (one wave of the rotation kernel), inside a tile block-major —
// [l-block][rotation][element of the block] — so that the 64 x (2l+1) doubles a wave produces for one l are contiguous
// and leave as full 512-byte wave stores.  (Rotation-major rows were written in 49 store instructions of scattered
// 8...104-byte runs per wave: WRITE_SIZE 1.3-1.5x the payload and a kernel bound by its own write pattern.)
// Element e = l^2 + r of rotation T sits at rot_index(L, T, l, r).  Measured (profiles/r03_u_ab_rottile.txt): rotation
// kernel 0.296 -> 0.220 ms at L = 6; the contact kernel's reads become 2L + 1 pieces per vector, which costs it more
// than the rotation kernel gains from L = 9 on (L = 12: +1.2 % per step) — there the rows stay rotation-major, padded
// to whole 64-byte lines.
__host__ __device__ constexpr bool rot_tiled(const int L) { return L <= 8; }
__host__ __device__ constexpr size_t rot_row_doubles(const int L) { return (size_t)(((L + 1) * (L + 1) + 7) & ~7); }
__host__ __device__ constexpr size_t rot_tile_doubles(const int L) { return (size_t)64 * (rot_tiled(L) ? (size_t)(L + 1) * (L + 1) : rot_row_doubles(L)); }
__host__ __device__ inline size_t rot_index(const int L, const int T, const int l, const int r)
{
  if (!rot_tiled(L)) return (size_t)T * rot_row_doubles(L) + (size_t)l * l + r;
  return (size_t)(T >> 6) * rot_tile_doubles(L) + (size_t)64 * l * l + (size_t)(T & 63) * (2 * l + 1) + r;
}
__host__ __device__ inline size_t rot_buffer_doubles(const int L, const size_t nrot) { return ((nrot + 63) / 64) * rot_tile_doubles(L); }
template <int L>
struct RotLaneLds {
  static constexpr int NB = 2 * L + 1;
  static constexpr int a() { return 0; }
  static constexpr int b() { return 0; }   // the second gather reads the block in place: a lane only ever touches its own column
  // L >= 9 (rows of the rotated vectors rotation-major in memory): the block's rows of X^T and of X wait in LDS behind
  // the column block, 2 (2l + 1)(L / 2 + 1) doubles
  static constexpr int xs() { return NB * 64; }
  static constexpr int bytes() { return 8 * (NB * 64 + (rot_tiled(L) ? 0 : 2 * NB * (L / 2 + 1))); }
};
// cos / sin(m angle), m = 1..L, of a lane's three Euler angles: registers (every index is a compile-time constant)
template <int L>
struct RotTrig {
  double c[3 * (L > 0 ? L : 1)], s[3 * (L > 0 ? L : 1)];
};
template <int L, int LB>
__device__ __forceinline__ void rotate_lane_block(const PairParams& P, double* __restrict__ sm, const int lane,
                                                  const double* __restrict__ cre, double* __restrict__ rot,
                                                  const int task0, const int ntasks, const RotTrig<L>& T)
{
  constexpr int ns = (L + 1) * (L + 1), n = 2 * LB + 1, base = LB * LB, XW = L / 2 + 1, XN = LB / 2 + 1;
  // The X matrices, their column indices and the ring scale are the same for every lane: through constant-address-space
  // pointers they are SCALAR loads into SGPRs (an SGPR can be the multiplier of a v_fma_f64).  Through the plain global
  // pointers of the argument struct the compiler emits ~220 per-lane vector loads of them per wave (the kernel also
  // stores to global memory, so it may not assume the tables unchanged).
  // Measured on the tiled layout: L = 6 rotation kernel 0.220 -> 0.149 ms; at L = 12 (244 VGPRs, 1 100 scalar loads per
  // wave) the step gets 3.9 % slower, so from L = 9 on the plain pointers stay (profiles/r03_z_ab_rot_scalar.txt).
  const auto xval = [&] { if constexpr (rot_tiled(L)) return launder_uniform(P.xval); else return P.xval; }();
  const auto gsc = [&] { if constexpr (rot_tiled(L)) return launder_uniform(P.gscale); else return P.gscale; }();
  double* A = sm + RotLaneLds<L>::a() + lane;
  double* B = sm + RotLaneLds<L>::b() + lane;
  // L >= 9 (round 4): this block's rows of X^T and X are staged in LDS by the wave (contiguous in the ELL table: row =
  // base + r) and read as broadcasts at immediate offsets, with the compile-time columns of the small orders — instead
  // of two vector loads (value, column) and six integer instructions of address arithmetic per v_fma_f64 (4 353 of the
  // L = 12 kernel's ~8 000 vector instructions per wave were 32-bit integer, 1 067 were vector memory reads).  With
  // constant addresses the compiler forwards a lane's LDS stores to its own loads, so the block lives in registers
  // (230-254 of them: two waves per SIMD as before).  L = 12: 0.926 -> 0.752 ms per launch, L = 9: 0.488 -> 0.457
  // (profiles/r04_x_rot_kernel_times.txt).  Tried on top and dropped: the trig multiples by recurrence instead of the
  // 6 L-double table (0.83 ms at two waves per SIMD; capped at three waves the kernel spills and runs 0.95 ms).
  constexpr bool XLDS = !rot_tiled(L);
  const double* xs = sm + RotLaneLds<L>::xs();
  if constexpr (XLDS) {
    double* xw = sm + RotLaneLds<L>::xs();
    for (int i = lane; i < n * XW; i += 64) {
      xw[i] = P.xval[((size_t)ns + base) * XW + i];
      xw[n * XW + i] = P.xval[(size_t)base * XW + i];
    }
    wave_lds_sync();
  }
  // Z(alpha) on the way in: the pair (l, +m), (l, -m) turns by m alpha
  A[64 * LB] = cre[base + LB];
#pragma unroll
  for (int m = 1; m <= LB; ++m) {
    const double c = T.c[0 * L + m - 1], s = T.s[0 * L + m - 1];
    const double p = cre[base + LB + m], q = cre[base + LB - m];
    A[64 * (LB + m)] = fma(c, p, s * q);
    A[64 * (LB - m)] = fma(c, q, -(s * p));
  }
  // X^T: rows ns + e of the ELL table
  double xb[n];
#pragma unroll
  for (int r = 0; r < n; ++r) {
    const size_t ro = ((size_t)ns + base + r) * XW;
    double o = 0.0;
    // the columns of row (LB, r - LB) are known at compile time (sh_const::xpat_*): immediate LDS offsets, no index loads
    // (constants once the loops are unrolled)
    const int first = sh_const::xpat_first(LB, r - LB), count = sh_const::xpat_count(LB, r - LB);
#pragma unroll
    for (int t = 0; t < XN; ++t) {
      if constexpr (rot_tiled(L)) {
        if (t < count) o = fma(xval[ro + t], A[64 * (LB + first + 2 * t)], o);
      } else {
        if (t < count) o = fma(xs[r * XW + t], A[64 * (LB + first + 2 * t)], o);   // L >= 9: X from LDS
      }
    }
    xb[r] = o;
  }
  // Z(beta), in registers
  B[64 * LB] = xb[LB];
#pragma unroll
  for (int m = 1; m <= LB; ++m) {
    const double c = T.c[1 * L + m - 1], s = T.s[1 * L + m - 1];
    const double p = xb[LB + m], q = xb[LB - m];
    B[64 * (LB + m)] = fma(c, p, s * q);
    B[64 * (LB - m)] = fma(c, q, -(s * p));
  }
  // X
#pragma unroll
  for (int r = 0; r < n; ++r) {
    const size_t ro = ((size_t)base + r) * XW;
    double o = 0.0;
    const int first = sh_const::xpat_first(LB, r - LB), count = sh_const::xpat_count(LB, r - LB);
#pragma unroll
    for (int t = 0; t < XN; ++t) {
      if constexpr (rot_tiled(L)) {
        if (t < count) o = fma(xval[ro + t], B[64 * (LB + first + 2 * t)], o);
      } else {
        if (t < count) o = fma(xs[(n + r) * XW + t], B[64 * (LB + first + 2 * t)], o);   // L >= 9: X from LDS
      }
    }
    xb[r] = o;
  }
  if constexpr (rot_tiled(L)) {
    // Z(gamma) and the ring scale, in registers; then the block leaves through LDS in ROTATION-major order (lane's row of
    // n numbers at lane n: odd stride, the plain two passes of a 64-bit write), so that consecutive lanes read — and
    // store to global memory — consecutive elements with no index arithmetic at all: element idx = lane + 64 it of the
    // tile's block is LDS cell idx.  (Read back from the column layout it was a division, a multiply and an exec-masked
    // branch per store: 490 of the kernel's 1 755 vector instructions at L = 6.)
    double* A2 = sm + RotLaneLds<L>::a() + lane * n;
    A2[LB] = xb[LB] * gsc[base + LB];
  #pragma unroll
    for (int m = 1; m <= LB; ++m) {
      const double c = T.c[2 * L + m - 1], s = T.s[2 * L + m - 1];
      const double p = xb[LB + m], q = xb[LB - m];
      A2[LB + m] = fma(c, p, s * q) * gsc[base + LB + m];
      A2[LB - m] = fma(c, q, -(s * p)) * gsc[base + LB - m];
    }
    wave_lds_sync();
    const double* At = sm + RotLaneLds<L>::a() + lane;
    double* out = rot + (size_t)(task0 >> 6) * rot_tile_doubles(L) + 64 * base + lane;
    if (task0 + 64 <= ntasks) {   // a full tile (every workgroup but the last): wave-uniform
  #pragma unroll
      for (int it = 0; it < n; ++it) out[64 * it] = At[64 * it];
    } else {
  #pragma unroll
      for (int it = 0; it < n; ++it) {
        const int idx = lane + 64 * it;   // < 64 n
        // task0 is a multiple of 64 (one tile per workgroup): cell idx is rot_index(L, task0 + idx / n, LB, idx % n)
        if (task0 + idx / n < ntasks) out[64 * it] = At[64 * it];
      }
    }
    wave_lds_sync();
  } else {
    // L >= 9 (rotation-major rows in memory, 244 vector registers: two waves per SIMD): the block leaves transposed
    // through LDS from the column layout; compile-time columns and the lane-major block push these kernels past 256
    // registers — one wave per SIMD, L = 12 / n_q = 32 2 % slower (profiles/r03_zzzzz_ab_rot.txt)
    A[64 * LB] = xb[LB] * gsc[base + LB];
  #pragma unroll
    for (int m = 1; m <= LB; ++m) {
      const double c = T.c[2 * L + m - 1], s = T.s[2 * L + m - 1];
      const double p = xb[LB + m], q = xb[LB - m];
      A[64 * (LB + m)] = fma(c, p, s * q) * gsc[base + LB + m];
      A[64 * (LB - m)] = fma(c, q, -(s * p)) * gsc[base + LB - m];
    }
    wave_lds_sync();
    const double* At = sm + RotLaneLds<L>::a();
  #pragma unroll
    for (int it = 0; it < n; ++it) {
      const int idx = lane + 64 * it;   // < 64 n
      const int tk = idx / n, r = idx - tk * n;
      if (task0 + tk < ntasks) rot[(size_t)(task0 + tk) * rot_row_doubles(L) + base + r] = At[64 * r + tk];
    }
    wave_lds_sync();
  }
  if constexpr (LB < L) rotate_lane_block<L, LB + 1>(P, sm, lane, cre, rot, task0, ntasks, T);
}
template <int L>
__global__ void __launch_bounds__(64) pair_rotate_lane_kernel(const PairParams P, double* __restrict__ rot)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_rl[];
  double* sm = (double*)smem_rl;
  const int lane = threadIdx.x;
  const int task0 = 2 * P.slot0 + blockIdx.x * 64, ntasks = 2 * P.npairs;   // slot0 is a multiple of 32: whole tiles
  const int task = task0 + lane;
  const int w = (task < ntasks ? task : ntasks - 1) >> 1, which = task & 1;
  const int* rid = P.rec_i + 4 * (size_t)w;
  const bool live = task < ntasks && rid[0] != 0;
  const int shape = live ? rid[1 + which] : 0;   // dead slots rotate shape 0 by the identity: nobody reads the result
  const double* eu = P.rec + (size_t)kRecStride * w + (which ? FR_EULERJ : FR_EULER);
  RotTrig<L> T;
  if constexpr (L >= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double c1 = live ? eu[2 * a] : 1.0, s1 = live ? eu[2 * a + 1] : 0.0;
      double cm = c1, sn = s1;
#pragma unroll
      for (int m = 1; m <= L; ++m) {
        T.c[a * L + m - 1] = cm;
        T.s[a * L + m - 1] = sn;
        const double c = fma(cm, c1, -(sn * s1)), s = fma(cm, s1, sn * c1);
        cm = c;
        sn = s;
      }
    }
  }
  rotate_lane_block<L, 0>(P, sm, lane, P.creal + (size_t)shape * ((L + 1) * (L + 1)), rot, task0, ntasks, T);
}

}  // namespace shp
