// contact_plan.hpp — the contact kernel's launch plan (plan_contact: which instance runs, with what sizes) and the
// LDS layout it is sized by.  Header-only plain C++: the CPU tests compile it with g++ (tests/test_contact_plan.py), and
// since it is compiled into every translation unit with the same flags, the knobs of `make variant` (SHP_LDS_PAD,
// SHP_ALIAS_FROM_L) move the host's plan and the kernels' layout together.
#pragma once
#include <cstdio>

#include "../../include/shpair.h"
#include "sh_const.hpp"

namespace shp {

constexpr int kMaxUnrolledL = 12;   // orders with compiled kernels (pair_kernels_L*.o); above, the run-time-order kernel
constexpr int kMaxWavesPerBlock = 4;
// ---- per-wave dynamic LDS (doubles unless noted) ---------------------------
//   frame[kFrame]        pair frame, FR_* (pair_params.hpp)
//   trig[6 (L+1)]        cos/sin of m alpha, m beta, m gamma
//   v0[(L+1)^2], v1[..]  ping-pong coefficient vectors of the rotation
//   ring[rows][L+1][4]   A_km, B_km, dA/dmu, dB/dmu of `rows` consecutive rings; the two B slots
//                        of m = 0 (identically zero) carry mu_k and sigma_k.  rows = nq when that
//                        leaves the CU enough waves, else the cap is processed in ring groups.
//   qri[n], qrj[n], qp[n] (16-bit)   queue of inside nodes, n = kQueue (body-frame and weighted kernels: a ring buffer)
//                        or queue_capacity() (per-azimuth kernels: a stack)
constexpr int kQueue = 128;  // entries: a slab of 64 nodes adds <= 64 to a queue holding < 64 (the per-azimuth kernels' slabs
                             // are 64 node PAIRS: see queue_capacity)
constexpr int kFrame = 40;
constexpr int kRedStride = 72;    // epilogue reduction: doubles between the 64-entry rows of the seven sums (64 + 8: rows
                                  // four apart share banks, not all seven)
constexpr int kRedDoubles = 7 * kRedStride + 56 + 7 + 6;   // scratch of the epilogue behind the frame
// The per-azimuth kernels keep only the slots they read from LDS — E1 ... WSC (12..29) and RHO, KN, EXPO, IJ (36..39):
// the Euler angles are the rotation kernel's, the pair's scalars arrive as scalar loads — packed to the front: 22
// doubles instead of 40.  LDS is allocated in granules of 1 280 B (profiles/r04_ac_lds_granule.txt); the 128 B put
// L = 7 / n_q = 16 and L = 10 / n_q = 16 a granule lower (18 instead of 16, 14 instead of 12 waves per CU).
constexpr int kFrameJ = 24;
#ifndef SHP_ALIAS_FROM_L
#define SHP_ALIAS_FROM_L 7
#endif
struct WaveLdsLayout {
  int trig, v0, v1, ring, qri, qrj, qp, bytes;  // offsets in doubles (qp: in doubles too), total bytes
  int qw;                                        // weighted rule only: the queued nodes' weights
  int coef;                                      // end of the queue region (the table of particle j starts here)
  int pj, gh;                                    // particle j's polynomials: first-stage scratch, per-azimuth table
  int tr;                                        // even L: (cos, sin)(psi_l), l < n_q, 2 doubles each, behind the table's rows
  int pi, v0i;                                   // JPT kernels: particle i's first-stage polynomials PJ^i (they stay for every ring
                                                 // group); particle i's rotated vector beside particle j's (both in the rows of
                                                 // the per-azimuth table, which is built after the first stage has read them)
  int glw;                                       // JPT kernels: the Gauss-Legendre weights (nqj doubles)
  int park;                                      // JPT kernels with ring groups: 2 x 64 sums parked around the builds of the later groups (in the empty queue)
  int stash;                                     // JPT kernels: 64 prefetched Gauss nodes for the first pass of the first ring build
  int qstride;                                   // two waves per pair: doubles between the waves' private queue regions
  int qcap;                                      // JPT kernels: entries of the node queue (kQueue ... kQueue + 64, see queue_capacity)
};
constexpr int kLdsGranule = 1280;                // bytes: a workgroup's LDS is allocated in 1/128 of the CU's 160 KB
// Row of the per-azimuth table: G_l (L + 1 coefficients, descending powers), H_l (L), cos(psi_l), sin(psi_l) (the
// higher orders follow by the angle-addition recurrence where r_i is evaluated), the Gauss-Legendre weight of the
// RING with the row's index (n_q rows, n_q rings: the table doubles as the weight table), then padding to 16-byte
// rows whose stride is 2 mod 4 doubles: sixteen lanes reading sixteen rows with ds_read_b128 then spread over all
// banks (a 128-byte stride, 2L + 4 = 16 at L = 6, puts every row on the same banks: the kernel ran 3x slower).
// Round 4: for EVEN L the 2L + 1 coefficients and the weight are 2L + 2 doubles — already 2 mod 4 — and (cos, sin)(psi_l)
// live in an array of their own behind the rows (jpoly_trig_sep; W.tr): 4 doubles per row less than the padded
// 2L + 6.  For odd L the row of 2L + 4 doubles holds all of it, as before.
SHP_HD constexpr bool jpoly_trig_sep(const int L) { return (L % 2) == 0; }
SHP_HD constexpr int jpoly_row(const int L) { return jpoly_trig_sep(L) ? 2 * L + 2 : 2 * L + 4; }
SHP_HD constexpr int jpoly_trig(const int L) { return 2 * L + 2; }   // odd L: offset of cos(psi_l) in a row; sin follows (one 16-byte pair)
SHP_HD constexpr int jpoly_glw(const int L) { return 2 * L + 1; }    // offset of the weight of ring `row index` (the odd slot behind the 2L + 1 coefficients)
// Rows of the first-stage table PJ: (order m, part) for m = 0..L+1 — the order L + 1 is empty (zeros), see jpoly_build.
SHP_HD constexpr int jpoly_rows(const int L) { return 2 * L + 4; }
// ... of which particle i needs the real orders only: PJ^i, (2L + 2) polynomials of L + 1 coefficients (an even count)
SHP_HD constexpr int jpoly_pi_doubles(const int L) { return (2 * L + 2) * (L + 1); }
SHP_HD constexpr WaveLdsLayout wave_lds_layout(const int L, const int rows, const bool weighted = false,
                                               const int nqj = 0, const int qcap = kQueue)
{
  WaveLdsLayout w{};
  const int ns = (L + 1) * (L + 1);
  // frame | [rotation scratch] | rotated coefficients v0 | ring rows | queue.  The scratch of the coefficient
  // rotation (the Euler trig tables and the second work vector v1) is dead before the first node is queued.  From
  // L = 7 on it lies over the queue, which leaves room for more resident ring rows (L = 12, n_q = 32: +3 %); up to
  // L = 6 it keeps its own place: the wave count is limited elsewhere there (A/B: no gain from 24 instead of 21
  // waves per CU) and the separate layout compiles without a spill under the 80-VGPR bound.
  // Compiled orders (nqj > 0): the rotations run in pair_rotate_kernel; frame | v0 | ring rows | queue | per-azimuth
  // polynomials of particle j.
  const bool alias = SHP_ALIAS_FROM_L <= L;
  w.trig = kFrame;
  w.pi = w.v0i = 0;
  // JPT kernels (nqj > 0), round 4: the ring tables are Horner evaluations of particle i's first-stage polynomials
  // PJ^i (cap_frame_rings_poly), (2L + 2)(L + 1) doubles that replace the rotated vector as what has to survive for the
  // ring builds.  With all rings resident (one ring group) they lie over the queue, which is empty while rings are
  // built; with ring groups they keep a place of their own behind the frame.  Both rotated vectors wait for the first
  // stage in the rows of particle j's table.
  const int npi = jpoly_pi_doubles(L);
  const bool one_group = nqj > 0 && rows >= nqj;
  w.v0 = (alias || nqj > 0) ? kFrame : w.trig + 6 * (L + 1);
  w.v1 = w.v0 + ns;
  w.ring = (nqj > 0) ? (one_group ? kFrameJ : kFrameJ + npi) : (alias ? w.v0 + ns : w.v1 + ns);
  w.ring += w.ring & 1;  // 16-byte aligned rows for ds_read_b128
  // the first stage of particle j's polynomials ((2L+4)(L+1) doubles, +2: a read one past a row's end) lies over the ring rows, which are built later
  int ringsz = 4 * rows * (L + 1);
  if (nqj > 0 && rows > 0 && ringsz < jpoly_rows(L) * (L + 1) + 2) ringsz = jpoly_rows(L) * (L + 1) + 2;
  w.pj = w.ring;
  w.qcap = qcap;   // (a multiple of 4: the 16-bit node indices end on an 8-byte boundary)
  w.qri = w.ring + ringsz;
  w.qrj = w.qri + qcap;
  w.qp = w.qrj + qcap;
  w.qw = w.qp + qcap / 4;
  w.park = w.qri;
  w.coef = w.qw + (weighted ? qcap : 0);
  w.stash = w.qri + 128;
  if (nqj > 0) {
    // PJ^i over the queue (one ring group: a single build, before any sum exists — nothing is parked) or behind the
    // frame (ring groups: the later builds park two sums in the empty queue).  The prefetched Gauss nodes of the first
    // pass wait at the end of the ring rows where the first pass (entries 0..63 = doubles 0..255) does not write and
    // particle j's first stage does not reach, else behind the polynomials / the parked sums.
    w.pi = one_group ? w.qri : kFrameJ;
    w.park = w.qri;
    const int pjsz = jpoly_rows(L) * (L + 1) + 2;
    if (ringsz - 64 >= 256 && ringsz - 64 >= pjsz) w.stash = w.ring + ringsz - 64;
    else w.stash = one_group ? w.pi + npi : w.qri + 128;
    int need = one_group ? w.pi + npi : w.park + 128;
    if (w.stash >= w.qri && w.stash + 64 > need) need = w.stash + 64;
    if (need > w.coef) w.coef = need;   // large L: the polynomials are longer than the queue
  }
  if (alias && nqj == 0) {
    w.trig = w.qri;
    w.v1 = w.trig + 6 * (L + 1);
    if (w.v1 + ns > w.coef) w.coef = w.v1 + ns;  // large L: the scratch is longer than the queue
  }
  w.coef += w.coef & 1;
  w.gh = w.coef;   // per-azimuth polynomials of particle j: nqj rows, resident for the whole pair
  w.glw = w.gh + jpoly_glw(L);   // weight of ring k at glw + k * jpoly_row(L)
  int ghsz = nqj * jpoly_row(L);
  w.tr = w.gh + ghsz;   // (even L; 16-byte aligned: rows are an even number of doubles)
  if (nqj > 0) {
    if (jpoly_trig_sep(L)) ghsz += 2 * nqj;
    w.v0 = w.gh;         // particle j's rotated vector, then particle i's behind it: read by the first stage only
    w.v0i = w.gh + ns;
    if (ghsz < 2 * ns) ghsz = 2 * ns;
  }
  w.bytes = 8 * (w.gh + ghsz);
  // the epilogue's reduction scratch lies behind the frame, over everything that is dead by then
  if (w.bytes < 8 * ((nqj > 0 ? kFrameJ : kFrame) + kRedDoubles)) w.bytes = 8 * ((nqj > 0 ? kFrameJ : kFrame) + kRedDoubles);
  w.bytes = (w.bytes + 15) & ~15;
#ifdef SHP_LDS_PAD   // experiment builds only (make variant): what do fewer resident waves cost?
  if (nqj > 0) w.bytes += SHP_LDS_PAD;
#endif
  w.qstride = 0;
  return w;
}
// TWO WAVES PER PAIR (template parameter WPP = 2 of pair_contact_azimuth_kernel): the workgroup is one pair, the
// tables — frame, particle i's rotated vector, the ring rows, particle j's per-azimuth polynomials — are shared and
// built by all 128 lanes, each wave classifies and integrates HALF of the azimuths (wave h the node pairs l, l + n_q
// with h n_q / 2 <= l < (h + 1) n_q / 2) with a node queue of its own.  For the orders and rules where one wave's
// private copy of the tables leaves a CU too few waves: L = 12, n_q = 32 needs 14.6 KB per one-wave pair (11 waves per
// CU, VALU 66 % busy, profiles/r03_e_L12_pmc.txt), 17.3 KB per two-wave pair (18 waves' worth; the registers allow 16).
//   frame | PJ^i (particle i's first-stage polynomials; stay for the ring groups) | ring rows (first: first stage of j's table) | j's table |
//   [epilogue scratch of both waves over everything behind the frame] | queue of wave 0 | queue of wave 1
constexpr int kRedPerWave = (7 * kRedStride + 56 + 7 + 6 + 1) & ~1;   // epilogue scratch of one wave, even
SHP_HD constexpr WaveLdsLayout pair_lds_layout2(const int L, const int rows, const int nq, const int qcap = kQueue)
{
  WaveLdsLayout w{};
  const int ns = (L + 1) * (L + 1);
  w.trig = w.v1 = w.qw = w.coef = 0;   // not used by the JPT kernels
  w.pi = kFrameJ;                       // particle i's first-stage polynomials: they stay for the ring groups
  w.ring = w.pi + jpoly_pi_doubles(L);
  w.ring += w.ring & 1;
  int ringsz = 4 * rows * (L + 1);
  if (ringsz < jpoly_rows(L) * (L + 1) + 2) ringsz = jpoly_rows(L) * (L + 1) + 2;
  ringsz += ringsz & 1;
  w.pj = w.ring;
  w.gh = w.ring + ringsz;
  w.glw = w.gh + jpoly_glw(L);
  w.v0 = w.gh;        // both rotated vectors wait for the first stage in the rows of particle j's table
  w.v0i = w.gh + ns;
  int ghsz = nq * jpoly_row(L);
  w.tr = w.gh + ghsz;
  if (jpoly_trig_sep(L)) ghsz += 2 * nq;
  if (ghsz < 2 * ns) ghsz = 2 * ns;
  int shared_end = w.gh + ghsz;
  // the epilogue's scratch (one block per wave) lies over everything behind the frame, the queues included: wave 0's
  // from the frame on, wave 1's at the end of the pair's LDS
  const int qs = 2 * qcap + qcap / 4;
  w.qcap = qcap;
  if (shared_end + 2 * qs < kFrameJ + 2 * kRedPerWave) shared_end = kFrameJ + 2 * kRedPerWave - 2 * qs;
  shared_end += shared_end & 1;
  w.qri = shared_end;
  w.qrj = w.qri + qcap;
  w.qp = w.qrj + qcap;
  w.park = w.qri;                          // 2 x 64 parked sums while the ring rows of a later group are built (the queue is empty then)
  w.stash = w.qri + 128;                   // (not used: two-wave kernels request their Gauss nodes where they use them)
  w.qstride = qs;                          // 288 at 128 entries
  w.bytes = (8 * (shared_end + 2 * w.qstride) + 15) & ~15;
  return w;
}
// Entries of the node queue of the per-azimuth kernels.  A slab of node pairs brings up to 128 inside nodes to a queue
// that holds fewer than 64: 128 entries overflow when a dense slab meets a leftover (the slab is then classified a second
// time after a short batch: 0.74 slabs per pair at the headline, 5 % of the kernel's instructions), 191 never do.  The
// LDS of a workgroup is allocated in granules of 1 280 bytes: the queue takes what the layout leaves of its last granule
// (18 bytes per entry; `waves` = queues in the workgroup's LDS), at no cost in resident waves.
SHP_HD constexpr int queue_capacity(const int bytes_at_128, const int waves)
{
  const int slack = (bytes_at_128 + kLdsGranule - 1) / kLdsGranule * kLdsGranule - bytes_at_128;
  int extra = (slack / (18 * waves)) & ~3;
  if (extra > 64) extra = 64;
  return kQueue + extra;
}
// Orders for which the two-waves-per-pair kernels are compiled (the rule that picks them: contact_split)
SHP_HD constexpr bool split_compiled(int L) { return L >= 7; }

// Specialised instances (round 5).  n_q, the resident ring rows and the queue capacity are launch parameters of the
// per-azimuth kernels: every node's (ring, azimuth) comes out of a multiply-shift division by 2 n_q or n_q, every row
// address out of a multiplication by the row length, every ring-group bound out of a compare with the group size.
// With the three as compile-time constants the divisions become shifts and masks, the products immediates, the
// one-group case loses its group loop: -4.3 % at the headline with the same arithmetic and per-pair results equal to
// 1e-13 (profiles/r05_ab_nq_const.txt, an experiment build with the constants forced).  One instance per compiled
// order, for the (n_q, rows, queue) the planner picks at that order's BASELINE shape — PairSpec<L> — launched when a
// plan is exactly that (ContactPlan::spec; option "spec" 0 keeps the general kernels, which every other (L, n_q) runs
// anyway).  The static_asserts below and tests/test_contact_plan.py hold PairSpec to the planner.
template <int L> struct PairSpec { static constexpr int nq = 0, rr = 0, qc = 0, wpp = 1; };
template <> struct PairSpec<4> { static constexpr int nq = 10, rr = 10, qc = 128, wpp = 1; };    // configs[0]'s shape
template <> struct PairSpec<6> { static constexpr int nq = 16, rr = 16, qc = 172, wpp = 1; };    // configs[1], [2], [3]
template <> struct PairSpec<12> { static constexpr int nq = 32, rr = 12, qc = 148, wpp = 2; };   // configs[4]

template <int L>
SHP_HD constexpr bool pair_spec_is(const int nq, const int rows, const int qcap, const int wpp)
{
  return PairSpec<L>::nq > 0 && nq == PairSpec<L>::nq && rows == PairSpec<L>::rr && qcap == PairSpec<L>::qc && wpp == PairSpec<L>::wpp;
}

// The options of include/shpair.h the plan reads (shpair_set_option), at their defaults.
struct ContactOptions {
  int variant = 0, rule = 0, jpoly = -1, split = -1, ring_rows = 0, waves_per_block = 0, spec = 1;
  int queue_slack = 1;   // (diagnostic) the node queue of the per-azimuth kernels takes the rest of its last LDS granule
};

struct ContactPlan {
  bool compiled = false;     // an unrolled order's kernels (L <= kMaxUnrolledL, option "variant" not 1), else the run-time-order kernel
  int family = 0;            // 0: particle j in its body frame (Horner); 1: per-azimuth polynomials in the pair's frame
  int waves_per_pair = 1;    // 2: two waves share a pair's tables (pair_lds_layout2)
  int ring_rows = 0;         // quadrature rings whose tables are resident at a time
  int qcap = kQueue;         // entries of a wave's node queue
  int lds_bytes = 0;         // dynamic LDS of one pair (of both waves when waves_per_pair = 2)
  int waves_per_block = 1;   // pairs per workgroup (one-wave kernels)
  bool spec = false;         // the PairSpec<L> instance runs
  bool weighted = false;     // the covered-fraction rule (SPEC §2.8)
};

// Which kernel family evaluates particle j (pair_kernel.hpp): per-azimuth polynomials in the pair's common frame
// (JPT kernels + rotation kernel) or the body-frame Horner evaluation.  The first trades ~170 instructions and a
// table build per pair for 60 fewer per radius evaluation: it wins unless a pair has very few cap nodes.  Option
// "jpoly": 1 / 0 force, -1 (default) the measured rule (interleaved A/B over L = 0..12 x n_q = 4..32,
// profiles/r02_y_jpoly_matrix.txt: the body-frame family was faster only at n_q = 4 from L = 6 and at n_q <= 8 from L = 9;
// re-measured in round 4, below).
SHP_HD constexpr int contact_family(const int L, const int nq, const ContactOptions& o)
{
  if (L > kMaxUnrolledL || o.variant == 1 || o.rule) return 0;
  if (o.jpoly >= 0) return o.jpoly == 1 ? 1 : 0;
  // Round 4 (end-of-round kernels, profiles/r04_q6_jpoly_small_nq.txt, r04_q6_jpoly_tiny_nq.txt): the per-azimuth family
  // has caught up everywhere but at L >= 10 with n_q <= 5 (L = 12 / 4 +3 %, L = 11 / 5 +3 %, L = 12 / 1 +16 %) — round 2's
  // rule kept the body-frame kernels at n_q < 6 from L = 6 and at n_q < 12 from L = 9, where they now lose by 5...28 %
  // (L = 9 / 10 3.10 -> 2.24 ms, L = 12 / 10 4.41 -> 3.29, L = 8 / 4 1.90 -> 1.55, L = 6 / 4 1.25 -> 1.09)
  if (L >= 10) return nq >= 6 ? 1 : 0;   // (L = 10 / 3, 4, 5: the body-frame kernels 3.5...4.5 % faster, r04_q7_sweep4.txt)
  return 1;
}

// Two waves per pair (pair_lds_layout2): the JPT kernels of the orders it is compiled for, even n_q.  Pays where one
// wave's private copy of the tables leaves a CU too few waves for its dependent FP64 chains — large L with large n_q
// (L = 12, n_q = 32: 14.6 KB per one-wave pair = 11 waves per CU, 17.3 KB per two-wave pair = the 16 the registers
// allow).  Option "split": 1 / 0 force, -1 (default) the measured rule (profiles/r03_*_split_matrix.txt).
SHP_HD constexpr bool contact_split(const int L, const int nq, const ContactOptions& o, const bool jpoly)
{
  if (!jpoly || !split_compiled(L) || L > kMaxUnrolledL || (nq & 1) || nq < 8) return false;
  if (o.split >= 0) return o.split == 1;
  // measured (interleaved A/B over L = 7..12 x n_q = 8..32, profiles/r03_g/h_split_matrix.txt and, on the end-of-round
  // kernels with their ring groups re-sized, r03_fin_split_matrix.txt; the boxes' noise is +-3 %): two waves win at
  // n_q = 32 from L = 8 on (0...-7 %), at n_q = 24 from L = 11 on (-3 %; L = 10: +2.5 %) and at L = 12 from n_q = 16
  // on (-11 %); they lose below (at n_q = 8 half of each wave's lanes have no node pair: +40 %)
  // Round 4, end-of-round kernels (Horner ring tables, larger node queue, direct batches; profiles/r04_q5_sweep2.txt):
  // with all 16 rings resident one wave beats two at L = 12 / n_q = 16 (-4.9 %), and one wave with 8-ring groups at
  // L = 11 / n_q = 24 (-4.9 %); two waves keep n_q >= 32 from L = 8 (L = 9 / 32 -4.8 %) and L = 12 from n_q = 18
  // (L = 12 / 20 -5.7 % against the best one-wave form)
  // ... and, from L = 9, n_q >= 22 where one wave's ring groups cannot end on slab boundaries (n_q = 22, 26, 28, 30; not
  // 24): L = 11 / 22 -13 %, L = 9 / 26 -7.7 %, L = 9 / 28 -6.1 %, L = 11 / 26 -5.0 %, L = 10 / 22 -4.2 %
  // (profiles/r04_q7_sweep4.txt)
  int g = 64, a = nq;
  while (a) { const int t = g % a; g = a; a = t; }   // gcd(64, n_q): a one-wave slab spans 64 / g rings
  const bool aligned1 = 2 * (64 / g) <= nq;
  return (L >= 8 && nq >= 32) || (L >= 12 && nq >= 18) || (L >= 9 && nq >= 22 && !aligned1);
}

// gfx950: 512 VGPRs per SIMD lane in blocks of 8, at most 8 waves per SIMD
SHP_HD constexpr int waves_per_simd_by_vgprs(const int vgprs)
{
  const int w = 512 / (((vgprs + 7) / 8) * 8);
  return w > 8 ? 8 : (w < 1 ? 1 : w);
}

// The launch plan at order L with n_q nodes per cap direction.  split_vgprs: VGPRs of the order's general two-wave kernel
// (pair_contact_azimuth_kernel<L, true, 2>; 0 if unknown), which sizes the ring groups of two-wave pairs.  Returns
// SHPAIR_OK, or SHPAIR_ELMAX with the reason in msg when no kernel can run the shape.
constexpr int plan_contact(const int L, const int nq, const ContactOptions& o, const int split_vgprs, ContactPlan& p,
                           char* msg = nullptr, const int msglen = 0)
{
  const bool jpoly = contact_family(L, nq, o) == 1;
  const bool split = contact_split(L, nq, o, jpoly);
  const int nqj = jpoly ? nq : 0;   // rows of the per-azimuth table in a wave's LDS
  // Resident ring rows: all nq if a wave then needs <= 8 KB of LDS (five 4-wave workgroups per CU,
  // the VGPR-limited 5 waves/SIMD), else as many as fit 8 KB, never fewer than one slab of 64 nodes
  // spans.  Measured at lmax 12, nq 32 (tools/ab_libs.py --ring-rows): 32 or 18 rows 55 ms
  // (2 workgroups per CU), 9 rows 38.7 ms, 4 rows 37.4 ms.
  const int npsi = 2 * nq;
  // lanes per ring in phase 1: 2 n_q nodes, or n_q node pairs in the per-azimuth-polynomial kernels, whose table of
  // particle j comes on top of the 8 KB
  const int per_ring = jpoly ? (split ? nq / 2 : nq) : npsi;
  const int rows_min = 1 + (63 + per_ring - 1) / per_ring;
  int rows = nq;
  if (o.ring_rows > 0) rows = o.ring_rows;
  else if (jpoly && !o.rule) {
    // Per-azimuth kernels, one wave per pair (sweeps of --ring-rows on the end-of-round kernels,
    // profiles/r03_fin_ring_rows.txt): one ring group while the wave's LDS — particle j's table included — stays
    // within 11.5 KB (13-14 waves per CU; L = 6, n_q = 24: one group of 24 rows beats two of 12 by 4 %); beyond, groups
    // of about 10 KB (L = 8, 9 / n_q = 24 -7...-9 % against 12-13 KB groups, L = 7 / 24 -4 %), see below (the rule
    // before sized the groups without j's table and left L = 9, n_q = 16 with groups of 14 + 2 rings: +6 %).  Known
    // exception: L = 8, n_q = 20, where 17 + 3 rings measured 4 % faster than the 10 + 10 this rule picks.
    const auto total = [&](const int r) { return wave_lds_layout(L, r, false, nqj).bytes; };
    int step = 64, a = per_ring;
    while (a) { const int t = step % a; step = a; a = t; }   // gcd(64, per_ring)
    step = 64 / step;   // rings per whole number of slabs
    // Round 4 (profiles/r04_q5_sweep2.txt, r04_q5_ring_rows.txt; the table builds got cheaper, the node loops did not):
    // one group up to 13 KB where the cap is four slabs (n_q <= 16: L = 11 / 16 -6.8 %, L = 12 / 16 -4.9 % with the one
    // wave that goes with it), and up to 14.5 KB from L = 9 on where groups cannot end on slab boundaries (n_q = 20:
    // L = 9 -3.6 %, L = 10 -3.2 %, L = 11 -2.7 %); n_q = 24 and 32 keep their aligned groups at those sizes
    const int one_group_max = (2 * step <= nq) ? (nq <= 16 ? 13312 : 11776) : (L >= 9 ? 14848 : 11776);
    if (total(nq) > one_group_max) {
      if (2 * step <= nq) {
        // groups that end on a slab boundary (no slab straddles a hand-over: at n_q = 24 every order measured,
        // L = 7...11, wants 8 rings = 3 slabs, not the 12 a budget alone gives): the largest such group within 10 KB
        // (16 waves per CU), the smallest if none fits; then as few groups as that takes, of equal aligned size
        int rfit = step;
        while (rfit + step <= nq && total(rfit + step) <= 10 * 1024) rfit += step;
        const int groups = (nq + rfit - 1) / rfit;
        rows = (((nq + groups - 1) / groups + step - 1) / step) * step;
      } else {
        int rmax = rows_min;
        while (rmax < nq && total(rmax + 1) <= 10752) ++rmax;   // 15 waves per CU
        const int groups = (nq + rmax - 1) / rmax;
        rows = (nq + groups - 1) / groups;
      }
      if (rows < (nq + 3) / 4) rows = (nq + 3) / 4;   // never more than four groups (large L x n_q: j's table alone
    }                                                  // fills the budget; those run two waves per pair anyway)
  } else if (wave_lds_layout(L, nq, false, 0).bytes > 8 * 1024) {
    const int fixed = wave_lds_layout(L, 0, false, 0).bytes;
    rows = (8 * 1024 - fixed) / (32 * (L + 1));
  }
  if (rows < rows_min) rows = rows_min;
  if (rows > nq) rows = nq;
  if (o.rule) {
    // SPEC §2.8: the weights of a slab need its neighbours' residuals, which the kernel keeps in a window of
    // three slabs; a ring group must hold the rings of the slab being weighed and of the next one
    if (L > kMaxUnrolledL || o.variant == 1 || nq > 32) {
      if (msg) snprintf(msg, msglen, "the weighted rule needs lmax <= %d and nq <= 32 (have lmax %d, nq %d)", kMaxUnrolledL, L, nq);
      return SHPAIR_ELMAX;
    }
    // the queue carries the weights too (+1 KB): all rings resident up to 8.75 KB per wave (18 waves per CU;
    // L = 6, n_q = 16 needs 8.5 KB and runs 6 % faster that way than in two groups), 8 KB groups beyond
    rows = (o.ring_rows > 0) ? o.ring_rows : nq;
    if (o.ring_rows <= 0 && wave_lds_layout(L, nq, true, nqj).bytes > 8960) {
      const int fixed = wave_lds_layout(L, 0, true, nqj).bytes;
      rows = (8 * 1024 - fixed) / (32 * (L + 1));
    }
    const int rows_min_w = 2 + (127 + npsi - 1) / npsi;
    if (rows < rows_min_w) rows = rows_min_w;
    if (rows > nq) rows = nq;
  }
  if (split && o.ring_rows <= 0) {
    // two waves per pair: a slab of one wave spans 64 / per_ring rings; two slabs' worth of rings per group, all of
    // them if the pair then stays within 20 KB (8 pairs = 16 waves per CU)
    // ... as many slabs' worth of rings per group as keep the pair within the LDS share of the waves its registers
    // allow (all rings if they fit), never fewer than two slabs' worth
    const int per_slab = (64 + per_ring - 1) / per_ring;
    const int wsimd = split_vgprs > 0 ? waves_per_simd_by_vgprs(split_vgprs) : 4;
    const int budget = (160 * 1024) / (2 * wsimd);   // bytes per pair: 4 wsimd waves per CU, two per pair
    rows = 2 * per_slab;
    if (pair_lds_layout2(L, nq, nq).bytes <= budget) rows = nq;
    else
      while (rows + per_slab <= nq && pair_lds_layout2(L, rows + per_slab, nq).bytes <= budget) rows += per_slab;
    if (rows < rows_min) rows = rows_min;
    if (rows > nq) rows = nq;
  }
  WaveLdsLayout wl = split ? pair_lds_layout2(L, rows, nq) : wave_lds_layout(L, rows, o.rule != 0, nqj);
  // per-azimuth kernels: the node queue grows into what is left of the last LDS granule (queue_capacity)
  int qcap = kQueue;
  if (jpoly && !o.rule && o.waves_per_block <= 1 && o.queue_slack) {
    qcap = queue_capacity(wl.bytes, split ? 2 : 1);
    if (qcap > kQueue) {
      const WaveLdsLayout wg = split ? pair_lds_layout2(L, rows, nq, qcap) : wave_lds_layout(L, rows, false, nqj, qcap);
      if ((wg.bytes + kLdsGranule - 1) / kLdsGranule == (wl.bytes + kLdsGranule - 1) / kLdsGranule) wl = wg;
      else qcap = kQueue;
    }
  }
  if (wl.bytes > 160 * 1024) {
    if (msg) snprintf(msg, msglen, "lmax %d with nq %d needs %d bytes of LDS per pair, more than a CU has", L, nq, wl.bytes);
    return SHPAIR_ELMAX;
  }
  // One wave (= one pair) per workgroup: pairs differ in cost (a grazing pair leaves after phase 1),
  // and a multi-wave workgroup holds its LDS and wave slots until its slowest pair is done.
  // A/B (tools/ab_libs.py --wpb): 1 wave 4.13 ms, 2 waves 4.22, 4 waves 4.34 at L = 6.
  int wpb = 1;
  if (o.waves_per_block > 1) {
    wpb = o.waves_per_block < kMaxWavesPerBlock ? o.waves_per_block : kMaxWavesPerBlock;
    if (wpb * wl.bytes > 160 * 1024) wpb = (160 * 1024) / wl.bytes;
  }
  if (split) wpb = 1;   // the workgroup is the pair; lds_bytes its whole LDS
  // the order's BASELINE shape: the specialised instance (n_q, ring rows and queue capacity as compile-time constants)
  const int wpp = split ? 2 : 1;
  const bool shape = L == 4 ? pair_spec_is<4>(nq, rows, qcap, wpp)
                            : (L == 6 ? pair_spec_is<6>(nq, rows, qcap, wpp) : (L == 12 ? pair_spec_is<12>(nq, rows, qcap, wpp) : false));
  const bool compiled = L <= kMaxUnrolledL && o.variant != 1;
  p = ContactPlan{compiled, jpoly ? 1 : 0, wpp, rows, qcap, wl.bytes, wpb, compiled && o.spec && jpoly && !o.rule && wpb == 1 && shape,
                  o.rule != 0};
  return SHPAIR_OK;
}

// At their BASELINE shapes L = 4 and 6 plan without the two-wave registers: PairSpec is what the planner picks there
// (L = 12 depends on them: tests/test_contact_plan.py checks it with the counts of the built kernels)
template <int L>
constexpr bool pair_spec_planned()
{
  ContactPlan p;   // (spec: the plan's n_q, ring rows, queue and waves per pair are exactly PairSpec<L>'s)
  return plan_contact(L, PairSpec<L>::nq, ContactOptions{}, 0, p) == SHPAIR_OK && p.spec;
}
static_assert(pair_spec_planned<4>() && pair_spec_planned<6>(), "PairSpec<4> / PairSpec<6> are not what plan_contact picks");

// What shpair_get_kernel_info reports of a plan whose kernel has `vgprs` registers (lmax, scratch and needv are the
// caller's).  gfx950 keeps at most 8 waves per SIMD, 4 SIMDs and 160 KiB of LDS per CU; LDS is allocated in granules of
// 1 280 B (160 KB / 128; measured: +448 B on 8 512 B is free, +512 B costs two waves, profiles/r04_ac_lds_granule.txt)
SHP_HD constexpr void contact_kernel_info(const ContactPlan& p, const int vgprs, shpair_kernel_info& k)
{
  k.compiled_order = p.compiled ? 1 : 0; k.family = p.family; k.weighted = p.weighted ? 1 : 0; k.specialised = p.spec ? 1 : 0;
  k.waves_per_pair = p.waves_per_pair; k.lds_bytes_per_wave = p.lds_bytes / p.waves_per_pair;
  k.ring_rows = p.ring_rows; k.queue_entries = p.qcap; k.vgprs = vgprs;
  k.waves_per_simd_vgpr = vgprs > 0 ? waves_per_simd_by_vgprs(vgprs) : 8;
  k.waves_per_cu_lds = p.waves_per_pair * ((160 * 1024) / ((p.lds_bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule));
  k.waves_per_cu = 4 * k.waves_per_simd_vgpr < k.waves_per_cu_lds ? 4 * k.waves_per_simd_vgpr : k.waves_per_cu_lds;
}

}  // namespace shp
