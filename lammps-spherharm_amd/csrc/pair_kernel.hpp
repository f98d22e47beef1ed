// pair_kernel.hpp — the contact kernel: ONE WAVEFRONT PER HALF-LIST PAIR.
//
// docs/SPEC.md §2.  Per pair: a set-up step and two phases, all 64 lanes wide:
//   set-up   particle i's expansion is rotated into the CAP frame (pole = the
//            direction to the neighbour): real-SH coefficients through
//            Z(alpha) X^T Z(beta) X Z(gamma) with the constant matrices
//            X^l = T(Rx(90 deg)) (no Wigner recursion, no trigonometry beyond
//            three sin/cos pairs), then per quadrature ring k and order m the
//            Fourier coefficients A_km, B_km of r_i around the ring and their
//            mu-derivatives.  After that r_i at a cap node costs 6 FP64 ops per
//            m instead of a full (L+1)(L+2)/2-term evaluation, and so does its
//            surface gradient.
//   phase 1  the lanes stride the Q = 2 nq^2 cap nodes in slabs of 64: r_i at
//            the node, the surface point in j's frame, r_j there -> inside?
//            Inside nodes are appended to a per-wave LDS queue (ballot + mbcnt).
//   phase 2  whenever 64 inside nodes are queued (and once for the rest), one
//            node per lane: the inner radius by safeguarded secant (overlap
//            volume) and the surface gradient of i (vector area, torque arm).
// Only ~30 % of the cap nodes of a packed bed are inside the neighbour, so
// queueing them keeps the two expensive passes at full lane occupancy.
// Per-pair data is wave-uniform: particle j's coefficients (monomial form, Horner,
// sh_device.hpp) arrive as scalar loads, the pair frame, the rotation's work vectors,
// the ring tables and the queue sit in per-wave LDS.  The seven integrals (V, S_n,
// T_n) are transposed through LDS and added in two levels; lanes 0-5 then own one
// component of the force / torque each, apply the force law and issue ONE 6-lane FP64
// atomic per atom (or, in the deterministic mode, one store per pair: det_kernels.hpp).
// One wave per workgroup — or, for large tables, two waves per pair (pair_lds_layout2).
// No MFMA: the work is polynomial evaluation per node, FP64 VALU bound.
// Two kernel families differ in how particle j's radius is evaluated (chosen per (L, n_q) by contact_plan.hpp
// contact_family), each a kernel template in a file of its own:
//   0  pair_contact_body_kernel<L, NEEDV, WEIGHTED> (contact_kernel_body.hpp): in j's body frame from scalar-fed
//      monomial coefficients (sh_device.hpp); one node per lane, a ring queue; the run-time-order kernel, the few
//      (L, n_q) contact_family leaves here, and the weighted variant;
//   1  pair_contact_azimuth_kernel<L, NEEDV, WPP, SPEC> (contact_kernel_azimuth.hpp) — the default almost everywhere:
//      from per-azimuth polynomials in the pair's common frame, with the coefficient rotations of both particles in a
//      kernel of their own (pair_rotate_lane_kernel) and node PAIRS per lane in phase 1, a stack queue with direct
//      batches, one or two waves per pair: see the block comment above jpoly_build (jpoly.hpp).
// This file keeps what the two share by NAME — the A/B knobs — and the one place where a plan becomes a family,
// pair_contact_instance.  Text the two kernels share is written out in both (see the head of either file for why).
// (Comments in the other headers call the per-azimuth family "the JPT kernels", after the template parameter that
// selected it while both families were one function.)
//
// Reference: PairSH::compute() of the reference is ABSENT FROM MOUNT
// (/root/reference/README.md:1 is the whole mount).
#pragma once
#include "contact_plan.hpp"
#include "pair_params.hpp"
#include "pair_rotate.hpp"

// Waves per SIMD the register allocator must leave room for, chosen per kernel so that NO kernel spills a vector
// register or touches scratch (tests/test_kernel_resources.py reads the code objects):
//   forces-only kernels (no root finder) fit 80 VGPRs = 6 waves up to L = 6;
//   kernels with the volume path fit 80 VGPRs at L = 0, 1 and 6 and need 96 (5 waves) in between (at 80 they would
//   spill 1-7 registers; round 1 shipped those with 8-32 bytes of scratch) and from L = 7 on;
//   the weighted variant (three-slab window) fits 96 VGPRs up to L = 6 except at L = 3 (128: 4 waves), 128 beyond.
// Interleaved A/B of 6 against 5 waves where both compile clean (round 1): L = 6, n_q = 16 +1 %, n_q = 8 +7 %.
#ifndef SHP_WMIN_WAVES
#define SHP_WMIN_WAVES(L) (((L) >= 0 && (L) <= 6 && (L) != 3) ? 5 : 4)
#endif
#ifndef SHP_MIN_WAVES
#define SHP_MIN_WAVES(L, NEEDV) \
  ((NEEDV) ? (((L) == 0 || (L) == 1 || (L) == 6) ? 6 : 5) : (((L) >= 0 && (L) <= 6) ? 6 : 5))
#endif
// kernels that evaluate particle j from per-azimuth polynomials: the rows of j's table are read from LDS
// (80 registers up to L = 4, 96 up to L = 6 and for the one-wave kernel of L = 9, 128 beyond — L = 5, 8 and the two-wave
// kernel of L = 9 come out a step below their bound; A/B per order: profiles/r03_zzzz_ab_root_loop.txt, r03_zzzzzz_ab_lds_abs.txt)
#ifndef SHP_JMIN_WAVES
#define SHP_JMIN_WAVES(L, NEEDV, WPP) (((L) <= 4) ? 6 : (((L) <= 6 || ((L) == 9 && (WPP) == 1 && !(NEEDV))) ? 5 : 4))
#endif

// the first trip of the inner-radius search written apart from its loop (per-azimuth kernels, phase 2)
#ifndef SHP_PEEL
#define SHP_PEEL(L) ((L) >= 6)
#endif
// the node (ring, azimuth, weight, mu, sigma) stays in registers across the inner-radius search (per-azimuth kernels
// that form S_n, T_n in the tail of phase 2, and the body-frame family: CARRY)
#ifndef SHP_CARRY_NODE
#define SHP_CARRY_NODE(L, WPP) ((L) >= 6 && !((L) == 9 && (WPP) == 1))
#endif
// Per-azimuth kernels: the surface integrals S_n, T_n formed in PHASE 1, for both nodes of a lane's pair from one pass over
// the ring row, and phase 2 the volume search alone (contact_kernel_azimuth.hpp).  From L = 6 on, except:
//   L <= 5 — L = 5 with the volume path needs 84 VGPRs against 80 with the tail (its sixth wave per SIMD), and L = 4 /
//   n_q = 10 measured slower on the new path (profiles/ab_phase1_orders.txt, last leg): few orders, little to share;
//   L = 12, two waves per pair — the register allocator spills 1-2 registers (tests/test_kernel_resources.py).
// Those keep the tail of phase 2.
#ifndef SHP_SURFACE_PHASE1
#define SHP_SURFACE_PHASE1(L, NEEDV, WPP) ((L) >= 6 && !((L) == 12 && (WPP) == 2))
#endif
// ... with the gradient pass of ring_pair_rec taken this many orders at a time (0: no constraint on the scheduler).
// L = 7 / 16 -4.0 %, 8 / 16 -2.2 %, 9 / 16 -4.8 %, 10 / 16 -3.6 %, 12 / 16 -2.8 % against the tail (profiles/ab_phase1_orders.txt)
#ifndef SHP_GRAD_CHUNK
#define SHP_GRAD_CHUNK(L) ((L) >= 7 ? 1 : 0)
#endif

namespace shp {
template <bool B>
struct BoolC { static constexpr bool value = B; };
}  // namespace shp

#include "contact_kernel_azimuth.hpp"
#include "contact_kernel_body.hpp"

namespace shp {

// the sharp instances of a family, `needv`: with the overlap-volume root finder
template <int L, bool AZIMUTH = false, int WPP = 1, bool SPEC = false>
const void* contact_kernel(const bool needv)
{
  if constexpr (AZIMUTH)
    return needv ? (const void*)pair_contact_azimuth_kernel<L, true, WPP, SPEC>
                 : (const void*)pair_contact_azimuth_kernel<L, false, WPP, SPEC>;
  else
    return needv ? (const void*)pair_contact_body_kernel<L, true>
                 : (const void*)pair_contact_body_kernel<L, false>;
}
// The kernel instance a plan (contact_plan.hpp) runs — the one place where a plan becomes a family: per-azimuth
// (contact_kernel_azimuth.hpp) or body-frame (contact_kernel_body.hpp).  The launch and the attribute query of
// shpair_get_kernel_info both take it from here.  (The order of the returns is the order of the kernels in .text.)
template <int L>
const void* pair_contact_instance(const ContactPlan& p, const bool needv)
{
  if constexpr (L >= 0) {
    if (p.weighted) return (const void*)pair_contact_body_kernel<L, true, true>;   // SPEC §2.8: one instance serves both force laws
    if constexpr (PairSpec<L>::nq > 0)
      if (p.spec) return contact_kernel<L, true, PairSpec<L>::wpp, true>(needv);   // n_q, rows, queue as constants
    if constexpr (split_compiled(L))
      if (p.waves_per_pair == 2) return contact_kernel<L, true, 2>(needv);
    if (p.family == 1) return contact_kernel<L, true>(needv);
  }
  return contact_kernel<L>(needv);
}

// wait_before_contact (nullable): an event the CONTACT kernel waits for, not the rotation kernel in front of it — the
// host-pointer entry point uploads f and torque on a second stream beside the set-up and rotation kernels.
template <int L>
void launch_pair_contact(const PairParams& P, const ContactPlan& plan, bool needv, hipStream_t st, hipEvent_t wait_before_contact)
{
  const int nslots = P.npairs - P.slot0;   // the launch covers the slots [slot0, npairs)
  if (nslots <= 0) return;
  if constexpr (L >= 0) {
    if (plan.family == 1)   // both particles' coefficient rotations, one lane each, then the contact kernel that reads them
      hipLaunchKernelGGL((pair_rotate_lane_kernel<L>), dim3((2 * (unsigned)nslots + 63) / 64), dim3(64),
                         RotLaneLds<L>::bytes(), st, P, const_cast<double*>(P.rot));
  }
  if (wait_before_contact) (void)hipStreamWaitEvent(st, wait_before_contact, 0);
  // waves_per_block pairs per workgroup; with two waves per pair the workgroup is the pair (waves_per_block 1)
  const int wpb = plan.waves_per_block;
  const size_t lds = (size_t)wpb * plan.lds_bytes;
  const void* kern = pair_contact_instance<L>(plan, needv);
  if (lds > 65536) (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  void* args[] = {const_cast<PairParams*>(&P)};
  (void)hipLaunchKernel(kern, dim3((nslots + wpb - 1) / wpb), dim3(64 * wpb * plan.waves_per_pair), args, lds, st);
}

}  // namespace shp
