// ring_tables.hpp — the ring tables of a pair (A_km, B_km and their mu-derivatives, per quadrature ring and order):
// built by Legendre recurrence (cap_frame_rings, body-frame family) or by Horner evaluation of particle i's
// polynomials (cap_frame_rings_poly, per-azimuth family), r_i evaluated from a ring row (ring_eval), and r_i or its
// gradient at a node pair of phase 1 (ring_pair_rec).
#pragma once
#include "contact_plan.hpp"
#include "sh_const.hpp"
#include "wave_ops.hpp"

namespace shp {

// Ring tables of rings k0 .. k0 + nrows - 1 from the rotated coefficients.
//
// Lanes are (ring, order class): G = 8, 4, 2 or 1 lanes per ring — as many as 64 lanes give the group's rows — and
// lane (kr, g) builds the orders m = g, g + G, g + 2G, ...  For one m the Legendre recurrence runs over n = m+1 .. L;
// all lanes step through n together (compile-time n for the compiled orders: every LDS and table offset is an
// immediate), a lane joins at n = m + 1 under the exec mask, and steps no lane of the pass needs (n <= the pass's
// smallest m) are skipped wave-uniformly.  Q_n lives in one of two registers by the parity of n, so a step updates
// the older value in place: 8 FP64 operations per step and no moves.  L = 6, n_q = 16: 8 steps in one pass, ~130
// vector instructions per ring group.  (Round 2 up to here: one (k, m) per lane and, for every lane, L steps each
// split by the divergent test t < m: ~200 instructions per 64 entries, 2 passes = ~400 per pair at the headline.)
// PRE (the JPT kernels, which have the registers): the recurrence constants of ALL steps of a
// pass are requested before the first step instead of inside each step's divergent branch — a pass then waits for
// one table load, not for one per step (six dependent ~1000-cycle round trips at L = 6).
// WPP = 2: `lane` is the thread index within the pair's two waves (0..127); with 128 lanes a group of <= 8 rings gets
// 16 lanes per ring — at L <= 15 one order per lane, a single pass.
// DENSE map (one wave per pair, (L + 1) x rows <= 64): lane = (ring, order), L + 1 lanes per ring — every (ring, order)
// of the group in ONE pass.  With power-of-two classes L = 4, n_q = 10 took two passes (orders 0-3, then order 4 alone
// with the whole pass overhead): 213 of that kernel's 1 150 instructions per pair.
// (JPT kernels only: in one forces-only body-frame kernel the extra map tips the register allocator into a spill.)
template <int L, int WPP, bool DENSE>
__device__ __forceinline__ void ring_lane_map(const int lane, const int nrows, int& krl, int& g, int& G, int& rpc, int& lg)
{
  const int lg1 = (nrows <= 8) ? 3 : (nrows <= 16) ? 2 : (nrows <= 32) ? 1 : 0;
  lg = lg1 + (WPP == 2 ? 1 : 0);   // log2 G: as many lanes per ring as the NT lanes give the group's rows; uniform
  G = 1 << lg;
  krl = lane >> lg;
  g = lane & (G - 1);
  rpc = (64 * WPP) >> lg;
  if constexpr (DENSE && L >= 1 && WPP == 1) {
    if ((L + 1) * nrows <= 64) {   // wave-uniform
      G = L + 1;
      krl = lane / (L + 1);
      g = lane - krl * (L + 1);
      rpc = 64 / (L + 1);
      lg = 0;
    }
  }
}

template <int L, bool PRE = false, int WPP = 1, bool DENSE = false>
__device__ __forceinline__ void cap_frame_rings(const PairParams& P, double* __restrict__ lw, const WaveLdsLayout& W,
                                                const int LL, const int lane, const int k0, const int nrows,
                                                const double hw, const double hm, const bool have_first = false)
{
  // have_first (PRE kernels): the Gauss-Legendre node of this lane's ring in the first pass of the first ring group
  // was requested at the start of the kernel and waits in the (empty) queue at lw[W.stash + lane]
  const double* ch = lw + W.v0;
  double* ring = lw + W.ring;
  int krl, g, G, rpc, lg;
  ring_lane_map<L, WPP, DENSE>(lane, nrows, krl, g, G, rpc, lg);
  for (int kr0 = 0; kr0 < nrows; kr0 += rpc) {
    const int kr = kr0 + krl;
    const bool row_ok = kr < nrows && krl < rpc;
    const double tk = (PRE && have_first && k0 == 0 && kr0 == 0) ? lw[W.stash + lane] : P.glt[k0 + (row_ok ? kr : 0)];
    const double mu = fma(hw, tk, hm);
    const double sig2 = fmax(0.0, fma(-mu, mu, 1.0));
    const double sig = sqrt_nr(sig2);
    double sp = 1.0, sigG = sig;   // sigma^g and sigma^G
    for (int t = 0; t < G - 1; ++t) {
      if (t < g) sp *= sig;
    }
    for (int t = 0; t < lg; ++t) sigG *= sigG;
    for (int m0 = 0; m0 <= LL; m0 += G) {
      const int m = m0 + g;
      const bool ok = row_ok && m <= LL;
      const int mc = ok ? m : 0;   // idle lanes read in bounds
      const double* rcm = P.rc + (sh_moff(LL, mc) - mc);   // a'_nm at rcm[n]
      const double* cp = ch + mc;                          // C_nm at cp[n^2 + n], C_n,-m at cm[n^2 + n]
      const double* cm = ch - mc;
      // Q_n and dQ_n/dmu in q[n & 1], d[n & 1]; start: Q_m = 1, Q_(m-1) = 0
      const bool modd = (mc & 1) != 0;
      double qe = modd ? 0.0 : 1.0, qo = modd ? 1.0 : 0.0, de = 0.0, dd = 0.0;
      // m = 0: the B sums read C_n0 again and are not stored (no select in the loop)
      double wa = cp[mc * mc + mc], wb = cm[mc * mc + mc], wad = 0.0, wbd = 0.0;
      constexpr int NPRE = (PRE && L >= 1) ? L : 1;
      double pa[NPRE];
      if constexpr (PRE && L >= 1) {
#pragma unroll
        for (int n = 1; n <= L; ++n) {
          if (n <= m0) continue;
          pa[n - 1] = rcm[n];   // every lane, whatever its m: the address is inside the table, the value unused
        }
#pragma unroll
        for (int n = 1; n <= L; ++n) {
          if (n <= m0) continue;
          asm volatile("" : "+v"(pa[n - 1]));   // keep the requests up here
        }
      }
#pragma unroll
      for (int n = 1; n <= ((L >= 0) ? L : LL); ++n) {
        if (n <= m0) continue;   // wave-uniform: no lane of this pass has m < n
        if (ok && n > m) {
          const double a = (PRE && L >= 1) ? pa[(PRE && L >= 1) ? n - 1 : 0] : rcm[n];
          const double ca = cp[n * n + n], cbm = cm[n * n + n];
          if (n & 1) {
            dd = fma(a, fma(mu, de, qe), -dd);
            qo = fma(a, mu * qe, -qo);
            wa = fma(ca, qo, wa); wb = fma(cbm, qo, wb); wad = fma(ca, dd, wad); wbd = fma(cbm, dd, wbd);
          } else {
            de = fma(a, fma(mu, dd, qo), -de);
            qe = fma(a, mu * qo, -qe);
            wa = fma(ca, qe, wa); wb = fma(cbm, qe, wb); wad = fma(ca, de, wad); wbd = fma(cbm, de, wbd);
          }
        }
      }
      if (ok) {
        // d/dmu [sigma^m W] = sigma^m (W' - m mu W / sigma^2)
        const double f = (m > 0) ? (double)m * mu * rcp_nr(sig2) : 0.0;
        double* o = ring + 4 * (kr * (LL + 1) + m);
        o[0] = sp * wa;
        o[2] = sp * fma(-f, wa, wad);
        if (m == 0) {
          o[1] = mu;   // B_k0 = 0: the slot carries mu_k
          o[3] = sig;  // dB_k0/dmu = 0: carries sigma_k
        } else {
          o[1] = sp * wb;
          o[3] = sp * fma(-f, wb, wbd);
        }
      }
      sp *= sigG;
    }
  }
  pair_sync<WPP>();
}

// Ring tables of the JPT kernels (round 4): HORNER EVALUATIONS of particle i's first-stage polynomials.
//
// jpoly_build leaves, for every order m and part (cos, sin), the polynomial PJ^i[2m + part](mu) with
//   r_i(mu, psi) = sum_m s_m [cos(m psi) PJ^i[2m](mu) + sin(m psi) PJ^i[2m + 1](mu)],   s_m = 1 (m even), sigma (m odd)
// (the host table folds (1 - mu^2)^floor(m / 2) into the polynomial: degree L for even m, L - 1 for odd m).  So
//   A_km = s_m PJ^i[2m](mu_k),   dA_km/dmu = s_m PJ^i[2m]'(mu_k)  [- (mu_k / sigma_k) PJ^i[2m](mu_k) for odd m],   B likewise:
// one lane per table entry (ring, order), value and derivative of both parts by Horner — 4L - 2 v_fma_f64 and L + 1
// ds_read_b128 (the two parts' coefficients are adjacent: 2 (L + 1) doubles) — no recurrence constants, no sigma^m, no
// division.  The associated-Legendre recurrence this replaces (cap_frame_rings: 8 FP64 operations per step, L - m steps
// per entry, a pass per order class) was 256 of the headline kernel's 1 826 vector instructions per pair, 59 % of them
// not FP64 (profiles/r04_d_headline_valu_sites.txt).
// Entry e = ring * (L + 1) + order IS the ring table's own index: the store needs no address arithmetic beyond 32 e.
// Lane map of cap_frame_rings_poly for a group of `nrows` rings on NT lanes: -1 = DENSE, one lane per table entry (ring,
// order), ceil(nrows (L + 1) / NT) passes; lg >= 1 = GROUPED, 2^lg lanes per ring, lane g of a ring takes the orders
// g, g + 2^lg, ... — one pass, and what an entry shares with the other orders of its ring (the Gauss node, mu, sigma,
// 1 / sigma: ~25 of a dense entry's ~69 vector instructions) is made once per lane.  Chosen by that instruction count.
__host__ __device__ inline int ring_poly_map(const int nrows, const int K, const int NT)
{
  const int nent = nrows * K;
  if (nent <= NT) return -1;
  int lg = 0;
  while ((NT >> (lg + 1)) >= nrows && (1 << lg) < K) ++lg;   // as many lanes per ring as one pass over the group allows
  if (lg < 1) return -1;
  const int E = (K + (1 << lg) - 1) >> lg, passes = (nent + NT - 1) / NT;
  return (25 + 44 * E < 69 * passes) ? lg : -1;
}

template <int L, int WPP, class PP = PairParams>
__device__ __forceinline__ void cap_frame_rings_poly(const PP& P, double* __restrict__ lw, const WaveLdsLayout& W,
                                                     const int lane, const int tid, const int k0, const int nrows,
                                                     const double hw, const double hm, const bool have_first)
{
  constexpr int K = L + 1, NT = 64 * WPP;
  const double* pi = lw + W.pi;
  double* ring = lw + W.ring;
  const int nent = nrows * K;
  const int lg = ring_poly_map(nrows, K, NT);   // wave-uniform
  // one table entry: value and mu-derivative of both parts of order m at (mu, sigma), stored at entry e
  auto entry = [&](const int m, const int e, const bool store, const double mu, const double sig, const double isig)
                   __attribute__((always_inline)) {
    const double* row = pi + (2 * K) * m;   // 16-byte aligned: 2K doubles per order, an aligned base
    v2d c[K];
#pragma unroll
    for (int t = 0; t < K; ++t) c[t] = lds2(row + 2 * t);
    // element j of the 2K doubles: cos-part coefficient of mu^p at j = p, sin-part at j = K + p
#define SHP_EL(j) c[(j) >> 1][(j) & 1]
    double pc = SHP_EL(L), ps = SHP_EL(K + L), dc = 0.0, ds = 0.0;
    if constexpr (L >= 1) {
      dc = pc;
      ds = ps;
      pc = fma(pc, mu, SHP_EL(L - 1));
      ps = fma(ps, mu, SHP_EL(K + L - 1));
#pragma unroll
      for (int q = L - 2; q >= 0; --q) {
        dc = fma(dc, mu, pc);
        ds = fma(ds, mu, ps);
        pc = fma(pc, mu, SHP_EL(q));
        ps = fma(ps, mu, SHP_EL(K + q));
      }
    }
#undef SHP_EL
    const bool odd = (m & 1) != 0;
    const double sm = odd ? sig : 1.0;            // s_m
    const double tm = odd ? -mu * isig : 0.0;     // d s_m / d mu
    const double A = sm * pc, dA = fma(tm, pc, sm * dc);
    double B = sm * ps, dB = fma(tm, ps, sm * ds);
    if (m == 0) {   // B_k0 = 0: the slots carry mu_k and sigma_k
      B = mu;
      dB = sig;
    }
    if (store) {
      double* o = ring + 4 * e;
      *(v2d*)__builtin_assume_aligned(o, 16) = v2d{A, B};
      *(v2d*)__builtin_assume_aligned(o + 2, 16) = v2d{dA, dB};
    }
  };
  if (lg >= 1) {
    // GROUPED: lane = (ring, g)
    const int G = 1 << lg, kr = tid >> lg, g = tid & (G - 1);
    const int krc = min(kr, nrows - 1);
    const double tk = (have_first && k0 == 0) ? lw[W.stash + lane] : P.glt[k0 + krc];
    const double mu = fma(hw, tk, hm);
    const double sig2 = max_raw(fma(-mu, mu, 1.0), 1e-300);
    const double isig = rsqrt_nr(sig2);
    const double sig = sig2 * isig;
    for (int m0 = 0; m0 < K; m0 += G) {   // wave-uniform trip count
      const int m = m0 + g;
      entry(min(m, K - 1), krc * K + m, kr < nrows && m < K, mu, sig, isig);
    }
  } else {
    for (int e0 = 0; e0 < nent; e0 += NT) {   // DENSE: wave-uniform passes
      const int e = e0 + tid;
      const int ec = min(e, nent - 1);   // idle lanes repeat the last entry and store nothing
      const int kr = (int)((unsigned)ec / (unsigned)K), m = ec - kr * K;
      // have_first: this lane's Gauss-Legendre node of the first pass of the first ring group was requested at the start
      // of the kernel and waits in the (empty) queue
      const double tk = (have_first && k0 == 0 && e0 == 0) ? lw[W.stash + lane] : P.glt[k0 + kr];
      const double mu = fma(hw, tk, hm);
      const double sig2 = max_raw(fma(-mu, mu, 1.0), 1e-300);
      const double isig = rsqrt_nr(sig2);
      const double sig = sig2 * isig;
      entry(m, e, e < nent, mu, sig, isig);
    }
  }
  pair_sync<WPP>();
}

// Layout of the cos/sin(m psi_l) table (host: upload_quadrature).  Up to L = 6 l-major: the orders of one azimuth are
// adjacent, a lane reads them with immediate offsets from one address (m-major costs a 64-bit address computation per
// order, ~10 VALU per slab).  Above, m-major: a lane's orders would span 16 (L - 1) > 128 bytes and every wave load
// would touch one cache line per lane (A/B at L = 12, n_q = 32: l-major +1.8 %), and at L = 7 the l-major form costs a spilled register.
__host__ __device__ constexpr bool trig_lmajor(int L) { return L >= 2 && L <= 6; }

// Layout of the quadrature table d_quad, in doubles (host only: shpair_upload_quadrature fills it, the pair and the
// wall parameter wiring read it; nothing else does arithmetic on that buffer):
//   glt[n_q] | glw[n_q] | cos psi_l, l < 2 n_q | sin psi_l | trig: (cos, sin)(m psi_l), m = 2..lmax, l < 2 n_q, laid
//   out by trig_lmajor() | trigj: (cos, sin)(m psi_l), m = 0..lmax + 1 (one order more than exists: jpoly_build reads it
//   against zeros) of the first n_q azimuths, l-major (psi_(l + n_q) = psi_l + pi only flips the sign of the odd orders)
struct QuadLayout {
  int lmax, npsi, nm;   // nm: orders m = 2..lmax of the trig block
  size_t glt, glw, cpsi, spsi, trig, trigj, size;
  int trig_stride;      // PairParams::trig_stride
  QuadLayout(const int L, const int nq)
      : lmax(L), npsi(2 * nq), nm(L >= 2 ? L - 1 : 0), glt(0), glw(nq), cpsi(2 * (size_t)nq), spsi(4 * (size_t)nq),
        trig(6 * (size_t)nq), trigj(trig + (size_t)nm * 2 * npsi), size(trigj + (size_t)nq * (L + 2) * 2),
        trig_stride(trig_lmajor(L) ? 2 * (L - 1) : 4 * nq)
  {
  }
  // where cos(m psi_l) sits; the sine follows it
  size_t trig_at(const int l, const int m) const
  {
    return trig + 2 * (trig_lmajor(lmax) ? ((size_t)l * nm + (m - 2)) : ((size_t)(m - 2) * npsi + l));
  }
  size_t trigj_at(const int l, const int m) const { return trigj + ((size_t)l * (lmax + 2) + m) * 2; }
};

// r_i (and its mu / psi derivatives) at ring row `row`, azimuth (c1, s1) = (cos psi, sin psi)
template <int L, bool GRAD>
__device__ __forceinline__ void ring_eval(const double* __restrict__ row, const int LL, const double c1, const double s1,
                                          const double* __restrict__ tr, const int tstride, double& r, double& rmu,
                                          double& rpsi)
{
  // cos/sin(m psi) of this lane's azimuth: compiled orders read them from the host-built table `tr`
  // (m = 2..L, 16 bytes per m, vector memory loads that cost no VALU slot); the run-time-order kernel keeps
  // the Chebyshev recurrence (4 FP64 operations per m).
  r = row[0];
  rmu = GRAD ? row[2] : 0.0;
  rpsi = 0.0;
  double cm = c1, sm = s1;
  const int lim = (L >= 0) ? L : LL;
#pragma unroll
  for (int m = 1; m <= lim; ++m) {
    if (L >= 2 && m >= 2) {
      cm = tr[trig_lmajor(L) ? 2 * (m - 2) : (m - 2) * tstride];
      sm = tr[(trig_lmajor(L) ? 2 * (m - 2) : (m - 2) * tstride) + 1];
    }
    const v2d ab = lds2(row + 4 * m);   // (A_km, B_km): one ds_read_b128
    const double A = ab[0], B = ab[1];
    r = fma(A, cm, r);
    r = fma(B, sm, r);
    if (GRAD) {
      const v2d dab = lds2(row + 4 * m + 2);
      rmu = fma(dab[0], cm, rmu);
      rmu = fma(dab[1], sm, rmu);
      const double dm = (double)m;
      rpsi = fma(dm * B, cm, rpsi);
      rpsi = fma(-dm * A, sm, rpsi);
    }
    if (L < 2 && m < lim) {
      const double c = fma(cm, c1, -(sm * s1)), s = fma(cm, s1, sm * c1);
      cm = c;
      sm = s;
    }
  }
}

// r_i — or, GRAD, its mu- and psi-derivatives — at the TWO azimuths psi and psi + pi of ring row `row`, from ONE pass
// over the row with the lane's (c1, s1) = (cos psi, sin psi): cos / sin(m (psi + pi)) = (-1)^m cos / sin(m psi), so the
// even and the odd orders are summed in chains of their own and the two azimuths are their sum and their difference
// (phase 1 of the per-azimuth kernels: a lane's node pair (k, l), (k, l + n_q)).  One three-term trig recurrence serves
// both (ring_grad_rec, ring_value in jpoly.hpp: the same recurrence for a single node).
//   GRAD false: v = r_i; a0 = A_k0, which the caller has read with mu_k; one ds_read_b128 and two v_fma_f64 per order.
//   GRAD true:  v = dr_i/dmu, w = dr_i/dpsi; a0 = dA_k0/dmu; two ds_read_b128 and five FP64 operations per order.  The
//               values are not formed again: the caller has them from the GRAD false pass of the same row, which it
//               makes for every slab — this one only where a slab holds an inside node.
//   CHUNK > 0:  the orders are taken CHUNK at a time — the row's address and the running sums go through an empty asm
//               between chunks, so the reads of the later orders cannot all be issued ahead of the first FMA (no
//               instruction; the high orders would otherwise hold 4 registers per order at once and spill).
template <int L, bool GRAD, int CHUNK = 0>
__device__ __forceinline__ void ring_pair_rec(const double* __restrict__ row0, const double a0, const double c1, const double s1,
                                              double& va, double& vb, double& wa, double& wb)
{
  double ve = a0, vo = 0.0, we = 0.0, wo = 0.0;
  const double* row = row0;
  if constexpr (L >= 1) {
    double cm = c1, sm = s1, cp = 1.0, sp = 0.0;   // three-term recurrence: one v_fma_f64 per cos / sin
    const double tc = c1 + c1;
#pragma unroll
    for (int m = 1; m <= L; ++m) {
      const v2d ab = lds2(row + 4 * m);
      const double A = ab[0], B = ab[1];
      if constexpr (!GRAD) {
        if (m & 1) vo = fma(A, cm, fma(B, sm, vo));
        else ve = fma(A, cm, fma(B, sm, ve));
      } else {
        const v2d dab = lds2(row + 4 * m + 2);
        const double t = fma(B, cm, -(A * sm)), dm = (double)m;
        if (m & 1) {
          vo = fma(dab[0], cm, fma(dab[1], sm, vo));
          wo = (m == 1) ? t : fma(dm, t, wo);
        } else {
          ve = fma(dab[0], cm, fma(dab[1], sm, ve));
          we = (m == 2) ? dm * t : fma(dm, t, we);
        }
      }
      if (m < L) {
        const double c = fma(tc, cm, -cp), s = fma(tc, sm, -sp);
        cp = cm;
        sp = sm;
        cm = c;
        sm = s;
        if constexpr (GRAD && CHUNK > 0) {
          if (m % CHUNK == 0) {
            unsigned ra_ = (unsigned)(size_t)(const __attribute__((address_space(3))) double*)row;
            asm volatile("" : "+v"(ra_), "+v"(ve), "+v"(vo), "+v"(cm), "+v"(sm));
            row = (const double*)(const __attribute__((address_space(3))) double*)(size_t)ra_;
          }
        }
      }
    }
  }
  va = ve + vo;
  vb = ve - vo;
  wa = we + wo;
  wb = we - wo;
}

}  // namespace shp
