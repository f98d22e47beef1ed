// jpoly.hpp — particle j's per-azimuth polynomials in the pair's common frame (per-azimuth kernel family): the
// per-pair build (jpoly_build) and the evaluations of the node loops (jpoly_eval*, ring_grad_rec, ring_value).
#pragma once
#include "contact_plan.hpp"
#include "wave_ops.hpp"

namespace shp {

// ---- particle j in the pair's COMMON frame ------------------------------------------------------------------------
// Every point at which a pair evaluates r_j — a cap node's surface point r_i u, or a point x_i + lambda u of the
// node's ray in the inner-radius search — lies in the half-plane through the line of centres that contains u: seen
// from x_j in the frame (e1, e2, c) it has the node's azimuth psi_l, and only its polar angle varies,
//   cos(theta_j) = (lambda mu_k - rho) / s,   sin(theta_j) = lambda sigma_k / s,   s^2 = lambda^2 - 2 lambda mu_k rho + rho^2.
// So particle j gets the treatment of particle i: its expansion is rotated into the common frame (the same
// cap_frame_rotate with M_j = [R_j^T e1, R_j^T e2, R_j^T c], whose Euler angles come with the pair record), where
//   r_j(mu, psi) = sum_m sigma^m [cos(m psi) Wc_m(mu) + sin(m psi) Ws_m(mu)],   sigma = sqrt(1 - mu^2).
// For a FIXED azimuth the even orders sum to a polynomial G_l(mu) of degree L (sigma^m = (1 - mu^2)^(m/2)) and the odd
// ones to sigma H_l(mu), H_l of degree L - 1:   r_j = G_l(mu_j) + sigma_j H_l(mu_j)   — 2L + 1 coefficients and 2L + 1
// v_fma_f64 per evaluation instead of (L+1)^2 coefficients and ~(L+1)^2 + 4L operations of a body-frame evaluation
// (L = 6: 13 against 69, and no direction in j's body frame: 14 more), kept in VGPRs across the inner-radius
// iterations (and across phase 1, where a lane's azimuth does not change when 2 n_q divides 64).  The azimuths
// psi_l and psi_(l + n_q) = psi_l + pi share a row: G is the same, H changes sign.
// Built per pair in two steps from the rotated, scaled vector v0 (both sparse matrix-vector products):
//   1. PJ[2m + part][k] = sum_n v0[n^2 + n +- m] E_nm[k]   (host table P.jval / P.jcol, ELL rows; sh_tables.cpp)
//   2. G_l[k] = sum_(m even) cos(m psi_l) PJ[2m][k] + sin(m psi_l) PJ[2m+1][k],  H_l likewise over the odd m.
// The first-stage rows of a lane (NP passes of 64 rows, XW entries each) and the cos/sin of its orders for the first
// 16 azimuths: constants of the launch, requested at the very start of the kernel so that their latency runs
// beside that of the pair's record (small orders only: 24 + 16 registers at L = 6).
template <int L>
struct JPolyPre {
  static constexpr int K = L + 1, NR = jpoly_rows(L) * K, XW = L / 2 + 1, NP = (NR + 63) / 64, NM = L / 2 + 1;
  static constexpr bool on = NP * XW <= 8;
  double val[on ? NP * XW : 1];
  int col[on ? NP * XW : 1];
  double cs[NM], sn[NM];
  __device__ __forceinline__ void fetch(const PairParams& P, const int lane, const int nq)
  {
    if constexpr (on) {
#pragma unroll
      for (int ps = 0; ps < NP; ++ps) {
        const int o = lane + 64 * ps;
        const size_t at = (size_t)(o < NR ? o : 0) * XW;
#pragma unroll
        for (int t = 0; t < XW; ++t) {
          val[ps * XW + t] = P.jval[at + t];
          col[ps * XW + t] = P.jcol[at + t];
        }
      }
    }
    const int l = lane & 15, par = (lane >> 4) & 1;
    const double* tj = P.trigj + (size_t)(l < nq ? l : 0) * (2 * (L + 2)) + 2 * par;
#pragma unroll
    for (int a = 0; a < NM; ++a) {
      cs[a] = tj[4 * a];
      sn[a] = tj[4 * a + 1];
    }
  }
};

// WPP = 2 (two waves per pair): both waves take rows of the first stage (stride 128) and azimuth passes of the second
// (wave h the passes h, h + 2, ...); `half` is the wave's index within the pair.
template <int L, int WPP = 1>
__device__ __forceinline__ void jpoly_build(const PairParams& P, double* __restrict__ lw, const WaveLdsLayout& W,
                                            const int lane, const int nq, const JPolyPre<L>& pre, const double glw_first,
                                            const int half = 0)
{
  // K powers per polynomial; the tables carry one order more than exist (m = L + 1: empty rows of PJ, a real
  // cos/sin pair) so that the azimuth stage below needs no guard on its reads
  constexpr int K = L + 1, NR = jpoly_rows(L) * K, NRI = jpoly_pi_doubles(L), XW = L / 2 + 1, RS = jpoly_row(L);
  // first stage for BOTH particles from one pass over the table rows: particle j's polynomials feed the azimuth stage
  // below, particle i's (the real orders only) are what the ring tables are evaluated from (cap_frame_rings_poly)
  const double* v0 = lw + W.v0;
  const double* v0i = lw + W.v0i;
  double* pj = lw + W.pj;
  double* pi = lw + W.pi;
  if constexpr (JPolyPre<L>::on && WPP == 1) {
#pragma unroll
    for (int ps = 0; ps < JPolyPre<L>::NP; ++ps) {
      const int o = lane + 64 * ps;
      double acc = 0.0, aci = 0.0;
#pragma unroll
      for (int t = 0; t < XW; ++t) {
        acc = fma(pre.val[ps * XW + t], v0[pre.col[ps * XW + t]], acc);
        aci = fma(pre.val[ps * XW + t], v0i[pre.col[ps * XW + t]], aci);
      }
      if (o < NR) pj[o] = acc;
      if (o < NRI) pi[o] = aci;
    }
  } else {
    for (int o = lane + 64 * half; o < NR; o += 64 * WPP) {
      const double* val = P.jval + (size_t)o * XW;
      const int* col = P.jcol + (size_t)o * XW;
      double acc = 0.0, aci = 0.0;
#pragma unroll
      for (int t = 0; t < XW; ++t) {
        acc = fma(val[t], v0[col[t]], acc);
        aci = fma(val[t], v0i[col[t]], aci);
      }
      pj[o] = acc;
      if (o < NRI) pi[o] = aci;
    }
  }
  pair_sync<WPP>();
  // the Gauss-Legendre weights go into the odd slot of the table's rows now that the rotated vectors are out of them
  for (int t = lane + 64 * half; t < nq; t += 64 * WPP) lw[W.glw + t * RS] = (t < 64 * WPP) ? glw_first : P.glw[t];
  // Azimuth stage.  Lanes are (azimuth l, parity of m, parity of k), 16 azimuths per pass: a lane loads the
  // cos/sin(m psi_l) of its orders m = par, par + 2, ... once and walks its powers k = kq, kq + 2, ...; every LDS
  // address is the lane's base plus an immediate.  G (par = 0) has the powers 0..L, H (par = 1) the powers 0..L-1.
  double* gh = lw + W.gh;
  constexpr int NM = L / 2 + 1;                  // orders of one parity (the last may be the empty order L + 1)
  const int par = (lane >> 4) & 1, kq = lane >> 5;
  const int kmax = L - par;
  const double* pjl = pj + (2 * par) * K + kq;   // PJ[2 (2a + par) + part][kq + 2 b] at pjl[(4 a + part) K + 2 b]
  for (int l0 = 16 * half; l0 < nq; l0 += 16 * WPP) {
    const int l = l0 + (lane & 15);
    const bool lok = l < nq;
    double cs[NM], sn[NM];
    if (l0 == 0) {   // wave-uniform: requested at the start of the kernel
#pragma unroll
      for (int a = 0; a < NM; ++a) {
        cs[a] = pre.cs[a];
        sn[a] = pre.sn[a];
      }
    } else {
      const double* tj = P.trigj + (size_t)(lok ? l : 0) * (2 * (L + 2)) + 2 * par;   // (cos, sin)(m psi_l) at tj[4a], tj[4a+1]
#pragma unroll
      for (int a = 0; a < NM; ++a) {
        cs[a] = tj[4 * a];
        sn[a] = tj[4 * a + 1];
      }
    }
    if (lok && kq == 0 && par == 1) {   // the row's own cos(psi_l), sin(psi_l): the first order of the odd lanes
      double* tw = jpoly_trig_sep(L) ? lw + W.tr + 2 * l : gh + l * RS + jpoly_trig(L);
      tw[0] = cs[0];
      tw[1] = sn[0];
    }
    // column of the power k in a row: G: L - k; H: 2L - k  (descending powers, Horner order)
    double* out = gh + (lok ? l : 0) * RS + (par ? 2 * L : L) - kq;
#pragma unroll
    for (int b = 0; b <= L / 2; ++b) {
      double acc = 0.0;
#pragma unroll
      for (int a = 0; a < NM; ++a) {
        acc = fma(cs[a], pjl[(4 * a) * K + 2 * b], acc);
        acc = fma(sn[a], pjl[(4 * a + 1) * K + 2 * b], acc);
      }
      if (lok && kq + 2 * b <= kmax) out[-2 * b] = acc;
    }
  }
  pair_sync<WPP>();
}

// r_j at polar angle (mu, sigma) of the common frame from a lane's row of the per-azimuth table; `sig` carries the
// sign of the azimuth's half (l >= n_q: -).  The row is read from LDS at every evaluation: the 64 lanes of a wave
// address at most n_q distinct rows (the hardware broadcasts), 7 ds_read_b128 at L = 6 beside ~25 v_fma_f64 — and the
// 2L + 1 coefficients do not sit in 4L + 2 registers through the node loops (held there they cost the kernel a wave
// per SIMD, and with the waves the cover for its dependent FP64 chains: 11 cycles from one v_fma_f64 to the next).
template <int L>
__device__ __forceinline__ double jpoly_eval(const double* __restrict__ row, const double mu, const double sig)
{
  // 2L + 1 coefficients in L + 1 aligned 16-byte pairs (the second half of the last pair is the ring weight)
  v2d c[L + 1];
#pragma unroll
  for (int t = 0; t <= L; ++t) c[t] = lds2(row + 2 * t);
  double g = c[0][0];
#pragma unroll
  for (int t = 1; t <= L; ++t) g = fma(g, mu, c[t >> 1][t & 1]);
  if constexpr (L >= 1) {
    double h = c[(L + 1) >> 1][(L + 1) & 1];
#pragma unroll
    for (int t = L + 2; t <= 2 * L; ++t) h = fma(h, mu, c[t >> 1][t & 1]);
    g = fma(sig, h, g);
  }
  return g;
}

// mu- and psi-derivative of r_i at a node of ring row `row` for the JPT kernels, from (cos psi, sin psi) alone: the
// higher orders by the angle-addition recurrence (4 v_fma_f64 per order), no table is read.
template <int L>
__device__ __forceinline__ void ring_grad_rec(const double* __restrict__ row, const double c1, const double s1, double& rmu,
                                              double& rpsi)
{
  rmu = row[2];
  rpsi = 0.0;
  // cos / sin((m + 1) psi) = 2 cos(psi) cos / sin(m psi) - cos / sin((m - 1) psi): ONE v_fma_f64 each (the angle
  // addition form costs two; the three-term form loses ~m^2 ulp, 1e-14 at L = 12, far inside the 1e-9 bar)
  double cm = c1, sm = s1, cp = 1.0, sp = 0.0;
  const double tc = c1 + c1;
#pragma unroll
  for (int m = 1; m <= L; ++m) {
    const v2d ab = lds2(row + 4 * m), dab = lds2(row + 4 * m + 2);   // two ds_read_b128 per order
    const double A = ab[0], B = ab[1], dm = (double)m;
    rmu = fma(dab[0], cm, rmu);
    rmu = fma(dab[1], sm, rmu);
    const double t = fma(B, cm, -(A * sm));   // three instructions per order (m B and m A as products of their own: four)
    rpsi = (m == 1) ? t : fma(dm, t, rpsi);
    if (m < L) {
      const double c = fma(tc, cm, -cp), s = fma(tc, sm, -sp);
      cp = cm;
      sp = sm;
      cm = c;
      sm = s;
    }
  }
}

// r_i at a node of ring row `row` from (cos psi, sin psi), the same recurrence (a direct batch computes it a second time
// behind the inner-radius search instead of carrying it through, see the direct batches of pair_contact_azimuth_kernel)
template <int L>
__device__ __forceinline__ double ring_value(const double* __restrict__ row, const double c1, const double s1)
{
  double r = row[0];
  double cm = c1, sm = s1, cp = 1.0, sp = 0.0;
  const double tc = c1 + c1;
#pragma unroll
  for (int m = 1; m <= L; ++m) {
    const v2d ab = lds2(row + 4 * m);
    r = fma(ab[0], cm, fma(ab[1], sm, r));
    if (m < L) {
      const double c = fma(tc, cm, -cp), s = fma(tc, sm, -sp);
      cp = cm;
      sp = sm;
      cm = c;
      sm = s;
    }
  }
  return r;
}

// Two evaluations from one pass over the row (phase 1: the two nodes of a lane's pair share it)
template <int L>
__device__ __forceinline__ void jpoly_eval2(const double* __restrict__ row, const double mua, const double siga,
                                            const double mub, const double sigb, double& ra, double& rb)
{
  v2d cc[L + 1];
#pragma unroll
  for (int t = 0; t <= L; ++t) cc[t] = lds2(row + 2 * t);
  const double c0 = cc[0][0];
  double ga = c0, gb = c0;
#pragma unroll
  for (int t = 1; t <= L; ++t) {
    const double c = cc[t >> 1][t & 1];
    ga = fma(ga, mua, c);
    gb = fma(gb, mub, c);
  }
  if constexpr (L >= 1) {
    const double h0 = cc[(L + 1) >> 1][(L + 1) & 1];
    double ha = h0, hb = h0;
#pragma unroll
    for (int t = L + 2; t <= 2 * L; ++t) {
      const double c = cc[t >> 1][t & 1];
      ha = fma(ha, mua, c);
      hb = fma(hb, mub, c);
    }
    ga = fma(siga, ha, ga);
    gb = fma(sigb, hb, gb);
  }
  ra = ga;
  rb = gb;
}

}  // namespace shp
