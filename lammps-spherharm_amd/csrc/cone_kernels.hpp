// cone_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.22: the contact of an SH particle with the INSIDE of a one-nappe
// circular cone (a hopper, the end cone of a mill) that may rotate about its own axis.
//
// The structure is the cylinder pass's (cylinder_kernels.hpp), the surface is another.  With y = x_i - a, t = y.a^,
// rho = y - t a^, d = |rho|, c^ = rho / d, the centre's distance to the wall is h = s t - c d (c, s the cosine and sine of
// the half-angle).  The cap lies about the outward wall normal at the nearest generator, n^ = c c^ - s a^, and the frame
// is (g^, n^ x g^, n^) = (g^, c^ x a^, n^) with g^ = s c^ + c a^ the generator, so that u.n^ = mu_k and u.g^ =
// sigma_k cos psi_l come from the node tables and u.a^ = c (u.g^) - s mu_k, u.c^ = s (u.g^) + c mu_k are two FMAs.  Along
// the ray y + lambda u the cone's form s^2 t^2 - c^2 d^2 is G - 2 B lambda - A lambda^2 with
//   A = c^2 q - s^2 ua^2,  B = c^2 d uc - s^2 t ua,  G = (s t - c d)(s t + c d) > 0,      q = 1 - ua^2,
// and the ray leaves the cone at lambda1 = G / (B + sqrt(B^2 + A G)) iff the denominator is positive: the interior of a
// cone is convex, a ray from a centre inside it leaves once.  The discriminant is a sum of squares and is formed as one,
// B^2 + A G = c^2 [s^2 w^2 + (u.e2)^2 G] with w = uc t - ua d; A itself is never formed.  The
// surface point is inside the wall iff lambda1 exists and r_i den > G.  No division in the test, no root search.  Always
// the sharp rule.
// The cap bound is the inscribed sphere's (SPEC §2.22 has the proof): the sphere about the axis point on the normal
// through the centre, radius P = (s d + c t) s / c, touches the cone along the circle through the foot point and lies
// inside it, so every direction that reaches the wall within R_i leaves that sphere within R_i:
//   cos alpha = (h (2 P - h) - R_i^2) / (2 (P - h) R_i), clamped to [-1, 1); -1 within R_i of the apex and on the axis.
// Where the cap is the whole sphere the frame is taken about the axis, (c^, a^ x c^, a^): the nodes keep the symmetry of
// the contact and the force is continuous where a centre crosses the axis.
//
// The pass is described in surface_pass.hpp.  Here: the cone's geometry and the two instances of the contact body,
// cone_contact_kernel (elastic), cone_contact_dissipative_kernel (damping, viscous friction and the rotation Omega
// about the axis; launched only while a cone has a coefficient) and conic_spring_kernel (SPEC §2.23, tangential springs
// with history; launched only while a cone has one), with its live sweep.  A row is (E_k, force on the wall, M_ax).
//
// Included by shstep_cones.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "contact_laws.hpp"
#include "pair_params.hpp"
#include "sh_const.hpp"
#include "sh_device.hpp"
#include "surface_pass.hpp"
#include "wall_sh_grad.hpp"

namespace shp {

constexpr int kMaxCones = 8;          // SHSTEP_MAX_CONES: a particle's cones are one 8-bit mask
constexpr int kConeStride = 10;       // doubles per cone: a[3], axis[3], cos theta, sin theta, kn, exponent
constexpr int kConeCoefRows = 4;      // the coefficient table is [4][ncone]: gamma_k, mu_k, gamma_t,k, Omega
constexpr int kConeRow = 5;           // doubles per (particle, cone) row and per cone total: E_k, F_w[3], M_ax
constexpr int kConeBlock = kSurfBlock;
constexpr int kConeMaxBlocks = kSurfMaxBlocks;

// `surf` holds kConeStride doubles per cone
struct ConeParams : SurfaceParams<unsigned char> {
  const double* coef;    // [kConeCoefRows][ncone]
  const double* twist;   // [nlocal][6]: velocity of the SH origin and angular velocity, space frame
};

#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(ConeParams) == 200 && offsetof(ConeParams, coef) == 184, "ConeParams: kernel-argument layout");

struct ConicSpringParams : SurfaceHistParams<ConeParams, unsigned char> {};   // SPEC §2.23: xi is (xi_g, xi_theta, phi_c)
static_assert(sizeof(ConicSpringParams) == 240 && offsetof(ConicSpringParams, kt) == 200, "ConicSpringParams: kernel-argument layout");
constexpr int kConicXi = 3;           // doubles of history per (particle, cone)

// t = (x - a).axis, rho = (x - a) - t axis, d = |rho| and h = s t - c d of a centre against cone C; the candidate pass
// and the contact kernel form them with the same operations, so they agree on h bit for bit.
struct ConeFoot { double r0, r1, r2, d, t, h; };
__device__ __forceinline__ ConeFoot cone_foot(const double* C, const double px, const double py, const double pz)
{
  const double y0 = px - C[0], y1 = py - C[1], y2 = pz - C[2];
  ConeFoot o;
  o.t = fma(y0, C[3], fma(y1, C[4], y2 * C[5]));
  o.r0 = fma(-o.t, C[3], y0); o.r1 = fma(-o.t, C[4], y1); o.r2 = fma(-o.t, C[5], y2);
  o.d = __builtin_sqrt(fma(o.r0, o.r0, fma(o.r1, o.r1, o.r2 * o.r2)));
  o.h = fma(C[7], o.t, -(C[6] * o.d));
  return o;
}

__global__ __launch_bounds__(kConeBlock) void cone_candidates_kernel(const ConeParams P)
{
  const int i = blockIdx.x * kConeBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  unsigned m = 0;
  int e = 0;
  if (i < P.nlocal) {
    if (P.mask[i] & P.groupbit) {
      const int st = P.shtype[i];
      if (st < 0 || st >= P.nshapes) {
        e = kPairErrShape;
      } else {
        const double R = P.rmax[st];
        const double px = P.x[3 * i], py = P.x[3 * i + 1], pz = P.x[3 * i + 2];
        for (int c = 0; c < P.nsurf; ++c) {
          const double h = cone_foot(P.surf + kConeStride * c, px, py, pz).h;
          if (!(h > 0.0)) e |= kPairErrCone;   // at or outside the wall, behind the apex, or not a number
          else if (h < R) m |= 1u << c;
        }
      }
    }
    P.smask[i] = (unsigned char)m;
  }
  if (e) atomicOr(P.err, e);
  surface_queue_push(m != 0, i, lane, P.count, P.queue);
}

// DISS = false is the elastic contact.  DISS = true adds, behind the wave sums and in the body frame: p_tot = max(0, p +
// gamma_k Vdot) with Vdot = S_n.w + T_n.omega (Omega does not enter: a cone turning about its own axis changes no
// overlap), and the friction F_t = -kappa v_t at the point where the normal wrench's line of action x_i + r_perp + s S^
// leaves the cone: the quadratic of the nodes with (rho + r_perp's part normal to the axis, t + r_perp.a^) in place of
// (rho, t) and S^ in place of u.  With A > 0 the larger root (the line is shallower than the generators and leaves the
// double cone forwards wherever its base lies), otherwise the smaller one, which needs the base inside (G > 0) and a
// positive denominator; no root, or a point that is not on the nappe (t_c <= 0, rho_c = 0): no friction.  v_t is the
// tangential part there of w + omega x r_i - Omega a^ x rho_c, n^_c = s a^ - c rho_c / |rho_c| the inward normal, kappa =
// gamma_t capped at mu N / |v_t|, N = p_tot |S_n|.  The rows' force on the wall is minus the whole force on the
// particle, M_ax the axial moment of that wrench about the axis through the apex.
// HIST = true (with DISS) is the spring law of SPEC §2.23 in place of kappa for a cone with mu_k != 0 and k_t,k != 0, at the
// same contact point and with the same v_t; the lanes, the writer and the live words are cyl_contact_body's.  (xi_g,
// xi_theta) are the components along the generator g^_c = s c^_c + c a^ and t^_c = a^ x c^_c of the accumulated displacement
// against the wall's material, kept with the azimuth phi_c of the contact point they were formed at.  A cone develops
// into a plane sector whose polar angle is beta = s phi, so the components of a parallel-transported vector turn by
// Delta beta = s (Delta phi - Omega dt) when the point moves through Delta phi and the material through Omega dt: one
// atan2 and one sincos per (particle, cone), behind the wave sums.  A cone that fails a guard leaves its bit out of the
// new word.
template <bool DISS, bool HIST = false, typename Params = ConeParams>
__device__ __forceinline__ void cone_contact_body(const Params& P)
{
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nwaves = gridDim.x * (kConeBlock / 64);
  const int count = P.count[0];
  const int nq = P.nq, npsi = 2 * nq, nnodes = npsi * nq;
  int ncontact = 0;
  for (int qi = blockIdx.x * (kConeBlock / 64) + wv; qi < count; qi += nwaves) {
    const int i = __builtin_amdgcn_readfirstlane(P.queue[qi]);
    unsigned cm = (unsigned)__builtin_amdgcn_readfirstlane((int)P.smask[i]);
    const int st = __builtin_amdgcn_readfirstlane(P.shtype[i]);   // in range: the candidate pass checked it
    const double Ri = P.rmax[st];
    const double* cw = P.cw + (size_t)P.cstride * st;
    const double px = P.x[3 * i], py = P.x[3 * i + 1], pz = P.x[3 * i + 2];
    double R[9];
    quat_to_mat(P.quat[4 * i], P.quat[4 * i + 1], P.quat[4 * i + 2], P.quat[4 * i + 3], R);
    double Ft[3] = {0.0, 0.0, 0.0}, Tt[3] = {0.0, 0.0, 0.0};
    double twb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // DISS: the twist in the body frame, v_b = R^T v
    if constexpr (DISS) {
      const double* tw = P.twist + 6 * (size_t)i;   // (twin text in wall_contact_body and cyl_contact_body)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        twb[k] = R[k] * tw[0] + R[3 + k] * tw[1] + R[6 + k] * tw[2];
        twb[3 + k] = R[k] * tw[3] + R[3 + k] * tw[4] + R[6 + k] * tw[5];
      }
    }
    unsigned lv = 0, nl = 0;   // HIST: the particle's live word as it was, and as this pass leaves it
    if constexpr (HIST) lv = P.live_dead ? 0u : (unsigned)__builtin_amdgcn_readfirstlane((int)P.live[i]);
    while (cm) {
      const int c = __builtin_ctz(cm);
      cm &= cm - 1;
      const double* C = P.surf + kConeStride * c;
      const ConeFoot ft = cone_foot(C, px, py, pz);
      const double d = ft.d, tt = ft.t, h = ft.h, ct = C[6], sn_ = C[7];
      const double ax[3] = {C[3], C[4], C[5]};
      // the inscribed sphere's bound: cos alpha = (h (2 P - h) - R_i^2) / (2 (P - h) R_i) clamped to [-1, 1), formed
      // without dividing where it is clamped; the whole sphere within R_i of the apex, and on the axis
      const double sg = fma(sn_, d, ct * tt);        // y.g^: the foot point's place along its generator
      const double Ps = sg * sn_ / ct;
      const double num = fma(h, 2.0 * Ps - h, -(Ri * Ri)), den = 2.0 * (Ps - h) * Ri;
      const bool whole = fma(d, d, tt * tt) <= Ri * Ri || !(d > 0.0) || num <= -den;
      const double ca = whole ? -1.0 : (num >= den ? 0x1.fffffffffffffp-1 : num / den);
      // c^ = rho / d; on the axis (d = 0 as computed) the e1 of the frame rule of SPEC §2.3 about the axis.  The frame is
      // (g^, c^ x a^, n^) with g^ = s c^ + c a^ and n^ = c c^ - s a^.  Where the cap is the whole sphere its pole is free,
      // and the frame is taken about the axis, (c^, a^ x c^, a^): the nodes then keep the symmetry of the contact, and
      // they map onto themselves when the centre crosses the axis (c^ -> -c^ is a turn by pi, n_q azimuth steps), so the
      // force is continuous there.  (k1, k2) and (k3, k4) give u.a^ and u.c^ from u.b1 and u.bc in either frame.
      double gn[3], nn[3], e2[3];
      double k1 = ct, k2 = -sn_, k3 = sn_, k4 = ct;
      const AxialUnit cu = axial_radial_unit(d, ft.r0, ft.r1, ft.r2, ax[0], ax[1], ax[2]);
      const double cc[3] = {cu.c0, cu.c1, cu.c2};
      if (!whole) {
        e2[0] = cc[1] * ax[2] - cc[2] * ax[1]; e2[1] = cc[2] * ax[0] - cc[0] * ax[2]; e2[2] = cc[0] * ax[1] - cc[1] * ax[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          gn[k] = fma(sn_, cc[k], ct * ax[k]);
          nn[k] = fma(ct, cc[k], -(sn_ * ax[k]));
        }
      } else {
        e2[0] = ax[1] * cc[2] - ax[2] * cc[1]; e2[1] = ax[2] * cc[0] - ax[0] * cc[2]; e2[2] = ax[0] * cc[1] - ax[1] * cc[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          gn[k] = cc[k];
          nn[k] = ax[k];
        }
        k1 = 0.0; k2 = 1.0; k3 = 1.0; k4 = 0.0;
      }
      // rotated into the body frame: v_b = R^T v
      double b1[3], b2[3], bc[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b1[k] = R[k] * gn[0] + R[3 + k] * gn[1] + R[6 + k] * gn[2];
        b2[k] = R[k] * e2[0] + R[3 + k] * e2[1] + R[6 + k] * e2[2];
        bc[k] = R[k] * nn[0] + R[3 + k] * nn[1] + R[6 + k] * nn[2];
      }
      const double hm = 0.5 * (1.0 + ca), hw = 0.5 * (1.0 - ca);
      const double wsc = hw * (3.14159265358979323846264338327950288 / nq);
      const double c2 = ct * ct, s2 = sn_ * sn_;
      const double G = h * fma(sn_, tt, ct * d);   // (s t - c d)(s t + c d)
      const double Bd = c2 * d, Bt = s2 * tt;
      double V = 0.0, S0 = 0.0, S1 = 0.0, S2 = 0.0, T0 = 0.0, T1 = 0.0, T2 = 0.0;
#pragma unroll 1
      for (int t = lane; t < nnodes; t += 64) {
        const int k = t / npsi, l = t - k * npsi;
        const SurfaceNode nd = surface_node(hw, hm, P.glt[k], P.cpsi[l], P.spsi[l], b1[0], b1[1], b1[2], b2[0], b2[1], b2[2], bc[0], bc[1], bc[2]);
        const double mu = nd.mu, cp = nd.cp, u0 = nd.u0, u1 = nd.u1, u2 = nd.u2;
        double r, g0, g1, g2;
        wall_sh_grad(P.rc, cw, P.lmax, u0, u1, u2, r, g0, g1, g2);
        const double ua = fma(k1, cp, k2 * mu), uc = fma(k3, cp, k4 * mu);   // u.b1 = cp, u.bc = mu
        // B^2 + A G as the sum of squares it is, c^2 [s^2 w^2 + (u.e2)^2 G] with w = uc t - ua d: never
        // negative, and no cancellation as theta -> pi/2, where the plain form loses every digit
        const double B = fma(Bd, uc, -(Bt * ua)), w = fma(uc, tt, -(ua * d));
        const double dn = fma(ct, __builtin_sqrt(fma(s2 * w, w, nd.sp * nd.sp * G)), B);
        if (dn > 0.0 && r * dn > G) {   // the ray leaves the cone, and the surface point lies beyond: inside the wall
          const double om = wsc * P.glw[k];
          const SurfaceSums Z = surface_add_area(S0, S1, S2, T0, T1, T2, om, r, u0, u1, u2, g0, g1, g2);
          S0 = Z.S0; S1 = Z.S1; S2 = Z.S2; T0 = Z.T0; T1 = Z.T1; T2 = Z.T2;
          V = surface_add_volume(V, om, r, G / dn);
        }
      }
      V = wave_sum(V);
      S0 = wave_sum(S0); S1 = wave_sum(S1); S2 = wave_sum(S2);
      T0 = wave_sum(T0); T1 = wave_sum(T1); T2 = wave_sum(T2);
      double E = 0.0, Fw[3] = {0.0, 0.0, 0.0}, Tw[3] = {0.0, 0.0, 0.0};
      if (V > 0.0) {
        const double kn = C[8], ex = C[9];
        const double pn = pair_pressure(kn, ex, V);
        E = pn * V / ex;   // kn V^m
        double pt = pn;
        // minus the particle's wrench in the body frame: pt S - F_t, pt T - r_i x F_t
        double Gf[3], Gt[3];
        if constexpr (DISS) {
          const double vd = fma(S0, twb[0], fma(S1, twb[1], fma(S2, twb[2], fma(T0, twb[3], fma(T1, twb[4], T2 * twb[5])))));
          pt = fmax(0.0, fma(P.coef[c], vd, pn));   // the wall never pulls
          Gf[0] = pt * S0; Gf[1] = pt * S1; Gf[2] = pt * S2;
          Gt[0] = pt * T0; Gt[1] = pt * T1; Gt[2] = pt * T2;
          const double mu = P.coef[P.nsurf + c], gt = P.coef[2 * P.nsurf + c], Om = P.coef[3 * P.nsurf + c];
          const double qq = fma(S0, S0, fma(S1, S1, S2 * S2));
          const double sn = __builtin_sqrt(qq), N = pt * sn;
          double kt = 0.0;
          bool hist = false;   // this cone takes the spring law
          if constexpr (HIST) {
            kt = P.kt[c];
            hist = mu != 0.0 && kt != 0.0;
          }
          if ((HIST ? (mu != 0.0 && (gt != 0.0 || hist)) : (mu != 0.0 && gt != 0.0)) && qq > 0.0 && N > 0.0) {
            const double qinv = 1.0 / qq, sinv = 1.0 / sn;
            const double rp[3] = {(S1 * T2 - S2 * T1) * qinv, (S2 * T0 - S0 * T2) * qinv, (S0 * T1 - S1 * T0) * qinv};
            const double sh[3] = {S0 * sinv, S1 * sinv, S2 * sinv};
            // a^ and c^ in the body frame, from the frame's two: a^ = c g^ - s n^, c^ = s g^ + c n^ (the frame about the axis: bc, b1)
            double ba[3], bcc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              ba[k] = fma(k1, b1[k], k2 * bc[k]);
              bcc[k] = fma(k3, b1[k], k4 * bc[k]);
            }
            // the axial and the normal-to-axis parts of x_i - a + r_perp and of S^
            const double ra = rp[0] * ba[0] + rp[1] * ba[1] + rp[2] * ba[2];
            const double sa = sh[0] * ba[0] + sh[1] * ba[1] + sh[2] * ba[2];
            const double t0 = tt + ra;
            double r0[3], sp[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              r0[k] = fma(d, bcc[k], rp[k] - ra * ba[k]);
              sp[k] = sh[k] - sa * ba[k];
            }
            const double Aq = fma(c2, sp[0] * sp[0] + sp[1] * sp[1] + sp[2] * sp[2], -(s2 * sa * sa));
            const double Bq = fma(c2, r0[0] * sp[0] + r0[1] * sp[1] + r0[2] * sp[2], -(s2 * t0 * sa));
            const double Gq = fma(s2 * t0, t0, -(c2 * fma(r0[0], r0[0], fma(r0[1], r0[1], r0[2] * r0[2]))));
            const double D = fma(Bq, Bq, Aq * Gq);
            bool ok = D >= 0.0;
            double s = 0.0;
            if (ok) {
              const double sq = __builtin_sqrt(D), dn = Bq + sq;
              if (Aq > 0.0) s = Bq > 0.0 ? Gq / dn : (sq - Bq) / Aq;   // the larger root, without cancellation
              else if (Gq > 0.0 && dn > 0.0) s = Gq / dn;              // the smaller root: the exit from the nappe
              else ok = false;                                        // S^ never leaves
            }
            double ri[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              ri[k] = fma(s, sh[k], rp[k]);
              r0[k] = fma(s, sp[k], r0[k]);   // rho_c
            }
            const double tc = fma(s, sa, t0);
            const double dc = __builtin_sqrt(fma(r0[0], r0[0], fma(r0[1], r0[1], r0[2] * r0[2])));
            if (ok && tc > 0.0 && dc > 0.0) {
              const double cd = ct / dc;
              const double nc[3] = {fma(sn_, ba[0], -(cd * r0[0])), fma(sn_, ba[1], -(cd * r0[1])), fma(sn_, ba[2], -(cd * r0[2]))};
              // w + omega x r_i - Omega a^ x rho_c
              const double vr[3] = {twb[0] + (twb[4] * ri[2] - twb[5] * ri[1]) - Om * (ba[1] * r0[2] - ba[2] * r0[1]),
                                    twb[1] + (twb[5] * ri[0] - twb[3] * ri[2]) - Om * (ba[2] * r0[0] - ba[0] * r0[2]),
                                    twb[2] + (twb[3] * ri[1] - twb[4] * ri[0]) - Om * (ba[0] * r0[1] - ba[1] * r0[0])};
              const double vn = vr[0] * nc[0] + vr[1] * nc[1] + vr[2] * nc[2];
              const double vt[3] = {vr[0] - vn * nc[0], vr[1] - vn * nc[1], vr[2] - vn * nc[2]};
              const double vtn = __builtin_sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
              const double kappa = capped_coefficient(gt, vtn, mu * N);
              double fr[3] = {-kappa * vt[0], -kappa * vt[1], -kappa * vt[2]};
              if constexpr (HIST) {
                if (hist) {
                  // the surface frame at the contact point, body frame: c^_c = rho_c / |rho_c|, g^_c = s c^_c + c a^, t^_c = a^ x c^_c
                  const double dci = 1.0 / dc;
                  const double ch[3] = {r0[0] * dci, r0[1] * dci, r0[2] * dci};
                  const double gc[3] = {fma(sn_, ch[0], ct * ba[0]), fma(sn_, ch[1], ct * ba[1]), fma(sn_, ch[2], ct * ba[2])};
                  const double th[3] = {ba[1] * ch[2] - ba[2] * ch[1], ba[2] * ch[0] - ba[0] * ch[2], ba[0] * ch[1] - ba[1] * ch[0]};
                  // phi_c = atan2(rho_c.e2, rho_c.e1) in the space frame: e1 the frame rule's vector about a^, e2 = a^ x e1
                  const double rs[3] = {R[0] * r0[0] + R[1] * r0[1] + R[2] * r0[2], R[3] * r0[0] + R[4] * r0[1] + R[5] * r0[2],
                                        R[6] * r0[0] + R[7] * r0[1] + R[8] * r0[2]};
                  const AxialUnit fu = axis_frame_e1(ax[0], ax[1], ax[2]);
                  const double f1[3] = {fu.c0, fu.c1, fu.c2};
                  const double f2[3] = {ax[1] * f1[2] - ax[2] * f1[1], ax[2] * f1[0] - ax[0] * f1[2], ax[0] * f1[1] - ax[1] * f1[0]};
                  const double phi = atan2(rs[0] * f2[0] + rs[1] * f2[1] + rs[2] * f2[2], rs[0] * f1[0] + rs[1] * f1[1] + rs[2] * f1[2]);
                  double* X = P.xi + ((size_t)i * P.nsurf + c) * kConicXi;
                  double xg = 0.0, xt = 0.0;
                  if ((lv >> c) & 1u) {   // the transport: Delta beta = s (wrap(phi' - phi) - Omega dt)
                    const double x0 = X[0], x1 = X[1];
                    double dp = phi - X[2];
                    if (dp > 3.14159265358979323846264338327950288) dp -= 6.28318530717958647692528676655900577;
                    else if (dp <= -3.14159265358979323846264338327950288) dp += 6.28318530717958647692528676655900577;
                    const double db = sn_ * (dp - Om * P.dt);
                    const double sb = sin(db), cb = cos(db);
                    xg = x0 * cb + x1 * sb;
                    xt = x1 * cb - x0 * sb;
                  }
                  xg = fma(P.dt, vt[0] * gc[0] + vt[1] * gc[1] + vt[2] * gc[2], xg);
                  xt = fma(P.dt, vt[0] * th[0] + vt[1] * th[1] + vt[2] * th[2], xt);
#pragma unroll
                  for (int k = 0; k < 3; ++k) fr[k] = -kt * (xg * gc[k] + xt * th[k]) - gt * vt[k];   // the trial force F*
                  const double cap = mu * N;
                  const double fn = __builtin_sqrt(fr[0] * fr[0] + fr[1] * fr[1] + fr[2] * fr[2]);
                  if (!(fn <= cap)) {   // slides: the capped force, and the xi it can hold
                    const double sc = cap / fn;
                    double hh[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                      fr[k] *= sc;
                      hh[k] = -(fr[k] + gt * vt[k]) / kt;
                    }
                    xg = hh[0] * gc[0] + hh[1] * gc[1] + hh[2] * gc[2];
                    xt = hh[0] * th[0] + hh[1] * th[1] + hh[2] * th[2];
                  }
                  nl |= 1u << c;
                  if (P.dt > 0.0 && lane == 0) { X[0] = xg; X[1] = xt; X[2] = phi; }
                }
              }
              Gf[0] -= fr[0]; Gf[1] -= fr[1]; Gf[2] -= fr[2];
              Gt[0] -= ri[1] * fr[2] - ri[2] * fr[1];
              Gt[1] -= ri[2] * fr[0] - ri[0] * fr[2];
              Gt[2] -= ri[0] * fr[1] - ri[1] * fr[0];
            }
          }
        } else {
          Gf[0] = pt * S0; Gf[1] = pt * S1; Gf[2] = pt * S2;
          Gt[0] = pt * T0; Gt[1] = pt * T1; Gt[2] = pt * T2;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // back to the space frame: v = R v_b (twin text in wall_contact_body and cyl_contact_body)
          Fw[k] = R[3 * k] * Gf[0] + R[3 * k + 1] * Gf[1] + R[3 * k + 2] * Gf[2];
          Tw[k] = R[3 * k] * Gt[0] + R[3 * k + 1] * Gt[1] + R[3 * k + 2] * Gt[2];
          Ft[k] -= Fw[k];
          Tt[k] -= Tw[k];
        }
        ++ncontact;
      }
      if (P.rows && lane == 0) {
        // M_ax = axis . [(x_i - a) x F_w + T_w]: the wall's wrench F_w, T_w is minus the particle's F_i, tau_i
        const double y0 = px - C[0], y1 = py - C[1], y2 = pz - C[2];
        const double m0 = y1 * Fw[2] - y2 * Fw[1] + Tw[0], m1 = y2 * Fw[0] - y0 * Fw[2] + Tw[1], m2 = y0 * Fw[1] - y1 * Fw[0] + Tw[2];
        double* row = P.rows + ((size_t)i * P.nsurf + c) * kConeRow;
        row[0] = E; row[1] = Fw[0]; row[2] = Fw[1]; row[3] = Fw[2];
        row[4] = ax[0] * m0 + ax[1] * m1 + ax[2] * m2;
      }
    }
    if (lane == 0) {   // the only writer of row i at this point of the stream
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        P.f[3 * i + k] += Ft[k];
        P.torque[3 * i + k] += Tt[k];
      }
      if constexpr (HIST) {
        if (P.dt > 0.0) P.live[i] = (unsigned char)nl;
      }
    }
  }
  if (lane == 0 && ncontact) atomicAdd(P.count + 1, ncontact);
}

// The two instances
__global__ __launch_bounds__(kConeBlock) void cone_contact_kernel(const ConeParams P) { cone_contact_body<false>(P); }
__global__ __launch_bounds__(kConeBlock) void cone_contact_dissipative_kernel(const ConeParams P) { cone_contact_body<true>(P); }

// ... and the one while a cone has a tangential spring (SPEC §2.23), launched only then
__global__ __launch_bounds__(kConeBlock) void conic_spring_kernel(const ConicSpringParams P) { cone_contact_body<true, true, ConicSpringParams>(P); }

// The live sweep of an advancing pass (SPEC §2.23), behind the candidate pass: a particle that left a cone's reach is not
// visited by the contact kernel for that cone (or at all), so the bits of the cones out of its mask die here.
__global__ __launch_bounds__(kConeBlock) void conic_live_sweep_kernel(int nlocal, const unsigned char* __restrict__ kmask,
                                                                      unsigned char* __restrict__ live)
{
  surface_live_sweep(nlocal, live, kmask);
}

// ---- per-cone totals in a fixed order (surface_pass.hpp): rows of kConeRow
__global__ __launch_bounds__(kConeBlock) void cone_rows_partial_kernel(int nlocal, int ncone, const unsigned char* __restrict__ kmask,
                                                                        const double* __restrict__ rows, double* __restrict__ part)
{
  surface_rows_partial<kConeRow>(nlocal, ncone, kmask, rows, part);
}

__global__ __launch_bounds__(kConeBlock) void cone_rows_final_kernel(int nb, const double* __restrict__ part, double* __restrict__ cone_out)
{
  surface_rows_final<kConeRow>(nb, part, cone_out);
}

}  // namespace shp
