// cylinder_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.18: the contact of an SH particle with the INSIDE of a
// circular cylinder that may rotate about its own axis.
//
// The structure is the planar pass's (wall_kernels.hpp), the surface is another: the cap lies about c = rho / d, the
// frame is (e1, e2, c) = (a, c x a, c) with a the axis, so that u.a = sigma_k cos psi_l and u.c = mu_k come from the node
// tables, the inside test is (q r + 2 b) r > g with q = 1 - (u.a)^2, b = d mu_k, g = Rc^2 - d^2, and the inner radius is
// the closed form r_in = g / (b + sqrt(b^2 + q g)): the interior of a cylinder is convex, a ray from a centre inside it
// leaves once.  No division in the test, no root search.  Always the sharp rule.
//
// The pass is described in surface_pass.hpp, which holds what it shares with the planar pass.  Here: the cylinder's
// geometry and the three instances of the contact body: cyl_contact_kernel (elastic), cyl_contact_dissipative_kernel
// (damping, viscous friction and the rotation Omega about the axis; launched only while a cylinder has a coefficient)
// and cyl_spring_kernel (SPEC §2.19).  A row is (E_c, force on the wall, M_ax).
//
// Included by shstep_cylinders.hip only (the kernels are not templates: one definition per library), and by
// cyl_power_kernels.hpp, which that file includes for the LEDGER instances of the contact body (SPEC §2.20).
#pragma once
#include <hip/hip_runtime.h>

#include "contact_laws.hpp"
#include "pair_params.hpp"
#include "sh_const.hpp"
#include "sh_device.hpp"
#include "surface_pass.hpp"
#include "wall_sh_grad.hpp"

namespace shp {

constexpr int kMaxCylinders = 8;     // SHSTEP_MAX_CYLINDERS: a particle's cylinders are one 8-bit mask
constexpr int kCylStride = 9;        // doubles per cylinder: a[3], axis[3], Rc, kn, exponent
constexpr int kCylCoefRows = 4;      // the coefficient table is [4][ncyl]: gamma_c, mu_c, gamma_t,c, Omega
constexpr int kCylRow = 5;           // doubles per (particle, cylinder) row and per cylinder total: E_c, F_w[3], M_ax
constexpr int kCylPowerRow = 3;      // SPEC §2.20: doubles per (particle, cylinder) power row and per shell entry: P_d, P_f, Wdot_c
constexpr int kCylBlock = kSurfBlock;
constexpr int kCylMaxBlocks = kSurfMaxBlocks;

// `surf` holds kCylStride doubles per cylinder
struct CylParams : SurfaceParams<unsigned char> {
  const double* coef;    // [kCylCoefRows][ncyl]
  const double* twist;   // [nlocal][6]: velocity of the SH origin and angular velocity, space frame
};

struct CylSpringParams : SurfaceHistParams<CylParams, unsigned char> {};   // SPEC §2.19: xi is (xi_a, xi_theta)

// the kernel arguments lie where they always lay
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(CylParams) == 200 && offsetof(CylParams, coef) == 184, "CylParams: kernel-argument layout");
static_assert(sizeof(CylSpringParams) == 240 && offsetof(CylSpringParams, kt) == 200, "CylSpringParams: kernel-argument layout");

// rho = (x - a) - ((x - a).axis) axis and d = |rho| of a centre against cylinder C; the candidate pass and the contact
// kernel form them with the same operations, so they agree on h = Rc - d bit for bit.
struct CylFoot { double r0, r1, r2, d; };
__device__ __forceinline__ CylFoot cyl_foot(const double* C, const double px, const double py, const double pz)
{
  const double y0 = px - C[0], y1 = py - C[1], y2 = pz - C[2];
  const double t = fma(y0, C[3], fma(y1, C[4], y2 * C[5]));
  CylFoot o;
  o.r0 = fma(-t, C[3], y0); o.r1 = fma(-t, C[4], y1); o.r2 = fma(-t, C[5], y2);
  o.d = __builtin_sqrt(fma(o.r0, o.r0, fma(o.r1, o.r1, o.r2 * o.r2)));
  return o;
}

__global__ __launch_bounds__(kCylBlock) void cyl_candidates_kernel(const CylParams P)
{
  const int i = blockIdx.x * kCylBlock + threadIdx.x;
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
          const double* C = P.surf + kCylStride * c;
          const double d = cyl_foot(C, px, py, pz).d;
          if (!(d < C[6])) e |= kPairErrCylinder;   // at or outside the cylinder, or not a number
          else if (C[6] - d < R) m |= 1u << c;
        }
      }
    }
    P.smask[i] = (unsigned char)m;
  }
  if (e) atomicOr(P.err, e);
  surface_queue_push(m != 0, i, lane, P.count, P.queue);
}

// DISS = false is the elastic contact.  DISS = true adds, behind the wave sums and in the body frame: p_tot = max(0, p +
// gamma_c Vdot) with Vdot = S_n.w + T_n.omega (Omega does not enter: a cylinder turning about its own axis changes no
// overlap), and the friction F_t = -kappa v_t at the point where the normal wrench's line of action x_i + r_perp + s S^
// leaves the cylinder, v_t the tangential part there of w + omega x r_i - Omega a x rho_c, kappa = gamma_t capped at
// mu N / |v_t|, N = p_tot |S_n|.  The rows' force on the wall is minus the whole force on the particle, M_ax the axial
// moment of that wrench about the axis.
// HIST = true (with DISS) is the spring law of SPEC §2.19 in place of kappa for a cylinder with mu_c != 0 and k_t,c != 0,
// at the same contact point and with the same v_t; the lanes, the writer and the live words are wall_contact_body's.
// (xi_a, xi_theta) are the components along a (b1 here) and t^_c = a x rho_c / Rc of the accumulated displacement against
// the wall's material: a cylinder is developable, so the two numbers ARE the spring's parallel transport along the
// surface; nothing is rotated or projected, and a particle carried round by the drum keeps them.  A cylinder that fails a
// guard (V <= 0, |S_n| = 0, N = 0, A = 0, D < 0) leaves its bit out of the new word.
// LEDGER = true (with DISS; cyl_power_kernels.hpp) is the pass while the energy ledger and the shell ledger are on (SPEC
// §2.20): lane 0 also leaves a row (P_d, P_f, Wdot_c) per cylinder of the particle's mask, zeros where V <= 0 or a guard
// drops the friction: P_d = (p_tot - p) Vdot, P_f = kappa |v_t|^2 (-F_t.v_t for a history cylinder) and Wdot_c =
// Omega F_t.(a x rho_c), the power the drive delivers.  Nothing else changes: f, torque, the rows, xi and the live words
// keep the bits of the other instances.
template <bool DISS, bool HIST = false, typename Params = CylParams, bool LEDGER = false>
__device__ __forceinline__ void cyl_contact_body(const Params& P)
{
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nwaves = gridDim.x * (kCylBlock / 64);
  const int count = P.count[0];
  const int nq = P.nq, npsi = 2 * nq, nnodes = npsi * nq;
  int ncontact = 0;
  for (int qi = blockIdx.x * (kCylBlock / 64) + wv; qi < count; qi += nwaves) {
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
      const double* tw = P.twist + 6 * (size_t)i;   // (twin text in wall_contact_body: no helper form keeps the kernels)
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
      const double* C = P.surf + kCylStride * c;
      const CylFoot ft = cyl_foot(C, px, py, pz);
      const double d = ft.d, Rc = C[6];
      const double ax[3] = {C[3], C[4], C[5]};
      // c = rho / d; on the axis (d = 0 as computed) the e1 of the frame rule of SPEC §2.3 about the axis
      const AxialUnit cu = axial_radial_unit(d, ft.r0, ft.r1, ft.r2, ax[0], ax[1], ax[2]);
      const double cc[3] = {cu.c0, cu.c1, cu.c2};
      // frame (e1, e2, c) = (a, c x a, c), rotated into the body frame: v_b = R^T v
      const double e2[3] = {cc[1] * ax[2] - cc[2] * ax[1], cc[2] * ax[0] - cc[0] * ax[2], cc[0] * ax[1] - cc[1] * ax[0]};
      double b1[3], b2[3], bc[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b1[k] = R[k] * ax[0] + R[3 + k] * ax[1] + R[6 + k] * ax[2];
        b2[k] = R[k] * e2[0] + R[3 + k] * e2[1] + R[6 + k] * e2[2];
        bc[k] = R[k] * cc[0] + R[3 + k] * cc[1] + R[6 + k] * cc[2];
      }
      // cos alpha = (g - R_i^2) / (2 d R_i) clamped to [-1, 1), formed without dividing where it is clamped
      const double g = (Rc - d) * (Rc + d);
      const double num = fma(-Ri, Ri, g), den = 2.0 * d * Ri;
      const double ca = num <= -den ? -1.0 : (num >= den ? 0x1.fffffffffffffp-1 : num / den);
      const double hm = 0.5 * (1.0 + ca), hw = 0.5 * (1.0 - ca);
      const double wsc = hw * (3.14159265358979323846264338327950288 / nq);
      double V = 0.0, S0 = 0.0, S1 = 0.0, S2 = 0.0, T0 = 0.0, T1 = 0.0, T2 = 0.0;
#pragma unroll 1
      for (int t = lane; t < nnodes; t += 64) {
        const int k = t / npsi, l = t - k * npsi;
        const SurfaceNode nd = surface_node(hw, hm, P.glt[k], P.cpsi[l], P.spsi[l], b1[0], b1[1], b1[2], b2[0], b2[1], b2[2], bc[0], bc[1], bc[2]);
        const double mu = nd.mu, cp = nd.cp, u0 = nd.u0, u1 = nd.u1, u2 = nd.u2;
        double r, g0, g1, g2;
        wall_sh_grad(P.rc, cw, P.lmax, u0, u1, u2, r, g0, g1, g2);
        const double q = fma(-cp, cp, 1.0), b = d * mu;   // u.a = cp, u.c = mu
        if (fma(q, r, 2.0 * b) * r > g) {   // the surface point is inside the wall
          const double om = wsc * P.glw[k];
          const SurfaceSums A = surface_add_area(S0, S1, S2, T0, T1, T2, om, r, u0, u1, u2, g0, g1, g2);
          S0 = A.S0; S1 = A.S1; S2 = A.S2; T0 = A.T0; T1 = A.T1; T2 = A.T2;
          const double rin = g / (b + __builtin_sqrt(fma(b, b, q * g)));
          V = surface_add_volume(V, om, r, rin);
        }
      }
      V = wave_sum(V);
      S0 = wave_sum(S0); S1 = wave_sum(S1); S2 = wave_sum(S2);
      T0 = wave_sum(T0); T1 = wave_sum(T1); T2 = wave_sum(T2);
      double E = 0.0, Fw[3] = {0.0, 0.0, 0.0}, Tw[3] = {0.0, 0.0, 0.0};
      double Pd = 0.0, Pf = 0.0, Wc = 0.0;   // LEDGER only
      if (V > 0.0) {
        const double kn = C[7], ex = C[8];
        const double pn = pair_pressure(kn, ex, V);
        E = pn * V / ex;   // kn V^m
        double pt = pn;
        // minus the particle's wrench in the body frame: pt S - F_t, pt T - r_i x F_t
        double Gf[3], Gt[3];
        if constexpr (DISS) {
          const double vd = fma(S0, twb[0], fma(S1, twb[1], fma(S2, twb[2], fma(T0, twb[3], fma(T1, twb[4], T2 * twb[5])))));
          pt = fmax(0.0, fma(P.coef[c], vd, pn));   // the wall never pulls
          if constexpr (LEDGER) Pd = (pt - pn) * vd;
          Gf[0] = pt * S0; Gf[1] = pt * S1; Gf[2] = pt * S2;
          Gt[0] = pt * T0; Gt[1] = pt * T1; Gt[2] = pt * T2;
          const double mu = P.coef[P.nsurf + c], gt = P.coef[2 * P.nsurf + c], Om = P.coef[3 * P.nsurf + c];
          const double qq = fma(S0, S0, fma(S1, S1, S2 * S2));
          const double sn = __builtin_sqrt(qq), N = pt * sn;
          double kt = 0.0;
          bool hist = false;   // this cylinder takes the spring law
          if constexpr (HIST) {
            kt = P.kt[c];
            hist = mu != 0.0 && kt != 0.0;
          }
          if ((HIST ? (mu != 0.0 && (gt != 0.0 || hist)) : (mu != 0.0 && gt != 0.0)) && qq > 0.0 && N > 0.0) {
            const double qinv = 1.0 / qq, sinv = 1.0 / sn;
            const double rp[3] = {(S1 * T2 - S2 * T1) * qinv, (S2 * T0 - S0 * T2) * qinv, (S0 * T1 - S1 * T0) * qinv};
            const double sh[3] = {S0 * sinv, S1 * sinv, S2 * sinv};
            // the parts normal to the axis (b1 in the body frame) of x_i - a + r_perp and of S^
            const double ra = rp[0] * b1[0] + rp[1] * b1[1] + rp[2] * b1[2];
            const double sa = sh[0] * b1[0] + sh[1] * b1[1] + sh[2] * b1[2];
            double r0[3], sp[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              r0[k] = fma(d, bc[k], rp[k] - ra * b1[k]);
              sp[k] = sh[k] - sa * b1[k];
            }
            const double A = sp[0] * sp[0] + sp[1] * sp[1] + sp[2] * sp[2];
            const double B = r0[0] * sp[0] + r0[1] * sp[1] + r0[2] * sp[2];
            const double Cq = fma(r0[0], r0[0], fma(r0[1], r0[1], r0[2] * r0[2])) - Rc * Rc;
            const double D = fma(B, B, -(A * Cq));
            if (A > 0.0 && D >= 0.0) {   // S^ along the axis, or a line that misses the cylinder: no friction
              const double sq = __builtin_sqrt(D);
              const double s = B > 0.0 ? -Cq / (B + sq) : (sq - B) / A;   // the larger root, without cancellation
              double ri[3], nc[3];
#pragma unroll
              for (int k = 0; k < 3; ++k) {
                ri[k] = fma(s, sh[k], rp[k]);
                r0[k] = fma(s, sp[k], r0[k]);   // rho_c
                nc[k] = -r0[k] / Rc;
              }
              // w + omega x r_i - Omega a x rho_c
              const double vr[3] = {twb[0] + (twb[4] * ri[2] - twb[5] * ri[1]) - Om * (b1[1] * r0[2] - b1[2] * r0[1]),
                                    twb[1] + (twb[5] * ri[0] - twb[3] * ri[2]) - Om * (b1[2] * r0[0] - b1[0] * r0[2]),
                                    twb[2] + (twb[3] * ri[1] - twb[4] * ri[0]) - Om * (b1[0] * r0[1] - b1[1] * r0[0])};
              const double vn = vr[0] * nc[0] + vr[1] * nc[1] + vr[2] * nc[2];
              const double vt[3] = {vr[0] - vn * nc[0], vr[1] - vn * nc[1], vr[2] - vn * nc[2]};
              const double vtn = __builtin_sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
              const double cap = mu * N;
              const double kappa = capped_coefficient(gt, vtn, cap);
              double fr[3] = {-kappa * vt[0], -kappa * vt[1], -kappa * vt[2]};
              if constexpr (LEDGER) Pf = kappa * (vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
              if constexpr (HIST) {
                if (hist) {
                  // t^_c = a x rho_c / Rc, the direction the wall moves for Omega > 0
                  const double tc[3] = {(b1[1] * r0[2] - b1[2] * r0[1]) / Rc, (b1[2] * r0[0] - b1[0] * r0[2]) / Rc,
                                        (b1[0] * r0[1] - b1[1] * r0[0]) / Rc};
                  double* X = P.xi + ((size_t)i * P.nsurf + c) * 2;
                  double xa = 0.0, xt = 0.0;
                  if ((lv >> c) & 1u) { xa = X[0]; xt = X[1]; }
                  xa = fma(P.dt, vt[0] * b1[0] + vt[1] * b1[1] + vt[2] * b1[2], xa);
                  xt = fma(P.dt, vt[0] * tc[0] + vt[1] * tc[1] + vt[2] * tc[2], xt);
#pragma unroll
                  for (int k = 0; k < 3; ++k) fr[k] = -kt * (xa * b1[k] + xt * tc[k]) - gt * vt[k];   // the trial force F*
                  const double fn = __builtin_sqrt(fr[0] * fr[0] + fr[1] * fr[1] + fr[2] * fr[2]);
                  if (!(fn <= cap)) {   // slides: the capped force, and the xi it can hold
                    const double sc = cap / fn;
                    double h[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                      fr[k] *= sc;
                      h[k] = -(fr[k] + gt * vt[k]) / kt;
                    }
                    xa = h[0] * b1[0] + h[1] * b1[1] + h[2] * b1[2];
                    xt = h[0] * tc[0] + h[1] * tc[1] + h[2] * tc[2];
                  }
                  nl |= 1u << c;
                  if (P.dt > 0.0 && lane == 0) { X[0] = xa; X[1] = xt; }
                  if constexpr (LEDGER) Pf = -(fr[0] * vt[0] + fr[1] * vt[1] + fr[2] * vt[2]);
                }
              }
              if constexpr (LEDGER)   // Omega F_t.(a x rho_c): the wall's material moves at Omega a x rho_c under -F_t
                Wc = Om * (fr[0] * (b1[1] * r0[2] - b1[2] * r0[1]) + fr[1] * (b1[2] * r0[0] - b1[0] * r0[2]) +
                           fr[2] * (b1[0] * r0[1] - b1[1] * r0[0]));
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
        for (int k = 0; k < 3; ++k) {   // back to the space frame: v = R v_b (twin text in wall_contact_body)
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
        double* row = P.rows + ((size_t)i * P.nsurf + c) * kCylRow;
        row[0] = E; row[1] = Fw[0]; row[2] = Fw[1]; row[3] = Fw[2];
        row[4] = ax[0] * m0 + ax[1] * m1 + ax[2] * m2;
      }
      if constexpr (LEDGER) {
        if (lane == 0) {
          double* prow = P.prows + ((size_t)i * P.nsurf + c) * kCylPowerRow;
          prow[0] = Pd; prow[1] = Pf; prow[2] = Wc;
        }
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

// The two instances ...
__global__ __launch_bounds__(kCylBlock) void cyl_contact_kernel(const CylParams P) { cyl_contact_body<false>(P); }
__global__ __launch_bounds__(kCylBlock) void cyl_contact_dissipative_kernel(const CylParams P) { cyl_contact_body<true>(P); }

// ... and the one while a cylinder has a tangential spring (SPEC §2.19), launched only then
__global__ __launch_bounds__(kCylBlock) void cyl_spring_kernel(const CylSpringParams P) { cyl_contact_body<true, true, CylSpringParams>(P); }

// The live sweep of an advancing pass (SPEC §2.19), behind the candidate pass: a particle that left a cylinder's reach is
// not visited by the contact kernel for that cylinder (or at all), so the bits of the cylinders out of its mask die here.
__global__ __launch_bounds__(kCylBlock) void cyl_live_sweep_kernel(int nlocal, const unsigned char* __restrict__ cmask,
                                                                    unsigned char* __restrict__ live)
{
  surface_live_sweep(nlocal, live, cmask);
}

// ---- per-cylinder totals in a fixed order (surface_pass.hpp): rows of kCylRow
__global__ __launch_bounds__(kCylBlock) void cyl_rows_partial_kernel(int nlocal, int ncyl, const unsigned char* __restrict__ cmask,
                                                                      const double* __restrict__ rows, double* __restrict__ part)
{
  surface_rows_partial<kCylRow>(nlocal, ncyl, cmask, rows, part);
}

__global__ __launch_bounds__(kCylBlock) void cyl_rows_final_kernel(int nb, const double* __restrict__ part, double* __restrict__ cyl_out)
{
  surface_rows_final<kCylRow>(nb, part, cyl_out);
}

}  // namespace shp
