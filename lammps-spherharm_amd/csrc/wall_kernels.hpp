// wall_kernels.hpp — gfx950 kernels of docs/SPEC.md §2.9: the contact of an SH particle with planar walls, fixed or
// translating at a constant velocity (§2.12).
//
// The wall contact is the pair contact of SPEC §2 with particle j replaced by a half-space: same cap, frame, nodes,
// vector area and force law, no r_j and no root search (r_in = h / mu in closed form).  Always the sharp rule.
//
// The pass (candidates, contact, live sweep, row passes) is described in surface_pass.hpp, which holds what it shares
// with the cylinder pass.  Here: the plane's geometry, the thirteen instances of the contact body, the advance.
// r_i and its gradient come from the recurrence form of sh_device.hpp (wall_sh_grad.hpp), evaluated in the particle's
// BODY frame: the cap frame is rotated into the body once per wall, the sums are rotated back once per wall.  One
// instance serves every order 0..20: the loops over (m, n) stay rolled, because unrolled they request every coefficient
// up front and the scalar registers spill into vector lanes (L = 6: 247 VGPRs and 191 spilled SGPRs against 175 / 7).
//
// Included by shstep_walls.hip only (the kernels are not templates: one definition per library).
#pragma once
#include <hip/hip_runtime.h>

#include "contact_laws.hpp"
#include "pair_params.hpp"
#include "sh_const.hpp"
#include "sh_device.hpp"
#include "surface_pass.hpp"
#include "wall_sh_grad.hpp"

namespace shp {

constexpr int kMaxWalls = 32;      // SHSTEP_MAX_WALLS: a particle's walls are one 32-bit mask
constexpr int kWallStride = 6;     // doubles per wall: n[3], c, kn, exponent
constexpr int kWallVelStride = 4;  // doubles per wall of the velocity table: u[3], n.u
constexpr int kWallBlock = kSurfBlock;
constexpr int kWallMaxBlocks = kSurfMaxBlocks;

// `surf` holds kWallStride doubles per wall, a row is (E, force on the wall)
struct WallParams : SurfaceParams<unsigned> {
  // volume-rate damping (SPEC §2.10; the DAMP instance only)
  const double* wgamma;   // [nwalls] gamma_w
  const double* twist;    // [nlocal][6]: velocity of the SH origin and angular velocity, space frame (dissipation_kernels.hpp)
  // Coulomb-capped friction (SPEC §2.11; the FRIC instance only)
  const double* wfric;    // [2][nwalls] mu_w, then gamma_t,w
  // translating walls (SPEC §2.12; the MOVE instances only)
  const double* wvel;     // kWallVelStride doubles per wall: u_w[3] in the space frame, then n_w.u_w
  // energy ledger (SPEC §2.13; the LEDGER instances only)
  double* prows;          // [nlocal][nwalls][2] dissipated power of the contact: damping, friction
};

struct WallHistParams : SurfaceHistParams<WallParams, unsigned> {};   // SPEC §2.15: xi is a space-frame vector, 3 doubles

// the kernel arguments lie where they always lay
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(WallParams) == 224 && offsetof(WallParams, wgamma) == 184, "WallParams: kernel-argument layout");
static_assert(sizeof(WallHistParams) == 264 && offsetof(WallHistParams, kt) == 224, "WallHistParams: kernel-argument layout");

__global__ __launch_bounds__(kWallBlock) void wall_candidates_kernel(const WallParams P)
{
  const int i = blockIdx.x * kWallBlock + threadIdx.x;
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
        for (int w = 0; w < P.nsurf; ++w) {
          const double* W = P.surf + kWallStride * w;
          const double h = fma(W[0], px, fma(W[1], py, fma(W[2], pz, -W[3])));
          if (!(h > 0.0)) e |= kPairErrWall;   // at or behind the plane, or not a number
          else if (h < R) m |= 1u << w;
        }
      }
    }
    P.smask[i] = m;
  }
  if (e) atomicOr(P.err, e);
  surface_queue_push(m != 0, i, lane, P.count, P.queue);
}

// The contact point of a wall contact and the tangential velocity there, body frame (SPEC §2.11 at a wall): r_perp =
// S_n x T_n / q dropped onto the plane, r_i = r_perp - (h + n.r_perp) n with the wall normal n = -c, and v_t the part of
// w + omega x r_i in the plane.  For the viscous and for the history wall alike.  Scalars in, a struct of scalars out:
// in this form, and in none that passes the body's arrays by pointer or reference, returns arrays or is a lambda of the
// body, every instance keeps the machine code it has with the text written out twice.
struct WallPoint { double r0, r1, r2, v0, v1, v2; };
__device__ __forceinline__ WallPoint wall_contact_point(const double S0, const double S1, const double S2, const double T0, const double T1,
                                                        const double T2, const double q, const double h, const double c0, const double c1,
                                                        const double c2, const double w0, const double w1, const double w2, const double o0,
                                                        const double o1, const double o2)
{
  const double qi = 1.0 / q;
  const double rp[3] = {(S1 * T2 - S2 * T1) * qi, (S2 * T0 - S0 * T2) * qi, (S0 * T1 - S1 * T0) * qi};
  const double hn = h - (c0 * rp[0] + c1 * rp[1] + c2 * rp[2]);
  WallPoint o;
  o.r0 = fma(hn, c0, rp[0]); o.r1 = fma(hn, c1, rp[1]); o.r2 = fma(hn, c2, rp[2]);
  const double vr[3] = {w0 + (o1 * o.r2 - o2 * o.r1), w1 + (o2 * o.r0 - o0 * o.r2), w2 + (o0 * o.r1 - o1 * o.r0)};
  const double vn = vr[0] * c0 + vr[1] * c1 + vr[2] * c2;
  o.v0 = vr[0] - vn * c0; o.v1 = vr[1] - vn * c1; o.v2 = vr[2] - vn * c2;
  return o;
}

// DAMP = false is the elastic contact of SPEC §2.9.  DAMP = true adds the volume-rate damping of SPEC §2.10: the
// particle's twist is rotated into the body frame once per particle (the sums are body-frame there), Vdot = S_n.w +
// T_n.omega is formed after the wave sums, and p_tot = max(0, p + gamma_w Vdot) takes the place of p in the force and
// the torque.  E_w, the per-wall rows' form and the contact count are the same in both.
// FRIC = true (with DAMP) adds the friction of SPEC §2.11, formed after the wave sums in the body frame as well: the
// contact point r_i is the point of the normal wrench's line of action (through S_n x T_n / |S_n|^2) dropped onto the
// plane, v_t the part of w + omega x r_i in the plane, F_t = -kappa v_t with kappa = gamma_t,w capped at mu_w N / |v_t|,
// N = p_tot |S_n|.  The force on the wall in the rows is minus the whole force on the particle.
// MOVE = true (with DAMP) is the translating wall of SPEC §2.12: u_w, rotated into the body frame once per wall, is taken
// off the linear part of the twist before Vdot and v_rel are formed — the wall moving by u is the particle moving by -u.
// MOVE = false reads no velocity table.
// LEDGER = true (with DAMP) is the pass while the energy ledger is on (SPEC §2.13): lane 0 also leaves the power the
// contact dissipates, P_d = (p_tot - p) Vdot and P_f = kappa |v_t|^2 of the wall-relative twist, in a row of its own
// beside the (E, F_w) row.  The elastic contact dissipates nothing: it has no such instance.
// HIST = true (with DAMP and FRIC) is the pass while a wall has a tangential spring (SPEC §2.15).  A wall with mu_w != 0
// and k_t,w != 0 takes the spring law in place of kappa: behind the wave sums xi_iw (space frame, 0 where the particle's
// live bit of the wall is dead) is rotated into the body frame, advanced by dt v_t, projected with the exact wall normal,
// and F* = -k_t xi - gamma_t v_t is capped at mu N; a sliding contact keeps the xi the capped force can hold.  Every lane
// holds the same sums, so the branch is wave-uniform; lane 0, the only writer of row i, stores xi and, once behind the
// wall loop, the particle's new live word — both only while dt > 0.  A wall in the mask that fails a guard (V <= 0,
// |S_n| = 0, N = 0) leaves its bit out of the new word; wall_spring_sweep_kernel clears the bits of walls out of reach.
// The other walls keep the law above; P_f of a history wall is -F_t.v_t.
template <bool DAMP, bool FRIC = false, bool MOVE = false, bool LEDGER = false, bool HIST = false, typename Params = WallParams>
__device__ __forceinline__ void wall_contact_body(const Params& P)
{
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nwaves = gridDim.x * (kWallBlock / 64);
  const int count = P.count[0];
  const int nq = P.nq, npsi = 2 * nq, nnodes = npsi * nq;
  int ncontact = 0;
  for (int q = blockIdx.x * (kWallBlock / 64) + wv; q < count; q += nwaves) {
    const int i = __builtin_amdgcn_readfirstlane(P.queue[q]);
    unsigned wm = (unsigned)__builtin_amdgcn_readfirstlane((int)P.smask[i]);
    const int st = __builtin_amdgcn_readfirstlane(P.shtype[i]);   // in range: the candidate pass checked it
    const double Ri = P.rmax[st];
    const double* cw = P.cw + (size_t)P.cstride * st;
    const double px = P.x[3 * i], py = P.x[3 * i + 1], pz = P.x[3 * i + 2];
    double R[9];
    quat_to_mat(P.quat[4 * i], P.quat[4 * i + 1], P.quat[4 * i + 2], P.quat[4 * i + 3], R);
    double Ft[3] = {0.0, 0.0, 0.0}, Tt[3] = {0.0, 0.0, 0.0};
    double twb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // DAMP: the twist in the body frame, v_b = R^T v
    if constexpr (DAMP || FRIC) {
      const double* tw = P.twist + 6 * (size_t)i;   // (twin text in cyl_contact_body: no helper form keeps the kernels)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        twb[k] = R[k] * tw[0] + R[3 + k] * tw[1] + R[6 + k] * tw[2];
        twb[3 + k] = R[k] * tw[3] + R[3 + k] * tw[4] + R[6 + k] * tw[5];
      }
    }
    unsigned lv = 0, nl = 0;   // HIST: the particle's live word as it was, and as this pass leaves it
    if constexpr (HIST) lv = P.live_dead ? 0u : (unsigned)__builtin_amdgcn_readfirstlane((int)P.live[i]);
    while (wm) {
      const int w = __builtin_ctz(wm);
      wm &= wm - 1;
      const double* W = P.surf + kWallStride * w;
      const double h = fma(W[0], px, fma(W[1], py, fma(W[2], pz, -W[3])));
      const double ca = h / Ri;
      // frame (e1, e2, c) about c = -n (SPEC §2.3), rotated into the body frame: v_b = R^T v
      const double c0 = -W[0], c1 = -W[1], c2 = -W[2];
      const double s = copysign(1.0, c2), a = -1.0 / (s + c2), b = c0 * c1 * a;
      const double e1[3] = {1.0 + s * c0 * c0 * a, s * b, -s * c0}, e2[3] = {b, s + c1 * c1 * a, -c1}, cc[3] = {c0, c1, c2};
      double b1[3], b2[3], bc[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b1[k] = R[k] * e1[0] + R[3 + k] * e1[1] + R[6 + k] * e1[2];
        b2[k] = R[k] * e2[0] + R[3 + k] * e2[1] + R[6 + k] * e2[2];
        bc[k] = R[k] * cc[0] + R[3 + k] * cc[1] + R[6 + k] * cc[2];
      }
      double wl[3] = {twb[0], twb[1], twb[2]};   // the SH origin's velocity relative to the wall, body frame
      if constexpr (MOVE) {
        const double* U = P.wvel + kWallVelStride * w;
#pragma unroll
        for (int k = 0; k < 3; ++k) wl[k] -= R[k] * U[0] + R[3 + k] * U[1] + R[6 + k] * U[2];
      }
      const double hm = 0.5 * (1.0 + ca), hw = 0.5 * (1.0 - ca);
      const double wsc = hw * (3.14159265358979323846264338327950288 / nq);
      double V = 0.0, S0 = 0.0, S1 = 0.0, S2 = 0.0, T0 = 0.0, T1 = 0.0, T2 = 0.0;
#pragma unroll 1
      for (int t = lane; t < nnodes; t += 64) {
        const int k = t / npsi, l = t - k * npsi;
        const SurfaceNode nd = surface_node(hw, hm, P.glt[k], P.cpsi[l], P.spsi[l], b1[0], b1[1], b1[2], b2[0], b2[1], b2[2], bc[0], bc[1], bc[2]);
        const double mu = nd.mu, u0 = nd.u0, u1 = nd.u1, u2 = nd.u2;
        double r, g0, g1, g2;
        wall_sh_grad(P.rc, cw, P.lmax, u0, u1, u2, r, g0, g1, g2);
        if (r * mu > h) {   // the surface point is inside the wall (u.c = mu)
          const double om = wsc * P.glw[k];
          const SurfaceSums A = surface_add_area(S0, S1, S2, T0, T1, T2, om, r, u0, u1, u2, g0, g1, g2);
          S0 = A.S0; S1 = A.S1; S2 = A.S2; T0 = A.T0; T1 = A.T1; T2 = A.T2;
          const double rin = h / mu;
          V = surface_add_volume(V, om, r, rin);
        }
      }
      V = wave_sum(V);
      S0 = wave_sum(S0); S1 = wave_sum(S1); S2 = wave_sum(S2);
      T0 = wave_sum(T0); T1 = wave_sum(T1); T2 = wave_sum(T2);
      double E = 0.0, Fw[3] = {0.0, 0.0, 0.0};
      double Pd = 0.0, Pf = 0.0;   // LEDGER only
      if (V > 0.0) {
        const double kn = W[4], ex = W[5];
        const double pn = pair_pressure(kn, ex, V);
        E = pn * V / ex;   // kn V^m
        double pt = pn;
        if constexpr (DAMP) {
          const double vd = fma(S0, wl[0], fma(S1, wl[1], fma(S2, wl[2], fma(T0, twb[3], fma(T1, twb[4], T2 * twb[5])))));
          pt = fmax(0.0, fma(P.wgamma[w], vd, pn));   // the wall never pulls
          if constexpr (LEDGER) Pd = (pt - pn) * vd;
        }
        if constexpr (FRIC) {
          // minus the particle's wrench in the body frame: pt S - F_t, pt T - r_i x F_t
          double Gf[3] = {pt * S0, pt * S1, pt * S2}, Gt[3] = {pt * T0, pt * T1, pt * T2};
          const double mu = P.wfric[w], gt = P.wfric[P.nsurf + w];
          const double q = fma(S0, S0, fma(S1, S1, S2 * S2));
          const double N = pt * __builtin_sqrt(q);
          double kt = 0.0;
          bool hist = false;   // this wall takes the spring law
          if constexpr (HIST) {
            kt = P.kt[w];
            hist = mu != 0.0 && kt != 0.0;
          }
          // A wall without a spring runs the block it always ran, whole and under the condition it always had (written out
          // for either case), so that it gives the same bits from every instance; a history wall has a block of its own.
          if (HIST ? (!hist && mu != 0.0 && gt != 0.0 && q > 0.0 && N > 0.0) : (mu != 0.0 && gt != 0.0 && q > 0.0 && N > 0.0)) {
            const WallPoint cp = wall_contact_point(S0, S1, S2, T0, T1, T2, q, h, bc[0], bc[1], bc[2], wl[0], wl[1], wl[2], twb[3], twb[4], twb[5]);
            const double ri[3] = {cp.r0, cp.r1, cp.r2}, vt[3] = {cp.v0, cp.v1, cp.v2};
            const double vtn = __builtin_sqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
            const double cap = mu * N;
            const double kappa = capped_coefficient(gt, vtn, cap);
            const double ft[3] = {-kappa * vt[0], -kappa * vt[1], -kappa * vt[2]};
            Gf[0] -= ft[0]; Gf[1] -= ft[1]; Gf[2] -= ft[2];
            Gt[0] -= ri[1] * ft[2] - ri[2] * ft[1];
            Gt[1] -= ri[2] * ft[0] - ri[0] * ft[2];
            Gt[2] -= ri[0] * ft[1] - ri[1] * ft[0];
            if constexpr (LEDGER) Pf = kappa * (vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2]);
          }
          if constexpr (HIST) {
            if (hist && q > 0.0 && N > 0.0) {
              const WallPoint cp = wall_contact_point(S0, S1, S2, T0, T1, T2, q, h, bc[0], bc[1], bc[2], wl[0], wl[1], wl[2], twb[3], twb[4], twb[5]);
              const double ri[3] = {cp.r0, cp.r1, cp.r2}, vt[3] = {cp.v0, cp.v1, cp.v2};
              const double cap = mu * N;
              double* X = P.xi + ((size_t)i * P.nsurf + w) * 3;
              double xs[3] = {0.0, 0.0, 0.0}, xb[3], ft[3];
              if ((lv >> w) & 1u) { xs[0] = X[0]; xs[1] = X[1]; xs[2] = X[2]; }
#pragma unroll
              for (int k = 0; k < 3; ++k) xb[k] = fma(P.dt, vt[k], R[k] * xs[0] + R[3 + k] * xs[1] + R[6 + k] * xs[2]);
              const double xn = xb[0] * bc[0] + xb[1] * bc[1] + xb[2] * bc[2];
#pragma unroll
              for (int k = 0; k < 3; ++k) {
                xb[k] -= xn * bc[k];
                ft[k] = -kt * xb[k] - gt * vt[k];   // the trial force F*
              }
              const double fn = __builtin_sqrt(ft[0] * ft[0] + ft[1] * ft[1] + ft[2] * ft[2]);
              if (!(fn <= cap)) {   // slides: the capped force, and the xi it can hold
                const double sc = cap / fn;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                  ft[k] *= sc;
                  xb[k] = -(ft[k] + gt * vt[k]) / kt;
                }
              }
              nl |= 1u << w;
              if (P.dt > 0.0 && lane == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) X[k] = R[3 * k] * xb[0] + R[3 * k + 1] * xb[1] + R[3 * k + 2] * xb[2];
              }
              Gf[0] -= ft[0]; Gf[1] -= ft[1]; Gf[2] -= ft[2];
              Gt[0] -= ri[1] * ft[2] - ri[2] * ft[1];
              Gt[1] -= ri[2] * ft[0] - ri[0] * ft[2];
              Gt[2] -= ri[0] * ft[1] - ri[1] * ft[0];
              if constexpr (LEDGER) Pf = -(ft[0] * vt[0] + ft[1] * vt[1] + ft[2] * vt[2]);
            }
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) {   // back to the space frame: v = R v_b (twin text in cyl_contact_body)
            Fw[k] = R[3 * k] * Gf[0] + R[3 * k + 1] * Gf[1] + R[3 * k + 2] * Gf[2];
            Ft[k] -= Fw[k];
            Tt[k] -= R[3 * k] * Gt[0] + R[3 * k + 1] * Gt[1] + R[3 * k + 2] * Gt[2];
          }
        } else {
#pragma unroll
          for (int k = 0; k < 3; ++k) {   // back to the space frame: v = R v_b (twin text in cyl_contact_body)
            Fw[k] = pt * (R[3 * k] * S0 + R[3 * k + 1] * S1 + R[3 * k + 2] * S2);
            Ft[k] -= Fw[k];
            Tt[k] -= pt * (R[3 * k] * T0 + R[3 * k + 1] * T1 + R[3 * k + 2] * T2);
          }
        }
        ++ncontact;
      }
      if (P.rows && lane == 0) {
        double* row = P.rows + ((size_t)i * P.nsurf + w) * 4;
        row[0] = E; row[1] = Fw[0]; row[2] = Fw[1]; row[3] = Fw[2];
      }
      if constexpr (LEDGER) {
        if (lane == 0) {
          double* prow = P.prows + ((size_t)i * P.nsurf + w) * 2;
          prow[0] = Pd; prow[1] = Pf;
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
        if (P.dt > 0.0) P.live[i] = nl;
      }
    }
  }
  if (lane == 0 && ncontact) atomicAdd(P.count + 1, ncontact);
}

// The three instances, under names of their own (the elastic one keeps the name every tool knows it by).
__global__ __launch_bounds__(kWallBlock) void wall_contact_kernel(const WallParams P) { wall_contact_body<false>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_contact_damped_kernel(const WallParams P) { wall_contact_body<true>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_contact_friction_kernel(const WallParams P) { wall_contact_body<true, true>(P); }
// ... and the two of a translating wall (SPEC §2.12), launched only while a u_w != 0 and a wall coefficient is set
__global__ __launch_bounds__(kWallBlock) void wall_moving_damped_kernel(const WallParams P) { wall_contact_body<true, false, true>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_moving_friction_kernel(const WallParams P) { wall_contact_body<true, true, true>(P); }
// ... and the four with a wall coefficient while the energy ledger is on (SPEC §2.13), launched only then
__global__ __launch_bounds__(kWallBlock) void wall_ledger_damped_kernel(const WallParams P) { wall_contact_body<true, false, false, true>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_ledger_friction_kernel(const WallParams P) { wall_contact_body<true, true, false, true>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_ledger_moving_damped_kernel(const WallParams P) { wall_contact_body<true, false, true, true>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_ledger_moving_friction_kernel(const WallParams P) { wall_contact_body<true, true, true, true>(P); }
// ... and the four while a wall has a tangential spring (SPEC §2.15), at rest or moving, plain or with the ledger, launched only then
__global__ __launch_bounds__(kWallBlock) void wall_spring_kernel(const WallHistParams P) { wall_contact_body<true, true, false, false, true, WallHistParams>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_spring_moving_kernel(const WallHistParams P) { wall_contact_body<true, true, true, false, true, WallHistParams>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_spring_ledger_kernel(const WallHistParams P) { wall_contact_body<true, true, false, true, true, WallHistParams>(P); }
__global__ __launch_bounds__(kWallBlock) void wall_spring_moving_ledger_kernel(const WallHistParams P) { wall_contact_body<true, true, true, true, true, WallHistParams>(P); }

// The live sweep of an advancing pass (SPEC §2.15), behind the candidate pass: a particle that left a wall's reach is not
// visited by the contact kernel for that wall (or at all), so the bits of the walls out of its mask die here.
__global__ __launch_bounds__(kWallBlock) void wall_spring_sweep_kernel(int nlocal, const unsigned* __restrict__ wmask, unsigned* __restrict__ live)
{
  surface_live_sweep(nlocal, live, wmask);
}

// One advance of the planes by dt (SPEC §2.12): c_w += dt (n_w.u_w), one thread per wall, in place in the wall table.
// The product and the sum are rounded separately: the plane position is DEFINED as this accumulation.
__global__ __launch_bounds__(64) void wall_advance_kernel(int nwalls, double* __restrict__ walls, const double* __restrict__ wvel, double dt)
{
  const int w = threadIdx.x;
  if (w < nwalls) walls[kWallStride * w + 3] = __dadd_rn(walls[kWallStride * w + 3], __dmul_rn(dt, wvel[kWallVelStride * w + 3]));
}

// ---- per-wall totals in a fixed order (surface_pass.hpp): rows of 4.  shstep_ledger.hip's fold relies on the partition
// of wall_rows_partial_kernel: block (b, w) sums the rows of particles [256 b, 256 b + 256) for wall w.
__global__ __launch_bounds__(kWallBlock) void wall_rows_partial_kernel(int nlocal, int nwalls, const unsigned* __restrict__ wmask,
                                                                        const double* __restrict__ rows, double* __restrict__ part)
{
  surface_rows_partial<4>(nlocal, nwalls, wmask, rows, part);
}

__global__ __launch_bounds__(kWallBlock) void wall_rows_final_kernel(int nb, const double* __restrict__ part, double* __restrict__ wall_out)
{
  surface_rows_final<4>(nb, part, wall_out);
}

}  // namespace shp
