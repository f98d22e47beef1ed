// surface_pass.hpp — what the planar wall pass (wall_kernels.hpp) and the cylinder pass (cylinder_kernels.hpp) share on
// the device.  A pass is two launches, nothing read back, nothing allocated:
//   candidates  one lane per owned particle: its distance to every surface, a mask word of the surfaces within reach
//               (32 walls in an unsigned, 8 cylinders in an unsigned char), the error bit for a centre at or behind a
//               surface, and a device queue of the particles that reach one (ballot + one atomic per wave).
//   contact     one wave per queued PARTICLE, a fixed grid striding over the device-side count.  The wave walks the
//               particle's surfaces in index order, spreads the 2 n_q^2 nodes of each cap over its lanes, reduces V, S_n,
//               T_n by an xor butterfly (every lane ends with the same bits) and adds the particle's total to f[i],
//               torque[i] with ONE plain read-add-write: no atomics, a result independent of the queue order.
// While a surface has a tangential spring the contact kernel is a HIST instance, which also keeps xi and the particles'
// live words, and an advancing pass puts the live sweep between the two.  Per-surface totals, when asked for: lane 0
// leaves one row per (particle, surface in its mask) and two ordered passes sum them, bit for bit reproducible.
// The kernels are non-template one-liners in the two family headers.  A helper is here only in a form with which every
// kernel keeps its machine code (shpair/codeobj.kernel_hashes); the twist into the body frame and the rotation of the
// wrench back have none and are text in the contact bodies, marked there.  The on-axis frame rule of
// the two axial families has one, scalars in and a struct of scalars out.
//
// Included by wall_kernels.hpp, cylinder_kernels.hpp and cone_kernels.hpp (SPEC §2.22: the cone pass is the cylinder
// pass with another geometry and two instances) only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace shp {

constexpr int kSurfBlock = 256;        // 4 waves: every kernel of a surface pass
constexpr int kSurfMaxBlocks = 2048;   // contact kernel: 8 workgroups per CU, striding over the queue

// the kernel arguments both families take; Word is the mask word
template <typename Word>
struct SurfaceParams {
  int nlocal, nsurf;
  const double* surf;    // the family's table: kWallStride / kCylStride doubles per surface
  const double *x, *quat;
  const int *shtype, *mask;
  int groupbit;
  double *f, *torque;
  // shape and quadrature tables of the context (sh_device.hpp recurrence form)
  const double *rc, *cw, *rmax;
  int cstride, lmax, nshapes, nq;
  const double *glt, *glw, *cpsi, *spsi;
  // work
  Word* smask;           // [nlocal] surfaces within reach of particle i
  int* queue;            // [nlocal] particles with a non-empty mask
  int* count;            // [0] queue length, [1] particle/surface contacts with V > 0
  int* err;              // the context's device error word (kPairErr*)
  double* rows;          // nullable: [nlocal][nsurf][row width]
};

// ... and what a HIST instance takes on top of its family's struct: a struct of its own, so that the kernel arguments of
// the other instances, and with them their register allocation, stay what they were
template <typename Base, typename Word>
struct SurfaceHistParams : Base {
  const double* kt;      // [nsurf] k_t
  double* xi;            // [nlocal][nsurf][3 or 2]; never zeroed: read as 0 where the bit is dead
  Word* live;            // [nlocal] one bit per surface whose xi is live
  double dt;             // > 0: the pass advances and stores xi and the live words; 0: a look, which writes neither
  int live_dead;         // a look at another nlocal than the state's: every live word reads as 0
};

// The queue of the candidate kernel: the lanes with `reaches` take consecutive slots behind one atomic per wave.
__device__ __forceinline__ void surface_queue_push(const bool reaches, const int i, const int lane, int* count, int* queue)
{
  const unsigned long long b = __ballot(reaches);
  if (b) {
    int base = 0;
    if (lane == 0) base = atomicAdd(count, (int)__popcll(b));
    base = __shfl(base, 0, 64);
    if (reaches) queue[base + (int)__popcll(b & ((1ULL << lane) - 1ULL))] = i;
  }
}

// node (k, l) of a cap about the frame (b1, b2, bc): mu = u.bc, cp = u.b1, sp = u.b2.  Scalars in, a struct of scalars out.
struct SurfaceNode { double mu, cp, sp, u0, u1, u2; };
__device__ __forceinline__ SurfaceNode surface_node(const double hw, const double hm, const double t, const double cpsi, const double spsi,
                                                    const double b10, const double b11, const double b12, const double b20, const double b21,
                                                    const double b22, const double bc0, const double bc1, const double bc2)
{
  SurfaceNode n;
  n.mu = fma(hw, t, hm);
  const double sg = __builtin_sqrt(fmax(0.0, 1.0 - n.mu * n.mu));
  n.cp = sg * cpsi; n.sp = sg * spsi;
  n.u0 = fma(n.cp, b10, fma(n.sp, b20, n.mu * bc0));
  n.u1 = fma(n.cp, b11, fma(n.sp, b21, n.mu * bc1));
  n.u2 = fma(n.cp, b12, fma(n.sp, b22, n.mu * bc2));
  return n;
}

// One node inside the surface, weight om, added to the lane's sums: A_i = r^2 u - r t with t = g - (u.g) u, and
// (r u) x A_i = -r^2 (u x g); then the volume down to r_in, which the family forms between the two calls.
struct SurfaceSums { double S0, S1, S2, T0, T1, T2; };
__device__ __forceinline__ SurfaceSums surface_add_area(const double S0, const double S1, const double S2, const double T0, const double T1,
                                                        const double T2, const double om, const double r, const double u0, const double u1,
                                                        const double u2, const double g0, const double g1, const double g2)
{
  SurfaceSums a;
  const double ug = fma(u0, g0, fma(u1, g1, u2 * g2));
  const double ku = om * r * (r + ug), kg = -om * r;
  a.S0 = fma(ku, u0, fma(kg, g0, S0));
  a.S1 = fma(ku, u1, fma(kg, g1, S1));
  a.S2 = fma(ku, u2, fma(kg, g2, S2));
  const double kt = kg * r;
  a.T0 = fma(kt, fma(u1, g2, -(u2 * g1)), T0);
  a.T1 = fma(kt, fma(u2, g0, -(u0 * g2)), T1);
  a.T2 = fma(kt, fma(u0, g1, -(u1 * g0)), T2);
  return a;
}
__device__ __forceinline__ double surface_add_volume(const double V, const double om, const double r, const double rin)
{
  return fma(om * (1.0 / 3.0), fma(r * r, r, -(rin * rin * rin)), V);
}

// The two axial families (cylinders, cones): the unit vector c^ = rho / d from the axis to a centre; on the axis (d = 0 as
// computed) the e1 of the frame rule of SPEC §2.3 about the axis a^.  The contact bodies and the roll row form it alike.
// Scalars in, a struct of scalars out.
struct AxialUnit { double c0, c1, c2; };
__device__ __forceinline__ AxialUnit axis_frame_e1(const double a0, const double a1, const double a2)
{
  const double s = copysign(1.0, a2), a = -1.0 / (s + a2);
  AxialUnit e;
  e.c0 = 1.0 + s * a0 * a0 * a; e.c1 = s * (a0 * a1 * a); e.c2 = -s * a0;
  return e;
}
__device__ __forceinline__ AxialUnit axial_radial_unit(const double d, const double r0, const double r1, const double r2, const double a0,
                                                       const double a1, const double a2)
{
  if (d > 0.0) {
    const double di = 1.0 / d;
    AxialUnit e;
    e.c0 = r0 * di; e.c1 = r1 * di; e.c2 = r2 * di;
    return e;
  }
  return axis_frame_e1(a0, a1, a2);
}

// the live sweep: the contact kernel does not visit a particle for a surface it no longer reaches, so those bits die here
template <typename Word>
__device__ __forceinline__ void surface_live_sweep(const int nlocal, Word* __restrict__ live, const Word* __restrict__ smask)
{
  const int i = blockIdx.x * kSurfBlock + threadIdx.x;
  if (i < nlocal) {
    Word* l = live + i;   // (formed ahead of the mask's: the order the kernels' address arithmetic always had)
    *l &= smask[i];
  }
}

// ---- per-surface totals in a fixed order: block (b, s) sums the rows of particles [256 b, 256 b + 256) for surface s ...
template <int W>
__device__ __forceinline__ void surface_block_sum(double v[W], double (*sh)[kSurfBlock])
{
  const int t = threadIdx.x;
  for (int k = 0; k < W; ++k) sh[k][t] = v[k];
  __syncthreads();
  for (int s = kSurfBlock / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < W; ++k) sh[k][t] += sh[k][t + s];
    __syncthreads();
  }
}

template <int W, typename Word>
__device__ __forceinline__ void surface_rows_partial(const int nlocal, const int nsurf, const Word* __restrict__ smask,
                                                     const double* __restrict__ rows, double* __restrict__ part)
{
  __shared__ double sh[W][kSurfBlock];
  const int i = blockIdx.x * kSurfBlock + threadIdx.x, s = blockIdx.y;
  double v[W] = {};
  if (i < nlocal && ((smask[i] >> s) & 1u)) {
    const double* row = rows + ((size_t)i * nsurf + s) * W;
    for (int k = 0; k < W; ++k) v[k] = row[k];
  }
  surface_block_sum<W>(v, sh);
  if (threadIdx.x < W) part[((size_t)s * gridDim.x + blockIdx.x) * W + threadIdx.x] = sh[threadIdx.x][0];
}

// ... and one block per surface adds the nb partial sums to out[W s ..]
template <int W>
__device__ __forceinline__ void surface_rows_final(const int nb, const double* __restrict__ part, double* __restrict__ out)
{
  __shared__ double sh[W][kSurfBlock];
  const int s = blockIdx.x;
  double v[W] = {};
  for (int b = threadIdx.x; b < nb; b += kSurfBlock)
    for (int k = 0; k < W; ++k) v[k] += part[((size_t)s * nb + b) * W + k];
  surface_block_sum<W>(v, sh);
  if (threadIdx.x < W) out[W * s + threadIdx.x] += sh[threadIdx.x][0];
}

}  // namespace shp
