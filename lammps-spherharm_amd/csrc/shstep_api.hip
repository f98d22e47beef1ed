// shstep_api.hip — the C ABI of include/shstep.h (docs/SPEC.md Part II) on top of step_kernels.hpp: the integrator,
// ghosts and the neighbour list.  Host side: per-shape rigid-body table, box / bin geometry, the blocking read-backs
// (ghost count, pair count, rebuild flag).  The state is in shstep_state.hpp, the run loop in shstep_run.cpp, the planar
// walls in shstep_walls.hip, contact dissipation in shstep_dissipation.hip.  No CPU fallback: every entry point launches
// gfx950 kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/shstep.h"
#include "sh_tables.hpp"
#include "shpair_ctx.hpp"
#include "shstep_state.hpp"
#include "step_kernels.hpp"

using namespace shp;

// called by shpair_destroy (shpair_context.cpp): the state's buffers go with it
void shstep_release_state(shpair_ctx* c)
{
  if (!c || !c->step) return;
  delete c->step->box;
  delete c->step;
  c->step = nullptr;
}

// a host-supplied list replaced the device-built one (shpair_api.hip)
void shstep_invalidate_list(shpair_ctx* c)
{
  if (c && c->step) c->step->l_nlocal = -1;
}

int shp::step_state(shpair_ctx* c, shstep_state** out)
{
  if (!c->step) {
    shstep_state* s = new (std::nothrow) shstep_state();
    if (s) s->box = new (std::nothrow) BoxParams();
    if (!s || !s->box) {
      delete s;
      CTX_FAIL(c, SHPAIR_ENOMEM, "out of host memory");
    }
    c->step = s;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, s->d_flags.ensure(4));
    HIPCHK(c, hipMemset(s->d_flags.p, 0, 4 * sizeof(int)));
    HIPCHK(c, s->h_flags.resize(4));
  }
  *out = c->step;
  return SHPAIR_OK;
}

// Per-shape rows: m, 1/m, c[3], Iinv[6], rmax.  Rebuilt when shapes or densities changed.
int shp::step_refresh_mass(shpair_ctx* c, shstep_state* s)
{
  if (c->nshapes <= 0) CTX_FAIL(c, SHPAIR_ESTATE, "shapes are not set");
  if (!c->mass_dirty && s->d_mass.p) return SHPAIR_OK;
  s->h_mass.assign((size_t)kMassStride * c->nshapes, 0.0);
  for (int k = 0; k < c->nshapes; ++k) {
    const Shape& sh = c->shapes[k];
    if (sh.lmax < 0) CTX_FAIL(c, SHPAIR_ESTATE, "shape %d is not set", k);
    double mp[10], inv[6];
    mass_props(sh.lmax, sh.anm.data(), mp);
    if (!(mp[0] > 0.0) || !inertia_inverse(mp, sh.density, inv))
      CTX_FAIL(c, SHPAIR_EINVAL, "shape %d: volume %g / inertia tensor is not positive (is r > 0 everywhere?)", k, mp[0]);
    double* r = &s->h_mass[(size_t)kMassStride * k];
    r[0] = sh.density * mp[0];
    r[1] = 1.0 / r[0];
    r[2] = mp[1]; r[3] = mp[2]; r[4] = mp[3];
    for (int q = 0; q < 6; ++q) r[5 + q] = inv[q];
    r[11] = sh.rmax;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());  // an enqueued kernel may still read the old table
  HIPCHK(c, s->d_mass.ensure(s->h_mass.size()));
  HIPCHK(c, hipMemcpy(s->d_mass.p, s->h_mass.data(), s->h_mass.size() * sizeof(double), hipMemcpyHostToDevice));
  c->mass_dirty = false;
  return SHPAIR_OK;
}

// cmax, bin grid. Needs shapes (bounding radii).
int shp::step_refresh_box(shpair_ctx* c, shstep_state* s)
{
  if (!s->have_box) CTX_FAIL(c, SHPAIR_ESTATE, "shstep_set_box() must come first");
  double rm = 0.0;
  for (int k = 0; k < c->nshapes; ++k) {
    if (c->shapes[k].lmax < 0) CTX_FAIL(c, SHPAIR_ESTATE, "shape %d is not set", k);
    rm = std::fmax(rm, c->shapes[k].rmax);
  }
  if (!(rm > 0.0)) CTX_FAIL(c, SHPAIR_ESTATE, "shapes are not set");
  BoxParams& b = *s->box;
  b.cmax = 2.0 * rm + s->skin;
  double ncell = 1.0;
  for (int d = 0; d < 3; ++d) {
    if (b.periodic[d] && b.len[d] < 2.0 * b.cmax)
      CTX_FAIL(c, SHPAIR_EINVAL, "periodic box edge %d (%g) is shorter than twice the ghost cutoff (%g)", d, b.len[d], b.cmax);
    b.glo[d] = b.periodic[d] ? b.lo[d] - b.cmax : b.lo[d];
    const double ext = b.periodic[d] ? b.len[d] + 2.0 * b.cmax : b.len[d];
    double n = std::floor(ext / b.cmax);
    if (!(n >= 1.0)) n = 1.0;
    if (n > 1024.0) n = 1024.0;  // <= 2^30 cells in all; further capped below
    b.nc[d] = (int)n;
    ncell *= n;
  }
  while (ncell > 67108864.0) {  // 2^26 cells: coarsen the longest direction
    int d = 0;
    for (int k = 1; k < 3; ++k)
      if (b.nc[k] > b.nc[d]) d = k;
    ncell /= b.nc[d];
    b.nc[d] = (b.nc[d] + 1) / 2;
    ncell *= b.nc[d];
  }
  for (int d = 0; d < 3; ++d) {
    const double ext = b.periodic[d] ? b.len[d] + 2.0 * b.cmax : b.len[d];
    b.binv[d] = b.nc[d] / ext;
  }
  return SHPAIR_OK;
}

static int exclusive_scan(shpair_ctx* c, shstep_state* s, const int* in, int* out, int n, hipStream_t st)
{
  const unsigned nb = nblk(n, kScanBlock);
  HIPCHK(c, s->d_sums.ensure(nb + 1));
  hipLaunchKernelGGL(scan_local_kernel, dim3(nb), dim3(kScanBlock), 0, st, in, n, out, s->d_sums.p);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kScanBlock), 0, st, s->d_sums.p, (int)nb);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kScanBlock), 0, st, out, n, (const int*)s->d_sums.p, (int)nb);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shp::step_decode_flags(shpair_ctx* c, shstep_state* s, hipStream_t st)
{
  const int bits = s->h_flags[0];
  if (!bits) return SHPAIR_OK;
  HIPCHK(c, hipMemsetAsync(s->d_flags.p, 0, sizeof(int), st));
  if (bits & kErrShape)
    CTX_FAIL(c, SHPAIR_EINVAL, "a shape index (shtype) outside [0,%d) reached a kernel; those particles were skipped", c->nshapes);
  return SHPAIR_OK;
}

// reads and clears the device error bits; blocks on the stream
static int check_device_flags(shpair_ctx* c, shstep_state* s, hipStream_t st)
{
  HIPCHK(c, download((int*)s->h_flags, s->d_flags, 1, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return step_decode_flags(c, s, st);
}

int shp::step_enqueue_displacement(shpair_ctx* c, shstep_state* s, int nlocal, const double* x, bool read_back, hipStream_t st)
{
  const double trig = 0.5 * s->skin;
  HIPCHK(c, hipMemsetAsync(s->d_flags.p + 1, 0, sizeof(int), st));
  hipLaunchKernelGGL(check_distance_kernel, dim3(nblk(nlocal, kStepBlock)), dim3(kStepBlock), 0, st, nlocal, x,
                     (const double*)s->d_xhold.p, trig * trig, s->d_flags.p + 1);
  HIPCHK(c, hipGetLastError());
  if (read_back) HIPCHK(c, download((int*)s->h_flags, s->d_flags, 2, st));
  return SHPAIR_OK;
}

// Internal (shpair_ctx.hpp): the three-pass exclusive scan, for the reverse index of shpair_api.hip and the plan
// builder of shhalo_api.hip.  out[n] = total.
int shstep_exclusive_scan(shpair_ctx* c, const int* in, int* out, int n, void* stream)
{
  STEP_PROLOGUE(c);
  return exclusive_scan(c, s, in, out, n, (hipStream_t)stream);
}

// Internal (shpair_ctx.hpp), for the multi-rank loop of shhalo_run.cpp: the error bits the step kernels raised (a shape
// index outside the table that reached the twist kernel), read once at the end of a call.  Blocks on the stream.
int shstep_check_flags(shpair_ctx* c, void* stream)
{
  STEP_PROLOGUE(c);
  return check_device_flags(c, s, (hipStream_t)stream);
}

// Internal (shpair_ctx.hpp), for the multi-rank loop of shhalo_api.hip: enqueues the displacement test of
// Neighbor::check_distance and hands back the device flag (1 = an owned row moved more than skin/2) instead of reading
// it, so that the caller can all-reduce it first.  *forced = 1 (only the flag is cleared): there is no list for these rows.
int shstep_enqueue_check(shpair_ctx* c, int nlocal, const double* x, int** flag_dev, int* forced, void* stream)
{
  STEP_PROLOGUE(c);
  if (!flag_dev || !forced) CTX_FAIL(c, SHPAIR_EINVAL, "null output pointer");
  *flag_dev = s->d_flags.p + 1;
  *forced = (s->l_nlocal < 0 || nlocal != s->l_nlocal) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (*forced || nlocal == 0) {
    HIPCHK(c, hipMemsetAsync(s->d_flags.p + 1, 0, sizeof(int), st));
    return SHPAIR_OK;
  }
  if (!x) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  return step_enqueue_displacement(c, s, nlocal, x, false, st);
}

// ---- the steps of shstep_neighbor_build_device --------------------------------------------------------------------

// a rank that lost all its atoms by migration: an empty list, and nothing of the previous list's partition survives
// (shhalo_run_device cuts its slot ranges at n_interior)
static int install_empty_list(shpair_ctx* c, shstep_state* s, int nall, hipStream_t st)
{
  c->npairs = 0;
  c->n_interior = 0;
  s->partitioned = false;
  c->max_atom_index = nall - 1;
  HIPCHK(c, c->d_pair_i.ensure(1));
  HIPCHK(c, c->d_pair_j.ensure(1));
  HIPCHK(c, s->d_offs.ensure(1));
  HIPCHK(c, hipMemsetAsync(s->d_offs.p, 0, sizeof(int), st));
  c->have_neighbors = true;
  s->l_nlocal = 0;
  return SHPAIR_OK;
}

// counting sort of all atoms into the bin grid: d_cell (bin of an atom), d_cellstart, d_atoms (atoms by bin)
static int bin_atoms(shpair_ctx* c, shstep_state* s, int nlocal, int nall, const double* x, hipStream_t st)
{
  const BoxParams& b = *s->box;
  const size_t ncell = (size_t)b.nc[0] * b.nc[1] * b.nc[2];
  HIPCHK(c, s->d_cell.ensure((size_t)nall));
  HIPCHK(c, s->d_atoms.ensure((size_t)nall));
  HIPCHK(c, s->d_cellcount.ensure(ncell));
  HIPCHK(c, s->d_cellstart.ensure(ncell + 1));
  HIPCHK(c, s->d_nn.ensure((size_t)nlocal));
  HIPCHK(c, s->d_offs.ensure((size_t)nlocal + 1));
  HIPCHK(c, s->d_xhold.ensure(3 * (size_t)nlocal));
  HIPCHK(c, hipMemsetAsync(s->d_cellcount.p, 0, ncell * sizeof(int), st));
  hipLaunchKernelGGL(bin_count_kernel, dim3(nblk(nall, kStepBlock)), dim3(kStepBlock), 0, st, nall, b, x, s->d_cell.p,
                     s->d_cellcount.p);
  RC(exclusive_scan(c, s, s->d_cellcount.p, s->d_cellstart.p, (int)ncell, st));
  HIPCHK(c, hipMemsetAsync(s->d_cellcount.p, 0, ncell * sizeof(int), st));  // reused as the fill cursor
  hipLaunchKernelGGL(bin_fill_kernel, dim3(nblk(nall, kStepBlock)), dim3(kStepBlock), 0, st, nall, (const int*)s->d_cell.p,
                     (const int*)s->d_cellstart.p, s->d_cellcount.p, s->d_atoms.p);
  return SHPAIR_OK;
}

// one pass of half_list_kernel over the owned rows: FILL = false counts a row's entries into d_nn, true writes them
template <bool FILL>
static void launch_half_list(shpair_ctx* c, shstep_state* s, int nlocal, int nall, const double* x, const int* shtype, const int* tag,
                             hipStream_t st)
{
  hipLaunchKernelGGL(half_list_kernel<FILL>, dim3(nblk(nlocal, kStepBlock)), dim3(kStepBlock), 0, st, nlocal, nall, *s->box, s->skin,
                     x, shtype, tag, (const int*)s->d_gowner.p, (const double*)s->d_mass.p, c->nshapes, (const int*)s->d_cell.p,
                     (const int*)s->d_cellstart.p, (const int*)s->d_atoms.p, FILL ? (int*)nullptr : s->d_nn.p,
                     FILL ? (const int*)s->d_offs.p : (const int*)nullptr, FILL ? c->d_pair_i.p : (int*)nullptr,
                     FILL ? c->d_pair_j.p : (int*)nullptr, s->d_flags.p);
}

// count, scan, fill: the half list in the context's slots, the positions it was built at in d_xhold
static int build_half_list(shpair_ctx* c, shstep_state* s, int nlocal, int nall, const double* x, const int* shtype, const int* tag,
                           int* npairs, hipStream_t st)
{
  launch_half_list<false>(c, s, nlocal, nall, x, shtype, tag, st);
  RC(exclusive_scan(c, s, s->d_nn.p, s->d_offs.p, nlocal, st));
  HIPCHK(c, hipMemcpyAsync(s->h_flags + 2, s->d_offs.p + nlocal, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int np = s->h_flags[2];
  if (np < 0) CTX_FAIL(c, SHPAIR_EINVAL, "half list too long (pair count overflowed)");
  HIPCHK(c, c->d_pair_i.ensure(np ? (size_t)np : 1));
  HIPCHK(c, c->d_pair_j.ensure(np ? (size_t)np : 1));
  HIPCHK(c, shp_size_pair_buffers(c, (size_t)np));   // per-slot buffers of the pair kernels (shpair_api.hip)
  if (np > 0) launch_half_list<true>(c, s, nlocal, nall, x, shtype, tag, st);
  hipLaunchKernelGGL(copy_x_kernel, dim3(nblk(3LL * nlocal, kStepBlock)), dim3(kStepBlock), 0, st, nlocal, x, s->d_xhold.p);
  HIPCHK(c, hipGetLastError());
  RC(check_device_flags(c, s, st));
  *npairs = np;
  return SHPAIR_OK;
}

// "halo_overlap": interior slots first (stable), ghost-j slots behind them: the context's list becomes the partitioned
// one, the row-major j list stays in d_part_j for shstep_copy_neighbors
static int partition_list(shpair_ctx* c, shstep_state* s, int nlocal, int np, hipStream_t st)
{
  HIPCHK(c, s->d_part_i.ensure((size_t)np));
  HIPCHK(c, s->d_part_j.ensure((size_t)np));
  HIPCHK(c, s->d_part_scan.ensure(2 * (size_t)np + 2));
  int* flag = s->d_part_scan.p + np + 1;
  hipLaunchKernelGGL(part_flag_kernel, dim3(nblk(np, kStepBlock)), dim3(kStepBlock), 0, st, np, nlocal, (const int*)c->d_pair_j.p, flag);
  RC(exclusive_scan(c, s, flag, s->d_part_scan.p, np, st));
  hipLaunchKernelGGL(part_scatter_kernel, dim3(nblk(np, kStepBlock)), dim3(kStepBlock), 0, st, np, nlocal, (const int*)c->d_pair_i.p,
                     (const int*)c->d_pair_j.p, (const int*)s->d_part_scan.p, s->d_part_i.p, s->d_part_j.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(s->h_flags + 2, s->d_part_scan.p + np, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  c->n_interior = s->h_flags[2];
  std::swap(c->d_pair_i, s->d_part_i);
  std::swap(c->d_pair_j, s->d_part_j);
  s->partitioned = true;
  return SHPAIR_OK;
}

extern "C" {

int shstep_shape_mass_props(int lmax, const double* anm, double* out)
{
  if (lmax < 0 || lmax > SHPAIR_MAX_LMAX || !anm || !out) return SHPAIR_EINVAL;
  mass_props(lmax, anm, out);
  return SHPAIR_OK;
}

int shstep_set_density(shpair_ctx* c, int ishape, double rho)
{
  if (!c) return SHPAIR_EINVAL;
  if (ishape < 0 || ishape >= c->nshapes || c->shapes[ishape].lmax < 0)
    CTX_FAIL(c, SHPAIR_EINVAL, "density: shape %d is not set", ishape);
  if (!(rho > 0.0) || !std::isfinite(rho)) CTX_FAIL(c, SHPAIR_EINVAL, "density %g must be finite and > 0", rho);
  c->shapes[ishape].density = rho;
  c->mass_dirty = true;
  return SHPAIR_OK;
}

int shstep_get_body(const shpair_ctx* c, int ishape, double* mass, double* com, double* inertia)
{
  if (!c) return SHPAIR_EINVAL;
  if (ishape < 0 || ishape >= c->nshapes || c->shapes[ishape].lmax < 0) return SHPAIR_EINVAL;
  const Shape& sh = c->shapes[ishape];
  double mp[10];
  mass_props(sh.lmax, sh.anm.data(), mp);
  if (mass) *mass = sh.density * mp[0];
  if (com)
    for (int k = 0; k < 3; ++k) com[k] = mp[1 + k];
  if (inertia)
    for (int k = 0; k < 6; ++k) inertia[k] = sh.density * mp[4 + k];
  return SHPAIR_OK;
}

int shstep_nve_device(shpair_ctx* c, int phase, int nlocal, double dt, double* x, double* v, double* quat,
                      double* angmom, const double* f, const double* torque, const int* shtype, const int* mask,
                      int groupbit, void* stream)
{
  STEP_PROLOGUE(c);
  if (phase != 0 && phase != 1) CTX_FAIL(c, SHPAIR_EINVAL, "phase %d is neither 0 (initial) nor 1 (final)", phase);
  if (nlocal < 0 || !std::isfinite(dt)) CTX_FAIL(c, SHPAIR_EINVAL, "bad nlocal (%d) or dt (%g)", nlocal, dt);
  if (nlocal == 0) return SHPAIR_OK;
  if (!x || !v || !quat || !angmom || !f || !torque || !shtype || !mask) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  RC(step_refresh_mass(c, s));
  const auto kernel = phase == 0 ? nve_kernel<0> : nve_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3(nblk(nlocal, kStepBlock)), dim3(kStepBlock), 0, (hipStream_t)stream, nlocal, dt,
                     (const double*)s->d_mass.p, c->nshapes, x, v, quat, angmom, f, torque, shtype, mask, groupbit, s->d_flags.p);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shstep_nve(shpair_ctx* c, int phase, int nlocal, double dt, double* x, double* v, double* quat, double* angmom,
               const double* f, const double* torque, const int* shtype, const int* mask, int groupbit)
{
  STEP_PROLOGUE(c);
  if (nlocal < 0) CTX_FAIL(c, SHPAIR_EINVAL, "nlocal %d < 0", nlocal);
  if (nlocal == 0) return SHPAIR_OK;
  if (!x || !v || !quat || !angmom || !f || !torque || !shtype || !mask) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  for (int i = 0; i < nlocal; ++i)
    if ((mask[i] & groupbit) && (shtype[i] < 0 || shtype[i] >= c->nshapes))
      CTX_FAIL(c, SHPAIR_EINVAL, "shtype[%d] = %d outside [0,%d)", i, shtype[i], c->nshapes);
  const size_t n = (size_t)nlocal;
  HIPCHK(c, s->s_x.ensure(3 * n)); HIPCHK(c, s->s_v.ensure(3 * n)); HIPCHK(c, s->s_q.ensure(4 * n));
  HIPCHK(c, s->s_L.ensure(3 * n)); HIPCHK(c, s->s_f.ensure(3 * n)); HIPCHK(c, s->s_t.ensure(3 * n));
  HIPCHK(c, s->s_sh.ensure(n)); HIPCHK(c, s->s_mask.ensure(n));
  hipStream_t st = c->stream;
  HIPCHK(c, upload(s->s_v, (const double*)v, 3 * n, st));
  HIPCHK(c, upload(s->s_q, (const double*)quat, 4 * n, st));
  HIPCHK(c, upload(s->s_L, (const double*)angmom, 3 * n, st));
  HIPCHK(c, upload(s->s_f, f, 3 * n, st));
  HIPCHK(c, upload(s->s_t, torque, 3 * n, st));
  HIPCHK(c, upload(s->s_sh, shtype, n, st));
  HIPCHK(c, upload(s->s_mask, mask, n, st));
  if (phase == 0) HIPCHK(c, upload(s->s_x, (const double*)x, 3 * n, st));
  RC(shstep_nve_device(c, phase, nlocal, dt, s->s_x.p, s->s_v.p, s->s_q.p, s->s_L.p, s->s_f.p, s->s_t.p, s->s_sh.p,
                       s->s_mask.p, groupbit, st));
  HIPCHK(c, download(v, s->s_v, 3 * n, st));
  HIPCHK(c, download(angmom, s->s_L, 3 * n, st));
  if (phase == 0) {
    HIPCHK(c, download(x, s->s_x, 3 * n, st));
    HIPCHK(c, download(quat, s->s_q, 4 * n, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  return SHPAIR_OK;
}

int shstep_force_clear_device(shpair_ctx* c, int nall, double* f, double* torque, void* stream)
{
  if (!c) return SHPAIR_EINVAL;
  if (nall < 0) CTX_FAIL(c, SHPAIR_EINVAL, "negative atom count");
  if (nall == 0) return SHPAIR_OK;
  if (!f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  HIPCHK(c, hipSetDevice(c->device));
  const long long n3 = 3LL * nall;
  long long blocks = (n3 + kStepBlock - 1) / kStepBlock;
  if (blocks > 4096) blocks = 4096;   // grid-stride: 16 workgroups per CU are plenty for a store-only kernel
  hipLaunchKernelGGL(force_clear_kernel, dim3((unsigned)blocks), dim3(kStepBlock), 0, (hipStream_t)stream, n3, f, torque);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shstep_post_force_device(shpair_ctx* c, int nlocal, const double* g, double gamma_t, double gamma_r, const double* v,
                             const double* quat, const double* angmom, const int* shtype, const int* mask, int groupbit,
                             double* f, double* torque, void* stream)
{
  STEP_PROLOGUE(c);
  if (nlocal < 0 || !g) CTX_FAIL(c, SHPAIR_EINVAL, "bad nlocal (%d) or null gravity", nlocal);
  if (!std::isfinite(g[0] + g[1] + g[2] + gamma_t + gamma_r)) CTX_FAIL(c, SHPAIR_EINVAL, "gravity / damping is not finite");
  if (nlocal == 0) return SHPAIR_OK;
  if (!v || !quat || !angmom || !f || !torque || !shtype || !mask) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  RC(step_refresh_mass(c, s));
  hipLaunchKernelGGL(post_force_kernel, dim3(nblk(nlocal, kStepBlock)), dim3(kStepBlock), 0, (hipStream_t)stream, nlocal,
                     (const double*)s->d_mass.p, c->nshapes, g[0], g[1], g[2], gamma_t, gamma_r, v, quat, angmom, shtype,
                     mask, groupbit, f, torque, s->d_flags.p);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shstep_energies_device(shpair_ctx* c, int nlocal, const double* g, const double* x, const double* v, const double* quat,
                           const double* angmom, const int* shtype, const int* mask, int groupbit, double* out3,
                           void* stream)
{
  STEP_PROLOGUE(c);
  if (nlocal < 0 || !g || !out3) CTX_FAIL(c, SHPAIR_EINVAL, "bad nlocal (%d), null gravity or null output", nlocal);
  if (nlocal == 0) return SHPAIR_OK;
  if (!x || !v || !quat || !angmom || !shtype || !mask) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  RC(step_refresh_mass(c, s));
  hipLaunchKernelGGL(energies_kernel, dim3(nblk(nlocal, kStepBlock)), dim3(kStepBlock), 0, (hipStream_t)stream, nlocal,
                     (const double*)s->d_mass.p, c->nshapes, g[0], g[1], g[2], x, v, quat, angmom, shtype, mask, groupbit,
                     out3, s->d_flags.p);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shstep_set_box(shpair_ctx* c, const double* lo, const double* hi, const int* periodic, double skin)
{
  STEP_PROLOGUE(c);
  if (!lo || !hi || !periodic) CTX_FAIL(c, SHPAIR_EINVAL, "null box pointer");
  if (!(skin >= 0.0) || !std::isfinite(skin)) CTX_FAIL(c, SHPAIR_EINVAL, "skin %g must be finite and >= 0", skin);
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(lo[d]) || !std::isfinite(hi[d]) || !(hi[d] > lo[d]))
      CTX_FAIL(c, SHPAIR_EINVAL, "box dimension %d: [%g, %g) is empty or not finite", d, lo[d], hi[d]);
  for (int d = 0; d < 3; ++d) {
    s->box->lo[d] = lo[d];
    s->box->hi[d] = hi[d];
    s->box->len[d] = hi[d] - lo[d];
    s->box->periodic[d] = periodic[d] ? 1 : 0;
  }
  s->skin = skin;
  s->have_box = true;
  s->l_nlocal = -1;
  s->nghost = 0;
  s->b_nlocal = 0;
  return SHPAIR_OK;
}

int shstep_borders_device(shpair_ctx* c, int nlocal, int nmax, double* x, double* quat, int* type, int* shtype, int* tag,
                          int* nghost, void* stream)
{
  STEP_PROLOGUE(c);
  if (nghost) *nghost = 0;
  if (nlocal < 0 || nmax < nlocal || !nghost) CTX_FAIL(c, SHPAIR_EINVAL, "bad nlocal (%d) / nmax (%d) / null nghost", nlocal, nmax);
  RC(step_refresh_box(c, s));
  s->nghost = 0;
  s->b_nlocal = nlocal;
  if (nlocal == 0) return SHPAIR_OK;
  if (!x || !quat || !type || !shtype) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, s->d_cnt.ensure((size_t)nlocal));
  HIPCHK(c, s->d_goff.ensure((size_t)nlocal + 1));
  hipLaunchKernelGGL(wrap_count_kernel, dim3(nblk(nlocal, kStepBlock)), dim3(kStepBlock), 0, st, nlocal, *s->box, x, s->d_cnt.p);
  RC(exclusive_scan(c, s, s->d_cnt.p, s->d_goff.p, nlocal, st));
  HIPCHK(c, hipMemcpyAsync(s->h_flags + 2, s->d_goff.p + nlocal, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int ng = s->h_flags[2];
  *nghost = ng;
  if ((long long)nlocal + ng > nmax)
    CTX_FAIL(c, SHPAIR_ENOMEM, "%d owned + %d ghost particles exceed the caller's capacity nmax = %d", nlocal, ng, nmax);
  if (ng > 0) {
    HIPCHK(c, s->d_gowner.ensure((size_t)ng));
    HIPCHK(c, s->d_gcode.ensure((size_t)ng));
    hipLaunchKernelGGL(fill_ghosts_kernel, dim3(nblk(nlocal, kStepBlock)), dim3(kStepBlock), 0, st, nlocal, nmax, *s->box,
                       (const int*)s->d_goff.p, x, quat, type, shtype, tag, s->d_gowner.p, s->d_gcode.p);
    HIPCHK(c, hipGetLastError());
  }
  s->nghost = ng;
  return SHPAIR_OK;
}

int shstep_forward_device(shpair_ctx* c, double* x, double* quat, void* stream)
{
  STEP_PROLOGUE(c);
  if (s->nghost == 0) return SHPAIR_OK;
  if (!x || !quat) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  hipLaunchKernelGGL(forward_kernel, dim3(nblk(s->nghost, kStepBlock)), dim3(kStepBlock), 0, (hipStream_t)stream, s->b_nlocal,
                     s->nghost, *s->box, (const int*)s->d_gowner.p, (const int*)s->d_gcode.p, x, quat);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shstep_reverse_device(shpair_ctx* c, double* f, double* torque, void* stream)
{
  STEP_PROLOGUE(c);
  if (s->nghost == 0) return SHPAIR_OK;
  if (!f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  hipLaunchKernelGGL(reverse_kernel, dim3(nblk(s->nghost, kStepBlock)), dim3(kStepBlock), 0, (hipStream_t)stream, s->b_nlocal,
                     s->nghost, (const int*)s->d_gowner.p, f, torque);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shstep_neighbor_build_device(shpair_ctx* c, int nlocal, int nghost, const double* x, const int* shtype, const int* tag,
                                 int* npairs, void* stream)
{
  STEP_PROLOGUE(c);
  if (npairs) *npairs = 0;
  if (nlocal < 0 || nghost < 0 || !npairs) CTX_FAIL(c, SHPAIR_EINVAL, "bad nlocal (%d) / nghost (%d) / null npairs", nlocal, nghost);
  RC(step_refresh_box(c, s));
  RC(step_refresh_mass(c, s));
  if (!tag && nghost > 0 && (nghost != s->nghost || nlocal != s->b_nlocal))
    CTX_FAIL(c, SHPAIR_ESTATE, "without tags the ghosts must be those of the last shstep_borders_device() (%d owned, %d ghosts)",
             s->b_nlocal, s->nghost);
  hipStream_t st = (hipStream_t)stream;
  const int nall = nlocal + nghost;
  // the previous list may still be in use by an enqueued compute on another stream
  HIPCHK(c, hipDeviceSynchronize());
  // SPEC §2.14: the offsets, keys and xi of the list this build replaces go aside (buffer swaps) while a spring is set
  const int old_np = c->hist_on ? step_history_put_aside(c, s, nlocal) : -1;
  if (!c->hist_on) c->hist_np = -1;   // a list built without a spring has no keys: xi of an earlier one is not its history
  c->have_neighbors = false;
  s->l_nlocal = -1;
  if (nlocal == 0) return install_empty_list(c, s, nall, st);
  if (!x || !shtype) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  int np = 0;
  RC(bin_atoms(c, s, nlocal, nall, x, st));
  RC(build_half_list(c, s, nlocal, nall, x, shtype, tag, &np, st));
  // ... and the new list's slots get their keys, and the xi of the slots that were there before
  if (c->hist_on) RC(step_history_carry(c, s, nlocal, np, tag, old_np, st));
  // no ghost j: every slot may run before the ghosts arrive; ghosts but no partition: none may
  c->n_interior = nghost > 0 ? 0 : np;
  s->partitioned = false;
  if (c->opt_overlap && nghost > 0 && np > 0) RC(partition_list(c, s, nlocal, np, st));
  c->npairs = np;
  c->max_atom_index = nall - 1;
  c->have_neighbors = true;
  s->l_nlocal = nlocal;
  *npairs = np;
  return SHPAIR_OK;
}

int shstep_neighbor_check_device(shpair_ctx* c, int nlocal, const double* x, int* rebuild, void* stream)
{
  STEP_PROLOGUE(c);
  if (!rebuild) CTX_FAIL(c, SHPAIR_EINVAL, "null rebuild pointer");
  *rebuild = 1;
  if (s->l_nlocal < 0 || nlocal != s->l_nlocal) return SHPAIR_OK;  // no list, or the particle count changed
  if (nlocal == 0) {
    *rebuild = 0;
    return SHPAIR_OK;
  }
  if (!x) CTX_FAIL(c, SHPAIR_EINVAL, "null array pointer");
  hipStream_t st = (hipStream_t)stream;
  RC(step_enqueue_displacement(c, s, nlocal, x, true, st));
  HIPCHK(c, hipStreamSynchronize(st));
  *rebuild = s->h_flags[1] ? 1 : 0;
  return step_decode_flags(c, s, st);
}

int shstep_copy_neighbors(shpair_ctx* c, int* offsets, int* jlist)
{
  STEP_PROLOGUE(c);
  if (s->l_nlocal < 0 || !c->have_neighbors) CTX_FAIL(c, SHPAIR_ESTATE, "no device-built neighbour list");
  HIPCHK(c, hipDeviceSynchronize());
  if (offsets) HIPCHK(c, hipMemcpy(offsets, s->d_offs.p, ((size_t)s->l_nlocal + 1) * sizeof(int), hipMemcpyDeviceToHost));
  // (with "halo_overlap" the context's list is partitioned interior / boundary; the row-major copy is kept beside it)
  if (jlist && c->npairs > 0)
    HIPCHK(c, hipMemcpy(jlist, s->partitioned ? s->d_part_j.p : c->d_pair_j.p, (size_t)c->npairs * sizeof(int), hipMemcpyDeviceToHost));
  return SHPAIR_OK;
}

}  // extern "C"
