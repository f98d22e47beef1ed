// shpair_api.hip — the part of the C ABI of include/shpair.h that launches kernels: installing a neighbour list, the
// pair path (shp_compute_range), the host-pointer entry point and the quadrature table, whose layout a kernel header
// defines.  The context and its options are in shpair_context.cpp, shapes and tables in shpair_tables.cpp.
// There is no CPU fallback in this library: every compute path launches the gfx950 kernels of pair_setup.hpp,
// pair_rotate.hpp and pair_kernel.hpp.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/shpair.h"
#include "fp64_peak.hpp"
#include "det_kernels.hpp"
#include "pair_params.hpp"
#include "pair_rotate.hpp"
#include "pair_setup.hpp"
#include "ring_tables.hpp"
#include "shpair_ctx.hpp"
#include "sh_const.hpp"
#include "sh_tables.hpp"

namespace shp {
#define SHP_DECL(L) void shp_launch_L##L(const PairParams&, const ContactPlan&, bool, hipStream_t, hipEvent_t); \
  const void* shp_instance_L##L(const ContactPlan&, bool);
SHP_DECL(0) SHP_DECL(1) SHP_DECL(2) SHP_DECL(3) SHP_DECL(4) SHP_DECL(5) SHP_DECL(6)
SHP_DECL(7) SHP_DECL(8) SHP_DECL(9) SHP_DECL(10) SHP_DECL(11) SHP_DECL(12) SHP_DECL(rt)
#undef SHP_DECL

static const pair_launch_fn kLaunch[kMaxUnrolledL + 1] = {
    shp_launch_L0, shp_launch_L1, shp_launch_L2, shp_launch_L3, shp_launch_L4, shp_launch_L5, shp_launch_L6,
    shp_launch_L7, shp_launch_L8, shp_launch_L9, shp_launch_L10, shp_launch_L11, shp_launch_L12};
static const pair_instance_fn kInstance[kMaxUnrolledL + 1] = {
    shp_instance_L0, shp_instance_L1, shp_instance_L2, shp_instance_L3, shp_instance_L4, shp_instance_L5, shp_instance_L6,
    shp_instance_L7, shp_instance_L8, shp_instance_L9, shp_instance_L10, shp_instance_L11, shp_instance_L12};

// VGPRs of the order's general two-wave kernel (plan_contact sizes two-wave ring groups by them): read once per order
static int two_wave_vgprs(const int L)
{
  static std::atomic<int> known[kMaxUnrolledL + 1];   // 0: not read yet
  if (L > kMaxUnrolledL || !split_compiled(L)) return 0;
  hipFuncAttributes fa;
  if (known[L] == 0 && hipFuncGetAttributes(&fa, kInstance[L](ContactPlan{true, 1, 2}, true)) == hipSuccess) known[L] = fa.numRegs;
  return known[L];
}

// Sums the per-slot flags the pair kernel wrote: out[0] = contact pairs
// (flag >= 1), out[1] = touching pairs (flag == 2). One atomic per wave.
__global__ void count_flags_kernel(const unsigned char* __restrict__ flags, int npairs, unsigned long long* out)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned char fl = (p < npairs) ? flags[p] : 0;
  const unsigned long long m1 = __ballot(fl >= 1), m2 = __ballot(fl == 2);
  if ((threadIdx.x & 63) == 0) {
    if (m1) atomicAdd(&out[0], (unsigned long long)__popcll(m1));
    if (m2) atomicAdd(&out[1], (unsigned long long)__popcll(m2));
  }
}

// Expands a device-resident CSR half list into one (i, j) per slot; one thread per row segment entry.
__global__ void expand_csr_kernel(const int* __restrict__ ilist, const int* __restrict__ offsets,
                                  const int* __restrict__ jlist, int inum, int* __restrict__ pair_i,
                                  int* __restrict__ pair_j)
{
  // one wave per row: rows are short (~6 entries), lanes stride the row
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (row >= inum) return;
  const int b = offsets[row], e = offsets[row + 1], i = ilist[row];
  for (int p = b + lane; p < e; p += 64) {
    pair_i[p] = i;
    pair_j[p] = jlist[p] & SHPAIR_NEIGHMASK;
  }
}

}  // namespace shp

using namespace shp;

// ---- installing a neighbour list ---------------------------------------------------------------------------------

// Host list -> device: the rows are flattened into ONE pinned buffer [ilist | offsets | jlist] (a LAMMPS list is
// paged, so one pass over it is unavoidable), uploaded with one copy and expanded to one (i, j) per slot on the
// device (expand_csr_kernel, which also strips the NEIGHMASK bits).
static int stage_list(shpair_ctx* c, int inum, size_t tot)
{
  const size_t need = 2 * (size_t)inum + 1 + tot;
  if (c->h_list.cap < need) HIPCHK(c, c->h_list.resize(need + need / 4 + 64));
  return SHPAIR_OK;
}

// a device-resident CSR list into the context's (i, j) slots: one wave per row
static int expand_csr(shpair_ctx* c, int inum, const int* ilist, const int* offsets, const int* jlist, hipStream_t st)
{
  const int threads = 256, rows_per_block = threads / 64;
  hipLaunchKernelGGL(expand_csr_kernel, dim3((inum + rows_per_block - 1) / rows_per_block), dim3(threads), 0, st, ilist, offsets,
                     jlist, inum, c->d_pair_i.p, c->d_pair_j.p);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

// the common tail of a list install from outside: per-slot buffers, counts, generation.  Which slots touch ghosts
// is not known here (n_interior = 0).
static int list_installed(shpair_ctx* c, size_t npairs, int max_index)
{
  HIPCHK(c, shp_size_pair_buffers(c, npairs));
  c->npairs = (int)npairs;
  c->n_interior = 0;
  c->max_atom_index = max_index;
  c->have_neighbors = true;
  ++c->list_gen;
  c->hist_np = -1;   // a caller's list has no keys: the contact history is dropped (SPEC §2.14)
  shstep_invalidate_list(c);
  return SHPAIR_OK;
}

static int upload_staged_list(shpair_ctx* c, int inum, size_t tot, int max_index)
{
  HIPCHK(c, hipSetDevice(c->device));
  const size_t need = 2 * (size_t)inum + 1 + tot;
  HIPCHK(c, c->d_list.ensure(need ? need : 1));
  HIPCHK(c, c->d_pair_i.ensure(tot ? tot : 1));
  HIPCHK(c, c->d_pair_j.ensure(tot ? tot : 1));
  // the previous list may still be in use by an enqueued compute
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (tot > 0) {
    HIPCHK(c, upload(c->d_list, (const int*)c->h_list, need, c->stream));
    const int* d = c->d_list.p;
    RC(expand_csr(c, inum, d, d + inum, d + 2 * (size_t)inum + 1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return list_installed(c, tot, max_index);
}

// the integrals the dissipation pass reads and, in deterministic mode, the rows it writes
hipError_t shp_size_dissipation_buffers(shpair_ctx* c, size_t np)
{
  if (!shp_keeps_integrals(c)) return hipSuccess;
  if (np == 0) np = 1;
  hipError_t e = c->pair_out ? hipSuccess : c->d_slot_int.ensure(np * 7);   // 56 B per slot
  if (e == hipSuccess && c->opt_deterministic) e = c->d_slot_ft.ensure(np * 12);
  if (e == hipSuccess && c->ledger_on) e = c->d_slot_pow.ensure(2 * (np + nblk((long long)np, kLedgerChunk)));   // SPEC §2.13
  // SPEC §2.14: 24 B + 4 B per slot.  They never grow under a live history: a list of another size comes from a build,
  // which has put the previous list's away by then.
  if (e == hipSuccess && c->hist_on) e = c->d_xi.ensure(3 * np);
  if (e == hipSuccess && c->hist_on) e = c->d_hkey.ensure(np);
  return e;
}

// Sizes the per-slot buffers the pair kernels write (records; rotated coefficient vectors of the JPT family) for a
// list of `np` slots: called wherever a list is installed, so that a compute — possibly inside a stream capture —
// allocates nothing.
hipError_t shp_size_pair_buffers(shpair_ctx* c, size_t np)
{
  if (np == 0) np = 1;
  c->rev_dirty = true;   // a list is being installed: the reverse index of the deterministic mode is stale
  c->integrals_src = nullptr; // ... and so are the integrals of the previous list
  c->ledger_pair_fresh = false;   // ... and the power rows of a pass over it (SPEC §2.13)
  c->ledger_rows_pair = false;
  hipError_t e = shp_size_dissipation_buffers(c, np);
  if (e == hipSuccess) e = c->d_rec.ensure(np * kRecStride);
  if (e == hipSuccess && c->opt_deterministic) {
    e = c->d_pair_ft.ensure(np * 12);
    if (e == hipSuccess) e = c->d_rev_ent.ensure(np * 2);
  }
  if (e == hipSuccess) e = c->d_rec_i.ensure(np * 4);
  if (e == hipSuccess) e = c->d_pair_ev.ensure(8 * (np + (np + kTallyChunk - 1) / kTallyChunk));   // 64 B per slot: thermo steps
  int L = c->lmax;
  for (int s = 0; s < c->nshapes; ++s)
    if (c->shapes[s].lmax > L) L = c->shapes[s].lmax;
  if (e == hipSuccess && L >= 0 && c->nq > 0) {
    if (contact_family(L, c->nq, c->plan_opt) == 1) e = c->d_rot.ensure(rot_buffer_doubles(L, 2 * np));
  }
  return e;
}

// ---- the quadrature table (layout: ring_tables.hpp QuadLayout) ----------------------------------------------------

int shpair_upload_quadrature(shpair_ctx* c)
{
  const int nq = c->nq;
  const QuadLayout lay(c->lmax, nq);
  std::vector<double> t, w, q(lay.size);
  gauss_legendre(nq, t, w);
  for (int k = 0; k < nq; ++k) {
    q[lay.glt + k] = t[k];
    q[lay.glw + k] = w[k];
  }
  for (int l = 0; l < lay.npsi; ++l) {
    const double psi = 2.0 * 3.14159265358979323846264338327950288 * (l + 0.5) / lay.npsi;
    q[lay.cpsi + l] = std::cos(psi);
    q[lay.spsi + l] = std::sin(psi);
    for (int m = 2; m <= c->lmax; ++m) {
      q[lay.trig_at(l, m)] = std::cos(m * psi);
      q[lay.trig_at(l, m) + 1] = std::sin(m * psi);
    }
    if (l < nq)
      for (int m = 0; m <= c->lmax + 1; ++m) {
        q[lay.trigj_at(l, m)] = std::cos(m * psi);
        q[lay.trigj_at(l, m) + 1] = std::sin(m * psi);
      }
  }
  HIPCHK(c, hipDeviceSynchronize());  // a kernel still in flight on any stream may be reading the old table
  HIPCHK(c, c->d_quad.ensure(q.size()));
  HIPCHK(c, hipMemcpy(c->d_quad.p, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice));
  c->quad_dirty = false;
  return SHPAIR_OK;
}

// ---- the pair path over a range of list slots: the steps of shp_compute_range ------------------------------------

static int check_range_args(shpair_ctx* c, int nlocal, int nghost, int eflag, int vflag, const double* ev, int slot0, int slot_end)
{
  if (slot0 < 0 || slot_end < slot0 || slot_end > c->npairs || (slot0 & 31) != 0)
    CTX_FAIL(c, SHPAIR_EINVAL, "compute range [%d, %d) of a list of %d slots (the first slot must be a multiple of 32)", slot0,
             slot_end, c->npairs);
  if (nlocal < 0 || nghost < 0) CTX_FAIL(c, SHPAIR_EINVAL, "negative atom counts");
  if (!c->have_neighbors) CTX_FAIL(c, SHPAIR_ESTATE, "no neighbour list: call shpair_set_neighbors() first");
  if ((eflag || vflag) && !ev) CTX_FAIL(c, SHPAIR_EINVAL, "eflag/vflag set but ev_dev is null");
  return SHPAIR_OK;
}

// The accumulation uses hardware FP64 atomics (-munsafe-fp-atomics), which are only reliable on ordinary
// (coarse-grained) device memory: on host-coherent / managed allocations the adds can be dropped silently.
static int check_output_pointers(shpair_ctx* c, const double* f, const double* torque, const double* ev)
{
  const void* outp[3] = {f, torque, ev};
  for (int k = 0; k < 3; ++k) {
    if (!outp[k] || outp[k] == c->ok_ptr[k]) continue;
    const char* name = k == 0 ? "f" : (k == 1 ? "torque" : "ev");
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, outp[k]);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      CTX_FAIL(c, SHPAIR_EINVAL, "%s is not a device pointer known to HIP (%s): the output arrays must be hipMalloc memory", name,
               hipGetErrorString(e));
    }
    if (at.type != hipMemoryTypeDevice)
      CTX_FAIL(c, SHPAIR_EINVAL, "%s is %s memory: the FP64 atomic accumulation needs ordinary device memory (hipMalloc)", name,
               at.type == hipMemoryTypeManaged ? "managed" : "host");
    c->ok_ptr[k] = outp[k];
  }
  return SHPAIR_OK;
}

// The per-slot buffers a launch writes.  They are sized when a list is installed (shp_size_pair_buffers), so nothing
// is allocated here — a compute may be inside a stream capture — unless an option changed since, or a caller swapped
// the list behind the context's back.
static int ensure_slot_buffers(shpair_ctx* c, bool tally, const ContactPlan& plan)
{
  const size_t np = (size_t)c->npairs;
  if (c->opt_deterministic) {
    const size_t nall_idx = (size_t)c->max_atom_index + 1;
    HIPCHK(c, c->d_pair_ft.ensure(np * 12));
    HIPCHK(c, c->d_rev_ent.ensure(np * 2));
    HIPCHK(c, c->d_rev_start.ensure(nall_idx + 1));
    HIPCHK(c, c->d_rev_cur.ensure(nall_idx + 1));
  }
  // per-slot rows + the block sums behind them
  if (tally) HIPCHK(c, c->d_pair_ev.ensure(8 * (np + (np + kTallyChunk - 1) / kTallyChunk)));
  if (c->opt_count) HIPCHK(c, c->d_flags.ensure(np));
  HIPCHK(c, c->d_rec.ensure(np * kRecStride));
  HIPCHK(c, c->d_rec_i.ensure(np * 4));
  if (plan.family == 1) HIPCHK(c, c->d_rot.ensure(rot_buffer_doubles(c->lmax, 2 * np)));
  HIPCHK(c, shp_size_dissipation_buffers(c, np));
  return SHPAIR_OK;
}

struct AtomArrays {
  int nlocal;
  const double *x, *quat;
  const int *type, *shtype;
  double *f, *torque, *ev;
};

// the kernel arguments: the caller's arrays, the slot range, the context's tables and buffers, the plan
static PairParams pair_params(const shpair_ctx* c, const AtomArrays& a, int slot0, int slot_end, int newton_pair, int eflag,
                              int vflag, const ContactPlan& plan)
{
  PairParams P;
  P.x = a.x; P.quat = a.quat; P.type = a.type; P.shtype = a.shtype; P.f = a.f; P.torque = a.torque;
  P.pair_i = c->d_pair_i.p; P.pair_j = c->d_pair_j.p; P.npairs = slot_end; P.slot0 = slot0;
  P.nlocal = a.nlocal; P.newton_pair = newton_pair ? 1 : 0;
  P.rc = c->d_rc.p; P.coef = c->d_coef.p; P.rmax = c->d_rmax.p; P.cstride = c->cstride; P.lmax = c->lmax;
  P.nshapes = c->nshapes; P.err = c->d_err.p;
  P.kn = c->d_kn.p; P.expo = c->d_expo.p; P.ntypes = c->ntypes;
  const QuadLayout lay(c->lmax, c->nq);
  const double* q = c->d_quad.p;
  P.glt = q + lay.glt; P.glw = q + lay.glw; P.cpsi = q + lay.cpsi; P.spsi = q + lay.spsi;
  P.trig = q + lay.trig; P.trig_stride = lay.trig_stride; P.trigj = q + lay.trigj;
  P.nq = c->nq;
  P.rule = c->plan_opt.rule;
  P.eatom = c->eatom_dev;
  P.vatom = c->vatom_dev;
  P.creal = c->d_creal.p; P.xval = c->d_xval.p; P.xcol = c->d_xcol.p; P.xinfo = c->d_xinfo.p; P.gscale = c->d_gscale.p;
  P.jval = c->d_jval.p; P.jcol = c->d_jcol.p;
  P.jpoly = plan.family; P.split = plan.waves_per_pair == 2 ? 1 : 0; P.ring_rows = plan.ring_rows; P.qcap = plan.qcap;
  P.wave_lds_bytes = plan.lds_bytes; P.waves_per_block = plan.waves_per_block; P.spec = c->plan_opt.spec ? 1 : 0;
  P.pair_ft = c->opt_deterministic ? c->d_pair_ft.p : nullptr;   // stores instead of atomics
  P.ev = a.ev;
  // while a pair coefficient is set, the integrals go to the context's own buffer unless the caller installed one (SPEC §2.10)
  P.pair_out = (c->pair_out || !shp_keeps_integrals(c)) ? c->pair_out : c->d_slot_int.p;
  P.pair_ev = (eflag || vflag) ? c->d_pair_ev.p : nullptr;
  P.flags = c->opt_count ? c->d_flags.p : nullptr;
  P.dbg = c->dbg;
  P.eflag = eflag ? 1 : 0; P.vflag = vflag ? 1 : 0;
  P.rec = c->d_rec.p;
  P.rec_i = c->d_rec_i.p;
  P.rot = plan.family == 1 ? c->d_rot.p : nullptr;
  return P;
}

// deterministic accumulation: the reverse index (atom -> its list slots), once per list
static int build_reverse_index(shpair_ctx* c, hipStream_t st)
{
  const int nall_idx = c->max_atom_index + 1;
  if (!c->rev_dirty && c->rev_nall == nall_idx) return SHPAIR_OK;
  const dim3 slots((c->npairs + kDetBlock - 1) / kDetBlock), block(kDetBlock);
  const int *pi = c->d_pair_i.p, *pj = c->d_pair_j.p;
  HIPCHK(c, hipMemsetAsync(c->d_rev_cur.p, 0, ((size_t)nall_idx + 1) * sizeof(int), st));
  hipLaunchKernelGGL(det_count_kernel, slots, block, 0, st, c->npairs, pi, pj, nall_idx, c->d_rev_cur.p);
  HIPCHK(c, hipGetLastError());
  RC(shstep_exclusive_scan(c, c->d_rev_cur.p, c->d_rev_start.p, nall_idx, st));
  HIPCHK(c, hipMemsetAsync(c->d_rev_cur.p, 0, ((size_t)nall_idx + 1) * sizeof(int), st));
  hipLaunchKernelGGL(det_fill_kernel, slots, block, 0, st, c->npairs, pi, pj, nall_idx, (const int*)c->d_rev_start.p, c->d_rev_cur.p,
                     c->d_rev_ent.p);
  hipLaunchKernelGGL(det_sort_kernel, dim3((nall_idx + kDetBlock - 1) / kDetBlock), block, 0, st, nall_idx,
                     (const int*)c->d_rev_start.p, c->d_rev_ent.p);
  HIPCHK(c, hipGetLastError());
  c->rev_dirty = false;
  c->rev_nall = nall_idx;
  return SHPAIR_OK;
}

// kPartPre: what has to happen once before the first slot of a step: clean per-slot buffers, the start-of-timing event
static int compute_pre(shpair_ctx* c, const PairParams& P, hipStream_t st)
{
  const size_t np = (size_t)c->npairs;
  if (P.pair_ft) HIPCHK(c, hipMemsetAsync(c->d_pair_ft.p, 0, np * 12 * sizeof(double), st));
  if (P.pair_ev) HIPCHK(c, hipMemsetAsync(c->d_pair_ev.p, 0, 8 * np * sizeof(double), st));
  // the contact kernels do not write the integrals of a slot culled before the epilogue: the damping pass reads zeros there
  if (shp_keeps_integrals(c)) HIPCHK(c, hipMemsetAsync(P.pair_out, 0, 7 * np * sizeof(double), st));
  if (P.flags) {
    HIPCHK(c, hipMemsetAsync(c->d_counters.p, 0, 2 * sizeof(unsigned long long), st));
    HIPCHK(c, hipMemsetAsync(c->d_flags.p, 0, np, st));
  }
  if (c->opt_timing) HIPCHK(c, hipEventRecord(c->ev0, st));
  return SHPAIR_OK;
}

// the set-up kernel (per-pair records, pair_setup.hpp), then the contact kernel of the plan
static int launch_range(shpair_ctx* c, PairParams P, const ContactPlan& plan, bool needv, hipStream_t st)
{
  launch_pair_setup(P, c->d_rec.p, c->d_rec_i.p, st);
  if (plan.compiled) {
    P.coef = c->d_coefm.p;  // compiled orders read the monomial (Horner) table
    kLaunch[c->lmax](P, plan, needv, st, c->pre_contact_wait);
  } else {
    shp_launch_Lrt(P, plan, needv, st, c->pre_contact_wait);
  }
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

int shp_det_gather(shpair_ctx* c, const double* pair_ft, double* f, double* torque, hipStream_t st)
{
  const int nall_idx = c->max_atom_index + 1;
  hipLaunchKernelGGL(det_gather_kernel, dim3((6 * nall_idx + kDetBlock - 1) / kDetBlock), dim3(kDetBlock), 0, st, nall_idx,
                     (const int*)c->d_rev_start.p, (const int*)c->d_rev_ent.p, pair_ft, f, torque);
  HIPCHK(c, hipGetLastError());
  return SHPAIR_OK;
}

// kPartPost: what follows the last slot: ordered gather, tally reduce, end-of-timing event, contact counts
static int compute_post(shpair_ctx* c, const PairParams& P, hipStream_t st)
{
  if (P.pair_ft) RC(shp_det_gather(c, c->d_pair_ft.p, P.f, P.torque, st));
  if (shp_keeps_integrals(c)) {   // what shstep_pair_damping_device / shstep_pair_dissipation_device read
    c->integrals_src = P.pair_out;
    c->integrals_needv = c->last_needv;
    c->ledger_rows_pair = false;   // power rows a pair pass wrote belong to the integrals this compute replaced (SPEC §2.16)
  }
  if (P.pair_ev) {
    const int tally_blocks = (c->npairs + kTallyChunk - 1) / kTallyChunk;
    double* part = c->d_pair_ev.p + 8 * (size_t)c->npairs;
    hipLaunchKernelGGL(tally_partial_kernel, dim3(tally_blocks), dim3(kTallyBlock), 0, st, c->npairs, (const double*)c->d_pair_ev.p, part);
    hipLaunchKernelGGL(tally_final_kernel, dim3(1), dim3(kTallyBlock), 0, st, tally_blocks, (const double*)part, P.ev, P.eflag, P.vflag);
    HIPCHK(c, hipGetLastError());
  }
  if (c->opt_timing) {
    HIPCHK(c, hipEventRecord(c->ev1, st));
    c->timed_last = true;
  }
  if (P.flags) {
    hipLaunchKernelGGL(count_flags_kernel, dim3((c->npairs + 255) / 256), dim3(256), 0, st, c->d_flags.p, c->npairs,
                       c->d_counters.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, download((unsigned long long*)c->h_counters, c->d_counters, 2, st));
    HIPCHK(c, hipEventRecord(c->evB, st));
    c->counted_last = true;
  }
  return SHPAIR_OK;
}

// ---- the host-pointer entry point: the two halves of shpair_compute around the device call ------------------------

// everything up: types and shape indices, the per-atom tallies of the host form, positions, and f / torque on the
// second stream
static int stage_inputs(shpair_ctx* c, size_t nall, const double* x, const double* quat, const int* type, const int* shtype,
                        const double* f, const double* torque, hipStream_t st)
{
  HIPCHK(c, c->d_x.ensure(3 * nall));
  HIPCHK(c, c->d_quat.ensure(4 * nall));
  HIPCHK(c, c->d_type.ensure(nall));
  HIPCHK(c, c->d_shtype.ensure(nall));
  HIPCHK(c, c->d_f.ensure(3 * nall));
  HIPCHK(c, c->d_torque.ensure(3 * nall));
  // Types and shape indices are not range-checked on the host any more (an O(nall) scan per step): the kernel guards
  // its table reads and raises an error bit, which shpair_compute reads back and reports.  They are uploaded every
  // call: LAMMPS may change a type without reneighbouring (fix atom/swap).
  HIPCHK(c, upload(c->d_type, type, nall, st));
  HIPCHK(c, upload(c->d_shtype, shtype, nall, st));
  // per-atom tallies of the host form: staged like the forces (shpair_set_peratom_host).  ADD semantics without a host
  // pass: the caller's values go up, the kernel adds to them, the sums come back
  const bool pe = c->eatom_host != nullptr, pv = c->vatom_host != nullptr;
  if (pe) HIPCHK(c, c->d_eatom.ensure(nall));
  if (pv) HIPCHK(c, c->d_vatom.ensure(6 * nall));
  if (pe) HIPCHK(c, upload(c->d_eatom, (const double*)c->eatom_host, nall, st));
  if (pv) HIPCHK(c, upload(c->d_vatom, (const double*)c->vatom_host, 6 * nall, st));
  if (pe || pv) {
    c->eatom_dev = pe ? c->d_eatom.p : nullptr;
    c->vatom_dev = pv ? c->d_vatom.p : nullptr;
  }
  HIPCHK(c, hipEventRecord(c->evA, st));
  HIPCHK(c, upload(c->d_x, x, 3 * nall, st));
  HIPCHK(c, upload(c->d_quat, quat, 4 * nall, st));
  // f and torque are ADDED to (another pair style of a hybrid run, or a pre_force fix, may have been there first): they
  // travel up, the kernel accumulates into them on the device, and the sums overwrite the host arrays.  Measured at
  // 100k atoms against staging zeros and adding on the host (interleaved runs, tools/gpu_check.py): call wall time
  // minus kernel time 0.45 ms instead of 0.52 ms; 16 MB cross PCIe per call either way.
  // They go up on a second stream, beside the set-up and rotation kernels, which do not touch them: the contact kernel
  // (its epilogue's atomics; the gather of the deterministic mode) waits for the event.  With the caller's arrays
  // registered (shpair_pin_host) the copies are true asynchronous DMA and the overlap is real; pageable memory is
  // staged by the runtime and mostly serialises.
  HIPCHK(c, hipEventRecord(c->ev_up, st));                 // the previous call's read-back of d_f / d_torque is long done;
  HIPCHK(c, hipStreamWaitEvent(c->stream_up, c->ev_up, 0));   // orders the second stream behind this one all the same
  HIPCHK(c, upload(c->d_f, f, 3 * nall, c->stream_up));
  HIPCHK(c, upload(c->d_torque, torque, 3 * nall, c->stream_up));
  HIPCHK(c, hipEventRecord(c->ev_up, c->stream_up));
  HIPCHK(c, hipMemsetAsync(c->d_ev.p, 0, 7 * sizeof(double), st));
  return SHPAIR_OK;
}

// everything down, and the call blocks until it has arrived
static int fetch_outputs(shpair_ctx* c, size_t nall, double* f, double* torque, hipStream_t st)
{
  if (c->eatom_host) HIPCHK(c, download(c->eatom_host, c->d_eatom, nall, st));
  if (c->vatom_host) HIPCHK(c, download(c->vatom_host, c->d_vatom, 6 * nall, st));
  HIPCHK(c, download(f, c->d_f, 3 * nall, st));
  HIPCHK(c, download(torque, c->d_torque, 3 * nall, st));
  HIPCHK(c, download((double*)c->h_ev, c->d_ev, 7, st));
  HIPCHK(c, download((int*)c->h_err, c->d_err, 1, st));
  HIPCHK(c, hipEventRecord(c->evB, st));
  HIPCHK(c, hipStreamSynchronize(st));
  c->total_timed_last = true;
  return SHPAIR_OK;
}

extern "C" {

int shpair_set_neighbors(shpair_ctx* c, int inum, const int* ilist, const int* numneigh, const int* const* firstneigh)
{
  if (!c) return SHPAIR_EINVAL;
  if (inum < 0 || (inum > 0 && (!ilist || !numneigh || !firstneigh))) CTX_FAIL(c, SHPAIR_EINVAL, "bad neighbour list arguments");
  size_t tot = 0;
  for (int ii = 0; ii < inum; ++ii) {
    const int i = ilist[ii];
    if (i < 0) CTX_FAIL(c, SHPAIR_EINVAL, "negative atom index in ilist (row %d)", ii);
    const int n = numneigh[i];
    if (n < 0) CTX_FAIL(c, SHPAIR_EINVAL, "numneigh[%d] = %d", i, n);
    if (n > 0 && !firstneigh[i]) CTX_FAIL(c, SHPAIR_EINVAL, "firstneigh[%d] is null", i);
    tot += (size_t)n;
  }
  if (tot > 0x7fffffffULL) CTX_FAIL(c, SHPAIR_EINVAL, "half list too long (%zu pairs)", tot);
  RC(stage_list(c, inum, tot));
  int* il = c->h_list;
  int* of = c->h_list + inum;
  int* jl = c->h_list + 2 * (size_t)inum + 1;
  int mx = -1;
  size_t p = 0;
  for (int ii = 0; ii < inum; ++ii) {
    const int i = ilist[ii];
    const int n = numneigh[i];
    const int* row = firstneigh[i];
    il[ii] = i;
    of[ii] = (int)p;
    if (i > mx) mx = i;
    for (int jj = 0; jj < n; ++jj) {
      const int j = row[jj] & SHPAIR_NEIGHMASK;
      jl[p + jj] = j;
      if (j > mx) mx = j;
    }
    p += (size_t)n;
  }
  if (inum >= 0) of[inum] = (int)p;
  return upload_staged_list(c, inum, tot, mx);
}

int shpair_set_neighbors_csr(shpair_ctx* c, int inum, const int* ilist, const int* offsets, const int* jlist)
{
  if (!c) return SHPAIR_EINVAL;
  if (inum < 0 || (inum > 0 && (!ilist || !offsets))) CTX_FAIL(c, SHPAIR_EINVAL, "bad neighbour list arguments");
  size_t tot = 0;
  if (inum > 0) {
    if (offsets[0] != 0) CTX_FAIL(c, SHPAIR_EINVAL, "offsets[0] must be 0");
    if (offsets[inum] < 0 || (offsets[inum] > 0 && !jlist)) CTX_FAIL(c, SHPAIR_EINVAL, "bad CSR neighbour list");
    tot = (size_t)offsets[inum];
    for (int ii = 0; ii < inum; ++ii) {
      if (offsets[ii + 1] < offsets[ii]) CTX_FAIL(c, SHPAIR_EINVAL, "offsets not monotone at %d", ii);
      if (ilist[ii] < 0) CTX_FAIL(c, SHPAIR_EINVAL, "negative atom index in ilist (row %d)", ii);
    }
  }
  RC(stage_list(c, inum, tot));
  int mx = -1;
  if (inum > 0) {
    std::memcpy(c->h_list, ilist, (size_t)inum * sizeof(int));
    std::memcpy(c->h_list + inum, offsets, ((size_t)inum + 1) * sizeof(int));
    int* jl = c->h_list + 2 * (size_t)inum + 1;
    for (int ii = 0; ii < inum; ++ii)
      if (ilist[ii] > mx) mx = ilist[ii];
    for (size_t k = 0; k < tot; ++k) {
      const int j = jlist[k] & SHPAIR_NEIGHMASK;
      jl[k] = j;
      if (j > mx) mx = j;
    }
  } else {
    c->h_list[0] = 0;
  }
  return upload_staged_list(c, inum, tot, mx);
}

int shpair_set_neighbors_device(shpair_ctx* c, int inum, const int* ilist, const int* offsets, const int* jlist,
                                int npairs, int max_atom_index, void* stream)
{
  if (!c) return SHPAIR_EINVAL;
  if (inum < 0 || npairs < 0 || (inum > 0 && (!ilist || !offsets)) || (npairs > 0 && !jlist))
    CTX_FAIL(c, SHPAIR_EINVAL, "bad device neighbour list arguments");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_pair_i.ensure(npairs ? npairs : 1));
  HIPCHK(c, c->d_pair_j.ensure(npairs ? npairs : 1));
  if (inum > 0 && npairs > 0) RC(expand_csr(c, inum, ilist, offsets, jlist, (hipStream_t)stream));
  return list_installed(c, (size_t)npairs, max_atom_index);
}

// The pair path over a RANGE of list slots.  part & kPartPre: everything that has to happen once before the first slot
// of a step (buffer memsets of the deterministic mode and the tallies, the reverse index, the start-of-timing event);
// part & kPartPost: what follows the last slot (ordered gather, tally reduce, end-of-timing event, contact counts).
// shpair_compute_device = both parts over the whole list; the halo loop (shhalo_run.cpp) runs the slots whose atoms
// are all owned — [0, split) — with kPartPre while the forward exchange is in flight, then [split, npairs) with
// kPartPost.  `split` must be a multiple of 32 (rotation tiles).
int shpair_compute_device(shpair_ctx* c, int nlocal, int nghost, const double* x, const double* quat, const int* type,
                          const int* shtype, int newton_pair, int eflag, int vflag, double* f, double* torque,
                          double* ev, void* stream)
{
  if (!c) return SHPAIR_EINVAL;
  return shp_compute_range(c, nlocal, nghost, x, quat, type, shtype, newton_pair, eflag, vflag, f, torque, ev, stream, 0,
                           c->npairs, kPartPre | kPartPost);
}

int shp_compute_range(shpair_ctx* c, int nlocal, int nghost, const double* x, const double* quat, const int* type,
                      const int* shtype, int newton_pair, int eflag, int vflag, double* f, double* torque, double* ev,
                      void* stream, const int slot0, const int slot_end, const int part)
{
  if (!c) return SHPAIR_EINVAL;
  RC(check_range_args(c, nlocal, nghost, eflag, vflag, ev, slot0, slot_end));
  HIPCHK(c, hipSetDevice(c->device));
  if (c->tables_dirty || c->quad_dirty) RC(shpair_prepare_tables(c));
  if (part & kPartPre) {
    c->timed_last = false;
    c->counted_last = false;
    c->stats.n_candidates = c->npairs;
  }
  if (c->npairs == 0) return SHPAIR_OK;
  if (!x || !quat || !type || !shtype || !f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null atom array");
  if ((long long)c->max_atom_index >= (long long)nlocal + nghost)
    CTX_FAIL(c, SHPAIR_EINVAL, "the neighbour list refers to atom %d but nlocal + nghost = %lld (stale list?)",
             c->max_atom_index, (long long)nlocal + nghost);
  RC(check_output_pointers(c, f, torque, ev));
  hipStream_t st = (hipStream_t)stream;  // NULL = HIP null stream
  // the launch plan: kernel family, waves per pair, ring rows, queue, LDS, waves per workgroup (contact_plan.hpp)
  ContactPlan plan;
  char msg[256] = "";
  if (const int rc = plan_contact(c->lmax, c->nq, c->plan_opt, two_wave_vgprs(c->lmax), plan, msg, (int)sizeof(msg)))
    CTX_FAIL(c, rc, "%s", msg);
  c->last_plan = plan;
  RC(ensure_slot_buffers(c, eflag || vflag, plan));
  const PairParams P = pair_params(c, AtomArrays{nlocal, x, quat, type, shtype, f, torque, ev}, slot0, slot_end, newton_pair, eflag,
                                   vflag, plan);
  const bool needv = c->opt_force_volume || eflag || c->any_nonunit_exponent || c->eatom_dev != nullptr;
  c->last_needv = needv || plan.weighted;   // the template argument launched: the weighted rule has one instance, with the volume path
  if (c->opt_deterministic) RC(build_reverse_index(c, st));
  if (part & kPartPre) RC(compute_pre(c, P, st));
  RC(launch_range(c, P, plan, needv, st));
  if (part & kPartPost) RC(compute_post(c, P, st));
  return SHPAIR_OK;
}

int shpair_compute(shpair_ctx* c, int nlocal, int nghost, const double* x, const double* quat, const int* type,
                   const int* shtype, int newton_pair, int eflag, int vflag, double* f, double* torque,
                   double* eng_vdwl, double* virial)
{
  if (!c) return SHPAIR_EINVAL;
  if (nlocal < 0 || nghost < 0) CTX_FAIL(c, SHPAIR_EINVAL, "negative atom counts");
  if (!c->have_neighbors) CTX_FAIL(c, SHPAIR_ESTATE, "no neighbour list: call shpair_set_neighbors() first");
  const size_t nall = (size_t)nlocal + (size_t)nghost;
  if (nall == 0 || c->npairs == 0) {
    c->stats.n_candidates = c->npairs;
    c->timed_last = c->counted_last = false;
    return SHPAIR_OK;
  }
  if (!x || !quat || !type || !shtype || !f || !torque) CTX_FAIL(c, SHPAIR_EINVAL, "null atom array");
  if (eflag && !eng_vdwl) CTX_FAIL(c, SHPAIR_EINVAL, "eflag set but eng_vdwl is null");
  if (vflag && !virial) CTX_FAIL(c, SHPAIR_EINVAL, "vflag set but virial is null");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // the staged per-atom tallies stand in for the device-form pointers for the duration of this call, whatever way it ends
  struct Restore {
    shpair_ctx* c;
    double *e, *v;
    ~Restore() { c->eatom_dev = e; c->vatom_dev = v; }
  } restore{c, c->eatom_dev, c->vatom_dev};
  RC(stage_inputs(c, nall, x, quat, type, shtype, f, torque, st));
  c->pre_contact_wait = c->ev_up;
  const int rc = shpair_compute_device(c, nlocal, nghost, c->d_x.p, c->d_quat.p, c->d_type.p, c->d_shtype.p,
                                       newton_pair, eflag, vflag, c->d_f.p, c->d_torque.p, c->d_ev.p, st);
  c->pre_contact_wait = nullptr;
  HIPCHK(c, hipStreamWaitEvent(st, c->ev_up, 0));   // whatever path the launch took (no pairs, an early error): st is behind the uploads
  if (rc) {
    (void)hipStreamSynchronize(st);   // stream_up may still be reading the caller's f / torque: not after this call has returned
    return rc;
  }
  RC(fetch_outputs(c, nall, f, torque, st));
  RC(shpair_decode_device_errors(c, *c->h_err, st));
  if (eflag) *eng_vdwl += c->h_ev[0];
  if (vflag)
    for (int a = 0; a < 6; ++a) virial[a] += c->h_ev[1 + a];
  return SHPAIR_OK;
}

int shpair_get_kernel_info(shpair_ctx* c, shpair_kernel_info* out)
{
  if (!c || !out) return SHPAIR_EINVAL;
  const ContactPlan& p = c->last_plan;
  if (c->lmax < 0 || p.lds_bytes <= 0) CTX_FAIL(c, SHPAIR_ESTATE, "kernel info: no compute has run yet");
  HIPCHK(c, hipSetDevice(c->device));
  hipFuncAttributes a;
  HIPCHK(c, hipFuncGetAttributes(&a, p.compiled ? kInstance[c->lmax](p, c->last_needv) : shp_instance_Lrt(p, c->last_needv)));
  contact_kernel_info(p, a.numRegs, *out);
  out->lmax = c->lmax;
  out->scratch_bytes = (int)a.localSizeBytes;
  out->needv = c->last_needv ? 1 : 0;
  return SHPAIR_OK;
}

int shpair_fp64_peak(shpair_ctx* c, int mode, double target_ms, double* valu_tflops, double* mfma_tflops)
{
  if (!c) return SHPAIR_EINVAL;
  if (mode < 0 || mode > 2 || !(target_ms > 0.0) || target_ms > 2000.0)
    CTX_FAIL(c, SHPAIR_EINVAL, "fp64_peak: mode %d not in 0..2 or target_ms %g not in (0, 2000]", mode, target_ms);
  HIPCHK(c, hipSetDevice(c->device));
  Fp64PeakResult r;
  HIPCHK(c, fp64_peak_run(mode, target_ms, 5, &r, c->stream));
  if (valu_tflops) *valu_tflops = r.valu_tflops;
  if (mfma_tflops) *mfma_tflops = r.mfma_tflops;
  return SHPAIR_OK;
}

}  // extern "C"
