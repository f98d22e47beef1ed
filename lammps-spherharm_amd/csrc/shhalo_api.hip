// shhalo_api.hip — the C ABI of include/shhalo.h: LAMMPS' Comm::exchange / borders / forward_comm / reverse_comm
// around PairSH::compute for a device-resident host, one rank per GPU.
//
// Host side: the brick geometry and message layout (halo_plan.cpp) and the device buffers of the plan.  Per step and
// direction of travel there is ONE pack kernel, ONE grouped point-to-point exchange (ncclGroupStart .. one ncclSend +
// one ncclRecv per remote peer .. ncclGroupEnd) and ONE unpack kernel on the caller's stream: forward_rows<W> below for
// the three forward messages (7, 9 and 13 doubles per row), its exchange_rows also for the reverse one; the host waits
// only where a count must be read back (at a reneighbouring) and for the rebuild decision.
//
// Every kernel launch of the halo layer is in this translation unit.  The three transports (RCCL, rank threads around
// a hub, host-staged) are behind halo_transport.hpp; Verlet::run over all ranks is shhalo_run.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "../../include/shhalo.h"
#include "halo_kernels.hpp"
#include "shhalo_ctx.hpp"

using namespace shp;

struct shp::HaloKernelTables {
  HaloSlots ghost_slots{}, mig_slots{};
  int ghost_peer_of_slot[kHaloMaxSlots] = {};  // index into peer_rank, -1: self
  HaloMsgTables tab{};                         // of the current plan
};

namespace {

constexpr int kPinTotals = 0, kPinMsgIn = kHaloMaxSlots, kPinFlags = kHaloMaxSlots + 26 * 27, kPinInts = kPinFlags + 4;

// exclusive scan of n ints into out[0..n] (out[n] = total): the three passes of step_kernels.hpp
int scan_ints(shhalo_ctx* h, const int* in, int* out, int n, hipStream_t st)
{
  H_SP(h, shstep_exclusive_scan(h->sp, in, out, n, st));
  return SHPAIR_OK;
}

int peer_index(const shhalo_ctx* h, int rank)
{
  for (int k = 0; k < h->npeers; ++k)
    if (h->peer_rank[k] == rank) return k;
  return -1;
}

// Stable partition of the n owned rows (halo_kernels.hpp): counts per (slot, workgroup), scan, per-slot totals and the
// count messages for the remote peers.  Leaves d_start (positions) for the fill pass.
template <int MODE>
int partition_count(shhalo_ctx* h, const HaloSlots& sl, int n, const double* x, hipStream_t st)
{
  const int nb = (int)nblk(n, kHaloBlock);
  const size_t cells = (size_t)sl.nslots * nb;
  H_HIP(h, h->d_blockcnt.ensure(cells));
  H_HIP(h, h->d_start.ensure(cells + 1));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(halo_count_kernel<MODE>), dim3(nb), dim3(kHaloBlock), 0, st, n, h->hg, sl, x,
                     (const unsigned char*)h->d_cat.p, h->d_blockcnt.p, nb);
  H_HIP(h, hipGetLastError());
  H_RC(h, scan_ints(h, h->d_blockcnt.p, h->d_start.p, (int)cells, st));
  H_HIP(h, hipMemsetAsync(h->d_msg.p, 0, (size_t)26 * 27 * sizeof(int), st));
  hipLaunchKernelGGL(halo_totals_kernel, dim3(1), dim3(64), 0, st, sl, (const int*)h->d_start.p, nb, MODE, h->npeers,
                     (const int*)h->d_peer_of_slot.p, h->d_totals.p, h->d_msg.p);
  H_HIP(h, hipGetLastError());
  return SHPAIR_OK;
}

// A block of rows of `width` doubles in the buffer at `base`, as a message: the one place where a row width becomes
// an offset and a byte count.
Msg rows_msg(const HaloRowBlock& b, int width, double* base)
{
  return {b.peer, base + (size_t)b.first * width, (size_t)b.count * width * sizeof(double)};
}

// One grouped exchange of the current layout at `width` doubles per row (halo_peer_blocks of halo_plan.hpp).
int exchange_rows(shhalo_ctx* h, bool reverse, int width, double* sendbase, double* recvbase, hipStream_t st)
{
  const HaloPeerBlocks b = halo_peer_blocks(h->lay, reverse);
  std::vector<Msg> sends, recvs;
  for (int k = 0; k < b.nsend; ++k) sends.push_back(rows_msg(b.send[k], width, sendbase));
  for (int k = 0; k < b.nrecv; ++k) recvs.push_back(rows_msg(b.recv[k], width, recvbase));
  H_TR(h, h->tr->exchange(sends, recvs, st));
  return SHPAIR_OK;
}

// Comm::forward_comm at W doubles per row, the one body behind shhalo_forward_device, shhalo_forward_twist_device and
// the ghost-row leg of shhalo_borders_device: `pack` over the nsend send rows, one exchange, `unpack` over the nghost ghost
// rows, all on st.  `more`: what the message carries after x and quat, read from the owned rows and written to the ghost
// rows (the two kernels take it in the same order).  have_arrays: no pointer the kernels dereference is null.
template <int W, class PackKernel, class UnpackKernel, class... More>
int forward_rows(shhalo_ctx* h, bool have_arrays, hipStream_t st, PackKernel pack, UnpackKernel unpack, double* x, double* quat,
                 More*... more)
{
  static_assert(W <= kFwdTwistWidth, "halo_size_forward_buffers sizes d_sendbuf / d_recvbuf for kFwdTwistWidth doubles per row");
  if (h->plan_nlocal < 0) H_FAIL(h, SHPAIR_ESTATE, "forward: no plan (shhalo_borders_device first)");
  const shhalo_layout& L = h->lay;
  if (L.nsend == 0 && L.nghost == 0) return SHPAIR_OK;
  if (!have_arrays) H_FAIL(h, SHPAIR_EINVAL, "null array pointer");
  H_HIP(h, hipSetDevice(h->sp->device));
  if (L.nsend > 0) {
    hipLaunchKernelGGL(pack, dim3(nblk(L.nsend, kHaloBlock)), dim3(kHaloBlock), 0, st, L.nsend, h->kt->tab, (const int*)h->d_send_idx.p,
                       (const unsigned char*)h->d_send_code.p, (const double*)x, (const double*)quat, (const More*)more...,
                       h->d_sendbuf.p, h->d_recvbuf.p);
    H_HIP(h, hipGetLastError());
  }
  if (const int rc = exchange_rows(h, false, W, h->d_sendbuf.p, h->d_recvbuf.p, st)) return rc;
  if (L.nghost > 0) {
    hipLaunchKernelGGL(unpack, dim3(nblk(L.nghost, kHaloBlock)), dim3(kHaloBlock), 0, st, L.nghost, h->plan_nlocal,
                       (const double*)h->d_recvbuf.p, x, quat, more...);
    H_HIP(h, hipGetLastError());
  }
  return SHPAIR_OK;
}

// the 27-int count vectors travel to / from every remote peer; then totals, the peers' vectors and the error flags
// come to the host in one go
int exchange_counts(shhalo_ctx* h, int nslots, hipStream_t st)
{
  std::vector<Msg> sends, recvs;
  for (int k = 0; k < h->npeers; ++k) {
    sends.push_back({h->peer_rank[k], h->d_msg.p + 27 * k, 27 * sizeof(int)});
    recvs.push_back({h->peer_rank[k], h->d_msgin.p + 27 * k, 27 * sizeof(int)});
  }
  H_TR(h, h->tr->exchange(sends, recvs, st));
  H_HIP(h, hipMemcpyAsync(h->h_ints + kPinTotals, h->d_totals.p, nslots * sizeof(int), hipMemcpyDeviceToHost, st));
  if (h->npeers)
    H_HIP(h, hipMemcpyAsync(h->h_ints + kPinMsgIn, h->d_msgin.p, (size_t)h->npeers * 27 * sizeof(int), hipMemcpyDeviceToHost, st));
  H_HIP(h, hipMemcpyAsync(h->h_ints + kPinFlags, h->d_flags.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  H_HIP(h, hipStreamSynchronize(st));
  return SHPAIR_OK;
}

}  // namespace

namespace shp {

// The decision to fail is COLLECTIVE wherever a rank-local condition (a lost atom, a capacity that is too small, an
// index outside a table) is found between two exchanges: a rank that simply returned would leave its peers inside
// ncclRecv for rows that are never sent — RCCL has no timeout.  Every rank contributes its code (0 or -SHPAIR_E*) to
// one max-all-reduce and all of them return an error if any did: the failing rank its own code and message, the
// others SHPAIR_ESTATE naming the code.  One rank: nothing to agree on.
int halo_agree(shhalo_ctx* h, int local_rc, hipStream_t st)
{
  if (h->tr->size() <= 1) return local_rc;
  const std::string mine = h->err;
  h->h_ints[kPinFlags + 3] = local_rc ? -local_rc : 0;
  H_HIP(h, hipMemcpyAsync(h->d_flags.p + 3, h->h_ints + kPinFlags + 3, sizeof(int), hipMemcpyHostToDevice, st));
  H_TR(h, h->tr->allreduce_max_i32(h->d_flags.p + 3, 1, st));
  H_HIP(h, hipMemcpyAsync(h->h_ints + kPinFlags + 3, h->d_flags.p + 3, sizeof(int), hipMemcpyDeviceToHost, st));
  H_HIP(h, hipStreamSynchronize(st));
  if (local_rc) {
    h->err = mine;
    return local_rc;
  }
  const int worst = h->h_ints[kPinFlags + 3];
  if (worst > 0)
    H_FAIL(h, SHPAIR_ESTATE, "rank %d stops because another rank failed (%s); its own state was consistent", h->geo.rank,
           shpair_strerror(-worst));
  return SHPAIR_OK;
}

// The send / receive buffers of the forward exchanges of the current layout, for the widest message (the border
// message is 9 doubles per row, the forward message with twists 13): at every borders and before the first step of
// shhalo_run_device, so that nothing is allocated inside a step whichever width the exchange then has.
int halo_size_forward_buffers(shhalo_ctx* h)
{
  static_assert(kFwdTwistWidth >= kBorderWidth && kFwdTwistWidth >= kFwdWidth, "the widest forward message sizes the buffers");
  const shhalo_layout& L = h->lay;
  H_HIP(h, h->d_sendbuf.ensure((size_t)(L.nsend > 0 ? L.nsend : 1) * kFwdTwistWidth));
  H_HIP(h, h->d_recvbuf.ensure((size_t)(L.nghost > 0 ? L.nghost : 1) * kFwdTwistWidth));
  return SHPAIR_OK;
}

int halo_check_arrays(shhalo_ctx* h, const shhalo_arrays* a)
{
  if (!a) H_FAIL(h, SHPAIR_EINVAL, "null arrays");
  if (a->nlocal < 0 || a->nmax < a->nlocal) H_FAIL(h, SHPAIR_EINVAL, "bad nlocal (%d) / nmax (%d)", a->nlocal, a->nmax);
  if (a->nmax > 0 && (!a->x || !a->v || !a->quat || !a->angmom || !a->f || !a->torque || !a->type || !a->shtype || !a->mask || !a->tag))
    H_FAIL(h, SHPAIR_EINVAL, "null array pointer");
  return SHPAIR_OK;
}

}  // namespace shp

namespace {

int finish_create(shhalo_ctx* h, shpair_ctx* sp, int rank, const int grid[3], const double lo[3], const double hi[3],
                  const int periodic[3], double skin)
{
  if (!(skin >= 0.0) || !std::isfinite(skin)) H_FAIL(h, SHPAIR_EINVAL, "skin %g must be finite and >= 0", skin);
  double rm = 0.0;
  for (int k = 0; k < sp->nshapes; ++k) {
    if (sp->shapes[k].lmax < 0) H_FAIL(h, SHPAIR_ESTATE, "shape %d is not set (the ghost cutoff needs every bounding radius)", k);
    rm = std::fmax(rm, sp->shapes[k].rmax);
  }
  if (!(rm > 0.0)) H_FAIL(h, SHPAIR_ESTATE, "shapes are not set");
  h->sp = sp;
  h->skin = skin;
  const double cut = 2.0 * rm + skin;
  if (shhalo_plan_geometry(grid, lo, hi, periodic, cut, rank, &h->geo))
    H_FAIL(h, SHPAIR_EINVAL, "grid %dx%dx%d does not fit the box: a decomposed brick edge is shorter than the ghost cutoff %g, an "
           "undecomposed periodic edge shorter than twice that, or the arguments are not finite", grid[0], grid[1], grid[2], cut);
  if (h->geo.nranks != h->tr->size())
    H_FAIL(h, SHPAIR_EINVAL, "grid %dx%dx%d has %d bricks but the transport has %d ranks", grid[0], grid[1], grid[2], h->geo.nranks,
           h->tr->size());
  h->hg = halo_geom_of(h->geo);
  // remote peers, ascending
  std::vector<int> pr;
  for (int c = 0; c < 27; ++c)
    if (h->geo.peer[c] >= 0 && h->geo.peer[c] != rank) pr.push_back(h->geo.peer[c]);
  std::sort(pr.begin(), pr.end());
  pr.erase(std::unique(pr.begin(), pr.end()), pr.end());
  h->npeers = (int)pr.size();
  for (int k = 0; k < h->npeers; ++k) h->peer_rank[k] = pr[k];
  // ghost slots: directions with a peer, by (peer, code) — the order of shhalo_plan_layout
  std::vector<int> dirs;
  for (int c = 0; c < 27; ++c)
    if (c != 13 && h->geo.peer[c] >= 0) dirs.push_back(c);
  std::sort(dirs.begin(), dirs.end(), [&](int a, int b) {
    return h->geo.peer[a] != h->geo.peer[b] ? h->geo.peer[a] < h->geo.peer[b] : a < b;
  });
  h->kt->ghost_slots.nslots = (int)dirs.size();
  for (int s = 0; s < (int)dirs.size(); ++s) {
    h->kt->ghost_slots.code_of_slot[s] = dirs[s];
    h->kt->ghost_peer_of_slot[s] = peer_index(h, h->geo.peer[dirs[s]]);
  }
  // migration categories: 0 stays (also where the direction wraps onto this rank), 1 + k goes to remote peer k
  h->kt->mig_slots.nslots = 1 + h->npeers;
  for (int c = 0; c < 27; ++c) {
    const int p = h->geo.peer[c];
    h->kt->mig_slots.cat_of_code[c] = (c == 13 || p < 0 || p == rank) ? 0 : 1 + peer_index(h, p);
  }
  H_HIP(h, hipSetDevice(sp->device));
  H_HIP(h, h->d_totals.ensure(kHaloMaxSlots));
  H_HIP(h, h->d_msg.ensure(26 * 27));
  H_HIP(h, h->d_msgin.ensure(26 * 27));
  H_HIP(h, h->d_flags.ensure(4));
  H_HIP(h, h->d_peer_of_slot.ensure(kHaloMaxSlots));
  H_HIP(h, hipMemset(h->d_flags.p, 0, 4 * sizeof(int)));
  H_HIP(h, hipMemset(h->d_msgin.p, 0, 26 * 27 * sizeof(int)));
  H_HIP(h, hipMemcpy(h->d_peer_of_slot.p, h->kt->ghost_peer_of_slot, kHaloMaxSlots * sizeof(int), hipMemcpyHostToDevice));
  H_HIP(h, h->h_ints.resize(kPinInts));
  // Neighbor::build of this rank bins its brick plus the ghost shell: a non-periodic box (the periodic images
  // are ghost rows like any other here)
  double blo[3], bhi[3];
  const int nonper[3] = {0, 0, 0};
  for (int d = 0; d < 3; ++d) {
    blo[d] = h->geo.blo[d] - cut;
    bhi[d] = h->geo.bhi[d] + cut;
  }
  H_SP(h, shstep_set_box(sp, blo, bhi, nonper, skin));
  h->stats.nranks_transport = h->tr->size();
  h->stats.transport = h->tr->kind();
  h->stats.rccl_version = h->tr->version();
  return SHPAIR_OK;
}

HaloArrays dev_arrays(const shhalo_arrays* a)
{
  HaloArrays d;
  d.x = a->x; d.v = a->v; d.quat = a->quat; d.angmom = a->angmom;
  d.type = a->type; d.shtype = a->shtype; d.mask = a->mask; d.tag = a->tag;
  return d;
}

// The common tail of the three creation functions: trc and t are what the transport's factory gave (its message is in
// sp->err; the context owns t from here on).
int create_ctx(shhalo_ctx** out, shpair_ctx* sp, int trc, Transport* t, int rank, const int grid[3], const double lo[3],
               const double hi[3], const int periodic[3], double skin)
{
  if (trc) return trc;
  shhalo_ctx* h = new (std::nothrow) shhalo_ctx();
  if (h) h->kt = new (std::nothrow) HaloKernelTables();
  if (!h || !h->kt) {
    delete h;
    delete t;
    return SHPAIR_ENOMEM;
  }
  h->tr = t;
  const int rc = finish_create(h, sp, rank, grid, lo, hi, periodic, skin);
  if (rc) {
    sp->err = h->err;
    shhalo_destroy(h);
    return rc;
  }
  *out = h;
  return SHPAIR_OK;
}

}  // namespace

extern "C" {

int shhalo_create_rccl(shhalo_ctx** out, shpair_ctx* sp, const unsigned char id[SHHALO_UNIQUE_ID_BYTES], int rank, int nranks,
                       const int grid[3], const double lo[3], const double hi[3], const int periodic[3], double skin)
{
  if (!out) return SHPAIR_EINVAL;
  *out = nullptr;
  if (!sp || !id || !grid || !lo || !hi || !periodic || rank < 0 || rank >= nranks) return SHPAIR_EINVAL;
  if (hipSetDevice(sp->device) != hipSuccess) CTX_FAIL(sp, SHPAIR_EHIP, "hipSetDevice(%d) failed", sp->device);
  Transport* t = nullptr;
  const int trc = make_rccl_transport(&t, &sp->err, id, rank, nranks);
  return create_ctx(out, sp, trc, t, rank, grid, lo, hi, periodic, skin);
}

int shhalo_create_staged(shhalo_ctx** out, shpair_ctx* sp, shhalo_exchange_fn exchange, shhalo_allreduce_fn allreduce, void* user,
                         int rank, int nranks, const int grid[3], const double lo[3], const double hi[3], const int periodic[3],
                         double skin)
{
  if (!out) return SHPAIR_EINVAL;
  *out = nullptr;
  if (!sp || !grid || !lo || !hi || !periodic || rank < 0 || rank >= nranks) return SHPAIR_EINVAL;
  Transport* t = nullptr;
  const int trc = make_staged_transport(&t, &sp->err, exchange, allreduce, user, rank, nranks);
  if (!trc && hipSetDevice(sp->device) != hipSuccess) {
    delete t;
    CTX_FAIL(sp, SHPAIR_EHIP, "hipSetDevice(%d) failed", sp->device);
  }
  return create_ctx(out, sp, trc, t, rank, grid, lo, hi, periodic, skin);
}

int shhalo_create_local(shhalo_ctx** out, shpair_ctx* sp, shhalo_hub* hub, int rank, int nranks, const int grid[3],
                        const double lo[3], const double hi[3], const int periodic[3], double skin)
{
  if (!out) return SHPAIR_EINVAL;
  *out = nullptr;
  if (!sp || !grid || !lo || !hi || !periodic || rank < 0 || rank >= nranks) return SHPAIR_EINVAL;
  Transport* t = nullptr;
  const int trc = make_local_transport(&t, &sp->err, hub, rank, nranks);
  return create_ctx(out, sp, trc, t, rank, grid, lo, hi, periodic, skin);
}

void shhalo_destroy(shhalo_ctx* h)
{
  if (!h) return;
  if (h->sp) (void)hipSetDevice(h->sp->device);
  (void)hipDeviceSynchronize();
  delete h->tr;
  delete h->kt;
  if (h->ev_ready) (void)hipEventDestroy(h->ev_ready);
  if (h->ev_ghosts) (void)hipEventDestroy(h->ev_ghosts);
  if (h->ev_bdone) (void)hipEventDestroy(h->ev_bdone);
  if (h->ev_rev) (void)hipEventDestroy(h->ev_rev);
  for (hipStream_t s2 : h->st2x)
    if (s2) (void)hipStreamDestroy(s2);
  delete h;   // its buffers go with it
}

const char* shhalo_last_error(const shhalo_ctx* h) { return h ? h->err.c_str() : "null context"; }

int shhalo_get_geometry(const shhalo_ctx* h, shhalo_geometry* out)
{
  if (!h || !out) return SHPAIR_EINVAL;
  *out = h->geo;
  return SHPAIR_OK;
}

int shhalo_get_stats(const shhalo_ctx* h, shhalo_stats* out)
{
  if (!h || !out) return SHPAIR_EINVAL;
  *out = h->stats;
  // the width the forward exchange of the current settings sends (the plan keeps the 7-wide figure)
  if (halo_forward_is_wide(h)) out->forward_bytes_per_step = h->stats.forward_bytes_per_step / kFwdWidth * kFwdTwistWidth;
  return SHPAIR_OK;
}

int shhalo_exchange_device(shhalo_ctx* h, shhalo_arrays* a, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  H_RC(h, halo_check_arrays(h, a));
  H_HIP(h, hipSetDevice(h->sp->device));
  hipStream_t st = (hipStream_t)stream;
  const int n = a->nlocal;
  h->plan_nlocal = -1;  // the send lists refer to the old rows
  H_HIP(h, h->d_cat.ensure((size_t)(n > 0 ? n : 1)));
  if (n > 0) {
    hipLaunchKernelGGL(halo_wrap_dest_kernel, dim3(nblk(n, kHaloBlock)), dim3(kHaloBlock), 0, st, n, h->hg, h->kt->mig_slots, a->x,
                       h->d_cat.p, h->d_flags.p);
    H_HIP(h, hipGetLastError());
  }
  H_RC(h, partition_count<1>(h, h->kt->mig_slots, n, a->x, st));
  H_RC(h, exchange_counts(h, h->kt->mig_slots.nslots, st));
  const int* tot = h->h_ints + kPinTotals;
  const int nstay = tot[0];
  int nleave = 0, narr = 0;
  for (int k = 0; k < h->npeers; ++k) {
    nleave += tot[1 + k];
    narr += h->h_ints[kPinMsgIn + 27 * k];
  }
  // rank-local failures, decided by all ranks together BEFORE the rows travel (halo_agree() above)
  int local_rc = SHPAIR_OK;
  char why[320] = "";
  if (h->h_ints[kPinFlags] & kHaloErrLost) {
    H_HIP(h, hipMemsetAsync(h->d_flags.p, 0, sizeof(int), st));
    local_rc = SHPAIR_ESTATE;
    snprintf(why, sizeof(why), "rank %d: an owned atom left its brick and the 26 neighbouring bricks since the last exchange "
             "(lost atom: the timestep or the skin is too large)", h->geo.rank);
  } else if (nstay + nleave != n) {
    local_rc = SHPAIR_EHIP;
    snprintf(why, sizeof(why), "internal: partition of %d rows gave %d + %d", n, nstay, nleave);
  } else if ((long long)nstay + narr > a->nmax) {
    local_rc = SHPAIR_ENOMEM;
    snprintf(why, sizeof(why), "rank %d: %d owned atoms after migration exceed the capacity nmax = %d", h->geo.rank,
             nstay + narr, a->nmax);
  }
  h->err = why;
  H_RC(h, halo_agree(h, local_rc, st));
  if (nleave == 0 && narr == 0) return SHPAIR_OK;
  const HaloArrays da = dev_arrays(a);
  std::vector<Msg> sends, recvs;
  if (nleave > 0) {
    const int nb = (int)nblk(n, kHaloBlock);
    H_HIP(h, h->d_order.ensure((size_t)n));
    H_HIP(h, h->d_migrows.ensure((size_t)n * kMigWidth));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(halo_fill_kernel<1>), dim3(nb), dim3(kHaloBlock), 0, st, n, h->hg, h->kt->mig_slots,
                       (const double*)a->x, (const unsigned char*)h->d_cat.p, (const int*)h->d_start.p, nb, h->d_order.p,
                       (unsigned char*)nullptr);
    hipLaunchKernelGGL(halo_mig_gather_kernel, dim3(nb), dim3(kHaloBlock), 0, st, n, (const int*)h->d_order.p, da, h->d_migrows.p);
    if (nstay > 0)
      hipLaunchKernelGGL(halo_mig_scatter_kernel, dim3(nblk(nstay, kHaloBlock)), dim3(kHaloBlock), 0, st, nstay, 0,
                         (const double*)h->d_migrows.p, da);
    H_HIP(h, hipGetLastError());
    int off = nstay;
    for (int k = 0; k < h->npeers; ++k) {
      if (tot[1 + k] > 0) sends.push_back(rows_msg({h->peer_rank[k], off, tot[1 + k]}, kMigWidth, h->d_migrows.p));
      off += tot[1 + k];
    }
  }
  if (narr > 0) {
    H_HIP(h, h->d_migin.ensure((size_t)narr * kMigWidth));
    int off = 0;
    for (int k = 0; k < h->npeers; ++k) {
      const int c = h->h_ints[kPinMsgIn + 27 * k];
      if (c > 0) recvs.push_back(rows_msg({h->peer_rank[k], off, c}, kMigWidth, h->d_migin.p));
      off += c;
    }
  }
  H_TR(h, h->tr->exchange(sends, recvs, st));
  if (narr > 0) {
    hipLaunchKernelGGL(halo_mig_scatter_kernel, dim3(nblk(narr, kHaloBlock)), dim3(kHaloBlock), 0, st, narr, nstay,
                       (const double*)h->d_migin.p, da);
    H_HIP(h, hipGetLastError());
  }
  a->nlocal = nstay + narr;
  h->stats.migrated_out += nleave;
  h->stats.migrated_in += narr;
  return SHPAIR_OK;
}

int shhalo_borders_device(shhalo_ctx* h, const shhalo_arrays* a, int* nghost, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  if (nghost) *nghost = 0;
  H_RC(h, halo_check_arrays(h, a));
  if (!nghost) H_FAIL(h, SHPAIR_EINVAL, "null nghost");
  H_HIP(h, hipSetDevice(h->sp->device));
  hipStream_t st = (hipStream_t)stream;
  const int n = a->nlocal;
  h->plan_nlocal = -1;
  h->nghost = 0;
  H_HIP(h, h->d_cat.ensure(1));
  H_RC(h, partition_count<0>(h, h->kt->ghost_slots, n, a->x, st));
  H_RC(h, exchange_counts(h, h->kt->ghost_slots.nslots, st));
  int send_cnt[27] = {0}, recv_cnt[27] = {0};
  for (int s = 0; s < h->kt->ghost_slots.nslots; ++s) send_cnt[h->kt->ghost_slots.code_of_slot[s]] = h->h_ints[kPinTotals + s];
  for (int c = 0; c < 27; ++c) {
    const int p = h->geo.peer[c];
    if (c == 13 || p < 0) continue;
    // what arrives through my direction c was sent with the sender's code 26 - c
    recv_cnt[c] = (p == h->geo.rank) ? send_cnt[26 - c] : h->h_ints[kPinMsgIn + 27 * peer_index(h, p) + (26 - c)];
  }
  if (shhalo_plan_layout(&h->geo, send_cnt, recv_cnt, &h->lay)) H_FAIL(h, SHPAIR_EINVAL, "internal: message layout");
  const shhalo_layout& L = h->lay;
  *nghost = L.nghost;
  {
    int local_rc = SHPAIR_OK;
    char why[256] = "";
    if ((long long)n + L.nghost > a->nmax) {
      local_rc = SHPAIR_ENOMEM;
      snprintf(why, sizeof(why), "rank %d: %d owned + %d ghost rows exceed the capacity nmax = %d", h->geo.rank, n, L.nghost,
               a->nmax);
    }
    h->err = why;
    H_RC(h, halo_agree(h, local_rc, st));   // before the ghost rows travel: every rank returns, or none
  }
  H_HIP(h, h->d_send_idx.ensure((size_t)(L.nsend > 0 ? L.nsend : 1)));
  H_HIP(h, h->d_send_code.ensure((size_t)(L.nsend > 0 ? L.nsend : 1)));
  H_RC(h, halo_size_forward_buffers(h));   // for the widest forward message (13 doubles per row, with twists)
  H_HIP(h, h->d_rsend.ensure((size_t)(L.nghost > 0 ? L.nghost : 1) * kRevWidth));
  H_HIP(h, h->d_rrecv.ensure((size_t)(L.nsend > 0 ? L.nsend : 1) * kRevWidth));
  for (int c = 0; c < 27; ++c) {
    for (int d = 0; d < 3; ++d) h->kt->tab.shift[c][d] = h->geo.shift[c][d];
    h->kt->tab.self[c] = (h->geo.peer[c] == h->geo.rank) ? 1 : 0;
    h->kt->tab.send_off[c] = L.send_off[c];
    h->kt->tab.recv_off[c] = L.recv_off[c];
    h->kt->tab.recv_cnt[c] = L.recv_cnt[c];
  }
  if (n > 0 && L.nsend > 0) {
    const int nb = (int)nblk(n, kHaloBlock);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(halo_fill_kernel<0>), dim3(nb), dim3(kHaloBlock), 0, st, n, h->hg, h->kt->ghost_slots,
                       (const double*)a->x, (const unsigned char*)nullptr, (const int*)h->d_start.p, nb, h->d_send_idx.p,
                       h->d_send_code.p);
    H_HIP(h, hipGetLastError());
  }
  h->plan_nlocal = n;
  h->nghost = L.nghost;
  h->stats.npeers = L.npeers;
  h->stats.nsend_rows = L.nsend;
  h->stats.nghost_rows = L.nghost;
  long long fb = 0, rb = 0;
  for (int k = 0; k < L.npeers; ++k) {
    fb += (long long)L.peer_send_cnt[k] * kFwdWidth * 8;
    rb += (long long)L.peer_recv_cnt[k] * kRevWidth * 8;
  }
  h->stats.forward_bytes_per_step = fb;
  h->stats.reverse_bytes_per_step = rb;
  ++h->stats.rebuilds;
  // the ghost rows: positions, orientations and the per-atom constants in one wider message
  return forward_rows<kBorderWidth>(h, true /* halo_check_arrays */, st, halo_pack_kernel<kBorderWidth>,
                                    halo_unpack_kernel<kBorderWidth>, a->x, a->quat, a->tag, a->type, a->shtype);
}

// Neighbor::build over the brick plus its ghost shell.  The list build reports shape indices outside the table (they
// may have arrived with migrated atoms or ghost rows): a rank-local failure between two exchanges, so the ranks agree
// on it before anyone posts the forward exchange.
int shhalo_neighbor_build_device(shhalo_ctx* h, const shhalo_arrays* a, int nghost, int* npairs, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  H_RC(h, halo_check_arrays(h, a));
  if (!npairs || nghost < 0) H_FAIL(h, SHPAIR_EINVAL, "null npairs or negative nghost");
  H_HIP(h, hipSetDevice(h->sp->device));
  hipStream_t st = (hipStream_t)stream;
  const int lrc = shstep_neighbor_build_device(h->sp, a->nlocal, nghost, a->x, a->shtype, a->tag, npairs, st);
  if (lrc) h->err = h->sp->err;
  else h->err.clear();
  return halo_agree(h, lrc, st);
}

int shhalo_forward_device(shhalo_ctx* h, double* x, double* quat, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  return forward_rows<kFwdWidth>(h, x && quat, (hipStream_t)stream, halo_pack_kernel<kFwdWidth>, halo_unpack_kernel<kFwdWidth>, x, quat,
                                 (int*)nullptr, (int*)nullptr, (int*)nullptr);   // no tag, type, shtype in this message
}

int shhalo_forward_twist_device(shhalo_ctx* h, double* x, double* quat, double* twist, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  return forward_rows<kFwdTwistWidth>(h, x && quat && twist, (hipStream_t)stream, halo_pack_twists_kernel, halo_unpack_twists_kernel, x,
                                      quat, twist);
}

int shhalo_reverse_device(shhalo_ctx* h, double* f, double* torque, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  if (h->plan_nlocal < 0) H_FAIL(h, SHPAIR_ESTATE, "reverse: no plan (shhalo_borders_device first)");
  const shhalo_layout& L = h->lay;
  if (L.nsend == 0 && L.nghost == 0) return SHPAIR_OK;
  if (!f || !torque) H_FAIL(h, SHPAIR_EINVAL, "null array pointer");
  H_HIP(h, hipSetDevice(h->sp->device));
  hipStream_t st = (hipStream_t)stream;
  if (L.nghost > 0) {
    hipLaunchKernelGGL(halo_rpack_kernel, dim3(nblk(L.nghost, kHaloBlock)), dim3(kHaloBlock), 0, st, L.nghost, h->plan_nlocal, h->kt->tab,
                       (const double*)f, (const double*)torque, h->d_rsend.p, h->d_rrecv.p);
    H_HIP(h, hipGetLastError());
  }
  // what came in through the forward exchange goes back to where it came from
  if (const int rc = exchange_rows(h, true, kRevWidth, h->d_rsend.p, h->d_rrecv.p, st)) return rc;
  if (L.nsend > 0) {
    if (h->sp->opt_deterministic) {
      // bitwise reproducible sums: one launch per direction (unique owners inside a block, plain adds), in code order
      for (int c = 0; c < 27; ++c)
        if (L.send_cnt[c] > 0)
          hipLaunchKernelGGL(halo_runpack_block_kernel, dim3(nblk(L.send_cnt[c], kHaloBlock)), dim3(kHaloBlock), 0, st,
                             L.send_cnt[c], L.send_off[c], (const int*)h->d_send_idx.p, (const double*)h->d_rrecv.p, f, torque);
    } else {
      hipLaunchKernelGGL(halo_runpack_kernel, dim3(nblk(L.nsend, kHaloBlock)), dim3(kHaloBlock), 0, st, L.nsend,
                         (const int*)h->d_send_idx.p, (const double*)h->d_rrecv.p, f, torque);
    }
    H_HIP(h, hipGetLastError());
  }
  return SHPAIR_OK;
}

int shhalo_check_rebuild_device(shhalo_ctx* h, int nlocal, const double* x, int* rebuild, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  if (!rebuild) H_FAIL(h, SHPAIR_EINVAL, "null rebuild pointer");
  H_HIP(h, hipSetDevice(h->sp->device));
  hipStream_t st = (hipStream_t)stream;
  int* flag = nullptr;
  int forced = 0;
  H_SP(h, shstep_enqueue_check(h->sp, nlocal, x, &flag, &forced, st));
  hipLaunchKernelGGL(halo_flag_merge_kernel, dim3(1), dim3(64), 0, st, (const int*)flag, h->d_flags.p + 2);
  H_HIP(h, hipGetLastError());
  if (forced) H_HIP(h, hipMemsetAsync(h->d_flags.p + 2, 0xff, 1, st));  // low byte set: > 0
  H_TR(h, h->tr->allreduce_max_i32(h->d_flags.p + 2, 1, st));
  H_HIP(h, hipMemcpyAsync(h->h_ints + kPinFlags + 2, h->d_flags.p + 2, sizeof(int), hipMemcpyDeviceToHost, st));
  H_HIP(h, hipStreamSynchronize(st));
  *rebuild = h->h_ints[kPinFlags + 2] > 0 ? 1 : 0;
  return SHPAIR_OK;
}

int shhalo_allreduce_sum_device(shhalo_ctx* h, double* data, int n, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  if (n < 0 || (n > 0 && !data)) H_FAIL(h, SHPAIR_EINVAL, "bad all-reduce arguments");
  if (n == 0) return SHPAIR_OK;
  H_HIP(h, hipSetDevice(h->sp->device));
  H_TR(h, h->tr->allreduce_sum_f64(data, n, (hipStream_t)stream));
  return SHPAIR_OK;
}

int shhalo_transport_selftest(shhalo_ctx* h, int nbytes, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  if (nbytes <= 0 || nbytes > (1 << 28)) H_FAIL(h, SHPAIR_EINVAL, "self-test size %d", nbytes);
  H_HIP(h, hipSetDevice(h->sp->device));
  hipStream_t st = (hipStream_t)stream;
  DevBuf<unsigned char> src, dst;
  DevBuf<double> red;
  DevBuf<int> redi;
  H_HIP(h, src.ensure((size_t)nbytes));
  H_HIP(h, dst.ensure((size_t)nbytes));
  H_HIP(h, red.ensure(3));
  H_HIP(h, redi.ensure(2));
  std::vector<unsigned char> pat((size_t)nbytes), back((size_t)nbytes, 0);
  for (int k = 0; k < nbytes; ++k) pat[k] = (unsigned char)((k * 131 + 7 + 17 * h->geo.rank) & 0xff);
  H_HIP(h, hipMemcpyAsync(src.p, pat.data(), (size_t)nbytes, hipMemcpyHostToDevice, st));
  H_HIP(h, hipMemsetAsync(dst.p, 0, (size_t)nbytes, st));
  const int me = h->geo.rank;
  std::vector<Msg> sends{{me, src.p, (size_t)nbytes}}, recvs{{me, dst.p, (size_t)nbytes}};
  // (the host-staged transport's caller may not be able to send to itself — gloo cannot — and a hub-less local transport
  // has nobody to talk to: there only the all-reduce is exercised)
  const bool p2p = h->tr->kind() == 1 || (h->tr->kind() == 0 && h->tr->size() > 1);
  if (p2p) {
    H_TR(h, h->tr->exchange(sends, recvs, st));
    H_HIP(h, hipMemcpyAsync(back.data(), dst.p, (size_t)nbytes, hipMemcpyDeviceToHost, st));
  } else {
    back = pat;
  }
  const int n = h->tr->size();
  const double dv[3] = {1.0, 0.5 * (me + 1), -2.0};
  const int iv[2] = {me + 1, -me};
  H_HIP(h, hipMemcpyAsync(red.p, dv, sizeof(dv), hipMemcpyHostToDevice, st));
  H_HIP(h, hipMemcpyAsync(redi.p, iv, sizeof(iv), hipMemcpyHostToDevice, st));
  H_TR(h, h->tr->allreduce_sum_f64(red.p, 3, st));
  H_TR(h, h->tr->allreduce_max_i32(redi.p, 2, st));
  double dr[3];
  int ir[2];
  H_HIP(h, hipMemcpyAsync(dr, red.p, sizeof(dr), hipMemcpyDeviceToHost, st));
  H_HIP(h, hipMemcpyAsync(ir, redi.p, sizeof(ir), hipMemcpyDeviceToHost, st));
  H_HIP(h, hipStreamSynchronize(st));
  for (int k = 0; k < nbytes; ++k)
    if (back[k] != pat[k]) H_FAIL(h, SHPAIR_ESTATE, "transport self-test: byte %d came back as %d, sent %d", k, (int)back[k], (int)pat[k]);
  if (dr[0] != (double)n || dr[1] != 0.25 * n * (n + 1) || dr[2] != -2.0 * n || ir[0] != n || ir[1] != 0)
    H_FAIL(h, SHPAIR_ESTATE, "transport self-test: all-reduce over %d rank(s) gave sum (%g, %g, %g), max (%d, %d)", n, dr[0], dr[1], dr[2],
           ir[0], ir[1]);
  return SHPAIR_OK;
}

}  // extern "C"
