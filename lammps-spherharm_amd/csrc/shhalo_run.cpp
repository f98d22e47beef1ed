// shhalo_run.cpp — shhalo_run_device of include/shhalo.h: Verlet::run over all ranks.  One step is
//   1 first half kick, 2 rebuild decision, 3 forward exchange, 4 clear forces, 5 pair forces, 6 reverse exchange,
//   7 walls, 8 gravity and drag, 9 second half kick
// where 1 and 7-9 are the step body shared with the single-rank loop (step_body.hpp) and 3, 5, 6 may run beside each
// other on two streams (option "halo_overlap").  With option "halo_twists" and a damping coefficient set (SPEC §2.10)
// two more, both halves of the step body as well: 2b the twists of the OWNED rows, ahead of the forward exchange, which
// carries them to the ghost rows (13 doubles per row instead of 7) while a gamma_ij is set; 5b the pair damping pass
// over owned + ghost rows, ahead of the reverse exchange.  Host code only: the kernels are launched by the entry points of
// shhalo_api.hip, shstep_api.hip and shpair_api.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/shhalo.h"
#include "../../include/shstep.h"
#include "shhalo_ctx.hpp"
#include "shstep_state.hpp"
#include "step_body.hpp"

using namespace shp;

namespace {

// "halo_overlap": the exchange stream.  Two kinds, made on first use, chosen per call by "halo_stream_priority":
//  [0] an ordinary non-blocking stream.  HIP maps a process's streams round robin onto a few hardware queues, and one
//      created as the fifth or later of the process (torch's, the context's two, RCCL's own come first) shares a queue
//      with one of them — if that is the compute stream the exchange runs behind the pair kernels it is meant to run
//      beside (measured for the host-pointer path's upload stream: +0.11 ms per call when it shared,
//      tools/host_path_probe.py);
//  [1] a stream at the highest stream priority: a priority level of its own is a queue of its own, and the pack /
//      RCCL / unpack kernels — a few workgroups, latency-critical — are dispatched ahead of the pair kernels' backlog.
//  Which is better between GPUs is unmeasured here (one GPU per box).  In the rehearsal of 8 rank threads on ONE GPU
//  [1] costs 5 % (26.0 against 24.8 ms per timestep; [0]: 24.5 against 24.6 without overlap,
//  profiles/r05_g_local8_priority.txt) — there every rank's high-priority kernels pre-empt every other rank's pair
//  kernels — so [0] is the default and bench.py --gpus N times both in the run itself.
// Also makes the four events of the overlap schedule.
int overlap_stream(shhalo_ctx* h, hipStream_t* out)
{
  const int kind = h->sp->opt_halo_prio ? 1 : 0;
  if (!h->st2x[kind]) {
    if (kind == 1) {
      int prio_least = 0, prio_greatest = 0;
      if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) {
        (void)hipGetLastError();
        prio_least = prio_greatest = 0;
      }
      if (hipStreamCreateWithPriority(&h->st2x[1], hipStreamNonBlocking, prio_greatest) != hipSuccess) {
        (void)hipGetLastError();
        h->st2x[1] = nullptr;
      }
    }
    if (!h->st2x[kind]) H_HIP(h, hipStreamCreateWithFlags(&h->st2x[kind], hipStreamNonBlocking));
  }
  if (!h->ev2) {
    H_HIP(h, hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming));
    H_HIP(h, hipEventCreateWithFlags(&h->ev_ghosts, hipEventDisableTiming));
    H_HIP(h, hipEventCreateWithFlags(&h->ev_bdone, hipEventDisableTiming));
    H_HIP(h, hipEventCreateWithFlags(&h->ev_rev, hipEventDisableTiming));
    h->ev2 = true;
  }
  *out = h->st2x[kind];
  return SHPAIR_OK;
}

// Pair-kernel time: one event pair around EACH slot range of a step — up to three with "halo_overlap" — so that the
// waits for the exchange's events between the ranges are not counted as kernel time (bounded pool; beyond it the
// steps are not timed).
struct StepTimers {
  static constexpr int kEvPerStep = 6, kMaxSteps = 2048;
  int ntimed = 0;
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> ev;
  std::vector<unsigned char> used;

  int create(shhalo_ctx* h, int nsteps, hipStream_t stream)
  {
    ntimed = nsteps < kMaxSteps ? nsteps : kMaxSteps;
    st = stream;
    ev.assign((size_t)kEvPerStep * ntimed, nullptr);
    used.assign((size_t)(kEvPerStep / 2) * ntimed, 0);
    for (auto& e : ev) H_HIP(h, hipEventCreate(&e));
    return SHPAIR_OK;
  }
  // range k (0, 1, 2) of `step`: record before (end = 0) / after (end = 1) on the caller's stream
  void tick(int step, int k, int end)
  {
    if (step >= ntimed) return;
    (void)hipEventRecord(ev[(size_t)kEvPerStep * step + 2 * k + end], st);
    if (end) used[(size_t)(kEvPerStep / 2) * step + k] = 1;
  }
  double sum_ms() const   // the stream must be idle
  {
    double sum = 0.0;
    for (size_t r = 0; r < used.size(); ++r) {
      float ms = 0.f;
      if (used[r] && hipEventElapsedTime(&ms, ev[2 * r], ev[2 * r + 1]) == hipSuccess) sum += ms;
    }
    return sum;
  }
  void destroy()
  {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    ev.clear();
  }
};

struct Run {
  shhalo_ctx* h;
  shhalo_arrays* a;
  const shhalo_run_params* p;
  hipStream_t st;    // the caller's
  hipStream_t st2;   // the exchange stream of "halo_overlap", or null
  StepTimers tm;
  int nghost, nreb;
  bool twists; // "halo_twists" and a dissipation coefficient set: the twists of the owned rows are computed every step
  bool wide;   // ... a pair coefficient among them: the forward exchange carries the twists, and the pair dissipation pass runs
};

// 2: Neighbor::decide over all ranks, and if any rank's atoms moved: exchange, borders, neighbour build
int rebuild_if_moved(Run& r)
{
  int rebuild = 0, np = 0;
  RC(shhalo_check_rebuild_device(r.h, r.a->nlocal, r.a->x, &rebuild, r.st));
  if (!rebuild) return SHPAIR_OK;
  RC(shhalo_exchange_device(r.h, r.a, r.st));
  RC(shhalo_borders_device(r.h, r.a, &r.nghost, r.st));
  // the list build reports shape indices outside the table (they may have arrived with migrated atoms): a
  // rank-local failure in the middle of the step, so the ranks agree on it before the forward exchange
  RC(shhalo_neighbor_build_device(r.h, r.a, r.nghost, &np, r.st));
  ++r.nreb;
  return SHPAIR_OK;
}

// 3: with "halo_overlap" the forward exchange (pack, ncclSend / ncclRecv per peer, unpack) goes to the second stream
// behind this step's positions (and twists: the twist kernel is on the caller's stream ahead of ev_ready); ev_ghosts
// marks its end.  The wide form is ONE message per peer as well: x, quat and the twist of a row travel together.
int forward_exchange(Run& r)
{
  shhalo_ctx* h = r.h;
  const auto forward = [&](hipStream_t st) {
    return r.wide ? shhalo_forward_twist_device(h, r.a->x, r.a->quat, h->sp->step->d_twist.p, st)
                  : shhalo_forward_device(h, r.a->x, r.a->quat, st);
  };
  if (!r.st2) return forward(r.st);
  if (hipEventRecord(h->ev_ready, r.st) != hipSuccess || hipStreamWaitEvent(r.st2, h->ev_ready, 0) != hipSuccess)
    H_FAIL(h, SHPAIR_EHIP, "hipEventRecord / hipStreamWaitEvent failed (halo_overlap)");
  RC(forward(r.st2));
  if (hipEventRecord(h->ev_ghosts, r.st2) != hipSuccess) H_FAIL(h, SHPAIR_EHIP, "hipEventRecord failed (halo_overlap)");
  return SHPAIR_OK;
}

// 5 (and 6) with "halo_overlap": the pair kernels of the slots whose atoms are all owned — the front segment of the
// partitioned list, down to a multiple of 32 slots — run beside the forward exchange; the slots with a ghost wait for it.
// "halo_overlap" 2 (atomic accumulation only): the REVERSE exchange is hidden too — the owned-only slots are cut in
// two, [0, cut) runs beside the forward exchange, the ghost slots follow it, and [cut, split) runs beside the reverse
// exchange, whose unpack adds into the owners' rows with the same FP64 atomics the pair kernels use.  (The
// deterministic mode adds in a fixed order with plain stores: there the reverse exchange stays behind the kernels.  So
// it does while a gamma_ij is set: the damping pass needs the integrals of every slot and adds into ghost rows, so it
// follows the last slot range and the reverse exchange follows it, on the caller's stream.)
// *reverse_done: the reverse exchange has been enqueued here.
int overlapped_force_stage(Run& r, int step, int ef, bool* reverse_done)
{
  shhalo_ctx* h = r.h;
  shpair_ctx* sp = h->sp;
  const shhalo_arrays* a = r.a;
  *reverse_done = false;
  const bool overlap_rev = sp->opt_overlap >= 2 && !sp->opt_deterministic && !r.wide;
  const int split = (sp->n_interior < sp->npairs ? sp->n_interior : sp->npairs) & ~31;   // never beyond the installed list
  const int cut = overlap_rev ? ((split / 2) & ~31) : split;   // [0, cut) beside the forward exchange
  const auto range = [&](int k, int slot0, int slot_end, int part) {
    r.tm.tick(step, k, 0);
    const int rc = shp_compute_range(sp, a->nlocal, r.nghost, a->x, a->quat, a->type, a->shtype, 1, ef, ef, a->f, a->torque,
                                     ef ? r.p->ev_dev : nullptr, r.st, slot0, slot_end, part);
    r.tm.tick(step, k, 1);
    return rc;
  };
  H_SP(h, range(0, 0, cut, kPartPre));
  if (hipStreamWaitEvent(r.st, h->ev_ghosts, 0) != hipSuccess) H_FAIL(h, SHPAIR_EHIP, "hipStreamWaitEvent failed (halo_overlap)");
  H_SP(h, range(1, split, sp->npairs, overlap_rev ? 0 : kPartPost));
  if (!overlap_rev) return SHPAIR_OK;
  // every contribution to a ghost row is in: the reverse exchange starts on the second stream ...
  if (hipEventRecord(h->ev_bdone, r.st) != hipSuccess || hipStreamWaitEvent(r.st2, h->ev_bdone, 0) != hipSuccess)
    H_FAIL(h, SHPAIR_EHIP, "hipEventRecord / hipStreamWaitEvent failed (halo_overlap 2)");
  RC(shhalo_reverse_device(h, a->f, a->torque, r.st2));
  if (hipEventRecord(h->ev_rev, r.st2) != hipSuccess) H_FAIL(h, SHPAIR_EHIP, "hipEventRecord failed (halo_overlap 2)");
  // ... beside the second half of the owned-only slots
  H_SP(h, range(2, cut, split, kPartPost));
  if (hipStreamWaitEvent(r.st, h->ev_rev, 0) != hipSuccess) H_FAIL(h, SHPAIR_EHIP, "hipStreamWaitEvent failed (halo_overlap 2)");
  *reverse_done = true;
  return SHPAIR_OK;
}

int one_step(Run& r, int step, int nsteps)
{
  shhalo_ctx* h = r.h;
  shpair_ctx* sp = h->sp;
  shhalo_arrays* a = r.a;
  H_SP(h, step_first_half(sp, step_view(a, r.p), r.st));                                     // 1
  if ((step + 1) % r.p->check_every == 0) RC(rebuild_if_moved(r));                           // 2
  // 2b: the twists of the owned rows from the half-step v, angmom and the drifted quat.  These are the values the
  // single-rank loop uses: it computes its twists after the pair compute, but from the same arrays, which nothing
  // between here and there writes.  The ghost rows' twists are their owners', brought by the wide forward exchange.
  if (r.twists) H_SP(h, step_twists(sp, step_view(a, r.p), 0, r.st));
  RC(forward_exchange(r));                                                                   // 3
  // 4: one launch (two memsets are four fill kernels)
  H_SP(h, shstep_force_clear_device(sp, (int)((size_t)a->nlocal + r.nghost), a->f, a->torque, r.st));
  const int ef = (r.p->eflag_last && step == nsteps - 1) ? 1 : 0;
  bool reverse_done = false;
  if (r.st2) {
    RC(overlapped_force_stage(r, step, ef, &reverse_done));                                  // 5 (and 6 with "halo_overlap" 2)
  } else {
    r.tm.tick(step, 0, 0);
    const int rc = shpair_compute_device(sp, a->nlocal, r.nghost, a->x, a->quat, a->type, a->shtype, 1, ef, ef, a->f, a->torque,
                                         ef ? r.p->ev_dev : nullptr, r.st);                  // 5
    r.tm.tick(step, 0, 1);
    H_SP(h, rc);
  }
  // 5b: behind the last slot range (every slot's integrals are in); its shares of ghost rows go home with the reverse
  if (r.wide) H_SP(h, step_dissipation_pass(sp, step_view(a, r.p), r.nghost, a->x, a->type, r.st));
  if (!reverse_done) RC(shhalo_reverse_device(h, a->f, a->torque, r.st));                    // 6
  H_SP(h, step_after_reverse(sp, step_view(a, r.p), r.st));                                  // 7, 8, 9
  return SHPAIR_OK;
}

}  // namespace

extern "C" int shhalo_run_device(shhalo_ctx* h, shhalo_arrays* a, const shhalo_run_params* p, int nsteps, int* nghost_io,
                                 int* rebuilds, double* kernel_ms, void* stream)
{
  if (!h) return SHPAIR_EINVAL;
  if (rebuilds) *rebuilds = 0;
  if (kernel_ms) *kernel_ms = 0.0;
  // SPEC §2.14: xi does not migrate with its atoms yet
  if (h->sp && h->sp->hist_on)
    H_FAIL(h, SHPAIR_ESTATE, "run: tangential history is single-rank (set every tangential spring to 0 or use shstep_run_device)");
  // SPEC §2.15: nor does xi_iw of the walls
  if (h->sp && step_wall_history(h->sp))
    H_FAIL(h, SHPAIR_ESTATE, "run: wall tangential history is single-rank (set every wall tangential spring to 0 or use shstep_run_device)");
  // SPEC §2.18: cylindrical walls are not modelled in the loop over several ranks
  if (h->sp && step_has_cylinders(h->sp))
    H_FAIL(h, SHPAIR_ESTATE, "run: cylindrical walls are single-rank (remove them with shstep_set_cylinders(ctx, 0, ...) or use shstep_run_device)");
  // SPEC §2.22: nor are conical walls
  if (h->sp && step_has_cones(h->sp))
    H_FAIL(h, SHPAIR_ESTATE, "run: conical walls are single-rank (remove them with shstep_set_cones(ctx, 0, ...) or use shstep_run_device)");
  // SPEC §2.10: the 7-wide forward exchange carries x and quat only, not the twists the damping pass needs for ghost
  // rows; option "halo_twists" sends them along
  // (§2.11: friction reads the same twists; the message names what is set, friction first; §2.16: rolling or twisting
  // resistance where nothing else is set)
  if (h->sp && step_has_dissipation(h->sp) && !h->sp->opt_halo_twists) {
    const bool only_rolling = shp_has_rolling(h->sp) && !shp_has_pair_pass(h->sp) && !step_wall_reads_twists(h->sp);
    const char* what = step_has_friction(h->sp) ? "friction" : only_rolling ? "rolling or twisting resistance" : "damping";
    H_FAIL(h, SHPAIR_EINVAL, "run: contact %s is not supported by the loop over several ranks (the forward exchange carries no "
           "velocities); set every %s coefficient to 0 or use shstep_run_device, or set option halo_twists", what, what);
  }
  H_RC(h, halo_check_arrays(h, a));
  if (!p || !nghost_io || nsteps < 0) H_FAIL(h, SHPAIR_EINVAL, "null arguments or nsteps < 0");
  if (p->check_every < 1 || !std::isfinite(p->dt)) H_FAIL(h, SHPAIR_EINVAL, "bad check_every (%d) / dt", p->check_every);
  if (p->eflag_last && !p->ev_dev) H_FAIL(h, SHPAIR_EINVAL, "eflag_last set but ev_dev is null");
  if (h->plan_nlocal != a->nlocal || *nghost_io != h->nghost || !h->sp->have_neighbors)
    H_FAIL(h, SHPAIR_ESTATE, "run: the plan, ghosts and neighbour list of the current atoms must be built first "
           "(shhalo_exchange_device + shhalo_borders_device + shstep_neighbor_build_device)");
  H_HIP(h, hipSetDevice(h->sp->device));
  hipStream_t st = (hipStream_t)stream;
  Run r{h, a, p, st, nullptr, StepTimers(), *nghost_io, 0, step_has_dissipation(h->sp), shp_keeps_integrals(h->sp)};
  if (h->sp->opt_overlap) RC(overlap_stream(h, &r.st2));
  // nothing is allocated inside a step: the exchange buffers for the widest forward message, and — as
  // shstep_run_device does — the twists of the step state and the dissipation pass' per-slot buffers
  H_RC(h, halo_size_forward_buffers(h));
  if (r.twists) {
    shstep_state* s = nullptr;
    H_SP(h, step_state(h->sp, &s));
    H_HIP(h, s->d_twist.ensure(6 * (size_t)(a->nmax > 0 ? a->nmax : 1)));
    H_HIP(h, shp_size_dissipation_buffers(h->sp, (size_t)h->sp->npairs));
  }
  if (const int trc = r.tm.create(h, kernel_ms ? nsteps : 0, st)) {
    r.tm.destroy();
    return trc;
  }
  int rc = SHPAIR_OK;
  for (int step = 0; step < nsteps && rc == SHPAIR_OK; ++step) rc = one_step(r, step, nsteps);
  const hipError_t es = hipStreamSynchronize(st);
  // a step that ended early may have left an exchange in flight on the second stream, reading the caller's arrays
  if (rc != SHPAIR_OK && r.st2) (void)hipStreamSynchronize(r.st2);
  if (rc == SHPAIR_OK && es == hipSuccess && kernel_ms) *kernel_ms = r.tm.sum_ms();
  r.tm.destroy();
  *nghost_io = r.nghost;
  if (rebuilds) *rebuilds = r.nreb;
  if (rc) return rc;
  if (es != hipSuccess) H_FAIL(h, SHPAIR_EHIP, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
  // the kernels' error bits (a type or shape index outside its table — such rows arrive from other ranks packed
  // into 64-bit words — makes a kernel skip the pair / particle and raise a bit instead of reading out of bounds):
  // read once per call, and agreed on by all ranks like the failures of a reneighbouring
  // (with them the twist kernel's, which is the step kernels' word)
  int local_rc = shpair_check_device_errors(h->sp, st);
  if (!local_rc && r.twists) local_rc = shstep_check_flags(h->sp, st);
  if (local_rc) h->err = h->sp->err;
  else h->err.clear();
  H_RC(h, halo_agree(h, local_rc, st));
  return SHPAIR_OK;
}
