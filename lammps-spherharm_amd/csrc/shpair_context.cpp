// shpair_context.cpp — the context behind include/shpair.h and its options: create / destroy, error text, options,
// pinned caller ranges, output pointers, stream, statistics, and the decoder of the kernels' error word.  Host code
// only: nothing here launches a kernel.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "../../include/shpair.h"
#include "pair_params.hpp"
#include "shpair_ctx.hpp"

using namespace shp;

// Decodes the device error word (pair_params.hpp kPairErr*) once it has been read back: returns the code with the
// message in c->err (SHPAIR_OK for no bits), and clears the device copy of a word that had any.
int shpair_decode_device_errors(shpair_ctx* c, int bits, hipStream_t st)
{
  if (!bits) return SHPAIR_OK;
  HIPCHK(c, hipMemsetAsync(c->d_err.p, 0, sizeof(int), st));
  if (bits & (kPairErrShape | kPairErrType))
    CTX_FAIL(c, SHPAIR_EINVAL, "an atom %s outside its table reached the pair kernel; the pairs of those atoms were skipped",
             (bits & kPairErrShape) ? "shape index (shtype)" : "type");
  if (!(bits & (kPairErrCoincident | kPairErrWall | kPairErrCylinder)))
    CTX_FAIL(c, SHPAIR_EINVAL, "particle centre outside a cone: a centre at or outside a cone's wall or behind its apex (or a position "
             "that is not a number); that particle/cone contact was skipped (docs/SPEC.md 2.22)");
  if (!(bits & (kPairErrCoincident | kPairErrWall)))
    CTX_FAIL(c, SHPAIR_EINVAL, "particle centre outside a cylinder: a centre at or outside a cylinder's wall (or a position that is "
             "not a number); that particle/cylinder contact was skipped (docs/SPEC.md 2.18)");
  if (!(bits & kPairErrCoincident))
    CTX_FAIL(c, SHPAIR_EINVAL, "particle centre behind a wall: a centre at or behind a wall's plane (or a position that is not a "
             "number); that particle/wall contact was skipped (docs/SPEC.md 2.9)");
  CTX_FAIL(c, SHPAIR_EINVAL, "coincident centres: a listed pair has separation 0 (or a position that is not a number); it was "
           "skipped (docs/SPEC.md 2, step 1)");
}

// Reads and clears the error bits the pair kernel raises instead of reading outside a table.  Blocks on `stream`.
int shpair_check_device_errors(shpair_ctx* c, void* stream)
{
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(c, hipMemcpyAsync(c->h_err, c->d_err.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return shpair_decode_device_errors(c, *c->h_err, st);
}

extern "C" {

const char* shpair_version(void) { return "shpair 0.1 gfx950"; }

const char* shpair_strerror(int code)
{
  switch (code) {
    case SHPAIR_OK: return "ok";
    case SHPAIR_EINVAL: return "invalid argument";
    case SHPAIR_ENODEV: return "no usable HIP device (this library has no CPU fallback)";
    case SHPAIR_EHIP: return "HIP runtime error";
    case SHPAIR_ESTATE: return "call order error: shapes, coefficients or neighbour list not set";
    case SHPAIR_ENOMEM: return "out of memory";
    case SHPAIR_ELMAX: return "lmax or nq above the compiled limit";
    default: return "unknown shpair error";
  }
}

const char* shpair_last_error(const shpair_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int shpair_create(shpair_ctx** out, int device_id)
{
  if (!out) return SHPAIR_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SHPAIR_ENODEV;
  if (device_id < 0 || device_id >= ndev) return SHPAIR_ENODEV;
  if (hipSetDevice(device_id) != hipSuccess) return SHPAIR_ENODEV;
  shpair_ctx* c = new (std::nothrow) shpair_ctx();
  if (!c) return SHPAIR_ENOMEM;
  c->device = device_id;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream_up, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreate(&c->evA) != hipSuccess || hipEventCreate(&c->evB) != hipSuccess ||
      c->h_ev.resize(7) != hipSuccess || c->h_counters.resize(2) != hipSuccess || c->h_err.resize(1) != hipSuccess ||
      c->d_err.ensure(1) != hipSuccess || hipMemset(c->d_err.p, 0, sizeof(int)) != hipSuccess ||
      c->d_counters.ensure(2) != hipSuccess || c->d_ev.ensure(7) != hipSuccess) {
    shpair_destroy(c);
    return SHPAIR_EHIP;
  }
  *out = c;
  return SHPAIR_OK;
}

// What order requires: the device of the allocations is current, nothing is in flight, the caller's ranges are
// unpinned, the step state goes before the streams.  Every buffer is freed by its owner when the context is deleted.
void shpair_destroy(shpair_ctx* c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& pr : c->pinned) (void)hipHostUnregister(pr.first);
  (void)hipGetLastError();
  shstep_release_state(c);
  for (hipEvent_t e : {c->ev0, c->ev1, c->evA, c->evB, c->ev_up})
    if (e) (void)hipEventDestroy(e);
  if (c->stream_up) (void)hipStreamDestroy(c->stream_up);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// Page-locks a caller-owned host array for the host-pointer entry point (hipHostRegister): hipMemcpyAsync of a
// registered range is a direct DMA at PCIe rate instead of the runtime's staged copy of pageable memory.
int shpair_pin_host(shpair_ctx* c, void* ptr, size_t bytes)
{
  if (!c) return SHPAIR_EINVAL;
  if (!ptr || bytes == 0) CTX_FAIL(c, SHPAIR_EINVAL, "pin_host: null pointer or zero size");
  HIPCHK(c, hipSetDevice(c->device));
  for (auto& pr : c->pinned)
    if (pr.first == ptr) {
      if (pr.second == bytes) return SHPAIR_OK;
      (void)hipHostUnregister(ptr);   // same start, another length: the array was reallocated in place
      (void)hipGetLastError();
      pr = c->pinned.back();
      c->pinned.pop_back();
      break;
    }
  const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    CTX_FAIL(c, SHPAIR_EHIP, "hipHostRegister(%p, %zu) failed: %s (the copies fall back to the runtime's staging)", ptr, bytes,
             hipGetErrorString(e));
  }
  c->pinned.emplace_back(ptr, bytes);
  return SHPAIR_OK;
}

int shpair_unpin_host(shpair_ctx* c, void* ptr)
{
  if (!c) return SHPAIR_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < c->pinned.size(); ++k)
    if (c->pinned[k].first == ptr) {
      (void)hipHostUnregister(ptr);
      (void)hipGetLastError();
      c->pinned[k] = c->pinned.back();
      c->pinned.pop_back();
      return SHPAIR_OK;
    }
  CTX_FAIL(c, SHPAIR_EINVAL, "unpin_host: %p was not pinned through this context", ptr);
}

int shpair_set_peratom_output(shpair_ctx* c, double* eatom_dev, double* vatom_dev)
{
  if (!c) return SHPAIR_EINVAL;
  c->eatom_dev = eatom_dev;
  c->vatom_dev = vatom_dev;
  return SHPAIR_OK;
}

int shpair_set_peratom_host(shpair_ctx* c, double* eatom, double* vatom)
{
  if (!c) return SHPAIR_EINVAL;
  c->eatom_host = eatom;
  c->vatom_host = vatom;
  return SHPAIR_OK;
}

int shpair_set_option(shpair_ctx* c, const char* key, int value)
{
  if (!c || !key) return SHPAIR_EINVAL;
  if (!strcmp(key, "force_volume")) c->opt_force_volume = value ? 1 : 0;
  else if (!strcmp(key, "timing")) c->opt_timing = value ? 1 : 0;
  else if (!strcmp(key, "count")) c->opt_count = value ? 1 : 0;
  else if (!strcmp(key, "variant")) c->plan_opt.variant = value;
  else if (!strcmp(key, "rule")) {
    if (value != 0 && value != 1) CTX_FAIL(c, SHPAIR_EINVAL, "rule %d is neither 0 (sharp) nor 1 (weighted)", value);
    c->plan_opt.rule = value;
  }
  else if (!strcmp(key, "ring_rows")) c->plan_opt.ring_rows = value;
  else if (!strcmp(key, "jpoly")) c->plan_opt.jpoly = value;
  else if (!strcmp(key, "split")) c->plan_opt.split = value;
  else if (!strcmp(key, "deterministic")) {
    c->opt_deterministic = value ? 1 : 0;
    c->rev_dirty = true;
  }
  else if (!strcmp(key, "waves_per_block")) c->plan_opt.waves_per_block = value;
  else if (!strcmp(key, "queue_slack")) c->plan_opt.queue_slack = value ? 1 : 0;
  else if (!strcmp(key, "spec")) c->plan_opt.spec = value != 0;
  else if (!strcmp(key, "halo_overlap")) c->opt_overlap = value <= 0 ? 0 : (value >= 2 ? 2 : 1);
  else if (!strcmp(key, "halo_stream_priority")) c->opt_halo_prio = value != 0;   // takes effect at the next shhalo_run_device (both kinds of stream are kept)
  else if (!strcmp(key, "halo_twists")) c->opt_halo_twists = value ? 1 : 0;
  else CTX_FAIL(c, SHPAIR_EINVAL, "unknown option '%s'", key);
  return SHPAIR_OK;
}

int shpair_get_stats(shpair_ctx* c, shpair_stats* out)
{
  if (!c || !out) return SHPAIR_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  c->stats.kernel_ms = 0.0;
  c->stats.total_ms = 0.0;
  c->stats.n_contact = -1;
  c->stats.n_touching = -1;
  if (c->timed_last) {
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->stats.kernel_ms = ms;
  }
  if (c->counted_last) {
    HIPCHK(c, hipEventSynchronize(c->evB));
    c->stats.n_contact = (long long)c->h_counters[0];
    c->stats.n_touching = (long long)c->h_counters[1];
  }
  if (c->total_timed_last) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->evA, c->evB) == hipSuccess) c->stats.total_ms = ms;
  }
  *out = c->stats;
  if (c->timed_last || c->counted_last) {
    // the compute these numbers belong to has finished: report what its kernel could not index
    HIPCHK(c, hipDeviceSynchronize());
    return shpair_check_device_errors(c, c->stream);
  }
  return SHPAIR_OK;
}

int shpair_set_pair_output(shpair_ctx* c, double* pair_out_dev)
{
  if (!c) return SHPAIR_EINVAL;
  c->pair_out = pair_out_dev;
  return SHPAIR_OK;
}

// Not part of include/shpair.h: work counters of SHP_STATS diagnostic builds.
int shpair_debug_set_counters(shpair_ctx* c, unsigned long long* dbg_dev)
{
  if (!c) return SHPAIR_EINVAL;
  c->dbg = dbg_dev;
  return SHPAIR_OK;
}

int shpair_get_stream(shpair_ctx* c, void** stream)
{
  if (!c || !stream) return SHPAIR_EINVAL;
  *stream = (void*)c->stream;
  return SHPAIR_OK;
}

int shpair_synchronize(shpair_ctx* c)
{
  if (!c) return SHPAIR_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return shpair_check_device_errors(c, c->stream);
}

}  // extern "C"
