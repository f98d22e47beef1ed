// halo_transport.cpp — the three transports behind halo_transport.hpp, the run-time RCCL binding and the thread hub.
// HIP runtime calls (events, copies, page-locked memory) but no kernel: host code only.
//
//   RCCL    librccl is bound at run time (dlopen; the copy already in the process — e.g. PyTorch's — is preferred,
//           so that there is one RCCL and one HIP runtime per process).  ncclSend/ncclRecv over xGMI.
//   local   the ranks are host threads of ONE process that share a hub: a send posts (pointer, bytes, ready event),
//           the matching receive enqueues a device copy behind that event on the receiver's stream.  Same message
//           pattern, same kernels; for rehearsing N ranks on fewer than N GPUs and for a self-periodic single rank.
//   staged  the caller's functions move the bytes between hosts (MPI in a LAMMPS host, gloo in bench.py); the library
//           stages through page-locked host memory around them.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "halo_transport.hpp"

using namespace shp;

namespace {

// ------------------------------------------------------------------------------------------------ RCCL binding
struct RcclApi {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*GetVersion)(int*) = nullptr;
  std::string error;
};

RcclApi* rccl_api()
{
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    const char* names[] = {"librccl.so.1", "librccl.so"};
    for (const char* n : names) {  // the copy the process already holds (PyTorch's), if any
      api.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
      if (api.handle) break;
    }
    for (int k = 0; k < 2 && !api.handle; ++k) api.handle = dlopen(names[k], RTLD_NOW | RTLD_LOCAL);
    if (!api.handle) {
      const char* e = dlerror();
      api.error = std::string("librccl.so.1 could not be loaded: ") + (e ? e : "unknown dlopen error");
      return;
    }
    auto sym = [&](const char* s) -> void* {
      void* p = dlsym(api.handle, s);
      if (!p && api.error.empty()) api.error = std::string("librccl does not export ") + s;
      return p;
    };
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.CommCount = (decltype(api.CommCount))sym("ncclCommCount");
    api.Send = (decltype(api.Send))sym("ncclSend");
    api.Recv = (decltype(api.Recv))sym("ncclRecv");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    api.GetVersion = (decltype(api.GetVersion))sym("ncclGetVersion");
  });
  return &api;
}

struct RcclTransport : Transport {
  RcclApi* api = nullptr;
  ncclComm_t comm = nullptr;
  int nranks = 0;
  ~RcclTransport() override
  {
    if (comm && api) (void)api->CommDestroy(comm);
  }
  int fail(const char* what, ncclResult_t r)
  {
    err = std::string(what) + " failed: " + (api && api->GetErrorString ? api->GetErrorString(r) : "?");
    return SHPAIR_EHIP;
  }
  int exchange(const std::vector<Msg>& sends, const std::vector<Msg>& recvs, hipStream_t st) override
  {
    if (sends.empty() && recvs.empty()) return SHPAIR_OK;
    ncclResult_t r = api->GroupStart();
    if (r != ncclSuccess) return fail("ncclGroupStart", r);
    for (const Msg& m : recvs) {
      r = api->Recv(m.ptr, m.bytes, ncclChar, m.peer, comm, st);
      if (r != ncclSuccess) break;
    }
    if (r == ncclSuccess)
      for (const Msg& m : sends) {
        r = api->Send(m.ptr, m.bytes, ncclChar, m.peer, comm, st);
        if (r != ncclSuccess) break;
      }
    const ncclResult_t r2 = api->GroupEnd();
    if (r != ncclSuccess) return fail("ncclSend/ncclRecv", r);
    if (r2 != ncclSuccess) return fail("ncclGroupEnd", r2);
    return SHPAIR_OK;
  }
  int allreduce_max_i32(int* dev, int n, hipStream_t st) override
  {
    const ncclResult_t r = api->AllReduce(dev, dev, (size_t)n, ncclInt32, ncclMax, comm, st);
    return r == ncclSuccess ? SHPAIR_OK : fail("ncclAllReduce", r);
  }
  int allreduce_sum_f64(double* dev, int n, hipStream_t st) override
  {
    const ncclResult_t r = api->AllReduce(dev, dev, (size_t)n, ncclFloat64, ncclSum, comm, st);
    return r == ncclSuccess ? SHPAIR_OK : fail("ncclAllReduce", r);
  }
  int size() const override { return nranks; }
  int kind() const override { return 1; }
  int version() const override
  {
    int v = 0;
    if (api && api->GetVersion) (void)api->GetVersion(&v);
    return v;
  }
};

}  // namespace

// ------------------------------------------------------------------------------------------------ local hub
struct shhalo_hub {
  struct Post {
    const void* src;
    size_t bytes;
    hipEvent_t ready = nullptr, done = nullptr;
    bool consumed = false;
  };
  int nranks = 0;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::deque<Post*>> box;  // [src * nranks + dst]
  // all-reduce
  std::vector<double> acc, result;
  int arrived = 0;
  unsigned long long generation = 0;
};

namespace {

// a rank thread that failed must not leave the others waiting for ever
std::chrono::seconds hub_timeout()
{
  static const long s = [] {
    const char* e = getenv("SHHALO_HUB_TIMEOUT_S");
    const long v = e ? atol(e) : 0;
    return v > 0 ? v : 120L;
  }();
  return std::chrono::seconds(s);
}

struct LocalTransport : Transport {
  shhalo_hub* hub = nullptr;  // null: single rank
  int rank = 0, nranks = 1;
  int exchange(const std::vector<Msg>& sends, const std::vector<Msg>& recvs, hipStream_t st) override
  {
    if (sends.empty() && recvs.empty()) return SHPAIR_OK;
    if (!hub) {
      err = "local transport without a hub was asked to talk to another rank";
      return SHPAIR_ESTATE;
    }
    std::vector<shhalo_hub::Post*> mine;
    for (const Msg& m : sends) {
      shhalo_hub::Post* p = new shhalo_hub::Post();
      p->src = m.ptr;
      p->bytes = m.bytes;
      if (hipEventCreateWithFlags(&p->ready, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&p->done, hipEventDisableTiming) != hipSuccess || hipEventRecord(p->ready, st) != hipSuccess) {
        err = "hub: event creation failed";
        return SHPAIR_EHIP;
      }
      mine.push_back(p);
      {
        std::lock_guard<std::mutex> lk(hub->mu);
        hub->box[(size_t)rank * nranks + m.peer].push_back(p);
      }
      hub->cv.notify_all();
    }
    for (const Msg& m : recvs) {
      shhalo_hub::Post* p = nullptr;
      {
        std::unique_lock<std::mutex> lk(hub->mu);
        auto& q = hub->box[(size_t)m.peer * nranks + rank];
        if (!hub->cv.wait_for(lk, hub_timeout(), [&] { return !q.empty(); })) {
          err = "hub: rank " + std::to_string(rank) + " timed out waiting for a message from rank " + std::to_string(m.peer) +
                " (did that rank fail?)";
          return SHPAIR_ESTATE;
        }
        p = q.front();
        q.pop_front();
      }
      if (p->bytes != m.bytes) {
        err = "hub: a message from rank " + std::to_string(m.peer) + " has " + std::to_string(p->bytes) + " bytes, " +
              std::to_string(m.bytes) + " expected";
        return SHPAIR_ESTATE;
      }
      if (hipStreamWaitEvent(st, p->ready, 0) != hipSuccess ||
          hipMemcpyAsync(m.ptr, p->src, m.bytes, hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipEventRecord(p->done, st) != hipSuccess) {
        err = "hub: device copy failed";
        return SHPAIR_EHIP;
      }
      {
        std::lock_guard<std::mutex> lk(hub->mu);
        p->consumed = true;
      }
      hub->cv.notify_all();
    }
    // the send buffers may be rewritten only after the receivers' copies: this rank's stream waits for them
    for (shhalo_hub::Post* p : mine) {
      {
        std::unique_lock<std::mutex> lk(hub->mu);
        if (!hub->cv.wait_for(lk, hub_timeout(), [&] { return p->consumed; })) {
          err = "hub: rank " + std::to_string(rank) + " timed out waiting for a receiver (did that rank fail?)";
          return SHPAIR_ESTATE;  // the post stays with the hub: the receiver may still come for it
        }
      }
      (void)hipStreamWaitEvent(st, p->done, 0);
      (void)hipEventDestroy(p->ready);
      (void)hipEventDestroy(p->done);
      delete p;
    }
    return SHPAIR_OK;
  }
  template <typename T, typename OP>
  int allreduce(T* dev, int n, hipStream_t st, OP op)
  {
    if (!hub || nranks == 1) return SHPAIR_OK;
    std::vector<T> h((size_t)n);
    if (hipMemcpyAsync(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      err = "hub: all-reduce read-back failed";
      return SHPAIR_EHIP;
    }
    {
      std::unique_lock<std::mutex> lk(hub->mu);
      if (hub->arrived == 0) hub->acc.assign((size_t)n, 0.0);
      for (int k = 0; k < n; ++k) hub->acc[k] = hub->arrived == 0 ? (double)h[k] : op(hub->acc[k], (double)h[k]);
      if (++hub->arrived == nranks) {
        hub->result = hub->acc;
        hub->arrived = 0;
        ++hub->generation;
        hub->cv.notify_all();
      } else {
        const unsigned long long g = hub->generation;
        if (!hub->cv.wait_for(lk, hub_timeout(), [&] { return hub->generation != g; })) {
          err = "hub: rank " + std::to_string(rank) + " timed out in an all-reduce (did another rank fail?)";
          return SHPAIR_ESTATE;
        }
      }
      for (int k = 0; k < n; ++k) h[k] = (T)hub->result[k];
    }
    if (hipMemcpyAsync(dev, h.data(), n * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      err = "hub: all-reduce write-back failed";
      return SHPAIR_EHIP;
    }
    return SHPAIR_OK;
  }
  int allreduce_max_i32(int* dev, int n, hipStream_t st) override
  {
    return allreduce(dev, n, st, [](double a, double b) { return a > b ? a : b; });
  }
  int allreduce_sum_f64(double* dev, int n, hipStream_t st) override
  {
    return allreduce(dev, n, st, [](double a, double b) { return a + b; });
  }
  int size() const override { return nranks; }
  int kind() const override { return 0; }
};

// Host-staged transport: the caller's functions move the bytes (MPI in a LAMMPS host, gloo in bench.py); the library
// stages through page-locked host memory around them.  Every call blocks the host until its messages are complete.
struct StagedTransport : Transport {
  shhalo_exchange_fn xfn = nullptr;
  shhalo_allreduce_fn rfn = nullptr;
  void* user = nullptr;
  int rank = 0, nranks = 1;
  unsigned char* hbuf = nullptr;   // pinned: [send bytes | recv bytes]
  size_t hcap = 0;
  ~StagedTransport() override
  {
    if (hbuf) (void)hipHostFree(hbuf);
  }
  int ensure(size_t bytes)
  {
    if (bytes <= hcap) return SHPAIR_OK;
    if (hbuf) (void)hipHostFree(hbuf);
    hbuf = nullptr;
    hcap = 0;
    const size_t want = bytes + bytes / 2 + 4096;
    if (hipHostMalloc((void**)&hbuf, want) != hipSuccess) {
      (void)hipGetLastError();
      err = "staged transport: hipHostMalloc of " + std::to_string(want) + " bytes failed";
      return SHPAIR_ENOMEM;
    }
    hcap = want;
    return SHPAIR_OK;
  }
  int exchange(const std::vector<Msg>& sends, const std::vector<Msg>& recvs, hipStream_t st) override
  {
    if (sends.empty() && recvs.empty()) return SHPAIR_OK;
    size_t sb = 0, rb = 0;
    for (const Msg& m : sends) sb += (m.bytes + 15) & ~(size_t)15;
    for (const Msg& m : recvs) rb += (m.bytes + 15) & ~(size_t)15;
    // the previous exchange's upward copies read this buffer: they are complete (this call ended with a stream wait)
    if (const int rc = ensure(sb + rb)) return rc;
    std::vector<int> sp_, rp_;
    std::vector<void*> sptr, rptr;
    std::vector<size_t> sby, rby;
    size_t off = 0;
    for (const Msg& m : sends) {
      if (hipMemcpyAsync(hbuf + off, m.ptr, m.bytes, hipMemcpyDeviceToHost, st) != hipSuccess) {
        err = "staged transport: copy of a send buffer to the host failed";
        return SHPAIR_EHIP;
      }
      sp_.push_back(m.peer); sptr.push_back(hbuf + off); sby.push_back(m.bytes);
      off += (m.bytes + 15) & ~(size_t)15;
    }
    for (const Msg& m : recvs) {
      rp_.push_back(m.peer); rptr.push_back(hbuf + off); rby.push_back(m.bytes);
      off += (m.bytes + 15) & ~(size_t)15;
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
      err = "staged transport: hipStreamSynchronize failed";
      return SHPAIR_EHIP;
    }
    const int xrc = xfn(user, (int)sends.size(), sp_.data(), sptr.data(), sby.data(), (int)recvs.size(), rp_.data(), rptr.data(),
                        rby.data());
    if (xrc != 0) {
      err = "staged transport: the caller's exchange function returned " + std::to_string(xrc) + " on rank " + std::to_string(rank);
      return SHPAIR_ESTATE;
    }
    for (size_t k = 0; k < recvs.size(); ++k)
      if (hipMemcpyAsync(recvs[k].ptr, rptr[k], recvs[k].bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
        err = "staged transport: copy of a received buffer to the device failed";
        return SHPAIR_EHIP;
      }
    if (hipStreamSynchronize(st) != hipSuccess) {   // the host buffer is free again, and the caller's next call may be another exchange
      err = "staged transport: hipStreamSynchronize failed";
      return SHPAIR_EHIP;
    }
    return SHPAIR_OK;
  }
  template <typename T>
  int allreduce(T* dev, int n, int kind, hipStream_t st)
  {
    if (nranks == 1) return SHPAIR_OK;
    if (const int rc = ensure((size_t)n * sizeof(T))) return rc;
    if (hipMemcpyAsync(hbuf, dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      err = "staged transport: all-reduce read-back failed";
      return SHPAIR_EHIP;
    }
    const int rrc = rfn(user, hbuf, n, kind);
    if (rrc != 0) {
      err = "staged transport: the caller's all-reduce function returned " + std::to_string(rrc) + " on rank " + std::to_string(rank);
      return SHPAIR_ESTATE;
    }
    if (hipMemcpyAsync(dev, hbuf, (size_t)n * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      err = "staged transport: all-reduce write-back failed";
      return SHPAIR_EHIP;
    }
    return SHPAIR_OK;
  }
  int allreduce_max_i32(int* dev, int n, hipStream_t st) override { return allreduce(dev, n, 0, st); }
  int allreduce_sum_f64(double* dev, int n, hipStream_t st) override { return allreduce(dev, n, 1, st); }
  int size() const override { return nranks; }
  int kind() const override { return 2; }
};

}  // namespace

// ------------------------------------------------------------------------------------------------ the factories
namespace shp {

int make_rccl_transport(Transport** out, std::string* err, const unsigned char id[SHHALO_UNIQUE_ID_BYTES], int rank, int nranks)
{
  RcclApi* api = rccl_api();
  if (!api->handle || !api->error.empty()) {
    *err = api->error;
    return SHPAIR_ENODEV;
  }
  RcclTransport* t = new (std::nothrow) RcclTransport();
  if (!t) return SHPAIR_ENOMEM;
  t->api = api;
  t->nranks = nranks;
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  const ncclResult_t r = api->CommInitRank(&t->comm, nranks, u, rank);
  if (r != ncclSuccess) {
    *err = std::string("ncclCommInitRank failed: ") + api->GetErrorString(r);
    t->comm = nullptr;
    delete t;
    return SHPAIR_EHIP;
  }
  int cnt = 0;
  if (api->CommCount(t->comm, &cnt) == ncclSuccess) t->nranks = cnt;
  *out = t;
  return SHPAIR_OK;
}

int make_local_transport(Transport** out, std::string* err, shhalo_hub* hub, int rank, int nranks)
{
  if (nranks > 1 && (!hub || hub->nranks != nranks)) {
    *err = "a hub created for " + std::to_string(nranks) + " ranks is needed";
    return SHPAIR_EINVAL;
  }
  LocalTransport* t = new (std::nothrow) LocalTransport();
  if (!t) return SHPAIR_ENOMEM;
  t->hub = nranks > 1 ? hub : nullptr;
  t->rank = rank;
  t->nranks = nranks;
  *out = t;
  return SHPAIR_OK;
}

int make_staged_transport(Transport** out, std::string* err, shhalo_exchange_fn exchange, shhalo_allreduce_fn allreduce, void* user,
                          int rank, int nranks)
{
  if (nranks > 1 && (!exchange || !allreduce)) {
    *err = "the staged transport needs an exchange and an all-reduce function";
    return SHPAIR_EINVAL;
  }
  StagedTransport* t = new (std::nothrow) StagedTransport();
  if (!t) return SHPAIR_ENOMEM;
  t->xfn = exchange;
  t->rfn = allreduce;
  t->user = user;
  t->rank = rank;
  t->nranks = nranks;
  *out = t;
  return SHPAIR_OK;
}

}  // namespace shp

extern "C" {

int shhalo_get_unique_id(unsigned char id[SHHALO_UNIQUE_ID_BYTES])
{
  if (!id) return SHPAIR_EINVAL;
  RcclApi* api = rccl_api();
  if (!api->handle || !api->error.empty()) return SHPAIR_ENODEV;
  static_assert(sizeof(ncclUniqueId) == SHHALO_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  if (api->GetUniqueId(&u) != ncclSuccess) return SHPAIR_EHIP;
  std::memcpy(id, &u, sizeof(u));
  return SHPAIR_OK;
}

int shhalo_hub_create(shhalo_hub** out, int nranks)
{
  if (!out || nranks < 1) return SHPAIR_EINVAL;
  shhalo_hub* hub = new (std::nothrow) shhalo_hub();
  if (!hub) return SHPAIR_ENOMEM;
  hub->nranks = nranks;
  hub->box.resize((size_t)nranks * nranks);
  *out = hub;
  return SHPAIR_OK;
}

void shhalo_hub_destroy(shhalo_hub* hub) { delete hub; }

}  // extern "C"
