// halo_transport.hpp — how the messages of the halo layer travel: the interface shhalo_api.hip and shhalo_run.cpp talk
// to, and one factory per transport kind (halo_transport.cpp).  Internal: nothing here is part of the boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/shhalo.h"

namespace shp {

struct Msg {
  int peer;
  void* ptr;
  size_t bytes;
};

struct Transport {
  std::string err;
  virtual ~Transport() {}
  // one grouped exchange: at most one send and one receive per peer; zero-byte messages are left out by the caller
  virtual int exchange(const std::vector<Msg>& sends, const std::vector<Msg>& recvs, hipStream_t st) = 0;
  virtual int allreduce_max_i32(int* dev, int n, hipStream_t st) = 0;   // in place
  virtual int allreduce_sum_f64(double* dev, int n, hipStream_t st) = 0;
  virtual int size() const = 0;
  virtual int kind() const = 0;  // 0 local, 1 RCCL, 2 host-staged
  virtual int version() const { return 0; }
};

// The factories return SHPAIR_OK and the transport in *out, or an error code, *out untouched and (except for
// SHPAIR_ENOMEM) the reason in *err.  The RCCL one joins the communicator of `id` on the current device.
int make_rccl_transport(Transport** out, std::string* err, const unsigned char id[SHHALO_UNIQUE_ID_BYTES], int rank, int nranks);
int make_local_transport(Transport** out, std::string* err, shhalo_hub* hub, int rank, int nranks);
int make_staged_transport(Transport** out, std::string* err, shhalo_exchange_fn exchange, shhalo_allreduce_fn allreduce, void* user,
                          int rank, int nranks);

}  // namespace shp
