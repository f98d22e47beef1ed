// shhalo_ctx.hpp — the context behind include/shhalo.h, shared by shhalo_api.hip (plan, exchanges: every kernel launch
// of the halo layer) and shhalo_run.cpp (the timestep loop over all ranks).  Internal: nothing here is part of the
// boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "../../include/shhalo.h"
#include "halo_plan.hpp"
#include "halo_transport.hpp"
#include "shpair_ctx.hpp"

namespace shp {
// the slot and message tables the kernels take by value: their types are those of halo_kernels.hpp, which only
// shhalo_api.hip may include (its kernels are not templates: one definition per library)
struct HaloKernelTables;
}  // namespace shp

struct shhalo_ctx {
  shpair_ctx* sp = nullptr;
  shp::Transport* tr = nullptr;
  shhalo_geometry geo{};
  shp::HaloGeom hg{};
  double skin = 0.0;
  std::string err;

  // static: remote peers (ascending rank); the slot tables of the two partitions are in kt
  int npeers = 0;
  int peer_rank[26] = {};
  shp::HaloKernelTables* kt = nullptr;

  // the current plan
  shhalo_layout lay{};
  int plan_nlocal = -1, nghost = 0;
  shp::DevBuf<int> d_send_idx, d_order;
  shp::DevBuf<unsigned char> d_send_code, d_cat;
  shp::DevBuf<double> d_sendbuf, d_recvbuf, d_rsend, d_rrecv, d_migrows, d_migin;
  shp::DevBuf<int> d_blockcnt, d_start, d_totals, d_msg, d_msgin, d_flags, d_peer_of_slot;
  shp::PinBuf<int> h_ints;  // totals[28] | msgin[26*27] | flags[4] (kPin* of shhalo_api.hip)
  shhalo_stats stats{};
  // option "halo_overlap" of the pair context: the forward exchange of a step runs on a stream of its own beside the
  // pair kernels of the slots that touch owned atoms only (made on first use, shhalo_run.cpp)
  hipStream_t st2x[2] = {nullptr, nullptr};   // the exchange stream of "halo_overlap": [0] ordinary, [1] at the highest stream priority
  bool ev2 = false;
  hipEvent_t ev_ready = nullptr, ev_ghosts = nullptr, ev_bdone = nullptr, ev_rev = nullptr;
};

namespace shp {
// shhalo_api.hip, for the run loop: argument check of the per-atom arrays, and the collective decision to fail
int halo_check_arrays(shhalo_ctx* h, const shhalo_arrays* a);
int halo_agree(shhalo_ctx* h, int local_rc, hipStream_t st);
int halo_size_forward_buffers(shhalo_ctx* h);   // send / receive buffers of the current layout for the widest forward message
// option "halo_twists" and a pair damping or pair friction coefficient set: the forward exchange of shhalo_run_device is
// the 13-wide one with the twists
inline bool halo_forward_is_wide(const shhalo_ctx* h) { return h->sp && h->sp->opt_halo_twists && shp_keeps_integrals(h->sp); }
}  // namespace shp

#define H_FAIL(h, code, ...)                \
  do {                                      \
    char _b[512];                           \
    snprintf(_b, sizeof(_b), __VA_ARGS__);  \
    (h)->err = _b;                          \
    return (code);                          \
  } while (0)
#define H_HIP(h, call)                                                                                  \
  do {                                                                                                  \
    hipError_t _e = (call);                                                                             \
    if (_e != hipSuccess)                                                                               \
      H_FAIL(h, SHPAIR_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define H_RC(h, call)                                        \
  do {                                                       \
    const int _rc = (call);                                  \
    if (_rc) {                                               \
      if ((h)->err.empty()) (h)->err = "internal error";     \
      return _rc;                                            \
    }                                                        \
  } while (0)
#define H_TR(h, call)                          \
  do {                                         \
    const int _rc = (call);                    \
    if (_rc) {                                 \
      (h)->err = (h)->tr->err;                 \
      return _rc;                              \
    }                                          \
  } while (0)
#define H_SP(h, call)                          \
  do {                                         \
    const int _rc = (call);                    \
    if (_rc) {                                 \
      (h)->err = (h)->sp->err;                 \
      return _rc;                              \
    }                                          \
  } while (0)
