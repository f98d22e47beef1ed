// shpair_ctx.hpp — the context behind the C ABI (include/shpair.h, include/shstep.h), shared by the
// translation units that implement it.  Internal: nothing here is part of the boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/shpair.h"
#include "contact_plan.hpp"

namespace shp {
// Device memory that belongs to its holder: freed when the holder goes (the device of the allocation must be
// current then: shpair_destroy / shhalo_destroy set it before they delete).  Moves and swaps, never copies.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    std::swap(p, o.p);   // o frees what this one held
    std::swap(cap, o.cap);
    return *this;
  }
  ~DevBuf()
  {
    if (p) (void)hipFree(p);
  }
  hipError_t ensure(size_t n)
  {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 16;
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
};

// The pinned-host counterpart (hipHostMalloc): read-back words and the staged neighbour list.  Stands in for its
// pointer wherever one is read.
template <typename T>
struct PinBuf {
  T* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf()
  {
    if (p) (void)hipHostFree(p);
  }
  operator T*() const { return p; }
  // exactly n elements, nothing kept: free, then allocate
  hipError_t resize(size_t n)
  {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
};

// the host-pointer entry points: one array up to / down from its staging buffer, asynchronous on `st`
template <typename T>
inline hipError_t upload(DevBuf<T>& b, const T* src, size_t n, hipStream_t st)
{
  return hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, st);
}
template <typename T>
inline hipError_t download(T* dst, const DevBuf<T>& b, size_t n, hipStream_t st)
{
  return hipMemcpyAsync(dst, b.p, n * sizeof(T), hipMemcpyDeviceToHost, st);
}

struct Shape {
  int lmax = -1;
  std::vector<double> anm;
  double rmax = 0.0;
  double density = 1.0;  // shstep_set_density
};

// The energy ledger (SPEC §2.13, ledger_kernels.hpp): the shapes of its fold and of its accumulator, which the
// translation units that size its buffers share with the one that holds its kernels.
constexpr int kLedgerBlock = 256;      // threads of a fold block; the wall rows' partition is wall_rows_partial_kernel's (kWallBlock)
constexpr int kLedgerChunk = 2048;     // list slots per block of the pair fold's first stage
constexpr int kLedgerWallTerms = 5;    // per (particle, wall): F_w[3], P_d, P_f
constexpr int kLedgerTotals = 5;       // pair damping, pair friction, wall damping, wall friction, wall work
constexpr int kLedgerPerWall = 3;      // per wall: damping, friction, work
constexpr int kLedgerDoubles = kLedgerTotals + kLedgerPerWall * 32;   // 32 = SHSTEP_MAX_WALLS
// Its cylinder entries (SPEC §2.20, cyl_power_kernels.hpp): the shell accumulator, which shstep_ledger.hip zeroes too.
constexpr int kShellTotals = 3;                         // D_d, D_f, W over the cylinders
constexpr int kShellDoubles = kShellTotals + 3 * 8;     // totals, then 3 (kCylPowerRow) per cylinder; 8 = SHSTEP_MAX_CYLINDERS

inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b > 0 ? (n + b - 1) / b : 1); }   // blocks of b over n rows

}  // namespace shp

struct shstep_state;  // shstep_state.hpp

struct shpair_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream_up = nullptr;   // host-pointer form: f / torque go up here beside the set-up and rotation kernels
  hipEvent_t ev_up = nullptr;        // ... and the contact kernel waits for this
  hipEvent_t pre_contact_wait = nullptr;   // set by shpair_compute for the duration of its call (launch_pair_contact)
  std::vector<std::pair<void*, size_t>> pinned;   // shpair_pin_host registrations
  std::string err;

  int nq = 16;
  int ntypes = 0, nshapes = 0;
  std::vector<shp::Shape> shapes;
  std::vector<double> kn, expo;
  bool tables_dirty = true, quad_dirty = true;
  bool mass_dirty = true;  // rigid-body table of shstep_api.hip
  bool any_nonunit_exponent = false;
  int lmax = -1, cstride = 0;

  shp::DevBuf<double> d_rc, d_coef, d_coefm, d_rmax, d_kn, d_expo, d_quad, d_creal, d_xval, d_gscale;
  shp::DevBuf<int> d_xcol, d_xinfo;
  shp::DevBuf<double> d_jval;   // first stage of particle j's per-azimuth polynomials (sh_tables.cpp build_jpoly_ell)
  shp::DevBuf<int> d_jcol;
  shp::DevBuf<int> d_pair_i, d_pair_j;
  shp::DevBuf<double> d_rot;  // rotated coefficient vectors of both particles of every list slot (pair_rotate_kernel)
  shp::DevBuf<double> d_rec;  // per-pair records of pair_setup.hpp, kRecStride doubles per list slot
  shp::DevBuf<int> d_rec_i;   // 4 ints per list slot
  int npairs = 0;
  int max_atom_index = -1;  // largest i or j in the uploaded list
  bool have_neighbors = false;

  // staging for the host-pointer entry point
  shp::DevBuf<double> d_x, d_quat, d_f, d_torque, d_ev;
  shp::DevBuf<int> d_type, d_shtype;
  shp::PinBuf<double> h_ev;  // 7

  // neighbour lists installed so far
  unsigned long long list_gen = 0;
  // flattened LAMMPS list on its way to the device (pinned), and its device copy (expanded by expand_csr_kernel)
  shp::PinBuf<int> h_list;
  shp::DevBuf<int> d_list;
  // device error bits raised by the pair kernel (pair_params.hpp kPairErr*), read at the blocking calls
  shp::DevBuf<int> d_err;
  shp::PinBuf<int> h_err;
  // last output pointers that passed the device-memory check of shpair_compute_device
  const void* ok_ptr[3] = {nullptr, nullptr, nullptr};

  shp::DevBuf<unsigned long long> d_counters;
  shp::DevBuf<unsigned char> d_flags;
  shp::PinBuf<unsigned long long> h_counters;  // 2

  int opt_force_volume = 0, opt_timing = 0, opt_count = 0;
  shp::ContactOptions plan_opt;   // the options the contact kernel's launch plan reads (contact_plan.hpp)
  shp::ContactPlan last_plan;     // ... and the plan of the last launch (shpair_get_kernel_info)
  bool last_needv = false;        // the volume path of the last launch's instance
  int opt_overlap = 0;   // "halo_overlap" (default 0 since round 5: the exchanges and the pair kernels follow each other on the caller's
                         // stream; 1 / 2 are opt-in until a run between GPUs has measured them — bench.py --gpus N tries 2, checks it
                         // against 0 in the run itself and reports both): device-built lists are partitioned interior / boundary and
                         // shhalo_run_device runs the interior slots while the forward (2: and the reverse) exchange is in flight
  int opt_halo_prio = 0; // "halo_stream_priority": 1 = the exchange stream of "halo_overlap" is one at the highest stream priority (a hardware queue of its own; shhalo_run.cpp)
  int opt_halo_twists = 0;   // "halo_twists": shhalo_run_device runs damped / with friction; while a pair coefficient of either is set its forward exchange carries the owners' twists (13 doubles per row)
  int n_interior = 0;    // slots [0, n_interior) of the installed list touch owned atoms only (device-built lists)
  // deterministic accumulation (det_kernels.hpp): per-slot results + reverse index (atom -> its list slots)
  int opt_deterministic = 0;
  shp::DevBuf<double> d_pair_ft;
  shp::DevBuf<double> d_pair_ev;    // eflag / vflag: 8 doubles per slot (E, 6 virial terms, pad) + the block sums of the ordered reduce
  shp::DevBuf<int> d_rev_start, d_rev_cur, d_rev_ent;
  bool rev_dirty = true;
  int rev_nall = 0;
  double* pair_out = nullptr;
  // contact dissipation of pairs (dissipation_kernels.hpp, entry points in shstep_dissipation.hip; the walls' share
  // is in WallState, shstep_state.hpp):
  // volume-rate damping (SPEC §2.10) and Coulomb-capped friction (§2.11)
  std::vector<double> damp_gamma;   // (ntypes+1)^2 like kn; empty until the first shstep_set_pair_damping
  std::vector<double> fric_coef;    // [2][(ntypes+1)^2]: mu_ij, then gamma_t,ij; empty until the first shstep_set_pair_friction
  bool damp_on = false;             // some gamma_ij != 0
  bool fric_on = false;             // some type pair has mu_ij != 0 and gamma_t,ij != 0
  shp::DevBuf<double> d_damp_gamma, d_fric_coef;
  // while damp_on or fric_on (shp_keeps_integrals) every compute leaves the per-slot integrals for the pair pass
  shp::DevBuf<double> d_slot_int;   // the context's own integral buffer, 7 doubles per slot (unless the caller installed one)
  shp::DevBuf<double> d_slot_ft;    // deterministic mode: the pair pass' own 12 doubles per slot
  const double* integrals_src = nullptr;   // the integrals of the last compute on the installed list; null: none since they are kept
  bool integrals_needv = false;            // ... and whether its kernel had the volume path
  // energy ledger (SPEC §2.13; entry points in shstep_ledger.hip, the accumulator is in the step state)
  bool ledger_on = false;           // shstep_set_energy_ledger: the dissipation and wall passes leave power rows
  shp::DevBuf<double> d_slot_pow;   // the pair pass' 2 doubles per slot, then the block sums of the fold's first stage
  bool ledger_pair_fresh = false;   // a pair pass has left rows the fold has not added yet ...
  int ledger_pair_np = 0;           // ... for this many slots
  bool ledger_rows_pair = false;    // the PAIR pass wrote them from the last compute's integrals: the rolling pass (SPEC §2.16) adds
                                    // to them, and writes them otherwise; set by the pair pass alone, cleared by every compute, list
                                    // install and fold
  // tangential springs with history (SPEC §2.14; history_kernels.hpp, entry points in shstep_dissipation.hip)
  std::vector<double> spring_kt;    // (ntypes+1)^2 like kn; empty until the first shstep_set_pair_tangential_spring
  bool hist_on = false;             // some k_t,ij != 0: the pair pass is shstep_pair_contact_device, builds keep keys and carry xi
  shp::DevBuf<double> d_spring_kt;
  // The *_old buffers are swap partners: a build swaps the installed list's in there and reads them in the carry.  They
  // are kept for the next swap, so after the first carried build they stand at the size of a list each.
  shp::DevBuf<double> d_xi, d_xi_old;       // xi of the installed list, 3 planes of hist_np doubles; the previous list's
  shp::DevBuf<int> d_hkey, d_hkey_old;      // per slot: the tag of j's owner
  shp::DevBuf<int> d_hoffs_old;             // the previous list's row offsets (swapped with the step state's d_offs)
  int hist_np = -1;                 // slots of the device-built list d_xi and d_hkey were filled for; -1: they hold nothing
  // rolling and twisting resistance (SPEC §2.16; rolling_kernels.hpp, entry points in shstep_rolling.hip)
  std::vector<double> roll_coef;    // [2][(ntypes+1)^2]: mu_r,ij, then gamma_r,ij; empty until the first shstep_set_pair_rolling
  std::vector<double> twist_coef;   // [2][(ntypes+1)^2]: mu_tw,ij, then gamma_tw,ij; empty until the first shstep_set_pair_twisting
  bool roll_on = false;             // some type pair has mu_r,ij != 0 and gamma_r,ij != 0
  bool twistres_on = false;         // some type pair has mu_tw,ij != 0 and gamma_tw,ij != 0
  shp::DevBuf<double> d_roll_coef, d_twist_coef;
  double *eatom_dev = nullptr, *vatom_dev = nullptr;    // shpair_set_peratom_output
  double *eatom_host = nullptr, *vatom_host = nullptr;  // shpair_set_peratom_host
  shp::DevBuf<double> d_eatom, d_vatom;                 // staging of the host form
  unsigned long long* dbg = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evA = nullptr, evB = nullptr;
  bool timed_last = false, counted_last = false, total_timed_last = false;
  shpair_stats stats{};

  shstep_state* step = nullptr;  // integrator / borders / neighbour-build state, created on first use
};

void shstep_release_state(shpair_ctx* c);   // shstep_api.hip: deletes the step state
void shstep_invalidate_list(shpair_ctx* c);
int shpair_prepare_tables(shpair_ctx* c);    // shpair_tables.cpp: the one place that refreshes stale tables (blocking copies)
int shpair_upload_quadrature(shpair_ctx* c); // shpair_api.hip: the d_quad table, laid out by ring_tables.hpp QuadLayout
int shpair_decode_device_errors(shpair_ctx* c, int bits, hipStream_t st);   // shpair_context.cpp: message for a read-back error word
int shpair_check_device_errors(shpair_ctx* c, void* stream);  // shpair_context.cpp: reads + clears the kernel's error bits (blocks)
int shstep_exclusive_scan(shpair_ctx* c, const int* in, int* out, int n, void* stream);                           // shstep_api.hip
int shstep_enqueue_check(shpair_ctx* c, int nlocal, const double* x, int** flag_dev, int* forced, void* stream);  // shstep_api.hip
int shstep_check_flags(shpair_ctx* c, void* stream);   // shstep_api.hip: reads + clears the step kernels' error bits (blocks)

#define CTX_FAIL(ctx, code, ...)                         \
  do {                                                   \
    char _b[512];                                        \
    snprintf(_b, sizeof(_b), __VA_ARGS__);               \
    (ctx)->err = _b;                                     \
    return (code);                                       \
  } while (0)

#define HIPCHK(ctx, call)                                                                          \
  do {                                                                                             \
    hipError_t _e = (call);                                                                        \
    if (_e != hipSuccess)                                                                          \
      CTX_FAIL(ctx, SHPAIR_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

#define RC(call)            \
  do {                      \
    const int _rc = (call); \
    if (_rc) return _rc;    \
  } while (0)

// shpair_api.hip: sizes the per-slot buffers of the pair kernels for a list of np slots (used by every list install)
hipError_t shp_size_pair_buffers(shpair_ctx* c, size_t np);
// ... and the dissipation pass' share of them (nothing while every pair coefficient is 0): touches no other state
hipError_t shp_size_dissipation_buffers(shpair_ctx* c, size_t np);
// damping, friction or a tangential spring is set: the pair pass of shstep_dissipation.hip has a kernel to launch
inline bool shp_has_pair_pass(const shpair_ctx* c) { return c->damp_on || c->fric_on || c->hist_on; }
// ... a rolling or twisting coefficient (SPEC §2.16): the pass of shstep_rolling.hip has
inline bool shp_has_rolling(const shpair_ctx* c) { return c->roll_on || c->twistres_on; }
// a pair coefficient is set: every compute zeroes and fills the per-slot integrals
inline bool shp_keeps_integrals(const shpair_ctx* c) { return shp_has_pair_pass(c) || shp_has_rolling(c); }
// shpair_api.hip: the ordered gather of the deterministic mode over a per-slot buffer of 12 doubles (the reverse index
// is the one the last compute built)
int shp_det_gather(shpair_ctx* c, const double* pair_ft, double* f, double* torque, hipStream_t st);
// the pair path over the slots [slot0, slot_end) of the installed list (shpair_api.hip; part: kPartPre | kPartPost)
enum { kPartPre = 1, kPartPost = 2 };
extern "C" int shp_compute_range(shpair_ctx* c, int nlocal, int nghost, const double* x, const double* quat, const int* type,
                                 const int* shtype, int newton_pair, int eflag, int vflag, double* f, double* torque, double* ev,
                                 void* stream, int slot0, int slot_end, int part);
