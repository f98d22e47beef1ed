// pair_params.hpp — what the set-up kernel, the contact kernel and the host share: the kernel arguments (PairParams),
// the device error bits, the layout of the per-pair record (FR_*) and the types of the per-order launch entry points.
#pragma once
#include <hip/hip_runtime.h>

#include "contact_plan.hpp"

namespace shp {

struct PairParams {
  // atoms (device)
  const double* x;
  const double* quat;
  const int* type;
  const int* shtype;
  double* f;
  double* torque;
  // half list, expanded: one (i, j) per slot
  const int* pair_i;
  const int* pair_j;
  int npairs;           // end of the slot range of this launch (exclusive); the whole list unless a caller splits it
  int slot0;            // ... and its first slot: a multiple of 32 (rotation tiles hold 64 rotations = 32 slots).  The halo
                        // loop runs the slots whose atoms are all owned before the forward exchange has landed (shhalo_api.hip)
  int nlocal;
  int newton_pair;
  // shape tables
  const double* rc;     // recurrence constants a'_nm for lmax, m-major (ring tables; run-time-order kernel)
  const double* coef;   // nshapes x cstride doubles: monomial table (compiled orders) or cw (run-time order)
  const double* rmax;   // nshapes
  int nshapes;
  int* err;             // device error bits (kPairErr*), raised instead of an out-of-bounds table read
  int cstride;
  int lmax;
  // pair coefficients, (ntypes+1)^2 row-major
  const double* kn;
  const double* expo;
  int ntypes;
  // cap-frame evaluation of particle i (sh_tables.hpp)
  const double* creal;   // nshapes x (lmax+1)^2 real-basis coefficients
  const double* xval;    // X = T(Rx(+90)) and X^T in ELL form: 2 x (lmax+1)^2 rows x (lmax/2+1) values
  const int* xcol;       // ... and absolute column indices
  const int* xinfo;      // (lmax+1)^2: l | (m + l) << 8
  const double* gscale;  // (lmax+1)^2 ring-recurrence scale g_lm
  // particle j in the pair's common frame (compiled orders; jpoly.hpp jpoly_build)
  const double* jval;    // first stage, ELL: (2 lmax + 4)(lmax + 1) rows x (lmax/2+1) values (sh_tables.cpp build_jpoly_ell)
  const int* jcol;       // ... and indices into the rotated coefficient vector
  const double* trigj;   // (cos, sin)(m psi_l), m = 0..lmax + 1, of the first nq azimuths, l-major
  const double* rot;     // compiled orders: rotated, scaled coefficient vectors of slot w's particles, rotation 2 w + which
                         // (which 0: i, 1: j), in the tiled layout of rot_index(); written by pair_rotate_lane_kernel
  int jpoly;             // 1: the pair records carry the Euler angles of j's frame in the slots of FR_BJ1 / FR_BJ2
  int split;             // 1: two waves per pair (pair_contact_azimuth_kernel<..., WPP = 2>); wave_lds_bytes is then the PAIR's LDS
  // per-pair records written by pair_setup_kernel (pair_setup.hpp), read here instead of redoing the scalar set-up on
  // 64 lanes: rec[kRecStride * w] = the pair frame FR_* and the Euler cos/sin; rec_i[4 w] = status, shape i, shape j,
  // [rho < R_j]
  const double* rec;
  const int* rec_i;
  int wave_lds_bytes;    // dynamic LDS per wave (wave_lds_layout)
  int ring_rows;         // quadrature rings whose tables are resident at a time (<= nq)
  int qcap;              // per-azimuth kernels: entries of a wave's node queue (queue_capacity)
  int waves_per_block;
  int spec;              // 1: a launch whose (n_q, ring_rows, qcap) are those of PairSpec<L> takes the specialised instance
  // quadrature tables
  const double* glt;    // nq Gauss-Legendre nodes on [-1,1]
  const double* glw;    // nq weights
  const double* cpsi;   // 2nq cos(psi_l)
  const double* spsi;   // 2nq sin(psi_l)
  int rule;             // 0: sharp inside test (SPEC §2.5); 1: covered-fraction weights (SPEC §2.8)
  double* eatom;        // nullable: per-atom energy  [nall], LAMMPS eatom (ev_tally_xyz halves)
  double* vatom;        // nullable: per-atom virial  [nall][6] (xx,yy,zz,xy,xz,yz)
  const double* trig;   // (cos, sin)(m psi_l), m = 2..lmax; trig_lmajor(lmax): at trig[l * trig_stride + 2 (m - 2)],
                        // else at trig[(m - 2) * trig_stride + 2 l]
  int trig_stride;      // doubles between consecutive azimuths (l-major: 2 (lmax - 1)) / orders (m-major: 4 nq)
  int nq;
  // outputs / flags
  double* ev;           // 7 doubles or null: where tally_reduce_kernel adds the sums of pair_ev (the pair kernels do not touch it)
  double* pair_ev;      // eflag / vflag: 8 doubles per slot, E xx yy zz xy xz yz -, zeroed before the launch; or null
  double* pair_out;     // 7 doubles per slot or null
  double* pair_ft;      // deterministic mode (det_kernels.hpp): 12 doubles per slot, F_i tau_i | F_j tau_j, written instead
                        // of the atomics; null in the default mode
  unsigned char* flags;  // per slot: 1 = contact pair, 2 = touching pair; or null (stats only)
  int eflag;
  int vflag;
  unsigned long long* dbg;  // SHP_STATS builds only: work counters (tools/kernel_stats.py)
};

constexpr int kPairErrShape = 1;  // a shape index outside [0, nshapes) reached the kernel: the pair was skipped
constexpr int kPairErrType = 2;   // an atom type outside [1, ntypes]
constexpr int kPairErrCoincident = 4;   // two centres coincide (rho = 0) or their separation is not a number: SPEC §2 step 1
constexpr int kPairErrWall = 8;   // a particle centre at or behind a wall (h <= 0 or not a number): SPEC §2.9; raised by wall_kernels.hpp only
constexpr int kPairErrCylinder = 16;   // a particle centre at or outside a cylinder (d >= Rc or not a number): SPEC §2.18; raised by cylinder_kernels.hpp only
constexpr int kPairErrCone = 32;   // a particle centre at or outside a cone, or behind its apex (h <= 0 or not a number): SPEC §2.22; raised by cone_kernels.hpp only

// docs/SPEC.md §2.6: residual below which the inverse-quadratic extrapolation is accepted
#ifndef SHP_TAU3
#define SHP_TAU3 1e-4
#endif

__host__ __device__ constexpr int frj(const int slot) { return slot >= 36 ? slot - 18 : slot - 12; }
constexpr int kRecStride = 40;   // doubles per pair record: the first kRecUsed are copied into the frame
constexpr int kRecUsed = 40;
// per-pair scalars live in the frame too: as VALU results they would sit in VGPR pairs for
// the whole kernel (wave-uniform FP64 values cannot be SGPRs without readfirstlane)
// With P.jpoly the six slots of FR_BJ1 / FR_BJ2 carry cos, sin of the Euler angles of j's frame M_j = [BJ1 BJ2 BJC]
// instead (FR_EULERJ): the compiled orders never form a direction in j's body frame.
enum { FR_EULERJ = 0, FR_JPJ = 6 /* rho^2 - R_j^2 */, FR_JTOL1 = 7 /* 1e-7 R_j */, FR_JTOL3 = 8 /* SHP_TAU3 R_j */,
       FR_JTINY = 9 /* 1e-14 R_j */ };   // ... and the slots of BJC, d_j these (pair_setup.hpp)
enum { FR_BJ1 = 0, FR_BJ2 = 3, FR_BJC = 6, FR_DJ = 9, FR_E1 = 12, FR_E2 = 15, FR_C = 18, FR_D = 21,
       FR_RJ = 24, FR_RJ2 = 25, FR_RHO2 = 26, FR_HW = 27, FR_HM = 28, FR_WSC = 29,
       FR_EULER = 30 /* cos, sin of alpha, beta, gamma */, FR_RHO = 36,
       // the force law's operands, looked up by the set-up kernel (pair_setup.hpp)
       FR_KN = 37, FR_EXPO = 38, FR_IJ = 39 /* i, j as two ints */ };

// Host-callable launcher and instance lookup, one each per compiled order (pair_kernels_inst.hip, pair_kernel.hpp).
typedef void (*pair_launch_fn)(const PairParams&, const ContactPlan&, bool needv, hipStream_t, hipEvent_t wait_before_contact);
typedef const void* (*pair_instance_fn)(const ContactPlan&, bool needv);

}  // namespace shp
