// shstep_state.hpp — the state behind include/shstep.h (integrator, ghosts, neighbour build, walls, dissipation), hung
// off the pair context on first use, and what shstep_api.hip, shstep_walls.hip and shstep_dissipation.hip (the kernel
// launches of this layer) share with each other and offer the run loops of shstep_run.cpp and shhalo_run.cpp.
// Internal: nothing here is part of the boundary.  Needs no kernel header.  What the three surface families (planar walls,
// cylinders, cones) share is surface_state.hpp's (work buffers, spring history) and surface_coefficients.hpp's (the record
// of the coefficients and the switches derived from it); the cylinder and the cone state are one ShellState, which the
// host layer of shell_host.hpp serves for both.
#pragma once
#include <vector>

#include "../../include/shstep.h"
#include "shpair_ctx.hpp"
#include "surface_coefficients.hpp"
#include "surface_state.hpp"

namespace shp {
// step_kernels.hpp, which only shstep_api.hip may include (its kernels are not templates: one definition per library)
struct BoxParams;

// planar walls (SPEC §2.9, wall_kernels.hpp): everything shstep_walls.hip keeps between calls
struct WallState {
  int nwalls = 0;
  DevBuf<double> d_walls;      // kWallStride doubles per wall
  SurfaceWork<unsigned> work;  // mask, queue, count; rows of 4 (E, force on the wall) and their block sums
  DevBuf<double> d_wout;       // per-wall totals: staging of the host form
  bool wall_called = false;    // a wall pass has been enqueued since the walls were set
  // The coefficients as the setters took them (zero after shstep_set_walls) and what they switch on: damping (SPEC
  // §2.10), friction (§2.11), history (§2.15: the pass is shstep_wall_contact_device), rolling or twisting resistance
  // (§2.17: the pass keeps work.rows and launches wall_roll_kernel).  One place installs a record (shstep_walls.hip), so
  // the friction and the spring setter give the same state in either order.
  SurfaceCoefficients coef;
  SurfaceSwitches on;
  DevBuf<double> d_wgamma;    // [nwalls] gamma_w; sized and zeroed by shstep_set_walls
  DevBuf<double> d_wfric;     // [2][nwalls] mu_w, gamma_t,w; allocated by the first setter that makes fric or hist
  DevBuf<double> d_wkt;       // [nwalls] k_t,w; allocated by the first setter that makes hist
  DevBuf<double> d_wroll;     // [4][nwalls] mu_r, gamma_r, mu_tw, gamma_tw; allocated by the first setter that makes roll
  // translating walls (SPEC §2.12)
  std::vector<double> h_normals;   // [nwalls][3] as shstep_set_walls took them: n_w.u_w is formed on the host
  DevBuf<double> d_wvel;           // kWallVelStride doubles per wall: u_w[3], n_w.u_w; allocated by the first shstep_set_wall_velocity that sets one
  bool wall_move_on = false;       // some u_w != 0: with a wall coefficient set, the moving kernel instances run
  bool wall_advance_on = false;    // some n_w.u_w != 0: shstep_advance_walls_device enqueues its kernel
  // energy ledger (SPEC §2.13): while it is on the pass always keeps work.rows, and its LEDGER instances fill d_wprows
  DevBuf<double> d_wprows;         // [nlocal][nwalls][2] P_d, P_f
  DevBuf<double> d_wlpart;         // block sums of the fold's first stage, kLedgerWallTerms per (wall, block)
  bool ledger_fresh = false;       // a wall pass has left rows the fold has not added yet ...
  int ledger_nlocal = 0;           // ... over this many particles ...
  bool ledger_power = false;       // ... and its instance wrote d_wprows (a wall coefficient is set)
  // tangential springs with history (SPEC §2.15)
  SurfaceHistory<unsigned, 3> hist;   // xi_iw, a space-frame vector, and the live words
};

// An axial shell family, cylindrical (SPEC §2.18) or conical (§2.22) container walls: everything the host layer of
// shell_host.hpp keeps between calls, once for both.  W is the doubles of spring history per (particle, surface).  Nothing
// is allocated while no surface is set.  Every table of the record has a setter in either family and every switch can
// come on: damping and friction (the dissipative instance), history (§2.19, §2.23: the pass is the call with a time step),
// rolling or twisting resistance (§2.21, §2.24: the pass keeps work.rows and launches the roll kernel).  One place installs
// a record (install_shell_coefficients), so the friction and the spring setter give the same state in either order.
template <int W>
struct ShellState {
  int n = 0;
  std::vector<double> h_surf;      // the family's stride of doubles per surface as its geometry setter took them (the geometry never moves)
  DevBuf<double> d_surf;           // the same on the device
  SurfaceCoefficients coef;        // as the setters took them (zero after the geometry setter)
  SurfaceSwitches on;              // what they switch on
  DevBuf<double> d_coef;           // [4][n] gamma, mu, gamma_t, Omega; sized and zeroed by the geometry setter
  DevBuf<double> d_kt;             // [n] k_t; allocated by the first setter that makes hist
  DevBuf<double> d_roll;           // [4][n] mu_r, gamma_r, mu_tw, gamma_tw; allocated by the first setter that makes roll
  SurfaceWork<unsigned char> work; // mask, queue, count; rows of 5 (E, force on the wall, M_ax) and their block sums
  bool called = false;             // a pass has been enqueued since the surfaces were set
  SurfaceHistory<unsigned char, W> hist;   // tangential springs with history: xi in surface coordinates, and the live words
};

// cylinders (cylinder_kernels.hpp; shstep_cylinders.hip): xi is (xi_a, xi_theta).  On top of the shell, the cylinder
// entries of the energy ledger (SPEC §2.20, cyl_power_kernels.hpp): a switch of its own; nothing below is allocated,
// zeroed or launched while it is off
struct CylState : ShellState<2> {
  bool shell_ledger_on = false;    // shstep_set_shell_ledger: a coefficient and the energy ledger may be on together
  DevBuf<double> d_shell;          // the shell accumulator, kShellDoubles: (D_d, D_f, W), then three per cylinder; kept when switched off
  DevBuf<double> d_cprows;         // [nlocal][ncyl][3] P_d, P_f, Wdot_c: written by the LEDGER instances only
  DevBuf<double> d_cppart;         // block sums of the fold's first stage, 3 per (cylinder, block)
  bool shell_fresh = false;        // a cylinder pass has left power rows the fold has not added yet ...
  int shell_nlocal = 0;            // ... over this many particles
};

// cones (cone_kernels.hpp; shstep_cones.hip): xi is (xi_g, xi_theta, phi_c), surface components and the azimuth they
// belong to.  Cones keep no ledger entries.
struct ConeState : ShellState<3> {};
}  // namespace shp

struct shstep_state {
  shp::BoxParams* box = nullptr;   // made and deleted with the state (shstep_api.hip)
  bool have_box = false;
  double skin = 0.0;

  shp::DevBuf<double> d_mass;  // kMassStride doubles per shape
  std::vector<double> h_mass;

  shp::DevBuf<int> d_flags;   // [0] error bits, [1] moved flag
  shp::PinBuf<int> h_flags;   // 4 ints

  // borders
  shp::DevBuf<int> d_cnt, d_goff, d_sums, d_gowner, d_gcode;
  int b_nlocal = 0, nghost = 0;
  // bins + list
  shp::DevBuf<int> d_cell, d_cellcount, d_cellstart, d_atoms, d_nn, d_offs;
  shp::DevBuf<int> d_part_i, d_part_j, d_part_scan;   // "halo_overlap": the row-major list (kept for shstep_copy_neighbors) / scan scratch
  bool partitioned = false;
  shp::DevBuf<double> d_xhold;
  int l_nlocal = -1;

  // staging of the host-pointer integrator
  shp::DevBuf<double> s_x, s_v, s_q, s_L, s_f, s_t;
  shp::DevBuf<int> s_sh, s_mask;

  shp::WallState walls;
  shp::CylState cyl;
  shp::ConeState cone;

  // contact dissipation (SPEC §2.10, §2.11; dissipation_kernels.hpp)
  shp::DevBuf<double> d_twist;     // the run loop's twists, 6 doubles per row (owned + ghost)

  // energy ledger (SPEC §2.13): kLedgerDoubles time integrals, 5 totals then 3 per wall; unallocated until the first
  // shstep_set_energy_ledger(on)
  shp::DevBuf<double> d_ledger;
};

namespace shp {
// shstep_api.hip
int step_state(shpair_ctx* c, shstep_state** out);         // the context's state, made on first use
int step_refresh_mass(shpair_ctx* c, shstep_state* s);     // rigid-body table, when shapes or densities changed
int step_refresh_box(shpair_ctx* c, shstep_state* s);      // ghost cutoff and bin grid
// shstep_dissipation.hip, around a device build while a tangential spring is set (SPEC §2.14).  Ahead of it: swaps the
// installed list's offsets, keys and xi into the "old" buffers; returns its slot count if its xi can be carried (a
// device-built list of the same nlocal with a live history), else -1.  Behind the row-major fill: the keys of the new
// slots, and their xi carried from the old rows (old_np >= 0) or zeroed.
int step_history_put_aside(shpair_ctx* c, shstep_state* s, int nlocal);
int step_history_carry(shpair_ctx* c, shstep_state* s, int nlocal, int np, const int* tag, int old_np, hipStream_t st);
// shstep_dissipation.hip: the common part of every pair setter of this layer (shstep_rolling.hip's too): validates,
// fills the ntab symmetric host tables of `host`, replaces the device copy and recomputes `on` (blocks)
int set_pair_coefficients(shpair_ctx* c, const char* what, int itype, int jtype, int ntab, const double* vals,
                          const char* const* names, std::vector<double>& host, DevBuf<double>& dev, bool& on);
// shstep_walls.hip
int step_size_wall_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out);
// a wall coefficient is set: the wall pass reads the twists (no step state yet, before any shstep_* call: none is)
inline bool step_wall_reads_twists(const shpair_ctx* c)
{
  return c->step && c->step->walls.on.any();
}
// a wall has rolling or twisting resistance (SPEC §2.17): the wall pass keeps its (E, F_w) rows, whoever asks for wall_out
inline bool step_wall_rolling(const shpair_ctx* c) { return c->step && c->step->walls.on.roll; }
// a wall has a tangential spring (SPEC §2.15): the wall pass of the loops is shstep_wall_contact_device with the step's dt
inline bool step_wall_history(const shpair_ctx* c) { return c->step && c->step->walls.on.hist; }
// ahead of a capture: sizes xi and the live words for nlocal rows and, if they are keyed by another nlocal, starts them
// from nothing live (blocks), so that the captured pass neither allocates nor zeroes
int step_bind_wall_history(shpair_ctx* c, shstep_state* s, int nlocal);
// a wall has a normal velocity: the loops advance the planes ahead of the wall pass
inline bool step_walls_advance(const shpair_ctx* c) { return c->step && c->step->walls.nwalls > 0 && c->step->walls.wall_advance_on; }
// shstep_cylinders.hip
int step_size_cyl_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out);
// a cylinder is set (SPEC §2.18): the single-rank loops run the cylinder pass behind the planar wall pass
inline bool step_has_cylinders(const shpair_ctx* c) { return c->step && c->step->cyl.n > 0; }
// a cylinder coefficient is set: the cylinder pass is the dissipative instance, or the one with springs, or launches
// cyl_roll_kernel (SPEC §2.21), and reads the twists
inline bool step_cyl_reads_twists(const shpair_ctx* c)
{
  return c->step && c->step->cyl.on.any();
}
// a cylinder has rolling or twisting resistance (SPEC §2.21): the cylinder pass keeps its rows, whoever asks for cyl_out
inline bool step_cyl_rolling(const shpair_ctx* c) { return c->step && c->step->cyl.on.roll; }
// a cylinder has a tangential spring (SPEC §2.19): the cylinder pass of the loops is shstep_cyl_contact_device with the step's dt
inline bool step_cyl_history(const shpair_ctx* c) { return c->step && c->step->cyl.on.hist; }
// ahead of a capture: sizes (xi_a, xi_theta) and the live words for nlocal rows and, if they are keyed by another nlocal,
// starts them from nothing live (blocks), so that the captured pass neither allocates nor zeroes
int step_bind_cyl_history(shpair_ctx* c, shstep_state* s, int nlocal);
// the shell ledger is on (SPEC §2.20): the energy ledger and a cylinder coefficient may be set together
inline bool step_shell_ledger(const shpair_ctx* c) { return c->step && c->step->cyl.shell_ledger_on; }
// the part of shstep_ledger_fold_device for the cylinders: dt times the fresh power rows into the shell accumulator
int step_fold_shell_rows(shpair_ctx* c, shstep_state* s, double dt, hipStream_t st);
// shstep_cones.hip
int step_size_cone_buffers(shpair_ctx* c, shstep_state* s, int nlocal, bool want_out);
// a cone is set (SPEC §2.22): the single-rank loops run the cone pass behind the cylinder pass
inline bool step_has_cones(const shpair_ctx* c) { return c->step && c->step->cone.n > 0; }
// a cone coefficient is set: the cone pass is the dissipative instance, or the one with springs, or launches
// conic_roll_kernel (SPEC §2.24), and reads the twists
inline bool step_cone_reads_twists(const shpair_ctx* c) { return c->step && c->step->cone.on.any(); }
// a cone has rolling or twisting resistance (SPEC §2.24): the cone pass keeps its rows, whoever asks for cone_out
inline bool step_cone_rolling(const shpair_ctx* c) { return c->step && c->step->cone.on.roll; }
// a cone has a tangential spring (SPEC §2.23): the cone pass of the loops is shstep_conic_contact_device with the step's dt
inline bool step_cone_history(const shpair_ctx* c) { return c->step && c->step->cone.on.hist; }
// ahead of a capture: sizes (xi_g, xi_theta, phi_c) and the live words for nlocal rows and, if they are keyed by another
// nlocal, starts them from nothing live (blocks), so that the captured pass neither allocates nor zeroes
int step_bind_conic_history(shpair_ctx* c, shstep_state* s, int nlocal);
// a cone coefficient (the kinds of §2.24 among them, through on.any()), a cone spring or a non-zero Omega is set: what the energy ledger, which keeps no cone entries, refuses
inline bool step_cone_dissipates(const shpair_ctx* c)
{
  if (!c->step) return false;
  if (c->step->cone.on.any()) return true;
  for (const double o : c->step->cone.coef.Omega)
    if (o != 0.0) return true;
  return false;
}
// a dissipation coefficient is set, pair, wall, cylinder or cone: the loops compute twists
inline bool step_has_dissipation(const shpair_ctx* c)
{
  return shp_keeps_integrals(c) || step_wall_reads_twists(c) || step_cyl_reads_twists(c) || step_cone_reads_twists(c);
}
// ... a friction coefficient among them
inline bool step_has_friction(const shpair_ctx* c) { return c->fric_on || (c->step && c->step->walls.on.fric); }
// Neighbor::check_distance against the positions of the last build: clears the moved flag and enqueues the test;
// read_back: the error and moved words follow into h_flags[0..1] on the same stream
int step_enqueue_displacement(shpair_ctx* c, shstep_state* s, int nlocal, const double* x, bool read_back, hipStream_t st);
// once a read-back of h_flags[0] has landed: clears the device word and reports what the step kernels raised
int step_decode_flags(shpair_ctx* c, shstep_state* s, hipStream_t st);
}  // namespace shp

#define STEP_PROLOGUE(c)                     \
  if (!(c)) return SHPAIR_EINVAL;            \
  shstep_state* s = nullptr;                 \
  RC(shp::step_state((c), &s));              \
  HIPCHK((c), hipSetDevice((c)->device))
