/*
 * shstep.h — C ABI of the steps either side of the `pair_style sh` contact path (SURVEY.md §8f rows 2
 * and 4): the rigid-body integrator of SH particles, gravity/viscous body forces, and — for a host
 * that keeps its atoms resident in HBM — periodic ghosts and the binned half neighbour list built on
 * the device.  Same library (libshpair.so), same context and conventions as include/shpair.h.
 *
 * Reference citations: the fork's `fix nve/sh`-style integrator and its neighbour code are ABSENT
 * FROM MOUNT (/root/reference/README.md:1 is the whole reference), so each entry point
 * names the stock LAMMPS interface it serves (Fix::initial_integrate / final_integrate / post_force,
 * Comm::borders / forward_comm / reverse_comm, Neighbor::build / check_distance) instead of a
 * file:line.  The algorithm is docs/SPEC.md Part II.  LAMMPS-side adapter of the integrator:
 * lammps-spherharm_amd/lammps/fix_nve_sh.{h,cpp}.
 *
 * All *_device functions take device pointers, enqueue on `stream` (NULL = HIP's null stream) and
 * return without waiting unless stated otherwise.  There is no CPU fallback.
 */
#ifndef SHSTEP_H
#define SHSTEP_H

#include "shpair.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- rigid-body properties (SPEC §5) -------------------------------------- */

/* Stateless host helper: out[10] = V, c[3], J_c (xx,yy,zz,xy,xz,yz) of a shape at unit density,
 * body frame (what the reference's atom style would hold per shape). */
int shstep_shape_mass_props(int lmax, const double *anm, double *out);

/* Density of shape `ishape` (default 1).  After shpair_set_shape(). */
int shstep_set_density(shpair_ctx *ctx, int ishape, double rho);

/* mass, centre of mass (body frame) and inertia about it (xx,yy,zz,xy,xz,yz) of a shape; any output
 * may be NULL.  What a LAMMPS fix needs for rmass / `compute erotate`. */
int shstep_get_body(const shpair_ctx *ctx, int ishape, double *mass, double *com, double *inertia);

/* ---- Fix::initial_integrate / final_integrate (SPEC §6) ------------------- */

/* phase 0: initial_integrate (half kick, drift, quaternion update); phase 1: final_integrate (half
 * kick).  Particles with (mask[i] & groupbit) == 0 are untouched.  x, v, angmom: [n][3]; quat: [n][4]
 * (w,x,y,z); v is the velocity of the centre of mass, angmom is about it, space frame. */
int shstep_nve_device(shpair_ctx *ctx, int phase, int nlocal, double dt, double *x_dev, double *v_dev,
                      double *quat_dev, double *angmom_dev, const double *f_dev, const double *torque_dev,
                      const int *shtype_dev, const int *mask_dev, int groupbit, void *stream);

/* Host-pointer form for a CPU-resident LAMMPS (stages through the device, blocks). */
int shstep_nve(shpair_ctx *ctx, int phase, int nlocal, double dt, double *x, double *v, double *quat,
               double *angmom, const double *f, const double *torque, const int *shtype, const int *mask,
               int groupbit);

/* Verlet::force_clear: zeroes f and torque of nall atoms (owned + ghost) in one launch on `stream`. */
int shstep_force_clear_device(shpair_ctx *ctx, int nall, double *f_dev, double *torque_dev, void *stream);

/* Fix::post_force of `fix gravity` + `fix viscous` in one pass: f += m g - gamma_t v,
 * torque += s x (m g - gamma_t v) - gamma_r omega  (s = R c: both act at the centre of mass). */
int shstep_post_force_device(shpair_ctx *ctx, int nlocal, const double *gravity3, double gamma_t, double gamma_r,
                             const double *v_dev, const double *quat_dev, const double *angmom_dev,
                             const int *shtype_dev, const int *mask_dev, int groupbit, double *f_dev,
                             double *torque_dev, void *stream);

/* `compute ke` / `compute erotate` / gravitational potential: ADDS into out3_dev[0..2] (device):
 * sum 1/2 m v^2, sum 1/2 omega.L, sum -m g.(x + s). */
int shstep_energies_device(shpair_ctx *ctx, int nlocal, const double *gravity3, const double *x_dev,
                           const double *v_dev, const double *quat_dev, const double *angmom_dev,
                           const int *shtype_dev, const int *mask_dev, int groupbit, double *out3_dev,
                           void *stream);

/* ---- Domain / Comm / Neighbor for a device-resident host (SPEC §7) --------- */

/* Orthogonal box, per-dimension periodic flags, neighbour skin. */
int shstep_set_box(shpair_ctx *ctx, const double *lo3, const double *hi3, const int *periodic3, double skin);

/* Domain::pbc + Comm::borders: wraps the owned rows of x into the box and appends the periodic images
 * as ghost rows nlocal .. nlocal+nghost-1 of x, quat, type, shtype and tag (arrays sized for nmax
 * rows; tag may be NULL = tag is the row index).  Blocks (nghost is read back).  Fails with
 * SHPAIR_ENOMEM if nlocal + nghost > nmax (nghost is still returned). */
int shstep_borders_device(shpair_ctx *ctx, int nlocal, int nmax, double *x_dev, double *quat_dev, int *type_dev,
                          int *shtype_dev, int *tag_dev, int *nghost, void *stream);

/* Comm::forward_comm: ghost x = owner x + shift, ghost quat = owner quat. */
int shstep_forward_device(shpair_ctx *ctx, double *x_dev, double *quat_dev, void *stream);
/* Comm::reverse_comm: owner f, torque += ghost f, torque. */
int shstep_reverse_device(shpair_ctx *ctx, double *f_dev, double *torque_dev, void *stream);

/* Neighbor::build: bins owned + ghost particles and builds the SPEC §7 half list on the device, installs
 * it as the context's neighbour list (as shpair_set_neighbors_device would) and records x for the
 * rebuild test.  tag may be NULL (row index; ghosts then use their owner's index).  Blocks (npairs is
 * read back). */
int shstep_neighbor_build_device(shpair_ctx *ctx, int nlocal, int nghost, const double *x_dev, const int *shtype_dev,
                                 const int *tag_dev, int *npairs, void *stream);

/* Neighbor::check_distance: *rebuild = 1 if an owned particle moved more than skin/2 since the last
 * build.  Blocks (one flag is read back). */
int shstep_neighbor_check_device(shpair_ctx *ctx, int nlocal, const double *x_dev, int *rebuild, void *stream);

/* Copies the current device-built list to the host in CSR form: offsets[nlocal+1], jlist[npairs]
 * (either may be NULL).  Blocks. */
int shstep_copy_neighbors(shpair_ctx *ctx, int *offsets, int *jlist);

/* ---- planar walls (SPEC §2.9): Fix::post_force of a `fix wall/gran`-style fix --- */

#define SHSTEP_MAX_WALLS 32

/* Planes the particles rest against, fixed unless shstep_set_wall_velocity gives them a velocity
 * (SPEC §2.12): the pair contact of SPEC §2 with particle j replaced by a half-space.  plane4[4w..] = nx, ny, nz, c of wall w: unit normal pointing INTO the domain, the wall
 * occupies n.p < c; kn[w], exponent[w] its force law (SPEC §2.7).  nwalls = 0 removes all walls.
 * SHPAIR_EINVAL for more than SHSTEP_MAX_WALLS walls, |n| off 1 by more than 1e-12, a number that is
 * not finite, kn < 0 or exponent < 1.  Walls always use the sharp rule: the "rule weighted" setting
 * of the pair path does not change them.  Blocks (the table is replaced). */
int shstep_set_walls(shpair_ctx *ctx, int nwalls, const double *plane4, const double *kn, const double *exponent);

/* ADDS the wall forces and torques (about x_i, like the pair path) to the owned rows with
 * (mask[i] & groupbit) != 0.  wall_out_dev is nullable: 4 doubles per wall, E_w and Fx, Fy, Fz of
 * the force ON the wall (the scalar and vector a LAMMPS `fix wall/...` reports), ADDED, summed in a
 * fixed order: bitwise reproducible with or without the "deterministic" option, as are f and torque
 * (one wave per particle adds its total with one plain store; no atomics).  A particle whose centre
 * is at or behind a plane contributes nothing for that wall and raises a device error bit:
 * SHPAIR_EINVAL ("particle centre behind a wall") from the call that next reads the error word
 * (shstep_wall_force, shstep_get_wall_stats, shpair_synchronize, the run loops, ...).
 * No read-back, no blocking call; its work buffers only grow, so one call ahead of a stream capture
 * (same nlocal, same wall_out != NULL) makes it capturable. */
int shstep_wall_force_device(shpair_ctx *ctx, int nlocal, const double *x_dev, const double *quat_dev,
                             const int *shtype_dev, const int *mask_dev, int groupbit, double *f_dev,
                             double *torque_dev, double *wall_out_dev, void *stream);

/* Host-pointer form for a CPU-resident LAMMPS (stages through the device, blocks); wall_out is
 * nullable, 4 doubles per wall, ADDED. */
int shstep_wall_force(shpair_ctx *ctx, int nlocal, const double *x, const double *quat, const int *shtype,
                      const int *mask, int groupbit, double *f, double *torque, double *wall_out);

/* Particle/wall contacts with V > 0 of the last wall pass.  Blocks. */
int shstep_get_wall_stats(shpair_ctx *ctx, int *ncontacts);

/* ---- translating walls (SPEC §2.12): pistons, lifting floors, belts ---------- */

/* vel3[3w..] = u_w, the constant translation velocity of wall w in the space frame: any finite vector,
 * default 0.  The normal never changes and there is no rotation.  The plane moves by its normal part
 * only, c_w += dt (n_w.u_w) per advance, with n_w.u_w formed once, here; a tangential u_w (n_w.u_w = 0)
 * never moves the plane: a belt.  The elastic contact sees the wall through c_w alone; damping and
 * friction see the particle's twist with u_w taken off its linear part (below).  Call it after
 * shstep_set_walls, which resets every u_w to 0; nwalls must match.  SHPAIR_EINVAL for a component that
 * is not finite.  With every u_w = 0 and none set before, nothing is allocated.  Blocks.
 * The power the wall delivers to the bed is -F_w.u_w, F_w the force ON the wall in wall_out; the energy ledger below
 * integrates it. */
int shstep_set_wall_velocity(shpair_ctx *ctx, int nwalls, const double *vel3);

/* One advance of the planes by dt: c_w += dt (n_w.u_w), one small kernel on `stream` that updates the
 * device wall table in place.  The plane position is this accumulation, not c_0 + k dt (n.u).  No
 * read-back, no allocation: capturable.  Nothing is enqueued while no wall has a normal velocity.
 * SHPAIR_EINVAL for a dt that is not finite.  The run loops call it ahead of the wall pass of every
 * step (the positions there are x(t + dt)); a host that drives the step itself does the same.  A wall
 * that runs over a particle's centre raises the "particle centre behind a wall" error of the wall pass. */
int shstep_advance_walls_device(shpair_ctx *ctx, double dt, void *stream);

/* The current planes, plane4_out[4w..] = nx, ny, nz, c (for restarts); nwalls must match.  Blocks. */
int shstep_get_walls(shpair_ctx *ctx, int nwalls, double *plane4_out);

/* ---- volume-rate contact damping (SPEC §2.10) ------------------------------ */

/* Normal dissipation of a contact, defined on the integrals the contact kernels leave per list slot: with the twist
 * (w, omega) of a particle — the velocity of its SH origin, w = v - omega x (R c), and its angular velocity — the rate of
 * the overlap volume of pair (i, j) is Vdot = S_n.(w_i - w_j) + T_n.omega_i - (T_n - d x S_n).omega_j, the contact
 * pressure becomes p_tot = max(0, p + gamma_ij Vdot), and the pass adds the wrench of delta = p_tot - p with the
 * structure of the elastic one (momentum and angular momentum conserved exactly, power -delta Vdot <= 0, no pull).
 * No friction, no tangential force; the energy / virial tallies do not include it.
 *
 * gamma_ij >= 0 per type pair, symmetric, default 0.  SHPAIR_EINVAL for a type outside [1, ntypes] or a gamma that is
 * negative or not finite.  After shpair_set_ntypes(), which resets every gamma to 0.  While any gamma_ij != 0 every
 * compute zeroes and fills a per-slot integral buffer (56 B per slot; the caller's, if shpair_set_pair_output
 * installed one, which must then hold 7 doubles for every slot).  Blocks (the table is replaced). */
int shstep_set_pair_damping(shpair_ctx *ctx, int itype, int jtype, double gamma);

/* gamma_w >= 0 per wall: p_tot = max(0, p + gamma_w Vdot), Vdot = S_n.(w_i - u_w) + T_n.omega_i (u_w: the wall's
 * velocity, 0 unless shstep_set_wall_velocity set one).  Call it after shstep_set_walls, which resets every gamma_w to 0; nwalls must match.  Blocks. */
int shstep_set_wall_damping(shpair_ctx *ctx, int nwalls, const double *gamma);

/* twist[row][6] = w[3], omega[3] of the owned rows from v, angmom [nlocal][3], quat, shtype and the context's rigid-body
 * table; ghost rows nlocal .. nlocal+nghost-1 of the last shstep_borders_device take their owner's six numbers (images
 * move with their owners).  nghost = 0: owned rows only — a host with ghosts of its own fills those rows itself (over
 * several ranks: shhalo_forward_twist_device of include/shhalo.h, which is what shhalo_run_device does with option
 * "halo_twists"). */
int shstep_twist_device(shpair_ctx *ctx, int nlocal, int nghost, const double *v_dev, const double *quat_dev,
                        const double *angmom_dev, const int *shtype_dev, double *twist_dev, void *stream);

/* ADDS the damping wrench of the integrals of the last shpair_compute_device on the installed list to f and torque
 * (ghost rows included; j gets its share when newton_pair is set or j < nlocal, as in the compute).  The velocities are
 * what `twist` holds.  With the "deterministic" option the pass writes 12 doubles per slot and the ordered gather adds
 * them: bitwise reproducible.  Nothing is launched while every gamma_ij is 0.  SHPAIR_EINVAL if no compute has run on
 * the installed list since damping was switched on.  Allocation-free after a first call with the same list size. */
int shstep_pair_damping_device(shpair_ctx *ctx, int nlocal, int nghost, const double *x_dev, const int *type_dev,
                               const double *twist_dev, int newton_pair, double *f_dev, double *torque_dev, void *stream);

/* shstep_wall_force_device with wall damping: twist_dev[nlocal][6] as shstep_twist_device writes it.  With every
 * gamma_w = 0 it is shstep_wall_force_device bit for bit (twist_dev is not read and may be NULL), whatever the walls'
 * velocities; while a u_w != 0 and a wall coefficient is set it launches the moving instance of the kernel; while a gamma_w is
 * set, shstep_wall_force_device and shstep_wall_force return SHPAIR_EINVAL ("wall damping needs the twist form").
 * E_w in wall_out stays kn V^m; the force on the wall is minus the damped force on the particles. */
int shstep_wall_force_damped_device(shpair_ctx *ctx, int nlocal, const double *x_dev, const double *quat_dev,
                                    const int *shtype_dev, const int *mask_dev, int groupbit, double *f_dev,
                                    double *torque_dev, double *wall_out_dev, const double *twist_dev, void *stream);

/* ---- Coulomb-capped tangential friction (SPEC §2.11) ----------------------- */

/* History-free friction (LAMMPS gran/hooke: no per-contact state), formed from the same per-slot integrals and twists as
 * the damping above.  The contact point of pair (i, j) is the point of the normal wrench's line of action — through
 * r_perp = S_n x T_n / |S_n|^2 from x_i, along S_n — nearest the radical plane of the two bounding spheres; with v_t the
 * part of the relative velocity there that is normal to S_n and N = p_tot |S_n| the normal load, the force on i is
 * F_t = -kappa v_t, kappa = gamma_t while gamma_t |v_t| <= mu N and mu N / |v_t| beyond, applied to both particles at
 * that one point: momentum and angular momentum conserved exactly, power -kappa |v_t|^2 <= 0, |F_t| <= mu N, nothing for
 * a common rigid motion or a clamped contact.  The energy / virial tallies do not include it.  No tangential history,
 * no rolling or twisting resistance.
 *
 * mu_ij >= 0 and gamma_t,ij >= 0 (force per velocity) per type pair, symmetric, default 0; a type pair has friction iff
 * both are non-zero.  Validated like shstep_set_pair_damping; after shpair_set_ntypes(), which resets them.  While any
 * pair has friction every compute keeps the per-slot integrals, as for a gamma_ij.  Blocks (the table is replaced). */
int shstep_set_pair_friction(shpair_ctx *ctx, int itype, int jtype, double mu, double gamma_t);

/* mu_w, gamma_t,w >= 0 per wall: the contact point is r_perp dropped onto the plane, v_t the in-plane part of the
 * particle's velocity there relative to the wall (w_i + omega_i x r_i - u_w), N = p_tot |S_n| with the wall's p_tot.  Call it after
 * shstep_set_walls, which resets both to 0; nwalls must match.  While a wall has friction
 * shstep_wall_force_damped_device runs the friction instance, and shstep_wall_force_device / shstep_wall_force return
 * SHPAIR_EINVAL ("wall friction needs the twist form").  The force on the wall in wall_out is minus the whole force on
 * the particles, friction included; E_w stays kn V^m.  Blocks. */
int shstep_set_wall_friction(shpair_ctx *ctx, int nwalls, const double *mu, const double *gamma_t);

/* shstep_pair_damping_device with friction: ADDS the damping and the friction wrench of the integrals of the last
 * compute in one pass.  shtype_dev[nlocal + nghost] gives the bounding radii (not read, and may be NULL, while no pair
 * has friction: then the call IS shstep_pair_damping_device, bit for bit).  While a pair has friction
 * shstep_pair_damping_device returns SHPAIR_EINVAL and names this call.  Deterministic mode, "no compute has run" and
 * allocation as there. */
int shstep_pair_dissipation_device(shpair_ctx *ctx, int nlocal, int nghost, const double *x_dev, const int *type_dev,
                                   const int *shtype_dev, const double *twist_dev, int newton_pair, double *f_dev,
                                   double *torque_dev, void *stream);

/* ---- tangential contact springs with history (SPEC §2.14): static friction of pairs ---- */

/* LAMMPS gran/hooke/history for SH pairs on one rank: every slot of a list built by shstep_neighbor_build_device holds
 * xi, the accumulated tangential displacement of i's contact point relative to j's (space frame).  A pass with a time
 * step advances it by dt v_t, takes off its part along S_n, forms F* = -k_t xi - gamma_t v_t and caps it at mu N; a
 * sliding contact keeps the xi the capped force can hold.  Contact point, v_t, N and the wrench are §2.11's.  A slot that
 * is not touched, or fails §2.11's guards, or is clamped (N = 0), loses its xi.
 *
 * k_t,ij >= 0 (force per length) per type pair, symmetric, default 0; a type pair has history iff mu_ij != 0 and
 * k_t,ij != 0 (gamma_t,ij may then be 0); the other pairs keep §2.11.  Validated like shstep_set_pair_friction; after
 * shpair_set_ntypes(), which resets it and drops the history.  Set it ahead of the build of the list it is to act on.
 * While any k_t != 0: every compute keeps the per-slot integrals; every device build writes one int per slot (the tag
 * of j's owner) and 24 B of xi, carried from the previous device build's slots of the same (i, owner tag) if that had the
 * same nlocal, zero otherwise (the previous offsets, keys and xi are swapped into buffers that stay allocated: 56 B per
 * slot in all once a build has carried); installing a caller's list drops the history, and so does setting the last
 * k_t to 0 or the first one again: a list built meanwhile has no keys and is refused (SHPAIR_ESTATE) until the next build,
 * which starts from zero.  With every k_t = 0 and none set before, nothing is allocated, zeroed or launched.  Blocks. */
int shstep_set_pair_tangential_spring(shpair_ctx *ctx, int itype, int jtype, double kt);

/* shstep_pair_dissipation_device with the law above and its time step: dt > 0 advances and stores xi, dt = 0 forms the
 * forces from the stored xi and writes nothing (the set-up forces of Verlet::setup).  While no k_t is set the call IS
 * shstep_pair_dissipation_device, bit for bit; while one is set, shstep_pair_dissipation_device returns SHPAIR_EINVAL
 * and names this call.  SHPAIR_EINVAL for a dt that is negative or not finite.  SHPAIR_ESTATE if the installed list
 * was not built by shstep_neighbor_build_device (or was built before the spring was set), if option "halo_overlap"
 * partitioned it, or if no compute has run on it.  With the energy ledger on, the friction row of a history slot is
 * -F_t.v_t times the slot's share (negative while a spring unloads).  Allocation-free: the build sized what it needs. */
int shstep_pair_contact_device(shpair_ctx *ctx, int nlocal, int nghost, const double *x_dev, const int *type_dev,
                               const int *shtype_dev, const double *twist_dev, int newton_pair, double dt, double *f_dev,
                               double *torque_dev, void *stream);

/* xi of the installed list to / from the host, npairs x 3 doubles in the slot order of shstep_copy_neighbors (restarts,
 * tests).  SHPAIR_ESTATE without a device-built list or without a k_t.  Both block. */
int shstep_copy_contact_history(shpair_ctx *ctx, double *xi3);
int shstep_set_contact_history(shpair_ctx *ctx, const double *xi3);

/* Zeroes every xi of the installed list (nothing to do where none is held).  Blocks. */
int shstep_reset_contact_history(shpair_ctx *ctx);

/* ---- tangential contact springs with history at planar walls (SPEC §2.15): static friction at walls ---- */

/* The law of §2.14 in the wall form of §2.11 and §2.12: every (owned particle i, wall w) holds xi_iw, the accumulated
 * tangential displacement of i's contact point relative to the wall's material (space frame), and one bit of a 32-bit
 * live word per particle; a xi whose bit is dead reads as 0.  Contact point, v_t (u_w taken off) and N are §2.11's and
 * §2.12's.  A pass with a time step advances xi by dt v_t, takes off its part along the wall normal, forms
 * F* = -k_t xi - gamma_t v_t and caps it at mu N; a sliding contact keeps the xi the capped force can hold.  The bit dies
 * where the wall is out of reach, V <= 0, |S_n| = 0 or N = 0 (a clamped contact).
 *
 * k_t,w >= 0 (force per length) per wall, default 0; a wall has history iff mu_w != 0 and k_t,w != 0 (gamma_t,w may then
 * be 0); the other walls keep §2.11 and §2.12 bit for bit.  Validated like shstep_set_wall_friction, and the two setters
 * give the same state in either order.  Call it after shstep_set_walls, which resets every k_t,w to 0 and drops the
 * history; nwalls must match.  Setting the last k_t to 0 (or the mu of the last history wall) drops the history too.
 * While a wall has history the wall pass keeps 24 nwalls + 4 B per owned particle, and shstep_wall_force_device,
 * shstep_wall_force and shstep_wall_force_damped_device return SHPAIR_EINVAL and name shstep_wall_contact_device.
 * xi is keyed by the row index (the single-rank loops never reorder owned rows): a pass over another nlocal than the
 * last advancing pass' starts from nothing live.  With every k_t = 0 and none set before, nothing is allocated.  Blocks. */
int shstep_set_wall_tangential_spring(shpair_ctx *ctx, int nwalls, const double *kt);

/* shstep_wall_force_damped_device with the law above and its time step: dt > 0 advances and stores xi and the live
 * words, dt = 0 forms the forces from the stored xi (projected and capped) and writes neither (the set-up forces of
 * Verlet::setup).  While no wall has history the call IS shstep_wall_force_damped_device, bit for bit, whatever dt.
 * SHPAIR_EINVAL for a dt that is negative or not finite, and for a NULL twist_dev while a wall has history.  With the
 * energy ledger on, the wall-friction power of a history wall is -F_t.v_t (negative while a spring unloads).  Its
 * buffers only grow, so one call ahead of a stream capture (same nlocal) makes it capturable. */
int shstep_wall_contact_device(shpair_ctx *ctx, int nlocal, const double *x_dev, const double *quat_dev,
                               const int *shtype_dev, const int *mask_dev, int groupbit, double *f_dev,
                               double *torque_dev, double *wall_out_dev, const double *twist_dev, double dt, void *stream);

/* xi of the walls to / from the host, [nlocal][nwalls][3] (restarts, tests).  The copy gives 0 where the bit is dead
 * (all of it while nothing is held); SHPAIR_EINVAL for another nlocal than the history is held for.  The set marks live
 * where any component is non-zero and keys the history by its nlocal (>= 1).  SHPAIR_ESTATE while no wall has history.
 * Both block. */
int shstep_copy_wall_history(shpair_ctx *ctx, int nlocal, double *xi_out);
int shstep_set_wall_history(shpair_ctx *ctx, int nlocal, const double *xi);

/* Drops every xi_iw: the next pass starts from nothing live (nothing to do where none is held).  Blocks. */
int shstep_reset_wall_history(shpair_ctx *ctx);

/* ---- rolling and twisting resistance of pairs (SPEC §2.16) ----------------- */

/* The two resisting couples of LAMMPS pair_style granular (rolling, twisting), history-free as §2.11 is to gran/hooke.
 * They act on the relative angular velocity Omega = omega_i - omega_j of a touched slot, split along the contact normal:
 * Omega_n = (Omega.S_n) S_n / |S_n|^2 (twisting) and Omega_r = Omega - Omega_n (rolling).  With N = p_tot |S_n| the
 * normal load of §2.11 (the p_tot of §2.10 where a gamma_ij is set), the torque on i is
 * M = -kappa_r Omega_r - kappa_tw Omega_n, kappa_r = gamma_r while gamma_r |Omega_r| <= mu_r N and mu_r N / |Omega_r|
 * beyond, kappa_tw alike; j takes -M.  A pure couple: no force, momentum and angular momentum conserved exactly,
 * power -kappa_r |Omega_r|^2 - kappa_tw |Omega_n|^2 <= 0, |M_r| <= mu_r N, |M_tw| <= mu_tw N, nothing for a common rigid
 * motion or a clamped contact; no contact point enters.  The energy / virial tallies do not include it.  No rolling or
 * twisting springs with history; the resistance at walls is §2.17's, further down.
 *
 * mu_r,ij >= 0 is a LENGTH (the arm of the resisting couple per unit normal load, the classical coefficient of rolling
 * friction) and gamma_r,ij >= 0 a torque per angular velocity, per type pair, symmetric, default 0; a type pair has
 * rolling resistance iff both are non-zero.  Validated like shstep_set_pair_friction; after shpair_set_ntypes(), which
 * resets them.  While any pair has one every compute keeps the per-slot integrals, as for a gamma_ij.  Blocks (the table
 * is replaced). */
int shstep_set_pair_rolling(shpair_ctx *ctx, int itype, int jtype, double mu_r, double gamma_r);

/* mu_tw,ij >= 0 (a length: 2/3 mu a for a Coulomb disc of radius a) and gamma_tw,ij >= 0 (torque per angular velocity):
 * twisting resistance, as shstep_set_pair_rolling. */
int shstep_set_pair_twisting(shpair_ctx *ctx, int itype, int jtype, double mu_tw, double gamma_tw);

/* ADDS the two couples of the integrals of the last compute to torque_dev (owned rows; ghost rows as
 * shstep_pair_damping_device takes newton_pair), in a pass of its own behind shstep_pair_dissipation_device /
 * shstep_pair_contact_device, which are what they are without it (with rolling or twisting alone they launch nothing).
 * Forces are not touched.  With neither kind set the call returns SHPAIR_OK and launches nothing.  Deterministic mode:
 * per-slot rows in the pair pass' row buffer and an ordered gather of the torques.  With the energy ledger on, its power
 * times the slot's share goes into totals5[1]: added to the power rows where shstep_pair_dissipation_device /
 * shstep_pair_contact_device has written them from the integrals of the same compute and no fold has taken them yet;
 * written as (0, share P) otherwise (no such pass exists or ran since that compute; rows an earlier call of THIS pass left
 * do not count and are overwritten, so a fold takes the last pass once, as for the pair pass).  One call per compute: a
 * second one behind the same pair pass adds its torques and its power again.  "No compute has run", stale list, changed
 * coefficients and allocation as shstep_pair_damping_device. */
int shstep_pair_rolling_device(shpair_ctx *ctx, int nlocal, int nghost, const double *x_dev, const int *type_dev,
                               const double *twist_dev, int newton_pair, double *torque_dev, void *stream);

/* ---- rolling and twisting resistance at planar walls (SPEC §2.17) ---------- */

/* The two couples above with a wall in the place of particle j (`fix wall/gran ... rolling ... twisting`): a wall does not
 * rotate, so Omega = omega_i (a wall velocity u_w does not enter), split along the exact wall normal n_w.  The normal load
 * is N = max(0, -n_w.F_w), F_w the whole force ON the wall from that particle as the wall pass leaves it per (particle,
 * wall) — friction and the tangential spring lie in the plane, so this is p_tot (-n_w.S_n), with the p_tot of whichever
 * wall coefficients are set.  M = -kappa_r Omega_r - kappa_tw Omega_n is added to the particle's torque; no force, and
 * wall_out keeps its bits.  Power <= 0, |M_r| <= mu_r N, |M_tw| <= mu_tw N, nothing for omega_i = 0, V <= 0 or a clamped
 * contact.
 *
 * mu_r,w >= 0 (a length) and gamma_r,w >= 0 (torque per angular velocity) per wall, default 0; a wall has rolling
 * resistance iff both are non-zero.  Validated like shstep_set_wall_friction (SHPAIR_EINVAL for a value that is negative
 * or not finite); call it after shstep_set_walls, which resets all four coefficients to 0; nwalls must match.  The device
 * table is allocated by the first call that sets a non-zero value.  While a wall has either kind: every wall pass reads
 * twist_dev (NULL: SHPAIR_EINVAL), keeps its 32 B rows per (particle, wall) whether or not wall_out is asked for, and
 * launches one more kernel behind the contact kernel, the same bits with and without "deterministic"; the run loops
 * compute twists; shstep_wall_force_device and shstep_wall_force return SHPAIR_ESTATE and name
 * shstep_wall_force_damped_device; shhalo_run_device needs option "halo_twists", as for any wall coefficient.  With the
 * energy ledger on, its power goes into the wall-friction entries (totals5[3] and per wall).  With every coefficient 0
 * and none set before, nothing is allocated, zeroed or launched.  Blocks. */
int shstep_set_wall_rolling(shpair_ctx *ctx, int nwalls, const double *mu_r, const double *gamma_r);

/* mu_tw,w >= 0 (a length) and gamma_tw,w >= 0 (torque per angular velocity): twisting resistance, as
 * shstep_set_wall_rolling. */
int shstep_set_wall_twisting(shpair_ctx *ctx, int nwalls, const double *mu_tw, const double *gamma_tw);

/* ---- energy ledger (SPEC §2.13): dissipated energy and wall work, kept on the device ---- */

/* Time integrals sum dt P of the five ways a bed exchanges energy with its contacts, with the velocities the force laws
 * themselves saw (the twists handed to the passes; in the run loops the half-step twists, at the positions x(t + dt)):
 *   totals5[0] pair damping     P_d = delta Vdot >= 0 (a clamped contact: p |Vdot|)
 *   totals5[1] pair friction    P_f = kappa |v_t|^2 >= 0
 *   totals5[2] wall damping     P_d = (p_tot - p) Vdot of the wall-relative twist
 *   totals5[3] wall friction    P_f = kappa |v_t|^2 of the wall-relative velocity at the contact point
 *   totals5[4] wall work        W_w = -F_w.u_w, F_w the whole force ON the wall as in wall_out (damping and friction included)
 * and per wall the last three (per_wall3[3w..] = damping, friction, work).  So E_mech(t) - E_mech(0) = W - D with
 * D = totals5[0] + ... + totals5[3], W = totals5[4], to first order in dt (SPEC §2.13).  A pair counts with the share of
 * the energy tally: 1 with newton_pair, else a half for i and a half for an owned j.  Over several ranks each rank's
 * ledger holds its share (its walls act on its owned particles, its list slots count once over all ranks): summing the
 * ranks is the caller's business.
 *
 * on != 0: allocates and zeroes the accumulator (5 + 3 SHSTEP_MAX_WALLS doubles) if the ledger was off; from then on
 * shstep_pair_dissipation_device leaves 16 B per list slot, and the wall pass always keeps its per-(particle, wall) rows
 * (also with wall_out = NULL) and 16 B more per row; these buffers are sized with the list and with the wall pass'
 * buffers.  on == 0: the passes are what they are without a ledger, bit for bit and launch for launch; nothing is freed
 * and the accumulator can still be read.  Strictly opt-in: default off.  Blocks. */
int shstep_set_energy_ledger(shpair_ctx *ctx, int on);

/* Adds dt times the powers the last shstep_pair_dissipation_device and the last wall pass left, and dt times -F_w.u_w of
 * that wall pass, into the accumulator: ordered sums over a partition fixed by the slot count and the particle count, no
 * atomics — bitwise reproducible with or without the "deterministic" option.  Each pass is folded at most once; a fold
 * with nothing fresh enqueues nothing.  No allocation, no read-back: capturable.  The run loops call it once per step
 * behind the wall pass while the ledger is on; a host that drives the step itself does the same.  SHPAIR_EINVAL for a
 * dt that is not finite, SHPAIR_ESTATE while the ledger is off. */
int shstep_ledger_fold_device(shpair_ctx *ctx, double dt, void *stream);

/* The accumulator: totals5[5] as above; per_wall3 is nullable, 3 doubles per wall (nwalls must then match the walls
 * set).  SHPAIR_ESTATE if the ledger was never switched on.  Blocks. */
int shstep_get_energy_ledger(shpair_ctx *ctx, double *totals5, int nwalls, double *per_wall3);

/* Zeroes the accumulator.  shstep_set_walls zeroes the three wall totals and every per-wall triple, as it resets every
 * wall coefficient.  Blocks. */
int shstep_reset_energy_ledger(shpair_ctx *ctx);

/* ---- cylindrical container walls (SPEC §2.18): drum, silo, triaxial cell ---------- */

#define SHSTEP_MAX_CYLINDERS 8

/* The INSIDE of circular cylinders as walls: the wall contact of §2.9 with the half-space replaced by the outside of a
 * cylinder.  cyl7[7c..] = a[3] (a point on the axis), axis[3] (unit vector), Rc (> 0) of cylinder c; kn[c], exponent[c]
 * its force law (SPEC §2.7).  The cylinder is infinite: close it with planes (shstep_set_walls).  The particles live
 * inside: a centre at or outside the wall (d >= Rc, d the distance from the axis, or not a number) contributes nothing
 * for that cylinder and raises a device error bit: SHPAIR_EINVAL ("particle centre outside a cylinder") from the call
 * that next reads the error word, as for the planes.  ncyl = 0 removes all cylinders.  Every call resets gamma_c, mu_c,
 * gamma_t,c, Omega, k_t,c and the four coefficients of §2.21 of the setters below to 0 and drops the history of §2.19.  SHPAIR_EINVAL for more than SHSTEP_MAX_CYLINDERS cylinders, an axis
 * whose length is off 1 by more than 1e-12, a number that is not finite, Rc <= 0, kn < 0 or exponent < 1.  Always the
 * sharp rule.  Not modelled: the outside of a cylinder, end caps, any motion but the rotation below,
 * a cylinder in the energy ledger unless the shell ledger is on (shstep_set_shell_ledger below), the
 * loop over several ranks (shhalo_run_device returns SHPAIR_ESTATE while a cylinder is set), a host-pointer form.  It also
 * zeroes the shell ledger's entries, as shstep_set_walls zeroes the wall entries.  Blocks. */
int shstep_set_cylinders(shpair_ctx *ctx, int ncyl, const double *cyl7, const double *kn, const double *exponent);

/* gamma_c >= 0 per cylinder: p_tot = max(0, p + gamma_c Vdot), Vdot = S_n.w_i + T_n.omega_i (the rotation does not enter:
 * a cylinder turning about its own axis changes no overlap).  After shstep_set_cylinders; ncyl must match.  While the
 * energy ledger is on a non-zero coefficient is SHPAIR_ESTATE (the ledger keeps no cylinder entries), and so is
 * switching the ledger on while one is set, unless the shell ledger is on (SPEC §2.20).  Blocks. */
int shstep_set_cylinder_damping(shpair_ctx *ctx, int ncyl, const double *gamma);

/* mu_c, gamma_t,c >= 0 per cylinder; a cylinder has friction iff both are non-zero: F_t = -kappa v_t at the point where
 * the normal wrench's line of action leaves the cylinder, v_t the tangential part of w_i + omega_i x r_i - Omega a x rho_c
 * there, kappa = gamma_t,c capped at mu_c N / |v_t|, N = p_tot |S_n|.  A cylinder of very large radius is NOT a plane with
 * shstep_set_wall_friction bit for bit, nor to rounding: the plane drops the line of action onto the wall along its
 * normal, the cylinder follows it along S_n, so the two contact points agree only as far as S_n is along the normal
 * (SPEC 2.18).  Otherwise as shstep_set_cylinder_damping. */
int shstep_set_cylinder_friction(shpair_ctx *ctx, int ncyl, const double *mu, const double *gamma_t);

/* Omega per cylinder, any finite value: the angular velocity of the cylinder about its own axis (right-handed about
 * axis[3]).  The geometry never moves; the rotation enters the friction, the springs of §2.19 and the couples of §2.21 only,
 * so without any of them it changes nothing.
 * After shstep_set_cylinders; ncyl must match.  Blocks. */
int shstep_set_cylinder_rotation(shpair_ctx *ctx, int ncyl, const double *omega);

/* ADDS the cylinder forces and torques (about x_i) to the owned rows with (mask[i] & groupbit) != 0; a particle in reach
 * of several cylinders adds them in index order.  cyl_out_dev is nullable: 5 doubles per cylinder, E_c, Fx, Fy, Fz of
 * the force ON the wall and M_ax = axis . sum_i [(x_i - a) x (-F_i) - tau_i], the moment of that force about the axis (the
 * drive torque of a drum balances it), ADDED, summed in a fixed order: the same bits with and without the
 * "deterministic" option.  twist_dev[nlocal][6] as shstep_twist_device writes it; it is read only while a cylinder has
 * damping or friction (NULL then: SHPAIR_EINVAL), and with every coefficient 0 the result is the same bits whatever it
 * is.  While a cylinder has rolling or twisting resistance (SPEC §2.21) it is read too (NULL: SHPAIR_EINVAL) and the
 * couples are added to torque_dev and to M_ax.  Two kernel launches and a memset (two more for cyl_out_dev), nothing read back; sizing it once (same nlocal, same
 * cyl_out_dev != NULL) makes it capturable.  With no cylinder set nothing is allocated, zeroed or launched.  While a
 * cylinder has a tangential spring (SPEC §2.19) it returns SHPAIR_EINVAL and names shstep_cyl_contact_device. */
int shstep_cylinder_force_device(shpair_ctx *ctx, int nlocal, const double *x_dev, const double *quat_dev,
                                 const int *shtype_dev, const int *mask_dev, int groupbit, double *f_dev,
                                 double *torque_dev, double *cyl_out_dev, const double *twist_dev, void *stream);

/* Particle/cylinder contacts with V > 0 of the last cylinder pass.  Blocks. */
int shstep_get_cylinder_stats(shpair_ctx *ctx, int *ncontacts);

/* The cylinders as set, cyl7_out[7c..] = a[3], axis[3], Rc (for restarts); ncyl must match. */
int shstep_get_cylinders(shpair_ctx *ctx, int ncyl, double *cyl7_out);

/* ---- tangential springs with history at the cylinders (SPEC §2.19): static friction at a drum or silo wall ---- */

/* The law of §2.15 at the contact point of shstep_set_cylinder_friction: every (owned particle i, cylinder c) holds two
 * doubles (xi_a, xi_theta), the accumulated tangential displacement of i's contact point relative to the wall's material
 * in the cylinder's own surface coordinates at the contact point, along the axis a and along t_c = a x rho_c / Rc (the
 * direction the wall moves for Omega > 0), and one bit of an 8-bit live word per particle; a xi whose bit is dead reads
 * as 0.  A cylinder is developable, so the two numbers are the exact parallel transport of the spring along the wall: a
 * particle carried round by the drum keeps them, and a screw motion of particle and wall about the axis leaves them
 * unchanged.  Contact point, v_t (Omega taken off) and N are §2.18's.  A pass with a time step advances them by
 * dt (v_t.a, v_t.t_c), forms F* = -k_t (xi_a a + xi_theta t_c) - gamma_t v_t and caps it at mu N; a sliding contact keeps the
 * xi the capped force can hold.  The bit dies where the cylinder is out of reach, V <= 0, |S_n| = 0, N = 0 or the contact
 * point does not exist (S_n along the axis, a line of action that misses the cylinder).  The totals rows stay minus the
 * whole force on the particle: M_ax contains the static load the drive holds.
 *
 * k_t,c >= 0 (force per length) per cylinder, default 0; a cylinder has history iff mu_c != 0 and k_t,c != 0 (gamma_t,c may
 * then be 0); the other cylinders keep §2.18 inside the same pass.  Validated like shstep_set_cylinder_friction, and the
 * two setters give the same state in either order.  Call it after shstep_set_cylinders, which resets every k_t,c to 0 and
 * drops the history; ncyl must match.  Setting the last k_t to 0 (or the mu of the last history cylinder) drops the
 * history too.  While a cylinder has history the pass keeps 16 ncyl + 1 B per owned particle, and
 * shstep_cylinder_force_device returns SHPAIR_EINVAL and names shstep_cyl_contact_device.  xi is keyed by the row index: a
 * pass over another nlocal than the last advancing pass' starts from nothing live.  With every k_t = 0 and none set
 * before, nothing is allocated.  SHPAIR_ESTATE while the energy ledger is on (and the ledger while a spring is set), like
 * every other cylinder coefficient, unless the shell ledger is on (SPEC §2.20).  Not modelled: the loop over several ranks, a host-pointer form.  Blocks. */
int shstep_set_cyl_tangential_spring(shpair_ctx *ctx, int ncyl, const double *kt);

/* shstep_cylinder_force_device with the law above and its time step: dt > 0 advances and stores xi and the live words,
 * dt = 0 forms the forces from the stored xi (capped) and writes neither (the set-up forces of Verlet::setup).  While no
 * cylinder has history the call IS shstep_cylinder_force_device, bit for bit, whatever dt, and nothing is allocated,
 * zeroed or launched on top.  SHPAIR_EINVAL for a dt that is negative or not finite, and for a NULL twist_dev while a
 * cylinder has history.  The couples of §2.21 are added by either form, and by a look (dt = 0) too: they have no state.
 * Its buffers only grow, so one call ahead of a stream capture (same nlocal) makes it capturable. */
int shstep_cyl_contact_device(shpair_ctx *ctx, int nlocal, const double *x_dev, const double *quat_dev,
                              const int *shtype_dev, const int *mask_dev, int groupbit, double *f_dev,
                              double *torque_dev, double *cyl_out_dev, const double *twist_dev, double dt, void *stream);

/* (xi_a, xi_theta) of the cylinders to / from the host, [nlocal][ncyl][2] (restarts, tests).  The copy gives 0 where the
 * bit is dead (all of it while nothing is held); SHPAIR_EINVAL for another nlocal than the history is held for.  The set
 * marks live where a component is non-zero and keys the history by its nlocal (>= 1).  SHPAIR_ESTATE while no cylinder
 * has history.  Both block. */
int shstep_copy_cyl_history(shpair_ctx *ctx, int nlocal, double *xi_out);
int shstep_set_cyl_history(shpair_ctx *ctx, int nlocal, const double *xi);

/* Drops every xi of the cylinders: the next pass starts from nothing live (nothing to do where none is held).  Blocks. */
int shstep_reset_cyl_history(shpair_ctx *ctx);

/* ---- the shell ledger (SPEC §2.20): the energy ledger's entries for the curved walls ---- */

/* Time integrals sum dt P of the three ways a bed exchanges energy with the shells of §2.18 and §2.19, with the
 * quantities the force law itself formed in the pass (the time level of the energy ledger):
 *   totals3[0] shell damping    P_d = (p_tot - p) Vdot >= 0 (a clamped contact: p |Vdot|)
 *   totals3[1] shell friction   P_f = kappa |v_t|^2 >= 0; for a shell with a tangential spring -F_t.v_t, negative while
 *                               the spring unloads (1/2 k_t (xi_a^2 + xi_theta^2) sits in the entry until released or slid away)
 *   totals3[2] drive work       W_c = Omega F_t.(a x rho_c) = Omega Rc F_t.t_c, the power the rotating shell delivers to the
 *                               bed; only friction does work, the normal wrench's axial moment in M_ax is quadrature noise
 * and per shell the same three (per_shell3[3c..]).  The bed's balance becomes E_mech(t) - E_mech(0) = (W + W_shell) -
 * (D + D_shell), to first order in dt, with W, D of shstep_get_energy_ledger.  The entries are kept apart from totals5.
 *
 * A switch of its own, default off; callable in any state.  on != 0 allocates and zeroes the shell accumulator
 * (3 + 3 SHSTEP_MAX_CYLINDERS doubles) if it was off.  While it is on, a shell coefficient or spring and the energy
 * ledger may be set together, in either order, and a shell pass with a coefficient leaves 24 B per (particle, shell) more
 * whenever the energy ledger is also on (its other outputs keep their bits); shstep_ledger_fold_device folds these rows
 * too, once per pass, in a fixed order and without atomics.  An elastic shell needs no switch.  on == 0: every refusal of
 * §2.18 and §2.19 is back; SHPAIR_ESTATE while the energy ledger is on and a shell coefficient or spring is set.  Nothing
 * is freed and the accumulator can still be read.  shstep_reset_energy_ledger zeroes the shell entries too, and
 * shstep_set_cylinders zeroes them as shstep_set_walls does the wall entries.  Blocks. */
int shstep_set_shell_ledger(shpair_ctx *ctx, int on);

/* The shell accumulator: totals3[3] as above; per_shell3 is nullable, 3 doubles per shell (ncyl must then match the
 * cylinders set: SHPAIR_EINVAL).  SHPAIR_ESTATE if the shell ledger was never switched on.  Blocks. */
int shstep_get_shell_ledger(shpair_ctx *ctx, double *totals3, int ncyl, double *per_shell3);

/* ---- rolling and twisting resistance at the cylinders (SPEC §2.21) ---------- */

/* The two couples of §2.17 at a shell.  Per owned particle i and cylinder c in its mask: F_w is the force ON the wall as
 * the cylinder pass leaves it per (particle, cylinder), minus the whole force on the particle; c^ = rho / d is the radial
 * direction through the particle's centre (on the axis: the e1 of the frame rule about the axis) and n = -c^ the shell's
 * exact inward normal there.  N = max(0, c^.F_w) is the radial load, Omega_rel = omega_i - Omega_c a the angular velocity
 * in the drum's frame (a particle carried rigidly round, omega_i = Omega_c a, feels exactly nothing), Omega_n =
 * (Omega_rel.c^) c^ and Omega_r = Omega_rel - Omega_n; a is normal to c^, so the drum's rotation only rolls, never twists.
 * M = -kappa_r Omega_r - kappa_tw Omega_n, either coefficient capped at mu N / |.|, is added to the particle's torque; no
 * force.  The couple on the shell is -M: M_ax of cyl_out gains -a.M, E_c and the force keep their bits.  The load is
 * radial, not along S_n: what that costs is measured in SPEC §2.21.
 *
 * mu_r,c >= 0 (a length) and gamma_r,c >= 0 (torque per angular velocity) per cylinder, default 0; a cylinder has rolling
 * resistance iff both are non-zero.  Validated like shstep_set_cylinder_friction; call it after shstep_set_cylinders,
 * which resets all four coefficients to 0; ncyl must match.  The device table is allocated by the first call that sets a
 * kind.  While a cylinder has either kind: every cylinder pass, of either form, reads twist_dev (NULL: SHPAIR_EINVAL),
 * keeps its 40 B rows per (particle, cylinder) whether or not cyl_out is asked for, and launches one more kernel behind
 * the contact kernel, no atomics, the same bits with and without "deterministic"; the run loops compute twists.
 * SHPAIR_ESTATE while the energy ledger is on (and the ledger while a kind is set), like every other cylinder
 * coefficient, unless the shell ledger is on: then P_roll = kappa_r |Omega_r|^2 + kappa_tw |Omega_n|^2 goes into the shell
 * friction entry and Wdot_roll = Omega_c (a.M) into the drive work, so that M.omega_i = -P_roll + Wdot_roll closes the
 * balance of §2.20.  With every coefficient 0 and none set before, nothing is allocated, zeroed or launched.  Not
 * modelled: rolling or twisting springs with history, the loop over several ranks, a host-pointer form.  Blocks. */
int shstep_set_rolling_cyl(shpair_ctx *ctx, int ncyl, const double *mu_r, const double *gamma_r);

/* mu_tw,c >= 0 (a length) and gamma_tw,c >= 0 (torque per angular velocity): twisting resistance, as
 * shstep_set_rolling_cyl. */
int shstep_set_twisting_cyl(shpair_ctx *ctx, int ncyl, const double *mu_tw, const double *gamma_tw);

/* ---- conical container walls (SPEC §2.22): hoppers, mill end cones ---------- */

#define SHSTEP_MAX_CONES 8

/* The INSIDE of one-nappe circular cones as walls: the wall contact of §2.9 with the half-space replaced by the outside
 * of a cone.  cone8[8k..] = a[3] (the apex), axis[3] (unit vector from the apex into the opening), cos theta, sin theta of
 * the half-angle of cone k, computed once by the caller (both > 0, that is 0 < theta < pi/2, and |cos^2 + sin^2 - 1| <=
 * 4 ulp); kn[k], exponent[k] its force law (SPEC §2.7).  The cone is infinite and has no outlet: close it and cut it with
 * planes (shstep_set_walls).  The particles live inside: with y = x_i - a, t = y.axis, d = |y - t axis| the centre's
 * distance to the wall is h = sin theta t - cos theta d; a centre with h <= 0 (at or outside the wall, behind the apex)
 * or a position that is not a number contributes nothing for that cone and raises a device error bit: SHPAIR_EINVAL
 * ("particle centre outside a cone") from the call that next reads the error word, as for the planes and the cylinders.
 * ncone = 0 removes all cones.  Every call resets gamma_k, mu_k, gamma_t,k and Omega of the setters below to 0.
 * It also resets every k_t,k of shstep_set_conic_tangential_spring to 0 and drops the spring history (SPEC §2.23), and
 * resets the four coefficients of §2.24 (shstep_set_rolling_con, shstep_set_twisting_con) to 0.
 * SHPAIR_EINVAL for more than SHSTEP_MAX_CONES cones, an axis that is not a unit vector to 1e-12, a cosine or sine that
 * is not > 0 or a pair that is not on the unit circle, kn < 0, an exponent < 1 or a number that is not finite.  Always
 * the sharp rule.  Not modelled, and absent rather than half-built: the outside of a cone, an outlet or a truncation,
 * any motion but the rotation below, a cone in the energy ledger or
 * the shell ledger (see shstep_set_cone_damping), the loop over several ranks (shhalo_run_device returns SHPAIR_ESTATE
 * while a cone is set), a host-pointer form.  Blocks. */
int shstep_set_cones(shpair_ctx *ctx, int ncone, const double *cone8, const double *kn, const double *exponent);

/* gamma_k >= 0 per cone: p_tot = max(0, p + gamma_k Vdot), Vdot = S_n.w_i + T_n.omega_i (the rotation does not enter: a
 * cone turning about its own axis changes no overlap).  After shstep_set_cones; ncone must match.  While the energy
 * ledger or the shell ledger is on, a non-zero coefficient of this or the next setter, and a non-zero Omega, are
 * SHPAIR_ESTATE (neither ledger keeps cone entries), and so is switching either ledger on while one is set; an elastic
 * cone at rest is allowed.  Blocks. */
int shstep_set_cone_damping(shpair_ctx *ctx, int ncone, const double *gamma);

/* mu_k, gamma_t,k >= 0 per cone; a cone has friction iff both are non-zero: F_t = -kappa v_t at the point where the
 * normal wrench's line of action leaves the cone, v_t the tangential part of w_i + omega_i x r_i - Omega a x rho_c there,
 * kappa = gamma_t,k capped at mu_k N / |v_t|, N = p_tot |S_n| (SPEC §2.22).  Otherwise as shstep_set_cone_damping. */
int shstep_set_cone_friction(shpair_ctx *ctx, int ncone, const double *mu, const double *gamma_t);

/* Omega per cone, any finite value: the angular velocity of the cone about its own axis (right-handed about axis).  It
 * enters the friction (and the springs of §2.23), through the wall's material velocity Omega axis x rho_c at the contact
 * point, and the couples of §2.24, through Omega axis itself; the geometry never moves.  After shstep_set_cones; ncone must match.  Blocks. */
int shstep_set_cone_rotation(shpair_ctx *ctx, int ncone, const double *omega);

/* ADDS the cone forces and torques (about x_i) to the owned rows with (mask[i] & groupbit) != 0; a particle in reach of
 * several cones adds them in index order.  cone_out_dev is nullable: 5 doubles per cone, E_k, Fx, Fy, Fz of the force ON
 * the wall and M_ax, the moment of that force about the axis through the apex, ADDED to what is there; the same bits
 * with and without the "deterministic" option.  twist_dev[nlocal][6] as shstep_twist_device writes it; it is read only
 * while a cone has damping or friction (NULL then: SHPAIR_EINVAL); with every coefficient 0 the elastic kernel runs
 * whatever twist_dev and Omega are.  While a cone has rolling or twisting resistance (SPEC §2.24) twist_dev is read too
 * (NULL: SHPAIR_EINVAL) and the couples are added to torque_dev and to M_ax.  Only enqueues on `stream`; sizing the buffers first (a call with the same nlocal and
 * cone_out_dev != NULL) makes it capturable.  With no cone set nothing is allocated, zeroed or launched.  While a cone has
 * a tangential spring (SPEC §2.23) it returns SHPAIR_EINVAL and names shstep_conic_contact_device. */
int shstep_cone_force_device(shpair_ctx *ctx, int nlocal, const double *x_dev, const double *quat_dev,
                             const int *shtype_dev, const int *mask_dev, int groupbit, double *f_dev,
                             double *torque_dev, double *cone_out_dev, const double *twist_dev, void *stream);

/* ---- tangential springs with history at the cones (SPEC §2.23): static friction.  The C names say "conic" ---- */

/* Replaces F_t = -kappa v_t of SPEC §2.22 at the cones that have a spring.  The contact point r_i, rho_c, the inward normal
 * n^_c = s a^ - c c^_c (c^_c = rho_c / |rho_c|), v_t and N are §2.22's.  The surface frame there is the generator g^_c =
 * s c^_c + c a^ (away from the apex) and t^_c = a^ x c^_c (the way the wall moves for Omega > 0); the azimuth is phi_c =
 * atan2(rho_c.e2, rho_c.e1), e1 the vector the frame rule of SPEC §2.3 gives about the axis, e2 = a^ x e1.  Per (owned
 * particle, cone) the pass keeps (xi_g, xi_theta, phi_c) and one bit of an 8-bit live word per particle.  A live state is
 * first transported: a cone develops into a plane sector of polar angle beta = s phi, so with Delta phi = phi_c' - phi_c
 * wrapped into (-pi, pi] and Delta beta = s (Delta phi - Omega dt),
 *   xi_g <- xi_g cos Delta beta + xi_theta sin Delta beta,   xi_theta <- -xi_g sin Delta beta + xi_theta cos Delta beta
 * (old values on the right); a particle carried round by the cone keeps its spring, theta -> 0 is §2.19 and theta -> pi/2
 * is §2.15.  Then xi_g += dt v_t.g^_c, xi_theta += dt v_t.t^_c, the trial force F* = -k_t (xi_g g^_c + xi_theta t^_c) -
 * gamma_t v_t, which sticks if |F*| <= mu N and otherwise slides: F_t = F* mu N / |F*| and xi = -(F_t + gamma_t v_t) / k_t in
 * components.  F_i += F_t, tau_i += r_i x F_t.  xi starts from 0 at a new contact and is reset (the bit cleared, no
 * tangential force) where the cone is out of the particle's mask, V <= 0, |S_n| = 0, N = 0 or a friction guard of §2.22
 * fires.  The totals rows stay minus the whole force on the particle: M_ax contains the static load the drive holds.
 *
 * k_t,k >= 0 (force per length) per cone, default 0; a cone has history iff mu_k != 0 and k_t,k != 0 (gamma_t,k may then be
 * 0); the other cones keep §2.22 inside the same pass.  Validated like shstep_set_cone_friction, and the two setters give
 * the same state in either order.  Call it after shstep_set_cones, which resets every k_t,k to 0 and drops the history;
 * ncone must match.  Setting the last k_t to 0 (or the mu of the last history cone) drops the history too.  While a cone
 * has history the pass keeps 24 ncone + 1 B per owned particle, and shstep_cone_force_device returns SHPAIR_EINVAL and
 * names shstep_conic_contact_device.  The state is keyed by the row index: a pass over another nlocal than the last
 * advancing pass' starts from nothing live.  With every k_t = 0 and none set before, nothing is allocated.
 * SHPAIR_ESTATE while the energy ledger or the shell ledger is on (and either ledger while a spring is set), like every
 * other cone coefficient.  Not modelled: the loop over several ranks, a host-pointer form.  Blocks. */
int shstep_set_conic_tangential_spring(shpair_ctx *ctx, int ncone, const double *kt);

/* shstep_cone_force_device with the law above and its time step: dt > 0 advances and stores the state and the live
 * words, dt = 0 forms the forces from the stored state (transported with no Omega dt term, capped) and writes nothing
 * (the set-up forces of Verlet::setup).  While no cone has history the call IS shstep_cone_force_device, bit for bit,
 * whatever dt, and nothing is allocated, zeroed or launched on top.  SHPAIR_EINVAL for a dt that is negative or not
 * finite, and for a NULL twist_dev while a cone has history.  The couples of §2.24 are added by either form, and by a
 * look (dt = 0) too: they have no state.  Its buffers only grow, so one call ahead of a stream capture
 * (same nlocal) makes it capturable. */
int shstep_conic_contact_device(shpair_ctx *ctx, int nlocal, const double *x_dev, const double *quat_dev,
                                const int *shtype_dev, const int *mask_dev, int groupbit, double *f_dev,
                                double *torque_dev, double *cone_out_dev, const double *twist_dev, double dt, void *stream);

/* (xi_g, xi_theta, phi_c) of the cones to / from the host, [nlocal][ncone][3] (restarts, tests).  The copy gives 0 where
 * the bit is dead (all of it while nothing is held); SHPAIR_EINVAL for another nlocal than the history is held for.  The
 * set marks live where one of the three is non-zero and keys the history by its nlocal (>= 1).  SHPAIR_ESTATE while no
 * cone has history.  Both block. */
int shstep_copy_conic_history(shpair_ctx *ctx, int nlocal, double *xi_out);
int shstep_set_conic_history(shpair_ctx *ctx, int nlocal, const double *xi);

/* Drops every spring of the cones: the next pass starts from nothing live (nothing to do where none is held).  Blocks. */
int shstep_reset_conic_history(shpair_ctx *ctx);

/* ---- rolling and twisting resistance at the cones (SPEC §2.24).  The C names end in "_con" ---- */

/* The two couples of §2.17 at a conical wall.  Per owned particle i and cone k in its mask: F_w is the force ON the wall
 * as the cone pass leaves it per (particle, cone), minus the whole force on the particle, whichever instance wrote it;
 * c^ = rho / d is the radial direction through the particle's centre (on the axis: the e1 of the frame rule about the
 * axis, a convention) and n^ = cos theta c^ - sin theta a^ the wall's outward normal at the nearest generator, the
 * geometric one, never S^.  N = max(0, n^.F_w) is the load, Omega_rel = omega_i - Omega_k a^ the angular velocity in the
 * cone's frame (a particle carried rigidly round, omega_i = Omega_k a^, feels exactly nothing), Omega_n = (Omega_rel.n^) n^
 * and Omega_r = Omega_rel - Omega_n.  Unlike a drum's, the cone's own rotation enters both: Omega_k a^ twists by
 * -Omega_k sin theta n^ and rolls by Omega_k cos theta g^ (g^ the generator).  M = -kappa_r Omega_r - kappa_tw Omega_n,
 * either coefficient capped at mu N / |.|, is added to the particle's torque; no force.  The couple on the wall is -M:
 * M_ax of cone_out gains -a^.M, E_k and the force keep their bits.  What taking the load along n^ costs is measured in
 * SPEC §2.24.
 *
 * mu_r,k >= 0 (a length) and gamma_r,k >= 0 (torque per angular velocity) per cone, default 0; a cone has rolling
 * resistance iff both are non-zero.  Validated like shstep_set_cone_friction; call it after shstep_set_cones, which
 * resets all four coefficients to 0; ncone must match.  The device table is allocated by the first call that sets a
 * kind.  While a cone has either kind: every cone pass, of either form, reads twist_dev (NULL: SHPAIR_EINVAL), keeps its
 * 40 B rows per (particle, cone) whether or not cone_out is asked for, and launches one more kernel behind the contact
 * kernel, no atomics, the same bits with and without "deterministic"; the run loops compute twists.  SHPAIR_ESTATE
 * while the energy ledger or the shell ledger is on (and either ledger while a kind is set), like every other cone
 * coefficient: M.omega_i = -P_roll + Omega_k (a^.M) with P_roll = kappa_r |Omega_r|^2 + kappa_tw |Omega_n|^2 >= 0 has no
 * ledger entry.  With every coefficient 0 and none set before, nothing is allocated, zeroed or launched.  Not modelled:
 * rolling or twisting springs with history, the loop over several ranks, a host-pointer form.  Blocks. */
int shstep_set_rolling_con(shpair_ctx *ctx, int ncone, const double *mu_r, const double *gamma_r);

/* mu_tw,k >= 0 (a length) and gamma_tw,k >= 0 (torque per angular velocity): twisting resistance, as
 * shstep_set_rolling_con. */
int shstep_set_twisting_con(shpair_ctx *ctx, int ncone, const double *mu_tw, const double *gamma_tw);

/* Particle/cone contacts with V > 0 of the last cone pass.  Blocks. */
int shstep_get_cone_stats(shpair_ctx *ctx, int *ncontacts);

/* The cones as set, cone8_out[8k..] = a[3], axis[3], cos theta, sin theta (for restarts); ncone must match. */
int shstep_get_cones(shpair_ctx *ctx, int ncone, double *cone8_out);

/* ---- the whole loop, for a host that owns nothing but the arrays ----------- */

/* Device pointers and scalars of one rank's particles; arrays sized for nmax rows (owned + ghosts) except
 * v, angmom, mask (nlocal rows). */
typedef struct shstep_arrays {
  int nlocal, nmax;
  double *x, *v, *quat, *angmom, *f, *torque;
  int *type, *shtype, *mask;
  int groupbit;
  double dt;
  double gravity[3], gamma_t, gamma_r; /* all zero: no post_force pass */
  int check_every;                      /* rebuild test every this many steps (>= 1), neigh_modify every N check yes */
} shstep_arrays;

/* Verlet::run for nsteps: initial_integrate -> [rebuild test -> borders + neighbour build] -> forward ->
 * clear -> pair compute -> [twist, pair damping / friction, when a coefficient of either is set: the half-step velocities; with a tangential
 * spring set the pass is shstep_pair_contact_device with the step's dt; behind it shstep_pair_rolling_device, while a rolling
 * or twisting coefficient is set] -> reverse ->
 * [wall advance, while a wall has a normal velocity; walls, when shstep_set_walls set any: with a wall tangential spring set the pass is shstep_wall_contact_device with the step's dt; cylinders, when shstep_set_cylinders set any: with a cylinder tangential spring set the pass is shstep_cyl_contact_device with the step's dt; cones, when shstep_set_cones set any: with a cone tangential spring set the pass is shstep_conic_contact_device with the step's dt; ledger fold, while the energy ledger is on] -> post_force -> final_integrate, entirely on `stream` (must not be
 * NULL when use_graph is set: the legacy null stream cannot be captured).  On entry the ghosts / list
 * of the current positions must exist (shstep_borders_device + shstep_neighbor_build_device) and f, torque
 * must hold their forces (as after Verlet::setup); *nghost is the current ghost count and is updated.
 * use_graph != 0: the launches of a step are replayed from two captured hipGraphs (re-captured after every
 * rebuild) instead of being issued one by one — the launch-bound regime of small systems.
 * Returns after the last step is enqueued and the stream is idle (blocks).  *rebuilds (nullable) counts
 * the list rebuilds. */
int shstep_run_device(shpair_ctx *ctx, const shstep_arrays *a, int nsteps, int use_graph, int *nghost, int *rebuilds,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SHSTEP_H */
