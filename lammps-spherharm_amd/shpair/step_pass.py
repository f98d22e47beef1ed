"""What the two Python step drivers share (run.DeviceRun: one rank; mrank.RankRun: one rank of several): the force pass of
a step, the contact set-up of a context and the block of device arrays of a rank.

`force_pass` is the Python restatement of enqueue_b / step_after_reverse (csrc/shstep_run.cpp) in the order of
csrc/shhalo_run.cpp; what it decides, it decides from the predicates of capi.ShPair that carry the library's names.
"""
from collections import namedtuple

import numpy as np

# One rank's device pointers (ints) and scalars, as StepView of csrc/step_body.hpp holds them; gravity: 3 doubles on the
# host; twist: [nlocal + nghost][6], or None where no dissipation coefficient is ever set; stream: a hipStream_t or None.
StepView = namedtuple("StepView", "nlocal nghost x quat v angmom type shtype mask f torque twist groupbit dt gravity gamma_t "
                                  "gamma_r stream")


def has_body_forces(v):
    """step_has_body_forces: gravity or viscous drag; all zero, and no post_force pass is enqueued."""
    g = v.gravity
    return g[0] != 0.0 or g[1] != 0.0 or g[2] != 0.0 or v.gamma_t != 0.0 or v.gamma_r != 0.0


def force_pass(sp, v, forward, reverse, twist_ghosts, eflag=False, ev=None, advance=False):
    """Enqueues the forces of the current positions on v.stream: twists, forward, pair compute, pair dissipation, reverse,
    wall advance, wall pass, cylinder pass, cone pass, body forces.  It only enqueues: zeroing f / torque / ev and every synchronisation are the
    caller's.

    forward(twist): the caller's forward exchange of x and quat; twist is v.twist while a pair coefficient is set (the
      ghost rows need their owners' twists) and None otherwise.  reverse(): its reverse exchange of f and torque.
    twist_ghosts: the ghost rows whose twists the twist kernel fills itself, as step_twists takes it: v.nghost where the
      ghosts are the context's own periodic images, 0 where forward(twist) brings them.
    advance: the force pass of a step: the planes of translating walls move by dt ahead of the wall pass."""
    pair = sp.keeps_integrals
    # The twists come first, as in the loop over all ranks; shstep_run_device enqueues them behind the compute.  No
    # result bit depends on which: the twist kernel reads v, quat, angmom, shtype and writes only twist, and the compute
    # reads none of that.
    if sp.has_dissipation:
        sp.twist_device(v.nlocal, twist_ghosts, v.v, v.quat, v.angmom, v.shtype, v.twist, stream=v.stream)
    forward(v.twist if pair else None)
    sp.compute_device(v.nlocal, v.nghost, v.x, v.quat, v.type, v.shtype, v.f, v.torque, eflag=eflag, ev=ev if eflag else None,
                      stream=v.stream)
    # rolling and twisting resistance (docs/SPEC.md §2.16) keeps the integrals too, but is a pass of its own behind the
    # pair pass: with it alone no pair pass is called (a context without the two predicates has neither)
    rolling = getattr(sp, "has_rolling", False)
    pair_pass = getattr(sp, "has_pair_pass", pair)
    if pair_pass and getattr(sp, "has_history", False):
        # tangential springs (docs/SPEC.md §2.14): the pass of a step advances xi by dt, as step_dissipation_pass; the one
        # that only fills set-up forces looks at it (dt = 0)
        sp.pair_contact_device(v.nlocal, v.nghost, v.x, v.type, v.shtype, v.twist, v.f, v.torque, v.dt if advance else 0.0,
                               stream=v.stream)
    elif pair_pass:
        sp.pair_dissipation_device(v.nlocal, v.nghost, v.x, v.type, v.shtype, v.twist, v.f, v.torque, stream=v.stream)
    if rolling:
        sp.pair_rolling_device(v.nlocal, v.nghost, v.x, v.type, v.twist, v.torque, stream=v.stream)
    reverse()
    # as step_after_reverse: x is x(t + dt), the planes follow (a rank that owns nothing advances its planes too) ...
    if advance and sp.walls_advance:
        sp.advance_walls_device(v.dt, stream=v.stream)
    # ... then one wall call, with the twists only while a wall coefficient is set, and the body forces: owned rows only
    if not v.nlocal:
        return
    if sp.nwalls and getattr(sp, "has_wall_history", False):
        # tangential springs of the walls (docs/SPEC.md §2.15): as for the pair springs above, the pass of a step advances
        # xi by dt and the one that only fills set-up forces looks at it
        sp.wall_contact_device(v.nlocal, v.x, v.quat, v.shtype, v.mask, v.f, v.torque, v.twist, v.dt if advance else 0.0,
                               groupbit=v.groupbit, stream=v.stream)
    elif sp.nwalls:
        sp.wall_force_damped_device(v.nlocal, v.x, v.quat, v.shtype, v.mask, v.f, v.torque,
                                    v.twist if sp.wall_reads_twists else None, groupbit=v.groupbit, stream=v.stream)
    # cylindrical container walls (docs/SPEC.md §2.18), directly behind the planar pass, as step_after_reverse
    if getattr(sp, "ncylinders", 0) and getattr(sp, "has_cyl_history", False) is True:
        # tangential springs of the cylinders (docs/SPEC.md §2.19): as for the walls above, the pass of a step advances xi by
        # dt and the set-up pass looks at it.  (`is True`: a stand-in context that answers every name with a callable has
        # no such predicate)
        sp.cyl_contact_device(v.nlocal, v.x, v.quat, v.shtype, v.mask, v.f, v.torque, v.twist, v.dt if advance else 0.0,
                              groupbit=v.groupbit, stream=v.stream)
    elif getattr(sp, "ncylinders", 0):
        sp.cylinder_force_device(v.nlocal, v.x, v.quat, v.shtype, v.mask, v.f, v.torque,
                                 v.twist if sp.cylinder_reads_twists else None, groupbit=v.groupbit, stream=v.stream)
    # conical container walls (docs/SPEC.md §2.22), directly behind the cylinder pass, as step_after_reverse.  (A count,
    # not a callable: a stand-in context that answers every name with a callable has no cones)
    ncones = getattr(sp, "ncones", 0)
    if isinstance(ncones, int) and ncones and getattr(sp, "has_conic_history", False) is True:
        # tangential springs of the cones (docs/SPEC.md §2.23): as for the cylinders above, the pass of a step advances the
        # state by dt and the set-up pass looks at it
        sp.conic_contact_device(v.nlocal, v.x, v.quat, v.shtype, v.mask, v.f, v.torque, v.twist, v.dt if advance else 0.0,
                                groupbit=v.groupbit, stream=v.stream)
    elif isinstance(ncones, int) and ncones:
        sp.cone_force_device(v.nlocal, v.x, v.quat, v.shtype, v.mask, v.f, v.torque,
                             v.twist if sp.cone_reads_twists else None, groupbit=v.groupbit, stream=v.stream)
    if has_body_forces(v):
        sp.post_force_device(v.nlocal, v.gravity, v.gamma_t, v.gamma_r, v.v, v.quat, v.angmom, v.shtype, v.mask, v.f, v.torque,
                             groupbit=v.groupbit, stream=v.stream)


def apply_contact_options(sp, walls=None, pair_damping=None, wall_damping=None, pair_friction=None, wall_friction=None,
                          wall_velocity=None, pair_spring=None, wall_spring=None, pair_rolling=None, pair_twisting=None,
                          wall_rolling=None, wall_twisting=None, cylinders=None, cylinder_damping=None, cylinder_friction=None,
                          cylinder_rotation=None, cylinder_spring=None, shell_ledger=None, cylinder_rolling=None,
                          cylinder_twisting=None, cones=None, cone_damping=None, cone_friction=None, cone_rotation=None,
                          conic_spring=None, conic_rolling=None, conic_twisting=None):
    """The contact options of a driver's constructor; None leaves what the context holds.
    walls: (planes[nw][4], kn, exponent) as ShPair.set_walls takes them; first, because it resets the other wall options.
    pair_damping: {(itype, jtype): gamma} ('*' allowed), wall_damping: gamma_w, a scalar or [nw] (docs/SPEC.md §2.10).
    pair_friction: {(itype, jtype): (mu, gamma_t)}, wall_friction: (mu_w, gamma_t,w), scalars or [nw] each (§2.11).
    wall_spring: k_t,w, a scalar or [nw]: tangential springs with history for the walls that have a mu (§2.15); applied
    after wall_friction.
    wall_velocity: u_w, one vector or [nw][3] (§2.12).
    pair_spring: {(itype, jtype): k_t}: tangential springs with history for the pairs that have a mu (§2.14); ahead of the
    driver's first list build.
    pair_rolling: {(itype, jtype): (mu_r, gamma_r)}, pair_twisting: {(itype, jtype): (mu_tw, gamma_tw)}: rolling and
    twisting resistance (§2.16).
    wall_rolling: (mu_r,w, gamma_r,w), wall_twisting: (mu_tw,w, gamma_tw,w), scalars or [nw] each: the same resistance at
    the walls (§2.17); applied behind wall_friction.
    cylinders: (cyl[nc][7], kn, exponent) as ShPair.set_cylinders takes them (§2.18); ahead of cylinder_damping: gamma_c,
    cylinder_friction: (mu_c, gamma_t,c), cylinder_rotation: Omega and cylinder_spring: k_t,c (tangential springs with
    history for the cylinders that have a mu, §2.19), scalars or [nc] each, which it resets.
    cylinder_rolling: (mu_r,c, gamma_r,c), cylinder_twisting: (mu_tw,c, gamma_tw,c), scalars or [nc] each: rolling and
    twisting resistance at the shells (§2.21); applied behind cylinder_spring.
    shell_ledger: the switch of the cylinder entries of the energy ledger (§2.20), ahead of everything else: while it is
    on, a cylinder coefficient and the energy ledger may be set together.
    cones: (cone[nk][8], kn, exponent) as ShPair.set_cones takes them (§2.22); ahead of cone_damping: gamma_k,
    cone_friction: (mu_k, gamma_t,k), cone_rotation: Omega and conic_spring: k_t,k (tangential springs with history for the
    cones that have a mu, §2.23), scalars or [nk] each, which it resets.
    conic_rolling: (mu_r,k, gamma_r,k), conic_twisting: (mu_tw,k, gamma_tw,k), scalars or [nk] each: rolling and twisting
    resistance at the conical walls (§2.24); applied behind conic_spring."""
    if shell_ledger is not None:
        sp.set_shell_ledger(shell_ledger)
    if walls is not None:
        sp.set_walls(*walls)
    if cylinders is not None:
        sp.set_cylinders(*cylinders)
    if cylinder_damping is not None:
        sp.cylinder_damping(cylinder_damping)
    if cylinder_friction is not None:
        sp.cylinder_friction(*cylinder_friction)
    if cylinder_rotation is not None:
        sp.cylinder_rotation(cylinder_rotation)
    if cylinder_spring is not None:
        sp.set_cyl_tangential_spring(cylinder_spring)
    if cylinder_rolling is not None:
        sp.cylinder_rolling(*cylinder_rolling)
    if cylinder_twisting is not None:
        sp.cylinder_twisting(*cylinder_twisting)
    if cones is not None:
        sp.set_cones(*cones)
    if cone_damping is not None:
        sp.cone_damping(cone_damping)
    if cone_friction is not None:
        sp.cone_friction(*cone_friction)
    if cone_rotation is not None:
        sp.cone_rotation(cone_rotation)
    if conic_spring is not None:
        sp.conic_spring(conic_spring)
    if conic_rolling is not None:
        sp.conic_rolling(*conic_rolling)
    if conic_twisting is not None:
        sp.conic_twisting(*conic_twisting)
    for (a, b), g in (pair_damping or {}).items():
        sp.pair_damping(a, b, g)
    if wall_damping is not None:
        sp.wall_damping(wall_damping)
    for (a, b), (mu, gt) in (pair_friction or {}).items():
        sp.pair_friction(a, b, mu, gt)
    if wall_friction is not None:
        sp.wall_friction(*wall_friction)
    if wall_rolling is not None:
        sp.wall_rolling(*wall_rolling)
    if wall_twisting is not None:
        sp.wall_twisting(*wall_twisting)
    if wall_spring is not None:
        sp.set_wall_tangential_spring(wall_spring)
    if wall_velocity is not None:
        sp.wall_velocity(wall_velocity)
    for (a, b), kt in (pair_spring or {}).items():
        sp.set_pair_tangential_spring(a, b, kt)
    for (a, b), (mu, g) in (pair_rolling or {}).items():
        sp.pair_rolling(a, b, mu, g)
    for (a, b), (mu, g) in (pair_twisting or {}).items():
        sp.pair_twisting(a, b, mu, g)


def rank_arrays(run, device, n, nmax, nrows, x, quat, shtype, type_=None, v=None, angmom=None, mask=None, tag=None):
    """A rank's device tensors as attributes of `run` (torch owns the memory: dev x q v L f tq ty sh mask ev en, and tag
    where one is given), the first n rows filled from the host arrays that are given.  x, q, f, tq, ty, sh and tag have
    nmax rows (owned + ghost); v, L and mask have nrows: n where ghosts never need them, nmax where atoms migrate."""
    import torch
    run.dev = torch.device(device)
    f64 = dict(dtype=torch.float64, device=run.dev)
    i32 = dict(dtype=torch.int32, device=run.dev)
    run.x, run.f, run.tq = (torch.zeros(nmax, 3, **f64) for _ in range(3))
    run.v, run.L = torch.zeros(nrows, 3, **f64), torch.zeros(nrows, 3, **f64)
    run.q = torch.zeros(nmax, 4, **f64)
    run.ty, run.mask = torch.ones(nmax, **i32), torch.ones(nrows, **i32)
    run.sh = torch.zeros(nmax, **i32)
    run.ev, run.en = torch.zeros(7, **f64), torch.zeros(3, **f64)
    fill = [(run.x, x, np.float64), (run.q, quat, np.float64), (run.v, v, np.float64), (run.L, angmom, np.float64),
            (run.sh, shtype, np.int32), (run.ty, type_, np.int32), (run.mask, mask, np.int32)]
    if tag is not None:
        run.tag = torch.zeros(nmax, **i32)
        fill.append((run.tag, tag, np.int32))
    for dst, src, dt_ in fill:
        if src is not None and n:
            dst[:n] = torch.from_numpy(np.ascontiguousarray(src, dtype=dt_)).to(run.dev)
