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

# The surface passes of a step in the library's order, by the names of capi.ShPair: (count, history predicate, contact pass,
# reads-twists predicate, force pass).  A new surface family is a row here.
_SURFACE_PASSES = (
    ("nwalls", "has_wall_history", "wall_contact_device", "wall_reads_twists", "wall_force_damped_device"),
    ("ncylinders", "has_cyl_history", "cyl_contact_device", "cylinder_reads_twists", "cylinder_force_device"),
    ("ncones", "has_conic_history", "conic_contact_device", "cone_reads_twists", "cone_force_device"),
)

# The contact options of apply_contact_options in the order they are applied: (option, method of capi.ShPair, whether the
# value is a tuple to unpack).  The order is part of the contract: shell_ledger first, a geometry ahead of the coefficients
# it resets, the shells' spring ahead of their rolling and twisting.  A new law is a row here and a keyword below.
_CONTACT_OPTIONS = (
    ("shell_ledger", "set_shell_ledger", False), ("walls", "set_walls", True),
    ("cylinders", "set_cylinders", True), ("cylinder_damping", "cylinder_damping", False),
    ("cylinder_friction", "cylinder_friction", True), ("cylinder_rotation", "cylinder_rotation", False),
    ("cylinder_spring", "set_cyl_tangential_spring", False), ("cylinder_rolling", "cylinder_rolling", True),
    ("cylinder_twisting", "cylinder_twisting", True),
    ("cones", "set_cones", True), ("cone_damping", "cone_damping", False), ("cone_friction", "cone_friction", True),
    ("cone_rotation", "cone_rotation", False), ("conic_spring", "conic_spring", False), ("conic_rolling", "conic_rolling", True),
    ("conic_twisting", "conic_twisting", True),
    ("pair_damping", "pair_damping", False), ("wall_damping", "wall_damping", False),
    ("pair_friction", "pair_friction", True), ("wall_friction", "wall_friction", True),
    ("wall_rolling", "wall_rolling", True), ("wall_twisting", "wall_twisting", True),
    ("wall_spring", "set_wall_tangential_spring", False), ("wall_velocity", "wall_velocity", False),
    ("pair_spring", "set_pair_tangential_spring", False), ("pair_rolling", "pair_rolling", True),
    ("pair_twisting", "pair_twisting", True),
)


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
    # the planar walls (docs/SPEC.md §2.9), the cylinders directly behind them (§2.18) and the cones behind those (§2.22), as
    # step_after_reverse.  A stand-in context may know fewer families than the binding, or answer every name with a
    # callable: a family is present iff its count is a non-zero int, and a predicate holds iff it is True.  The walls are
    # the exception: every context has nwalls.  The reads-twists predicate of a family that is present is required.
    for count, has_history, contact_device, reads_twists, force_device in _SURFACE_PASSES:
        n = sp.nwalls if count == "nwalls" else getattr(sp, count, 0)
        if not (isinstance(n, int) and n):
            continue
        if getattr(sp, has_history, False) is True:
            # tangential springs of the family (§2.15, §2.19, §2.23): as for the pair springs above, the pass of a step
            # advances the state by dt and the one that only fills set-up forces looks at it
            getattr(sp, contact_device)(v.nlocal, v.x, v.quat, v.shtype, v.mask, v.f, v.torque, v.twist,
                                        v.dt if advance else 0.0, groupbit=v.groupbit, stream=v.stream)
        else:
            getattr(sp, force_device)(v.nlocal, v.x, v.quat, v.shtype, v.mask, v.f, v.torque,
                                      v.twist if getattr(sp, reads_twists) is True else None, groupbit=v.groupbit, stream=v.stream)
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
    given = locals()
    for option, method, star in _CONTACT_OPTIONS:
        value = given[option]
        if value is None:
            continue
        # a pair option is a dict {(itype, jtype): value}: one call per entry, the type pair ahead of the value
        for types, val in (value.items() if option.startswith("pair_") else [((), value)]):
            getattr(sp, method)(*types, *(val if star else (val,)))


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
