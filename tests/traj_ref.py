"""Whole-step reference: the time step of docs/SPEC.md §6, "Order of a step with every model on", in plain numpy, item by
item.  It is made only of pieces that do not go through the HIP library: the CPU oracle's compute (per-slot integrals),
nve and post_force; step_ref.images / half_list for ghosts and list; history_ref.owner_tags / carry for the rebuild;
damp_ref.twists; history_ref.pair_history; rolling_ref.pair_rolling; wall_move_ref.advance;
wall_history_ref.wall_forces_history; ledger_ref for powers and fold.  What is written out here is the ORDER, the wrap and
the rebuild decision of §7, and the bookkeeping (counts, margins, snapshots).

A scene is a dict (see `scene`); the state a dict: x v quat angmom f torque [n][3|4], planes [nw][4], the list (offs, jl,
own, code, keys), pair xi [nslots][3] keyed by (i, owner tag), wall xi [n][nw][3] and live [n][nw], the ledger (totals [5],
per_wall [nw][3]), builds, xhold.

A scene may carry cylinders (the cylinder items of the list: the pass of §2.18, §2.19 and §2.21 directly behind the planar
wall pass of item 11, and the shell rows of item 13's fold).  The arithmetic of that pass is cyl_history_ref.
cyl_forces_history (wrench, (xi_a, xi_theta), live), cyl_roll_ref.reach_sums / cyl_roll (couples and the power rows, which
it takes from shell_ledger_ref.contact_powers) and shell_ledger_ref.shell_fold; written out here are which rows and which
twists it gets, its dt, and where its rows go.  Such a scene has the further entries cyl [nc][7], cyl_kn, cyl_expo,
cyl_damping, cyl_mu, cyl_gt, cyl_omega, cyl_kt, cyl_mur, cyl_gr, cyl_mutw, cyl_gtw [nc] and shell_ledger; its state cyl_xi
[n][nc][2], cyl_live [n][nc], shell [3] and per_cylinder [nc][3]; its passes leave CYL_COUNTS beside COUNTS, its
snapshots are compared in CYL_QUANTITIES beside QUANTITIES, and CYL_VARIANTS are its wrong steps.  A scene without the
entry `cyl` (the two older fixtures have none of these keys) takes the path it always took.

A scene may carry cones (the cone half of item 11: the pass of §2.22 and §2.23 directly behind the cylinder pass).  The
arithmetic of that pass is conic_history_ref.cone_forces_history, which falls through to cone_ref.contact_wrench for a
cone without a spring; written out here are which rows and which twists it gets, its dt (0 in the set-up look), that its
state is keyed by the row (a rebuild moves nothing, a wrap does not touch it) and that its f and torque add behind the
cylinders'.  Such a scene has the further entries cone [nk][8] (the records cone_ref.cone builds), cone_kn, cone_expo,
cone_damping, cone_mu, cone_gt, cone_omega, cone_kt [nk]; its state cone_xi [n][nk][3] = (xi_g, xi_theta, phi_c) and
cone_live [n][nk]; its passes leave CONE_COUNTS, its snapshots are compared in CONE_QUANTITIES, and CONE_VARIANTS are its
wrong steps.  The cone pass leaves no power row (§2.22 refuses a cone coefficient beside either ledger): the fold has no
cone term.  A scene without the entry `cone` takes the path it always took.

`variant` names ONE deliberately wrong step (VARIANTS, CYL_VARIANTS, CONE_VARIANTS, or MRANK_VARIANTS: the wrong steps of
a decomposition, made here at the periodic images): each breaks exactly one item of the list.  `noise`: a
numpy Generator; every per-slot integral row, every wall sum, every cylinder sum and every cone sum is scaled by
1 + NOISE * eta, eta uniform in [-1, 1].
"""
import contextlib

import numpy as np

import cone_ref as Co
import conic_history_ref as KH
import cyl_history_ref as CH
import cyl_ref as Cy
import cyl_roll_ref as CR
import damp_ref as D
import history_ref as H
import ledger_ref as LG
import rolling_ref as RL
import shell_ledger_ref as SL
import step_ref as SR
import wall_history_ref as WH
import wall_move_ref as WM
import wall_ref as W
from oracle import oracle as O

NOISE = 1.0e-12
# name: (the item of the list it breaks, the quantities it must move)
VARIANTS = {
    "twists_prekick": (3, ("v", "angmom", "xi", "ledger")),        # twists from v, angmom ahead of the half kick
    "twists_old_quat": (3, ("v", "angmom", "xi", "ledger")),       # twists with the quaternion ahead of the drift
    "xi_half_dt": (7, ("xi", "wall_xi", "v")),                     # both spring passes advance xi by dt / 2
    "xi_in_setup": (7, ("xi", "wall_xi", "v")),                    # the set-up force pass advances xi too
    "planes_late": (10, ("x", "v", "wall_xi")),                    # planes advanced behind the wall pass
    "rolling_stale_integrals": (8, ("angmom", "quat")),            # rolling pass on the previous step's integrals
    "wall_stale_twists": (11, ("v", "angmom", "wall_xi")),         # wall pass on the previous step's twists
    "fold_skips_rolling": (13, ("ledger",)),                       # fold drops the rolling power beside a pair pass
    "carry_by_row": (2, ("xi",)),                                  # carry keyed by j's row index, not its owner's tag
}
# Wrong steps that only a decomposition can make (the loop over several ranks, docs/SPEC.md §6 "The same step over several
# ranks").  In this reference a ghost row is a periodic image, so each can be broken here; with no periodic direction there
# is no ghost and each is the right run bit for bit.
MRANK_VARIANTS = {
    "ghost_twists_stale": (3, ("v", "angmom", "ledger")),          # ghost rows keep their owner's twists of the previous force pass
    "ghost_type_one": (4, ("v", "angmom", "ledger")),              # a ghost row's type did not travel at borders: it reads as 1
    "ghost_rolling_torque_lost": (8, ("angmom", "quat")),          # the rolling pass' torque on ghost rows never goes home
    "ghost_slot_half_power": (13, ("ledger",)),                    # a slot with a ghost j counts half in the fold
}
# The wrong steps of the cylinder items (a scene with cylinders only): name: (item, the quantities it must move)
CYL_VARIANTS = {
    "cyl_stale_twists": (11, ("v", "angmom", "cyl_xi", "shell")),  # the cylinder pass on the previous pass's twists
    "cyl_xi_half_dt": (11, ("cyl_xi", "v", "shell")),              # (xi_a, xi_theta) advance by dt / 2
    "cyl_xi_in_setup": (11, ("cyl_xi", "v", "shell")),             # the set-up pass advances (xi_a, xi_theta) too
    "cyl_roll_stale_rows": (11, ("angmom", "quat", "shell")),      # couples from the previous pass's F_w rows
    "cyl_roll_omega_kept": (11, ("angmom", "quat", "shell")),      # Omega_c not subtracted (cyl_roll_ref's omega_c_kept)
    "shell_fold_skips_roll": (13, ("shell",)),                     # fold drops the couples' power beside a ledger instance
    "shell_fold_in_setup": (13, ("shell",)),                       # the look folds its rows, with dt
    "cyl_pushes_frozen": (11, ("cyl_xi", "shell")),                # rows outside the group get the cylinder pass too
    "cyl_prekick_twists": (11, ("v", "angmom", "cyl_xi", "shell")),  # cylinder pass alone: twists ahead of the half kick
}
# The wrong steps of the cone half of item 11 (a scene with cones only): name: (item, the quantities it must move).  The
# issue's table also lists "the cone pass ahead of item 10's advance"; it is no variant here because it is no observable
# order: the cone pass reads no plane, so running it ahead of the advance changes only the order in which three wrenches
# are added to f and torque, which is rounding.
CONE_VARIANTS = {
    "cone_stale_twists": (11, ("v", "angmom", "cone_xi", "cone_phi")),    # the cone pass on the previous pass's twists
    "cone_prekick_twists": (11, ("v", "angmom", "cone_xi", "cone_phi")),  # cone pass alone: twists ahead of the half kick
    "cone_xi_half_dt": (11, ("cone_xi", "v")),                 # the cone pass gets dt / 2: the advance and Omega dt see it
    "cone_xi_in_setup": (11, ("cone_xi", "v")),                # the set-up look advances the conic state
    "cone_pushes_frozen": (11, ("cone_xi",)),                  # rows outside the group get the cone pass too
    "cone_drops_at_rebuild": (2, ("cone_xi", "v")),            # a rebuilding step zeroes cone_xi and cone_live
    "cone_transport_dropped": (11, ("cone_xi", "v")),          # conic_history_ref.NO_TRANSPORT for the whole run
}
QUANTITIES = ("x", "v", "quat", "angmom", "xi", "wall_xi", "ledger")
CYL_QUANTITIES = ("cyl_xi", "shell")
# cone_xi: (xi_g, xi_theta) to the largest |xi|; cone_phi: |phi_c difference| wrapped to (-pi, pi], entries live in both
CONE_QUANTITIES = ("cone_xi", "cone_phi")
# what a cone pass leaves, per pass: (particle, cone) by branch; V > 0 with N = 0; friction contacts of a cone without k_t
# beside a history cone; rows touching two cones, a plane and a cone, a shell and a cone; rows outside the group within
# reach of a cone
CONE_COUNTS = ("cone_stick", "cone_slide", "cone_reset", "cone_clamp", "cone_plain_friction", "two_cones", "plane_and_cone",
               "shell_and_cone", "cone_frozen_in_reach")
# what a cylinder pass leaves beside COUNTS, per pass: (particle, cylinder) by branch; rows touching a plane and a shell,
# two shells; rows outside the group within reach of a cylinder; friction contacts of a cylinder without k_t beside a
# history cylinder
CYL_COUNTS = ("cyl_stick", "cyl_slide", "cyl_reset", "cyl_clamp", "cyl_roll_viscous", "cyl_roll_capped", "cyl_twist_viscous",
              "cyl_twist_capped", "plane_and_shell", "two_shells", "frozen_in_reach", "plain_friction")
COUNTS = ("pair_stick", "pair_slide", "pair_clamp", "roll_viscous", "roll_capped", "twist_viscous", "twist_capped",
          "wall_stick", "wall_slide", "wall_reset", "two_walls", "frozen_sprung")
# further counts a force pass leaves beside COUNTS (not part of the all-on fixture): slots in contact with a frozen row
# and a moving one; slots in contact
MRANK_COUNTS = ("frozen_touched", "touching")
CARRY = ("to_ghost", "to_owned", "vanished", "new", "owned_to_ghost", "ghost_to_owned")


def table(ntypes, entries, col=None):
    """(ntypes+1)^2 symmetric table from {(a, b): value or tuple}; col picks a tuple's entry."""
    t = np.zeros((ntypes + 1, ntypes + 1))
    for (a, b), val in (entries or {}).items():
        t[a, b] = t[b, a] = val if col is None else val[col]
    return t


def scene(lmax, nq, shapes, density, x, v, quat, angmom, type_, shtype, lo, hi, periodic, skin, dt, kn, expo, tag=None, mask=None,
          groupbit=1, gravity=(0.0, 0.0, 0.0), gamma_t=0.0, gamma_r=0.0, pair_damping=None, pair_friction=None, pair_spring=None,
          pair_rolling=None, pair_twisting=None, planes=None, wall_kn=None, wall_expo=None, wall_damping=None, wall_mu=None,
          wall_gt=None, wall_kt=None, wall_velocity=None, ledger=False, cylinders=None, cyl_kn=None, cyl_expo=None,
          cyl_damping=None, cyl_friction=None, cyl_rotation=None, cyl_spring=None, cyl_rolling=None, cyl_twisting=None,
          shell_ledger=False, cones=None, cone_kn=None, cone_expo=None, cone_damping=None, cone_friction=None, cone_rotation=None,
          cone_spring=None):
    """The inputs of a run as one dict of arrays.  kn, expo: (ntypes+1)^2 tables.  The pair options are dicts keyed by the
    type pair, as run.DeviceRun takes them; the wall options arrays of one entry per wall.  cylinders [nc][7] = a point on
    the axis, the unit axis, Rc, with cyl_kn, cyl_expo, cyl_damping, cyl_rotation (Omega), cyl_spring (k_t,c), scalars or
    [nc], and cyl_friction, cyl_rolling, cyl_twisting, each a (mu, gamma) of scalars or [nc]; without cylinders the
    dict has none of the cylinder entries.  cones [nk][8] as cone_ref.cone builds them, with cone_kn, cone_expo,
    cone_damping, cone_rotation (Omega), cone_spring (k_t,k), scalars or [nk], and cone_friction = (mu, gamma_t); without
    cones the dict has none of the cone entries."""
    n, nt = len(x), np.asarray(kn).shape[0] - 1
    nw = 0 if planes is None else len(planes)
    per = lambda a: np.zeros(nw) if a is None else np.broadcast_to(np.asarray(a, float), (nw,)).copy()
    rmax = np.array([O.shape_rmax(lmax, a) for a in shapes])
    s = dict(lmax=int(lmax), nq=int(nq), a_nm=np.array(shapes, float), rmax=rmax, density=np.asarray(density, float),
             massprops=np.array([O.mass_props(lmax, a) for a in shapes]),
             x=np.array(x, float), v=np.array(v, float), quat=np.array(quat, float), angmom=np.array(angmom, float),
             type=np.asarray(type_, np.int32), shtype=np.asarray(shtype, np.int32),
             tag=np.arange(n, dtype=np.int32) if tag is None else np.asarray(tag, np.int32),
             mask=np.ones(n, np.int32) if mask is None else np.asarray(mask, np.int32), groupbit=int(groupbit),
             lo=np.asarray(lo, float), hi=np.asarray(hi, float), periodic=np.asarray(periodic, np.int32), skin=float(skin),
             dt=float(dt), gravity=np.asarray(gravity, float), gamma_t=float(gamma_t), gamma_r=float(gamma_r),
             K=np.asarray(kn, float), E=np.asarray(expo, float), G=table(nt, pair_damping), MU=table(nt, pair_friction, 0),
             GT=table(nt, pair_friction, 1), KT=table(nt, pair_spring), MUR=table(nt, pair_rolling, 0),
             GR=table(nt, pair_rolling, 1), MUTW=table(nt, pair_twisting, 0), GTW=table(nt, pair_twisting, 1),
             planes=np.zeros((0, 4)) if planes is None else np.array(planes, float), wall_kn=per(wall_kn), wall_expo=per(wall_expo),
             wall_damping=per(wall_damping), wall_mu=per(wall_mu), wall_gt=per(wall_gt), wall_kt=per(wall_kt),
             wall_velocity=np.zeros((nw, 3)) if wall_velocity is None else np.array(wall_velocity, float).reshape(nw, 3),
             ledger=int(bool(ledger)))
    assert sorted(s["tag"].tolist()) == list(range(n)), "tags must be a permutation of the rows"
    if cylinders is not None and len(cylinders):
        nc = len(cylinders)
        perc = lambda a: np.zeros(nc) if a is None else np.broadcast_to(np.asarray(a, float), (nc,)).copy()
        two = lambda a: (None, None) if a is None else a
        s.update(cyl=np.array(cylinders, float).reshape(nc, 7), cyl_kn=perc(cyl_kn), cyl_expo=perc(cyl_expo),
                 cyl_damping=perc(cyl_damping), cyl_mu=perc(two(cyl_friction)[0]), cyl_gt=perc(two(cyl_friction)[1]),
                 cyl_omega=perc(cyl_rotation), cyl_kt=perc(cyl_spring), cyl_mur=perc(two(cyl_rolling)[0]),
                 cyl_gr=perc(two(cyl_rolling)[1]), cyl_mutw=perc(two(cyl_twisting)[0]), cyl_gtw=perc(two(cyl_twisting)[1]),
                 shell_ledger=int(bool(shell_ledger)))
        assert np.allclose(np.linalg.norm(s["cyl"][:, 3:6], axis=1), 1.0, atol=1e-14), "cylinder axes must be unit vectors"
    if cones is not None and len(cones):
        nk = len(cones)
        perk = lambda a: np.zeros(nk) if a is None else np.broadcast_to(np.asarray(a, float), (nk,)).copy()
        mu, gt = (None, None) if cone_friction is None else cone_friction
        s.update(cone=np.array(cones, float).reshape(nk, 8), cone_kn=perk(cone_kn), cone_expo=perk(cone_expo),
                 cone_damping=perk(cone_damping), cone_mu=perk(mu), cone_gt=perk(gt), cone_omega=perk(cone_rotation),
                 cone_kt=perk(cone_spring))
        assert np.allclose(np.linalg.norm(s["cone"][:, 3:6], axis=1), 1.0, atol=1e-14), "cone axes must be unit vectors"
        assert np.allclose(s["cone"][:, 6] ** 2 + s["cone"][:, 7] ** 2, 1.0, atol=1e-14), "(cos theta, sin theta)"
        coeff = any(s[k].any() for k in ("cone_damping", "cone_mu", "cone_gt", "cone_omega", "cone_kt"))
        assert not (coeff and (s["ledger"] or s.get("shell_ledger"))), "§2.22, §2.23: a cone coefficient beside a ledger"
    return s


def flags(sc):
    """Which passes a loop enqueues, by the rules of §2.10-§2.16."""
    fric = (sc["MU"] != 0) & (sc["GT"] != 0)
    hist = (sc["MU"] != 0) & (sc["KT"] != 0)
    roll = ((sc["MUR"] != 0) & (sc["GR"] != 0)).any() or ((sc["MUTW"] != 0) & (sc["GTW"] != 0)).any()
    nw = len(sc["planes"])
    cyl = {}
    if "cyl" in sc:
        cf, ch = (sc["cyl_mu"] != 0) & (sc["cyl_gt"] != 0), (sc["cyl_mu"] != 0) & (sc["cyl_kt"] != 0)
        kind = ((sc["cyl_mur"] != 0) & (sc["cyl_gr"] != 0)) | ((sc["cyl_mutw"] != 0) & (sc["cyl_gtw"] != 0))
        # cyl_coeff: the contact kernel is a dissipative or a spring instance, which with both ledgers on writes the
        # power rows itself (§2.20); cyl_roll: a cylinder has a kind of §2.21
        cyl = dict(cyl_friction=cf, cyl_history=ch, cyl_coeff=bool((sc["cyl_damping"] != 0).any() or cf.any() or ch.any()),
                   cyl_roll=bool(kind.any()))
    if "cone" in sc:
        kf, kh = (sc["cone_mu"] != 0) & (sc["cone_gt"] != 0), (sc["cone_mu"] != 0) & (sc["cone_kt"] != 0)
        # cone_history: the cones with a spring (any: the pass is conic_contact_device with dt); cone_reads_twists: the
        # pass is a dissipative or a spring instance
        cyl.update(cone_friction=kf, cone_history=kh,
                   cone_reads_twists=bool((sc["cone_damping"] != 0).any() or kf.any() or kh.any()))
    return dict(cyl, nc=len(sc["cyl"]) if "cyl" in sc else 0, nk=len(sc["cone"]) if "cone" in sc else 0,
                pair_pass=bool((sc["G"] != 0).any() or fric.any() or hist.any()), rolling=bool(roll), nw=nw,
                wall_moves=bool(nw and (WM.normal_speed(sc["planes"], sc["wall_velocity"]) != 0).any()),
                body=bool(sc["gravity"].any() or sc["gamma_t"] != 0 or sc["gamma_r"] != 0))


def brick_owner(x, lo, hi, periodic, grid):
    """The brick (ix, iy, iz) [n][3] that owns each row in a grid of equal bricks: floor((x - lo) / brick), clipped along a
    direction that is not periodic (a row outside the box there belongs to the outermost brick).  x: wrapped rows."""
    grid = np.asarray(grid)
    cell = np.floor((x - lo) / ((hi - lo) / grid)).astype(np.int64)
    for d in range(3):
        if periodic[d]:
            assert ((cell[:, d] >= 0) & (cell[:, d] < grid[d])).all(), "a row outside the box along a periodic direction"
    return np.clip(cell, 0, grid - 1)


def wrap(x, lo, hi, periodic):
    """§7: owned rows into [lo, hi) along the periodic directions; a row inside keeps its bits.  Returns the rows moved."""
    moved = np.zeros(len(x), bool)
    for d in range(3):
        if not periodic[d]:
            continue
        ln = hi[d] - lo[d]
        out = ~((x[:, d] >= lo[d]) & (x[:, d] < hi[d]))
        k = np.floor((x[out, d] - lo[d]) / ln)
        x[out, d] = x[out, d] - k * ln
        assert ((x[:, d] >= lo[d]) & (x[:, d] < hi[d])).all()
        moved |= out
    return moved


@contextlib.contextmanager
def _wall_sums_hook(noise):
    """wall_ref.wall_sums memoised for the length of one force pass (the wall pass and the ledger's powers ask for the same
    sums) and, for the noise run, scaled once per (particle, plane)."""
    plain, memo = W.wall_sums, {}

    def sums(lmax, anm, rmax, x, q, plane, nq):
        key = (int(lmax), float(rmax), np.asarray(x, float).tobytes(), np.asarray(q, float).tobytes(),
               np.asarray(plane, float).tobytes(), int(nq), np.asarray(anm, float).tobytes())
        if key not in memo:
            V, S, T, st = plain(lmax, anm, rmax, x, q, plane, nq)
            if noise is not None and st > 0:
                e = 1.0 + NOISE * noise.uniform(-1.0, 1.0)
                V, S, T = V * e, S * e, T * e
            memo[key] = (V, S, T, st)
        return memo[key]
    W.wall_sums = sums
    try:
        yield
    finally:
        W.wall_sums = plain


@contextlib.contextmanager
def _cyl_sums_hook(noise):
    """cyl_ref.cyl_sums memoised for the length of one cylinder pass (the contact, the couples and the powers ask for the
    same sums) and, for the noise run, scaled once per (particle, cylinder)."""
    plain, memo = Cy.cyl_sums, {}

    def sums(lmax, anm, rmax, x, q, cyl, nq, boundary=None):
        key = (int(lmax), float(rmax), np.asarray(x, float).tobytes(), np.asarray(q, float).tobytes(),
               np.asarray(cyl, float).tobytes(), int(nq), np.asarray(anm, float).tobytes())
        if key not in memo:
            V, S, T, st = plain(lmax, anm, rmax, x, q, cyl, nq)
            if noise is not None and st > 0:
                e = 1.0 + NOISE * noise.uniform(-1.0, 1.0)
                V, S, T = V * e, S * e, T * e
            memo[key] = (V, S, T, st)
        return memo[key]
    Cy.cyl_sums = sums
    try:
        yield
    finally:
        Cy.cyl_sums = plain


def cylinder_pass(sc, shp, rows, x, quat, tw, xi, live, dt, variant=None, noise=None, stale_rows=None):
    """The cylinder pass of item 11 on the given rows (indices into the owned rows): §2.18 + §2.19 from
    cyl_history_ref.cyl_forces_history, the couples of §2.21 and the power rows of §2.20 from cyl_roll_ref.cyl_roll on
    the same sums and the same springs.  xi, live: the state of those rows going in.  Returns dict f, torque (couples
    included) [len(rows)][3], xi, live (coming out; going in for dt = 0), kind, P and P0 [len(rows)][nc][3] (the power
    rows with and without the couples'), Fw {(row, c): the row's force on the wall}, sums {(k, c): (V, S_n, T_n)}, branch,
    NS.  stale_rows: the Fw of the previous pass (the wrong variant cyl_roll_stale_rows forms its couples from them)."""
    cyls, sh = sc["cyl"], sc["shtype"][rows]
    co = (sc["cyl_kn"], sc["cyl_expo"], sc["cyl_damping"], sc["cyl_mu"], sc["cyl_gt"], sc["cyl_omega"], sc["cyl_kt"])
    for k in range(len(rows)):
        for c in cyls:
            assert Cy.foot(x[k], c)[1] < c[6], "a centre is at or outside a cylinder"
    with _cyl_sums_hook(noise):
        r = CH.cyl_forces_history(shp, sc["nq"], x, quat, sh, tw, cyls, *co, xi, live, dt)
        sums = CR.reach_sums(shp, sc["nq"], x, quat, sh, cyls)
        rr = CR.cyl_roll(sums, len(rows), x, tw, cyls, co[0], co[1], sc["cyl_mur"], sc["cyl_gr"], sc["cyl_mutw"], sc["cyl_gtw"],
                         *co[2:], dt=dt, variant="omega_c_kept" if variant == "cyl_roll_omega_kept" else None, xi=xi, live=live)
    # one contact law, asked twice
    assert np.array_equal(r["f"], rr["f"]) and np.array_equal(r["torque"], rr["torque0"])
    cpl, P = rr["couple"], rr["P"]
    if variant == "cyl_roll_stale_rows" and stale_rows is not None:
        cpl, P = np.zeros_like(cpl), rr["P0"].copy()
        for (k, c) in sorted(sums):
            Fw = stale_rows.get((int(rows[k]), c), np.zeros(3))
            M, pr, wr, _, _ = CR.couple(Fw, x[k], cyls[c], tw[k, 3:], sc["cyl_omega"][c], sc["cyl_mur"][c], sc["cyl_gr"][c],
                                        sc["cyl_mutw"][c], sc["cyl_gtw"][c])
            cpl[k] += M
            P[k, c, 1] += pr
            P[k, c, 2] += wr
    return dict(f=r["f"], torque=r["torque"] + cpl, xi=r["xi"], live=r["live"], kind=r["kind"], P=P, P0=rr["P0"],
                Fw={(int(rows[k]), c): v for (k, c), v in rr["rows"].items()}, sums=sums, branch=rr["branch"], NS=rr["NS"])


@contextlib.contextmanager
def _cone_sums_hook(noise):
    """cone_ref.cone_sums memoised for the length of one cone pass (the contact and the counts ask for the same sums) and,
    for the noise run, scaled once per (particle, cone)."""
    plain, memo = Co.cone_sums, {}

    def sums(lmax, anm, rmax, x, q, co, nq, boundary=None):
        key = (int(lmax), float(rmax), np.asarray(x, float).tobytes(), np.asarray(q, float).tobytes(),
               np.asarray(co, float).tobytes(), int(nq), np.asarray(anm, float).tobytes())
        if key not in memo:
            V, S, T, st = plain(lmax, anm, rmax, x, q, co, nq)
            if noise is not None and st > 0:
                e = 1.0 + NOISE * noise.uniform(-1.0, 1.0)
                V, S, T = V * e, S * e, T * e
            memo[key] = (V, S, T, st)
        return memo[key]
    Co.cone_sums = sums
    try:
        yield
    finally:
        Co.cone_sums = plain


def cone_pass(sc, shp, rows, x, quat, tw, xi, live, dt, law=KH.EXACT, noise=None):
    """The cone pass of item 11 on the given rows (indices into the owned rows): §2.22 + §2.23 from
    conic_history_ref.cone_forces_history.  xi, live: the state of those rows going in.  Returns dict f, torque
    [len(rows)][3], xi, live (coming out; going in for dt = 0), kind, and per contact with V > 0 {(k, c): N}, the normal
    force pt |S_n| the friction is capped by (0: the damping clamped the pressure)."""
    cones = sc["cone"]
    co = (sc["cone_kn"], sc["cone_expo"], sc["cone_damping"], sc["cone_mu"], sc["cone_gt"], sc["cone_omega"], sc["cone_kt"])
    for k in range(len(rows)):
        for c in cones:
            assert Co.foot(x[k], c)[4] > 0, "a centre is at or outside a cone"
    N = {}
    with _cone_sums_hook(noise):
        r = KH.cone_forces_history(shp, sc["nq"], x, quat, sc["shtype"][rows], tw, cones, *co, xi, live, dt, law=law)
        for k in range(len(rows)):
            lmax, anm, rmax = shp[int(sc["shtype"][rows[k]])]
            for c in range(len(cones)):
                V, S, T, status = Co.cone_sums(lmax, anm, rmax, x[k], quat[k], cones[c], sc["nq"])
                if status > 0 and V > 0:
                    p = co[0][c] * co[1][c] * V ** (co[1][c] - 1)
                    N[(k, c)] = max(0.0, p + co[2][c] * (S @ tw[k, :3] + T @ tw[k, 3:])) * np.linalg.norm(S)
    assert len(N) == r["ncontacts"]
    return dict(f=r["f"], torque=r["torque"], xi=r["xi"], live=r["live"], kind=r["kind"], N=N)


def _elastic(pairs, pi, pj, x, type_, K, E, nall):
    """The elastic wrench of §2.7 from per-slot integrals (the noise run: the oracle's own f comes from unscaled ones)."""
    f, tq = np.zeros((nall, 3)), np.zeros((nall, 3))
    for s, (i, j) in enumerate(zip(pi, pj)):
        V, S, T = pairs[s, 0], pairs[s, 1:4], pairs[s, 4:7]
        if not V > 0:
            continue
        k, m = K[type_[i], type_[j]], E[type_[i], type_[j]]
        p = k * m * V ** (m - 1)
        f[i] -= p * S
        tq[i] -= p * T
        f[j] += p * S
        tq[j] += p * (T - np.cross(x[j] - x[i], S))
    return f, tq


def build(sc, st, variant=None):
    """Item 2, the rebuild: wrap, ghosts, half list, keys, and the carry of xi from the previous list (if any).  Returns the
    carry counts."""
    n = len(st["x"])
    box = sc["hi"] - sc["lo"]
    cmax = 2.0 * sc["rmax"].max() + sc["skin"]
    wrapped = wrap(st["x"], sc["lo"], sc["hi"], sc["periodic"])
    own, code = SR.images(st["x"], sc["lo"], sc["hi"], sc["periodic"], cmax)
    xa = np.concatenate([st["x"], st["x"][own] + SR.shift_of(code) * box])
    sha = np.concatenate([sc["shtype"], sc["shtype"][own]])
    taga = np.concatenate([sc["tag"], sc["tag"][own]])
    offs, jl = SR.half_list(n, xa, sha, taga, sc["rmax"], sc["skin"])
    keys = H.owner_tags(jl, n, tag=taga)
    counts = dict.fromkeys(CARRY, 0)
    old = st.get("offs") is not None
    if old:
        okeys = st["jl"].astype(np.int64) if variant == "carry_by_row" else st["keys"]
        nkeys = jl.astype(np.int64) if variant == "carry_by_row" else keys
        xi = H.carry(st["offs"], okeys, st["xi"], offs, nkeys)
        for i in range(n):                          # the four kinds, by the right key whatever the variant
            ok, oj = st["keys"][st["offs"][i]:st["offs"][i + 1]], st["jl"][st["offs"][i]:st["offs"][i + 1]]
            oxi = st["xi"][st["offs"][i]:st["offs"][i + 1]]
            nk, nj = keys[offs[i]:offs[i + 1]], jl[offs[i]:offs[i + 1]]
            counts["vanished"] += int((~np.isin(ok, nk)).sum())
            counts["new"] += int((~np.isin(nk, ok)).sum())
            for k, j in zip(nk, nj):
                hit = np.flatnonzero(ok == k)
                if hit.size and oxi[hit[0]].any():  # a loaded spring travels
                    counts["to_ghost" if j >= n else "to_owned"] += 1
                    if j >= n and oj[hit[0]] < n:
                        counts["owned_to_ghost"] += 1
                    if j < n and oj[hit[0]] >= n:
                        counts["ghost_to_owned"] += 1
    else:
        xi = np.zeros((len(jl), 3))
    st.update(own=own, code=code, offs=offs, jl=jl, keys=keys, xi=xi, xhold=st["x"].copy(), builds=st.get("builds", 0) + 1)
    counts["wrapped"] = int(wrapped.sum())
    return counts


def check(sc, st):
    """§7's rebuild test with its margin: (rebuild?, |max d^2 - (skin/2)^2| / (skin/2)^2)."""
    d = st["x"] - st["xhold"]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).max()
    trig2 = (0.5 * sc["skin"]) * (0.5 * sc["skin"])
    return bool(not d2 <= trig2), float(abs(d2 - trig2) / trig2) if trig2 > 0 else np.inf


def force_pass(sc, st, dt, advance, twist_from=None, variant=None, noise=None, memory=None, xi_dt=None, cyl_dt=None,
               cyl_twist_from=None, cone_dt=None, cone_twist_from=None):
    """Items 3 to 12 on the state's positions: f and torque of the owned rows, xi of pairs, walls, cylinders and cones
    advanced by dt (0: a look), the planes advanced if `advance`.  twist_from: (v, quat, angmom) the twists are formed from
    (default: the state's).  memory: what a wrong variant keeps from the previous pass.  xi_dt: the dt the two spring passes
    get where a wrong variant hands them another than the planes'; cyl_dt, cone_dt: the same for the cylinder pass and the
    cone pass; cyl_twist_from, cone_twist_from: (v, quat, angmom) a wrong variant forms that pass's twists from.  Returns
    (powers for the fold, counts)."""
    fl, n = flags(sc), len(st["x"])
    xi_dt = dt if xi_dt is None else xi_dt
    memory = {} if memory is None else memory
    own, box = st["own"], sc["hi"] - sc["lo"]
    group = (sc["mask"] & sc["groupbit"]) != 0
    shp = [(sc["lmax"], a, r) for a, r in zip(sc["a_nm"], sc["rmax"])]
    cnt = dict.fromkeys(COUNTS, 0)
    # 3. twists from the half-step v, angmom and the drifted quat; a ghost row takes its owner's
    tv, tq_, tl = twist_from or (st["v"], st["quat"], st["angmom"])
    tw = D.twists(sc["massprops"], sc["density"], tv, tq_, tl, sc["shtype"])
    twa = np.concatenate([tw, tw[own]])
    if variant == "ghost_twists_stale" and memory.get("tw") is not None:
        twa = np.concatenate([tw, memory["tw"][own]])
    # 4. forward: ghost x = owner + shift, ghost quat = owner's
    xa = np.concatenate([st["x"], st["x"][own] + SR.shift_of(st["code"]) * box])
    qa = np.concatenate([st["quat"], st["quat"][own]])
    tya, sha = np.concatenate([sc["type"], sc["type"][own]]), np.concatenate([sc["shtype"], sc["shtype"][own]])
    if variant == "ghost_type_one":
        tya = np.concatenate([sc["type"], np.ones(len(own), sc["type"].dtype)])
    # 5. clear, 6. pair integrals and the elastic wrench
    o = O.compute(shp, sc["K"], sc["E"], sc["nq"], n, xa, qa, tya, sha, np.arange(n, dtype=np.int32), st["offs"], st["jl"],
                  want_pairs=True)
    pairs = o["pairs"]
    pi, pj = D.expand(np.arange(n), st["offs"], st["jl"])
    if noise is not None:
        pairs = pairs * (1.0 + NOISE * noise.uniform(-1.0, 1.0, (len(pairs), 1)))
        f, tq = _elastic(pairs, pi, pj, xa, tya, sc["K"], sc["E"], len(xa))
    else:
        f, tq = o["f"], o["torque"]
    P = dict(pair=np.zeros(2), roll=0.0, pair_ran=False, wall=None)
    a = (pairs, pi, pj, xa, twa, tya)
    # the share of a slot in the fold: 1 (the wrong variant of item 13: a half where j is a ghost row)
    share = np.where(pj >= n, 0.5, 1.0) if variant == "ghost_slot_half_power" else None
    touching = pairs[:, 0] > 0
    frozen = ~group[np.concatenate([np.arange(n), own])[pj]] | ~group[pi]
    moving = np.abs(twa[pi]).sum(axis=1) + np.abs(twa[pj]).sum(axis=1) > 0
    cnt["touching"], cnt["frozen_touched"] = int(touching.sum()), int((touching & frozen & moving).sum())
    st["touch"] = touching
    # 7. the pair pass with dt: damping, friction, springs
    if fl["pair_pass"]:
        df, dtq, xi1, det = H.pair_history(*a, sha, sc["rmax"], sc["K"], sc["E"], sc["G"], sc["MU"], sc["GT"], sc["KT"], st["xi"],
                                           xi_dt, n)
        f, tq = f + df, tq + dtq
        pw = LG.pair_powers(*a, sha, sc["rmax"], sc["K"], sc["E"], sc["G"], sc["MU"], sc["GT"], n)
        hs = det["kind"] != H.NONE
        pw[hs, 1] = det["power"][hs]                # §2.14: a history slot's friction row is -F_t.v_t
        P["pair"], P["pair_ran"] = (pw if share is None else pw * share[:, None]).sum(axis=0), True
        _, _, dd = D.pair_damping(*a, sc["K"], sc["E"], sc["G"], n, details=True)
        cnt["pair_stick"], cnt["pair_slide"] = int((det["kind"] == H.STICK).sum()), int((det["kind"] == H.SLIDE).sum())
        cnt["pair_clamp"] = int((dd[:, 0] == -dd[:, 2]).sum())
        live = (det["kind"] == H.STICK) | (det["kind"] == H.SLIDE)
        fr = ~group[np.concatenate([np.arange(n), own])[pj]] | ~group[pi]
        mv = np.abs(twa[pi]).sum(axis=1) + np.abs(twa[pj]).sum(axis=1) > 0
        cnt["frozen_sprung"] = int((live & fr & mv & (np.abs(xi1).sum(axis=1) > 0)).sum())
        st["xi"] = xi1
    # 8. the rolling pass on the same integrals and twists
    if fl["rolling"]:
        ra = a
        if variant == "rolling_stale_integrals" and memory.get("pairs") is not None and len(memory["pairs"]) == len(pairs):
            ra = (memory["pairs"],) + a[1:]
        dtq, rd = RL.pair_rolling(*ra, sc["K"], sc["E"], sc["G"], sc["MUR"], sc["GR"], sc["MUTW"], sc["GTW"], n)
        if variant == "ghost_rolling_torque_lost":
            dtq = dtq.copy()
            dtq[n:] = 0.0
        tq = tq + dtq
        P["roll"] = float((rd["power"] if share is None else rd["power"] * share).sum())
        lr, lt = rd["live"] & rd["roll"], rd["live"] & rd["twist"]
        cnt["roll_viscous"], cnt["roll_capped"] = int((lr & ~rd["capped_r"]).sum()), int((lr & rd["capped_r"]).sum())
        cnt["twist_viscous"], cnt["twist_capped"] = int((lt & ~rd["capped_tw"]).sum()), int((lt & rd["capped_tw"]).sum())
    memory["pairs"] = pairs
    # 9. reverse: the ghost rows go home
    fo, to = f[:n].copy(), tq[:n].copy()
    np.add.at(fo, own, f[n:])
    np.add.at(to, own, tq[n:])
    # 10. wall advance by dt, ahead of the wall pass
    late = variant == "planes_late"
    if advance and fl["wall_moves"] and not late:
        st["planes"] = WM.advance(st["planes"], sc["wall_velocity"], dt, 1)
    # 11. the wall pass with dt on those twists: the group's rows only
    plane_rows, shell_rows = set(), set()
    if fl["nw"]:
        g = np.flatnonzero(group)
        wtw = tw
        if variant == "wall_stale_twists" and memory.get("tw") is not None:
            wtw = memory["tw"]
        assert (st["x"][g] @ st["planes"][:, :3].T - st["planes"][:, 3] > 0).all(), "a centre went behind a plane"
        with _wall_sums_hook(noise):
            wa = (shp, sc["nq"], st["x"][g], st["quat"][g], sc["shtype"][g], wtw[g], st["planes"], sc["wall_kn"], sc["wall_expo"],
                  sc["wall_damping"], sc["wall_mu"], sc["wall_gt"])
            r = WH.wall_forces_history(*wa, sc["wall_kt"], sc["wall_velocity"], st["wall_xi"][g], st["wall_live"][g], xi_dt)
            Pw, _ = LG.wall_powers(*wa, sc["wall_velocity"])
        fo[g] += r["f"]
        to[g] += r["torque"]
        Pw[:, :, 1] = 0.0
        for c in r["contacts"]:                    # P_f = -F_t.v_t: kappa |v_t|^2 without a spring, §2.15's row with one
            if np.isfinite(c[9]).all():
                Pw[c[0], c[1], 1] = -(c[5] @ c[9])
        P["wall"] = (Pw.sum(axis=0), r["wall_out"][:, 1:].copy())
        cnt["wall_stick"], cnt["wall_slide"] = int((r["kind"] == WH.STICK).sum()), int((r["kind"] == WH.SLIDE).sum())
        if xi_dt != 0:
            cnt["wall_reset"] = int((st["wall_live"][g] & ~r["live"]).sum())
        touch = np.zeros((len(g), fl["nw"]), int)
        for c in r["contacts"]:
            touch[c[0], c[1]] = 1
        cnt["two_walls"] = int((touch.sum(axis=1) >= 2).sum())
        st["wall_xi"][g], st["wall_live"][g] = r["xi"], r["live"]
        plane_rows = set(g[touch.any(axis=1)].tolist())
    # 11, second half. the cylinder pass with dt directly behind the planar pass: the same rows, the same twists; the
    # couples from the rows of THIS pass.  xi is keyed by the row: a rebuild moves nothing
    if fl["nc"]:
        cnt.update(dict.fromkeys(CYL_COUNTS, 0))
        cyl_dt = dt if cyl_dt is None else cyl_dt
        g = np.arange(n) if variant == "cyl_pushes_frozen" else np.flatnonzero(group)
        ctw = tw
        if variant == "cyl_stale_twists" and memory.get("tw") is not None:
            ctw = memory["tw"]
        if variant == "cyl_prekick_twists" and cyl_twist_from is not None:
            ctw = D.twists(sc["massprops"], sc["density"], *cyl_twist_from, sc["shtype"])
        r = cylinder_pass(sc, shp, g, st["x"][g], st["quat"][g], ctw[g], st["cyl_xi"][g], st["cyl_live"][g], cyl_dt, variant, noise,
                          memory.get("cyl_rows"))
        fo[g] += r["f"]
        to[g] += r["torque"]
        P["cyl"], P["cyl0"] = r["P"], r["P0"]
        memory["cyl_rows"] = r["Fw"]
        cnt["cyl_stick"], cnt["cyl_slide"] = int((r["kind"] == CH.STICK).sum()), int((r["kind"] == CH.SLIDE).sum())
        if cyl_dt != 0:
            cnt["cyl_reset"] = int((st["cyl_live"][g] & ~r["live"]).sum())
        contact = np.zeros((len(g), fl["nc"]), bool)
        for (k, c), (V, _, _) in r["sums"].items():
            contact[k, c] = V > 0
            cnt["cyl_clamp"] += int(V > 0 and r["NS"][(k, c)] == 0)
            cnt["plain_friction"] += int(V > 0 and r["NS"][(k, c)] > 0 and fl["cyl_friction"][c] and not fl["cyl_history"][c]
                                         and fl["cyl_history"].any())
        bc = CR.branch_counts(r["branch"])
        cnt["cyl_roll_viscous"], cnt["cyl_roll_capped"] = bc[("roll", CR.VISCOUS)], bc[("roll", CR.CAPPED)]
        cnt["cyl_twist_viscous"], cnt["cyl_twist_capped"] = bc[("twist", CR.VISCOUS)], bc[("twist", CR.CAPPED)]
        cnt["two_shells"] = int((contact.sum(axis=1) >= 2).sum())
        cnt["plane_and_shell"] = int(sum(int(i) in plane_rows for i in g[contact.any(axis=1)]))
        for i in np.flatnonzero(~group):
            h = [c[6] - Cy.foot(st["x"][i], c)[1] for c in sc["cyl"]]
            cnt["frozen_in_reach"] += int(any(0 < hc < sc["rmax"][sc["shtype"][i]] for hc in h))
        st["cyl_xi"][g], st["cyl_live"][g] = r["xi"], r["live"]
        shell_rows = set(g[contact.any(axis=1)].tolist())
    # 11, third part. the cone pass with dt directly behind the cylinder pass: the group's rows, the twists of item 3.
    # (xi_g, xi_theta, phi_c) is keyed by the row: a rebuild moves nothing and a wrap does not touch it
    if fl["nk"]:
        cnt.update(dict.fromkeys(CONE_COUNTS, 0))
        cone_dt = dt if cone_dt is None else cone_dt
        g = np.arange(n) if variant == "cone_pushes_frozen" else np.flatnonzero(group)
        ktw = tw
        if variant == "cone_stale_twists" and memory.get("tw") is not None:
            ktw = memory["tw"]
        if variant == "cone_prekick_twists" and cone_twist_from is not None:
            ktw = D.twists(sc["massprops"], sc["density"], *cone_twist_from, sc["shtype"])
        law = KH.NO_TRANSPORT if variant == "cone_transport_dropped" else KH.EXACT
        r = cone_pass(sc, shp, g, st["x"][g], st["quat"][g], ktw[g], st["cone_xi"][g], st["cone_live"][g], cone_dt, law, noise)
        fo[g] += r["f"]
        to[g] += r["torque"]
        cnt["cone_stick"], cnt["cone_slide"] = int((r["kind"] == KH.STICK).sum()), int((r["kind"] == KH.SLIDE).sum())
        if cone_dt != 0:
            cnt["cone_reset"] = int((st["cone_live"][g] & ~r["live"]).sum())
        contact = np.zeros((len(g), fl["nk"]), bool)
        for (k, c), N in r["N"].items():
            contact[k, c] = True
            cnt["cone_clamp"] += int(N == 0)
            cnt["cone_plain_friction"] += int(N > 0 and fl["cone_friction"][c] and not fl["cone_history"][c]
                                              and fl["cone_history"].any())
        touched = g[contact.any(axis=1)]
        cnt["two_cones"] = int((contact.sum(axis=1) >= 2).sum())
        cnt["plane_and_cone"] = int(sum(int(i) in plane_rows for i in touched))
        cnt["shell_and_cone"] = int(sum(int(i) in shell_rows for i in touched))
        for i in np.flatnonzero(~group):
            h = [Co.foot(st["x"][i], c)[4] for c in sc["cone"]]
            cnt["cone_frozen_in_reach"] += int(any(0 < hc < sc["rmax"][sc["shtype"][i]] for hc in h))
        st["cone_xi"][g], st["cone_live"][g] = r["xi"], r["live"]
    memory["tw"] = tw
    if advance and fl["wall_moves"] and late:
        st["planes"] = WM.advance(st["planes"], sc["wall_velocity"], dt, 1)
    # 12. body forces: gravity and drag on the group's rows, from the half-step v and angmom
    if fl["body"]:
        O.post_force(sc["massprops"], sc["density"], sc["gravity"], sc["gamma_t"], sc["gamma_r"], st["v"], st["quat"], st["angmom"],
                     sc["shtype"], sc["mask"], fo, to, groupbit=sc["groupbit"])
    st["f"], st["torque"] = fo, to
    return P, cnt


def fold(sc, st, P, dt, variant=None):
    """Item 13: dt times the powers the passes of this step left, once."""
    roll = 0.0 if (variant == "fold_skips_rolling" and P["pair_ran"]) else P["roll"]
    st["ledger"][0] += dt * P["pair"][0]
    st["ledger"][1] += dt * (P["pair"][1] + roll)
    if P["wall"] is not None:
        Pw, Fw = P["wall"]
        per = np.zeros((len(Pw), 3))
        per[:, :2] = dt * Pw
        per[:, 2] = -dt * (Fw * sc["wall_velocity"]).sum(axis=1)
        st["per_wall"] += per
        st["ledger"][2:] += per.sum(axis=0)
    if P.get("cyl") is not None and sc.get("shell_ledger"):
        # the shell rows go into the shell accumulator only (§2.20); the wrong variant: where a ledger instance of the
        # contact kernel wrote the rows, the couples' share is lost
        skip = variant == "shell_fold_skips_roll" and flags(sc)["cyl_coeff"]
        per, tot = SL.shell_fold(P["cyl0"] if skip else P["cyl"], dt)
        st["per_cylinder"] += per
        st["shell"] += tot


def setup(sc, variant=None, noise=None):
    """The state a driver starts from: first build, then the set-up force pass — a look (dt = 0): no advance, no fold."""
    n, nw = len(sc["x"]), len(sc["planes"])
    st = dict(x=sc["x"].copy(), v=sc["v"].copy(), quat=sc["quat"].copy(), angmom=sc["angmom"].copy(), planes=sc["planes"].copy(),
              wall_xi=np.zeros((n, nw, 3)), wall_live=np.zeros((n, nw), bool), ledger=np.zeros(5), per_wall=np.zeros((nw, 3)),
              steps=0, memory={})
    if "cyl" in sc:
        nc = len(sc["cyl"])
        st.update(cyl_xi=np.zeros((n, nc, 2)), cyl_live=np.zeros((n, nc), bool), shell=np.zeros(3), per_cylinder=np.zeros((nc, 3)))
    if "cone" in sc:
        nk = len(sc["cone"])
        st.update(cone_xi=np.zeros((n, nk, 3)), cone_live=np.zeros((n, nk), bool))
    build(sc, st)
    P, _ = force_pass(sc, st, 0.0, False, variant=variant, noise=noise, memory=st["memory"],
                      xi_dt=sc["dt"] if variant == "xi_in_setup" else None, cyl_dt=sc["dt"] if variant == "cyl_xi_in_setup" else None,
                      cone_dt=sc["dt"] if variant == "cone_xi_in_setup" else None)
    if variant == "shell_fold_in_setup" and sc["ledger"]:
        fold(sc, st, dict(P, pair=np.zeros(2), roll=0.0, wall=None), sc["dt"])
    return st


def step(sc, st, variant=None, noise=None, check_rebuild=True):
    """One step, in the order of docs/SPEC.md §6 "Order of a step with every model on".  Returns a record: rebuilt, margin,
    the branch counts and, at a rebuild, the carry counts."""
    dt, mp, rho = sc["dt"], sc["massprops"], sc["density"]
    before = (st["v"].copy(), st["quat"].copy(), st["angmom"].copy())
    # 1. half kick and drift
    O.nve(0, dt, mp, rho, st["x"], st["v"], st["quat"], st["angmom"], st["f"], st["torque"], sc["shtype"], sc["mask"], sc["groupbit"])
    # 2. neighbour check and rebuild, with the history carry
    rec = dict(rebuilt=False, margin=np.inf, carry=None)
    if check_rebuild:
        rec["rebuilt"], rec["margin"] = check(sc, st)
        if rec["rebuilt"]:
            rec["carry"] = build(sc, st, variant)
            if variant == "cone_drops_at_rebuild" and "cone_xi" in st:
                st["cone_xi"][:], st["cone_live"][:] = 0.0, False
    # 3. twists: from the half-step v, angmom and the drifted quat
    tf = None
    if variant == "twists_prekick":
        tf = (before[0], st["quat"], before[2])
    elif variant == "twists_old_quat":
        tf = (st["v"], before[1], st["angmom"])
    # 4 ... 12. forward, clear, integrals, pair pass, rolling pass, reverse, wall advance, wall pass, body forces
    P, cnt = force_pass(sc, st, dt, True, twist_from=tf, variant=variant, noise=noise, memory=st["memory"],
                        xi_dt=0.5 * dt if variant == "xi_half_dt" else None, cyl_dt=0.5 * dt if variant == "cyl_xi_half_dt" else None,
                        cyl_twist_from=(before[0], st["quat"], before[2]) if variant == "cyl_prekick_twists" else None,
                        cone_dt=0.5 * dt if variant == "cone_xi_half_dt" else None,
                        cone_twist_from=(before[0], st["quat"], before[2]) if variant == "cone_prekick_twists" else None)
    # 13. the ledger fold with dt
    if sc["ledger"]:
        fold(sc, st, P, dt, variant)
    # 14. the final half kick
    O.nve(1, dt, mp, rho, st["x"], st["v"], st["quat"], st["angmom"], st["f"], st["torque"], sc["shtype"], sc["mask"], sc["groupbit"])
    st["steps"] += 1
    rec["counts"] = cnt
    return rec


def snapshot(st):
    """What a fixture keeps of a state; pair xi with its (i, owner tag) keys."""
    n = len(st["x"])
    pi = np.repeat(np.arange(n), np.diff(st["offs"]))
    out = dict(x=st["x"].copy(), v=st["v"].copy(), quat=st["quat"].copy(), angmom=st["angmom"].copy(), f=st["f"].copy(),
               torque=st["torque"].copy(), xi=st["xi"].copy(), xi_i=pi.astype(np.int32), xi_key=np.asarray(st["keys"], np.int32),
               wall_xi=st["wall_xi"].copy(), wall_live=st["wall_live"].copy(), planes=st["planes"].copy(),
               ledger=st["ledger"].copy(), per_wall=st["per_wall"].copy(), builds=np.int32(st["builds"]),
               step=np.int32(st["steps"]))
    if "cyl_xi" in st:                             # a scene with cylinders
        out.update(cyl_xi=st["cyl_xi"].copy(), cyl_live=st["cyl_live"].copy(), shell=st["shell"].copy(),
                   per_cylinder=st["per_cylinder"].copy())
    if "cone_xi" in st:                            # a scene with cones
        out.update(cone_xi=st["cone_xi"].copy(), cone_live=st["cone_live"].copy())
    return out


def xi_by_key(xi_i, xi_key, xi):
    """{(i, owner tag): xi} of the slots whose xi is not zero."""
    return {(int(i), int(k)): v for i, k, v in zip(xi_i, xi_key, xi) if np.any(v != 0)}


def deviation(a, b):
    """The per-quantity deviation of two snapshots, each on its own scale (QUANTITIES): x, v, quat, angmom relative to the
    largest magnitude, xi (by key) and wall_xi to the largest |xi|, the ledger to the total dissipated."""
    out = {}
    for q in ("x", "v", "quat", "angmom"):
        out[q] = float(np.abs(a[q] - b[q]).max() / np.abs(b[q]).max())
    ka, kb = xi_by_key(a["xi_i"], a["xi_key"], a["xi"]), xi_by_key(b["xi_i"], b["xi_key"], b["xi"])
    sc = max([np.abs(v).max() for v in kb.values()], default=0.0)
    z = np.zeros(3)
    out["xi"] = float(max([np.abs(ka.get(k, z) - kb.get(k, z)).max() for k in set(ka) | set(kb)], default=0.0) / sc) if sc else 0.0
    sw = np.abs(b["wall_xi"]).max() if b["wall_xi"].size else 0.0
    out["wall_xi"] = float(np.abs(a["wall_xi"] - b["wall_xi"]).max() / sw) if sw else 0.0
    tot = abs(b["ledger"][:4].sum())
    led = max(np.abs(a["ledger"] - b["ledger"]).max(), np.abs(a["per_wall"] - b["per_wall"]).max() if b["per_wall"].size else 0.0)
    out["ledger"] = float(led / tot) if tot else 0.0
    if "cyl_xi" in b:                              # CYL_QUANTITIES: cyl_xi to the largest |xi|, the shell ledger to D_d + D_f
        sx = np.abs(b["cyl_xi"]).max() if b["cyl_xi"].size else 0.0
        out["cyl_xi"] = float(np.abs(a["cyl_xi"] - b["cyl_xi"]).max() / sx) if sx else 0.0
        tot = abs(b["shell"][:2].sum())
        led = max(np.abs(a["shell"] - b["shell"]).max(), np.abs(a["per_cylinder"] - b["per_cylinder"]).max())
        out["shell"] = float(led / tot) if tot else 0.0
    if "cone_xi" in b:                             # CONE_QUANTITIES: (xi_g, xi_theta) to the largest |xi|; phi_c in radians
        sx = np.abs(b["cone_xi"][..., :2]).max() if b["cone_xi"].size else 0.0
        out["cone_xi"] = float(np.abs(a["cone_xi"][..., :2] - b["cone_xi"][..., :2]).max() / sx) if sx else 0.0
        both = np.asarray(a["cone_live"], bool) & np.asarray(b["cone_live"], bool)
        d = (a["cone_xi"][..., 2] - b["cone_xi"][..., 2])[both]
        d = d - 2.0 * np.pi * np.ceil((d - np.pi) / (2.0 * np.pi))          # into (-pi, pi]
        out["cone_phi"] = float(np.abs(d).max()) if d.size else 0.0
    return out


def run(sc, nsteps, variant=None, noise=None, keep=None):
    """setup + nsteps steps.  Returns (snapshots {label: snapshot}, records [nsteps]); snapshots: "setup", "step1", every
    rebuilding step ("step<k>") and the last; keep: further steps to keep."""
    st = setup(sc, variant, noise)
    snaps, recs = {"setup": snapshot(st)}, []
    for k in range(1, nsteps + 1):
        rec = step(sc, st, variant, noise)
        recs.append(rec)
        if k == 1 or k == nsteps or rec["rebuilt"] or (keep and k in keep):
            snaps[f"step{k}"] = snapshot(st)
    return snaps, recs
