"""Recorder of tests/golden/traj_drum.npz: a periodic drum with every cylinder model on, followed by the whole-step
reference tests/traj_ref.py.  CPU only, minutes:

    python tests/golden/make_traj_drum.py

The fixture holds what tests/golden/traj_all_on.npz holds (see make_traj_ref.py): the inputs (in_*), the reference's state
after the set-up pass, after step 1, after every rebuilding step, at the restart step and after the last step, per step the
rebuild decision, its margin and the branch counts (traj_ref.COUNTS + CYL_COUNTS), per rebuild the carry counts, D_q (the
reference against itself with every pair integral, wall sum and cylinder sum scaled by 1 + 1e-12 eta), the bars 10 D_q and
per wrong variant of traj_ref.CYL_VARIANTS its deviation W_q.  The conditions are asserted here (`conditions`) and again
by tests/test_traj_drum_ref.py on the file.

The scene.  28 particles (L = 4, n_q = 8, two shapes of densities 1.3 and 0.8 with off-centre mass, two types) in four
layers of seven (a ring of six about one) along the axis of a drum, the box periodic along that axis (x) only; every pair
model of the all-on scene.  Cylinder 0 is the drum: rotating, with damping, friction, a spring, rolling and twisting.
Cylinder 1 crosses it along y and contains the bed: friction without k_t and rolling only, so the pass mixes a history
cylinder with a plain-friction one.  Cylinder 2, along z, is elastic.  A chord plane under the bed rises and slides
(friction and a spring; §2.12), so item 10 runs ahead of both surface passes and the two bottom rows of every layer
touch it and the drum.  Every seventh row is frozen; rows 0, 7, 14, 21 sit on the ring, within reach of the drum.  Gravity,
drag, the ledger and the shell ledger are on.  The bed drifts along +x: the last layer leaves the box in the first steps
and the first rebuild wraps it.

What came out.  20 steps, rebuilds at 7, 12 and 18 (smallest margin 2.5e-2), the first two in steps that wrapped rows;
restart step 13 (no rebuild, every row inside the box, as at step 20).  Particle-steps: cyl_stick 27, cyl_slide 133,
cyl_reset 13, cyl_clamp 87, cyl_roll_viscous 107, cyl_roll_capped 83, cyl_twist_viscous 37, cyl_twist_capped 123,
plain_friction 30, plane_and_shell 63, two_shells 46, frozen_in_reach 80; pair_stick 66, pair_slide 203, wall_stick 7,
wall_slide 73.  Shell ledger at the end: drum (960.1, 674.8, 143.4), cylinder 1 (0, 33.3, 0), cylinder 2 zeros.
D_q: x 5.1e-13, v 8.4e-11, quat 3.6e-12, angmom 1.1e-10, xi 1.3e-12, wall_xi 1.0e-12, ledger 3.3e-13, cyl_xi 2.4e-12,
shell 1.9e-11; bars 10 D_q.  Smallest W_q / bar over a variant's named quantities: cyl_stale_twists 1.1e8 (v),
cyl_xi_half_dt 4.9e7 (v), cyl_xi_in_setup 4.3e7 (v), cyl_roll_stale_rows 5.0e7 (shell), cyl_roll_omega_kept 3.5e6 (shell),
shell_fold_skips_roll 4.6e7, shell_fold_in_setup 3.1e8, cyl_pushes_frozen 1.1e9 (shell), cyl_prekick_twists 5.2e7 (v):
every named quantity of every variant is past 1000 x bar, none was dropped.  cyl_pushes_frozen names cyl_xi and shell
only: rows outside the group are not integrated, so a wrench on them moves no trajectory; what it leaves is live springs
and power rows of frozen rows.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "lammps-spherharm_amd"), ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import traj_ref as TR                            # noqa: E402
from make_traj_ref import BAR_FACTOR, MARGIN, PAIR, WRONG_FACTOR, scene_of  # noqa: E402,F401
from shpair import bed, shapes                   # noqa: E402

PATH = os.path.join(HERE, "traj_drum.npz")
NSTEPS = 20
NOISE_SEED = 20261021
QUANTITIES = TR.QUANTITIES + TR.CYL_QUANTITIES
COUNTS = TR.COUNTS + TR.CYL_COUNTS
RING, SPACING, LAYERS = 1.9, 1.9, 4


def drum():
    """The scene of the fixture, as traj_ref.scene makes it."""
    lmax, nq = 4, 8
    shp = [shapes.random_shape(lmax, 7100 + 17 * s, amp=0.2) for s in range(2)]
    rng = np.random.default_rng(1821)
    lx = LAYERS * SPACING
    pts = []
    for k in range(LAYERS):
        xk = lx - 0.07 - (LAYERS - 1 - k) * SPACING        # the last layer starts close to the face it leaves through
        for j in range(6):                                 # the ring first: rows 0, 7, 14, 21 are ring rows
            a = np.pi / 3.0 * (j + k) + 0.1
            pts.append([xk, RING * np.cos(a), RING * np.sin(a)])
        pts.append([xk, 0.0, 0.0])
    pts = np.array(pts)
    n = len(pts)
    x = pts + rng.uniform(-0.04, 0.04, pts.shape)
    x[:, 0] = np.mod(x[:, 0], lx)
    lo, hi = np.array([0.0, -4.5, -4.5]), np.array([lx, 4.5, 4.5])
    quat = bed.random_quaternions(n, rng)
    shtype = rng.integers(0, 2, n).astype(np.int32)
    type_ = (1 + rng.integers(0, 2, n)).astype(np.int32)
    mask = np.ones(n, np.int32)
    mask[::7] = 4                                # outside the group: frozen
    v = np.array([9.0, 0.0, 0.0]) + 1.5 * rng.normal(size=(n, 3))
    L = 1.2 * rng.normal(size=(n, 3))
    rad = x[:, 1:] / np.linalg.norm(x[:, 1:], axis=1)[:, None]
    ring = np.arange(n) % 7 != 6
    v[2::5, 1:] -= 5.0 * rad[2::5] * ring[2::5, None]    # some ring rows outrun the shell: their springs reset
    L[3::4] *= 6.0                                       # and some spin fast enough for the caps of the couples
    v[mask == 4], L[mask == 4] = 0.0, 0.0
    K, E = np.zeros((3, 3)), np.ones((3, 3))
    K[1:, 1:], E[1:, 1:] = [[1000.0, 1500.0], [1500.0, 2000.0]], [[1.25, 1.5], [1.5, 1.25]]
    c = 0.5 * lx
    s8, c8 = np.sin(0.02), np.cos(0.02)
    cyls = [[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 2.93],                    # the drum
            [c, 0.0, 0.0, 0.0, 1.0, 0.0, 5.1],                       # across, along y: contains the bed
            [c, 0.0, 0.0, 0.0, 0.0, 1.0, 5.2]]                       # along z: elastic
    planes = [[s8, 0.0, c8, -2.70 * c8 + s8 * c]]                    # a chord under the bed, tilted about y
    vel = [[2.0, 1.0, 1.5]]
    return TR.scene(lmax, nq, shp, [1.3, 0.8], x, v, quat, L, type_, shtype, lo, hi, (1, 0, 0), 0.3, 2.0e-3, K, E, mask=mask,
                    gravity=(0.0, 0.0, -9.81), gamma_t=0.05, gamma_r=0.02, planes=planes, wall_kn=[2000.0], wall_expo=[1.25],
                    wall_damping=[500.0], wall_mu=[0.5], wall_gt=[20.0], wall_kt=[4.0e3], wall_velocity=vel, ledger=True,
                    cylinders=cyls, cyl_kn=[2000.0, 1500.0, 1000.0], cyl_expo=[1.25, 1.5, 1.25], cyl_damping=[3000.0, 0.0, 0.0],
                    cyl_friction=([0.5, 0.4, 0.0], [20.0, 30.0, 0.0]), cyl_rotation=[2.0, 0.0, 0.0], cyl_spring=[4.0e3, 0.0, 0.0],
                    cyl_rolling=([0.02, 0.03, 0.0], [2.0, 40.0, 0.0]), cyl_twisting=([0.02, 0.0, 0.0], [30.0, 0.0, 0.0]),
                    shell_ledger=True, **PAIR)


def totals(recs):
    """The sums of the conditions: per branch over the steps, per carry kind over the rebuilds."""
    cnt = {k: int(sum(r["counts"][k] for r in recs)) for k in COUNTS}
    car = {k: int(sum(r["carry"][k] for r in recs if r["rebuilt"])) for k in TR.CARRY}
    car["rebuilds"] = int(sum(r["rebuilt"] for r in recs))
    car["rebuilds_with_wrap"] = int(sum(r["rebuilt"] and r["carry"]["wrapped"] > 0 for r in recs))
    return cnt, car


def conditions(cnt, car, margins):
    """The conditions on the scene's run, from the reference alone: a list of the ones that fail."""
    bad = []
    if car["rebuilds"] < 2:
        bad.append(f"rebuilds {car['rebuilds']} < 2")
    if car["rebuilds_with_wrap"] < 1:
        bad.append("no rebuild in a step that wrapped a row")
    if min(margins) < MARGIN:
        bad.append(f"a rebuild decision has margin {min(margins):.2e} < {MARGIN:.0e}")
    for k in ("cyl_stick", "cyl_slide", "cyl_reset", "cyl_roll_viscous", "cyl_roll_capped", "cyl_twist_viscous", "cyl_twist_capped",
              "plain_friction"):
        if cnt[k] < 3:
            bad.append(f"{k} {cnt[k]} < 3 particle-steps")
    for k in ("cyl_clamp", "plane_and_shell", "two_shells", "frozen_in_reach"):
        if cnt[k] < 1:
            bad.append(f"{k}: none")
    for k in ("pair_stick", "pair_slide"):
        if cnt[k] < 5:
            bad.append(f"{k} {cnt[k]} < 5 slot-steps")
    if cnt["wall_stick"] + cnt["wall_slide"] < 3:
        bad.append("the wall spring is not live")
    return bad


def final_conditions(sc, snaps, last):
    """The conditions on the stored states: no centre outside a cylinder or behind the plane, the drum's row of the shell
    ledger non-zero in every entry, the elastic cylinder's all zero."""
    bad = []
    g = (sc["mask"] & sc["groupbit"]) != 0
    for lab, s in snaps.items():
        if not (s["x"][g] @ s["planes"][:, :3].T - s["planes"][:, 3] > 0).all():
            bad.append(f"{lab}: a centre behind the plane")
        for c in sc["cyl"]:
            y = s["x"] - c[:3]
            rho = y - (y @ c[3:6])[:, None] * c[3:6]
            if not (np.linalg.norm(rho, axis=1) < c[6]).all():
                bad.append(f"{lab}: a centre outside a cylinder")
    per = snaps[last]["per_cylinder"]
    if not (per[0] != 0).all():
        bad.append(f"the drum's shell row has a zero: {per[0]}")
    if per[2].any():
        bad.append(f"the elastic cylinder's shell row is not zero: {per[2]}")
    return bad


def ratios(D, W):
    """The variants whose named quantities do not reach WRONG_FACTOR x bar: a list of strings."""
    bad = []
    for name, (_, named) in TR.CYL_VARIANTS.items():
        for q in named:
            if not W[name][q] >= WRONG_FACTOR * BAR_FACTOR * D[q]:
                bad.append(f"{name}: W_{q} = {W[name][q]:.2e} < {WRONG_FACTOR * BAR_FACTOR * D[q]:.2e}")
    return bad


def restart_step(sc, snaps, recs):
    """The first step that does not rebuild, lies between two rebuilds and leaves every row inside the box along x."""
    reb = [k + 1 for k, r in enumerate(recs) if r["rebuilt"]]
    for k in range(reb[0] + 1, reb[-1]):
        if k not in reb and f"step{k}" in snaps:
            xs = snaps[f"step{k}"]["x"][:, 0]
            if ((xs >= sc["lo"][0]) & (xs < sc["hi"][0])).all():
                return k
    return 0


def record(nsteps=NSTEPS, variants=True, verbose=True):
    sc = drum()
    snaps, recs = TR.run(sc, nsteps, keep=range(1, nsteps + 1))
    cnt, car = totals(recs)
    margins = [r["margin"] for r in recs]
    reb = [k + 1 for k, r in enumerate(recs) if r["rebuilt"]]
    if verbose:
        print("counts", cnt, "\ncarry", car, "\nmin margin", min(margins), "rebuilt at", reb, flush=True)
    last = f"step{nsteps}"
    bad = conditions(cnt, car, margins) + final_conditions(sc, snaps, last)
    assert not bad, bad
    restart = restart_step(sc, snaps, recs)
    xs = snaps[last]["x"][:, 0]
    assert restart and ((xs >= sc["lo"][0]) & (xs < sc["hi"][0])).all(), "no restart step, or a row outside the box at the end"
    keep = {"setup", "step1", last, f"step{restart}"} | {f"step{k}" for k in reb}
    snaps = {lab: s for lab, s in snaps.items() if lab in keep}
    noisy, nrecs = TR.run(sc, nsteps, noise=np.random.default_rng(NOISE_SEED))
    assert [r["rebuilt"] for r in nrecs] == [r["rebuilt"] for r in recs]
    D = TR.deviation(noisy[last], snaps[last])
    if verbose:
        print("shell", snaps[last]["shell"], snaps[last]["per_cylinder"].tolist(), "restart", restart, "\nD", D, flush=True)
    W = {}
    for name in (TR.CYL_VARIANTS if variants else ()):
        ws, _ = TR.run(sc, nsteps, variant=name)
        W[name] = TR.deviation(ws[last], snaps[last])
        if verbose:
            print(name, {q: f"{W[name][q] / (BAR_FACTOR * D[q]):.1e}" for q in TR.CYL_VARIANTS[name][1]}, "(W / bar)", flush=True)
    if variants:
        bad = ratios(D, W)
        assert not bad, bad
    out = {"in_" + k: v for k, v in sc.items()}
    out["labels"] = np.array(list(snaps))
    for lab, s in snaps.items():
        out.update({f"{lab}_{k}": v for k, v in s.items()})
    out["nsteps"], out["restart"] = np.int32(nsteps), np.int32(restart)
    out["rebuilt"] = np.array([r["rebuilt"] for r in recs])
    out["margin"] = np.array(margins)
    out["count_names"] = np.array(COUNTS)
    out["counts"] = np.array([[r["counts"][k] for k in COUNTS] for r in recs], np.int32)
    out["carry_names"] = np.array(TR.CARRY + ("wrapped",))
    out["carry"] = np.array([[r["carry"][k] for k in TR.CARRY + ("wrapped",)] for r in recs if r["rebuilt"]], np.int32)
    out["quantities"] = np.array(QUANTITIES)
    out["D"] = np.array([D[q] for q in QUANTITIES])
    out["bar"] = BAR_FACTOR * out["D"]
    out["variants"] = np.array(list(W))
    out["W"] = np.array([[W[v][q] for q in QUANTITIES] for v in W]).reshape(len(W), len(QUANTITIES))
    np.savez_compressed(PATH, **out)
    return out


if __name__ == "__main__":
    record()
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
