"""Recorder of tests/golden/traj_all_on.npz: one small scene with every contact model on, followed by the whole-step
reference tests/traj_ref.py.  CPU only, minutes:

    python tests/golden/make_traj_ref.py

The fixture holds the inputs (in_*), the reference's state after the set-up force pass, after step 1, after every
rebuilding step and after the last step (<label>_*; the labels in `labels`), per step the rebuild decision with its margin
and the branch counts, per rebuild the carry counts, and the measured bar: D_q (the reference against itself with every
integral scaled by 1 + 1e-12 eta), the bars 10 D_q, and per wrong variant of traj_ref.VARIANTS its deviation W_q from the
right run.  The conditions on the scene are asserted here (`conditions`) and again by tests/test_traj_ref.py on the file.

The scene.  48 particles (L = 4, n_q = 8, two shapes of densities 1.3 and 0.8, both with a centre of mass off the SH
origin, two types) on three hcp layers in a box periodic in x and y and open in z, squeezed between a rising floor (a
piston: damping, friction, spring) and a ceiling without a coefficient; an oblique belt (friction, no spring) reaches the
bottom layer's rows at high x, which then touch two walls.  Every seventh particle is frozen.  The bed drifts along +x and
+y fast enough that rows leave the box between two rebuilds, and spins fast enough that the rolling and twisting couples
reach their caps.  22 steps: the rebuild of step 21 is the first at which five vanished slots have been seen, and one
more step leaves a last snapshot that is not a rebuilding step's.  The run loops take no tag array (run.DeviceRun and shstep_run_device build their lists with the row
index as the tag), so the scene's tags are the row indices; traj_ref itself takes any permutation
(tests/test_traj_ref.py runs one).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "lammps-spherharm_amd"), ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import traj_ref as TR                            # noqa: E402
from shpair import bed, shapes                   # noqa: E402

PATH = os.path.join(HERE, "traj_all_on.npz")
NSTEPS = 22
NOISE_SEED = 20261019
WRONG_FACTOR = 1000.0                            # W_q >= WRONG_FACTOR * bar for the quantities a variant names
BAR_FACTOR = 10.0                                # bar = BAR_FACTOR * D_q
MARGIN = 1.0e-6

PAIR = dict(pair_damping={(1, 1): 30.0, (2, 2): 800.0},
            pair_friction={(1, 1): (0.5, 20.0), (1, 2): (0.4, 40.0)},
            pair_spring={(1, 1): 4.0e3},
            pair_rolling={(1, 1): (0.02, 2.0), (1, 2): (0.03, 1.0)},
            pair_twisting={(1, 2): (0.02, 1.5), (2, 2): (0.03, 1.0)})


def all_on():
    """The scene of the fixture, as traj_ref.scene makes it."""
    lmax, nq, spacing = 4, 8, 1.9
    shp = [shapes.random_shape(lmax, 7100 + 17 * s, amp=0.2) for s in range(2)]
    # 4 x 4 x 3 hcp sites; the box is commensurate with the lattice in x and y (edges 7.6 and 6.58 >= 2 c_max = 6.26)
    dx, dy, dz = spacing, spacing * np.sqrt(3.0) / 2.0, spacing * np.sqrt(2.0 / 3.0)
    k, j, i = (a.ravel() for a in np.meshgrid(np.arange(3), np.arange(4), np.arange(4), indexing="ij"))
    pts = np.stack([(i + 0.5 * (j % 2) + 0.5 * (k % 2)) * dx, (j + (k % 2) / 3.0) * dy, k * dz], axis=1)
    lo, hi = np.zeros(3), np.array([4 * dx, 4 * dy, 0.0])
    pts[:, 0] = np.mod(pts[:, 0] + 0.9, hi[0])   # the last column starts close to the face it leaves through
    pts[:, 1] = np.mod(pts[:, 1] + 0.475, hi[1])
    n = len(pts)
    rng = np.random.default_rng(4711)
    x = pts + rng.uniform(-0.05, 0.05, pts.shape)
    zlo, zhi = x[:, 2].min(), x[:, 2].max()
    lo, hi = lo.copy(), hi.copy()
    lo[2], hi[2] = zlo - 3.0, zhi + 3.0
    quat = bed.random_quaternions(n, rng)
    shtype = rng.integers(0, 2, n).astype(np.int32)
    type_ = (1 + rng.integers(0, 2, n)).astype(np.int32)
    mask = np.ones(n, np.int32)
    mask[::7] = 4                                # outside the group: frozen
    v = np.array([9.0, 5.0, 0.0]) + 1.5 * rng.normal(size=(n, 3))
    L = 1.2 * rng.normal(size=(n, 3))
    v[:16:3, 2] += 6.0                           # some rows of the bottom layer outrun the floor: their springs reset
    v[mask == 4], L[mask == 4] = 0.0, 0.0
    K, E = np.zeros((3, 3)), np.ones((3, 3))
    K[1:, 1:], E[1:, 1:] = [[1000.0, 1500.0], [1500.0, 2000.0]], [[1.25, 1.5], [1.5, 1.25]]
    s, c = np.sin(0.1), np.cos(0.1)
    planes = [[0.0, 0.0, 1.0, zlo - 0.93],                               # the floor, rising
              [-s, 0.0, c, -s * (hi[0] - 1.0) + c * (zlo - 0.9)],        # the belt: within reach at high x only
              [0.0, 0.0, -1.0, -(zhi + 0.95)]]                           # the ceiling, no coefficient
    vel = [[0.0, 0.0, 4.0], [3.0 * c, 2.0, 3.0 * s], [0.0, 0.0, 0.0]]
    return TR.scene(lmax, nq, shp, [1.3, 0.8], x, v, quat, L, type_, shtype, lo, hi, (1, 1, 0), 0.3, 2.0e-3, K, E, mask=mask,
                    gravity=(0.0, 0.0, -9.81), gamma_t=0.05, gamma_r=0.02, planes=planes, wall_kn=[2000.0, 1500.0, 1000.0],
                    wall_expo=[1.25, 1.5, 1.25], wall_damping=[3000.0, 0.0, 0.0], wall_mu=[0.5, 0.4, 0.0], wall_gt=[20.0, 30.0, 0.0],
                    wall_kt=[4.0e3, 0.0, 0.0], wall_velocity=vel, ledger=True, **PAIR)


def totals(recs):
    """The sums of the conditions: per branch over the steps, per carry kind over the rebuilds."""
    cnt = {k: int(sum(r["counts"][k] for r in recs)) for k in TR.COUNTS}
    car = {k: int(sum(r["carry"][k] for r in recs if r["rebuilt"])) for k in TR.CARRY}
    car["rebuilds"] = int(sum(r["rebuilt"] for r in recs))
    car["rebuilds_with_wrap"] = int(sum(r["rebuilt"] and r["carry"]["wrapped"] > 0 for r in recs))
    return cnt, car


def conditions(cnt, car, margins):
    """The conditions on the scene, from the reference alone: a list of the ones that fail."""
    bad = []
    if car["rebuilds"] < 2:
        bad.append(f"rebuilds {car['rebuilds']} < 2")
    for k in ("to_ghost", "to_owned", "vanished", "new"):
        if car[k] < 5:
            bad.append(f"carry {k} {car[k]} < 5")
    if car["rebuilds_with_wrap"] < 1:
        bad.append("no rebuild in a step that wrapped a row")
    for k in ("pair_stick", "pair_slide", "pair_clamp", "roll_viscous", "roll_capped", "twist_viscous", "twist_capped"):
        if cnt[k] < 5:
            bad.append(f"{k} {cnt[k]} < 5 slot-steps")
    for k in ("wall_stick", "wall_slide", "wall_reset"):
        if cnt[k] < 3:
            bad.append(f"{k} {cnt[k]} < 3 particle-steps")
    if cnt["frozen_sprung"] < 1:
        bad.append("no frozen particle in a sprung contact with a moving neighbour")
    if cnt["two_walls"] < 1:
        bad.append("no particle touches two walls in one step")
    if min(margins) < MARGIN:
        bad.append(f"a rebuild decision has margin {min(margins):.2e} < {MARGIN:.0e}")
    return bad


def ratios(D, W):
    """The variants whose named quantities do not reach WRONG_FACTOR x bar: a list of strings."""
    bad = []
    for name, (_, named) in TR.VARIANTS.items():
        for q in named:
            if not W[name][q] >= WRONG_FACTOR * BAR_FACTOR * D[q]:
                bad.append(f"{name}: W_{q} = {W[name][q]:.2e} < {WRONG_FACTOR * BAR_FACTOR * D[q]:.2e}")
    return bad


def scene_of(fix):
    """The scene dict from a fixture's in_* entries."""
    return {k[3:]: fix[k] for k in fix.files if k.startswith("in_")}


def record(nsteps=NSTEPS, variants=True, verbose=True):
    sc = all_on()
    snaps, recs = TR.run(sc, nsteps)
    cnt, car = totals(recs)
    margins = [r["margin"] for r in recs]
    if verbose:
        print("counts", cnt, "\ncarry", car, "\nmin margin", min(margins), "rebuilt at",
              [k + 1 for k, r in enumerate(recs) if r["rebuilt"]], flush=True)
    bad = conditions(cnt, car, margins)
    assert not bad, bad
    last = f"step{nsteps}"
    noisy, nrecs = TR.run(sc, nsteps, noise=np.random.default_rng(NOISE_SEED))
    assert [r["rebuilt"] for r in nrecs] == [r["rebuilt"] for r in recs]
    D = TR.deviation(noisy[last], snaps[last])
    if verbose:
        print("D", D, flush=True)
    W = {}
    for name in (TR.VARIANTS if variants else ()):
        ws, _ = TR.run(sc, nsteps, variant=name)
        W[name] = TR.deviation(ws[last], snaps[last])
        if verbose:
            print(name, W[name], flush=True)
    if variants:
        bad = ratios(D, W)
        assert not bad, bad
    out = {"in_" + k: v for k, v in sc.items()}
    out["labels"] = np.array(list(snaps))
    for lab, s in snaps.items():
        out.update({f"{lab}_{k}": v for k, v in s.items()})
    out["nsteps"] = np.int32(nsteps)
    out["rebuilt"] = np.array([r["rebuilt"] for r in recs])
    out["margin"] = np.array(margins)
    out["count_names"] = np.array(TR.COUNTS)
    out["counts"] = np.array([[r["counts"][k] for k in TR.COUNTS] for r in recs], np.int32)
    out["carry_names"] = np.array(TR.CARRY + ("wrapped",))
    out["carry"] = np.array([[r["carry"][k] for k in TR.CARRY + ("wrapped",)] for r in recs if r["rebuilt"]], np.int32)
    out["quantities"] = np.array(TR.QUANTITIES)
    out["D"] = np.array([D[q] for q in TR.QUANTITIES])
    out["bar"] = BAR_FACTOR * out["D"]
    out["variants"] = np.array(list(W))
    out["W"] = np.array([[W[v][q] for q in TR.QUANTITIES] for v in W]).reshape(len(W), len(TR.QUANTITIES))
    np.savez_compressed(PATH, **out)
    return out


if __name__ == "__main__":
    record()
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
