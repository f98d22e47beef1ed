"""Recorder of tests/golden/traj_mrank.npz: the all-on scene of make_traj_ref.py without tangential springs — what the loop
over several ranks accepts (shhalo_run_device refuses the springs) — followed by the whole-step reference tests/traj_ref.py.
CPU only, minutes:

    python tests/golden/make_traj_mrank.py

The scene is make_traj_ref.all_on() with three inputs changed here: the pair spring and every wall k_t are 0; the tags are
a permutation of the rows (the loop over ranks takes a tag array, and the half list is decided by tag); the bed is shifted
along y, a periodic direction the walls do not depend on, so that rows cross the y cut of a 2 x 2 x 2 grid and the periodic
y face between rebuilds.  Two types, two shapes, frozen rows, pair damping, history-free friction, rolling, twisting, a
piston, a belt, gravity, drag and the ledger stay on.

The fixture has the format of traj_all_on.npz (in_*, <label>_*, per-step rebuild flags, margins and counts, D, bar,
variants, W; the spring quantities are 0) and, for the conditions a decomposition needs, per build the slots in contact
(touch_b<k>: row i, row of j's owner) and per step the rows within reach of each wall (wall_reach).  Ownership is decided
here from the reference alone: traj_ref.brick_owner on the wrapped rows of a build.  The conditions are asserted here
(`conditions`) and again by tests/test_traj_mrank_ref.py on the file.

The bars: D_q as in make_traj_ref.py (the reference against itself with every integral scaled by 1 + 1e-12 eta), bar =
10 D_q.  The wrong variants: those of traj_ref.VARIANTS that exist without springs, with the quantities they name there
less xi and wall_xi, and traj_ref.MRANK_VARIANTS; each must move what it names by 1000 bars, and ghost_slot_half_power
must leave everything but the ledger exactly where it was.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "lammps-spherharm_amd"), ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_traj_ref as M0                       # noqa: E402
import traj_ref as TR                            # noqa: E402

PATH = os.path.join(HERE, "traj_mrank.npz")
NSTEPS = 22
NOISE_SEED = 20261019
TAG_SEED = 48
Y_SHIFT = -0.575                                 # rows of two layers start 0.05 to 0.15 under the y cut and the y face
WRONG_FACTOR = M0.WRONG_FACTOR
BAR_FACTOR = M0.BAR_FACTOR
MARGIN = M0.MARGIN
GRID = (2, 2, 2)                                 # the grid the conditions on migration are set for
SPRING = ("xi", "wall_xi")
QUANTITIES = tuple(q for q in TR.QUANTITIES if q not in SPRING)
# the variants of the single-rank fixture that need a spring to exist
NEED_SPRING = ("xi_half_dt", "xi_in_setup", "carry_by_row")
VARIANTS = {k: (item, tuple(q for q in named if q not in SPRING)) for k, (item, named) in TR.VARIANTS.items()
            if k not in NEED_SPRING}
VARIANTS.update(TR.MRANK_VARIANTS)
LEDGER_ONLY = "ghost_slot_half_power"


def no_springs():
    """The scene of the fixture, as traj_ref.scene's dict."""
    sc = dict(M0.all_on())
    n = len(sc["x"])
    sc["KT"] = np.zeros_like(sc["KT"])
    sc["wall_kt"] = np.zeros_like(sc["wall_kt"])
    sc["tag"] = np.random.default_rng(TAG_SEED).permutation(n).astype(np.int32)
    x = sc["x"].copy()
    x[:, 1] = sc["lo"][1] + np.mod(x[:, 1] + Y_SHIFT - sc["lo"][1], sc["hi"][1] - sc["lo"][1])
    sc["x"] = x
    assert not (sc["planes"][:, 1] != 0).any(), "the walls must not depend on y"
    assert sc["ledger"] == 1 and TR.flags(sc)["pair_pass"] and TR.flags(sc)["rolling"]
    return sc


def touching(st):
    """[m][2]: row i and the row of j's owner of every slot in contact at the state's last force pass."""
    n = len(st["x"])
    pi = np.repeat(np.arange(n), np.diff(st["offs"]))
    pj = np.concatenate([np.arange(n), st["own"]])[st["jl"]]
    return np.stack([pi, pj], axis=1)[st["touch"]].astype(np.int32)


def wall_reach(sc, st):
    """[n][nw]: the group's rows whose bounding sphere reaches over each plane, at the positions and planes of the state's
    last wall pass."""
    group = (sc["mask"] & sc["groupbit"]) != 0
    gap = st["x"] @ st["planes"][:, :3].T - st["planes"][:, 3]
    return group[:, None] & (gap < sc["rmax"][sc["shtype"]][:, None])


def follow(sc, nsteps):
    """traj_ref.run with, beside its snapshots and records, the slots in contact at every build and the walls' reach at
    every step."""
    st = TR.setup(sc)
    snaps, recs, touch, reach = {"setup": TR.snapshot(st)}, [], [touching(st)], []
    for k in range(1, nsteps + 1):
        rec = TR.step(sc, st)
        recs.append(rec)
        reach.append(wall_reach(sc, st))
        if rec["rebuilt"]:
            touch.append(touching(st))
        if k == 1 or k == nsteps or rec["rebuilt"]:
            snaps[f"step{k}"] = TR.snapshot(st)
    return snaps, recs, touch, np.array(reach)


def build_rows(snaps, rebuilt):
    """The wrapped rows of every build: x of the set-up and of every rebuilding step (the second half kick moves no x)."""
    return [snaps["setup"]["x"]] + [snaps[f"step{k + 1}"]["x"] for k in np.flatnonzero(rebuilt)]


def rank_of(sc, x, grid):
    c = TR.brick_owner(x, sc["lo"], sc["hi"], sc["periodic"], grid)
    return (c[:, 0] * grid[1] + c[:, 1]) * grid[2] + c[:, 2], c


def migration(sc, xs, grid):
    """Over the builds of a grid: rows that change rank through the cut of each direction, through a periodic face, per
    rebuild, and the smallest number of rows a rank owns.  A row that changed its brick along a periodic direction and
    moved more than half the box there went through the face."""
    box = sc["hi"] - sc["lo"]
    cut, face, per_build, least = [0, 0, 0], 0, [], len(xs[0])
    for b, x in enumerate(xs):
        rk, c = rank_of(sc, x, grid)
        least = min(least, int(np.bincount(rk, minlength=int(np.prod(grid))).min()))
        if b:
            through_face = np.zeros(len(x), bool)
            for d in range(3):
                ch = c[:, d] != c0[:, d]
                far = (np.abs(x[:, d] - x0[:, d]) > 0.5 * box[d]) & bool(sc["periodic"][d])
                cut[d] += int((ch & ~far).sum())
                through_face |= ch & far
            face += int(through_face.sum())
            per_build.append(int((rk != rk0).sum()))
        x0, c0, rk0 = x, c, rk
    return dict(cut=cut, face=face, per_build=per_build, least=least)


def cross_slots(sc, xs, touch, grid):
    """Per build: the slots in contact between rows of different ranks, and those of them between different types."""
    out = []
    for x, t in zip(xs, touch):
        rk, _ = rank_of(sc, x, grid)
        cross = rk[t[:, 0]] != rk[t[:, 1]]
        out.append((int(cross.sum()), int((cross & (sc["type"][t[:, 0]] != sc["type"][t[:, 1]])).sum())))
    return np.array(out, np.int32)


def conditions(sc, cnt, rebuilt, wrapped, margins, xs, touch):
    """The conditions on the scene, from the reference alone: a list of the ones that fail."""
    bad = []
    if int(np.sum(rebuilt)) < 2:
        bad.append(f"rebuilds {int(np.sum(rebuilt))} < 2")
    if min(margins) < MARGIN:
        bad.append(f"a rebuild decision has margin {min(margins):.2e} < {MARGIN:.0e}")
    if not (np.asarray(wrapped) > 0).any():
        bad.append("no rebuild in a step that wrapped a row")
    for k in ("pair_clamp", "roll_viscous", "roll_capped", "twist_viscous", "twist_capped"):
        if cnt[k] < 5:
            bad.append(f"{k} {cnt[k]} < 5 slot-steps")
    if cnt["two_walls"] < 1:
        bad.append("no particle touches two walls in one step")
    if cnt["frozen_touched"] < 1:
        bad.append("no frozen row touched by a moving neighbour")
    m = migration(sc, xs, GRID)
    for d in range(3):
        if m["cut"][d] < 3:
            bad.append(f"{m['cut'][d]} < 3 rows change rank through the {'xyz'[d]} cut")
    if m["face"] < 3:
        bad.append(f"{m['face']} < 3 rows change rank through a periodic face")
    if sum(1 for k in m["per_build"] if k > 0) < 2:
        bad.append(f"rows change rank at fewer than two rebuilds: {m['per_build']}")
    if m["least"] < 1:
        bad.append("a rank owns no row at some build")
    cs = cross_slots(sc, xs, touch, GRID)
    if cs[:, 1].min() < 10:
        bad.append(f"slots in contact between ranks and types: {cs[:, 1].tolist()}, one under 10")
    return bad


def ratios(D, W):
    """The variants whose named quantities do not reach WRONG_FACTOR x bar, or that move what they must not."""
    bad = []
    for name, (_, named) in VARIANTS.items():
        for q in named:
            if not W[name][q] >= WRONG_FACTOR * BAR_FACTOR * D[q]:
                bad.append(f"{name}: W_{q} = {W[name][q]:.2e} < {WRONG_FACTOR * BAR_FACTOR * D[q]:.2e}")
    for q in TR.QUANTITIES:
        if q != "ledger" and W[LEDGER_ONLY][q] != 0.0:
            bad.append(f"{LEDGER_ONLY}: W_{q} = {W[LEDGER_ONLY][q]:.2e} is not 0")
    return bad


def scene_of(fix):
    return M0.scene_of(fix)


def record(nsteps=NSTEPS, verbose=True):
    sc = no_springs()
    snaps, recs, touch, reach = follow(sc, nsteps)
    names = TR.COUNTS + TR.MRANK_COUNTS
    cnt = {k: int(sum(r["counts"][k] for r in recs)) for k in names}
    rebuilt = np.array([r["rebuilt"] for r in recs])
    margins = [r["margin"] for r in recs]
    wrapped = [r["carry"]["wrapped"] for r in recs if r["rebuilt"]]
    xs = build_rows(snaps, rebuilt)
    if verbose:
        print("counts", cnt, "\nmin margin", min(margins), "rebuilt at", (np.flatnonzero(rebuilt) + 1).tolist(), "wrapped", wrapped)
        for g in ((2, 1, 1), (1, 2, 1), (1, 1, 2), GRID):
            print(g, migration(sc, xs, g), cross_slots(sc, xs, touch, g).tolist(), flush=True)
        print("ledger", snaps[f"step{nsteps}"]["ledger"], "\nper wall", snaps[f"step{nsteps}"]["per_wall"].tolist(), flush=True)
    bad = conditions(sc, cnt, rebuilt, wrapped, margins, xs, touch)
    assert not bad, bad
    last = f"step{nsteps}"
    assert (snaps[last]["ledger"] != 0).all() and snaps[last]["per_wall"][1, 2] != 0     # every total, and work on the belt
    noisy, nrecs = TR.run(sc, nsteps, noise=np.random.default_rng(NOISE_SEED))
    assert [r["rebuilt"] for r in nrecs] == rebuilt.tolist()
    D = TR.deviation(noisy[last], snaps[last])
    if verbose:
        print("D", D, flush=True)
    W = {}
    for name in VARIANTS:
        ws, _ = TR.run(sc, nsteps, variant=name)
        W[name] = TR.deviation(ws[last], snaps[last])
        if verbose:
            print(name, W[name], flush=True)
    bad = ratios(D, W)
    assert not bad, bad
    out = {"in_" + k: v for k, v in sc.items()}
    out["labels"] = np.array(list(snaps))
    for lab, s in snaps.items():
        out.update({f"{lab}_{k}": v for k, v in s.items()})
    out["nsteps"] = np.int32(nsteps)
    out["rebuilt"] = rebuilt
    out["margin"] = np.array(margins)
    out["count_names"] = np.array(names)
    out["counts"] = np.array([[r["counts"][k] for k in names] for r in recs], np.int32)
    out["wrapped"] = np.array(wrapped, np.int32)
    for b, t in enumerate(touch):
        out[f"touch_b{b}"] = t
    out["cross_slots"] = cross_slots(sc, xs, touch, GRID)
    out["wall_reach"] = reach
    out["quantities"] = np.array(TR.QUANTITIES)
    out["D"] = np.array([D[q] for q in TR.QUANTITIES])
    out["bar"] = BAR_FACTOR * out["D"]
    out["variants"] = np.array(list(W))
    out["W"] = np.array([[W[v][q] for q in TR.QUANTITIES] for v in W])
    np.savez_compressed(PATH, **out)
    return out


if __name__ == "__main__":
    record()
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
