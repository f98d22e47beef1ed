"""CPU tests of the recorded scene tests/golden/traj_mrank.npz — the all-on scene without tangential springs, what the loop
over several ranks accepts — and of the wrong variants only a decomposition can make (traj_ref.MRANK_VARIANTS): the
fixture meets the conditions its recorder sets, every condition computed from the reference alone; the reference still
reproduces it bit for bit; permuted tags change nothing but the order of the sums; and without a periodic direction,
hence without ghost rows, each new variant is the right run."""
import os
import sys

import numpy as np
import pytest

import traj_ref as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_traj_mrank as M                      # noqa: E402
import make_traj_ref as M0                       # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return np.load(M.PATH)


@pytest.fixture(scope="module")
def rerun(fix):
    """The reference once more from the fixture's inputs, the whole run."""
    return TR.run(M.scene_of(fix), int(fix["nsteps"]))


def snap(fix, label):
    return {k[len(label) + 1:]: fix[k] for k in fix.files if k.startswith(label + "_")}


def test_fixture_meets_the_conditions_of_the_scene(fix):
    sc = M.scene_of(fix)
    names = [str(s) for s in fix["count_names"]]
    assert tuple(names) == TR.COUNTS + TR.MRANK_COUNTS
    cnt = {k: int(fix["counts"][:, names.index(k)].sum()) for k in names}
    labels = [str(s) for s in fix["labels"]]
    snaps = {lab: snap(fix, lab) for lab in labels}
    xs = M.build_rows(snaps, fix["rebuilt"])
    nb = int(fix["rebuilt"].sum()) + 1
    touch = [fix[f"touch_b{b}"] for b in range(nb)]
    assert len(xs) == nb == int(fix[f"step{int(fix['nsteps'])}_builds"]) and f"touch_b{nb}" not in fix.files
    mig = M.migration(sc, xs, M.GRID)
    cs = M.cross_slots(sc, xs, touch, M.GRID)
    print(cnt, "\nrebuilt at", (np.flatnonzero(fix["rebuilt"]) + 1).tolist(), "wrapped", fix["wrapped"].tolist(), "smallest margin",
          fix["margin"].min(), "\n2x2x2:", mig, "slots between ranks / and types per build", cs.tolist())
    assert M.conditions(sc, cnt, fix["rebuilt"], fix["wrapped"], list(fix["margin"]), xs, touch) == []
    assert np.array_equal(cs, fix["cross_slots"])
    # the scene: the all-on scene, springs off, tags a permutation that is not the identity, ledger on
    n = len(sc["x"])
    assert not sc["KT"].any() and not sc["wall_kt"].any() and sc["ledger"] == 1
    assert sorted(sc["tag"].tolist()) == list(range(n)) and (sc["tag"] != np.arange(n)).sum() > n // 2
    assert set(sc["type"]) == {1, 2} and set(sc["shtype"]) == {0, 1} and ((sc["mask"] & sc["groupbit"]) == 0).sum() >= 5
    for k in ("G", "MU", "GT", "MUR", "GR", "MUTW", "GTW", "wall_damping", "wall_mu", "wall_gt", "wall_velocity", "gravity"):
        assert sc[k].any(), k
    assert sc["gamma_t"] > 0 and sc["gamma_r"] > 0 and sc["periodic"].tolist() == [1, 1, 0]
    fl = TR.flags(sc)
    assert fl["pair_pass"] and fl["rolling"] and fl["wall_moves"] and fl["body"] and fl["nw"] == 3
    cmax = 2 * sc["rmax"].max() + sc["skin"]
    assert ((sc["hi"] - sc["lo"]) >= 2 * cmax).all()                      # two bricks fit along every axis
    # no spring ever loads, every ledger total moves, the belt does work
    last = snaps[labels[-1]]
    assert all(not snaps[lab]["xi"].any() and not snaps[lab]["wall_xi"].any() for lab in labels)
    assert (last["ledger"] != 0).all() and last["per_wall"][1, 2] != 0
    g = (sc["mask"] & sc["groupbit"]) != 0
    for lab in labels:
        s = snaps[lab]
        assert (s["x"][g] @ s["planes"][:, :3].T - s["planes"][:, 3] > 0).all(), lab
    assert fix["wall_reach"].shape == (int(fix["nsteps"]), n, 3) and fix["wall_reach"][:, :, :2].any() and not fix["wall_reach"][:, ~g].any()
    assert os.path.getsize(M.PATH) <= 1.25 * os.path.getsize(M0.PATH)


def test_fixture_bars_and_wrong_variants(fix):
    q = [str(s) for s in fix["quantities"]]
    assert tuple(q) == TR.QUANTITIES and [str(v) for v in fix["variants"]] == list(M.VARIANTS)
    assert set(TR.MRANK_VARIANTS) <= set(M.VARIANTS) and len(M.VARIANTS) == len(TR.VARIANTS) - len(M.NEED_SPRING) + 4
    Dq = dict(zip(q, fix["D"]))
    W = {str(v): dict(zip(q, row)) for v, row in zip(fix["variants"], fix["W"])}
    assert np.array_equal(fix["bar"], M.BAR_FACTOR * fix["D"])
    assert all(Dq[k] > 0 for k in M.QUANTITIES) and all(Dq[k] == 0 for k in M.SPRING)
    for name, row in W.items():
        print(f"{name:26s}" + " ".join(f"{k} {row[k] / (M.BAR_FACTOR * Dq[k]):9.2e}" for k in M.VARIANTS[name][1]), "(W / bar)")
    assert M.ratios(Dq, W) == []
    # what the issue names for the four
    mv = TR.MRANK_VARIANTS
    assert mv["ghost_twists_stale"][1] == mv["ghost_type_one"][1] == ("v", "angmom", "ledger")
    assert mv["ghost_rolling_torque_lost"][1] == ("angmom", "quat") and mv["ghost_slot_half_power"][1] == ("ledger",)
    assert all(W["ghost_slot_half_power"][k] == 0 for k in q if k != "ledger")
    assert not set(mv) & set(TR.VARIANTS)


def test_reference_reproduces_every_snapshot_bit_for_bit(fix, rerun):
    snaps, recs = rerun
    assert list(snaps) == [str(s) for s in fix["labels"]]
    for lab, s in snaps.items():
        want = snap(fix, lab)
        assert set(s) == set(want)
        for k, v in s.items():
            assert np.array_equal(np.asarray(v), want[k]), (lab, k)
    names = [str(s) for s in fix["count_names"]]
    assert [r["rebuilt"] for r in recs] == fix["rebuilt"].tolist()
    assert np.array_equal([r["margin"] for r in recs], fix["margin"])
    assert np.array_equal([[r["counts"][k] for k in names] for r in recs], fix["counts"])


def test_identity_tags_follow_the_same_trajectory(fix):
    """The scene's particles in the order of their tags, with the row index as the tag — what the single-rank loops see —
    through the first rebuild: the same pairs with the same integrated particle, so row for row after unpermuting the
    recorded trajectory up to the order of the sums, a relative 1e-16 per term; the fixture's bars, made for a relative
    1e-12 in every integral, hold with room."""
    sc = M.scene_of(fix)
    first = int(np.flatnonzero(fix["rebuilt"])[0]) + 1
    rows = np.argsort(sc["tag"])
    ident = dict(sc)
    for k in ("x", "v", "quat", "angmom", "type", "shtype", "mask"):
        ident[k] = sc[k][rows].copy()
    ident["tag"] = np.arange(len(rows), dtype=np.int32)
    snaps, recs = TR.run(ident, first)
    assert [r["rebuilt"] for r in recs] == fix["rebuilt"][:first].tolist() and recs[-1]["carry"]["wrapped"] > 0
    bar = dict(zip((str(q) for q in fix["quantities"]), fix["bar"]))
    for lab in ("setup", "step1", f"step{first}"):
        want = snap(fix, lab)
        got = dict(snaps[lab])
        for k in ("x", "v", "quat", "angmom", "f", "torque"):
            want[k] = want[k][rows]
        err = TR.deviation(got, dict(want, xi=got["xi"], xi_i=got["xi_i"], xi_key=got["xi_key"], wall_xi=got["wall_xi"]))
        print(lab, {k: f"{err[k]:.1e} / {bar[k]:.1e}" for k in M.QUANTITIES})
        assert all(err[k] <= bar[k] for k in M.QUANTITIES), (lab, err)
    want = snap(fix, "setup")["f"][rows]                                  # the same positions: the order of the sums alone
    assert np.abs(snaps["setup"]["f"] - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("variant", list(TR.MRANK_VARIANTS))
def test_without_ghost_rows_a_decomposition_variant_is_the_right_run(fix, variant):
    """No periodic direction: no image, no ghost row, nothing for the variant to break.  Two steps, bit for bit."""
    sc = dict(M.scene_of(fix))
    sc["periodic"] = np.zeros(3, np.int32)
    right, wrong = _open_run(sc, None), _open_run(sc, variant)
    assert right["pairs"] > 20 and right["ghosts"] == 0
    for k in ("x", "v", "quat", "angmom", "f", "torque", "ledger", "per_wall", "planes"):
        assert np.array_equal(right[k], wrong[k]), k
    assert right["ledger"][:2].min() > 0


_OPEN = {}


def _open_run(sc, variant):
    if variant not in _OPEN:
        st = TR.setup(sc, variant)
        for _ in range(2):
            TR.step(sc, st, variant)
        _OPEN[variant] = dict(TR.snapshot(st), pairs=len(st["jl"]), ghosts=len(st["own"]))
    return _OPEN[variant]
