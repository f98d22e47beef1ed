"""CPU tests of the cone half of item 11 of the whole-step reference tests/traj_ref.py (docs/SPEC.md §6, "Order of a step
with every model on") and of its recorded scene tests/golden/traj_hopper.npz: the fixture meets the conditions its
recorder sets and its wrong variants land far outside the bars, the reference still reproduces it, a scene without cone
entries takes the path it always took, the cone part of a force pass is conic_history_ref.cone_forces_history called with
that pass's inputs and nothing else, and neither the tags nor the order of the cones matter."""
import copy
import os
import sys

import numpy as np
import pytest

import cone_ref as Co
import conic_history_ref as KH
import damp_ref as D
import traj_ref as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_traj_drum as MD                      # noqa: E402
import make_traj_hopper as M                     # noqa: E402
import make_traj_ref as MA                       # noqa: E402

DRUM_SNAPSHOT = ("x", "v", "quat", "angmom", "f", "torque", "xi", "xi_i", "xi_key", "wall_xi", "wall_live", "planes", "ledger",
                 "per_wall", "builds", "step", "cyl_xi", "cyl_live", "shell", "per_cylinder")


@pytest.fixture(scope="module")
def fix():
    return np.load(M.PATH)


def snap(fix, label):
    return {k[len(label) + 1:]: fix[k] for k in fix.files if k.startswith(label + "_")}


def without_cones(sc):
    return {k: v for k, v in sc.items() if k not in M.CONE_KEYS}


# ---- 1. the fixture --------------------------------------------------------------------------------------------------------

def test_fixture_meets_the_conditions_of_the_scene(fix):
    names = [str(s) for s in fix["count_names"]]
    assert tuple(names) == M.COUNTS
    cnt = {k: int(fix["counts"][:, names.index(k)].sum()) for k in M.COUNTS}
    cnames = [str(s) for s in fix["carry_names"]]
    car = {k: int(fix["carry"][:, cnames.index(k)].sum()) for k in TR.CARRY}
    car["rebuilds"] = int(fix["rebuilt"].sum())
    print(cnt, car, "smallest margin", fix["margin"].min())
    assert M.conditions(cnt, car, list(fix["margin"])) == []
    nst = int(fix["nsteps"])
    assert 18 <= nst <= 24 and len(fix["carry"]) == car["rebuilds"] == int(fix[f"step{nst}_builds"]) - 1
    sc = M.scene_of(fix)
    snaps = {str(lab): snap(fix, str(lab)) for lab in fix["labels"]}
    # the restart step the GPU test uses: between two rebuilds, no rebuild, a transported conic state
    reb = np.flatnonzero(fix["rebuilt"]) + 1
    r = int(fix["restart"])
    assert reb.min() < r < reb.max() and r not in reb and f"step{r}" in snaps
    assert M.final_conditions(sc, snaps, r) == []
    assert sorted(snaps) == sorted({"setup", "step1", f"step{nst}", f"step{r}"} | {f"step{k}" for k in reb})
    # the scene is the one the issue describes
    n = len(sc["x"])
    assert 24 <= n <= 32 and sc["lmax"] == 4 and sc["nq"] == 8
    assert len(sc["a_nm"]) == 2 and sc["density"][0] != sc["density"][1] and set(sc["type"]) == {1, 2} and set(sc["shtype"]) == {0, 1}
    assert np.abs(sc["massprops"][:, 1:4]).max() > 0.05                   # a centre of mass off the SH origin
    assert sc["tag"].tolist() == list(range(n))
    assert not sc["periodic"].any() and sc["gravity"][2] < 0 and not sc["gravity"][:2].any() and sc["gamma_t"] > 0 and sc["gamma_r"] > 0
    assert sc["ledger"] == 0 and sc["shell_ledger"] == 0                   # §2.22, §2.23: no coefficient beside a ledger
    assert ((sc["mask"] & sc["groupbit"]) == 0).tolist() == [i % 7 == 0 for i in range(n)]
    for k in ("G", "MU", "GT", "KT", "MUR", "GR", "MUTW", "GTW"):          # every pair model of the all-on scene
        assert np.array_equal(sc[k], MA.scene_of(np.load(MA.PATH))[k]), k
    fl = TR.flags(sc)
    assert fl["nk"] == 3 and fl["nc"] == 1 and fl["nw"] == 1 and fl["wall_moves"] and sc["wall_kt"][0] != 0 and sc["wall_mu"][0] != 0
    assert fl["cyl_history"].tolist() == [True] and fl["cone_reads_twists"]
    # the hopper: axis +z, 25 to 40 degrees, turning, damping, friction, k_t; cone 1: oblique, another angle, friction
    # without k_t; cone 2: no coefficient
    cone = sc["cone"]
    th = np.degrees(np.arctan2(cone[:, 7], cone[:, 6]))
    assert np.array_equal(cone[0, 3:6], [0.0, 0.0, 1.0]) and 25 <= th[0] <= 40
    assert all(sc[k][0] != 0 for k in M.CONE_KEYS[3:])
    assert abs(cone[1, 5]) < 0.95 and abs(th[1] - th[0]) > 5
    assert fl["cone_friction"].tolist() == [True, True, False] and fl["cone_history"].tolist() == [True, False, False]
    assert sc["cone_omega"][1] == 0 and not any(sc[k][2] for k in M.CONE_KEYS[3:])
    # the plane closes the hopper on the apex side of the bed and rises
    assert sc["planes"][0, 2] > 0.99 and sc["planes"][0, :3] @ sc["wall_velocity"][0] > 0
    assert (sc["x"] @ sc["planes"][0, :3] > sc["planes"][0, 3]).all() and sc["planes"][0, 3] > 0
    assert os.path.getsize(M.PATH) <= 1.6 * os.path.getsize(MD.PATH)      # eleven snapshots (four rebuilds, el_) against six
    # the el_ run: the same scene, no cone coefficient, both ledgers
    el = M.el_scene_of(fix)
    assert set(el) == set(sc) and el["ledger"] == 1 and el["shell_ledger"] == 1 and not any(el[k].any() for k in M.CONE_KEYS[3:])
    differ = {k for k in sc if not np.array_equal(sc[k], el[k])}
    assert differ == {"ledger", "shell_ledger"} | set(M.CONE_KEYS[3:])
    last = snap(fix, f"el_step{int(fix['el_nsteps'])}")
    assert int(fix["el_nsteps"]) == 6 and not last["cone_live"].any() and last["ledger"][:4].sum() > 0 and last["shell"].any()


def test_fixture_bars_and_wrong_variants(fix):
    q = [str(s) for s in fix["quantities"]]
    assert tuple(q) == M.QUANTITIES and [str(v) for v in fix["variants"]] == list(TR.CONE_VARIANTS)
    assert M.QUANTITIES == ("x", "v", "quat", "angmom", "xi", "wall_xi", "cyl_xi", "cone_xi", "cone_phi")
    Dq = dict(zip(q, fix["D"]))
    W = {str(v): dict(zip(q, row)) for v, row in zip(fix["variants"], fix["W"])}
    assert np.array_equal(fix["bar"], M.BAR_FACTOR * fix["D"]) and (fix["D"] > 0).all()
    assert M.BAR_FACTOR == 10.0 and M.WRONG_FACTOR == 1000.0
    for name, row in W.items():
        print(f"{name:24s}" + " ".join(f"{k} {row[k] / (M.BAR_FACTOR * Dq[k]):9.2e}" for k in TR.CONE_VARIANTS[name][1]), "(W / bar)")
    assert M.ratios(Dq, W) == []
    assert all(len(named) >= 1 and set(named) <= set(q) for _, named in TR.CONE_VARIANTS.values())
    assert set(TR.CONE_QUANTITIES) <= {k for _, named in TR.CONE_VARIANTS.values() for k in named}
    eq = [str(s) for s in fix["el_quantities"]]
    assert tuple(eq) == M.EL_QUANTITIES and np.array_equal(fix["el_bar"], M.BAR_FACTOR * fix["el_D"]) and (fix["el_D"] > 0).all()


@pytest.fixture(scope="module")
def rerun(fix):
    """The reference from the fixture's inputs up to the first rebuilding step: the states, the records and, for the
    tests of the pass below, a copy of the state ahead of step 4."""
    sc = M.scene_of(fix)
    first = int(np.flatnonzero(fix["rebuilt"])[0]) + 1
    st = TR.setup(sc)
    got, recs, mid = {"setup": TR.snapshot(st)}, [], None
    for k in range(1, first + 1):
        if k == 4:
            mid = copy.deepcopy(st)
        recs.append(TR.step(sc, st))
        if k in (1, first):
            got[f"step{k}"] = TR.snapshot(st)
    return dict(sc=sc, got=got, recs=recs, mid=mid, first=first)


def test_reference_reproduces_the_fixture(fix, rerun):
    """Set-up, step 1 and the first rebuilding step bit for bit; decisions, margins and counts of the steps up to it; and
    the whole el_ run."""
    nst = rerun["first"]
    assert nst >= 4 and sorted(rerun["got"]) == sorted(["setup", "step1", f"step{nst}"])
    for lab, s in rerun["got"].items():
        want = snap(fix, lab)
        assert set(s) == set(want)
        for k, v in s.items():
            assert np.array_equal(np.asarray(v), want[k]), (lab, k)
    recs = rerun["recs"]
    assert [r["rebuilt"] for r in recs] == fix["rebuilt"][:nst].tolist() and recs[-1]["rebuilt"]
    assert np.array_equal([r["margin"] for r in recs], fix["margin"][:nst])
    assert np.array_equal([[r["counts"][k] for k in M.COUNTS] for r in recs], fix["counts"][:nst])
    el, n = M.el_scene_of(fix), int(fix["el_nsteps"])
    snaps, recs = TR.run(el, n)
    assert [r["rebuilt"] for r in recs] == fix["el_rebuilt"].tolist()
    for lab in ("setup", f"step{n}"):
        want = snap(fix, "el_" + lab)
        assert set(snaps[lab]) == set(want)
        for k, v in snaps[lab].items():
            assert np.array_equal(np.asarray(v), want[k]), ("el", lab, k)


# ---- 2. a scene without cones ---------------------------------------------------------------------------------------------------

def test_without_cone_entries_the_old_path_is_taken_bit_for_bit(fix):
    """The drum scene (no cone entry) through the extended code: the flags say no cone, the snapshots have the layout the
    drum fixture stores, and set-up and step 1 come out bit for bit as recorded.  And the hopper scene with its cone entries
    removed against the same scene with three cones that nothing reaches and no coefficient — the extended path, whose cone
    pass runs and adds exact zeros: the same bits in everything the old path keeps."""
    dfix = np.load(MD.PATH)
    drum = MD.scene_of(dfix)
    assert not set(drum) & set(M.CONE_KEYS) and TR.flags(drum)["nk"] == 0 and "cone_history" not in TR.flags(drum)
    st = TR.setup(drum)
    for lab in ("setup", "step1"):
        if lab == "step1":
            rec = TR.step(drum, st)
            assert set(rec["counts"]) == set(TR.COUNTS + TR.MRANK_COUNTS + TR.CYL_COUNTS)
        s = TR.snapshot(st)
        assert tuple(s) == DRUM_SNAPSHOT
        for key, v in s.items():
            assert np.array_equal(np.asarray(v), dfix[f"{lab}_{key}"]), (lab, key)
    assert set(TR.deviation(s, s)) == set(TR.QUANTITIES + TR.CYL_QUANTITIES)
    sc = M.scene_of(fix)
    plain = without_cones(sc)
    assert set(plain) == set(drum)
    far = dict(plain)
    cone = sc["cone"].copy()
    cone[:, :3] -= 1.0e3 * cone[:, 3:6]
    z = np.zeros(3)
    far.update(cone=cone, cone_kn=sc["cone_kn"], cone_expo=sc["cone_expo"], **{k: z for k in M.CONE_KEYS[3:]})
    a, b = TR.setup(plain), TR.setup(far)
    for k in range(3):
        sa, sb = TR.snapshot(a), TR.snapshot(b)
        assert tuple(sa) == DRUM_SNAPSHOT and set(sb) == set(sa) | {"cone_xi", "cone_live"}
        for key in DRUM_SNAPSHOT:
            assert np.array_equal(sa[key], sb[key]), (k, key)
        assert not sb["cone_live"].any() and not sb["cone_xi"].any()
        ra, rb = TR.step(plain, a), TR.step(far, b)
        assert all(ra["counts"][q] == rb["counts"][q] for q in ra["counts"]) and not any(rb["counts"][q] for q in TR.CONE_COUNTS)


# ---- 3. the cone part of a force pass is the per-pass reference and nothing else --------------------------------------------

@pytest.mark.parametrize("where", ["setup", "mid"])
def test_cone_part_of_a_force_pass_is_the_per_pass_reference(oracle, rerun, where):
    """In set-up (a look at the initial state) and ahead of step 4 (live springs, dt): the state goes through force_pass
    with and without the cone entries; what the cones contributed is compared bit for bit with cone_forces_history called
    directly on the group's rows, the twists of item 3 and the state going in.  Gravity and drag are taken out of both
    scenes (they read nothing the cones write), so that the cone wrench is the last term added to f and torque and
    `without + direct` must give the bits of `with`."""
    sc = dict(rerun["sc"], gravity=np.zeros(3), gamma_t=0.0, gamma_r=0.0)
    plain = without_cones(sc)
    n, nk = len(sc["x"]), len(sc["cone"])
    if where == "setup":
        st = TR.setup(plain)          # the state a set-up pass sees; its planes, list and (empty) histories
        st.update(cone_xi=np.zeros((n, nk, 3)), cone_live=np.zeros((n, nk), bool))
        dt, advance = 0.0, False
    else:
        st = copy.deepcopy(rerun["mid"])
        assert st["cone_live"].sum() >= 2 and st["steps"] == 3
        oracle.nve(0, sc["dt"], sc["massprops"], sc["density"], st["x"], st["v"], st["quat"], st["angmom"], st["f"], st["torque"],
                   sc["shtype"], sc["mask"], sc["groupbit"])
        assert not TR.check(sc, st)[0]
        dt, advance = sc["dt"], True
    g = np.flatnonzero((sc["mask"] & sc["groupbit"]) != 0)
    tw = D.twists(sc["massprops"], sc["density"], st["v"], st["quat"], st["angmom"], sc["shtype"])
    shp = [(sc["lmax"], a, r) for a, r in zip(sc["a_nm"], sc["rmax"])]
    xi0, live0 = st["cone_xi"].copy(), st["cone_live"].copy()
    a, b = copy.deepcopy(st), copy.deepcopy(st)
    _, ca = TR.force_pass(sc, a, dt, advance, memory=a["memory"])
    _, cb = TR.force_pass(plain, b, dt, advance, memory=b["memory"])
    for k in ("xi", "wall_xi", "wall_live", "planes", "cyl_xi", "cyl_live"):
        assert np.array_equal(a[k], b[k]), k                             # the cones touch nothing of the others'
    assert all(ca[k] == cb[k] for k in cb) and set(ca) == set(cb) | set(TR.CONE_COUNTS)
    r = KH.cone_forces_history(shp, sc["nq"], st["x"][g], st["quat"][g], sc["shtype"][g], tw[g], sc["cone"], sc["cone_kn"],
                               sc["cone_expo"], sc["cone_damping"], sc["cone_mu"], sc["cone_gt"], sc["cone_omega"], sc["cone_kt"],
                               xi0[g], live0[g], dt)
    assert r["ncontacts"] >= 8 and np.abs(r["f"]).max() > 0
    # state: the group's rows are the pass's, the others keep theirs
    frozen = np.setdiff1d(np.arange(n), g)
    assert np.array_equal(a["cone_xi"][g], r["xi"]) and np.array_equal(a["cone_live"][g], r["live"])
    assert not a["cone_xi"][frozen].any() and not a["cone_live"][frozen].any()
    if where == "setup":
        assert not a["cone_live"].any() and (r["kind"] != KH.NONE).any()
    else:
        assert r["live"].sum() >= 2 and not np.array_equal(r["xi"], xi0[g])
        assert ca["cone_stick"] + ca["cone_slide"] == r["live"].sum()
    # wrench: behind everything else, on the group's rows only
    assert np.array_equal(a["f"][g], b["f"][g] + r["f"]) and np.array_equal(a["torque"][g], b["torque"][g] + r["torque"])
    assert np.array_equal(a["f"][frozen], b["f"][frozen]) and np.array_equal(a["torque"][frozen], b["torque"][frozen])
    # a cone without a spring beside the history cone is cone_ref's plain law
    i, c = next((i, c) for i in range(len(g)) for c in (1, 2)
                if Co.cone_sums(*shp[sc["shtype"][g[i]]], st["x"][g[i]], st["quat"][g[i]], sc["cone"][c], sc["nq"])[0] > 0)
    V, S, T, _ = Co.cone_sums(*shp[sc["shtype"][g[i]]], st["x"][g[i]], st["quat"][g[i]], sc["cone"][c], sc["nq"])
    only = KH.cone_forces_history(shp, sc["nq"], st["x"][g[i]][None], st["quat"][g[i]][None], sc["shtype"][g[i]][None], tw[g[i]][None],
                                  sc["cone"][c][None], *(sc[k][c] for k in M.CONE_KEYS[1:]), np.zeros((1, 1, 3)),
                                  np.zeros((1, 1), bool), dt)
    F, tau, _, _ = Co.contact_wrench(V, S, T, st["x"][g[i]], sc["cone"][c], sc["cone_kn"][c], sc["cone_expo"][c], tw[g[i]],
                                     sc["cone_damping"][c], sc["cone_mu"][c], sc["cone_gt"][c], sc["cone_omega"][c])
    assert np.array_equal(only["f"][0], F) and np.array_equal(only["torque"][0], tau)


# ---- 4. tags and the order of the cones -----------------------------------------------------------------------------------------

def test_rows_permuted_under_their_tags_follow_the_same_trajectory(fix):
    """Up to the first rebuilding step, against the fixture within its bars: the conic state, keyed by the row, travels
    with the rows; pair xi is keyed by (row, owner tag) and is mapped back through the tags."""
    sc = M.scene_of(fix)
    n = len(sc["x"])
    perm = np.random.default_rng(5).permutation(n)
    ps = dict(sc)
    for k in ("x", "v", "quat", "angmom", "type", "shtype", "mask"):
        ps[k] = sc[k][perm].copy()
    ps["tag"] = perm.astype(np.int32)
    first = int(np.flatnonzero(fix["rebuilt"])[0]) + 1
    snaps, recs = TR.run(ps, first)
    assert [r["rebuilt"] for r in recs] == fix["rebuilt"][:first].tolist()
    got, want = snaps[f"step{first}"], snap(fix, f"step{first}")
    back = np.argsort(perm)
    got = dict(got, xi_i=perm[got["xi_i"]].astype(np.int32),
               **{k: got[k][back] for k in ("x", "v", "quat", "angmom", "wall_xi", "wall_live", "cyl_xi", "cyl_live", "cone_xi", "cone_live")})
    assert want["cone_live"].sum() >= 2 and np.array_equal(got["cone_live"], want["cone_live"])
    assert np.array_equal(got["cyl_live"], want["cyl_live"]) and np.array_equal(got["wall_live"], want["wall_live"])
    err, bar = TR.deviation(got, want), dict(zip((str(s) for s in fix["quantities"]), fix["bar"]))
    print("  ".join(f"{q} {err[q]:.1e} / {bar[q]:.1e}" for q in bar))
    assert all(err[q] <= bar[q] for q in bar)


def test_cones_in_another_order_follow_the_same_trajectory(fix):
    """The three cones relabelled: a particle's wrenches add in index order, so the run agrees within the bars, not bit
    for bit."""
    sc = M.scene_of(fix)
    order = np.array([2, 0, 1])
    ps = dict(sc)
    for k in M.CONE_KEYS:
        ps[k] = sc[k][order].copy()
    nst = int(fix["nsteps"])
    snaps, recs = TR.run(ps, nst)
    assert [r["rebuilt"] for r in recs] == fix["rebuilt"].tolist()
    got, want = snaps[f"step{nst}"], snap(fix, f"step{nst}")
    back = np.argsort(order)
    got = dict(got, cone_xi=got["cone_xi"][:, back], cone_live=got["cone_live"][:, back])
    assert np.array_equal(got["cone_live"], want["cone_live"])
    names = [str(s) for s in fix["count_names"]]
    assert np.array_equal([[r["counts"][k] for k in names] for r in recs], fix["counts"])
    err, bar = TR.deviation(got, want), dict(zip((str(s) for s in fix["quantities"]), fix["bar"]))
    print("  ".join(f"{q} {err[q]:.1e} / {bar[q]:.1e}" for q in bar))
    assert all(err[q] <= bar[q] for q in bar)
