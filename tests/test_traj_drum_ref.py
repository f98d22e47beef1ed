"""CPU tests of the cylinder items of the whole-step reference tests/traj_ref.py (docs/SPEC.md §6, "Order of a step with
every model on", items 11 and 13) and of its recorded scene tests/golden/traj_drum.npz: the fixture meets the conditions
its recorder sets and its wrong variants land far outside the bars, the reference still reproduces it, a scene without
cylinder entries takes the path it always took, the cylinder part of a force pass is the per-pass restatements called
with that pass's inputs and nothing else, and neither the tags nor the order of the cylinders matter."""
import copy
import os
import sys

import numpy as np
import pytest

import cyl_history_ref as CH
import cyl_roll_ref as CR
import damp_ref as D
import shell_ledger_ref as SL
import traj_ref as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_traj_drum as M                       # noqa: E402
import make_traj_ref as MA                       # noqa: E402

CYL_KEYS = ("cyl", "cyl_kn", "cyl_expo", "cyl_damping", "cyl_mu", "cyl_gt", "cyl_omega", "cyl_kt", "cyl_mur", "cyl_gr", "cyl_mutw",
            "cyl_gtw")
OLD_SNAPSHOT = ("x", "v", "quat", "angmom", "f", "torque", "xi", "xi_i", "xi_key", "wall_xi", "wall_live", "planes", "ledger",
                "per_wall", "builds", "step")


@pytest.fixture(scope="module")
def fix():
    return np.load(M.PATH)


def snap(fix, label):
    return {k[len(label) + 1:]: fix[k] for k in fix.files if k.startswith(label + "_")}


def without_cylinders(sc):
    return {k: v for k, v in sc.items() if k not in CYL_KEYS + ("shell_ledger",)}


# ---- 1. the fixture --------------------------------------------------------------------------------------------------------

def test_fixture_meets_the_conditions_of_the_scene(fix):
    names = [str(s) for s in fix["count_names"]]
    assert tuple(names) == M.COUNTS
    cnt = {k: int(fix["counts"][:, names.index(k)].sum()) for k in M.COUNTS}
    cnames = [str(s) for s in fix["carry_names"]]
    car = {k: int(fix["carry"][:, cnames.index(k)].sum()) for k in TR.CARRY}
    car["rebuilds"] = int(fix["rebuilt"].sum())
    car["rebuilds_with_wrap"] = int((fix["carry"][:, cnames.index("wrapped")] > 0).sum())
    print(cnt, car, "smallest margin", fix["margin"].min())
    assert M.conditions(cnt, car, list(fix["margin"])) == []
    nst = int(fix["nsteps"])
    assert len(fix["carry"]) == car["rebuilds"] == int(fix[f"step{nst}_builds"]) - 1
    sc = M.scene_of(fix)
    snaps = {str(lab): snap(fix, str(lab)) for lab in fix["labels"]}
    assert M.final_conditions(sc, snaps, f"step{nst}") == []
    per = snaps[f"step{nst}"]["per_cylinder"]
    assert np.allclose(per.sum(axis=0), snaps[f"step{nst}"]["shell"], rtol=1e-13, atol=0.0)
    assert per[2, 2] == 0.0 and per[1, 0] == 0.0            # W of the elastic cylinder exactly 0; no damping at cylinder 1
    # the scene is the one the issue describes
    n = len(sc["x"])
    assert 24 <= n <= 32 and sc["lmax"] == 4 and sc["nq"] == 8
    assert len(sc["a_nm"]) == 2 and sc["density"][0] != sc["density"][1] and set(sc["type"]) == {1, 2} and set(sc["shtype"]) == {0, 1}
    assert np.abs(sc["massprops"][:, 1:4]).max() > 0.05                   # a centre of mass off the SH origin
    assert sc["tag"].tolist() == list(range(n))
    assert sc["periodic"].tolist() == [1, 0, 0] and sc["gravity"].any() and sc["gamma_t"] > 0 and sc["gamma_r"] > 0
    assert sc["ledger"] == 1 and sc["shell_ledger"] == 1
    assert ((sc["mask"] & sc["groupbit"]) == 0).tolist() == [i % 7 == 0 for i in range(n)]
    cmax = 2 * sc["rmax"].max() + sc["skin"]
    assert (sc["hi"] - sc["lo"])[0] >= 2 * cmax                           # §7: a periodic edge is at least 2 c_max
    for k in ("G", "MU", "GT", "KT", "MUR", "GR", "MUTW", "GTW"):          # every pair model of the all-on scene
        assert np.array_equal(sc[k], MA.scene_of(np.load(MA.PATH))[k]), k
    fl = TR.flags(sc)
    assert fl["nc"] == 3 and fl["nw"] == 1 and fl["wall_moves"] and sc["wall_kt"][0] != 0 and sc["wall_mu"][0] != 0
    assert np.array_equal(sc["cyl"][0, 3:6], [1.0, 0.0, 0.0]) and abs(sc["cyl"][1, 3:6] @ sc["cyl"][0, 3:6]) < 1   # along the periodic axis
    # the drum: everything; cylinder 1: friction without k_t and one kind of couple; cylinder 2: no coefficient
    assert all(sc[k][0] != 0 for k in CYL_KEYS[3:])
    assert fl["cyl_friction"].tolist() == [True, True, False] and fl["cyl_history"].tolist() == [True, False, False]
    assert sc["cyl_mur"][1] * sc["cyl_gr"][1] != 0 and sc["cyl_mutw"][1] == 0 and sc["cyl_gtw"][1] == 0 and sc["cyl_damping"][1] == 0
    assert not any(sc[k][2] for k in CYL_KEYS[3:])
    # the restart step the GPU test uses: between two rebuilds, no rebuild, every row inside the box, as at the end
    reb = np.flatnonzero(fix["rebuilt"]) + 1
    r = int(fix["restart"])
    assert reb.min() < r < reb.max() and r not in reb and f"step{r}" in snaps
    for lab in (f"step{r}", f"step{nst}"):
        assert ((snaps[lab]["x"][:, 0] >= sc["lo"][0]) & (snaps[lab]["x"][:, 0] < sc["hi"][0])).all()
    assert snaps[f"step{r}"]["cyl_live"].sum() >= 3
    assert os.path.getsize(M.PATH) <= 1.25 * os.path.getsize(MA.PATH)


def test_fixture_bars_and_wrong_variants(fix):
    q = [str(s) for s in fix["quantities"]]
    assert tuple(q) == M.QUANTITIES and [str(v) for v in fix["variants"]] == list(TR.CYL_VARIANTS)
    Dq = dict(zip(q, fix["D"]))
    W = {str(v): dict(zip(q, row)) for v, row in zip(fix["variants"], fix["W"])}
    assert np.array_equal(fix["bar"], M.BAR_FACTOR * fix["D"]) and (fix["D"] > 0).all()
    assert M.BAR_FACTOR == 10.0 and M.WRONG_FACTOR == 1000.0
    for name, row in W.items():
        print(f"{name:24s}" + " ".join(f"{k} {row[k] / (M.BAR_FACTOR * Dq[k]):9.2e}" for k in TR.CYL_VARIANTS[name][1]), "(W / bar)")
    assert M.ratios(Dq, W) == []
    assert all(len(named) >= 1 for _, named in TR.CYL_VARIANTS.values())
    assert {"cyl_xi", "shell"} <= {k for _, named in TR.CYL_VARIANTS.values() for k in named}


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
    """Set-up, step 1 and the first rebuilding step bit for bit; decisions, margins and counts of the steps up to it."""
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


# ---- 2. a scene without cylinders ---------------------------------------------------------------------------------------------

def test_without_cylinder_entries_the_old_path_is_taken_bit_for_bit(fix):
    """The drum scene with its cylinder entries removed has the keys of the older fixtures and the snapshot layout they
    store.  Against it, the same scene with three cylinders that nothing reaches and no coefficient — the extended path,
    whose cylinder pass runs and adds exact zeros — gives the same bits in everything the old path keeps: what the
    extension does outside the cylinder pass is nothing.  And the first steps of traj_all_on.npz still come out bit for bit."""
    sc = M.scene_of(fix)
    plain = without_cylinders(sc)
    old = MA.scene_of(np.load(MA.PATH))
    assert set(plain) == set(old)
    far = dict(plain)
    cyl = sc["cyl"].copy()
    cyl[:, 6] = 1.0e3
    z = np.zeros(3)
    far.update(cyl=cyl, cyl_kn=sc["cyl_kn"], cyl_expo=sc["cyl_expo"], shell_ledger=1, **{k: z for k in CYL_KEYS[3:]})
    a, b = TR.setup(plain), TR.setup(far)
    for k in range(3):
        sa, sb = TR.snapshot(a), TR.snapshot(b)
        assert tuple(sa) == OLD_SNAPSHOT and set(sb) == set(sa) | {"cyl_xi", "cyl_live", "shell", "per_cylinder"}
        for key in OLD_SNAPSHOT:
            assert np.array_equal(sa[key], sb[key]), (k, key)
        assert not sb["cyl_live"].any() and not sb["shell"].any()
        ra, rb = TR.step(plain, a), TR.step(far, b)
        assert set(ra["counts"]) == set(TR.COUNTS + TR.MRANK_COUNTS) and all(ra["counts"][q] == rb["counts"][q] for q in ra["counts"])
    assert set(TR.deviation(TR.snapshot(a), TR.snapshot(a))) == set(TR.QUANTITIES)
    # the all-on fixture
    afix = np.load(MA.PATH)
    st = TR.setup(old)
    for lab in ("setup", "step1"):
        if lab == "step1":
            TR.step(old, st)
        s = TR.snapshot(st)
        assert tuple(s) == OLD_SNAPSHOT
        for key, v in s.items():
            assert np.array_equal(np.asarray(v), afix[f"{lab}_{key}"]), (lab, key)


# ---- 3. the cylinder part of a force pass is the per-pass restatements and nothing else -------------------------------------

def _pass_inputs(sc, st):
    g = np.flatnonzero((sc["mask"] & sc["groupbit"]) != 0)
    tw = D.twists(sc["massprops"], sc["density"], st["v"], st["quat"], st["angmom"], sc["shtype"])
    shp = [(sc["lmax"], a, r) for a, r in zip(sc["a_nm"], sc["rmax"])]
    co = (sc["cyl"], sc["cyl_kn"], sc["cyl_expo"], sc["cyl_damping"], sc["cyl_mu"], sc["cyl_gt"], sc["cyl_omega"], sc["cyl_kt"])
    return g, tw, shp, co


@pytest.mark.parametrize("where", ["setup", "mid"])
def test_cylinder_part_of_a_force_pass_is_the_per_pass_references(oracle, rerun, where):
    """In set-up (a look at the initial state) and ahead of step 4 (live springs, dt): the state goes through force_pass
    with and without the cylinder entries; what the cylinders contributed is compared with cyl_forces_history, cyl_roll
    and shell_pass called directly with that pass's inputs.  xi, live and the power rows bit for bit; f and torque, which
    can only be recovered by a subtraction, to 4 ulp of the largest force."""
    sc = rerun["sc"]
    plain = without_cylinders(sc)
    if where == "setup":
        st = TR.setup(plain)          # the state a set-up pass sees; its planes, list and (empty) histories
        st.update(cyl_xi=np.zeros((len(sc["x"]), 3, 2)), cyl_live=np.zeros((len(sc["x"]), 3), bool), shell=np.zeros(3),
                  per_cylinder=np.zeros((3, 3)))
        dt, advance = 0.0, False
    else:
        st = copy.deepcopy(rerun["mid"])
        assert st["cyl_live"].sum() >= 3 and st["steps"] == 3
        oracle.nve(0, sc["dt"], sc["massprops"], sc["density"], st["x"], st["v"], st["quat"], st["angmom"], st["f"], st["torque"],
                   sc["shtype"], sc["mask"], sc["groupbit"])
        assert not TR.check(sc, st)[0]
        dt, advance = sc["dt"], True
    g, tw, shp, co = _pass_inputs(sc, st)
    xi0, live0 = st["cyl_xi"].copy(), st["cyl_live"].copy()
    a, b = copy.deepcopy(st), copy.deepcopy(st)
    Pa, _ = TR.force_pass(sc, a, dt, advance, memory=a["memory"])
    TR.force_pass(plain, b, dt, advance, memory=b["memory"])
    for k in ("xi", "wall_xi", "wall_live", "planes"):
        assert np.array_equal(a[k], b[k]), k                             # the cylinders touch nothing of the others'
    # the direct calls
    x, q, sh = st["x"][g], st["quat"][g], sc["shtype"][g]
    r = CH.cyl_forces_history(shp, sc["nq"], x, q, sh, tw[g], *co, xi0[g], live0[g], dt)
    sums = CR.reach_sums(shp, sc["nq"], x, q, sh, sc["cyl"])
    rr = CR.cyl_roll(sums, len(g), x, tw[g], sc["cyl"], sc["cyl_kn"], sc["cyl_expo"], sc["cyl_mur"], sc["cyl_gr"], sc["cyl_mutw"],
                     sc["cyl_gtw"], *co[3:], dt=dt, xi=xi0[g], live=live0[g])
    sp = SL.shell_pass(shp, sc["nq"], x, q, sh, tw[g], *co, xi0[g], live0[g], dt)
    assert r["ncontacts"] >= 8 and np.abs(rr["couple"]).max() > 0
    # state: the group's rows are the pass's, the others keep theirs
    frozen = np.setdiff1d(np.arange(len(st["x"])), g)
    assert np.array_equal(a["cyl_xi"][g], r["xi"]) and np.array_equal(a["cyl_live"][g], r["live"])
    assert np.array_equal(a["cyl_xi"][frozen], xi0[frozen]) and not a["cyl_live"][frozen].any()
    if where == "setup":
        assert not a["cyl_live"].any()
    else:
        assert r["live"].sum() >= 3 and not np.array_equal(r["xi"], xi0[g])
    # power rows: cyl_roll's, whose contact part is shell_pass's
    assert np.array_equal(Pa["cyl"], rr["P"]) and np.array_equal(Pa["cyl0"], rr["P0"]) and np.array_equal(rr["P0"], sp["P"])
    assert np.array_equal(sp["f"], r["f"]) and np.array_equal(sp["torque"], r["torque"]) and np.array_equal(sp["xi"], r["xi"])
    assert (rr["P"][:, :, 1] != rr["P0"][:, :, 1]).any()
    # wrench
    tol = 4 * np.finfo(float).eps * max(np.abs(a["f"]).max(), np.abs(a["torque"]).max())
    assert np.abs((a["f"] - b["f"])[g] - r["f"]).max() <= tol
    assert np.abs((a["torque"] - b["torque"])[g] - (r["torque"] + rr["couple"])).max() <= tol
    assert np.array_equal(a["f"][frozen], b["f"][frozen]) and np.array_equal(a["torque"][frozen], b["torque"][frozen])
    # the fold: shell_fold of those rows with dt, into the shell accumulator alone
    c = copy.deepcopy(a)
    TR.fold(sc, c, Pa, sc["dt"])
    per, tot = SL.shell_fold(rr["P"], sc["dt"])
    assert np.array_equal(c["per_cylinder"], a["per_cylinder"] + per) and np.array_equal(c["shell"], a["shell"] + tot)
    d = copy.deepcopy(a)
    TR.fold(plain, d, dict(Pa, cyl=None), sc["dt"])
    assert np.array_equal(c["ledger"], d["ledger"]) and np.array_equal(c["per_wall"], d["per_wall"])


# ---- 4. tags and the order of the cylinders -------------------------------------------------------------------------------------

def test_rows_permuted_under_their_tags_follow_the_same_trajectory(fix):
    """As tests/test_traj_ref.py's: the same trajectory row for row up to the order of the sums (its tolerances); the
    cylinder springs, keyed by the row, travel with the rows."""
    sc = M.scene_of(fix)
    n = len(sc["x"])
    perm = np.random.default_rng(5).permutation(n)
    ps = dict(sc)
    for k in ("x", "v", "quat", "angmom", "type", "shtype", "mask"):
        ps[k] = sc[k][perm].copy()
    ps["tag"] = perm.astype(np.int32)
    a, b = TR.setup(sc), TR.setup(ps)
    for _ in range(2):
        TR.step(sc, a)
        TR.step(ps, b)
    for k in ("x", "v", "quat", "angmom"):
        assert np.abs(b[k] - a[k][perm]).max() <= 1e-11 * np.abs(a[k]).max(), k
    assert a["cyl_live"].sum() >= 3 and np.array_equal(b["cyl_live"], a["cyl_live"][perm])
    assert np.abs(b["cyl_xi"] - a["cyl_xi"][perm]).max() <= 1e-10 * np.abs(a["cyl_xi"]).max()
    assert np.abs(b["per_cylinder"] - a["per_cylinder"]).max() <= 1e-10 * np.abs(a["shell"][:2]).sum()


def test_cylinders_in_another_order_follow_the_same_trajectory(fix):
    """The three cylinders relabelled: a particle's sums add in index order, so the run agrees within D_q, not bit for bit."""
    sc = M.scene_of(fix)
    order = np.array([2, 0, 1])
    ps = dict(sc)
    for k in CYL_KEYS:
        ps[k] = sc[k][order].copy()
    nst = int(fix["nsteps"])
    snaps, recs = TR.run(ps, nst)
    assert [r["rebuilt"] for r in recs] == fix["rebuilt"].tolist()
    got, want = snaps[f"step{nst}"], snap(fix, f"step{nst}")
    back = np.argsort(order)
    got = dict(got, cyl_xi=got["cyl_xi"][:, back], cyl_live=got["cyl_live"][:, back], per_cylinder=got["per_cylinder"][back])
    assert np.array_equal(got["cyl_live"], want["cyl_live"])
    err, Dq = TR.deviation(got, want), dict(zip((str(s) for s in fix["quantities"]), fix["D"]))
    print("  ".join(f"{q} {err[q]:.1e} / {Dq[q]:.1e}" for q in Dq))
    assert all(err[q] <= Dq[q] for q in Dq)
