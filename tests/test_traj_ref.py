"""CPU tests of the whole-step reference tests/traj_ref.py (docs/SPEC.md §6, "Order of a step with every model on") and of
its recorded scene tests/golden/traj_all_on.npz: the fixture meets the conditions its recorder sets, the reference still
reproduces it, and the reference itself is held to what the suite already trusts — the oracle pipeline of
tests/test_gpu_step.py for the elastic step, and each model's own per-pass reference composed by hand."""
import os
import sys

import numpy as np
import pytest

import damp_ref as D
import friction_ref as F
import history_ref as H
import ledger_ref as LG
import rolling_ref as RL
import step_ref as SR
import traj_ref as TR
import wall_history_ref as WH
import wall_move_ref as WM
from common import coeff_tables, random_quats

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_traj_ref as M                        # noqa: E402


@pytest.fixture(scope="module")
def fix():
    return np.load(M.PATH)


def snap(fix, label):
    keys = ("x", "v", "quat", "angmom", "f", "torque", "xi", "xi_i", "xi_key", "wall_xi", "wall_live", "planes", "ledger", "per_wall",
            "builds", "step")
    return {k: fix[f"{label}_{k}"] for k in keys}


# ---- 1. the fixture --------------------------------------------------------------------------------------------------------

def test_fixture_meets_the_conditions_of_the_scene(fix):
    names = [str(s) for s in fix["count_names"]]
    cnt = {k: int(fix["counts"][:, names.index(k)].sum()) for k in TR.COUNTS}
    cnames = [str(s) for s in fix["carry_names"]]
    car = {k: int(fix["carry"][:, cnames.index(k)].sum()) for k in TR.CARRY}
    car["rebuilds"] = int(fix["rebuilt"].sum())
    car["rebuilds_with_wrap"] = int((fix["carry"][:, cnames.index("wrapped")] > 0).sum())
    print(cnt, car, "smallest margin", fix["margin"].min())
    assert M.conditions(cnt, car, list(fix["margin"])) == []
    # the stricter reading of "to ghost / to owned": a loaded spring whose j changed sides at a wrap
    assert car["owned_to_ghost"] >= 5 and car["ghost_to_owned"] >= 5
    assert len(fix["carry"]) == car["rebuilds"] == int(fix[f"step{int(fix['nsteps'])}_builds"]) - 1
    # the scene is the one the issue describes
    sc = M.scene_of(fix)
    n = len(sc["x"])
    assert 40 <= n <= 60 and sc["lmax"] == 4 and sc["nq"] == 8
    assert len(sc["a_nm"]) == 2 and sc["density"][0] != sc["density"][1] and set(sc["type"]) == {1, 2} and set(sc["shtype"]) == {0, 1}
    assert np.abs(sc["massprops"][:, 1:4]).max() > 0.05                   # a centre of mass off the SH origin
    assert sorted(sc["tag"].tolist()) == list(range(n))
    assert sc["periodic"].tolist() == [1, 1, 0] and sc["gravity"].any() and sc["gamma_t"] > 0 and sc["gamma_r"] > 0
    assert ((sc["mask"] & sc["groupbit"]) == 0).tolist() == [i % 7 == 0 for i in range(n)]
    cmax = 2 * sc["rmax"].max() + sc["skin"]
    assert ((sc["hi"] - sc["lo"])[:2] >= 2 * cmax).all()                  # §7: a periodic edge is at least 2 c_max
    # no centre behind a plane, at any snapshot
    g = (sc["mask"] & sc["groupbit"]) != 0
    for lab in fix["labels"]:
        s = snap(fix, str(lab))
        assert (s["x"][g] @ s["planes"][:, :3].T - s["planes"][:, 3] > 0).all(), lab
    assert os.path.getsize(M.PATH) <= max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                                          if f != os.path.basename(M.PATH))


def test_fixture_bars_and_wrong_variants(fix):
    q = [str(s) for s in fix["quantities"]]
    assert tuple(q) == TR.QUANTITIES and [str(v) for v in fix["variants"]] == list(TR.VARIANTS)
    Dq = dict(zip(q, fix["D"]))
    W = {str(v): dict(zip(q, row)) for v, row in zip(fix["variants"], fix["W"])}
    assert np.array_equal(fix["bar"], M.BAR_FACTOR * fix["D"]) and (fix["D"] > 0).all()
    for name, row in W.items():
        print(f"{name:26s}" + " ".join(f"{k} {row[k] / (M.BAR_FACTOR * Dq[k]):9.2e}" for k in TR.VARIANTS[name][1]), "(W / bar)")
    assert M.ratios(Dq, W) == []
    assert sorted(v[0] for v in TR.VARIANTS.values()) == [2, 3, 3, 7, 7, 8, 10, 11, 13]   # one item of the list each


def test_reference_reproduces_the_fixture(fix):
    """The recorder's reference from the fixture's inputs: the set-up and step-1 snapshots bit for bit, and the decisions,
    margins and counts of the steps ahead of the first rebuild (five at the most)."""
    sc = M.scene_of(fix)
    nst = min(5, int(np.flatnonzero(fix["rebuilt"])[0]))
    st = TR.setup(sc)
    got = {"setup": TR.snapshot(st)}
    recs = []
    for k in range(nst):
        recs.append(TR.step(sc, st))
        if k == 0:
            got["step1"] = TR.snapshot(st)
    for lab, s in got.items():
        want = snap(fix, lab)
        for k, v in s.items():
            assert np.array_equal(np.asarray(v), want[k]), (lab, k)
    assert [r["rebuilt"] for r in recs] == fix["rebuilt"][:nst].tolist()
    assert np.array_equal([r["margin"] for r in recs], fix["margin"][:nst])
    assert np.array_equal([[r["counts"][k] for k in TR.COUNTS] for r in recs], fix["counts"][:nst])


# ---- 2. every coefficient off: the oracle pipeline of tests/test_gpu_step.py -----------------------------------------------------

def _elastic_case(oracle, m=4):
    """tests/test_gpu_step.py's _periodic_case at 64 particles, with its velocities, gravity and drag."""
    from shpair import shapes
    rng = np.random.default_rng(62)
    shp = [shapes.random_shape(4, 50 + s, amp=0.2) for s in range(2)]
    lo = np.array([-1.0, 0.5, 2.0])
    box = np.array([m, m, m]) * 1.9
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    x = lo + (g + 0.5) * 1.9 + rng.uniform(-0.3, 0.3, (g.shape[0], 3))
    x[:3] -= box                                   # a few outside the box
    n = len(x)
    quat, shtype = random_quats(rng, n), rng.integers(0, 2, n).astype(np.int32)
    rng = np.random.default_rng(7)
    v, L = 0.1 * rng.normal(size=(n, 3)), 0.05 * rng.normal(size=(n, 3))
    K, E = coeff_tables(1, 1000.0, 1.25)
    return TR.scene(4, 8, shp, [1.2, 0.8], x, v, quat, L, np.ones(n, np.int32), shtype, lo, lo + box, (1, 1, 1), 0.15, 2e-3, K, E,
                    gravity=(0.0, 0.0, -1.0), gamma_t=0.05, gamma_r=0.02)


def test_elastic_step_is_the_oracle_pipeline(oracle):
    sc = _elastic_case(oracle)
    n, box = len(sc["x"]), sc["hi"] - sc["lo"]
    assert n <= 64
    st = TR.setup(sc)
    for _ in range(3):
        rec = TR.step(sc, st)
        assert not rec["rebuilt"]
    # the sequence of oracle pieces of test_device_resident_step_matches_oracle_pipeline
    mp, rho, g = sc["massprops"], sc["density"], sc["gravity"]
    xo, qo, vo, Lo = sc["x"].copy(), sc["quat"].copy(), sc["v"].copy(), sc["angmom"].copy()
    own, shift = oracle.borders(xo, sc["lo"], sc["hi"], (1, 1, 1), 2 * sc["rmax"].max() + sc["skin"])
    sha = np.concatenate([sc["shtype"], sc["shtype"][own]])
    tya = np.ones(n + own.size, dtype=np.int32)
    tag = np.concatenate([np.arange(n), own]).astype(np.int32)
    offs, jl = oracle.half_list(n, np.concatenate([xo, xo[own] + shift * box]), sha, tag, sc["rmax"], sc["skin"])
    assert jl.size > 100 and own.size > 0
    mk = np.ones(n, dtype=np.int32)

    def oforce():
        xa, qa = np.concatenate([xo, xo[own] + shift * box]), np.concatenate([qo, qo[own]])
        o = oracle.compute([(4, a, r) for a, r in zip(sc["a_nm"], sc["rmax"])], sc["K"], sc["E"], 8, n, xa, qa, tya, sha,
                           np.arange(n, dtype=np.int32), offs, jl, eflag=True)
        fo, to = o["f"][:n].copy(), o["torque"][:n].copy()
        np.add.at(fo, own, o["f"][n:])
        np.add.at(to, own, o["torque"][n:])
        oracle.post_force(mp, rho, g, 0.05, 0.02, vo, qo, Lo, sc["shtype"], mk, fo, to)
        return fo, to
    fo, to = oforce()
    for _ in range(3):
        oracle.nve(0, sc["dt"], mp, rho, xo, vo, qo, Lo, fo, to, sc["shtype"], mk)
        fo, to = oforce()
        oracle.nve(1, sc["dt"], mp, rho, xo, vo, qo, Lo, fo, to, sc["shtype"], mk)
    assert np.abs(fo).max() > 1.0
    for name, a, b in (("x", st["x"], xo), ("v", st["v"], vo), ("quat", st["quat"], qo), ("angmom", st["angmom"], Lo),
                       ("f", st["f"], fo), ("torque", st["torque"], to)):
        assert np.array_equal(a, b), name


# ---- 3. each model alone: two steps against its own per-pass reference, composed by hand ------------------------------------------

PAIR_TABLES = ("G", "MU", "GT", "KT", "MUR", "GR", "MUTW", "GTW")
WALL_ROWS = ("wall_damping", "wall_mu", "wall_gt", "wall_kt")


def only(sc, *keep, walls=False, ledger=False):
    """The all-on scene with every option off but the named tables and per-wall rows."""
    out = dict(sc)
    for k in PAIR_TABLES + WALL_ROWS:
        if k not in keep:
            out[k] = np.zeros_like(sc[k])
    if "wall_velocity" not in keep:
        out["wall_velocity"] = np.zeros_like(sc["wall_velocity"])
    if not walls:
        for k in ("planes", "wall_kn", "wall_expo", "wall_velocity") + WALL_ROWS:
            out[k] = sc[k][:0]
    out["ledger"] = int(ledger)
    return out


def hand_steps(oracle, sc, pair_pass=None, wall_pass=None, nsteps=2):
    """Two steps written out once more around ONE model's own reference: pair_pass(pairs, pi, pj, xa, twa, tya, sha, state,
    dt) -> (dF, dtau), wall_pass(x, quat, tw, planes, state, dt) -> (f, torque) over all rows; the planes advance ahead of
    the wall pass.  No rebuild (asserted by the caller through traj_ref's records)."""
    n, box, dt = len(sc["x"]), sc["hi"] - sc["lo"], sc["dt"]
    x, v, q, L = sc["x"].copy(), sc["v"].copy(), sc["quat"].copy(), sc["angmom"].copy()
    TR.wrap(x, sc["lo"], sc["hi"], sc["periodic"])
    own, code = SR.images(x, sc["lo"], sc["hi"], sc["periodic"], 2 * sc["rmax"].max() + sc["skin"])
    sha, tya = np.concatenate([sc["shtype"], sc["shtype"][own]]), np.concatenate([sc["type"], sc["type"][own]])
    offs, jl = SR.half_list(n, np.concatenate([x, x[own] + SR.shift_of(code) * box]), sha, np.concatenate([sc["tag"], sc["tag"][own]]),
                            sc["rmax"], sc["skin"])
    pi, pj = D.expand(np.arange(n), offs, jl)
    shp = [(sc["lmax"], a, r) for a, r in zip(sc["a_nm"], sc["rmax"])]
    state = dict(planes=sc["planes"].copy(), nslots=len(jl))
    g = (sc["mask"] & sc["groupbit"]) != 0

    def force(step_dt, advance):
        tw = D.twists(sc["massprops"], sc["density"], v, q, L, sc["shtype"])
        xa, qa, twa = np.concatenate([x, x[own] + SR.shift_of(code) * box]), np.concatenate([q, q[own]]), np.concatenate([tw, tw[own]])
        o = oracle.compute(shp, sc["K"], sc["E"], sc["nq"], n, xa, qa, tya, sha, np.arange(n, dtype=np.int32), offs, jl, want_pairs=True)
        f, tq = o["f"], o["torque"]
        if pair_pass:
            df, dtq = pair_pass(o["pairs"], pi, pj, xa, twa, tya, sha, state, step_dt)
            f, tq = f + df, tq + dtq
        fo, to = f[:n].copy(), tq[:n].copy()
        np.add.at(fo, own, f[n:])
        np.add.at(to, own, tq[n:])
        if wall_pass:
            if advance:
                state["planes"] = WM.advance(state["planes"], sc["wall_velocity"], dt, 1)
            wf, wt = wall_pass(x[g], q[g], tw[g], state["planes"], state, step_dt)
            fo[g] += wf
            to[g] += wt
        oracle.post_force(sc["massprops"], sc["density"], sc["gravity"], sc["gamma_t"], sc["gamma_r"], v, q, L, sc["shtype"], sc["mask"],
                          fo, to, groupbit=sc["groupbit"])
        return fo, to
    fo, to = force(0.0, False)
    for _ in range(nsteps):
        oracle.nve(0, dt, sc["massprops"], sc["density"], x, v, q, L, fo, to, sc["shtype"], sc["mask"], sc["groupbit"])
        fo, to = force(dt, True)
        state["folds"] = state.get("folds", 0) + 1
        oracle.nve(1, dt, sc["massprops"], sc["density"], x, v, q, L, fo, to, sc["shtype"], sc["mask"], sc["groupbit"])
    return dict(x=x, v=v, quat=q, angmom=L, f=fo, torque=to, state=state)


def _models(sc):
    """name -> (scene with that model alone, pair_pass, wall_pass, what of the state to compare)."""
    shp = [(sc["lmax"], a, r) for a, r in zip(sc["a_nm"], sc["rmax"])]
    n = len(sc["x"])

    def damping(s):
        return lambda p, pi, pj, xa, twa, tya, sha, st, dt: D.pair_damping(p, pi, pj, xa, twa, tya, s["K"], s["E"], s["G"], n)

    def friction(s):
        return lambda p, pi, pj, xa, twa, tya, sha, st, dt: F.pair_friction(p, pi, pj, xa, twa, tya, sha, s["rmax"], s["K"], s["E"],
                                                                              s["G"], s["MU"], s["GT"], n)[:2]

    def ledger(s):
        def run(p, pi, pj, xa, twa, tya, sha, st, dt):
            if dt:
                st["ledger"] = st.get("ledger", 0.0) + dt * LG.pair_powers(p, pi, pj, xa, twa, tya, sha, s["rmax"], s["K"], s["E"], s["G"],
                                                                         s["MU"], s["GT"], n).sum(axis=0)
            return friction(s)(p, pi, pj, xa, twa, tya, sha, st, dt)
        return run

    def springs(s):
        def run(p, pi, pj, xa, twa, tya, sha, st, dt):
            xi = st.get("xi", np.zeros((len(pi), 3)))
            df, dtq, st["xi"], _ = H.pair_history(p, pi, pj, xa, twa, tya, sha, s["rmax"], s["K"], s["E"], s["G"], s["MU"], s["GT"], s["KT"],
                                                  xi, dt, n)
            return df, dtq
        return run

    def rolling(s):
        return lambda p, pi, pj, xa, twa, tya, sha, st, dt: (np.zeros((len(xa), 3)),
                                                               RL.pair_rolling(p, pi, pj, xa, twa, tya, s["K"], s["E"], s["G"], s["MUR"],
                                                                               s["GR"], s["MUTW"], s["GTW"], n)[0])

    def moving_wall(s):
        def run(x, q, tw, planes, st, dt):
            r = WM.wall_forces_moving(shp, s["nq"], x, q, s["shtype"][(s["mask"] & s["groupbit"]) != 0], tw, planes, s["wall_kn"],
                                      s["wall_expo"], s["wall_damping"], s["wall_mu"], s["wall_gt"], s["wall_velocity"])
            return r["f"], r["torque"]
        return run

    def wall_springs(s):
        def run(x, q, tw, planes, st, dt):
            ng, nw = len(x), len(planes)
            xi, live = st.get("wall_xi", np.zeros((ng, nw, 3))), st.get("wall_live", np.zeros((ng, nw), bool))
            r = WH.wall_forces_history(shp, s["nq"], x, q, s["shtype"][(s["mask"] & s["groupbit"]) != 0], tw, planes, s["wall_kn"],
                                       s["wall_expo"], s["wall_damping"], s["wall_mu"], s["wall_gt"], s["wall_kt"], s["wall_velocity"],
                                       xi, live, dt)
            st["wall_xi"], st["wall_live"] = r["xi"], r["live"]
            return r["f"], r["torque"]
        return run

    wall = ("wall_damping", "wall_mu", "wall_gt", "wall_velocity")
    out = {}
    for name, s, make in (("damping", only(sc, "G"), damping),
                          ("friction", only(sc, "G", "MU", "GT"), friction),
                          ("ledger", only(sc, "G", "MU", "GT", ledger=True), ledger),
                          ("pair_springs", only(sc, "G", "MU", "GT", "KT"), springs),
                          ("rolling", only(sc, "MUR", "GR", "MUTW", "GTW"), rolling)):
        out[name] = (s, make(s), None)
    for name, s, make in (("moving_walls", only(sc, *wall, walls=True), moving_wall),
                          ("wall_springs", only(sc, *wall, "wall_kt", walls=True), wall_springs)):
        out[name] = (s, None, make(s))
    return out


MODELS = ("damping", "friction", "ledger", "pair_springs", "rolling", "moving_walls", "wall_springs")
TOL = 1e-13      # the same formulas in another association here and there (f -= delta S against f += (-delta S)): a few ulp


@pytest.mark.parametrize("model", MODELS)
def test_one_model_alone_is_its_own_reference_composed_by_hand(oracle, fix, model):
    sc, pair_pass, wall_pass = _models(M.scene_of(fix))[model]
    st = TR.setup(sc)
    for _ in range(2):
        assert not TR.step(sc, st)["rebuilt"]
    hand = hand_steps(oracle, sc, pair_pass, wall_pass)
    for k in ("x", "v", "quat", "angmom", "f", "torque"):
        err = np.abs(st[k] - hand[k]).max() / np.abs(hand[k]).max()
        assert err <= TOL, (model, k, err)
    hs = hand["state"]
    if model == "pair_springs":
        assert np.abs(st["xi"]).max() > 0 and np.abs(st["xi"] - hs["xi"]).max() <= TOL * np.abs(hs["xi"]).max()
    if model == "wall_springs":
        g = (sc["mask"] & sc["groupbit"]) != 0
        assert hs["wall_live"].any() and np.array_equal(st["wall_live"][g], hs["wall_live"]) and not st["wall_live"][~g].any()
        assert np.abs(st["wall_xi"][g] - hs["wall_xi"]).max() <= TOL * np.abs(hs["wall_xi"]).max()
    if model in ("moving_walls", "wall_springs"):
        assert np.array_equal(st["planes"], hs["planes"]) and not np.array_equal(st["planes"], sc["planes"])
    if model == "ledger":
        assert hs["ledger"].min() > 0 and np.abs(st["ledger"][:2] - hs["ledger"]).max() <= TOL * hs["ledger"].sum()
        assert not st["ledger"][2:].any()
    else:
        assert not st["ledger"].any()


# ---- 4. tags ----------------------------------------------------------------------------------------------------------------

def test_rows_permuted_under_their_tags_follow_the_same_trajectory(fix):
    """The scene's rows in another order with the old row index as the tag: the same pairs with the same integrated
    particle, so the same trajectory row for row, up to the order of the sums; pair xi is found under the same keys."""
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
    sa, sb = TR.snapshot(a), TR.snapshot(b)
    ka = TR.xi_by_key(sa["xi_i"], sa["xi_key"], sa["xi"])
    kb = TR.xi_by_key(perm[sb["xi_i"]], sb["xi_key"], sb["xi"])
    assert len(ka) > 20 and set(ka) == set(kb)
    scale = max(np.abs(v).max() for v in ka.values())
    assert max(np.abs(ka[k] - kb[k]).max() for k in ka) <= 1e-10 * scale
