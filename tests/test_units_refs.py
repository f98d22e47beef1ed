"""The references are homogeneous in length (CPU): for the scenes tests/test_gpu_units.py uses, the reference at scale s
divided by the output powers of tests/units_common.py reproduces the reference at scale 1 — 1e-12 at powers of two, with
identical touching sets, lists and branch counts, and 1e-11 at s = 1e-3.  This proves the tables of units_common and
keeps the conditions of the GPU tests true by the references alone.  The oracle, wall_ref, damp_ref, friction_ref,
history_ref, rolling_ref, the tree list of step_ref and traj_ref (the whole step, which proves the rows gravity, drag,
angmom and ledger), pair_ref on slots of the two exact-root fixtures, wall_history_ref with springs and moving walls, and
the powers of ledger_ref are covered here."""
import numpy as np
import pytest

import units_common as U
from common import coeff_tables, oracle_compute
from dissipation_common import NQ


def gate(s):
    return 1e-12 if U.is_pow2(s) else 1e-11


def dev(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


@pytest.mark.parametrize("s", U.S)
@pytest.mark.parametrize("plan", U.PLANS, ids=[p["id"] for p in U.PLANS])
def test_oracle_is_homogeneous_on_the_pair_beds(oracle, plan, s):
    base = U.plan_bed(plan, oracle)
    out = {}
    oracle.set_rule("weighted" if plan["opts"].get("rule") else "sharp")
    try:
        for scale in (1.0, s):
            case, K, E = U.plan_scaled(base, plan, scale, oracle.shape_rmax)
            out[scale] = oracle_compute(oracle, case, plan["nq"], K, E, eflag=True, vflag=True, want_pairs=True, nthreads=8)
    finally:
        oracle.set_rule("sharp")
    o1, os_ = out[1.0], out[s]
    rows = U.unscale_rows(os_["pairs"], s)
    d = dict(rows=float((np.abs(rows - o1["pairs"]) / np.abs(o1["pairs"]).max(axis=0)).max()),
             f=dev(U.unscale("f", os_["f"], s), o1["f"]), torque=dev(U.unscale("torque", os_["torque"], s), o1["torque"]),
             energy=dev(U.unscale("energy", os_["eng_virial"][:1], s), o1["eng_virial"][:1]),
             virial=dev(U.unscale("virial", os_["eng_virial"][1:], s), o1["eng_virial"][1:]))
    same = np.array_equal(os_["pairs"][:, 0] > 0, o1["pairs"][:, 0] > 0)
    print(f"{plan['id']} s={s:g}: {int(o1['counts'][2])} touching, same set {same}, " + " ".join(f"{k} {v:.1e}" for k, v in d.items()))
    assert o1["counts"][2] >= 30
    assert max(d.values()) <= gate(s), d
    if U.is_pow2(s):
        assert same and np.array_equal(os_["counts"], o1["counts"])


def test_shape_radius_and_mass_properties_scale(oracle):
    from shpair import shapes
    for lmax in (4, 6, 12):
        a = shapes.random_shape(lmax, 1600 + lmax, amp=0.2)
        r1, m1 = oracle.shape_rmax(lmax, a), oracle.mass_props(lmax, a)
        for s in U.S:
            rs, ms = oracle.shape_rmax(lmax, a * s), oracle.mass_props(lmax, a * s)
            pw = np.array([3, 1, 1, 1, 5, 5, 5, 5, 5, 5])
            d = np.abs(ms / s ** pw - m1).max() / np.abs(m1).max()
            print(f"L={lmax} s={s:g}: rmax {abs(rs / s - r1) / r1:.1e} mass props {d:.1e}")
            assert abs(rs / s - r1) <= 1e-15 * r1 and d <= gate(s)


def _dissipation_refs(oracle, sc):
    import damp_ref as D
    import history_ref as H
    import test_gpu_friction as TF
    import test_gpu_rolling as TR
    import test_gpu_history as TH
    case, K, E, v, L = sc["case"], sc["K"], sc["E"], sc["v"], sc["L"]
    b, n = case["bed"], case["n"]
    fr = TF.reference(oracle, case, K, E, sc["gamma"], sc["fric"], v, L)
    o = oracle_compute(oracle, case, NQ, K, E, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], case["offsets"], case["jlist"])
    c = dict(case=case, K=K, E=E, v=v, L=L, o=o, pi=pi, pj=pj, tw=fr["twist"], nlocal=n, newton=True)
    ro = TR.reference(c, sc["gamma"], sc["roll"], sc["twist"])
    a = (o["pairs"], pi, pj, b["x"], fr["twist"], b["type"], b["shtype"], case["rmax"], K, E, TH.table(sc["gamma"]),
         TH.table(sc["fric"], 0), TH.table(sc["fric"], 1), TH.table(sc["spring"]), sc["xi"])
    hi = H.pair_history(*a, TH.DT, n, newton_pair=True)
    return dict(fric=fr, roll=ro, hist=hi)


@pytest.mark.parametrize("s", U.S)
def test_dissipation_references_are_homogeneous(oracle, s):
    """damp_ref, friction_ref, rolling_ref and history_ref on the L = 4 / n_q = 8 bed: wrenches, twists, xi, and the
    branch of every slot (clamped, capped, stick / slide / reset)."""
    r1 = _dissipation_refs(oracle, U.dissipation_scene(oracle, 1.0))
    rs = _dissipation_refs(oracle, U.dissipation_scene(oracle, s))
    f1, fs = r1["fric"], rs["fric"]
    tw = fs["twist"] / np.array([s, s, s, 1, 1, 1])
    d = dict(twist=dev(tw, f1["twist"]), f=dev(fs["f"] / s ** 4, f1["f"]), torque=dev(fs["torque"] / s ** 5, f1["torque"]),
             roll=dev(rs["roll"]["torque"] / s ** 5, r1["roll"]["torque"]),
             hist_f=dev(rs["hist"][0] / s ** 4, r1["hist"][0]), hist_t=dev(rs["hist"][1] / s ** 5, r1["hist"][1]),
             xi=dev(rs["hist"][2] / s, r1["hist"][2]))
    b1 = dict(capped=f1["det"]["capped"], clamped=f1["det"]["N"] == 0, live=r1["roll"]["det"]["live"],
              capped_r=r1["roll"]["det"]["capped_r"], capped_tw=r1["roll"]["det"]["capped_tw"], kind=r1["hist"][3]["kind"])
    bs = dict(capped=fs["det"]["capped"], clamped=fs["det"]["N"] == 0, live=rs["roll"]["det"]["live"],
              capped_r=rs["roll"]["det"]["capped_r"], capped_tw=rs["roll"]["det"]["capped_tw"], kind=rs["hist"][3]["kind"])
    same = {k: bool(np.array_equal(b1[k], bs[k])) for k in b1}
    print(f"s={s:g}: " + " ".join(f"{k} {v:.1e}" for k, v in d.items()) + f" same branches {same}")
    assert max(d.values()) <= gate(s), d
    assert all(same.values()), same           # no slot sits within rounding of a branch point: at every scale


@pytest.mark.parametrize("s", U.S)
def test_wall_reference_is_homogeneous(oracle, s):
    import wall_ref as W
    sc1 = U.wall_scene(oracle.shape_rmax, 1.0)
    scs = U.wall_scene(oracle.shape_rmax, s)
    r1 = W.wall_forces(sc1["shapes"], sc1["nq"], sc1["x"], sc1["quat"], sc1["shtype"], sc1["planes"], sc1["kn"], sc1["expo"])
    rs = W.wall_forces(scs["shapes"], scs["nq"], scs["x"], scs["quat"], scs["shtype"], scs["planes"], scs["kn"], scs["expo"])
    d = dict(f=dev(rs["f"] / s ** 4, r1["f"]), torque=dev(rs["torque"] / s ** 5, r1["torque"]),
             wall_energy=dev(rs["wall_out"][:, 0] / s ** 5, r1["wall_out"][:, 0]),
             wall_force=dev(rs["wall_out"][:, 1:] / s ** 4, r1["wall_out"][:, 1:]))
    print(f"s={s:g}: {r1['ncontacts']} contacts, " + " ".join(f"{k} {v:.1e}" for k, v in d.items()))
    assert r1["ncontacts"] >= 20 and rs["ncontacts"] == r1["ncontacts"] and rs["nbehind"] == r1["nbehind"] == 0
    assert max(d.values()) <= gate(s), d


@pytest.mark.parametrize("s", [v for v in U.S if U.is_pow2(v)])
def test_tree_list_of_a_periodic_box_is_the_same_list_at_powers_of_two(oracle, s):
    import step_ref as SR
    sc = U.list_scene(oracle.shape_rmax)
    lists = []
    for scale in (1.0, s):
        x, lo, hi, rmax, skin = sc["x"] * scale, sc["lo"] * scale, sc["hi"] * scale, sc["rmax"] * scale, sc["skin"] * scale
        cmax = 2.0 * rmax.max() + skin
        own, code = SR.images(x, lo, hi, sc["periodic"], cmax)
        xa = np.concatenate([x, x[own] + SR.shift_of(code) * (hi - lo)])
        sh = np.concatenate([sc["shtype"], sc["shtype"][own]])
        tag = np.concatenate([np.arange(sc["n"]), own])
        lists.append((own, code) + SR.half_list(sc["n"], xa, sh, tag, rmax, skin))
    print(f"s={s:g}: {lists[0][0].size} ghosts, {lists[0][3].size} slots")
    assert lists[0][3].size > 1000 and lists[0][0].size > 100
    for a, b in zip(*lists):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("s", U.S)
def test_tree_list_of_a_translated_periodic_box_at_every_scale(oracle, s):
    """The box at scale s, translated by (-1024, 2048, 4096) s R: the images and the half list are those of the box at
    scale 1 where it stands (no pair of this scene sits within rounding of its cutoff)."""
    import step_ref as SR
    sc = U.list_scene(oracle.shape_rmax)
    t = U.OFFSET * sc["rmax"].max()
    lists = []
    for scale, shift in ((1.0, 0.0 * t), (s, t * s)):
        x, lo, hi = sc["x"] * scale + shift, sc["lo"] * scale + shift, sc["hi"] * scale + shift
        rmax, skin = sc["rmax"] * scale, sc["skin"] * scale
        own, code = SR.images(x, lo, hi, sc["periodic"], 2.0 * rmax.max() + skin)
        xa = np.concatenate([x, x[own] + SR.shift_of(code) * (hi - lo)])
        sh = np.concatenate([sc["shtype"], sc["shtype"][own]])
        lists.append((own, code) + SR.half_list(sc["n"], xa, sh, np.concatenate([np.arange(sc["n"]), own]), rmax, skin))
    for a, b in zip(*lists):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("s", U.S)
def test_whole_step_reference_is_homogeneous(s):
    """traj_ref on the 24-particle scene of mixed_common (gravity, drag, pair damping, friction, rolling, twisting, a
    damped wall with friction, frozen rows, the ledger; one rebuild in 10 steps) at scale s against scale 1: the last
    state divided by the output powers, the rebuild decisions and every branch count of every step.  This is what proves
    the rows gravity, drag, angmom and ledger of the table.  The scene has no spring and no moving wall."""
    import traj_ref as TR
    import mixed_common as MC
    r1 = _step_ref(1.0)
    rs = _step_ref(s)
    back = dict(rs["last"])
    for q, p in U.STATE_POW.items():
        if q in back:
            back[q] = np.asarray(back[q]) / s ** p
    d = TR.deviation(back, r1["last"])
    print(f"s={s:g}: rebuilt {[k + 1 for k, r in enumerate(rs['rebuilt']) if r]}, smallest margin {min(rs['margin']):.2e}, "
          + " ".join(f"{q} {d[q]:.1e}" for q in ("x", "v", "quat", "angmom", "ledger"))
          + " D_q " + " ".join(f"{q} {rs['D'][q]:.1e}" for q in ("x", "v", "quat", "angmom", "ledger")))
    assert sum(r1["rebuilt"]) >= 1 and rs["rebuilt"] == r1["rebuilt"]
    assert min(rs["margin"]) >= MC.STEP_MARGIN and min(rs["touching"]) >= 40
    assert max(d[q] for q in ("x", "v", "quat", "angmom", "ledger")) <= gate(s), d
    if U.is_pow2(s):
        assert [r["counts"] for r in rs["recs"]] == [r["counts"] for r in r1["recs"]]


_step_refs = {}


def _step_ref(s):
    import mixed_common as MC
    if s not in _step_refs:
        sc = MC.step_scene(True)
        _step_refs[s] = U.step_reference(sc if s == 1.0 else U.scale(sc, s), MC.STEP_NSTEPS)
    return _step_refs[s]


@pytest.mark.parametrize("name", ["l6_shallow", "l3_9_mixed"])
def test_exact_root_reference_reproduces_the_scaled_fixture(name):
    """pair_ref (roots bisected to 4 ulp, no oracle) on the fixture's inputs times 2^-10 gives the fixture's rows times
    (s^3, s^2, s^3): on 12 touching slots and 4 that do not touch (a slot takes about a tenth of a second)."""
    import pair_ref
    s = 2.0 ** -10
    g = pair_ref.load_fixture(name)
    gs = U.scale_fixture(g, s)
    touch = np.nonzero(g["V"] > 0)[0]
    slots = np.concatenate([touch[:: max(1, touch.size // 12)][:12], np.nonzero(~(g["V"] > 0))[0][:4]])
    slots.sort()
    got = pair_ref.pair_list(gs["shape_table"], g["nq"], gs["x"], g["quat"], g["shtype"], *g["nlist"], slots=slots)
    d = dict(V=np.abs(got["V"] - gs["V"][slots]).max() / gs["V"].max(), S=np.abs(got["S"] - gs["S"][slots]).max() / np.abs(gs["S"]).max(),
             T=np.abs(got["T"] - gs["T"][slots]).max() / np.abs(gs["T"]).max())
    print(f"{name}: {slots.size} slots, " + " ".join(f"{k} {v:.1e}" for k, v in d.items()))
    assert (g["V"][slots] > 0).sum() >= 10 and np.array_equal(got["V"] > 0, g["V"][slots] > 0)
    assert np.array_equal(got["nin"], g["nin"][slots]) and np.array_equal(got["branch"], g["branch"][slots])
    assert max(d.values()) <= 1e-12, d


@pytest.mark.parametrize("s", U.S)
def test_wall_spring_and_moving_wall_reference_is_homogeneous(oracle, s):
    """wall_history_ref on the corner scene: springs on two walls, every wall translating.  Proves the rows k_t,w and wall
    velocity of the table; the kinds (stick / slide / reset) are the same at every scale."""
    import wall_history_ref as H
    out = []
    for scale in (1.0, s):
        c = U.corner_wall_scene(scale)
        sh = [(c["lmax"], c["anm"], oracle.shape_rmax(c["lmax"], c["anm"]))]
        out.append(H.wall_forces_history(sh, c["nq"], c["x"], c["quat"], np.zeros(1, np.int32), c["twist"], c["planes"], c["kn"],
                                         c["expo"], c["gamma"], c["mu"], c["gt"], c["kt"], c["vel"], c["xi0"][None],
                                         c["xi0"].any(axis=1)[None, :], c["dt"]))
    r1, rs = out
    d = dict(f=dev(rs["f"] / s ** 4, r1["f"]), torque=dev(rs["torque"] / s ** 5, r1["torque"]), xi=dev(rs["xi"] / s, r1["xi"]),
             wall_energy=dev(rs["wall_out"][:, 0] / s ** 5, r1["wall_out"][:, 0]),
             wall_force=dev(rs["wall_out"][:, 1:] / s ** 4, r1["wall_out"][:, 1:]))
    print(f"s={s:g}: kinds {list(r1['kind'][0])}, " + " ".join(f"{k} {v:.1e}" for k, v in d.items()))
    assert np.array_equal(rs["kind"], r1["kind"]) and np.array_equal(rs["live"], r1["live"])
    assert len(set(r1["kind"][0])) >= 2                     # more than one branch of the spring law
    assert max(d.values()) <= gate(s), d


@pytest.mark.parametrize("s", U.S)
def test_ledger_powers_are_homogeneous(oracle, s):
    """ledger_ref: the powers of the pair pass (damping, friction) per slot and of the corner walls scale with s^5."""
    import damp_ref as D
    import ledger_ref as LR
    import test_gpu_friction as TF
    P, W = [], []
    for scale in (1.0, s):
        sc = U.dissipation_scene(oracle, scale)
        P.append(U.pair_powers(oracle, sc))
        c = U.corner_wall_scene(scale)
        sh = [(c["lmax"], c["anm"], oracle.shape_rmax(c["lmax"], c["anm"]))]
        Pw, Fw = LR.wall_powers(sh, c["nq"], c["x"], c["quat"], np.zeros(1, np.int32), c["twist"], c["planes"], c["kn"], c["expo"],
                                c["gamma"], c["mu"], c["gt"], c["vel"])
        W.append(LR.wall_ledger(Pw, Fw, c["vel"], c["dt"])[0])
    d = dict(pair=dev(P[1] / s ** 5, P[0]), wall=dev(W[1] / s ** 5, W[0]))
    print(f"s={s:g}: " + " ".join(f"{k} {v:.1e}" for k, v in d.items()))
    assert (P[0][:, 0] > 0).sum() >= 5 and (P[0][:, 1] > 0).sum() >= 5 and np.count_nonzero(W[0]) >= 7
    assert max(d.values()) <= gate(s), d
