"""The unit of length on the GPU (docs/SPEC.md §4): the kernels and host table builders listed below at the scales
S = 2^-10, 1e-3 (SI grains of a millimetre) and 2^12 against the reference run AT THE SAME SCALE, at the suite's own gates:
1e-9 for wrenches, energy and virial, 1e-10 for the per-slot rows, counts and touching sets equal.  The scaling tables are
tests/units_common.py's, proven on the references by tests/test_units_refs.py.  One absolute constant in a kernel — a
tolerance, a clamp, a threshold that does not scale with R — would pass every other test of the suite, whose scenes all
have radii of about 1, and fail here.

Covered: the pair compute on one bed per launch plan (one of them also translated, one with newton off and ghost rows),
with the metamorphic check that the rows at a power of two are the rows at scale 1; the shape upload (bounding radius,
refusal of a radius that is too small, body table); the elastic and the damped / friction wall passes; pair damping,
friction, rolling and twisting on the L = 4 / n_q = 8 bed of dissipation_common; a bed of mixed orders (3, 9); ghosts, bins
and the half list of a periodic 512-particle box; the whole step (24 particles, every model but springs and moving walls,
the ledger, one rebuild) through DeviceRun.step, run_native and a 2x1x1 hub of rank threads.

Also: the two exact-root fixtures at 2^-10; the history (spring) pass of pairs on a device-built list; the ledger rows
of the pair pass and of the wall pass; the walls' spring and moving instances.  The refined largest radius is not
exported by the C ABI and is held through the refusal of a radius below it."""
import numpy as np
import pytest

import units_common as U
from common import oracle_compute, rel_err
from dissipation_common import NQ, _wall_ctx, _wall_pass, dev, gpu_forces, ctx
from test_gpu_parity import make_ctx

pytestmark = pytest.mark.gpu
TOL = 1e-9
TOL_ROWS = 1e-10


def gpu_pair(case, plan, K, E, nlocal=None, newton=True):
    import torch
    sp = make_ctx(case, plan["nq"], K, E)
    for k, v in plan["opts"].items():
        sp.set_option(k, v)
    sp.set_option("count", 1)
    npairs = case["jlist"].size
    rows = torch.zeros(npairs, 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(rows.data_ptr())
    b = case["bed"]
    f, tq, eng, vir = sp.compute(case["n"] if nlocal is None else nlocal, b["x"], b["quat"], b["type"], b["shtype"],
                                 newton_pair=newton, eflag=True, vflag=True)
    ki, st = sp.kernel_info(), sp.stats()
    rmax = [sp.rmax(k) for k in range(len(case["shapes"]))]
    sp.set_pair_output(None)
    sp.close()
    return dict(f=f, torque=tq, eng=eng, vir=vir, rows=rows.cpu().numpy(), ki=ki, rmax=rmax,
                counts=(st["n_candidates"], st["n_contact"], st["n_touching"]))


def pair_deviations(g, o, R):
    """The suite's scales, with the largest force times the length unit R beside the largest torque (at R ~ 1 the suite
    compares the two numbers as they are)."""
    fs = np.abs(o["f"]).max()
    ts = max(fs * R, np.abs(o["torque"]).max())
    return dict(f=rel_err(g["f"], o["f"], fs), torque=rel_err(g["torque"], o["torque"], ts),
                energy=abs(g["eng"] - o["eng_virial"][0]) / abs(o["eng_virial"][0]), virial=rel_err(g["vir"], o["eng_virial"][1:]),
                rows=float((np.abs(g["rows"] - o["pairs"]) / np.abs(o["pairs"]).max(axis=0)).max()))


def assert_pair(g, o, plan, label, R):
    d = pair_deviations(g, o, R)
    print(f"{label}: {int(o['counts'][2])} touching, " + " ".join(f"{k} {v:.1e}" for k, v in d.items()))
    assert {k: g["ki"][k] for k in plan["info"]} == plan["info"] and g["ki"]["lmax"] == plan["lmax"], g["ki"]
    assert o["counts"][2] >= 30
    assert max(d["f"], d["torque"], d["energy"], d["virial"]) < TOL and d["rows"] < TOL_ROWS, d
    assert g["counts"] == tuple(o["counts"]) and np.array_equal(g["rows"][:, 0] > 0, o["pairs"][:, 0] > 0)
    return d


@pytest.mark.parametrize("plan", U.PLANS, ids=[p["id"] for p in U.PLANS])
def test_pair_compute_at_every_scale(oracle, plan):
    base = U.plan_bed(plan, oracle)
    oracle.set_rule("weighted" if plan["opts"].get("rule") else "sharp")
    try:
        case, K, E = U.plan_scaled(base, plan, 1.0, oracle.shape_rmax)
        g1 = gpu_pair(case, plan, K, E)
        assert_pair(g1, oracle_compute(oracle, case, plan["nq"], K, E, eflag=True, vflag=True, want_pairs=True, nthreads=8), plan,
                    f"{plan['id']} s=1", 1.0)
        col = np.abs(g1["rows"]).max(axis=0)
        for s in U.S:
            case, K, E = U.plan_scaled(base, plan, s, oracle.shape_rmax)
            g = gpu_pair(case, plan, K, E)
            o = oracle_compute(oracle, case, plan["nq"], K, E, eflag=True, vflag=True, want_pairs=True, nthreads=8)
            assert_pair(g, o, plan, f"{plan['id']} s={s:g}", s)
            for k, r in enumerate(g["rmax"]):          # the library's own bounding radius scales with the shape
                assert abs(r - s * g1["rmax"][k]) <= 1e-15 * r
            if U.is_pow2(s):
                # the same path through every search: the rows differ from the rows at scale 1 by rounding only
                back = U.unscale_rows(g["rows"], s)
                dm = float((np.abs(back - g1["rows"]) / col).max())
                print(f"{plan['id']} s={s:g}: GPU rows / (s^3, s^2, s^3) against GPU rows at scale 1: {dm:.1e}, "
                      f"bit-identical {np.array_equal(back, g1['rows'])}")
                assert dm <= 1e-12
    finally:
        oracle.set_rule("sharp")


@pytest.mark.parametrize("s", U.S)
def test_translated_bed(oracle, s):
    """The L = 6 / n_q = 16 bed at scale s, moved by (-1024, 2048, 4096) s R: nothing may depend on where the origin is."""
    plan = U.PLANS[1]
    base = U.plan_bed(plan, oracle)
    case, K, E = U.plan_scaled(base, plan, s, oracle.shape_rmax, offset=U.OFFSET)
    assert np.abs(case["bed"]["x"]).max() > 4000 * s
    g = gpu_pair(case, plan, K, E)
    o = oracle_compute(oracle, case, plan["nq"], K, E, eflag=True, vflag=True, want_pairs=True, nthreads=8)
    assert_pair(g, o, plan, f"translated s={s:g}", s)


@pytest.mark.parametrize("s", U.S)
def test_newton_off_with_ghost_rows(oracle, s):
    plan = U.PLANS[0]
    base = dict(U.plan_bed(plan, oracle))
    nlocal = 80
    base["ilist"] = base["ilist"][:nlocal]
    base["jlist"] = base["jlist"][:base["offsets"][nlocal]]
    base["offsets"] = base["offsets"][:nlocal + 1]
    case, K, E = U.plan_scaled(base, plan, s, oracle.shape_rmax)
    g = gpu_pair(case, plan, K, E, nlocal=nlocal, newton=False)
    o = oracle_compute(oracle, case, plan["nq"], K, E, nlocal=nlocal, newton_pair=False, eflag=True, vflag=True, want_pairs=True)
    assert_pair(g, o, plan, f"newton off s={s:g}", s)
    assert not g["f"][nlocal:].any() and not g["torque"][nlocal:].any()


@pytest.mark.parametrize("s", U.S)
def test_shape_upload_at_every_scale(oracle, s):
    """The bounding radius (default), the refusal of a user radius 1e-6 relative below the largest sampled radius, and the
    body table against the oracle's mass properties of the scaled shape, at the gates of test_body_table_matches_oracle
    taken relative to the size of each quantity."""
    from shpair import ShPair, ShPairError, shapes
    lmax = 6
    a = shapes.random_shape(lmax, 1700, amp=0.2)
    sp = ShPair(0)
    sp.settings(8)
    sp.set_ntypes(1, 2)
    sp.set_shape(0, lmax, a)
    sp.set_shape(1, lmax, a * s)
    r1, rs = sp.rmax(0), sp.rmax(1)
    print(f"s={s:g}: rmax {rs:.17g} against s x {r1:.17g}: {abs(rs - s * r1) / rs:.1e}")
    assert abs(rs - s * r1) <= 1e-15 * rs
    # the refined largest radius (the "true" one of shpair_set_shape) is not exported; the sampled maximum rs / 1.01
    # (docs/SPEC.md §1) is at or below it, so a radius 1e-6 relative below the sampled maximum is more than 1e-6 below the
    # true one and must be refused: at every scale, which an absolute step or tolerance in the refinement would break
    sampled = rs / 1.01
    with pytest.raises(ShPairError) as e:
        sp.set_shape(1, lmax, a * s, sampled * (1.0 - 1e-6))
    assert e.value.code == -1
    sp.set_shape(1, lmax, a * s, rs)                      # its own default is accepted as a user radius
    assert sp.rmax(1) == rs
    rho = 0.7
    sp.set_density(1, rho)
    m, com, inertia = sp.body(1)
    mp = oracle.mass_props(lmax, a * s)
    d = dict(mass=abs(m - rho * mp[0]) / m, com=np.abs(com - mp[1:4]).max() / rs, inertia=np.abs(inertia - rho * mp[4:]).max() / np.abs(mp[4:]).max())
    print(f"s={s:g}: body table " + " ".join(f"{k} {v:.1e}" for k, v in d.items()))
    assert d["mass"] < 1e-13 and d["com"] < 1e-14 and d["inertia"] < 1e-13
    sp.close()


@pytest.mark.parametrize("s", U.S)
def test_elastic_walls_at_every_scale(oracle, s):
    import wall_ref as W
    from test_gpu_wall import run_device, check_against_ref
    sc = U.wall_scene(oracle.shape_rmax, s)
    sp = _wall_ctx([(sc["lmax"], a) for a in sc["anm"]], sc["nq"], deterministic=1)
    case = dict(x=sc["x"], quat=sc["quat"], shtype=sc["shtype"], planes=sc["planes"], n=sc["n"])
    got = run_device(sp, case, sc["kn"], sc["expo"])
    shp = [(sc["lmax"], a, sp.rmax(k)) for k, a in enumerate(sc["anm"])]
    sp.close()
    ref = W.wall_forces(shp, sc["nq"], sc["x"], sc["quat"], sc["shtype"], sc["planes"], sc["kn"], sc["expo"])
    assert ref["nbehind"] == 0 and ref["ncontacts"] >= 20
    check_against_ref(got, ref, f"walls s={s:g}")
    # the torque on its own scale: check_against_ref sets it beside the largest force, a number 1/s times as large
    assert np.abs(got[1] - ref["torque"]).max() <= TOL * max(s * np.abs(ref["f"]).max(), np.abs(ref["torque"]).max())


@pytest.mark.parametrize("s", U.S)
def test_damped_walls_with_friction_at_every_scale(oracle, s):
    """The corner case of test_gpu_friction.py (three walls, damping and friction on each) at scale s."""
    import friction_ref as F
    for offset in (None, U.OFFSET):
        c = U.corner_wall_scene(s, offset)
        _corner_walls(F, c, s, "translated" if offset is not None else "in place")


def _corner_walls(F, c, s, label):
    x, quat, tw = c["x"], c["quat"], c["twist"]
    sp = _wall_ctx([(c["lmax"], c["anm"])], c["nq"])
    sp.set_walls(c["planes"], c["kn"], c["expo"])
    sp.wall_damping(c["gamma"])
    sp.wall_friction(c["mu"], c["gt"])
    f, tq, out = _wall_pass(sp, x, quat, tw, 3)
    nc = sp.wall_stats()
    ref = F.wall_forces_friction([(c["lmax"], c["anm"], sp.rmax(0))], c["nq"], x, quat, np.zeros(1, np.int32), tw, c["planes"], c["kn"],
                                 c["expo"], c["gamma"], c["mu"], c["gt"])
    sp.close()
    scale = np.abs(ref["f"]).max()
    tscale = max(scale * s, np.abs(ref["torque"]).max())          # force x length beside torque
    d = dict(f=np.abs(f - ref["f"]).max() / scale, torque=np.abs(tq - ref["torque"]).max() / tscale,
             wall_force=np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() / scale,
             wall_energy=np.abs(out[:, 0] - ref["wall_out"][:, 0]).max() / np.abs(ref["wall_out"][:, 0]).max())
    print(f"s={s:g} {label}: contacts {nc}, capped {[c[7] for c in ref['contacts']]}, " + " ".join(f"{k} {v:.1e}" for k, v in d.items()))
    assert nc == len(ref["contacts"]) == 3 and all(c[3] > 0 for c in ref["contacts"])
    assert max(d.values()) <= TOL, d


@pytest.mark.parametrize("s", U.S)
def test_pair_dissipation_at_every_scale(oracle, s):
    """Damping and friction (the pair pass), then rolling and twisting (the pass behind it), on the L = 4 / n_q = 8 bed
    at scale s against damp_ref, friction_ref and rolling_ref at the same scale; the branch counts are the references'."""
    import torch
    import damp_ref as D
    import test_gpu_friction as TF
    import test_gpu_rolling as TR
    sc = U.dissipation_scene(oracle, s)
    case, K, E, v, L = sc["case"], sc["K"], sc["E"], sc["v"], sc["L"]
    b, n = case["bed"], case["n"]
    ref = TF.reference(oracle, case, K, E, sc["gamma"], sc["fric"], v, L)
    cond = TF.input_conditions(ref, True)
    o = oracle_compute(oracle, case, NQ, K, E, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], case["offsets"], case["jlist"])
    c = dict(case=case, K=K, E=E, v=v, L=L, o=o, pi=pi, pj=pj, tw=ref["twist"], nlocal=n, newton=True)
    rref = TR.reference(c, sc["gamma"], sc["roll"], sc["twist"])
    rcond = TR.input_conditions(rref, True, sc["roll"], sc["twist"])
    print(f"s={s:g}: inputs {cond} {rcond}")
    TF.assert_input_conditions(cond)
    TR.assert_input_conditions(rcond)
    assert cond["ncapped"] >= 5 and cond["clamped"] >= 5
    # damping + friction
    sp = ctx(case, K, E)
    f0, t0, _ = gpu_forces(sp, case, v, L)
    for (a, bb), g in sc["gamma"].items():
        sp.pair_damping(a, bb, g)
    for (a, bb), (mu, gt) in sc["fric"].items():
        sp.pair_friction(a, bb, mu, gt)
    sp.set_energy_ledger(True)
    f1, t1, tw = gpu_forces(sp, case, v, L)
    sp.ledger_fold_device(1.0)
    tot, _ = sp.energy_ledger()
    sp.close()
    P = U.pair_powers(oracle, sc).sum(axis=0)             # the ledger rows of the pass: ledger_ref on the oracle's rows
    assert P[0] > 0 and P[1] > 0
    scale = cond["scale"]
    tscale = max(scale * s, np.abs(ref["elastic_t"] + ref["torque"]).max())          # force x length beside torque
    d = dict(dF=np.abs((f1 - f0) - ref["f"]).max() / scale, dtau=np.abs((t1 - t0) - ref["torque"]).max() / tscale,
             elastic=np.abs(f0 - ref["elastic_f"]).max() / scale,
             twist=np.abs((tw - ref["twist"]) / np.abs(ref["twist"]).max(axis=0)).max())
    # rolling + twisting behind the damping pass
    sp = TR.rolling_ctx(case, K, E, gamma=sc["gamma"], roll=sc["roll"], twist=sc["twist"])
    g0, u0, g1, u1, _ = TR.gpu_pass(sp, case, v, L)
    sp.close()
    assert np.array_equal(TR.bits(g0), TR.bits(g1))
    rscale = max(np.abs(rref["f0"]).max() * s, np.abs(rref["t0"] + rref["torque"]).max())   # force x length beside torque
    d["rolling"] = np.abs((u1 - u0).cpu().numpy() - rref["torque"]).max() / rscale
    d["ledger_damping"], d["ledger_friction"] = abs(tot[0] - P[0]) / P[0], abs(tot[1] - P[1]) / P[1]
    print(f"s={s:g}: " + " ".join(f"{k} {x:.1e}" for k, x in d.items()))
    assert d["twist"] <= 1e-12
    assert max(d["dF"], d["dtau"], d["elastic"], d["rolling"], d["ledger_damping"], d["ledger_friction"]) <= TOL, d


@pytest.mark.parametrize("s", (1.0,) + U.S)
def test_mixed_orders_bed_at_every_scale(oracle, s):
    """Orders (3, 9) in one context, n_q = 16, m = 1.25: every shape at its own order, the reference's bounding radii."""
    import mixed_common as MC
    from common import coeff_tables
    base = MC.make_mixed_case(120, (3, 9), seed=612, rmax_fn=oracle.shape_rmax)
    case = dict(base)
    if s != 1.0:
        case["shapes"] = [np.asarray(a) * s for a in base["shapes"]]
        case["rmax"] = [oracle.shape_rmax(l, a) for l, a in zip(base["orders"], case["shapes"])]
        case["bed"] = dict(base["bed"], x=base["bed"]["x"] * s)
    K, E = coeff_tables(1, 1000.0, 1.25)
    K = U.scale_kn(K, E, s)
    o = MC.mixed_oracle_compute(oracle, case, 16, K, E, eflag=True, vflag=True, want_pairs=True, nthreads=8)
    MC.assert_mixed_slots(case, o["pairs"])
    import torch
    sp = MC.mixed_ctx(case, 16, K, E)
    sp.set_option("count", 1)
    rows = torch.zeros(case["jlist"].size, 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(rows.data_ptr())
    b = case["bed"]
    f, tq, eng, vir = sp.compute(case["n"], b["x"], b["quat"], b["type"], b["shtype"], eflag=True, vflag=True)
    st, ki = sp.stats(), sp.kernel_info()
    sp.set_pair_output(None)
    sp.close()
    g = dict(f=f, torque=tq, eng=eng, vir=vir, rows=rows.cpu().numpy(), ki=ki,
             counts=(st["n_candidates"], st["n_contact"], st["n_touching"]))
    assert_pair(g, o, dict(info=dict(compiled_order=1), lmax=9), f"orders (3, 9) s={s:g}", s)


@pytest.mark.parametrize("s", U.S)
def test_ghosts_bins_and_half_list_of_a_periodic_box(oracle, s):
    """512 particles in a periodic box at scale s, translated by (-1024, 2048, 4096) s R: the device's ghosts are the
    images of step_ref, its half list the tree list on its own rows, and (tests/test_units_refs.py holds the reference
    to that) the list of the box at scale 1 where it stands, slot for slot."""
    import torch
    import step_ref as SR
    from shpair import ShPair
    sc = U.list_scene(oracle.shape_rmax)
    n, t = sc["n"], U.OFFSET * sc["rmax"].max() * s
    x, lo, hi, rmax, skin = sc["x"] * s + t, sc["lo"] * s + t, sc["hi"] * s + t, sc["rmax"] * s, sc["skin"] * s
    own, code = SR.images(x, lo, hi, sc["periodic"], 2.0 * rmax.max() + skin)
    xa = np.concatenate([x, x[own] + SR.shift_of(code) * (hi - lo)])
    sha = np.concatenate([sc["shtype"], sc["shtype"][own]])
    r_offs, r_jl = SR.half_list(n, xa, sha, np.concatenate([np.arange(n), own]), rmax, skin)
    own1, code1 = SR.images(sc["x"], sc["lo"], sc["hi"], sc["periodic"], 2.0 * sc["rmax"].max() + sc["skin"])
    xa1 = np.concatenate([sc["x"], sc["x"][own1] + SR.shift_of(code1) * (sc["hi"] - sc["lo"])])
    u_offs, u_jl = SR.half_list(n, xa1, np.concatenate([sc["shtype"], sc["shtype"][own1]]), np.concatenate([np.arange(n), own1]),
                                sc["rmax"], sc["skin"])
    sp = ShPair(0)
    sp.settings(8)
    sp.set_ntypes(1, 2)
    for k, a in enumerate(sc["anm"]):
        sp.set_shape(k, sc["lmax"], a * s, float(rmax[k]))
    sp.coeff(1, 1, 1000.0, 1.25)
    sp.set_box(lo, hi, sc["periodic"], skin)
    nmax = n + 4 * own.size + 64
    pad = lambda a_, w: np.concatenate([a_, np.zeros((nmax - n,) + a_.shape[1:], a_.dtype)])
    quat = np.tile([1.0, 0, 0, 0], (n, 1))
    xd, qd = dev(pad(x, 3)), dev(pad(quat, 4))
    tyd, shd = dev(pad(np.ones(n, np.int32), 0)), dev(pad(sc["shtype"], 0))
    tagd = dev(pad(np.arange(n, dtype=np.int32), 0))
    ng = sp.borders_device(n, nmax, xd.data_ptr(), qd.data_ptr(), tyd.data_ptr(), shd.data_ptr(), tag=tagd.data_ptr())
    npairs = sp.neighbor_build_device(n, ng, xd.data_ptr(), shd.data_ptr(), tag=tagd.data_ptr())
    offs, jl = sp.copy_neighbors(n, npairs)
    torch.cuda.synchronize()
    gx, gtag = xd.cpu().numpy()[:n + ng], tagd.cpu().numpy()[:n + ng]
    sp.close()
    print(f"s={s:g}: {ng} ghosts (reference {own.size}), {npairs} slots (reference {r_jl.size})")
    assert np.array_equal(gx[:n], x)                                       # rows inside the box keep their bits
    assert ng == own.size and np.array_equal(gtag[n:], own) and np.array_equal(gx[n:], xa[n:])
    assert npairs == r_jl.size > 1000 and np.array_equal(offs, r_offs) and np.array_equal(jl, r_jl)
    assert np.array_equal(offs, u_offs) and np.array_equal(jl, u_jl)        # the unscaled list, slot for slot


# ---- the whole step: the 24-particle scene of mixed_common (every model it composes on, frozen rows, the ledger, one
# rebuild in 10 steps) at scale, against traj_ref on the scaled scene, computed here; bars 10 D_q of that scaled scene

_step_refs = {}


def _scaled_step_ref(frozen, s, offset):
    import mixed_common as MC
    key = (frozen, s, offset is not None)
    if key not in _step_refs:
        ref = U.step_reference(U.scale(MC.step_scene(frozen), s, offset), MC.STEP_NSTEPS)
        print(f"reference s={s:g}: rebuilt at {[k + 1 for k, r in enumerate(ref['rebuilt']) if r]}, smallest margin "
              f"{min(ref['margin']):.2e}; D_q " + "  ".join(f"{q} {ref['D'][q]:.1e}" for q in ("x", "v", "quat", "angmom", "ledger")))
        assert sum(ref["rebuilt"]) >= 1 and min(ref["margin"]) >= MC.STEP_MARGIN      # as the recorder asks
        assert min(ref["touching"]) >= 40 and ref["last"]["ledger"][:4].min() > 0
        _step_refs[key] = ref
    return _step_refs[key]


STEP_SCALES = [(2.0 ** -10, None), (1e-3, tuple(U.OFFSET))]


@pytest.mark.parametrize("s,offset", STEP_SCALES, ids=["2^-10", "1e-3-translated"])
def test_whole_step_through_step_and_run_native(s, offset):
    import mixed_common as MC
    import test_gpu_mixed_orders as TM
    ref = _scaled_step_ref(True, s, offset)
    sc = ref["sc"]
    sp, r = TM.device_run(sc, 1)
    got0 = TM.read_run(r)
    scale = np.abs(ref["setup"]["f"]).max()
    ef = np.abs(got0["f"] - ref["setup"]["f"]).max() / scale
    et = np.abs(got0["torque"] - ref["setup"]["torque"]).max() / max(scale * s, np.abs(ref["setup"]["torque"]).max())
    print(f"s={s:g} set-up forces: |dF| {ef:.1e}, |dtau| {et:.1e}")
    assert ef < TOL and et < TOL
    for _ in range(MC.STEP_NSTEPS):
        r.step()
    stepped = TM.read_run(r)
    sp.close()
    sp, r = TM.device_run(sc, 1)
    r.run_native(MC.STEP_NSTEPS)
    native = TM.read_run(r)
    sp.close()
    bad = TM.over_bar(stepped, ref, f"s={s:g} DeviceRun.step") + TM.over_bar(native, ref, f"s={s:g} run_native")
    assert not bad, bad
    assert stepped["builds"] == native["builds"] == int(ref["last"]["builds"])


@pytest.mark.parametrize("s,offset", STEP_SCALES, ids=["2^-10", "1e-3-translated"])
def test_whole_step_on_two_ranks(s, offset):
    import torch
    import mixed_common as MC
    import test_gpu_mixed_orders as TM
    from shpair import mrank
    ref = _scaled_step_ref(False, s, offset)
    sc = ref["sc"]
    grid, per = (2, 1, 1), tuple(int(p) for p in sc["periodic"])
    xw, owner = TM._distribute(grid, sc["lo"], sc["hi"], per, 2.0 * sc["rmax"].max() + float(sc["skin"]), sc["x"])
    hub = mrank.Hub(2)

    def body(rank):
        sp = TM.step_ctx(sc, 1)
        sp.set_option("halo_twists", 1)
        sp.set_energy_ledger(True)
        halo = mrank.Halo(sp, rank, 2, grid, sc["lo"], sc["hi"], per, float(sc["skin"]), hub=hub)
        m = owner == rank
        run = mrank.RankRun(sp, halo, xw[m], sc["quat"][m], sc["shtype"][m], sc["tag"][m], type_=sc["type"][m], v=sc["v"][m],
                            angmom=sc["angmom"][m], mask=sc["mask"][m], check_every=1, **TM.step_options(sc))
        run.run(MC.STEP_NSTEPS)
        run.sync()
        torch.cuda.synchronize()
        n = run.n
        tot, pw = sp.energy_ledger()
        out = dict(tag=run.tag[:n].cpu().numpy(), x=run.x[:n].cpu().numpy(), v=run.v[:n].cpu().numpy(), quat=run.q[:n].cpu().numpy(),
                   angmom=run.L[:n].cpu().numpy(), planes=sp.get_walls(), builds=run.builds, ledger=np.array(tot), per_wall=np.array(pw))
        halo.close()
        sp.close()
        return out
    parts = TM._run_ranks(2, body)
    hub.close()
    keys = ("x", "v", "quat", "angmom")
    got = dict(zip(keys, TM._gather(parts, len(sc["x"]), keys)))
    got.update(ledger=sum(p["ledger"] for p in parts), per_wall=sum(p["per_wall"] for p in parts), planes=parts[0]["planes"])
    assert all(len(p["tag"]) > 0 for p in parts)
    assert TM.over_bar(got, ref, f"s={s:g} 2x1x1") == []
    assert [p["builds"] for p in parts] == [int(ref["last"]["builds"])] * 2


# ---- the exact-root fixtures at 2^-10: inputs scaled, expected rows scaled analytically (exact), the gates of
# tests/test_gpu_pair_ref.py unchanged (the torque beside s x the largest force)

@pytest.mark.parametrize("m", (1.0, 1.25, 2.0))
@pytest.mark.parametrize("tag,opts", [("own", ()), ("det", (("deterministic", 1),))])
@pytest.mark.parametrize("name", ["l6_shallow", "l3_9_mixed"])
def test_exact_root_fixtures_at_two_to_the_minus_ten(name, tag, opts, m):
    import torch
    import pair_ref
    from shpair import ShPair
    from test_gpu_pair_ref import GATE, MARGIN, expect_kernel
    assert m in pair_ref.EXPONENTS
    s = 2.0 ** -10
    g, rec = U.scale_fixture(pair_ref.load_fixture(name), s), pair_ref.load_shortcut()[name]
    newton = bool(g["newton"])
    touch = g["V"] > 0
    flagged = touch & g["multi"]
    drop = flagged if m != 1.0 else np.zeros_like(flagged)
    keep = ~drop
    ilist, offsets, jlist = pair_ref.without_slots(g["nlist"], drop)
    K, E = pair_ref.kn_table(g["ntypes"], m)
    K = U.scale_kn(K, E, s)
    sp = ShPair(0)
    sp.settings(g["nq"])
    sp.set_ntypes(g["ntypes"], len(g["a_nm"]))
    for k, a in enumerate(g["a_nm"]):
        if "own_lmax" in g:
            l = int(g["own_lmax"][k])
            sp.set_shape(k, l, a[:(l + 1) * (l + 2)], float(g["rmax"][k]))
        else:
            sp.set_shape(k, g["lmax"], a)
        assert abs(sp.rmax(k) - g["rmax"][k]) < 1e-14 * s
    for a in range(1, g["ntypes"] + 1):
        for b in range(1, g["ntypes"] + 1):
            sp.coeff(a, b, K[a, b], E[a, b])
    sp.set_neighbors_csr(ilist, offsets, jlist)
    sp.set_option("force_volume", 1)
    sp.set_option("count", 1)
    for key, value in opts:
        sp.set_option(key, value)
    out = torch.zeros(max(jlist.size, 1), 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(out.data_ptr())
    nall = len(g["x"])
    f, tq = np.zeros((nall, 3)), np.zeros((nall, 3))
    _, _, eng, _ = sp.compute(g["nlocal"], g["x"], g["quat"], g["type"], g["shtype"], newton_pair=newton, eflag=True, f=f, torque=tq)
    got = out.cpu().numpy()[:jlist.size]
    ntouch = sp.stats()["n_touching"]
    kinfo = sp.kernel_info()
    sp.set_pair_output(None)
    sp.close()
    expect_kernel(name, tag, kinfo)
    f_ref, tq_ref, e_ref = pair_ref.assemble(g, g["nlist"], g["x"], g["type"], K, E, g["nlocal"], newton, skip=drop)
    fs = np.abs(f_ref).max()
    df, dt = np.abs(f - f_ref).max() / fs, np.abs(tq - tq_ref).max() / max(fs * s, np.abs(tq_ref).max())
    V, S, T = g["V"][keep], g["S"][keep], g["T"][keep]
    dS = np.abs(got[:, 1:4] - S).max() / np.abs(g["S"]).max()
    dT = np.abs(got[:, 4:7] - T).max() / np.abs(g["T"]).max()
    tv = V > 0
    dV = (np.abs(got[tv, 0] - V[tv]) / V[tv]).max()
    dE = abs(eng - e_ref) / e_ref
    print(f"{name} {tag} m={m} s=2^-10: S {dS:.2e} T {dT:.2e} V {dV:.2e} (recorded {rec['v_dev_max']:.2e}) F {df:.2e} tau {dt:.2e} "
          f"(recorded {rec['f_dev'][repr(m)]:.2e} {rec['tau_dev'][repr(m)]:.2e}) E {dE:.2e}")
    assert ntouch == tv.sum() and np.array_equal(got[:, 0] > 0, tv)
    assert dS <= GATE and dT <= GATE
    if m == 1.0:
        assert df <= GATE and dt <= GATE
    else:
        assert df <= MARGIN * rec["f_dev"][repr(m)] and dt <= MARGIN * rec["tau_dev"][repr(m)]
    cmp_v = ~g["multi"][keep] & tv
    assert (np.abs(got[cmp_v, 0] - V[cmp_v]) / V[cmp_v]).max() <= MARGIN * rec["v_dev_max"]
    if not flagged[keep].any():
        assert dE <= MARGIN * rec["v_dev_max"] * m


@pytest.mark.parametrize("s", U.S)
def test_history_springs_of_the_pair_pass(oracle, s):
    """The pair pass with tangential springs (pair_contact_device, history_kernels.hpp) on the device-built list of the
    L = 4 / n_q = 8 bed at scale s, against history_ref at the same scale: the added wrench, xi, the kind of every slot."""
    import damp_ref as D
    import history_ref as H
    import step_ref as SR
    import test_gpu_friction as TF
    import test_gpu_history as TH
    sc = U.dissipation_scene(oracle, s)
    case, K, E, v, L = dict(sc["case"]), sc["K"], sc["E"], sc["v"], sc["L"]
    b, n = case["bed"], case["n"]
    skin = 0.1 * s
    offs, jl = SR.half_list(n, b["x"], b["shtype"], np.arange(n), np.asarray(case["rmax"]), skin)
    case["ilist"], case["offsets"], case["jlist"] = np.arange(n, dtype=np.int32), offs, jl
    o = oracle_compute(oracle, case, NQ, K, E, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], offs, jl)
    tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
    xi0 = 0.01 * s * np.random.default_rng(3).normal(size=(jl.size, 3))
    a = (o["pairs"], pi, pj, b["x"], tw, b["type"], b["shtype"], case["rmax"], K, E, TH.table(sc["gamma"]), TH.table(sc["fric"], 0),
         TH.table(sc["fric"], 1))
    rf, rt, rxi, rdet = H.pair_history(*a, TH.table(sc["spring"]), xi0, TH.DT, n, newton_pair=True)
    kind = rdet["kind"]
    counts = {k: int((kind == k).sum()) for k in (H.STICK, H.SLIDE, H.RESET_UNTOUCHED, H.RESET_GUARD)}
    print(f"s={s:g}: {jl.size} slots, kinds {counts}")
    assert counts[H.STICK] >= 10 and counts[H.SLIDE] >= 10 and counts[H.RESET_UNTOUCHED] >= 10
    # the context: the library's own bounding radii would do as well; the reference's keep list and reference in step
    from shpair import ShPair
    sp = ShPair(0)
    sp.settings(NQ)
    sp.set_ntypes(2, 2)
    for k, anm in enumerate(case["shapes"]):
        sp.set_shape(k, case["lmax"], anm, float(case["rmax"][k]))
    for i in (1, 2):
        for j in (1, 2):
            sp.coeff(i, j, K[i, j], E[i, j])
    sp.set_option("deterministic", 1)
    for (p, q), g in sc["gamma"].items():
        sp.pair_damping(p, q, g)
    for (p, q), (mu, gt) in sc["fric"].items():
        sp.pair_friction(p, q, mu, gt)
    for (p, q), kt in sc["spring"].items():
        sp.set_pair_tangential_spring(p, q, kt)
    sp.set_box(b["x"].min(axis=0) - s, b["x"].max(axis=0) + s, (0, 0, 0), skin)
    bed = TH._Bed(sp, case, v, L, n, True)
    assert np.array_equal(bed.offs, offs) and np.array_equal(bed.jl, jl)
    sp.set_contact_history(n, xi0)
    df, dt_, f1, _ = bed.pass_(TH.DT)
    xi1 = sp.contact_history(n)
    sp.close()
    scale = np.abs(o["f"] + rf).max()
    tscale = max(scale * s, np.abs(o["torque"] + rt).max())
    vt = np.where(np.isnan(rdet["vt"]), 0.0, rdet["vt"])
    xscale = (np.linalg.norm(xi0, axis=1) + TH.DT * np.linalg.norm(vt, axis=1)).max()
    d = dict(dF=np.abs(df - rf).max() / scale, dtau=np.abs(dt_ - rt).max() / tscale, xi=np.abs(xi1 - rxi).max() / xscale,
             elastic=np.abs((f1 - df) - o["f"]).max() / scale)
    print(f"s={s:g}: " + " ".join(f"{k} {x:.1e}" for k, x in d.items()))
    assert np.abs(rf).max() > 0.05 * scale
    assert max(d.values()) <= TOL, d
    dead = ~np.isin(kind, (H.STICK, H.SLIDE))
    assert not xi1[dead].any()


@pytest.mark.parametrize("s", U.S)
def test_wall_springs_moving_walls_and_the_wall_ledger(oracle, s):
    """The corner scene with springs on two walls and every wall translating (wall_contact_device: the spring and moving
    instances of wall_kernels.hpp), in place and translated, against wall_history_ref at the same scale; the per-wall
    ledger rows of that pass against ledger_ref."""
    import wall_history_ref as H
    import ledger_ref as LR
    from test_gpu_wall_history import _contact_pass
    for offset in (None, U.OFFSET):
        c = U.corner_wall_scene(s, offset)
        sp = _wall_ctx([(c["lmax"], c["anm"])], c["nq"])
        sp.set_walls(c["planes"], c["kn"], c["expo"])
        sp.wall_damping(c["gamma"])
        sp.wall_friction(c["mu"], c["gt"])
        sp.set_wall_tangential_spring(c["kt"])
        sp.wall_velocity(c["vel"])
        sp.set_energy_ledger(True)
        sp.set_wall_history(1, c["xi0"][None])
        f, tq, out = _contact_pass(sp, c["x"], c["quat"], c["twist"], 3, c["dt"])
        xi = sp.wall_history(1)
        sp.ledger_fold_device(c["dt"])
        _, per = sp.energy_ledger()
        sh = [(c["lmax"], c["anm"], sp.rmax(0))]
        sp.close()
        live = c["xi0"].any(axis=1)[None, :]
        ref = H.wall_forces_history(sh, c["nq"], c["x"], c["quat"], np.zeros(1, np.int32), c["twist"], c["planes"], c["kn"], c["expo"],
                                    c["gamma"], c["mu"], c["gt"], c["kt"], c["vel"], c["xi0"][None], live, c["dt"])
        scale = np.abs(ref["f"]).max()
        d = dict(f=np.abs(f - ref["f"]).max() / scale,
                 torque=np.abs(tq - ref["torque"]).max() / max(scale * s, np.abs(ref["torque"]).max()),
                 wall_force=np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() / scale,
                 wall_energy=np.abs(out[:, 0] - ref["wall_out"][:, 0]).max() / np.abs(ref["wall_out"][:, 0]).max(),
                 xi=np.abs(xi - ref["xi"]).max() / np.abs(ref["xi"]).max())
        # the damping power and the wall work of the same pass (the friction power of a wall with a spring is the spring
        # law's, which ledger_ref's history-free wall_powers does not form: the wall without a spring is compared)
        Pw, Fw = LR.wall_powers(sh, c["nq"], c["x"], c["quat"], np.zeros(1, np.int32), c["twist"], c["planes"], c["kn"], c["expo"],
                                c["gamma"], c["mu"], c["gt"], c["vel"])
        pref = LR.wall_ledger(Pw, Fw, c["vel"], c["dt"])[0]
        d["ledger_damping"] = np.abs(per[:, 0] - pref[:, 0]).max() / np.abs(pref[:, 0]).max()
        d["ledger_friction_wall3"] = abs(per[2, 1] - pref[2, 1]) / max(np.abs(pref[:, 1]).max(), 1e-300)
        print(f"s={s:g} {'translated' if offset is not None else 'in place'}: kinds {list(ref['kind'][0])}, "
              + " ".join(f"{k} {x:.1e}" for k, x in d.items()) + f"; work GPU {per[:, 2]} ref (springless force) {pref[:, 2]}")
        assert len(set(ref["kind"][0])) >= 2
        assert max(d.values()) <= TOL, d
        assert np.array_equal(xi.any(axis=2), ref["live"])
