"""GPU tests of contexts that mix shapes of different orders (docs/SPEC.md §1).  The library widens every shape to the
largest order present when it uploads its tables (csrc/shpair_tables.cpp: upload_tables), and sizes the launch plan, the
rotation buffer and the cos/sin table by that order; the references (the oracle, tests/wall_ref.py, tests/damp_ref.py)
evaluate each shape at its own order and never pad.  Every comparison hands the same explicit bounding radius to both
sides, and every bed has at least 30 touching slots with a low-order i on a high-order j and 30 the other way round,
counted from the oracle's result (tests/mixed_common.py; the beds themselves: tests/test_mixed_refs.py)."""
import functools

import numpy as np
import pytest

import traj_ref as TR
from common import coeff_tables, rel_err
from mixed_common import (bed_case, mixed_ctx, mixed_oracle_compute, assert_mixed_slots, own_tuples,
                          soup_case, soup_branches, MIN_BRANCH_PAIRS, wall_case, WALL_NQ, make_mixed_case, slot_classes,
                          MIN_MIXED_SLOTS, step_reference, assert_step_conditions, STEP_NSTEPS)
from mrank_common import _distribute, _gather, _run_ranks
from test_gpu_traj import pair_options

pytestmark = pytest.mark.gpu
TOL = 1e-9          # docs/SPEC.md §4
SLOT_TOL = 1e-10    # per-slot V, S_n, T_n against the column maximum, as tests/test_gpu_weighted.py

_ORACLE = {}        # (bed, exponent key, weighted) -> the oracle's result: computed once, shared, never written to


def two_type_tables():
    return coeff_tables(2, kn=lambda i, j: 300.0 * (i + j), expo=lambda i, j: 1.25 + 0.25 * abs(i - j))


def tables(case, expo):
    return two_type_tables() if case["ntypes"] == 2 else coeff_tables(1, 1000.0, expo)


def reference(oracle, name, expo, weighted=False):
    key = (name, expo, weighted)
    if key not in _ORACLE:
        case, nq = bed_case(name, oracle.shape_rmax)
        K, E = tables(case, expo)
        oracle.set_rule("weighted" if weighted else "sharp")
        try:
            o = mixed_oracle_compute(oracle, case, nq, K, E, eflag=True, vflag=True, want_pairs=True, nthreads=8)
        finally:
            oracle.set_rule("sharp")
        cls = assert_mixed_slots(case, o["pairs"])
        for v in o.values():
            v.setflags(write=False)
        _ORACLE[key] = (case, nq, K, E, o, cls)
    return _ORACLE[key]


def check(f, tq, o):
    """As tests/test_gpu_parity.py::check; returns the two figures."""
    fs = np.abs(o["f"]).max()
    ts = max(fs, np.abs(o["torque"]).max())
    assert fs > 0
    ef, et = rel_err(f, o["f"], fs), rel_err(tq, o["torque"], ts)
    assert ef < TOL and et < TOL, (ef, et)
    return ef, et


def check_all(label, f, tq, eng, vir, st, pr, o, tol=TOL):
    ef, et = check(f, tq, o)
    ee = abs(eng - o["eng_virial"][0]) / abs(o["eng_virial"][0])
    ev = np.abs(vir - o["eng_virial"][1:]).max() / np.abs(o["eng_virial"][1:]).max()
    ep = (np.abs(pr - o["pairs"]) / np.abs(o["pairs"]).max(axis=0)).max()
    print(f"{label}: rel err f {ef:.1e} torque {et:.1e} energy {ee:.1e} virial {ev:.1e} per-slot {ep:.1e}")
    assert ee < tol and ev < tol and ep < SLOT_TOL
    assert (st["n_candidates"], st["n_contact"], st["n_touching"]) == tuple(o["counts"])
    assert np.array_equal(pr[:, 0] > 0, o["pairs"][:, 0] > 0)


SPEC6 = dict(compiled_order=1, family=1, waves_per_pair=1, specialised=1)
# id: bed, options, exponent, what kernel_info must report (lmax is always the largest order)
ROWS = {
    "o0_6-own": ("o0_6", {}, 1.25, SPEC6),
    "o0_6-own-m1": ("o0_6", {}, 1.0, SPEC6),
    "o0_6-spec0": ("o0_6", {"spec": 0}, 1.25, dict(compiled_order=1, family=1, waves_per_pair=1, specialised=0)),
    "o0_6-spec0-m1": ("o0_6", {"spec": 0}, 1.0, dict(compiled_order=1, family=1, waves_per_pair=1, specialised=0)),
    "o0_6-jpoly0": ("o0_6", {"jpoly": 0}, 1.25, dict(compiled_order=1, family=0, waves_per_pair=1, specialised=0)),
    "o0_6-jpoly0-m1": ("o0_6", {"jpoly": 0}, 1.0, dict(compiled_order=1, family=0, waves_per_pair=1, specialised=0)),
    "o4_6_2-own": ("o4_6_2", {}, 1.25, SPEC6),
    "o4_6_2-own-m1": ("o4_6_2", {}, 1.0, SPEC6),
    "o4_6_2-det": ("o4_6_2", {"deterministic": 1}, 1.25, SPEC6),
    "o4_6_2-det-m1": ("o4_6_2", {"deterministic": 1}, 1.0, SPEC6),
    "o0_4-own": ("o0_4", {}, 1.25, dict(compiled_order=1, family=1, waves_per_pair=1, specialised=1)),
    "o3_12_q32-own": ("o3_12_q32", {}, 1.25, dict(compiled_order=1, family=1, waves_per_pair=2, specialised=1)),
    "o3_12_q20-split": ("o3_12_q20", {"jpoly": 1, "split": 1}, 1.25, dict(compiled_order=1, family=1, waves_per_pair=2, specialised=0)),
    "o5_9-jpoly0-two-types": ("o5_9", {"jpoly": 0}, None, dict(compiled_order=1, family=0, waves_per_pair=1, specialised=0)),
    "o5_9-jpoly1-two-types": ("o5_9", {"jpoly": 1}, None, dict(compiled_order=1, family=1, waves_per_pair=1, specialised=0)),
    "o3_6-variant1": ("o3_6", {"variant": 1}, 1.25, dict(compiled_order=0, family=0, specialised=0)),
    "o12_13-own": ("o12_13", {}, 1.25, dict(compiled_order=0, family=0, specialised=0)),
    "o0_20-own": ("o0_20", {}, 1.25, dict(compiled_order=0, family=0, specialised=0)),   # TOL as test_extreme_quadrature_orders (20, 24)
    "o2_6-weighted": ("o2_6", {"rule": 1}, 1.25, dict(compiled_order=1, family=0, weighted=1, specialised=0)),
    "o4_6-ring-rows5": ("o4_6", {"ring_rows": 5}, 1.25, dict(compiled_order=1, family=1, waves_per_pair=1, ring_rows=5, specialised=0)),
}


@pytest.mark.parametrize("row", list(ROWS))
def test_bed_matches_oracle_under_every_launch_plan(oracle, row):
    """One case per launch plan the largest order can select: forces, torques, energy, virial and the counts at SPEC §4's
    1e-9, the per-slot integrals at 1e-10 of the column maximum, and the plan the library reports.  A first compute asks
    for forces only (with exponent 1 that is the instance without the volume path), a second for energy and virial."""
    import torch
    name, opts, expo, plan = ROWS[row]
    case, nq, K, E, o, cls = reference(oracle, name, expo, weighted=bool(opts.get("rule")))
    b, n = case["bed"], case["n"]
    sp = mixed_ctx(case, nq, K, E)
    for k, v in opts.items():
        sp.set_option(k, v)
    sp.set_option("count", 1)
    pairs = torch.zeros(case["jlist"].size, 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(pairs.data_ptr())
    f0, t0, _, _ = sp.compute(n, b["x"], b["quat"], b["type"], b["shtype"])
    check(f0, t0, o)
    ki0 = sp.kernel_info()
    pairs.zero_()
    f, tq, eng, vir = sp.compute(n, b["x"], b["quat"], b["type"], b["shtype"], eflag=True, vflag=True)
    ki = sp.kernel_info()
    st = sp.stats()
    pr = pairs.cpu().numpy()
    sp.set_pair_output(None)
    for s in range(len(case["shapes"])):
        assert sp.rmax(s) == case["rmax"][s]
    sp.close()
    print(f"{row}: orders {case['orders']} n_q {nq}, touching slots {cls}, plan {ki}")
    check_all(row, f, tq, eng, vir, st, pr, o)
    for k in (ki0, ki):
        assert k["lmax"] == case["lmax"] and (k["scratch_bytes"] == 0 or not plan["compiled_order"])
        assert {key: k[key] for key in plan} == plan, k


def test_newton_off_with_ghost_rows_behind_the_owned_rows(oracle):
    """Orders (0, 4), the rows behind nlocal are ghosts and own no list row, as test_newton_off_with_ghosts builds them."""
    import torch
    case, nq = bed_case("o0_4", oracle.shape_rmax)
    K, E = coeff_tables(1, 1000.0, 1.25)
    n, nlocal = case["n"], 130
    sub = dict(case)
    sub["ilist"] = case["ilist"][:nlocal]
    sub["offsets"] = case["offsets"][:nlocal + 1]
    sub["jlist"] = case["jlist"][:case["offsets"][nlocal]]
    sp = mixed_ctx(sub, nq, K, E)
    pairs = torch.zeros(sub["jlist"].size, 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(pairs.data_ptr())
    b = case["bed"]
    for newton in (True, False):
        o = mixed_oracle_compute(oracle, sub, nq, K, E, nlocal=nlocal, newton_pair=newton, eflag=True, vflag=True, want_pairs=True)
        cls = assert_mixed_slots(sub, o["pairs"])
        f, tq = np.zeros((n, 3)), np.zeros((n, 3))
        pairs.zero_()
        _, _, eng, vir = sp.compute(nlocal, b["x"], b["quat"], b["type"], b["shtype"], newton_pair=newton, eflag=True, vflag=True,
                                    f=f, torque=tq)
        ef, et = check(f, tq, o)
        print(f"newton {newton}: touching slots {cls}, rel err f {ef:.1e} torque {et:.1e}")
        assert abs(eng - o["eng_virial"][0]) < TOL * abs(o["eng_virial"][0])
        assert np.abs(vir - o["eng_virial"][1:]).max() < TOL * np.abs(o["eng_virial"][1:]).max()
        assert (np.abs(pairs.cpu().numpy() - o["pairs"]) / np.abs(o["pairs"]).max(axis=0)).max() < SLOT_TOL
        if not newton:
            assert not f[nlocal:].any() and not tq[nlocal:].any()
    assert sp.kernel_info()["lmax"] == 4
    sp.set_pair_output(None)
    sp.close()


def test_peratom_energy_and_virial_of_three_orders(oracle):
    """Orders (4, 6, 2): Pair::eatom / vatom as test_peratom_energy_and_virial checks them, host form."""
    case, nq = bed_case("o4_6_2", oracle.shape_rmax)
    K, E = coeff_tables(1, 1000.0, 1.25)
    o = mixed_oracle_compute(oracle, case, nq, K, E, eflag=True, vflag=True, want_pairs=True, want_peratom=True)
    assert_mixed_slots(case, o["pairs"])
    es, vs = o["eatom"].max(), np.abs(o["vatom"]).max()
    sp = mixed_ctx(case, nq, K, E)
    b, n = case["bed"], case["n"]
    ea, va = np.zeros(n), np.zeros((n, 6))
    sp.set_peratom_host(ea, va)
    f, tq, eng, vir = sp.compute(n, b["x"], b["quat"], b["type"], b["shtype"], eflag=True, vflag=True)
    check(f, tq, o)
    print(f"per-atom: rel err energy {np.abs(ea - o['eatom']).max() / es:.1e} virial {np.abs(va - o['vatom']).max() / vs:.1e}")
    assert np.abs(ea - o["eatom"]).max() < TOL * es and np.abs(va - o["vatom"]).max() < TOL * vs
    assert abs(ea.sum() - eng) < 1e-12 * eng and np.abs(va.sum(0) - vir).max() < 1e-11 * np.abs(vir).max()
    sp.set_peratom_host(None, None)
    sp.close()


def test_weighted_rule_refuses_a_context_whose_largest_order_is_13(oracle):
    from shpair.capi import ShPairError
    case = make_mixed_case(40, (4, 13), seed=72, rmax_fn=oracle.shape_rmax)
    K, E = coeff_tables(1, 900.0, 1.0)
    sp = mixed_ctx(case, 8, K, E)
    sp.set_option("rule", 1)
    b = case["bed"]
    with pytest.raises(ShPairError) as e:
        sp.compute(40, b["x"], b["quat"], b["type"], b["shtype"])
    assert e.value.code == -6
    sp.set_option("rule", 0)                           # the sharp rule runs the same context
    f, tq, _, _ = sp.compute(40, b["x"], b["quat"], b["type"], b["shtype"])
    check(f, tq, mixed_oracle_compute(oracle, case, 8, K, E))
    sp.close()


@pytest.mark.parametrize("nq,jpoly", [(9, 0), (9, 1), (16, 0), (16, 1)])
def test_pair_soup_through_every_cap_branch(oracle, nq, jpoly):
    """Isolated pairs of the orders (1, 5, 9): at least 20 touching pairs in each of the three cap branches of SPEC §2.2
    with the lower order as i and 20 with the lower order as j, counted from the oracle; per-pair integrals, forces and
    energy against the oracle, both kernel families."""
    import torch
    soup = soup_case(oracle.shape_rmax)
    npair = soup["npair"]
    x, q, ty, sh = soup["x"], soup["quat"], soup["type"], soup["shtype"]
    K, E = coeff_tables(1, 1000.0, 1.25)
    key = ("soup", nq)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.compute(own_tuples(soup), K, E, nq, 2 * npair, x, q, ty, sh, soup["ilist"], soup["offsets"],
                                      soup["jlist"], eflag=True, want_pairs=True, nthreads=8)
    o = _ORACLE[key]
    br = soup_branches(soup, o["pairs"])
    assert br.min() >= MIN_BRANCH_PAIRS, br
    bed_like = dict(soup, bed=dict(x=x, quat=q, type=ty, shtype=sh))
    sp = mixed_ctx(bed_like, nq, K, E)
    sp.set_option("jpoly", jpoly)
    out = torch.zeros(npair, 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(out.data_ptr())
    f, tq, eng, _ = sp.compute(2 * npair, x, q, ty, sh, eflag=True)
    ki = sp.kernel_info()
    got = out.cpu().numpy()
    sp.set_pair_output(None)
    sp.close()
    assert ki["family"] == jpoly and ki["lmax"] == 9
    ep = (np.abs(got - o["pairs"]) / np.abs(o["pairs"]).max(axis=0)).max()
    ef, et = check(f, tq, o)
    print(f"soup n_q {nq} family {jpoly}: touching pairs by branch and orientation {br.tolist()}, rel err per pair {ep:.1e} "
          f"f {ef:.1e} torque {et:.1e}")
    assert ep < SLOT_TOL and np.array_equal(got[:, 0] > 0, o["pairs"][:, 0] > 0)
    assert abs(eng - o["eng_virial"][0]) < TOL * o["eng_virial"][0]


def test_padding_by_the_caller_makes_no_difference(oracle):
    """Context A gets the shapes at their own orders, context B zero-padded to the largest by the caller; the same explicit
    radii, list and deterministic mode.  Both must select the same kernel and agree within 1e-9; the measured difference is
    printed (docs/DESIGN.md records it) and not asserted to be zero."""
    import torch
    case, nq, K, E, o, cls = reference(oracle, "o4_6_2", 1.25)
    b, n = case["bed"], case["n"]
    res = []
    for padded in (False, True):
        sp = mixed_ctx(case, nq, K, E, padded=padded)
        sp.set_option("deterministic", 1)
        pairs = torch.zeros(case["jlist"].size, 7, dtype=torch.float64, device="cuda:0")
        sp.set_pair_output(pairs.data_ptr())
        f, tq, eng, _ = sp.compute(n, b["x"], b["quat"], b["type"], b["shtype"], eflag=True)
        res.append((f, tq, eng, pairs.cpu().numpy(), sp.kernel_info()))
        sp.set_pair_output(None)
        sp.close()
    A, B = res
    assert A[4] == B[4], (A[4], B[4])
    fs = np.abs(o["f"]).max()
    d = dict(f=np.abs(A[0] - B[0]).max() / fs, torque=np.abs(A[1] - B[1]).max() / max(fs, np.abs(o["torque"]).max()),
             energy=abs(A[2] - B[2]) / abs(o["eng_virial"][0]), slots=(np.abs(A[3] - B[3]) / np.abs(o["pairs"]).max(axis=0)).max())
    bitwise = all(np.array_equal(a, c) for a, c in zip(A[:4], B[:4]))
    print(f"own order against padded by the caller: {({k: float(v) for k, v in d.items()})}, bitwise equal: {bitwise}")
    assert max(d.values()) < TOL
    check(A[0], A[1], o)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("device_list", [False, True], ids=["csr-list", "device-built-list-det"])
def test_an_order_changes_between_computes_list_kept(oracle, device_list):
    """Orders (4, 4) at n_q = 8, then shape 1 becomes order 8, 2, 13 (the run-time-order kernel), then n_q = 16, the list
    installed once at the start: shpair_prepare_tables re-sizes the rotation buffer, swaps every table and may change the
    kernel family under the installed list.  After each step the forces are the oracle's and kernel_info() is that of a
    fresh context given the same tables.  Shape 1 keeps one explicit bounding radius (the largest over its orders), so
    the list stays valid."""
    import torch
    from shpair import ShPair, shapes, bed
    n, nq0 = 200, 8
    a0 = shapes.random_shape(4, 9001, amp=0.1)
    versions = {l: shapes.random_shape(l, 9100 + l, amp=0.1) for l in (4, 8, 2, 13)}
    r0 = oracle.shape_rmax(4, a0)
    r1 = max(oracle.shape_rmax(l, a) for l, a in versions.items())
    rmax = [r0, r1]
    b = bed.make_bed(n, rmax, 2, spacing=1.9, seed=bed.SEED0 + 95)
    skin = 0.1
    K, E = coeff_tables(1, 1000.0, 1.25)

    def configure(sp, l1, nq):
        sp.settings(nq)
        sp.set_ntypes(1, 2)
        sp.set_shape(0, 4, a0, r0)
        sp.set_shape(1, l1, versions[l1], r1)
        sp.coeff(1, 1, 1000.0, 1.25)
        if device_list:
            sp.set_option("deterministic", 1)

    sp = ShPair(0)
    configure(sp, 4, nq0)
    x, q, ty, sh = _dev(b["x"]), _dev(b["quat"]), _dev(b["type"]), _dev(b["shtype"])
    if device_list:
        lo, hi = b["x"].min(axis=0) - 2.0, b["x"].max(axis=0) + 2.0
        sp.set_box(lo, hi, (0, 0, 0), skin)
        npairs = sp.neighbor_build_device(n, 0, x.data_ptr(), sh.data_ptr())
        of, jl = sp.copy_neighbors(n, npairs)
        il = np.arange(n, dtype=np.int32)
    else:
        il, of, jl = bed.half_neighbor_list(b["x"], b["shtype"], rmax, skin=skin)
        sp.set_neighbors_csr(il, of, jl)

    def run(ctx):
        f = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
        tq = torch.zeros_like(f)
        ev = torch.zeros(7, dtype=torch.float64, device="cuda:0")
        ctx.compute_device(n, 0, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f.data_ptr(), tq.data_ptr(),
                           eflag=True, ev=ev.data_ptr())
        torch.cuda.synchronize()
        ctx.synchronize()
        return f.cpu().numpy(), tq.cpu().numpy(), ev.cpu().numpy()

    steps = [(4, nq0), (8, nq0), (2, nq0), (13, nq0), (13, 16)]
    for k, (l1, nq) in enumerate(steps):
        if k and steps[k - 1][0] != l1:
            sp.set_shape(1, l1, versions[l1], r1)
        if k and steps[k - 1][1] != nq:
            sp.settings(nq)
        f, tq, ev = run(sp)
        ki = sp.kernel_info()
        shp = [(4, a0, r0), (l1, versions[l1], r1)]
        o = oracle.compute(shp, K, E, nq, n, b["x"], b["quat"], b["type"], b["shtype"], il, of, jl, eflag=True, want_pairs=True,
                           nthreads=8)
        if l1 != 4:               # the first step has one order: nothing to count
            cls = slot_classes((4, l1), b["shtype"], il, of, jl, o["pairs"][:, 0] > 0)
            assert cls["low-high"] >= MIN_MIXED_SLOTS and cls["high-low"] >= MIN_MIXED_SLOTS, cls
        ef, et = check(f, tq, o)
        ee = abs(ev[0] - o["eng_virial"][0]) / abs(o["eng_virial"][0])
        print(f"step {k}: orders (4, {l1}) n_q {nq}: rel err f {ef:.1e} torque {et:.1e} energy {ee:.1e}, plan {ki}")
        assert ee < TOL and ki["lmax"] == max(4, l1)
        fresh = ShPair(0)
        configure(fresh, l1, nq)
        fresh.set_neighbors_csr(il, of, jl)
        f2, t2, _ = run(fresh)
        assert fresh.kernel_info() == ki, (fresh.kernel_info(), ki)
        fresh.close()
        fs = np.abs(o["f"]).max()
        assert np.abs(f2 - f).max() < 1e-12 * fs and np.abs(t2 - tq).max() < 1e-12 * fs
    sp.close()


def test_body_table_of_mixed_orders(oracle):
    """Orders (0, 3, 8) in one context: the body table (csrc/shstep_api.hip: mass_props at the shape's own order) against
    the oracle at the own order, with the tolerances of tests/test_gpu_step.py::test_body_table_matches_oracle."""
    from shpair import ShPair, shapes
    orders, rho = (0, 3, 8), (2.0, 0.7, 1.3)
    shp = [shapes.random_shape(l, 31 + l, amp=0.3) for l in orders]
    sp = ShPair(0)
    sp.settings(8)
    sp.set_ntypes(1, 3)
    for s, (l, a) in enumerate(zip(orders, shp)):
        sp.set_shape(s, l, a, oracle.shape_rmax(l, a))
        sp.set_density(s, rho[s])
    sp.coeff(1, 1, 1000.0, 1.25)
    for s, (l, a) in enumerate(zip(orders, shp)):
        mp = oracle.mass_props(l, a)
        m, com, inertia = sp.body(s)
        assert abs(m - rho[s] * mp[0]) < 1e-13 * m
        assert np.abs(com - mp[1:4]).max() < 1e-14
        assert np.abs(inertia - rho[s] * mp[4:]).max() < 1e-13
    sp.close()


def _wall_run(sp, c, damped, tw=None):
    import torch
    n = c["n"]
    x, q, sh, m = _dev(c["x"]), _dev(c["quat"]), _dev(c["shtype"]), _dev(np.ones(n, dtype=np.int32))
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    out = torch.zeros(len(c["planes"]), 4, dtype=torch.float64, device="cuda:0")
    if damped:
        twd = _dev(tw)
        sp.wall_force_damped_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                    twd.data_ptr(), wall_out=out.data_ptr())
    else:
        sp.wall_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(),
                             wall_out=out.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy(), sp.wall_stats()


def test_walls_with_three_orders(oracle):
    """Orders (0, 4, 6), 200 particles, three planes: wall_force_device against tests/wall_ref.py and
    wall_force_damped_device against tests/damp_ref.py, both with own-order tuples, at the gate of tests/test_gpu_wall.py
    (1e-9 of the largest force); at least 15 particles of each shape touch a wall."""
    import damp_ref as D
    import wall_ref as W
    GATE = 1e-9
    c = wall_case(oracle.shape_rmax)
    shapes_ref = own_tuples(c)
    ref = W.wall_forces(shapes_ref, WALL_NQ, c["x"], c["quat"], c["shtype"], c["planes"], c["kn"], c["expo"])
    per_shape = np.bincount(c["shtype"][np.abs(ref["f"]).max(axis=1) > 0], minlength=3)
    assert ref["nbehind"] == 0 and per_shape.min() >= 15, per_shape
    sp = mixed_ctx(c, WALL_NQ, *coeff_tables(1, 1000.0, 1.25), neighbors=False)      # asserts the radii are kept
    sp.set_option("deterministic", 1)
    sp.set_walls(c["planes"], c["kn"], c["expo"])
    f, tq, out, nc = _wall_run(sp, c, damped=False)
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ef, et = np.abs(f - ref["f"]).max() / scale, np.abs(tq - ref["torque"]).max() / tscale
    eo = np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() / np.abs(ref["wall_out"][:, 1:]).max()
    ee = np.abs(out[:, 0] - ref["wall_out"][:, 0]).max() / np.abs(ref["wall_out"][:, 0]).max()
    print(f"walls: in contact per shape {per_shape.tolist()}, contacts {nc}, rel err f {ef:.1e} torque {et:.1e} wall force {eo:.1e} "
          f"wall energy {ee:.1e}")
    assert scale > 0 and nc == ref["ncontacts"] and max(ef, et, eo, ee) <= GATE
    # damped: random twists, some approaching and some leaving fast enough for the clamp
    rng = np.random.default_rng(5)
    tw = np.concatenate([rng.normal(size=(c["n"], 3)), 0.5 * rng.normal(size=(c["n"], 3))], axis=1)
    gam = np.array([400.0, 250.0, 600.0])
    sp.wall_damping(gam)
    refd = D.wall_forces_damped(shapes_ref, WALL_NQ, c["x"], c["quat"], c["shtype"], tw, c["planes"], c["kn"], c["expo"], gam)
    assert any(ct[3] == 0.0 for ct in refd["contacts"]) and any(ct[3] > ct[2] for ct in refd["contacts"])
    f, tq, out, nc = _wall_run(sp, c, damped=True, tw=tw)
    sp.close()
    scale = max(scale, np.abs(refd["f"]).max())
    tscale = max(scale, np.abs(refd["torque"]).max())
    ef, et = np.abs(f - refd["f"]).max() / scale, np.abs(tq - refd["torque"]).max() / tscale
    eo = np.abs(out[:, 1:] - refd["wall_out"][:, 1:]).max() / scale
    ee = np.abs(out[:, 0] - refd["wall_out"][:, 0]).max() / np.abs(refd["wall_out"][:, 0]).max()
    print(f"damped walls: contacts {nc}, rel err f {ef:.1e} torque {et:.1e} wall force {eo:.1e} wall energy {ee:.1e}")
    assert nc == len(refd["contacts"]) and max(ef, et, eo, ee) <= GATE


# ---- the whole step (tests/mixed_common.py: step_scene) against tests/traj_ref.py, which gets the shapes zero-padded.  The
# reference runs on the CPU inside the tests (seconds), once per scene; the bars are 10 x its own deviation under a 1e-12
# perturbation of every integral, as tests/golden/make_traj_ref.py measures them.

@functools.lru_cache(maxsize=None)
def step_ref(frozen):
    ref = step_reference(frozen)
    print(f"reference (frozen rows: {frozen}): rebuilt at {[k + 1 for k, r in enumerate(ref['rebuilt']) if r]}, smallest margin "
          f"{min(ref['margin']):.2e}, touching slots per step {ref['touching']}, cross-rank mixed slots {len(ref['cross_mixed'])}")
    print("D_q " + "  ".join(f"{q} {ref['D'][q]:.1e}" for q in TR.QUANTITIES))
    assert_step_conditions(ref, frozen)      # from the reference alone
    return ref


def step_ctx(sc, det):
    """A context of the scene: each shape at its own order, the scene's bounding radii."""
    from shpair import ShPair
    nt = sc["K"].shape[0] - 1
    sp = ShPair(0)
    sp.settings(int(sc["nq"]))
    sp.set_ntypes(nt, len(sc["a_nm"]))
    for s, a in enumerate(sc["a_nm"]):
        l = int(sc["own_lmax"][s])
        assert not a[(l + 1) * (l + 2):].any()
        sp.set_shape(s, l, a[:(l + 1) * (l + 2)], float(sc["rmax"][s]))
        assert sp.rmax(s) == sc["rmax"][s]
        sp.set_density(s, float(sc["density"][s]))
    for a in range(1, nt + 1):
        for b in range(1, nt + 1):
            sp.coeff(a, b, sc["K"][a, b], sc["E"][a, b])
    sp.set_option("deterministic", det)
    return sp


def step_options(sc):
    opts = pair_options(sc)
    assert not opts.pop("pair_spring") and not sc["wall_kt"].any()           # history-free friction
    return dict(opts, walls=(sc["planes"], sc["wall_kn"], sc["wall_expo"]), wall_damping=sc["wall_damping"],
                wall_friction=(sc["wall_mu"], sc["wall_gt"]), dt=float(sc["dt"]), gravity=tuple(sc["gravity"]),
                gamma_t=float(sc["gamma_t"]), gamma_r=float(sc["gamma_r"]), groupbit=int(sc["groupbit"]))


def device_run(sc, det):
    import torch
    from shpair.run import DeviceRun
    sp = step_ctx(sc, det)
    r = DeviceRun(sp, sc["x"], sc["quat"], sc["shtype"], sc["lo"], sc["hi"], tuple(int(p) for p in sc["periodic"]), float(sc["skin"]),
                  type_=sc["type"], mask=sc["mask"], ledger=True, **step_options(sc))
    r.v[:] = _dev(sc["v"])
    r.L[:] = _dev(sc["angmom"])
    r.force()               # the set-up forces of the scene's velocities: a look, dt = 0
    torch.cuda.synchronize()
    sp.synchronize()
    return sp, r


def read_run(r):
    import torch
    torch.cuda.synchronize()
    r.sp.synchronize()
    n = r.n
    tot, per = r.sp.energy_ledger()
    return dict(x=r.x[:n].cpu().numpy(), v=r.v[:n].cpu().numpy(), quat=r.q[:n].cpu().numpy(), angmom=r.L[:n].cpu().numpy(),
                f=r.f[:n].cpu().numpy(), torque=r.tq[:n].cpu().numpy(), planes=r.sp.get_walls(), builds=r.builds,
                ledger=np.array(tot), per_wall=np.array(per))


STEP_STATE = ("x", "v", "quat", "angmom", "ledger")       # the scene has no spring: xi and wall_xi are nothing


def over_bar(got, ref, what):
    """Prints measured error against bar per quantity; returns what is over its bar."""
    want = ref["last"]
    # the spring quantities are placeholders so that TR.deviation runs: the scene has no spring (step_options), they are not judged
    full = dict(got, **{k: want[k] for k in ("xi", "xi_i", "xi_key", "wall_xi")})
    err = TR.deviation(full, want)
    print(f"{what}: " + "  ".join(f"{q} {err[q]:.1e} / {ref['bar'][q]:.1e}" for q in STEP_STATE))
    bad = [q for q in STEP_STATE if not err[q] <= ref["bar"][q]]
    if not np.abs(got["planes"] - want["planes"]).max() <= 1e-14 * np.abs(want["planes"]).max():
        bad.append("planes")
    return bad


def test_step_and_run_native_of_mixed_orders_follow_the_whole_step_reference():
    """Orders (2, 4), 24 particles, every model the step composes on the per-shape tables: DeviceRun.step and run_native
    against the reference at the last step, and bit for bit against each other in deterministic mode."""
    ref = step_ref(True)
    sc = ref["sc"]
    sp, r = device_run(sc, 1)
    got0 = read_run(r)
    scale = np.abs(ref["setup"]["f"]).max()
    ef = np.abs(got0["f"] - ref["setup"]["f"]).max() / scale
    et = np.abs(got0["torque"] - ref["setup"]["torque"]).max() / max(scale, np.abs(ref["setup"]["torque"]).max())
    print(f"set-up forces: |dF| {ef:.1e}, |dtau| {et:.1e} of max|F| = {scale:.4g} (bar 1e-9)")
    assert scale > 100 and ef < TOL and et < TOL
    for _ in range(STEP_NSTEPS):
        r.step()
    stepped = read_run(r)
    sp.close()
    sp, r = device_run(sc, 1)
    r.run_native(STEP_NSTEPS)
    native = read_run(r)
    sp.close()
    bad = over_bar(stepped, ref, "DeviceRun.step") + over_bar(native, ref, "run_native")
    assert not bad, bad
    assert stepped["builds"] == native["builds"] == int(ref["last"]["builds"])
    assert [k for k in STEP_STATE + ("f", "torque", "per_wall", "planes") if not np.array_equal(stepped[k], native[k])] == []


def test_two_ranks_of_mixed_orders_follow_the_whole_step_reference():
    """The scene without frozen rows on a 2x1x1 hub of rank threads: the ghost cutoff comes from the largest bounding radius
    over shapes of different orders.  At least 5 slots in contact join a low-order and a high-order row of different ranks
    (counted on the reference's rows with traj_ref.brick_owner)."""
    from shpair import mrank
    import torch
    ref = step_ref(False)
    sc = ref["sc"]
    grid, per = (2, 1, 1), tuple(int(p) for p in sc["periodic"])
    xw, owner = _distribute(grid, sc["lo"], sc["hi"], per, 2.0 * sc["rmax"].max() + float(sc["skin"]), sc["x"])
    hub = mrank.Hub(2)

    def body(rank):
        sp = step_ctx(sc, 1)
        sp.set_option("halo_twists", 1)
        sp.set_energy_ledger(True)
        halo = mrank.Halo(sp, rank, 2, grid, sc["lo"], sc["hi"], per, float(sc["skin"]), hub=hub)
        m = owner == rank
        run = mrank.RankRun(sp, halo, xw[m], sc["quat"][m], sc["shtype"][m], sc["tag"][m], type_=sc["type"][m], v=sc["v"][m],
                            angmom=sc["angmom"][m], mask=sc["mask"][m], check_every=1, **step_options(sc))
        run.run(STEP_NSTEPS)
        run.sync()
        torch.cuda.synchronize()
        n = run.n
        tot, pw = sp.energy_ledger()
        out = dict(tag=run.tag[:n].cpu().numpy(), x=run.x[:n].cpu().numpy(), v=run.v[:n].cpu().numpy(), quat=run.q[:n].cpu().numpy(),
                   angmom=run.L[:n].cpu().numpy(), planes=sp.get_walls(), builds=run.builds, ledger=np.array(tot), per_wall=np.array(pw))
        halo.close()
        sp.close()
        return out
    parts = _run_ranks(2, body)
    hub.close()
    keys = ("x", "v", "quat", "angmom")
    got = dict(zip(keys, _gather(parts, len(sc["x"]), keys)))                # the scene's tags are its rows
    got.update(ledger=sum(p["ledger"] for p in parts), per_wall=sum(p["per_wall"] for p in parts), planes=parts[0]["planes"])
    assert all(len(p["tag"]) > 0 for p in parts)
    assert over_bar(got, ref, "2x1x1") == []
    assert [p["builds"] for p in parts] == [int(ref["last"]["builds"])] * 2
    assert np.array_equal(parts[0]["planes"], parts[1]["planes"])
