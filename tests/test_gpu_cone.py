"""GPU tests of the conical container walls of docs/SPEC.md §2.22 (csrc/cone_kernels.hpp through the C ABI of
include/shstep.h) against tests/cone_ref.py: forces, torques and per-cone totals at SPEC §4's gate (1e-9 of the largest
force), every order, the axis and the apex, two cones and a cone beside a cylinder and a plane, masks, errors, the
dissipative instance, reproducibility, every refusal, the step loops, and a sphere at rest and dragged in a hopper.
Every case has at most 16 particles."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dissipation_common import _wall_ctx as ctx, dev  # noqa: E402

GATE = 1e-9
AXIS = np.array([2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0])   # a unit axis with rational components


def oblique(theta=np.pi / 6):
    import cone_ref as Co
    return Co.cone([0.3, -0.2, 0.5], AXIS, theta)


def ref_shapes(sp, shp):
    return [(lmax, a, sp.rmax(s)) for s, (lmax, a) in enumerate(shp)]


def cone_case(seed, n, nshapes, rmax, co, lo=0.5, hi=1.15, smin=4.0, smax=8.0):
    """n particles inside cone `co`, their distances h to the wall uniform in [lo, hi] Rmax of their shape, their foot
    points between smin and smax along a generator."""
    from shpair import bed
    rng = np.random.default_rng(seed)
    a, ax, ct, st = co[:3], co[3:6], co[6], co[7]
    e1 = np.cross(ax, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(ax, e1)
    sht = rng.integers(0, nshapes, n).astype(np.int32)
    h = rng.uniform(lo, hi, n) * np.asarray(rmax)[sht]
    s, phi = rng.uniform(smin, smax, n), rng.uniform(0, 2 * np.pi, n)
    t, d = ct * s + st * h, st * s - ct * h
    assert (d > 0).all()
    x = a + d[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2) + t[:, None] * ax
    return dict(x=x, quat=bed.random_quaternions(n, rng), shtype=sht, n=n)


def run_device(sp, case, cones, kn, expo, mask=None, groupbit=1, f0=None, want_out=True, tw=None, coef=None, pass_twist=True,
               set_cones=True):
    """One shstep_cone_force_device call on fresh device arrays.  coef: (gamma, mu, gamma_t, omega).  Returns f, torque,
    cone_out, ncontacts."""
    import torch
    n = case["n"]
    cones = np.atleast_2d(cones)
    if set_cones:
        sp.set_cones(cones, kn, expo)
        if coef is not None:
            sp.cone_damping(coef[0])
            sp.cone_friction(coef[1], coef[2])
            sp.cone_rotation(coef[3])
    x, q, sh = dev(case["x"]), dev(case["quat"]), dev(case["shtype"])
    m = dev(np.ones(n, dtype=np.int32) if mask is None else mask.astype(np.int32))
    f = dev(np.zeros((n, 3)) if f0 is None else f0[0])
    tq = dev(np.zeros((n, 3)) if f0 is None else f0[1])
    twd = None if tw is None else dev(tw)
    out = torch.zeros(len(cones), 5, dtype=torch.float64, device="cuda:0")
    sp.cone_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(),
                         twist=twd.data_ptr() if twd is not None and pass_twist else None, groupbit=groupbit,
                         cone_out=out.data_ptr() if want_out else None)
    torch.cuda.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy(), sp.cone_stats()


def check_against_ref(got, ref, label):
    f, tq, out, nc = got
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ef, et = np.abs(f - ref["f"]).max() / scale, np.abs(tq - ref["torque"]).max() / tscale
    ro = ref["cone_out"]
    eo = np.abs(out[:, 1:4] - ro[:, 1:4]).max() / np.abs(ro[:, 1:4]).max()
    ee = np.abs(out[:, 0] - ro[:, 0]).max() / np.abs(ro[:, 0]).max()
    em = np.abs(out[:, 4] - ro[:, 4]).max() / max(tscale, np.abs(ro[:, 4]).max())
    print(f"{label}: contacts {nc}, max|F| {scale:.4g}, rel err f {ef:.1e} torque {et:.1e} wall force {eo:.1e} energy {ee:.1e} M_ax {em:.1e}")
    assert scale > 0 and nc == ref["ncontacts"] and nc > 0
    assert max(ef, et, eo, ee, em) <= GATE
    assert np.abs(f.sum(axis=0) + out[:, 1:4].sum(axis=0)).max() <= GATE * scale * max(1, nc)   # momentum


@pytest.mark.parametrize("nq", [8, 32])
def test_oblique_cone_with_mixed_orders_matches_reference(oracle, nq):
    """An oblique 30-degree cone, shapes of L = 2 and L = 6 in one context, exponent 1.25; the totals, M_ax among them,
    are the same bits with and without "deterministic"."""
    import cone_ref as Co
    from shpair import shapes
    shp = [(2, shapes.random_shape(2, 502, amp=0.1)), (6, shapes.random_shape(6, 506, amp=0.1))]
    sp = ctx(shp, nq, deterministic=1)
    rs = ref_shapes(sp, shp)
    co = oblique()
    case = cone_case(nq, 16, 2, [r[2] for r in rs], co)
    assert set(case["shtype"]) == {0, 1}
    got = run_device(sp, case, co, 1000.0, 1.25)
    ref = Co.cone_forces(rs, nq, case["x"], case["quat"], case["shtype"], [co], [1000.0], [1.25])
    assert ref["noutside"] == 0
    check_against_ref(got, ref, f"mixed L, nq={nq}")
    again = run_device(sp, case, co, 1000.0, 1.25)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3]))
    assert np.array_equal(sp.get_cones(), np.atleast_2d(co))
    sp.close()
    sp2 = ctx(shp, nq)
    plain = run_device(sp2, case, co, 1000.0, 1.25)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], plain[:3]))
    sp2.close()


@pytest.mark.parametrize("lmax", list(range(13)) + [15, 20])
def test_every_order(oracle, lmax):
    """Every compiled order 0..12 and the run-time orders 15 and 20, 8 particles, an axis along z, 50 degrees, exponent 2."""
    import cone_ref as Co
    from shpair import shapes
    shp = [(lmax, shapes.random_shape(lmax, 900 + lmax, amp=0.1))]
    sp = ctx(shp, 8)
    rs = ref_shapes(sp, shp)
    co = Co.cone([0.1, 0.2, 0.0], [0.0, 0.0, 1.0], np.radians(50.0))
    case = cone_case(100 + lmax, 8, 1, [rs[0][2]], co, hi=0.9)
    got = run_device(sp, case, co, 800.0, 2.0)
    ref = Co.cone_forces(rs, 8, case["x"], case["quat"], case["shtype"], [co], [800.0], [2.0])
    check_against_ref(got, ref, f"L={lmax}")
    sp.close()


def test_centre_on_the_axis_and_within_reach_of_the_apex(oracle):
    """One centre exactly on the axis (d = 0 as computed: c^ from the frame rule, the whole sphere), one within R_i of the
    apex off the axis (the whole sphere too; both take the frame about the axis), one just beyond R_i of the apex (the
    inscribed sphere's bound, the frame about n^)."""
    import cone_ref as Co
    from shpair import shapes
    shp = [(6, shapes.random_shape(6, 3, amp=0.1))]
    sp = ctx(shp, 16)
    rs = ref_shapes(sp, shp)
    rm = rs[0][2]
    co = Co.cone([0.5, -0.25, 0.0], [0.0, 0.0, 1.0], np.pi / 6)
    x = np.array([[0.5, -0.25, 1.6 * rm], [0.5 + 0.2 * rm, -0.25, 0.9 * rm], [0.5, -0.25 + 0.3 * rm, 1.3 * rm]])
    case = dict(x=x, quat=np.array([[0.5, 0.5, -0.5, 0.5], [1.0, 0, 0, 0], [0.5, -0.5, 0.5, 0.5]]), shtype=np.zeros(3, np.int32), n=3)
    t0, _, d0, _, h0 = Co.foot(x[0], co)
    assert d0 == 0.0 and 0 < h0 < rm and Co.cap_cos(co, t0, d0, rm) == -1.0
    t1, _, d1, _, h1 = Co.foot(x[1], co)
    assert d1 > 0 and 0 < h1 < rm and t1 * t1 + d1 * d1 < rm * rm and Co.cap_cos(co, t1, d1, rm) == -1.0
    t2, _, d2, _, h2 = Co.foot(x[2], co)
    assert 0 < h2 < rm and t2 * t2 + d2 * d2 > rm * rm and -1.0 < Co.cap_cos(co, t2, d2, rm) < 1.0
    got = run_device(sp, case, co, 1000.0, 1.25)
    ref = Co.cone_forces(rs, 16, x, case["quat"], case["shtype"], [co], [1000.0], [1.25])
    assert ref["ncontacts"] == 3
    check_against_ref(got, ref, "axis and apex")
    sp.close()


def test_two_cones_and_a_cone_beside_a_cylinder_and_a_plane_add_in_order(oracle):
    """Two cones whose walls both reach the particles, different force laws: the reference at the gate, and bit for bit
    the two single-cone passes in index order.  Then a plane, a cylinder and a cone in reach of the same particles, in
    the order of a step (planes, cylinders, cones): the same bits as the three passes from contexts that hold one each."""
    import torch
    import cone_ref as Co
    from shpair import shapes, bed
    shp = [(6, shapes.random_shape(6, 5, amp=0.1))]
    sp = ctx(shp, 16)
    rs = ref_shapes(sp, shp)
    rm = rs[0][2]
    th = np.pi / 6
    # two 30-degree cones along z, apices 1.4 Rmax apart in x: a centre between the two axes is near both walls
    t0 = 4.0
    Rloc = t0 * np.tan(th)
    off = Rloc - 0.7 * rm / np.cos(th)
    cones = np.array([Co.cone([-off, 0, 0], [0, 0, 1.0], th), Co.cone([off, 0, 0], [0, 0, 1.0], th)])
    rng = np.random.default_rng(4)
    n = 6
    x = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.2, 0.2, n), t0 + rng.uniform(-0.2, 0.2, n)], axis=1)
    case = dict(x=x, quat=bed.random_quaternions(n, rng), shtype=np.zeros(n, np.int32), n=n)
    kn, ex = np.array([1000.0, 700.0]), np.array([1.25, 2.0])
    got = run_device(sp, case, cones, kn, ex)
    ref = Co.cone_forces(rs, 16, x, case["quat"], case["shtype"], cones, kn, ex)
    assert ref["ncontacts"] == 2 * n
    check_against_ref(got, ref, "two cones")
    f0, t0_, _, _ = run_device(sp, case, cones[0], kn[:1], ex[:1])
    f01, t01, _, _ = run_device(sp, case, cones[1], kn[1:], ex[1:], f0=(f0, t0_))
    assert np.array_equal(f01, got[0]) and np.array_equal(t01, got[1])
    # a plane below, a cylinder round and cone 0, all within reach
    plane = np.array([[0.0, 0.0, 1.0, 4.0 - 0.2 - 0.5 * rm]])
    cyl = np.array([[-off, 0.0, 0.0, 0.0, 0.0, 1.0, Rloc - 0.25 * rm]])

    def three(s, which, f0):
        xd, q, sh, m = dev(x), dev(case["quat"]), dev(case["shtype"]), dev(np.ones(n, dtype=np.int32))
        f, tq = dev(f0[0]), dev(f0[1])
        a = (n, xd.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
        counts = []
        if "plane" in which:
            s.wall_force_device(*a)
            torch.cuda.synchronize()
            counts.append(s.wall_stats())
        if "cyl" in which:
            s.cylinder_force_device(*a)
            torch.cuda.synchronize()
            counts.append(s.cylinder_stats())
        if "cone" in which:
            s.cone_force_device(*a)
            torch.cuda.synchronize()
            counts.append(s.cone_stats())
        return (f.cpu().numpy(), tq.cpu().numpy()), counts
    sp.set_walls(plane, 900.0, 1.5)
    sp.set_cylinders(cyl, 800.0, 1.25)
    sp.set_cones(cones[:1], 1000.0, 1.25)
    zero = (np.zeros((n, 3)), np.zeros((n, 3)))
    all3, counts = three(sp, ("plane", "cyl", "cone"), zero)
    assert all(c > 0 for c in counts), counts
    sp.close()
    acc = zero
    for which in ("plane", "cyl", "cone"):
        s1 = ctx(shp, 16)
        if which == "plane":
            s1.set_walls(plane, 900.0, 1.5)
        elif which == "cyl":
            s1.set_cylinders(cyl, 800.0, 1.25)
        else:
            s1.set_cones(cones[:1], 1000.0, 1.25)
        acc, _ = three(s1, (which,), acc)
        s1.close()
    assert np.array_equal(acc[0], all3[0]) and np.array_equal(acc[1], all3[1])


def test_groupbit_masks_particles_and_the_pass_adds(oracle):
    import cone_ref as Co
    from shpair import shapes
    shp = [(4, shapes.random_shape(4, 11, amp=0.1))]
    sp = ctx(shp, 10)
    rs = ref_shapes(sp, shp)
    n = 16
    co = oblique()
    case = cone_case(5, n, 1, [rs[0][2]], co, hi=0.95)
    rng = np.random.default_rng(3)
    mask = np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.int32)
    f0 = (rng.normal(size=(n, 3)), rng.normal(size=(n, 3)))
    f, tq, out, nc = run_device(sp, case, co, 1000.0, 1.25, mask=mask, groupbit=2, f0=f0)
    ref = Co.cone_forces(rs, 10, case["x"], case["quat"], case["shtype"], [co], [1000.0], [1.25], mask=mask, groupbit=2)
    off = mask == 1
    assert np.array_equal(f[off], f0[0][off]) and np.array_equal(tq[off], f0[1][off])   # masked rows: not a bit changed
    check_against_ref((f - f0[0], tq - f0[1], out, nc), ref, "groupbit")   # the forces are ADDED to what was there
    # no cone set: the call returns at once, f and torque keep their bits, and there is nothing to count
    sp.set_cones(None)
    assert sp.ncones == 0
    x, q, sh, m = dev(case["x"]), dev(case["quat"]), dev(case["shtype"]), dev(np.ones(n, dtype=np.int32))
    fd, td = dev(f0[0]), dev(f0[1])
    sp.cone_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), fd.data_ptr(), td.data_ptr())
    sp.synchronize()
    assert np.array_equal(fd.cpu().numpy(), f0[0]) and np.array_equal(td.cpu().numpy(), f0[1]) and sp.cone_stats() == 0
    sp.close()


def test_centre_outside_a_cone_is_an_error_and_the_rest_is_right(oracle):
    import torch
    import cone_ref as Co
    from shpair import shapes
    from shpair.capi import ShPairError
    shp = [(4, shapes.random_shape(4, 11, amp=0.1))]
    sp = ctx(shp, 10)
    rs = ref_shapes(sp, shp)
    n = 12
    co = Co.cone([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], np.pi / 6)
    case = cone_case(6, n, 1, [rs[0][2]], co)
    case["x"][7] = [4.0, 0.0, 5.0]      # outside the wall
    case["x"][8] = [0.0, 0.1, -0.5]     # behind the apex
    sp.set_cones([co], 1000.0, 1.25)
    x, q, sh, m = dev(case["x"]), dev(case["quat"]), dev(case["shtype"]), dev(np.ones(n, dtype=np.int32))
    f, tq = dev(np.zeros((n, 3))), dev(np.zeros((n, 3)))
    sp.cone_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    torch.cuda.synchronize()
    with pytest.raises(ShPairError, match="particle centre outside a cone") as e:
        sp.cone_stats()
    assert e.value.code == -1   # SHPAIR_EINVAL
    sp.synchronize()            # the error word was read and cleared
    ref = Co.cone_forces(rs, 10, case["x"], case["quat"], case["shtype"], [co], [1000.0], [1.25])
    assert ref["noutside"] == 2 and not ref["f"][7].any() and not ref["f"][8].any() and ref["ncontacts"] > 0
    scale = np.abs(ref["f"]).max()
    assert np.abs(f.cpu().numpy() - ref["f"]).max() <= GATE * scale and np.abs(tq.cpu().numpy() - ref["torque"]).max() <= GATE * scale
    sp.close()


def test_dissipative_instance_matches_reference(oracle):
    """gamma_k, mu_k, gamma_t,k and Omega != 0 with random twists: (a) one oblique cone, two shapes; (b) two cones both in
    reach of every particle, with different coefficients per cone (one capped by a small mu, one viscous), so that the
    rows of the coefficient table are read at ncone = 2."""
    import cone_ref as Co
    from shpair import shapes, bed
    from shpair.capi import ShPairError
    shp = [(6, shapes.random_shape(6, 21 + s, amp=0.1)) for s in range(2)]
    sp = ctx(shp, 16, deterministic=1)
    rs = ref_shapes(sp, shp)
    rng = np.random.default_rng(2)
    rm = max(r[2] for r in rs)
    n = 8
    th, t0 = np.pi / 6, 4.0
    off = t0 * np.tan(th) - 0.55 * rm / np.cos(th)
    duct = np.array([Co.cone([-off, 0, 0], [0, 0, 1.0], th), Co.cone([off, 0, 0], [0, 0, 1.0], th)])
    xd = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.2, 0.2, n), t0 + rng.uniform(-0.2, 0.2, n)], axis=1)
    co = oblique()
    legs = [("one oblique cone", cone_case(9, 16, 2, [r[2] for r in rs], co, hi=0.9), np.atleast_2d(co),
             np.array([1000.0]), np.array([1.25]), (np.array([40.0]), np.array([0.02]), np.array([900.0]), np.array([1.7]))),
            ("two cones", dict(x=xd, quat=bed.random_quaternions(n, rng), shtype=rng.integers(0, 2, n).astype(np.int32), n=n),
             duct, np.array([1000.0, 800.0]), np.array([1.25, 1.5]),
             (np.array([40.0, 15.0]), np.array([0.02, 0.6]), np.array([900.0, 3.0]), np.array([1.7, -0.8])))]
    for label, case, cones, kn, ex, coef in legs:
        m = case["n"]
        tw = np.concatenate([rng.normal(size=(m, 3)), 0.5 * rng.normal(size=(m, 3))], axis=1)
        args = (rs, 16, case["x"], case["quat"], case["shtype"], cones, kn, ex)
        got = run_device(sp, case, cones, kn, ex, tw=tw, coef=coef)
        ref = Co.cone_forces(*args, tw=tw, gamma=coef[0], mu=coef[1], gt=coef[2], omega=coef[3])
        check_against_ref(got, ref, f"dissipative, {label}")
        assert ref["ncontacts"] >= len(cones) * 8 and all(np.linalg.norm(d["Ft"]) > 0 for _, _, d in ref["contacts"])
        for c in range(len(cones)):   # cone 0 is capped by its small mu, cone 1 stays viscous
            assert {d["capped"] for _, cc, d in ref["contacts"] if cc == c} == {c == 0}
        elastic = Co.cone_forces(*args)
        assert np.abs(elastic["f"] - ref["f"]).max() > 1e-3 * np.abs(ref["f"]).max()   # the coefficients did act
        still = Co.cone_forces(*args, tw=tw, gamma=coef[0], mu=coef[1], gt=coef[2])      # ... and so did Omega
        assert np.abs(still["f"] - ref["f"]).max() > 1e-6 * np.abs(ref["f"]).max()
        undamped = Co.cone_forces(*args, tw=tw, mu=coef[1], gt=coef[2], omega=coef[3])  # ... and gamma_k on its own
        assert np.abs(undamped["f"] - ref["f"]).max() > 1e-3 * np.abs(ref["f"]).max()
        if len(cones) == 2:   # the coefficients of the two cones exchanged give another answer: each row is read at its own index
            swapped = Co.cone_forces(*args, tw=tw, gamma=coef[0][::-1], mu=coef[1][::-1], gt=coef[2][::-1], omega=coef[3][::-1])
            assert np.abs(swapped["f"] - ref["f"]).max() > 1e-3 * np.abs(ref["f"]).max()
        with pytest.raises(ShPairError, match="null twist pointer") as e:   # a coefficient is set: the twists are needed
            run_device(sp, case, cones, kn, ex, tw=tw, coef=coef, pass_twist=False)
        assert e.value.code == -1
    sp.close()


def test_zero_coefficients_give_the_elastic_bits_with_or_without_twists(oracle):
    from shpair import shapes
    shp = [(6, shapes.random_shape(6, 21, amp=0.1))]
    sp = ctx(shp, 16)
    rm = sp.rmax(0)
    co = oblique()
    case = cone_case(12, 16, 1, [rm], co)
    tw = np.random.default_rng(1).normal(size=(16, 6))
    zero = (0.0, 0.0, 0.0, 0.0)
    a = run_device(sp, case, co, 1000.0, 1.25)
    b = run_device(sp, case, co, 1000.0, 1.25, tw=tw, coef=zero)
    c = run_device(sp, case, co, 1000.0, 1.25, tw=tw, coef=zero, pass_twist=False)
    d = run_device(sp, case, co, 1000.0, 1.25, tw=tw, coef=(0.0, 0.5, 0.0, 2.0))   # a mu without a gamma_t, a rotation: no coefficient
    assert a[3] > 0
    for other in (b, c, d):
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], other[:3]))
    sp.close()


def test_every_refusal(oracle):
    from shpair import shapes
    from shpair.capi import ShPairError
    sp = ctx([(0, shapes.sphere(1.0))], 8)
    co = oblique()
    sp.set_cones([co], 1000.0, 1.25)
    sp.set_energy_ledger(True)            # an elastic cone at rest dissipates nothing and takes no work: allowed
    for call in (lambda: sp.cone_damping(2.0), lambda: sp.cone_friction(0.5, 2.0), lambda: sp.cone_rotation(1.5)):
        with pytest.raises(ShPairError, match="energy ledger is on and keeps no cone entries") as e:
            call()
        assert e.value.code == -4 and not sp.cone_reads_twists   # SHPAIR_ESTATE, and the state stays what it was
    sp.cone_friction(0.5, 0.0)            # no coefficient: fine
    sp.set_energy_ledger(False)
    sp.set_shell_ledger(True)             # the shell ledger keeps the cylinders' entries, none for a cone
    with pytest.raises(ShPairError, match="shell ledger is on and keeps no cone entries") as e:
        sp.cone_damping(2.0)
    assert e.value.code == -4
    sp.set_shell_ledger(False)
    for setter in (lambda: sp.cone_damping(2.0), lambda: sp.cone_rotation(1.5)):   # and the reverse, for a coefficient and for Omega alone
        sp.set_cones([co], 1000.0, 1.25)
        setter()
        with pytest.raises(ShPairError, match="ledger keeps no cone entries") as e:
            sp.set_energy_ledger(True)
        assert e.value.code == -4 and not sp.ledger_on
        with pytest.raises(ShPairError, match="ledger keeps no cone entries") as e:
            sp.set_shell_ledger(True)
        assert e.value.code == -4 and not sp.shell_ledger_on
    sp.set_cones([co], 1000.0, 1.25)
    sp.cone_damping(2.0)
    # the geometry: the outside of a cone (an angle beyond pi/2 has a cosine < 0), theta = 0 and pi/2, a pair that is not on
    # the unit circle, the axis, the law, the count
    ok = co.tolist()
    for cones, kn, ex in (([ok[:6] + [-ok[6], ok[7]]], 1.0, 1.0), ([ok[:6] + [1.0, 0.0]], 1.0, 1.0), ([ok[:6] + [0.0, 1.0]], 1.0, 1.0),
                          ([ok[:6] + [ok[6], ok[7] + 1e-9]], 1.0, 1.0), ([ok[:3] + [0, 0, 1.0 + 1e-9] + ok[6:]], 1.0, 1.0),
                          ([ok[:6] + [np.nan, ok[7]]], 1.0, 1.0), ([[np.inf] + ok[1:]], 1.0, 1.0), ([ok], -1.0, 1.0), ([ok], 1.0, 0.5),
                          ([ok], np.nan, 1.0), ([ok] * 9, 1.0, 1.0)):
        with pytest.raises(ShPairError) as e:
            sp.set_cones(cones, kn, ex)
        assert e.value.code == -1
    assert sp.ncones == 1 and sp.cone_reads_twists   # a refused call changes nothing
    for bad in ((-1.0,), (np.nan,), (1.0, 2.0)):
        with pytest.raises(ShPairError) as e:
            sp.cone_damping(np.array(bad))
        assert e.value.code == -1
    with pytest.raises(ShPairError):
        sp.cone_rotation(np.inf)
    sp.set_cones([ok] * 8, 1.0, 1.0)
    assert sp.ncones == 8 and not sp.cone_reads_twists
    # springs, rolling and twisting at cones, an outlet, a translation: there is no entry point and no option for them
    from shpair import step_pass
    import inspect
    assert not [m for m in dir(sp) if "cone" in m and any(w in m for w in ("spring", "rolling", "twisting", "history", "velocity"))]
    assert not [p for p in inspect.signature(step_pass.apply_contact_options).parameters
                if "cone" in p and p not in ("cones", "cone_damping", "cone_friction", "cone_rotation")]
    # the loop over several ranks, and its Python driver: refused while a cone is set, elastic or not
    from shpair import mrank
    from shpair.capi import HaloArrays, HaloRunParams
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    stand_in = type("R", (), dict(sp=sp, a=None, stream=None, halo=None))()
    with pytest.raises(ShPairError, match="conical walls are single-rank") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -4
    with pytest.raises(ShPairError, match="conical walls are single-rank") as e:
        mrank.RankRun.force(stand_in)
    assert e.value.code == -4
    sp.set_cones(None)                    # the cause removed: both get past the refusal (and stop at the empty arguments)
    with pytest.raises(Exception) as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert "single-rank" not in str(e.value)
    with pytest.raises(Exception) as e:
        mrank.RankRun.force(stand_in)
    assert "single-rank" not in str(e.value)
    halo.close()
    sp.close()


# ---- steps ---------------------------------------------------------------------------------------------------------

def _state(r):
    n = r.n
    return [t.cpu().numpy().copy() for t in (r.x[:n], r.v, r.q[:n], r.L, r.f[:n], r.tq[:n])]


@pytest.mark.parametrize("dissipative", [False, True])
def test_run_loops_with_a_cone_are_bitwise_identical(oracle, dissipative):
    """shstep_run_device plain, with hipGraph replay, and the call-by-call Python loop: the same bits over 32 steps, for
    the elastic instance and for the dissipative one with a turning cone; and the cone did act."""
    import torch
    import cone_ref as Co
    from shpair import shapes, bed
    from shpair.run import DeviceRun
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    rm = oracle.shape_rmax(4, shp[0][1])
    rng = np.random.default_rng(12)
    # a hopper along z in the box [0, 8]^3, apex at z = 0.5: eight particles on a ring, each 0.9 Rmax from the wall
    th = np.pi / 6
    co = Co.cone([4.0, 4.0, 0.5], [0.0, 0.0, 1.0], th)
    s = 6.0
    t, d = np.cos(th) * s + np.sin(th) * 0.9 * rm, np.sin(th) * s - np.cos(th) * 0.9 * rm
    phi = np.arange(8) * np.pi / 4
    x = np.stack([4.0 + d * np.cos(phi), 4.0 + d * np.sin(phi), 0.5 + t + 0 * phi], axis=1) + rng.uniform(-0.02, 0.02, (8, 3))
    quat, sht = bed.random_quaternions(8, rng), np.zeros(8, np.int32)
    extra = dict(cone_damping=20.0, cone_friction=(0.4, 30.0), cone_rotation=0.8) if dissipative else {}

    def go(mode, cones):
        sp = ctx(shp, 10, kn=2000.0, deterministic=1)
        r = DeviceRun(sp, x, quat, sht, (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, dt=5e-4, gravity=(0.0, 0.0, -9.81), gamma_t=0.2,
                      gamma_r=0.1, cones=cones, **(extra if cones else {}))
        if mode == "python":
            r.run(32)
        else:
            r.run_native(32, use_graph=(mode == "graph"))
        torch.cuda.synchronize()
        st, nc = _state(r), sp.cone_stats()
        sp.close()
        return st, nc
    ref, nc = go("python", ([co], 2000.0, 1.25))
    assert nc > 0
    for mode in ("plain", "graph"):
        got, nc2 = go(mode, ([co], 2000.0, 1.25))
        assert nc2 == nc
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), mode
    never, _ = go("graph", None)
    assert not np.array_equal(never[0], ref[0])


def _rest_depth(Co, co, kn, m, weight, nq, lateral=(0.0, 0.0)):
    """h* of a unit sphere (Rmax 1.01) with kn m V^(m-1) |S_n.a^| = weight, by bisection on the reference along the line
    parallel to the axis (z) at the lateral place `lateral`; h is sin(theta) t, the wall distance of the axis point."""
    from shpair import shapes
    a = shapes.sphere(1.0)

    def force(h):
        x = co[:3] + (h / co[7]) * co[3:6] + np.array([lateral[0], lateral[1], 0.0])
        V, S, T, _ = Co.cone_sums(0, a, 1.01, x, (1, 0, 0, 0), co, nq)
        return kn * m * V ** (m - 1) * abs(S @ co[3:6]) if V > 0 else 0.0
    lo, hi = 0.8, 1.0
    assert force(lo) > weight > force(hi)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if force(mid) > weight else (lo, mid)
    return 0.5 * (lo + hi)


def test_sphere_rests_on_the_axis_at_the_depth_of_the_force_balance_and_a_turning_cone_drags_it(oracle):
    """A unit sphere dropped on the axis of a 30-degree hopper (axis z, gravity -z) with gamma_k comes to rest on the axis
    with h = sin(theta) t = h*, kn m V^(m-1) |S_n.a^| = m g at h* from the reference.  Tolerance, formed as for the cylinder
    (tests/test_gpu_cylinder.py): the sharp rule makes S_n a step function of h with steps of up to 1.1e-2 |S_n| for a unit
    sphere (SPEC §2.9), the force goes as (1 - h)^1.5, so the balance is uncertain by 0.8e-2 (1 - h*); the bar is
    2e-2 (1 - h*).  (Measured: h = h* to 1e-6; the sphere ends chattering across the step that h* is, at 4.4e-4.)  Near
    the axis the cap is the whole sphere and the frame is about the axis, so the nodes keep the symmetry of the contact:
    the centre stays on the axis to rounding (measured 9e-17); the bar for its distance from it is the same
    2e-2 (1 - h*), h* being taken on the line parallel to the axis through the place where the centre came to rest.  A body
    drag damps the lateral motion, which nothing else does on the axis.
    With Omega > 0, friction and a drag on the sphere's spin and velocity, the same sphere on the lowest generator of a
    cone whose axis is tilted up by theta (that generator is horizontal, along x, and the wall moves along +y there) ends
    displaced towards +y, and the moment M_ax of the particle's force on the wall opposes Omega."""
    import torch
    import cone_ref as Co
    from shpair import shapes
    from shpair.run import DeviceRun
    m, nq = 1.25, 32
    co = Co.cone([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], np.pi / 6)
    tilted = Co.cone([0.0, 0.0, 0.0], [np.cos(np.pi / 6), 0.0, np.sin(np.pi / 6)], np.pi / 6)
    res = {}
    # (the ring of contact of a sphere on the axis is stiff: kn = 40 puts h* near 0.96, and gamma_k = 40 is its critical
    # damping; the sphere on a generator has the cylinder's patch, and its kn and gamma_k)
    for label, cone, x0, kn, gam, extra in (("rest", co, [0.0, 0.0, 2.02], 40.0, 40.0, {}),
                                            ("drag", tilted, [5.0, 0.0, 1.05], 1e4, 3e5, dict(cone_friction=(0.5, 50.0), cone_rotation=2.0))):
        sp = ctx([(0, shapes.sphere(1.0))], nq, kn=kn, expo=m, rmax=[1.01])
        mass = sp.body(0)[0]
        r = DeviceRun(sp, np.array([x0]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-8, -8, -8), (8, 8, 8), (0, 0, 0), 0.5,
                      dt=1e-4, gravity=(0.0, 0.0, -9.81), gamma_t=40.0 if extra else 25.0, gamma_r=5.0 if extra else 0.0,   # (on the axis nothing else damps the lateral motion)
                      cones=([cone], kn, m), cone_damping=gam, check=False, **extra)
        r.run_native(12000, use_graph=True)
        out = torch.zeros(1, 5, dtype=torch.float64, device="cuda:0")
        f, tq = torch.zeros_like(r.f), torch.zeros_like(r.tq)
        sp.twist_device(1, 0, r.v.data_ptr(), r.q.data_ptr(), r.L.data_ptr(), r.sh.data_ptr(), r.twist.data_ptr())
        sp.cone_force_device(1, r.x.data_ptr(), r.q.data_ptr(), r.sh.data_ptr(), r.mask.data_ptr(), f.data_ptr(), tq.data_ptr(),
                             twist=r.twist.data_ptr(), cone_out=out.data_ptr())
        torch.cuda.synchronize()
        sp.synchronize()   # no error bit
        res[label] = (r.x[0].cpu().numpy().copy(), r.v[0].cpu().numpy().copy(), out.cpu().numpy()[0], mass)
        sp.close()
    x, v, out, mass = res["rest"]
    hstar = _rest_depth(Co, co, 40.0, m, mass * 9.81, nq, lateral=x[:2])
    h = co[7] * x[2]
    print(f"rest: h {h:.6f}, h* {hstar:.6f}, |v| {np.linalg.norm(v):.1e}, x {x[0]:.1e} y {x[1]:.1e}, wall force z {out[3]:.4f}, weight {mass * 9.81:.4f}")
    assert abs(h - hstar) <= 2e-2 * (1.0 - hstar) and np.linalg.norm(v) <= 1e-3 and np.hypot(x[0], x[1]) <= 2e-2 * (1.0 - hstar)
    x, v, out, mass = res["drag"]
    print(f"drag: x {x[0]:.5f}, y {x[1]:.5f}, z {x[2]:.5f}, M_ax {out[4]:.4f}")
    assert x[1] > 1e-4 and out[4] < 0.0
