"""GPU tests of the cylindrical container walls of docs/SPEC.md §2.18 (csrc/cylinder_kernels.hpp through the C ABI of
include/shstep.h) against tests/cyl_ref.py: forces, torques and per-cylinder totals at SPEC §4's gate (1e-9 of the
largest force), every order and both ends of the n_q range, the axis and two cylinders, masks, errors, the dissipative
instance, reproducibility, the step loops, and a sphere at rest and dragged in a drum."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dissipation_common import _wall_ctx as ctx, dev  # noqa: E402

GATE = 1e-9
OBLIQUE = np.array([0.3, -0.2, 0.5, 2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0, 4.0])   # a, a unit axis with rational components, Rc


def ref_shapes(sp, shp):
    return [(lmax, a, sp.rmax(s)) for s, (lmax, a) in enumerate(shp)]


def cyl_case(seed, n, nshapes, rmax, cyl, lo=0.5, hi=1.15):
    """n particles inside cylinder `cyl`, their depth margins h = Rc - d uniform in [lo, hi] Rmax of their shape."""
    from shpair import bed
    rng = np.random.default_rng(seed)
    a, ax, Rc = cyl[:3], cyl[3:6], cyl[6]
    e1 = np.cross(ax, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(ax, e1)
    sht = rng.integers(0, nshapes, n).astype(np.int32)
    d = Rc - rng.uniform(lo, hi, n) * np.asarray(rmax)[sht]
    phi, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(-3, 3, n)
    x = a + d[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2) + z[:, None] * ax
    return dict(x=x, quat=bed.random_quaternions(n, rng), shtype=sht, n=n)


def run_device(sp, case, cyls, kn, expo, mask=None, groupbit=1, f0=None, want_out=True, tw=None, coef=None, pass_twist=True):
    """One shstep_cylinder_force_device call on fresh device arrays.  coef: (gamma, mu, gamma_t, omega).  Returns f,
    torque, cyl_out, ncontacts."""
    import torch
    n = case["n"]
    cyls = np.atleast_2d(cyls)
    sp.set_cylinders(cyls, kn, expo)
    if coef is not None:
        sp.cylinder_damping(coef[0])
        sp.cylinder_friction(coef[1], coef[2])
        sp.cylinder_rotation(coef[3])
    x, q, sh = dev(case["x"]), dev(case["quat"]), dev(case["shtype"])
    m = dev(np.ones(n, dtype=np.int32) if mask is None else mask.astype(np.int32))
    f = dev(np.zeros((n, 3)) if f0 is None else f0[0])
    tq = dev(np.zeros((n, 3)) if f0 is None else f0[1])
    twd = None if tw is None else dev(tw)
    out = torch.zeros(len(cyls), 5, dtype=torch.float64, device="cuda:0")
    sp.cylinder_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(),
                             twist=twd.data_ptr() if twd is not None and pass_twist else None, groupbit=groupbit,
                             cyl_out=out.data_ptr() if want_out else None)
    torch.cuda.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy(), sp.cylinder_stats()


def check_against_ref(got, ref, label):
    f, tq, out, nc = got
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ef, et = np.abs(f - ref["f"]).max() / scale, np.abs(tq - ref["torque"]).max() / tscale
    ro = ref["cyl_out"]
    eo = np.abs(out[:, 1:4] - ro[:, 1:4]).max() / np.abs(ro[:, 1:4]).max()
    ee = np.abs(out[:, 0] - ro[:, 0]).max() / np.abs(ro[:, 0]).max()
    em = np.abs(out[:, 4] - ro[:, 4]).max() / max(tscale, np.abs(ro[:, 4]).max())
    print(f"{label}: contacts {nc}, max|F| {scale:.4g}, rel err f {ef:.1e} torque {et:.1e} wall force {eo:.1e} energy {ee:.1e} M_ax {em:.1e}")
    assert scale > 0 and nc == ref["ncontacts"] and nc > 0
    assert max(ef, et, eo, ee, em) <= GATE
    assert np.abs(f.sum(axis=0) + out[:, 1:4].sum(axis=0)).max() <= GATE * scale * max(1, nc)   # momentum


@pytest.mark.parametrize("lmax,nq,nshapes,n", [(4, 10, 1, 40), (6, 16, 4, 40), (12, 32, 1, 8)])
def test_oblique_cylinder_matches_reference(oracle, lmax, nq, nshapes, n):
    """An oblique axis, exponent 1.25; the totals, M_ax among them, are the same bits with and without "deterministic"."""
    import cyl_ref as Cy
    from shpair import shapes
    shp = [(lmax, shapes.random_shape(lmax, 500 + 7 * s + lmax, amp=0.1)) for s in range(nshapes)]
    sp = ctx(shp, nq, deterministic=1)
    rs = ref_shapes(sp, shp)
    case = cyl_case(lmax + nshapes, n, nshapes, [r[2] for r in rs], OBLIQUE)
    got = run_device(sp, case, OBLIQUE, 1000.0, 1.25)
    ref = Cy.cyl_forces(rs, nq, case["x"], case["quat"], case["shtype"], [OBLIQUE], [1000.0], [1.25])
    assert ref["noutside"] == 0
    check_against_ref(got, ref, f"L={lmax} nq={nq} shapes={nshapes}")
    again = run_device(sp, case, OBLIQUE, 1000.0, 1.25)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3]))
    assert np.array_equal(sp.get_cylinders(), np.atleast_2d(OBLIQUE))
    sp.close()
    sp2 = ctx(shp, nq)
    plain = run_device(sp2, case, OBLIQUE, 1000.0, 1.25)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], plain[:3]))
    sp2.close()


@pytest.mark.parametrize("lmax", list(range(13)) + [15, 20])
def test_every_order(oracle, lmax):
    """Every compiled order 0..12 and the run-time orders 15 and 20, 8 particles, an axis along z, exponent 2."""
    import cyl_ref as Cy
    from shpair import shapes
    shp = [(lmax, shapes.random_shape(lmax, 900 + lmax, amp=0.1))]
    sp = ctx(shp, 8)
    rs = ref_shapes(sp, shp)
    cyl = np.array([0.1, 0.2, 0.0, 0.0, 0.0, 1.0, 3.0])
    case = cyl_case(100 + lmax, 8, 1, [rs[0][2]], cyl, hi=0.9)
    got = run_device(sp, case, cyl, 800.0, 2.0)
    ref = Cy.cyl_forces(rs, 8, case["x"], case["quat"], case["shtype"], [cyl], [800.0], [2.0])
    check_against_ref(got, ref, f"L={lmax}")
    sp.close()


@pytest.mark.parametrize("nq", [1, 2, 128])
def test_both_ends_of_the_nq_range(oracle, nq):
    import cyl_ref as Cy
    from shpair import shapes
    shp = [(4, shapes.random_shape(4, 77, amp=0.1))]
    sp = ctx(shp, nq)
    rs = ref_shapes(sp, shp)
    case = cyl_case(200 + nq, 4, 1, [rs[0][2]], OBLIQUE, hi=0.8)
    got = run_device(sp, case, OBLIQUE, 1000.0, 1.0)
    ref = Cy.cyl_forces(rs, nq, case["x"], case["quat"], case["shtype"], [OBLIQUE], [1000.0], [1.0])
    check_against_ref(got, ref, f"nq={nq}")
    sp.close()


def test_centre_on_the_axis_of_a_narrow_cylinder(oracle):
    """Rmax > Rc with one centre exactly on the axis: the whole sphere is the cap and the frame falls back to the e1 of
    the frame rule about the axis; a second centre off the axis takes the ordinary branch with cos alpha < 0."""
    import cyl_ref as Cy
    from shpair import shapes
    shp = [(6, shapes.random_shape(6, 3, amp=0.1))]
    sp = ctx(shp, 16)
    rs = ref_shapes(sp, shp)
    cyl = np.array([0.5, -0.25, 0.0, 0.0, 0.0, 1.0, 0.9 * rs[0][2]])
    case = dict(x=np.array([[0.5, -0.25, 2.5], [0.5 + 0.25, -0.25, -1.0]]), quat=np.array([[0.5, 0.5, -0.5, 0.5], [1.0, 0, 0, 0]]),
                shtype=np.zeros(2, np.int32), n=2)
    assert Cy.foot(case["x"][0], cyl)[1] == 0.0 and Cy.cap_cos(cyl[6], 0.0, rs[0][2]) == -1.0
    assert -1.0 < Cy.cap_cos(cyl[6], 0.25, rs[0][2]) < 0.0
    got = run_device(sp, case, cyl, 1000.0, 1.25)
    ref = Cy.cyl_forces(rs, 16, case["x"], case["quat"], case["shtype"], [cyl], [1000.0], [1.25])
    assert ref["ncontacts"] == 2
    check_against_ref(got, ref, "on the axis")
    sp.close()


def test_two_cylinders_in_reach_add_in_index_order(oracle):
    """Two parallel cylinders whose walls both reach the particles (a lens-shaped duct), different force laws: the
    reference at the gate, and bit for bit the sum of the two single-cylinder passes in index order."""
    import cyl_ref as Cy
    from shpair import shapes
    shp = [(6, shapes.random_shape(6, 5, amp=0.1))]
    sp = ctx(shp, 16)
    rs = ref_shapes(sp, shp)
    rm = rs[0][2]
    cyls = np.array([[-2.0 + 0.7 * rm, 0, 0, 0, 0, 1.0, 2.0], [2.0 - 0.7 * rm, 0, 0, 0, 0, 1.0, 2.0]])
    rng = np.random.default_rng(4)
    from shpair import bed
    n = 6
    x = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-2, 2, n)], axis=1)
    case = dict(x=x, quat=bed.random_quaternions(n, rng), shtype=np.zeros(n, np.int32), n=n)
    kn, ex = np.array([1000.0, 700.0]), np.array([1.25, 2.0])
    got = run_device(sp, case, cyls, kn, ex)
    ref = Cy.cyl_forces(rs, 16, x, case["quat"], case["shtype"], cyls, kn, ex)
    assert ref["ncontacts"] == 2 * n
    check_against_ref(got, ref, "two cylinders")
    f0, t0, _, _ = run_device(sp, case, cyls[0], kn[:1], ex[:1])
    f01, t01, _, _ = run_device(sp, case, cyls[1], kn[1:], ex[1:], f0=(f0, t0))
    assert np.array_equal(f01, got[0]) and np.array_equal(t01, got[1])
    sp.close()


def test_groupbit_masks_particles_and_the_pass_adds(oracle):
    import cyl_ref as Cy
    from shpair import shapes
    shp = [(4, shapes.random_shape(4, 11, amp=0.1))]
    sp = ctx(shp, 10)
    rs = ref_shapes(sp, shp)
    n = 40
    case = cyl_case(5, n, 1, [rs[0][2]], OBLIQUE)
    rng = np.random.default_rng(3)
    mask = np.where(rng.uniform(size=n) < 0.5, 1, 2).astype(np.int32)
    f0 = (rng.normal(size=(n, 3)), rng.normal(size=(n, 3)))
    f, tq, out, nc = run_device(sp, case, OBLIQUE, 1000.0, 1.25, mask=mask, groupbit=2, f0=f0)
    ref = Cy.cyl_forces(rs, 10, case["x"], case["quat"], case["shtype"], [OBLIQUE], [1000.0], [1.25], mask=mask, groupbit=2)
    off = mask == 1
    assert np.array_equal(f[off], f0[0][off]) and np.array_equal(tq[off], f0[1][off])   # masked rows: not a bit changed
    check_against_ref((f - f0[0], tq - f0[1], out, nc), ref, "groupbit")   # the forces are ADDED to what was there
    # no cylinder set: the call returns at once, f and torque keep their bits, and there is nothing to count
    sp.set_cylinders(None)
    assert sp.ncylinders == 0
    x, q, sh, m = dev(case["x"]), dev(case["quat"]), dev(case["shtype"]), dev(np.ones(n, dtype=np.int32))
    fd, td = dev(f0[0]), dev(f0[1])
    sp.cylinder_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), fd.data_ptr(), td.data_ptr())
    sp.synchronize()
    assert np.array_equal(fd.cpu().numpy(), f0[0]) and np.array_equal(td.cpu().numpy(), f0[1]) and sp.cylinder_stats() == 0
    sp.close()


def test_centre_outside_a_cylinder_is_an_error_and_the_rest_is_right(oracle):
    import torch
    import cyl_ref as Cy
    from shpair import shapes
    from shpair.capi import ShPairError
    shp = [(4, shapes.random_shape(4, 11, amp=0.1))]
    sp = ctx(shp, 10)
    rs = ref_shapes(sp, shp)
    n = 20
    cyl = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 3.0])
    case = cyl_case(6, n, 1, [rs[0][2]], cyl)
    case["x"][7] = [3.5, 0.0, 0.0]     # outside
    case["x"][8] = [0.0, 3.0, 0.4]     # exactly on the wall
    sp.set_cylinders([cyl], 1000.0, 1.25)
    x, q, sh, m = dev(case["x"]), dev(case["quat"]), dev(case["shtype"]), dev(np.ones(n, dtype=np.int32))
    f, tq = dev(np.zeros((n, 3))), dev(np.zeros((n, 3)))
    sp.cylinder_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    torch.cuda.synchronize()
    with pytest.raises(ShPairError, match="particle centre outside a cylinder") as e:
        sp.cylinder_stats()
    assert e.value.code == -1   # SHPAIR_EINVAL
    sp.synchronize()            # the error word was read and cleared
    ref = Cy.cyl_forces(rs, 10, case["x"], case["quat"], case["shtype"], [cyl], [1000.0], [1.25])
    assert ref["noutside"] == 2 and not ref["f"][7].any() and not ref["f"][8].any()
    scale = np.abs(ref["f"]).max()
    assert np.abs(f.cpu().numpy() - ref["f"]).max() <= GATE * scale and np.abs(tq.cpu().numpy() - ref["torque"]).max() <= GATE * scale
    sp.close()


def test_dissipative_instance_matches_reference(oracle):
    """gamma_c, mu_c, gamma_t,c and Omega != 0 with random twists: (a) one oblique cylinder, two shapes; (b) the two
    parallel cylinders of the lens-shaped duct, both in reach of every particle, with different coefficients per
    cylinder (one capped by a small mu, one viscous), so that the rows of the coefficient table are read at ncyl = 2."""
    import cyl_ref as Cy
    from shpair import shapes, bed
    from shpair.capi import ShPairError
    shp = [(6, shapes.random_shape(6, 21 + s, amp=0.1)) for s in range(2)]
    sp = ctx(shp, 16, deterministic=1)
    rs = ref_shapes(sp, shp)
    rng = np.random.default_rng(2)
    rm = max(r[2] for r in rs)
    n = 8
    duct = np.array([[-2.0 + 0.7 * rm, 0, 0, 0, 0, 1.0, 2.0], [2.0 - 0.7 * rm, 0, 0, 0, 0, 1.0, 2.0]])
    xd = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-2, 2, n)], axis=1)
    legs = [("one oblique cylinder", cyl_case(9, 24, 2, [r[2] for r in rs], OBLIQUE, hi=0.9), np.atleast_2d(OBLIQUE),
             np.array([1000.0]), np.array([1.25]), (np.array([40.0]), np.array([0.02]), np.array([900.0]), np.array([1.7]))),
            ("two cylinders", dict(x=xd, quat=bed.random_quaternions(n, rng), shtype=rng.integers(0, 2, n).astype(np.int32), n=n),
             duct, np.array([1000.0, 800.0]), np.array([1.25, 1.5]),
             (np.array([40.0, 15.0]), np.array([0.02, 0.6]), np.array([900.0, 3.0]), np.array([1.7, -0.8])))]
    for label, case, cyls, kn, ex, coef in legs:
        m = case["n"]
        tw = np.concatenate([rng.normal(size=(m, 3)), 0.5 * rng.normal(size=(m, 3))], axis=1)
        args = (rs, 16, case["x"], case["quat"], case["shtype"], cyls, kn, ex)
        got = run_device(sp, case, cyls, kn, ex, tw=tw, coef=coef)
        ref = Cy.cyl_forces(*args, tw=tw, gamma=coef[0], mu=coef[1], gt=coef[2], omega=coef[3])
        check_against_ref(got, ref, f"dissipative, {label}")
        assert ref["ncontacts"] >= len(cyls) * 8 and all(np.linalg.norm(d["Ft"]) > 0 for _, _, d in ref["contacts"])
        for c in range(len(cyls)):   # cylinder 0 is capped by its small mu, cylinder 1 stays viscous
            assert {d["capped"] for _, cc, d in ref["contacts"] if cc == c} == {c == 0}
        elastic = Cy.cyl_forces(*args)
        assert np.abs(elastic["f"] - ref["f"]).max() > 1e-3 * np.abs(ref["f"]).max()   # the coefficients did act
        still = Cy.cyl_forces(*args, tw=tw, gamma=coef[0], mu=coef[1], gt=coef[2])      # ... and so did Omega
        assert np.abs(still["f"] - ref["f"]).max() > 1e-6 * np.abs(ref["f"]).max()
        if len(cyls) == 2:   # the coefficients of the two cylinders exchanged give another answer: each row is read at its own index
            swapped = Cy.cyl_forces(*args, tw=tw, gamma=coef[0][::-1], mu=coef[1][::-1], gt=coef[2][::-1], omega=coef[3][::-1])
            assert np.abs(swapped["f"] - ref["f"]).max() > 1e-3 * np.abs(ref["f"]).max()
        with pytest.raises(ShPairError, match="null twist pointer") as e:   # a coefficient is set: the twists are needed
            run_device(sp, case, cyls, kn, ex, tw=tw, coef=coef, pass_twist=False)
        assert e.value.code == -1
    sp.close()


def test_zero_coefficients_give_the_elastic_bits_with_or_without_twists(oracle):
    from shpair import shapes
    shp = [(6, shapes.random_shape(6, 21, amp=0.1))]
    sp = ctx(shp, 16)
    rm = sp.rmax(0)
    case = cyl_case(12, 16, 1, [rm], OBLIQUE)
    tw = np.random.default_rng(1).normal(size=(16, 6))
    zero = (0.0, 0.0, 0.0, 0.0)
    a = run_device(sp, case, OBLIQUE, 1000.0, 1.25)
    b = run_device(sp, case, OBLIQUE, 1000.0, 1.25, tw=tw, coef=zero)
    c = run_device(sp, case, OBLIQUE, 1000.0, 1.25, tw=tw, coef=zero, pass_twist=False)
    d = run_device(sp, case, OBLIQUE, 1000.0, 1.25, tw=tw, coef=(0.0, 0.5, 0.0, 2.0))   # a mu without a gamma_t, a rotation: no coefficient
    assert a[3] > 0
    for other in (b, c, d):
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], other[:3]))
    sp.close()


def test_refusals_with_the_ledger_and_the_loop_over_ranks(oracle):
    from shpair import shapes
    from shpair.capi import ShPairError
    sp = ctx([(0, shapes.sphere(1.0))], 8)
    sp.set_cylinders([OBLIQUE], 1000.0, 1.25)
    sp.set_energy_ledger(True)            # an elastic cylinder dissipates nothing: allowed
    with pytest.raises(ShPairError, match="energy ledger is on") as e:
        sp.cylinder_damping(2.0)
    assert e.value.code == -4 and not sp.cylinder_reads_twists   # SHPAIR_ESTATE, and the state stays what it was
    with pytest.raises(ShPairError, match="energy ledger is on"):
        sp.cylinder_friction(0.5, 2.0)
    sp.cylinder_friction(0.5, 0.0)        # no coefficient: fine
    sp.set_energy_ledger(False)
    sp.cylinder_damping(2.0)
    with pytest.raises(ShPairError, match="cylinder damping or friction coefficient is set") as e:
        sp.set_energy_ledger(True)
    assert e.value.code == -4 and not sp.ledger_on
    # argument checks, as for the planes
    ok = OBLIQUE.tolist()
    for cyls, kn, ex in (([ok[:3] + [0, 0, 1.0 + 1e-9] + [2.0]], 1.0, 1.0), ([ok[:6] + [0.0]], 1.0, 1.0), ([ok[:6] + [-1.0]], 1.0, 1.0),
                         ([ok[:6] + [np.nan]], 1.0, 1.0), ([[np.inf] + ok[1:]], 1.0, 1.0), ([ok], -1.0, 1.0), ([ok], 1.0, 0.5),
                         ([ok], np.nan, 1.0), ([ok] * 9, 1.0, 1.0)):
        with pytest.raises(ShPairError) as e:
            sp.set_cylinders(cyls, kn, ex)
        assert e.value.code == -1
    assert sp.ncylinders == 1 and sp.cylinder_reads_twists   # a refused call changes nothing
    for bad in ((-1.0,), (np.nan,), (1.0, 2.0)):
        with pytest.raises(ShPairError) as e:
            sp.cylinder_damping(np.array(bad))
        assert e.value.code == -1
    with pytest.raises(ShPairError):
        sp.cylinder_rotation(np.inf)
    sp.set_cylinders([ok] * 8, 1.0, 1.0)
    assert sp.ncylinders == 8 and not sp.cylinder_reads_twists
    # the loop over several ranks, and its Python driver: refused while a cylinder is set, elastic or not
    from shpair import mrank
    from shpair.capi import HaloArrays, HaloRunParams
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    stand_in = type("R", (), dict(sp=sp, a=None, stream=None, halo=None))()
    with pytest.raises(ShPairError, match="cylindrical walls are single-rank") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -4
    with pytest.raises(ShPairError, match="cylindrical walls are single-rank") as e:
        mrank.RankRun.force(stand_in)
    assert e.value.code == -4
    sp.set_cylinders(None)                # the cause removed: both get past the refusal (and stop at the empty arguments)
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
def test_run_loops_with_a_cylinder_are_bitwise_identical(oracle, dissipative):
    """shstep_run_device plain, with hipGraph replay, and the call-by-call Python loop: the same bits over 20 steps, for
    the elastic instance and for the dissipative one with a rotating drum; and the cylinder did act."""
    import torch
    from shpair import shapes, bed
    from shpair.run import DeviceRun
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    rng = np.random.default_rng(12)
    # a horizontal drum along y in the box [0, 8]^3, four columns of four particles, each column 0.9 Rmax from the wall
    g = np.array([-0.95, 0.95])
    cyl = np.array([4.0, 4.0, 4.0, 0.0, 1.0, 0.0, np.hypot(0.95, 0.95) + 0.9 * oracle.shape_rmax(4, shp[0][1])])
    x = np.stack(np.meshgrid(g, np.arange(4) * 1.9 - 2.85, g, indexing="ij"), axis=-1).reshape(-1, 3) + [4.0, 4.0, 4.0]
    x += rng.uniform(-0.05, 0.05, x.shape)
    quat, sht = bed.random_quaternions(x.shape[0], rng), np.zeros(x.shape[0], np.int32)
    extra = dict(cylinder_damping=20.0, cylinder_friction=(0.4, 30.0), cylinder_rotation=0.8) if dissipative else {}

    def go(mode, cylinders):
        sp = ctx(shp, 10, kn=2000.0, deterministic=1)
        r = DeviceRun(sp, x, quat, sht, (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, dt=5e-4, gravity=(0.0, 0.0, -9.81), gamma_t=0.2,
                      gamma_r=0.1, cylinders=cylinders, **(extra if cylinders else {}))
        if mode == "python":
            r.run(20)
        else:
            r.run_native(20, use_graph=(mode == "graph"))
        torch.cuda.synchronize()
        st, nc = _state(r), sp.cylinder_stats()
        sp.close()
        return st, nc
    ref, nc = go("python", ([cyl], 2000.0, 1.25))
    assert nc > 0
    for mode in ("plain", "graph"):
        got, nc2 = go(mode, ([cyl], 2000.0, 1.25))
        assert nc2 == nc
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), mode
    never, _ = go("graph", None)
    assert not np.array_equal(never[0], ref[0])


def _rest_depth(Cy, cyl, kn, m, weight, nq):
    """h* of a unit sphere (Rmax 1.01) with kn m V^(m-1) |S_n| = weight, by bisection on the reference."""
    from shpair import shapes
    a = shapes.sphere(1.0)

    def force(h):
        x = cyl[:3] + (cyl[6] - h) * np.array([0.0, 0.0, -1.0])
        V, S, T, _ = Cy.cyl_sums(0, a, 1.01, x, (1, 0, 0, 0), cyl, nq)
        return kn * m * V ** (m - 1) * np.linalg.norm(S) if V > 0 else 0.0
    lo, hi = 0.9, 1.0
    assert force(lo) > weight > force(hi)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if force(mid) > weight else (lo, mid)
    return 0.5 * (lo + hi)


def test_sphere_rests_at_the_depth_of_the_force_balance_and_a_drum_drags_it(oracle):
    """A unit sphere dropped inside a horizontal cylinder (axis x, gravity -z) with gamma_c comes to rest with d = Rc - h*,
    kn m V^(m-1) |S_n| = m g at h* from the reference.  Tolerance: the sharp rule makes S_n a step function of h with
    steps of up to 1.1e-2 |S_n| for a unit sphere (SPEC §2.9), the force goes as (1 - h)^1.5, so the balance is uncertain
    by 0.8e-2 (1 - h*); the bar is 2e-2 (1 - h*).
    With Omega > 0, friction and a drag on the sphere's spin and velocity (without the first it would end rolling without
    slip at the bottom, without the second it swings for seconds) the same sphere ends displaced from the bottom in the direction of the wall's motion there, +y, and the moment M_ax of the
    particle's force on the wall opposes Omega."""
    import torch
    import cyl_ref as Cy
    from shpair import shapes
    from shpair.run import DeviceRun
    Rc, kn, m, nq = 3.0, 1e4, 1.25, 32
    cyl = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, Rc])
    res = {}
    for label, extra in (("rest", {}), ("drum", dict(cylinder_friction=(0.5, 50.0), cylinder_rotation=2.0))):
        sp = ctx([(0, shapes.sphere(1.0))], nq, kn=kn, expo=m, rmax=[1.01])
        mass = sp.body(0)[0]
        r = DeviceRun(sp, np.array([[0.0, 0.0, -(Rc - 1.05)]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-5, -5, -5),
                      (5, 5, 5), (0, 0, 0), 0.5, dt=1e-4, gravity=(0.0, 0.0, -9.81), gamma_t=40.0 if extra else 0.0, gamma_r=5.0 if extra else 0.0,
                      cylinders=([cyl], kn, m), cylinder_damping=3e5, check=False, **extra)
        r.run_native(12000, use_graph=True)
        out = torch.zeros(1, 5, dtype=torch.float64, device="cuda:0")
        f, tq = torch.zeros_like(r.f), torch.zeros_like(r.tq)
        sp.twist_device(1, 0, r.v.data_ptr(), r.q.data_ptr(), r.L.data_ptr(), r.sh.data_ptr(), r.twist.data_ptr())
        sp.cylinder_force_device(1, r.x.data_ptr(), r.q.data_ptr(), r.sh.data_ptr(), r.mask.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                 twist=r.twist.data_ptr(), cyl_out=out.data_ptr())
        torch.cuda.synchronize()
        sp.synchronize()   # no error bit
        res[label] = (r.x[0].cpu().numpy().copy(), r.v[0].cpu().numpy().copy(), out.cpu().numpy()[0], mass)
        sp.close()
    x, v, out, mass = res["rest"]
    hstar = _rest_depth(Cy, cyl, kn, m, mass * 9.81, nq)
    d = np.hypot(x[1], x[2])
    print(f"rest: d {d:.6f}, Rc - h* {Rc - hstar:.6f} (h* {hstar:.6f}), |v| {np.linalg.norm(v):.1e}, wall force z {out[3]:.4f}, weight {mass * 9.81:.4f}")
    assert abs(d - (Rc - hstar)) <= 2e-2 * (1.0 - hstar) and np.linalg.norm(v) <= 1e-3 and abs(x[1]) <= 1e-9
    x, v, out, mass = res["drum"]
    print(f"drum: y {x[1]:.5f}, z {x[2]:.5f}, M_ax {out[4]:.4f}")
    assert x[1] > 1e-4 and out[4] < 0.0
