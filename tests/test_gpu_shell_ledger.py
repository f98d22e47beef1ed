"""GPU tests of the cylinder entries of the energy ledger, docs/SPEC.md §2.20 (the cyl_power_* kernels of
csrc/cyl_power_kernels.hpp through the C ABI of include/shstep.h), against tests/shell_ledger_ref.py.  The gate is
tests/test_gpu_cylinder.py's, 1e-9 of the scale (the largest reference power row, the largest reference total): a power is
a bilinear form of the integrals the force is held to at that gate.  Beds of at most 16 particles, L <= 6, n_q 8 and 16."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dissipation_common import _wall_ctx as ctx, dev  # noqa: E402
from test_gpu_cylinder import GATE  # noqa: E402

KN, EXPO, DT, NPASS = 1000.0, 1.25, 2e-3, 3


def geometry(name, rmax):
    """cyls, gamma, mu, gamma_t, k_t, Omega per cylinder of a named case (the geometries of tests/cyl_history_cases.py)."""
    import cyl_history_cases as K
    ob = K.OBLIQUE
    e1, _ = K._perp(ob[3:6])
    second = np.array([*(ob[:3] + 0.12 * e1), *ob[3:6], 4.1])
    third = np.array([*(ob[:3] - 0.05 * e1), *ob[3:6], 4.05])
    if name == "dissipative":    # §2.18 alone: cyl_power_dissipative_kernel; a small mu, so that both branches of the cap occur
        return np.array([ob]), [3.0], [0.05], [30.0], [0.0], [0.7]
    if name == "history":        # §2.19: cyl_power_spring_kernel
        return np.array([ob]), [3.0], [0.5], [2.0], [4e3], [0.7]
    if name == "mixed":          # a history cylinder, a dissipative one and an elastic one, all in reach of most particles
        return np.array([ob, second, third]), [3.0, 5.0, 0.0], [0.5, 0.4, 0.0], [0.0, 30.0, 0.0], [4e3, 0.0, 0.0], [0.6, -0.5, 0.0]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, lmax, nq):
    """The prescribed inputs of NPASS advancing passes and the reference's trajectory through them, computed once."""
    import cyl_history_cases as K
    import shell_ledger_ref as SL
    from oracle import oracle as O
    from shpair import bed, shapes
    anm = shapes.random_shape(lmax, 40 + lmax, amp=0.1)
    rmax = O.shape_rmax(lmax, anm)
    cyls, gamma, mu, gt, kt, om = geometry(name, rmax)
    rng = np.random.default_rng(100 * lmax + nq + len(name))
    n = 14
    x0 = K._ring(rng, n, rmax, K.OBLIQUE, 0.5, 0.85)
    quat = bed.random_quaternions(n, rng)
    scale = 10.0 ** rng.uniform(-2.0, 1.0, n)
    mask = np.ones(n, np.int32)
    mask[[3, 9]] = 2                              # two particles outside the group
    xs, tws, refs = [], [], []
    xi, live = np.zeros((n, len(cyls), 2)), np.zeros((n, len(cyls)), bool)
    for k in range(NPASS):
        xs.append(x0 + DT * k * 0.05 * rng.normal(size=(n, 3)))
        tws.append(rng.normal(size=(n, 6)) * scale[:, None])
        r = SL.shell_pass([(lmax, anm, rmax)], nq, xs[k], quat, np.zeros(n, np.int32), tws[k], cyls, KN, EXPO, gamma, mu, gt, om, kt, xi,
                          live, DT, mask=mask)
        xi, live = r["xi"], r["live"]
        refs.append(r)
    return dict(name=name, lmax=lmax, nq=nq, anm=anm, rmax=rmax, cyls=cyls, gamma=gamma, mu=mu, gt=gt, kt=kt, om=om, n=n, quat=quat,
                mask=mask, xs=xs, tws=tws, refs=refs)


def make(c, ledger, det=0, ledger_first=False):
    """A context with the case's cylinders; ledger: both ledgers on, in either order around the coefficients."""
    sp = ctx([(c["lmax"], c["anm"])], c["nq"], deterministic=det)
    if ledger:
        sp.set_shell_ledger(True)
        if ledger_first:
            sp.set_energy_ledger(True)
    sp.set_cylinders(c["cyls"], KN, EXPO)
    sp.cylinder_damping(c["gamma"])
    sp.cylinder_friction(c["mu"], c["gt"])
    if any(c["kt"]):
        sp.set_cyl_tangential_spring(c["kt"])
    sp.cylinder_rotation(c["om"])
    if ledger and not ledger_first:
        sp.set_energy_ledger(True)
    return sp


def passes(c, ledger, det=0, ledger_first=False):
    """The NPASS advancing passes on the device: per pass (f, torque, cyl_out, xi or None, per_cylinder, totals)."""
    from test_gpu_cyl_history import Pass
    sp = make(c, ledger, det, ledger_first)
    P = Pass(sp, c["n"])
    out = []
    for k in range(NPASS):
        if ledger:
            sp.reset_energy_ledger()
        f, tq, co = P.go(c["xs"][k], c["quat"], c["tws"][k], DT, mask=c["mask"])
        xi = sp.cyl_history(c["n"]) if sp.has_cyl_history else None
        tot = per = None
        if ledger:
            sp.ledger_fold_device(DT)
            tot, per = sp.shell_ledger()
            sp.ledger_fold_device(DT)              # nothing fresh: the fold runs once per pass
            tot2, per2 = sp.shell_ledger()
            assert np.array_equal(tot, tot2) and np.array_equal(per, per2)
        out.append((f, tq, co, xi, per, tot))
    return sp, P, out


CASES = [("dissipative", 6, 16), ("history", 4, 8), ("mixed", 6, 16), ("mixed", 4, 8)]


@pytest.mark.parametrize("name,lmax,nq", CASES)
def test_rows_and_totals_match_the_reference_and_the_pass_keeps_its_bits(oracle, name, lmax, nq):
    """Three advancing passes with a group mask: the per-cylinder entries and the totals of every pass against the reference
    at the gate; f, torque, cyl_out, xi and the live words (the zero pattern of the history's copy) bit for bit those of the
    same passes with both ledgers off; the same ledger bits with "deterministic" and with the energy ledger switched on
    ahead of the coefficients; then the rows of single particles, one of them in reach of two cylinders, by looks (dt = 0)
    through a one-particle group."""
    import shell_ledger_ref as SL
    c = case(name, lmax, nq)
    if any(c["kt"]):
        assert np.abs(np.concatenate([r["ratios"] for r in c["refs"]]) - 1).min() > 1e-6   # no contact sits on the cap
    sp, P, got = passes(c, True)
    sp0, _, plain = passes(c, False)
    sp0.close()
    sp1, _, det = passes(c, True, det=1, ledger_first=True)
    sp1.close()
    nhit = 0
    for k in range(NPASS):
        ref = c["refs"][k]
        per, tot = SL.shell_fold(ref["P"], DT)
        scale = np.abs(per).max()
        e_per, e_tot = np.abs(got[k][4] - per).max() / scale, np.abs(got[k][5] - tot).max() / scale
        print(f"{name} L={lmax} nq={nq} pass {k}: contacts {ref['ncontacts']}, per-cylinder {per.tolist()}, rel err {e_per:.1e} totals {e_tot:.1e}")
        assert ref["ncontacts"] > 0 and sp.cylinder_stats() > 0 and (np.abs(per).max(axis=0) > 0).all()
        assert max(e_per, e_tot) <= GATE
        assert np.abs(got[k][0] - ref["f"]).max() <= GATE * np.abs(ref["f"]).max()
        for a, b in zip(got[k][:4], plain[k][:4]):          # the LEDGER instance changes no other output
            assert (a is None and b is None) or np.array_equal(a, b)
        assert np.array_equal(got[k][4], det[k][4]) and np.array_equal(got[k][5], det[k][5])
        nhit += int((np.abs(ref["P"]).sum(axis=2) > 0).sum(axis=1).max() >= 2)
    if name == "mixed":
        assert nhit == NPASS and not got[-1][4][2].any()     # a particle dissipates at two cylinders; the elastic one has no entry
    # rows: a look at the last pass' inputs through a one-particle group, folded with dt = 1
    ref = c["refs"][-1]
    both = np.argsort(-(np.abs(ref["P"]).sum(axis=2) > 0).sum(axis=1), kind="stable")[:3]
    scale = np.abs(ref["P"]).max()
    xi, live = c["refs"][-1]["xi"], c["refs"][-1]["live"]
    for i in list(both) + [3]:                               # ... and a particle the advancing passes' group left out
        m = np.full(c["n"], 2, np.int32)
        m[i] = 1
        look = SL.shell_pass([(lmax, c["anm"], c["rmax"])], nq, c["xs"][-1], c["quat"], np.zeros(c["n"], np.int32), c["tws"][-1], c["cyls"],
                             KN, EXPO, c["gamma"], c["mu"], c["gt"], c["om"], c["kt"], xi, live, 0.0, mask=m)
        sp.reset_energy_ledger()
        P.go(c["xs"][-1], c["quat"], c["tws"][-1], 0.0, mask=m)
        sp.ledger_fold_device(1.0)
        tot, per = sp.shell_ledger()
        err = np.abs(per - look["P"][i]).max() / scale
        print(f"  row of particle {i}: {per.tolist()} rel err {err:.1e}")
        assert err <= GATE and np.array_equal(look["P"].sum(axis=0), look["P"][i])
    sp.close()


# ---- the run loops ---------------------------------------------------------------------------------------------------

def _drum(mode, det=1, nsteps=200, spring=True):
    """tests/test_gpu_cylinder.py's drum (a horizontal cylinder along y, four columns of four L = 4 particles, gravity) with
    pair damping, gamma_c, friction, springs and Omega = 0.8, both ledgers on."""
    import torch
    from shpair import shapes, bed
    from shpair.run import DeviceRun
    from oracle import oracle as O
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    rng = np.random.default_rng(12)
    g = np.array([-0.95, 0.95])
    cyl = np.array([4.0, 4.0, 4.0, 0.0, 1.0, 0.0, np.hypot(0.95, 0.95) + 0.9 * O.shape_rmax(4, shp[0][1])])
    x = np.stack(np.meshgrid(g, np.arange(4) * 1.9 - 2.85, g, indexing="ij"), axis=-1).reshape(-1, 3) + [4.0, 4.0, 4.0]
    x += rng.uniform(-0.05, 0.05, x.shape)
    quat, sht = bed.random_quaternions(x.shape[0], rng), np.zeros(x.shape[0], np.int32)
    sp = ctx(shp, 8, kn=2000.0, deterministic=det)
    extra = dict(cylinder_spring=3e3) if spring else {}
    r = DeviceRun(sp, x, quat, sht, (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, dt=5e-4, gravity=(0.0, 0.0, -9.81), gamma_t=0.2, gamma_r=0.1,
                  ledger=True, shell_ledger=True, cylinders=([cyl], 2000.0, 1.25), cylinder_damping=20.0, cylinder_friction=(0.4, 30.0),
                  cylinder_rotation=0.8, pair_damping={(1, 1): 40.0}, **extra)
    r.v[:] = dev(rng.normal(size=x.shape) * 0.5)
    r.force()
    if mode == "python":
        r.run(nsteps)
    else:
        r.run_native(nsteps, use_graph=(mode == "graph"))
    torch.cuda.synchronize()
    return sp, r, cyl


@pytest.mark.parametrize("spring", [True, False])
def test_the_loops_give_the_same_ledger_bits_and_the_setters_zero_what_they_should(oracle, spring):
    """200 steps of a rotating drum with "deterministic": the Python driver, plain launches and graph replay leave the same
    bits in the shell ledger and in the energy ledger.  (Without the option the PAIR forces of a particle with several
    contacts are added in an order that varies, and the trajectory of this bed with them; the fold itself has no atomics.
    The two settings are compared bit for bit on prescribed inputs in the test above, and over 600 steps on the thrown
    sphere below, which has no pair contact.)  Then shstep_set_cylinders zeroes the shell entries and keeps the pair entries,
    and shstep_reset_energy_ledger zeroes both."""
    sp, r, cyl = _drum("python", spring=spring)
    ref, led = r.shell_ledger(), r.ledger()
    print(f"spring {spring}: shell ledger {ref}, pair damping {led['pair_damping']:.6g}, cylinder contacts {sp.cylinder_stats()}")
    assert ref["damping"] > 0 and ref["work"] != 0 and ref["friction"] != 0 and led["pair_damping"] > 0
    assert np.array_equal(ref["per_cylinder"][0], [ref["damping"], ref["friction"], ref["work"]])
    for mode, det in (("plain", 1), ("graph", 1)):
        sp2, r2, _ = _drum(mode, det=det, spring=spring)
        got, led2 = r2.shell_ledger(), r2.ledger()
        sp2.close()
        for k in ("damping", "friction", "work"):
            assert got[k] == ref[k], (mode, det, k)
        assert np.array_equal(got["per_cylinder"], ref["per_cylinder"])
        if det:
            assert led2["pair_damping"] == led["pair_damping"]
    sp.set_cylinders([cyl], 2000.0, 1.25)
    tot, per = sp.shell_ledger()
    assert not tot.any() and not per.any() and r.ledger()["pair_damping"] == led["pair_damping"]
    r.run_native(5, use_graph=True)                        # elastic now: nothing is added
    assert not sp.shell_ledger()[0].any() and r.ledger()["pair_damping"] >= led["pair_damping"]
    sp.cylinder_damping(20.0)                              # both ledgers on: allowed
    r.run_native(5, use_graph=True)
    assert sp.shell_ledger()[0][0] > 0
    sp.reset_energy_ledger()
    assert not sp.shell_ledger()[0].any() and not sp.shell_ledger()[1].any() and not sp.energy_ledger()[0].any()
    sp.close()


def _throw(k, elastic, det=1):
    """tests/shell_ledger_ref.py's THROW through shstep_run_device with graph replay at dt / k."""
    import torch
    from shell_ledger_ref import THROW as c
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = ctx([(0, shapes.sphere(1.0))], c["nq"], kn=c["kn"], expo=c["m"], rmax=[1.01], deterministic=det)
    extra = {} if elastic else dict(cylinder_damping=c["gamma"], cylinder_friction=(c["mu"], c["gt"]))
    r = DeviceRun(sp, np.array([c["x0"]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.5,
                  dt=c["dt"] / k, ledger=True, shell_ledger=True, cylinders=([np.array(c["cyl"])], c["kn"], c["m"]),
                  cylinder_rotation=c["omega"], check=False, **extra)
    mass, _, inertia = sp.body(0)
    r.v[:] = dev(np.array([c["v0"]]))
    r.L[:] = dev(np.array([c["w0"]]) * inertia[0])
    r.force()
    e0 = r.energies()
    Ds = [0.0]
    for _ in range(6):
        r.run_native(c["nsteps"] * k // 6, use_graph=True)
        s = r.shell_ledger()
        Ds.append(s["damping"])
    torch.cuda.synchronize()
    e1, led, wall = r.energies(), r.shell_ledger(), r.ledger()
    d = float(np.hypot(r.x[0, 0].item() - 4.0, r.x[0, 2].item() - 4.0))
    sp.synchronize()
    sp.close()
    assert not any(wall[t] for t in ("pair_damping", "pair_friction", "wall_damping", "wall_friction", "wall_work"))
    return e0[1] + e0[2], e1[1] + e1[2], led, c["Rc"] - d, np.array(Ds)


def test_the_balance_of_a_thrown_sphere_closes_to_first_order_in_dt(oracle):
    """The inputs are tests/test_shell_ledger_ref.py's, chosen there on the reference's own sharp-rule sums (which predict
    R = 6.845e-2 / 3.360e-2, ratio 0.491, elastic R0 = 2.1e-3 / 5.6e-5 for this run); the two inequalities are
    tests/test_gpu_ledger.py's for the planar collision.  The 600 steps at dt leave the same ledger bits with and without
    "deterministic"."""
    R, R0, leds = [], [], []
    for k in (1, 2):
        E0, E1, led, h, Ds = _throw(k, False)
        e0, e1, led0, h0, _ = _throw(k, True)
        leds.append(led)
        R.append(abs(E1 - E0 - (led["work"] - led["damping"] - led["friction"])))
        R0.append(abs(e1 - e0))
        print(f"dt/{k}: E0 {E0:.6f} E1 {E1:.6f} D_d {led['damping']:.6f} D_f {led['friction']:.6f} W {led['work']:.6f} R {R[-1]:.3e} "
              f"elastic R0 {R0[-1]:.3e}, final h {h:.3f}")
        assert h > 1.01 and h0 > 1.01 and abs(E1 - E0) > 0.5             # it met the wall and parted
        assert led["damping"] > 0 and led["friction"] > 0 and led["work"] > 0 and (np.diff(Ds) >= 0).all()
        assert not any(led0[t] for t in ("damping", "friction", "work"))  # an elastic shell has no entries
    print(f"R(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert R0[0] <= 0.1 * R[0] and R0[1] <= 0.1 * R[1]
    assert R[1] <= 0.75 * R[0]
    atomic = _throw(1, False, det=0)[2]
    assert all(atomic[t] == leds[0][t] for t in ("damping", "friction", "work")) and np.array_equal(atomic["per_cylinder"], leds[0]["per_cylinder"])


# ---- the switch ------------------------------------------------------------------------------------------------------

def test_the_switch_lifts_the_refusals_and_off_they_are_what_they_were(oracle):
    from shpair import shapes
    from shpair.capi import ShPairError
    from test_gpu_cylinder import OBLIQUE
    sp = ctx([(0, shapes.sphere(1.0))], 8)
    with pytest.raises(ShPairError, match="never switched on") as e:
        sp.shell_ledger()
    assert e.value.code == -4
    sp.set_cylinders([OBLIQUE], 1000.0, 1.25)
    # off (the default): both refusals, their codes and their words
    sp.set_energy_ledger(True)
    with pytest.raises(ShPairError, match="energy ledger is on and keeps no cylinder entries") as e:
        sp.cylinder_damping(2.0)
    assert e.value.code == -4 and not sp.cylinder_reads_twists and not sp.shell_ledger_on
    sp.cylinder_friction(0.5, 0.0)
    with pytest.raises(ShPairError, match="energy ledger is on and keeps no cylinder entries") as e:
        sp.set_cyl_tangential_spring(4e3)
    assert e.value.code == -4
    sp.set_energy_ledger(False)
    sp.cylinder_damping(2.0)
    with pytest.raises(ShPairError, match="cylinder damping or friction coefficient is set and the ledger keeps no cylinder") as e:
        sp.set_energy_ledger(True)
    assert e.value.code == -4 and not sp.ledger_on
    sp.set_cyl_tangential_spring(4e3)
    with pytest.raises(ShPairError, match="cylinder tangential spring is set and the ledger keeps no cylinder") as e:
        sp.set_energy_ledger(True)
    assert e.value.code == -4 and not sp.ledger_on
    # on: the ledger behind the coefficients ...
    sp.set_shell_ledger(True)
    assert sp.shell_ledger_on
    sp.set_energy_ledger(True)
    tot, per = sp.shell_ledger()
    assert tot.shape == (3,) and per.shape == (1, 3) and not tot.any() and not per.any()
    with pytest.raises(ShPairError, match="energy ledger is on and a cylinder coefficient") as e:   # off would recreate the refused state
        sp.set_shell_ledger(False)
    assert e.value.code == -4 and sp.shell_ledger_on
    # ... and the coefficients behind the ledger
    sp.set_cylinders([OBLIQUE, OBLIQUE], 1000.0, 1.25)
    sp.cylinder_damping(2.0)
    sp.cylinder_friction(0.5, 2.0)
    sp.set_cyl_tangential_spring([4e3, 0.0])
    assert sp.cylinder_reads_twists and sp.has_cyl_history and sp.ledger_on
    dp = ctypes.POINTER(ctypes.c_double)
    assert sp._lib.shstep_get_shell_ledger(sp._h, tot.ctypes.data_as(dp), 1, per.ctypes.data_as(dp)) == -1   # a count mismatch
    assert sp._lib.shstep_get_shell_ledger(sp._h, tot.ctypes.data_as(dp), 1, None) == 0                      # no per-shell room asked for
    sp.set_energy_ledger(False)
    sp.set_shell_ledger(False)          # allowed now, and the refusals are back
    with pytest.raises(ShPairError, match="cylinder tangential spring is set"):
        sp.set_energy_ledger(True)
    assert not sp.shell_ledger()[0].any()   # nothing is freed: the accumulator can still be read
    sp.close()
