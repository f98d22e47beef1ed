"""GPU tests of the tangential springs with history at the cones of docs/SPEC.md §2.23 (conic_spring_kernel and
conic_live_sweep_kernel of csrc/cone_kernels.hpp through the C ABI of include/shstep.h) against
tests/conic_history_ref.py.  The gate is tests/test_gpu_cone.py's, 1e-9 of the largest reference force (SPEC §4), for
(xi_g, xi_theta) 1e-9 of the largest reference |xi| and for phi_c 1e-9 rad.  Every test uses at most 40 particles."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dissipation_common import _wall_ctx as ctx, dev  # noqa: E402

GATE = 1e-9


class Pass:
    """Device arrays of one particle set and the two cone calls on them."""

    def __init__(self, sp, n, shtype=None):
        self.sp, self.n = sp, n
        self.sh = dev(np.zeros(n, np.int32) if shtype is None else np.asarray(shtype, np.int32))
        self.nk = sp.ncones

    def go(self, x, quat, tw, dt, mask=None, old_call=False, want_out=True):
        import torch
        n = self.n
        xd, qd, twd = dev(x), dev(quat), dev(tw)
        m = dev(np.ones(n, np.int32) if mask is None else np.asarray(mask).astype(np.int32))
        f, tq = (torch.zeros(n, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
        out = torch.zeros(self.nk, 5, dtype=torch.float64, device="cuda:0")
        args = (n, xd.data_ptr(), qd.data_ptr(), self.sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
        if old_call:
            self.sp.cone_force_device(*args, twist=twd.data_ptr(), cone_out=out.data_ptr() if want_out else None)
        else:
            self.sp.conic_contact_device(*args, twd.data_ptr(), dt, cone_out=out.data_ptr() if want_out else None)
        torch.cuda.synchronize()
        return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy()


def errors(got, ref, xi=None):
    f, tq, out = got
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ro = ref["cone_out"]
    e = dict(f=np.abs(f - ref["f"]).max() / scale, torque=np.abs(tq - ref["torque"]).max() / tscale,
             wall=np.abs(out[:, 1:4] - ro[:, 1:4]).max() / np.abs(ro[:, 1:4]).max(),
             energy=np.abs(out[:, 0] - ro[:, 0]).max() / np.abs(ro[:, 0]).max(),
             M_ax=np.abs(out[:, 4] - ro[:, 4]).max() / max(tscale, np.abs(ro[:, 4]).max()))
    if xi is not None:
        e["xi"] = np.abs(xi[..., :2] - ref["xi"][..., :2]).max() / np.abs(ref["xi"][..., :2]).max()
        e["phi"] = np.abs(xi[..., 2] - ref["xi"][..., 2]).max()
    return e


def live_bytes(xi):
    """The live word of every particle as the boundary shows it: bit k where a number of (particle, cone k) is not 0."""
    return (xi != 0).any(axis=2) @ (1 << np.arange(xi.shape[1]))


def setup(sp, cones, mu, gt, kt, om, gamma=3.0, kn=1000.0, expo=1.25, spring_first=False):
    sp.set_cones(cones, kn, expo)
    sp.cone_damping(gamma)
    if spring_first:   # the two setters give the same state in either order
        sp.conic_spring(kt)
        sp.cone_friction(mu, gt)
    else:
        sp.cone_friction(mu, gt)
        sp.conic_spring(kt)
    sp.cone_rotation(om)


def _shapes(oracle):
    from shpair import shapes
    return [(0, shapes.sphere(1.0)), (6, shapes.random_shape(6, 3, amp=0.1))]


def test_a_sphere_and_a_rough_shape_stick_then_slide_like_the_reference(oracle):
    """Two particles against one oblique 30-degree cone that turns, six advancing passes on a path that carries both
    round the axis and across the cut of the azimuth; the device carries (xi_g, xi_theta, phi_c) on its side, the reference
    on its own."""
    import cone_ref as Co
    import conic_history_cases as K
    import conic_history_ref as CH
    shp = _shapes(oracle)
    sp = ctx(shp, 16, rmax=[1.01, 0.0])
    shapes3 = [(l, a, sp.rmax(s)) for s, (l, a) in enumerate(shp)]
    co = Co.cone(K.APEX, K.AXIS, np.pi / 6)
    mu, gt, kt, om, dt, npass = 0.5, 2.0, 4e3, 1.7, 0.01, 6
    setup(sp, [co], mu, gt, kt, om, spring_first=True)
    assert sp.has_conic_history and sp.cone_reads_twists
    P = Pass(sp, 2, shtype=[0, 1])
    quat = np.stack([[1.0, 0, 0, 0], K.unit([0.5, -0.3, 0.7, 0.4])])
    xi, live = np.zeros((2, 1, 3)), np.zeros((2, 1), bool)
    kinds = [set(), set()]
    for k in range(npass):
        x = np.stack([K.centre(co, np.pi - 0.3 + 0.125 * k, 6.0 + 0.1 * k, 0.7 * shapes3[0][2]),
                      K.centre(co, 0.4 + 0.125 * k, 9.0 + 0.1 * k, 0.7 * shapes3[1][2])])
        tw = np.stack([(1 + 0.1 * k) * np.array([0.3, -0.2, 0.1, 0.5 * np.cos(0.3 * k), 0.4, -0.6 * np.sin(0.3 * k) - 0.6]),
                       (1 + 0.1 * k) * np.array([-0.2, 0.3, 0.15, 0.4, -0.5 * np.cos(0.3 * k), 0.3])])
        ref = CH.cone_forces_history(shapes3, 16, x, quat, [0, 1], tw, [co], 1000.0, 1.25, 3.0, mu, gt, om, kt, xi, live, dt)
        xi, live = ref["xi"], ref["live"]
        got = P.go(x, quat, tw, dt)
        held = sp.conic_history(2)
        e = errors(got, ref, held)
        for i in range(2):
            kinds[i].add(ref["kind"][i, 0])
        print(f"pass {k}: kinds {list(ref['kind'][:, 0])}, contacts {sp.cone_stats()}, " + " ".join(f"{a} {b:.1e}" for a, b in e.items()))
        assert sp.cone_stats() == ref["ncontacts"] == 2
        assert np.array_equal(live_bytes(held), live_bytes(ref["xi"])) and live.all()
        assert max(e.values()) <= GATE
    assert kinds[0] == kinds[1] == {CH.STICK, CH.SLIDE}
    sp.close()


@functools.lru_cache(maxsize=None)
def _crowd():
    """40 particles of two L = 4 shapes near the walls of 8 cones that share a region: one axis, apexes and half-angles a
    little apart, so that most particles reach several cones and every mask bit is used.  Cones 0, 2, 3, 6 have history
    (3 with gamma_t = 0), 1 and 5 plain friction, 4 a k_t without a mu, 7 nothing.  Two advancing passes and a look of the
    reference, computed once."""
    import cone_ref as Co
    import conic_history_cases as K
    import conic_history_ref as CH
    from oracle import oracle as O
    from shpair import shapes, bed
    nq, n, nk, dt = 6, 40, 8, 5e-3
    shp = [(4, shapes.random_shape(4, 21, amp=0.15)), (4, shapes.random_shape(4, 22, amp=0.1))]
    shapes3 = [(l, a, O.shape_rmax(l, a)) for l, a in shp]
    rng = np.random.default_rng(31)
    cones = np.stack([Co.cone(K.APEX - 0.04 * k * K.AXIS, K.AXIS, np.pi / 6 + 0.004 * (k % 3)) for k in range(nk)])
    sht = rng.integers(0, 2, n).astype(np.int32)
    rm = np.array([shapes3[s][2] for s in sht])
    x = np.stack([K.centre(cones[0], rng.uniform(0, 2 * np.pi), rng.uniform(6.0, 9.0), rng.uniform(0.55, 1.1) * rm[i]) for i in range(n)])
    quat = bed.random_quaternions(n, rng)
    mask = np.ones(n, np.int32)
    mask[5] = 2                                            # out of the group
    coef = dict(gamma=[3.0, 0.0, 2.0, 3.0, 1.0, 0.0, 3.0, 0.0], mu=[0.5, 0.4, 0.05, 0.5, 0.0, 0.3, 0.02, 0.0],
                gt=[2.0, 3.0, 2.0, 0.0, 0.0, 300.0, 2.0, 0.0], om=[1.7, 0.0, -0.8, 0.5, 0.3, 1.1, 0.0, 0.0],
                kt=[4e3, 0.0, 3e3, 5e3, 2e3, 0.0, 4e3, 0.0])
    xi, live = np.zeros((n, nk, 3)), np.zeros((n, nk), bool)
    steps = []
    for k in range(3):
        xs = x + 0.02 * k * rng.normal(size=(n, 3))
        tw = rng.normal(size=(n, 6)) * 0.4
        d = dt if k < 2 else 0.0
        ref = CH.cone_forces_history(shapes3, nq, xs, quat, sht, tw, cones, 1000.0, 1.25, coef["gamma"], coef["mu"], coef["gt"],
                                     coef["om"], coef["kt"], xi, live, d, mask=mask)
        xi, live = ref["xi"], ref["live"]
        steps.append((xs, tw, d, ref))
    reach = np.zeros(nk, int)
    for i in range(n):
        for c in range(nk):
            reach[c] += 0 < Co.foot(x[i], cones[c])[4] < rm[i]
    return dict(shp=shp, nq=nq, n=n, cones=cones, sht=sht, quat=quat, mask=mask, coef=coef, steps=steps, reach=reach)


_crowd_bits = {}


@pytest.mark.parametrize("deterministic", [0, 1])
def test_forty_particles_in_eight_cones_match_the_reference_and_the_option_changes_no_bit(oracle, deterministic):
    import conic_history_ref as CH
    c = _crowd()
    kinds = np.concatenate([s[3]["kind"].ravel() for s in c["steps"]])
    assert (c["reach"] > 0).all() and {CH.STICK, CH.SLIDE, CH.RESET, CH.NONE} <= set(kinds)
    sp = ctx(c["shp"], c["nq"], deterministic=deterministic)
    k = c["coef"]
    setup(sp, c["cones"], k["mu"], k["gt"], k["kt"], k["om"], gamma=k["gamma"])
    P = Pass(sp, c["n"], shtype=c["sht"])
    bits = []
    for j, (xs, tw, dt, ref) in enumerate(c["steps"]):
        got = P.go(xs, c["quat"], tw, dt, mask=c["mask"])
        held = sp.conic_history(c["n"])
        e = errors(got, ref, held)
        print(f"deterministic {deterministic} pass {j} (dt {dt}): contacts {sp.cone_stats()}, " + " ".join(f"{a} {b:.1e}" for a, b in e.items()))
        assert sp.cone_stats() == ref["ncontacts"] > 40
        assert np.array_equal(live_bytes(held), live_bytes(ref["xi"]))
        assert max(e.values()) <= GATE
        bits.append((*got, held))
    assert np.array_equal(bits[2][3], bits[1][3])          # the look changed no stored byte
    _crowd_bits[deterministic] = bits
    if len(_crowd_bits) == 2:                              # the same bits with and without the option
        for a, b in zip(_crowd_bits[0], _crowd_bits[1]):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
    sp.close()


def _one_rough(oracle):
    import cone_ref as Co
    import conic_history_cases as K
    from shpair import shapes
    anm = shapes.random_shape(6, 3, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    co = Co.cone(K.APEX, K.AXIS, np.pi / 6)
    return anm, rm, co, K.centre(co, 0.8, 6.0 * rm, 0.7 * rm), np.array([0.5, -0.5, 0.5, 0.5])


def test_a_particle_carried_round_by_the_cone_keeps_its_spring(oracle):
    """The history pre-set with set_conic_history; x and quat turned by Omega dt per pass, w = Omega a^ x (x - a), omega =
    Omega a^: over 8 advancing passes (xi_g, xi_theta) stay what they were given to 1e-12 relative, phi_c follows the
    contact point and the wrench only rotates."""
    import conic_history_cases as K
    import conic_history_ref as CH
    anm, rm, co, x, q = _one_rough(oracle)
    a, ax = co[:3], co[3:6]
    Om, dt = 2.0, 0.05
    sp = ctx([(6, anm)], 16)
    setup(sp, [co], 0.5, 2.0, 4e3, Om)
    P = Pass(sp, 1)
    tw = lambda x: np.concatenate([Om * np.cross(ax, x - a), Om * ax])[None]
    look = CH.cone_forces_history([(6, anm, rm)], 16, x[None], q[None], [0], tw(x), [co], 1000.0, 1.25, 3.0, 0.5, 2.0, Om, 4e3,
                                  np.zeros((1, 1, 3)), [[False]], 0.0)
    phi0 = CH.azimuth(co, look["contacts"][0][4])
    xi0 = np.array([[[2e-3, -1e-3, CH.wrap(phi0 - Om * dt)]]])     # as the pass before the first left it
    sp.set_conic_history(1, xi0)
    g, G = K.turn(ax, Om * dt)
    Gk, first = np.eye(3), None
    for k in range(8):
        f, tq, out = P.go(x[None], q[None], tw(x), dt)
        xi = sp.conic_history(1)
        if first is None:
            first = (f[0], tq[0], out[0, 4])
        sc = np.linalg.norm(first[0])
        dx = np.abs(xi[0, 0, :2] - xi0[0, 0, :2]).max() / np.abs(xi0[0, 0, :2]).max()
        dp = abs(CH.wrap(xi[0, 0, 2] - phi0 - k * Om * dt))
        dw = max(np.abs(f[0] - Gk @ first[0]).max(), np.abs(tq[0] - Gk @ first[1]).max(), abs(out[0, 4] - first[2])) / sc
        print(f"co-rotation pass {k}: dxi {dx:.1e} dphi {dp:.1e} wrench {dw:.1e}")
        assert dx <= 1e-12 and dp <= 1e-12 and dw <= 1e-12
        x, q, Gk = a + G @ (x - a), K.qmul(g, q), G @ Gk
    sp.close()


def test_a_look_writes_nothing_and_leaving_reach_drops_the_spring(oracle):
    import conic_history_cases as K
    import conic_history_ref as CH
    anm, rm, co, x, q = _one_rough(oracle)
    sp = ctx([(6, anm)], 16)
    co2 = co.copy()
    co2[:3] -= 0.05 * co[3:6]
    cones = np.stack([co, co2])
    mu, gt, kt, om = [0.5, 0.5], [2.0, 2.0], [4e3, 3e3], [0.7, 0.0]
    setup(sp, cones, mu, gt, kt, om)
    n = 3
    xs = np.stack([x, K.centre(co, 1.3, 6.0 * rm, 0.7 * rm), K.centre(co, 0.2, 6.5 * rm, 0.75 * rm)])
    qs = np.stack([q, q, q])
    tw = np.random.default_rng(5).normal(size=(n, 6)) * 0.05
    P = Pass(sp, n)
    xi0 = np.random.default_rng(6).normal(size=(n, 2, 3)) * 1e-3
    sp.set_conic_history(n, xi0)
    shape = [(6, anm, rm)]
    ref = CH.cone_forces_history(shape, 16, xs, qs, [0] * n, tw, cones, 1000.0, 1.25, 3.0, mu, gt, om, kt, xi0, np.ones((n, 2), bool), 0.0)
    got = P.go(xs, qs, tw, 0.0)
    assert max(errors(got, ref).values()) <= GATE
    assert np.array_equal(sp.conic_history(n), xi0)                    # a look: neither the state nor the live word
    P.go(xs, qs, tw, 1e-3)
    held = sp.conic_history(n)
    assert (held != 0).all() and not np.array_equal(held, xi0)
    P.go(xs, qs, tw, 0.0)
    assert np.array_equal(sp.conic_history(n), held)                   # a look after an advance changes no stored byte
    away = xs.copy()
    away[1] = K.centre(co, 1.3, 6.0 * rm, 1.3 * rm)                    # particle 1 out of reach of both cones
    f, _, _ = P.go(away, qs, tw, 1e-3)
    after = sp.conic_history(n)
    assert not f[1].any() and not after[1].any() and (after[0] != 0).all() and (after[2] != 0).all()
    P.go(xs, qs, tw, 1e-3)                                             # ... and back: it starts from nothing
    back = sp.conic_history(n)
    ref = CH.cone_forces_history(shape, 16, xs, qs, [0] * n, tw, cones, 1000.0, 1.25, 3.0, mu, gt, om, kt, np.zeros((n, 2, 3)),
                                 np.zeros((n, 2), bool), 1e-3)
    big = np.abs(ref["xi"][..., :2]).max()
    assert np.abs(back[1, :, :2] - ref["xi"][1, :, :2]).max() <= GATE * big and np.abs(back[1, :, 2] - ref["xi"][1, :, 2]).max() <= GATE
    assert np.abs(back[0, :, :2] - ref["xi"][0, :, :2]).max() > 1e-3 * big   # the particles that stayed kept theirs
    sp.reset_conic_history()
    assert not sp.conic_history(n).any()
    sp.close()


def test_without_a_spring_the_contact_call_is_the_force_call(oracle):
    anm, rm, co, x, q = _one_rough(oracle)
    sp = ctx([(6, anm)], 16)
    sp.set_cones([co], 1000.0, 1.25)
    sp.cone_damping(3.0)
    sp.cone_friction(0.5, 2.0)
    sp.cone_rotation(0.7)
    sp.conic_spring(0.0)
    assert not sp.has_conic_history
    tw = np.array([[0.3, -0.2, 0.1, 0.5, 0.4, -0.6]])
    P = Pass(sp, 1)
    old = P.go(x[None], q[None], tw, 0.0, old_call=True)
    for dt in (0.0, 1e-3):
        new = P.go(x[None], q[None], tw, dt)
        assert old[0].any() and all(np.array_equal(a, b) for a, b in zip(old, new))
    sp.close()


def test_refusals(oracle):
    from shpair import mrank
    from shpair.capi import HaloArrays, HaloRunParams, ShPairError
    anm, rm, co, x, q = _one_rough(oracle)
    sp = ctx([(6, anm)], 16)
    setup(sp, [co], 0.5, 2.0, 4e3, 0.0, gamma=0.0)
    tw = np.zeros((1, 6))
    P = Pass(sp, 1)
    with pytest.raises(ShPairError, match="shstep_conic_contact_device") as e:   # the old force call while a spring is set
        P.go(x[None], q[None], tw, 0.0, old_call=True)
    assert e.value.code == -1
    sp.cone_friction(0.5, 0.0)                                                   # the spring alone, gamma_t = 0
    assert sp.has_conic_history
    with pytest.raises(ShPairError, match="energy ledger: a cone tangential spring is set") as e:   # a ledger behind the spring ...
        sp.set_energy_ledger(True)
    assert e.value.code == -4 and not sp.ledger_on
    with pytest.raises(ShPairError, match="shell ledger: a cone tangential spring is set") as e:
        sp.set_shell_ledger(True)
    assert e.value.code == -4 and not sp.shell_ledger_on
    sp.conic_spring(0.0)
    assert not sp.has_conic_history
    sp.set_energy_ledger(True)
    with pytest.raises(ShPairError, match="cone tangential spring: the energy ledger is on") as e:   # ... and the spring behind a ledger
        sp.conic_spring(4e3)
    assert e.value.code == -4 and not sp.has_conic_history
    sp.set_energy_ledger(False)
    sp.set_shell_ledger(True)
    with pytest.raises(ShPairError, match="cone tangential spring: the shell ledger is on") as e:
        sp.conic_spring(4e3)
    assert e.value.code == -4 and not sp.has_conic_history
    sp.set_shell_ledger(False)
    for bad in ((-1.0,), (np.nan,), (np.inf,), (1.0, 2.0)):                      # negative, not finite, a count mismatch
        with pytest.raises(ShPairError) as e:
            sp.conic_spring(np.array(bad))
        assert e.value.code == -1 and not sp.has_conic_history
    with pytest.raises(ShPairError, match="no cone tangential spring is set") as e:
        sp.conic_history(1)
    assert e.value.code == -4
    sp.conic_spring(4e3)
    with pytest.raises(ShPairError, match="dt") as e:
        P.go(x[None], q[None], tw, -1e-3)
    assert e.value.code == -1
    # the loop over several ranks, and its Python driver
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    stand_in = type("R", (), dict(sp=sp, a=None, stream=None, halo=None))()
    with pytest.raises(ShPairError, match="conical walls are single-rank") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -4
    with pytest.raises(ShPairError, match="conical walls are single-rank") as e:
        mrank.RankRun.force(stand_in)
    assert e.value.code == -4
    halo.close()
    sp.set_cones([co], 1000.0, 1.25)                                             # resets every k_t and drops the history
    assert not sp.has_conic_history
    P.go(x[None], q[None], tw, 0.0, old_call=True)
    sp.close()


# ---- steps ---------------------------------------------------------------------------------------------------------

def _run(oracle, mode, nsteps, restart_at=None):
    """Eight particles on a ring in a turning hopper along z, gravity, springs at the cone."""
    import torch
    import cone_ref as Co
    from shpair import shapes, bed
    from shpair.run import DeviceRun
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    rm = oracle.shape_rmax(4, shp[0][1])
    rng = np.random.default_rng(12)
    th = np.pi / 6
    co = Co.cone([4.0, 4.0, 0.5], [0.0, 0.0, 1.0], th)
    s = 6.0
    t, d = np.cos(th) * s + np.sin(th) * 0.9 * rm, np.sin(th) * s - np.cos(th) * 0.9 * rm
    phi = np.arange(8) * np.pi / 4
    x = np.stack([4.0 + d * np.cos(phi), 4.0 + d * np.sin(phi), 0.5 + t + 0 * phi], axis=1) + rng.uniform(-0.02, 0.02, (8, 3))
    quat, sht = bed.random_quaternions(8, rng), np.zeros(8, np.int32)
    opts = dict(cones=([co], 2000.0, 1.25), cone_damping=20.0, cone_friction=(0.4, 30.0), cone_rotation=0.8, conic_spring=5e3)
    kw = dict(dt=5e-4, gravity=(0.0, 0.0, -9.81), gamma_t=0.2, gamma_r=0.1)
    sp = ctx(shp, 10, kn=2000.0, deterministic=1)
    r = DeviceRun(sp, x, quat, sht, (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, **kw, **opts)

    def advance(r, k):
        if mode == "python":
            r.run(k)
        else:
            r.run_native(k, use_graph=(mode == "graph"))
        torch.cuda.synchronize()
    if restart_at is not None:
        advance(r, restart_at)
        n = r.n
        saved = [t.cpu().numpy().copy() for t in (r.x[:n], r.q[:n], r.v, r.L, r.f[:n], r.tq[:n])]
        cones, hist = sp.get_cones(), r.cone_history()
        sp.close()
        sp = ctx(shp, 10, kn=2000.0, deterministic=1)
        opts["cones"] = (cones, 2000.0, 1.25)
        r = DeviceRun(sp, saved[0], saved[1], sht, (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, **kw, **opts)
        r.v.copy_(dev(saved[2]))
        r.L.copy_(dev(saved[3]))
        r.f[:n].copy_(dev(saved[4]))               # the forces of the last step, as a restart file holds them
        r.tq[:n].copy_(dev(saved[5]))
        sp.set_conic_history(n, hist)
        nsteps -= restart_at
    advance(r, nsteps)
    n = r.n
    state = [t.cpu().numpy().copy() for t in (r.x[:n], r.v, r.q[:n], r.L)] + [r.cone_history()]
    nc = sp.cone_stats()
    sp.close()
    return state, nc


def test_run_loops_and_a_restart_leave_the_same_bits(oracle):
    """DeviceRun stepping, shstep_run_device plain and replayed from graphs: the same bits of x, v, q, L and the cone
    history after 32 steps; and a restart after 16 steps from get_cones(), the arrays and cone_history() continues
    bitwise."""
    ref, nc = _run(oracle, "python", 32)
    assert nc > 0 and np.abs(ref[4][..., :2]).max() > 0
    for mode, at in (("plain", None), ("graph", None), ("python", 16), ("graph", 16)):
        got, nc2 = _run(oracle, mode, 32, restart_at=at)
        assert nc2 == nc
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), (mode, at)
