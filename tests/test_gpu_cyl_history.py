"""GPU tests of the tangential springs with history at the cylinders of docs/SPEC.md §2.19 (cyl_spring_kernel and
cyl_live_sweep_kernel of csrc/cylinder_kernels.hpp through the C ABI of include/shstep.h) against
tests/cyl_history_ref.py.  The gate is tests/test_gpu_cylinder.py's, 1e-9 of the largest reference force (SPEC §4), and
for xi 1e-9 of the largest reference |xi|.  Every test uses at most 40 particles."""
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
    """Device arrays of one particle set and the two cylinder calls on them."""

    def __init__(self, sp, n, shtype=None):
        self.sp, self.n = sp, n
        self.sh = dev(np.zeros(n, np.int32) if shtype is None else shtype)
        self.nc = sp.ncylinders

    def go(self, x, quat, tw, dt, mask=None, old_call=False, want_out=True):
        import torch
        n = self.n
        xd, qd, twd = dev(x), dev(quat), dev(tw)
        m = dev(np.ones(n, np.int32) if mask is None else mask.astype(np.int32))
        f, tq = (torch.zeros(n, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
        out = torch.zeros(self.nc, 5, dtype=torch.float64, device="cuda:0")
        args = (n, xd.data_ptr(), qd.data_ptr(), self.sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
        if old_call:
            self.sp.cylinder_force_device(*args, twist=twd.data_ptr(), cyl_out=out.data_ptr() if want_out else None)
        else:
            self.sp.cyl_contact_device(*args, twd.data_ptr(), dt, cyl_out=out.data_ptr() if want_out else None)
        torch.cuda.synchronize()
        return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy()


def errors(got, ref):
    f, tq, out = got
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ro = ref["cyl_out"]
    return dict(f=np.abs(f - ref["f"]).max() / scale, torque=np.abs(tq - ref["torque"]).max() / tscale,
                wall=np.abs(out[:, 1:4] - ro[:, 1:4]).max() / np.abs(ro[:, 1:4]).max(),
                energy=np.abs(out[:, 0] - ro[:, 0]).max() / np.abs(ro[:, 0]).max(),
                M_ax=np.abs(out[:, 4] - ro[:, 4]).max() / max(tscale, np.abs(ro[:, 4]).max()))


def setup(sp, cyls, mu, gt, kt, om, gamma=3.0, kn=1000.0, expo=1.25, spring_first=False):
    sp.set_cylinders(cyls, kn, expo)
    sp.cylinder_damping(gamma)
    if spring_first:   # the two setters give the same state in either order
        sp.set_cyl_tangential_spring(kt)
        sp.cylinder_friction(mu, gt)
    else:
        sp.cylinder_friction(mu, gt)
        sp.set_cyl_tangential_spring(kt)
    sp.cylinder_rotation(om)


@pytest.mark.parametrize("name", ["oblique", "two", "axis"])
@pytest.mark.parametrize("lmax,nq", [(6, 16), (4, 10), (4, 1)])
def test_four_advancing_passes_match_the_reference(oracle, lmax, nq, name):
    """x, quat and the twists of four passes are prescribed; the device carries (xi_a, xi_theta) on its side, the reference
    on its own.  The inputs hold every kind of contact and none near the cap (read from the reference alone)."""
    import cyl_history_cases as K
    c = K.case(lmax, nq, name)
    counts = K.check_conditions(c)
    assert (counts["none"] > 0) == (name == "two")
    sp = ctx([(lmax, c["anm"])], nq, deterministic=(nq == 10))
    setup(sp, c["cyls"], c["mu"], c["gt"], c["kt"], c["om"], spring_first=(nq == 16))
    assert sp.has_cyl_history
    P = Pass(sp, c["n"])
    for k in range(K.NPASS):
        ref = c["refs"][k]
        got = P.go(c["xs"][k], c["quat"], c["tws"][k], K.DT, mask=c["masks"][k])
        xi = sp.cyl_history(c["n"])
        e = errors(got, ref)
        e["xi"] = np.abs(xi - ref["xi"]).max() / np.abs(ref["xi"]).max()
        print(f"L={lmax} nq={nq} {name} pass {k}: contacts {sp.cylinder_stats()}, " + " ".join(f"{a} {b:.1e}" for a, b in e.items()))
        assert sp.cylinder_stats() == ref["ncontacts"] > 0
        assert np.array_equal(xi != 0, np.repeat(ref["live"][:, :, None], 2, axis=2) & (ref["xi"] != 0))
        assert max(e.values()) <= GATE
    sp.close()


def _one_rough(oracle):
    from shpair import shapes
    anm = shapes.random_shape(6, 3, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    cyl = np.array([0.3, -0.2, 0.5, 2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0, 2.5 * rm])
    e1 = np.cross(cyl[3:6], [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    x = cyl[:3] + (cyl[6] - 0.7 * rm) * e1 + 0.3 * cyl[3:6]
    q = np.array([0.5, -0.5, 0.5, 0.5])
    return anm, rm, cyl, x, q


def test_a_contact_at_rest_carries_a_load(oracle):
    """Zero twists and a xi well inside the cap: F_t = -k_t (xi_a a^ + xi_theta t^_c) to the gate, M_ax holds it, and a look
    writes nothing.  Without k_t the same pass equals the elastic one bit for bit: §2.18 alone carries nothing at rest."""
    import cyl_history_ref as CH
    anm, rm, cyl, x, q = _one_rough(oracle)
    sp = ctx([(6, anm)], 16)
    kt, xi0 = 4e3, np.array([[[2e-3, -1e-3]]])
    setup(sp, [cyl], 0.5, 2.0, kt, 0.0)
    P = Pass(sp, 1)
    sp.set_cyl_history(1, xi0)
    zero = np.zeros((1, 6))
    got = P.go(x[None], q[None], zero, 0.0)
    ref = CH.cyl_forces_history([(6, anm, rm)], 16, x[None], q[None], [0], zero, [cyl], 1000.0, 1.25, 3.0, 0.5, 2.0, 0.0, kt, xi0,
                                [[True]], 0.0)
    (_, _, Ft, ri, rc, vt, N, kind, ratio), = ref["contacts"]
    assert kind == CH.STICK and ratio < 0.5
    ea, et = CH.surface_frame(cyl[3:6], rc, cyl[6])
    want = -kt * (xi0[0, 0, 0] * ea + xi0[0, 0, 1] * et)
    sp.set_cyl_tangential_spring(0.0)            # no k_t: the dissipative instance at rest ...
    off = P.go(x[None], q[None], zero, 0.0)
    sp.cylinder_friction(0.0, 0.0)
    sp.cylinder_damping(0.0)                     # ... and the elastic one
    ela = P.go(x[None], q[None], zero, 0.0, old_call=True)
    scale = np.abs(ref["f"]).max()
    e = errors(got, ref)
    ft = got[0][0] - ela[0][0]
    print("at rest: |F_t| %.4g of |F| %.4g, " % (np.linalg.norm(want), scale) + " ".join(f"{a} {b:.1e}" for a, b in e.items()))
    assert max(e.values()) <= GATE and np.abs(ft - want).max() <= GATE * scale and np.linalg.norm(want) > 1e-3 * scale
    assert got[2][0, 4] != ela[2][0, 4]          # the static load the drive holds
    assert all(np.array_equal(a, b) for a, b in zip(off, ela))
    sp.close()


def test_a_particle_carried_round_by_the_drum_keeps_its_spring(oracle):
    """x and quat turned by Omega dt per pass, w = Omega a^ x (x - a), omega = Omega a^: over 8 advancing passes
    (xi_a, xi_theta) stay what they were given to 1e-12 relative and the wrench only rotates.  A space-frame vector with a
    projection would lose 1 - cos(Omega dt) = 5e-3 of its length per pass."""
    from test_cyl_ref import qmul
    import wall_ref as W
    anm, rm, cyl, x, q = _one_rough(oracle)
    a, ax = cyl[:3], cyl[3:6]
    Om, dt = 2.0, 0.05
    sp = ctx([(6, anm)], 16)
    setup(sp, [cyl], 0.5, 2.0, 4e3, Om)
    P = Pass(sp, 1)
    xi0 = np.array([[[2e-3, -1e-3]]])
    sp.set_cyl_history(1, xi0)
    g = np.array([np.cos(Om * dt / 2), *(np.sin(Om * dt / 2) * ax)])
    G, Gk, first = W.quat_to_mat(g), np.eye(3), None
    for k in range(8):
        tw = np.concatenate([Om * np.cross(ax, x - a), Om * ax])[None]
        f, tq, out = P.go(x[None], q[None], tw, dt)
        xi = sp.cyl_history(1)
        if first is None:
            first = (f[0], tq[0], out[0, 4])
        sc = np.linalg.norm(first[0])
        dx = np.abs(xi - xi0).max() / np.abs(xi0).max()
        dw = max(np.abs(f[0] - Gk @ first[0]).max(), np.abs(tq[0] - Gk @ first[1]).max(), abs(out[0, 4] - first[2])) / sc
        print(f"co-rotation pass {k}: dxi {dx:.1e} wrench {dw:.1e}")
        assert dx <= 1e-12 and dw <= 1e-12
        x, q, Gk = a + G @ (x - a), qmul(g, q), G @ Gk
    sp.close()


def test_a_look_writes_nothing_and_leaving_reach_drops_the_spring(oracle):
    import cyl_history_ref as CH
    anm, rm, cyl, x, q = _one_rough(oracle)
    sp = ctx([(6, anm)], 16)
    setup(sp, [cyl, cyl + np.array([0, 0, 0, 0, 0, 0, 0.05])], [0.5, 0.5], [2.0, 2.0], [4e3, 3e3], [0.7, 0.0])
    cyls = sp.get_cylinders()
    n = 3
    xs = np.stack([x, x + 0.4 * cyl[3:6], x - 0.4 * cyl[3:6]])
    qs = np.stack([q, q, q])
    tw = np.random.default_rng(5).normal(size=(n, 6)) * 0.05
    P = Pass(sp, n)
    xi0 = np.random.default_rng(6).normal(size=(n, 2, 2)) * 1e-3
    sp.set_cyl_history(n, xi0)
    got = P.go(xs, qs, tw, 0.0)
    ref = CH.cyl_forces_history([(6, anm, rm)], 16, xs, qs, [0] * n, tw, cyls, 1000.0, 1.25, 3.0, 0.5, 2.0, [0.7, 0.0], [4e3, 3e3], xi0,
                                np.ones((n, 2), bool), 0.0)
    assert max(errors(got, ref).values()) <= GATE
    assert np.array_equal(sp.cyl_history(n), xi0)                      # a look: neither xi nor the live word
    P.go(xs, qs, tw, 1e-3)
    held = sp.cyl_history(n)
    assert (held != 0).all() and not np.array_equal(held, xi0)
    away = xs.copy()
    away[1] = cyl[:3] + 0.1 * cyl[3:6]                                 # particle 1 out of reach of both cylinders
    f, _, _ = P.go(away, qs, tw, 1e-3)
    after = sp.cyl_history(n)
    assert not f[1].any() and not after[1].any() and (after[0] != 0).all() and (after[2] != 0).all()
    P.go(xs, qs, tw, 1e-3)                                             # ... and back: it starts from nothing
    back = sp.cyl_history(n)
    ref = CH.cyl_forces_history([(6, anm, rm)], 16, xs, qs, [0] * n, tw, cyls, 1000.0, 1.25, 3.0, 0.5, 2.0, [0.7, 0.0], [4e3, 3e3],
                                np.zeros((n, 2, 2)), np.zeros((n, 2), bool), 1e-3)
    assert np.abs(back[1] - ref["xi"][1]).max() <= GATE * np.abs(ref["xi"]).max()
    assert np.abs(back[0] - ref["xi"][0]).max() > 1e-3 * np.abs(ref["xi"]).max()   # the particles that stayed kept theirs
    sp.reset_cyl_history()
    assert not sp.cyl_history(n).any()
    sp.close()


def test_without_a_spring_the_contact_call_is_the_force_call(oracle):
    anm, rm, cyl, x, q = _one_rough(oracle)
    sp = ctx([(6, anm)], 16)
    sp.set_cylinders([cyl], 1000.0, 1.25)
    sp.cylinder_damping(3.0)
    sp.cylinder_friction(0.5, 2.0)
    sp.cylinder_rotation(0.7)
    sp.set_cyl_tangential_spring(0.0)
    assert not sp.has_cyl_history
    tw = np.array([[0.3, -0.2, 0.1, 0.5, 0.4, -0.6]])
    P = Pass(sp, 1)
    old = P.go(x[None], q[None], tw, 0.0, old_call=True)
    for dt in (0.0, 1e-3):
        new = P.go(x[None], q[None], tw, dt)
        assert old[0].any() and all(np.array_equal(a, b) for a, b in zip(old, new))
    sp.close()


def test_refusals(oracle):
    from shpair import shapes
    from shpair.capi import ShPairError
    anm, rm, cyl, x, q = _one_rough(oracle)
    sp = ctx([(6, anm)], 16)
    setup(sp, [cyl], 0.5, 2.0, 4e3, 0.0)
    tw = np.zeros((1, 6))
    P = Pass(sp, 1)
    with pytest.raises(ShPairError, match="shstep_cyl_contact_device") as e:   # the old force call while a spring is set
        P.go(x[None], q[None], tw, 0.0, old_call=True)
    assert e.value.code == -1
    with pytest.raises(ShPairError, match="cylinder tangential spring is set") as e:   # the ledger behind the spring ...
        sp.set_energy_ledger(True)
    assert e.value.code == -4 and not sp.ledger_on
    sp.set_cyl_tangential_spring(0.0)
    sp.cylinder_friction(0.5, 0.0)
    sp.cylinder_damping(0.0)
    sp.set_energy_ledger(True)
    with pytest.raises(ShPairError, match="energy ledger is on") as e:         # ... and the spring behind the ledger
        sp.set_cyl_tangential_spring(4e3)
    assert e.value.code == -4 and not sp.has_cyl_history
    sp.set_energy_ledger(False)
    for bad in ((-1.0,), (np.nan,), (np.inf,), (1.0, 2.0)):                     # negative, not finite, a count mismatch
        with pytest.raises(ShPairError) as e:
            sp.set_cyl_tangential_spring(np.array(bad))
        assert e.value.code == -1 and not sp.has_cyl_history
    with pytest.raises(ShPairError) as e:
        sp.cyl_history(1)                                                       # no spring set
    assert e.value.code == -4
    sp.set_cyl_tangential_spring(4e3)
    with pytest.raises(ShPairError) as e:
        P.go(x[None], q[None], tw, -1e-3)
    assert e.value.code == -1
    sp.set_cylinders([cyl], 1000.0, 1.25)                                       # resets every k_t and drops the history
    assert not sp.has_cyl_history
    P.go(x[None], q[None], tw, 0.0, old_call=True)
    sp.close()


# ---- steps ---------------------------------------------------------------------------------------------------------

def _drum(oracle):
    from shpair import shapes, bed
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    rng = np.random.default_rng(12)
    g = np.array([-0.95, 0.95])
    cyl = np.array([4.0, 4.0, 4.0, 0.0, 1.0, 0.0, np.hypot(0.95, 0.95) + 0.9 * oracle.shape_rmax(4, shp[0][1])])
    x = np.stack(np.meshgrid(g, np.arange(4) * 1.9 - 2.85, g, indexing="ij"), axis=-1).reshape(-1, 3) + [4.0, 4.0, 4.0]
    x += rng.uniform(-0.05, 0.05, x.shape)
    return shp, cyl, x, bed.random_quaternions(x.shape[0], rng), np.zeros(x.shape[0], np.int32)


def _run(oracle, mode, nsteps, restart_at=None):
    """16 particles in a closed drum (a cylinder along y and two planes), gravity, springs at the shell."""
    import torch
    from shpair.run import DeviceRun
    shp, cyl, x, quat, sht = _drum(oracle)
    opts = dict(walls=([[0, 1, 0, 0.2], [0, -1, 0, -7.8]], 2000.0, 1.25), cylinders=([cyl], 2000.0, 1.25), cylinder_damping=20.0,
                cylinder_friction=(0.4, 30.0), cylinder_rotation=0.8, cylinder_spring=5e3)
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
        cyls, hist = sp.get_cylinders(), r.cylinder_history()
        sp.close()
        sp = ctx(shp, 10, kn=2000.0, deterministic=1)
        opts["cylinders"] = (cyls, 2000.0, 1.25)
        r = DeviceRun(sp, saved[0], saved[1], sht, (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, **kw, **opts)
        r.v.copy_(dev(saved[2]))
        r.L.copy_(dev(saved[3]))
        r.f[:n].copy_(dev(saved[4]))               # the forces of the last step, as a restart file holds them
        r.tq[:n].copy_(dev(saved[5]))
        sp.set_cyl_history(n, hist)
        nsteps -= restart_at
    advance(r, nsteps)
    n = r.n
    state = [t.cpu().numpy().copy() for t in (r.x[:n], r.v, r.q[:n], r.L)] + [r.cylinder_history()]
    nc = sp.cylinder_stats()
    sp.close()
    return state, nc


def test_run_loops_and_a_restart_leave_the_same_bits(oracle):
    """DeviceRun stepping, shstep_run_device plain and replayed from graphs: the same bits of x, v, q, L and the cylinder
    history after 20 steps; and a restart after 8 steps from get_cylinders(), the arrays and cylinder_history()
    continues bitwise."""
    ref, nc = _run(oracle, "python", 20)
    assert nc > 0 and np.abs(ref[4]).max() > 0
    for mode, at in (("plain", None), ("graph", None), ("python", 8), ("graph", 8)):
        got, nc2 = _run(oracle, mode, 20, restart_at=at)
        assert nc2 == nc
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), (mode, at)
