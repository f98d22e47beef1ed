"""GPU tests of the coefficient setters of the planar walls and the cylinders (csrc/shstep_walls.hip,
csrc/shstep_cylinders.hip through the C ABI of include/shstep.h): a context that went through a setter history which
crosses every transition of damp / fric / hist / roll computes, bit for bit, what a fresh context computes that was given
only the coefficients in force.  One particle of order 2 with n_q = 8 in a corner of two planar walls, and the same
particle against one cylinder of two: the smallest setup in which a coefficient on the wrong surface, a stale device
table or a wrong kernel instance changes a number.  Every input is one the setters accept; no reference is needed: the
fresh context is the reference."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dissipation_common import _wall_ctx, dev  # noqa: E402

LMAX, NQ = 2, 8
TW = np.array([[0.3, -0.2, 0.1, 0.5, -0.4, 0.2]])
Q = np.array([[0.5, -0.5, 0.5, 0.5]])
ZERO2 = [0.0, 0.0]


def _ctx():
    from shpair import shapes
    return _wall_ctx([(LMAX, shapes.random_shape(LMAX, 3, amp=0.1))], NQ)


def _pass(call, nsurf, width, x):
    """One pass with twists and dt = 0 on fresh arrays: f, torque, the per-surface totals, as bytes."""
    import torch
    xd, qd, twd = dev(x), dev(Q), dev(TW)
    sh, m = dev(np.zeros(1, np.int32)), dev(np.ones(1, np.int32))
    f, tq = (torch.zeros(1, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
    out = torch.zeros(nsurf, width, dtype=torch.float64, device="cuda:0")
    call(1, xd.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), twd.data_ptr(), 0.0, out.data_ptr())
    torch.cuda.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy()


def _same(got, want, label):
    for name, a, b in zip(("f", "torque", "totals"), got, want):
        assert a.tobytes() == b.tobytes(), (label, name, a, b)


# ---- planar walls -------------------------------------------------------------------------------------------------------

def _planes():
    return np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]])


def _wall_x(sp):
    rm = sp.rmax(0)
    return np.array([[0.6 * rm, 0.65 * rm, 0.1]])


def _wall_apply(sp, co):
    """The coefficients `co` through the setters, each once, in one fixed order."""
    sp.wall_damping(co.get("gamma", ZERO2))
    sp.wall_friction(*co.get("fric", (ZERO2, ZERO2)))
    sp.set_wall_tangential_spring(co.get("kt", ZERO2))
    sp.wall_rolling(*co.get("roll", (ZERO2, ZERO2)))
    sp.wall_twisting(*co.get("twist", (ZERO2, ZERO2)))


def _wall_go(sp, xi0):
    if sp.has_wall_history:   # a spring only shows with a live xi: the same one on both sides
        sp.set_wall_history(1, xi0)
    call = lambda *a: sp.wall_contact_device(*a[:8], a[8], wall_out=a[9])   # noqa: E731
    got = _pass(call, 2, 4, _wall_x(sp))
    return got, sp.wall_stats()


def _wall_check(sp, co, label, kn=1000.0):
    """sp against a fresh context that was given only `co`; and `co` matters: the elastic pass gives other bits."""
    xi0 = np.array([[[1e-3, -2e-3, 1.5e-3], [-1e-3, 5e-4, 2e-3]]])
    got, count = _wall_go(sp, xi0)
    fresh = _ctx()
    fresh.set_walls(_planes(), kn, 1.25)
    _wall_apply(fresh, co)
    for name in ("wall_reads_twists", "has_wall_rolling", "has_wall_history", "damp_walls", "fric_walls"):
        assert getattr(sp, name) == getattr(fresh, name), (label, name)
    want, wcount = _wall_go(fresh, xi0)
    fresh.set_walls(_planes(), kn, 1.25)
    ela, ecount = _wall_go(fresh, xi0)
    fresh.close()
    print(f"walls {label}: contacts {count}, f {got[0][0]}, elastic f {ela[0][0]}")
    assert count == wcount == ecount == 2
    _same(got, want, label)
    assert got[0].tobytes() != ela[0].tobytes() and got[1].tobytes() != ela[1].tobytes(), label


def test_a_wall_setter_history_ends_where_a_fresh_context_starts():
    sp = _ctx()
    sp.set_walls(_planes(), 1000.0, 1.25)
    sp.wall_friction([0.5, 0.3], [2.0, 1.5])                      # 1. friction
    assert sp.fric_walls and not sp.has_wall_history
    _wall_check(sp, dict(fric=([0.5, 0.3], [2.0, 1.5])), "friction")
    sp.set_wall_tangential_spring([4000.0, 3000.0])               # 2. spring: hist on
    assert sp.has_wall_history
    assert not sp.wall_history(1).any()
    _wall_check(sp, dict(fric=([0.5, 0.3], [2.0, 1.5]), kt=[4000.0, 3000.0]), "friction, spring")   # (leaves a live xi)
    assert sp.wall_history(1).all()
    sp.wall_friction(ZERO2, ZERO2)                                # 3. friction zeroed: hist off, xi dropped
    assert not sp.has_wall_history and not sp.wall_reads_twists
    sp.set_wall_tangential_spring([3500.0, 0.0])                  # 4. spring again: no mu, no history
    assert not sp.has_wall_history
    sp.wall_damping([3.0, 1.0])                                   # 5. damping
    _wall_check(sp, dict(gamma=[3.0, 1.0], kt=[3500.0, 0.0]), "damping, spring without mu")
    sp.wall_rolling([0.01, 0.02], [0.5, 0.4])                     # 6. rolling, twisting, rolling zeroed
    sp.wall_twisting([0.02, 0.01], [0.3, 0.6])
    _wall_check(sp, dict(gamma=[3.0, 1.0], kt=[3500.0, 0.0], roll=([0.01, 0.02], [0.5, 0.4]), twist=([0.02, 0.01], [0.3, 0.6])),
                "damping, rolling, twisting")
    sp.wall_rolling(ZERO2, ZERO2)
    assert sp.has_wall_rolling
    # friction back: wall 0 has mu and k_t but no gamma_t (history, no friction), wall 1 mu and gamma_t but no k_t
    sp.wall_friction([0.4, 0.6], [0.0, 1.0])
    assert sp.has_wall_history and sp.fric_walls
    assert not sp.wall_history(1).any()                           # hist changed since the xi of step 2 was live
    _wall_check(sp, dict(gamma=[3.0, 1.0], kt=[3500.0, 0.0], twist=([0.02, 0.01], [0.3, 0.6]), fric=([0.4, 0.6], [0.0, 1.0])),
                "every kind, split over the walls")
    assert sp.wall_history(1)[0, 0].all()
    sp.set_walls(_planes(), 900.0, 1.25)                          # 7. the geometry setter
    assert not sp.wall_reads_twists
    final = dict(gamma=[2.0, 0.0], fric=([0.5, 0.3], [2.0, 1.5]), kt=[0.0, 4000.0], roll=([0.01, 0.0], [0.5, 0.0]))
    sp.set_wall_tangential_spring(final["kt"])                    # 8. the final coefficients, spring first
    sp.wall_rolling(*final["roll"])
    sp.wall_friction(*final["fric"])
    sp.wall_damping(final["gamma"])
    assert sp.has_wall_history and not sp.wall_history(1).any()
    _wall_check(sp, final, "final", kn=900.0)
    sp.close()


# ---- cylinders ----------------------------------------------------------------------------------------------------------

def _cyls(sp):
    """Two cylinders about one axis; the particle of _cyl_x reaches the second (0.6 rmax from its wall), not the first."""
    rm = sp.rmax(0)
    a, ax = [0.3, -0.2, 0.5], [2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0]
    return np.array([a + ax + [10.0 * rm], a + ax + [2.5 * rm]])


def _cyl_x(sp):
    rm = sp.rmax(0)
    c = _cyls(sp)[1]
    e1 = np.cross(c[3:6], [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return (c[:3] + (c[6] - 0.6 * rm) * e1 + 0.3 * c[3:6])[None]


def _cyl_apply(sp, co):
    sp.cylinder_damping(co.get("gamma", ZERO2))
    sp.cylinder_friction(*co.get("fric", (ZERO2, ZERO2)))
    sp.set_cyl_tangential_spring(co.get("kt", ZERO2))
    sp.cylinder_rotation(co.get("omega", ZERO2))


def _cyl_go(sp, xi0):
    if sp.has_cyl_history:
        sp.set_cyl_history(1, xi0)
    call = lambda *a: sp.cyl_contact_device(*a[:8], a[8], cyl_out=a[9])   # noqa: E731
    got = _pass(call, 2, 5, _cyl_x(sp))
    return got, sp.cylinder_stats()


def _cyl_check(sp, co, label, kn=1000.0):
    xi0 = np.array([[[1e-3, -2e-3], [-1e-3, 5e-4]]])
    got, count = _cyl_go(sp, xi0)
    fresh = _ctx()
    fresh.set_cylinders(_cyls(fresh), kn, 1.25)
    _cyl_apply(fresh, co)
    for name in ("cylinder_reads_twists", "has_cyl_history"):
        assert getattr(sp, name) == getattr(fresh, name), (label, name)
    want, wcount = _cyl_go(fresh, xi0)
    fresh.set_cylinders(_cyls(fresh), kn, 1.25)
    ela, ecount = _cyl_go(fresh, xi0)
    fresh.close()
    print(f"cylinders {label}: contacts {count}, f {got[0][0]}, elastic f {ela[0][0]}")
    assert count == wcount == ecount == 1
    assert not got[2][0].any() and got[2][1, 0] > 0.0             # the totals are the second cylinder's
    _same(got, want, label)
    assert got[0].tobytes() != ela[0].tobytes() and got[1].tobytes() != ela[1].tobytes(), label


def test_a_cylinder_setter_history_ends_where_a_fresh_context_starts():
    sp = _ctx()
    sp.set_cylinders(_cyls(sp), 1000.0, 1.25)
    sp.cylinder_friction([0.3, 0.5], [1.5, 2.0])                  # 1. friction
    assert sp.cylinder_reads_twists and not sp.has_cyl_history
    _cyl_check(sp, dict(fric=([0.3, 0.5], [1.5, 2.0])), "friction")
    sp.set_cyl_tangential_spring([3000.0, 4000.0])                # 2. spring: hist on
    assert sp.has_cyl_history and not sp.cyl_history(1).any()
    _cyl_check(sp, dict(fric=([0.3, 0.5], [1.5, 2.0]), kt=[3000.0, 4000.0]), "friction, spring")   # (leaves a live xi)
    assert sp.cyl_history(1).all()
    sp.cylinder_friction(ZERO2, ZERO2)                            # 3. friction zeroed: hist off, xi dropped
    assert not sp.has_cyl_history and not sp.cylinder_reads_twists
    sp.set_cyl_tangential_spring([0.0, 3500.0])                   # 4. spring again: no mu, no history
    assert not sp.has_cyl_history
    sp.cylinder_rotation([0.2, -0.7])                             # (Omega alone is no coefficient)
    assert not sp.cylinder_reads_twists
    sp.cylinder_damping([1.0, 3.0])                               # 5. damping
    _cyl_check(sp, dict(gamma=[1.0, 3.0], kt=[0.0, 3500.0], omega=[0.2, -0.7]), "damping, spring without mu, rotation")
    sp.cylinder_friction([0.6, 0.4], [0.0, 1.0])                  # friction back: hist on again
    assert sp.has_cyl_history
    assert not sp.cyl_history(1).any()                            # hist changed since the xi of step 2 was live
    _cyl_check(sp, dict(gamma=[1.0, 3.0], kt=[0.0, 3500.0], omega=[0.2, -0.7], fric=([0.6, 0.4], [0.0, 1.0])), "every kind")
    assert sp.cyl_history(1)[0, 1].all()
    sp.set_cylinders(_cyls(sp), 900.0, 1.25)                      # 7. the geometry setter
    assert not sp.cylinder_reads_twists
    final = dict(gamma=[0.0, 2.0], fric=([0.3, 0.5], [1.5, 2.0]), kt=[3000.0, 4000.0], omega=[0.0, 0.5])
    sp.set_cyl_tangential_spring(final["kt"])                     # 8. the final coefficients, spring first
    sp.cylinder_rotation(final["omega"])
    sp.cylinder_friction(*final["fric"])
    sp.cylinder_damping(final["gamma"])
    assert sp.has_cyl_history and not sp.cyl_history(1).any()
    _cyl_check(sp, final, "final", kn=900.0)
    sp.close()
