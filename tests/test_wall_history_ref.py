"""CPU pins of tests/wall_history_ref.py, the numpy restatement of docs/SPEC.md §2.15 that the GPU wall-history tests
compare against: without a spring it is the moving-wall reference, the cap holds, a sliding contact keeps the xi its force
can hold, xi stays in the plane, a common velocity of wall and particle leaves it alone, and a constant v_t draws the
closed-form hysteresis loop.  It pins the yardstick, not the kernels."""
import numpy as np
import pytest

import wall_history_ref as H
import wall_move_ref as M
from shpair import shapes


@pytest.fixture(scope="module")
def corner(oracle):
    """The corner of tests/test_wall_move_ref.py: one L = 4 particle against three walls, n_q = 8, and a spring on the
    first two walls (the third keeps the history-free law)."""
    anm = shapes.random_shape(4, 3, amp=0.1)
    sh = [(4, anm, oracle.shape_rmax(4, anm))]
    planes = np.array([[1.0, 0, 0, 0.0], [0, 1.0, 0, 0.0], [0, 0, 1.0, 0.0]])
    a = (sh, 8, np.array([[0.8, 0.9, 0.7]]), np.array([[0.5, 0.5, -0.5, 0.5]]), np.zeros(1, np.int32))
    tw = np.array([[0.35, -0.6, -0.25, 0.5, 0.8, -0.7]])
    co = (planes, np.array([1000.0, 800.0, 1200.0]), np.array([1.25, 1.0, 2.0]), np.array([400.0, 250.0, 600.0]),
          np.array([0.5, 0.1, 0.6]), np.array([200.0, 400.0, 100.0]))
    kt = np.array([3000.0, 500.0, 0.0])
    return a, tw, co, kt


def _state(seed, scale=0.02):
    rng = np.random.default_rng(seed)
    return scale * rng.normal(size=(1, 3, 3)), np.array([[True, True, True]])


def test_without_a_spring_it_is_the_moving_wall_reference_exactly(corner):
    a, tw, co, _ = corner
    vel = np.array([[0.9, -0.7, 0.4], [0.6, -1.1, 0.8], [-0.1, 0.2, -0.1]])
    xi, live = _state(1)
    got = H.wall_forces_history(*a, tw, *co, np.zeros(3), vel, xi, live, 1e-3)
    ref = M.wall_forces_moving(*a, tw, *co, vel)
    assert len(ref["contacts"]) == 3 and np.abs(ref["f"]).max() > 0
    for k in ("f", "torque", "wall_out"):
        assert np.array_equal(got[k], ref[k]), k
    for c, d in zip(got["contacts"], ref["contacts"]):
        assert c[:5] == d[:5] and np.array_equal(c[5], d[5]) and np.array_equal(c[6], d[6]) and c[7] == d[7]
    assert (got["kind"] == H.NONE).all() and not got["live"].any() and not got["xi"].any()


def test_cap_sliding_state_and_projection(corner):
    """|F_t| <= mu N always; a sliding contact leaves k_t xi + gamma_t v_t = -F_t with |F_t| = mu N; xi.n = 0 after every
    pass; the wall without a spring keeps no state."""
    a, tw, co, kt = corner
    planes, mu, gt = co[0], co[4], co[5]
    kinds = set()
    for seed, scale, dt in ((1, 1e-3, 1e-3), (2, 0.05, 1e-3), (3, 0.5, 1e-2), (4, 1e-4, 1e-4)):
        xi, live = _state(seed, scale)
        r = H.wall_forces_history(*a, tw, *co, kt, np.zeros((3, 3)), xi, live, dt)
        for (i, w, p, pt, N, Ft, ri, cp, kind, vt) in r["contacts"]:
            if w == 2:
                assert kind == H.NONE and not r["live"][0, 2] and not r["xi"][0, 2].any()
                continue
            kinds.add(kind)
            n = planes[w, :3]
            assert np.linalg.norm(Ft) <= mu[w] * N * (1 + 1e-14)
            assert abs(r["xi"][0, w] @ n) <= 1e-16 * max(1.0, np.abs(r["xi"][0, w]).max()) and r["live"][0, w]
            assert abs(Ft @ n) <= 1e-12 * np.linalg.norm(Ft)
            if kind == H.SLIDE:
                assert abs(np.linalg.norm(Ft) - mu[w] * N) <= 1e-13 * mu[w] * N
                assert np.abs(kt[w] * r["xi"][0, w] + gt[w] * vt + Ft).max() <= 1e-13 * mu[w] * N
            else:
                assert kind == H.STICK
                assert np.abs(kt[w] * r["xi"][0, w] + gt[w] * vt + Ft).max() <= 1e-13 * max(mu[w] * N, np.abs(gt[w] * vt).max())
    assert kinds == {H.STICK, H.SLIDE}


def test_a_look_leaves_the_state_and_forms_the_force_of_the_stored_xi(corner):
    a, tw, co, kt = corner
    xi, live = _state(5, 1e-3)
    live[0, 1] = False
    look = H.wall_forces_history(*a, tw, *co, kt, np.zeros((3, 3)), xi, live, 0.0)
    assert np.array_equal(look["xi"], xi) and np.array_equal(look["live"], live)
    dead = xi.copy()
    dead[0, 1] = 0.0                                    # a xi that is not live reads as 0
    again = H.wall_forces_history(*a, tw, *co, kt, np.zeros((3, 3)), dead, np.array([[True, True, True]]), 0.0)
    assert np.array_equal(look["f"], again["f"]) and np.array_equal(look["torque"], again["torque"])


def test_a_common_velocity_of_wall_and_particle_leaves_xi_unchanged(corner):
    a, tw, co, kt = corner
    u = np.array([0.7, -1.1, 0.9])
    planes = co[0]
    xi, live = _state(6, 1e-3)
    for w in range(3):                                  # a stored xi lies in its wall's plane
        xi[0, w] -= (xi[0, w] @ planes[w, :3]) * planes[w, :3]
    common = H.wall_forces_history(*a, np.array([[*u, 0.0, 0.0, 0.0]]), *co, kt, np.broadcast_to(u, (3, 3)), xi, live, 1e-3)
    rest = H.wall_forces_history(*a, np.zeros((1, 6)), *co, kt, np.zeros((3, 3)), xi, live, 1e-3)
    for w in (0, 1):
        assert common["kind"][0, w] == H.STICK
        assert np.array_equal(common["xi"][0, w], xi[0, w])
    for k in ("f", "torque", "wall_out", "xi"):
        assert np.array_equal(common[k], rest[k]), k


def test_constant_tangential_velocity_draws_the_closed_form_hysteresis_loop():
    """The law alone (no shape): F_t = -k_t K dt v_t until mu N, then |xi| = mu N / k_t, then unloading at the reversed
    velocity with slope k_t."""
    n = np.array([0.0, 0.0, 1.0])
    vt = np.array([0.3, -0.4, 0.0])                     # |v_t| = 0.5
    kt, mu, N, dt = 2000.0, 0.5, 40.0, 1e-3             # mu N = 20: reached after 20 passes of k_t dt |v_t| = 1
    xi = np.zeros(3)
    for K in range(1, 31):
        Ft, xi, kind = H.spring_law(xi, vt, n, N, mu, 0.0, kt, dt)
        if K <= 19:
            assert kind == H.STICK and np.abs(Ft + kt * K * dt * vt).max() <= 1e-12 * mu * N
        elif K >= 21:
            assert kind == H.SLIDE
            assert abs(np.linalg.norm(xi) - mu * N / kt) <= 1e-15 and abs(np.linalg.norm(Ft) - mu * N) <= 1e-12
            assert np.abs(Ft / (mu * N) + vt / 0.5).max() <= 1e-14          # against the motion
    top = xi.copy()
    for K in range(1, 41):                              # back: 40 passes take k_t xi from +mu N to -mu N
        Ft, xi, kind = H.spring_law(xi, -vt, n, N, mu, 0.0, kt, dt)
        if K <= 39:
            assert kind == H.STICK
            assert np.abs(Ft + kt * (top - K * dt * vt)).max() <= 1e-12 * mu * N     # slope k_t from the turning point
    for K in range(3):
        Ft, xi, kind = H.spring_law(xi, -vt, n, N, mu, 0.0, kt, dt)
        assert kind == H.SLIDE and abs(np.linalg.norm(xi) - mu * N / kt) <= 1e-15
        assert np.abs(Ft / (mu * N) - vt / 0.5).max() <= 1e-14
