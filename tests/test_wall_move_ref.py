"""CPU pins of tests/wall_move_ref.py, the numpy restatement of docs/SPEC.md §2.12 that the GPU moving-wall tests compare
against: it is the friction reference when nothing moves, a wall velocity is a shift of the particle's linear velocity,
and the kinematic claim behind both — displacing the plane along u changes V at the rate -S_n.u.  Passes on any tree that
has the reference: it pins the yardstick, not the kernels."""
import numpy as np
import pytest

import friction_ref as F
import wall_move_ref as M
import wall_ref as W
from shpair import shapes

S3 = 1.0 / np.sqrt(3.0)


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


@pytest.fixture(scope="module")
def corner(oracle):
    """One L = 4 particle in a corner of three walls, n_q = 8: coefficients of the size tests/test_gpu_friction.py uses."""
    anm = shapes.random_shape(4, 3, amp=0.1)
    sh = [(4, anm, oracle.shape_rmax(4, anm))]
    planes = np.array([[1.0, 0, 0, 0.0], [0, 1.0, 0, 0.0], [0, 0, 1.0, 0.0]])
    a = (sh, 8, np.array([[0.8, 0.9, 0.7]]), np.array([[0.5, 0.5, -0.5, 0.5]]), np.zeros(1, np.int32))
    tw = np.array([[0.35, -0.6, -0.25, 0.5, 0.8, -0.7]])
    co = (planes, np.array([1000.0, 800.0, 1200.0]), np.array([1.25, 1.0, 2.0]), np.array([400.0, 250.0, 600.0]),
          np.array([0.5, 0.1, 0.6]), np.array([200.0, 400.0, 100.0]))
    return a, tw, co


def test_without_a_velocity_it_is_the_friction_reference_exactly(corner):
    a, tw, co = corner
    got = M.wall_forces_moving(*a, tw, *co, np.zeros((3, 3)))
    ref = F.wall_forces_friction(*a, tw, *co)
    assert len(ref["contacts"]) == 3 and np.abs(ref["f"]).max() > 0
    for k in ("f", "torque", "wall_out"):
        assert np.array_equal(got[k], ref[k]), k
    for c, d in zip(got["contacts"], ref["contacts"]):
        assert c[:5] == d[:5] and np.array_equal(c[5], d[5]) and np.array_equal(c[6], d[6]) and c[7] == d[7]


def test_a_common_wall_velocity_is_a_shift_of_the_particles_velocity(corner):
    """(tw, u) == (tw - (u, 0), 0) to rounding — and a common translation of particle and walls gives the elastic force."""
    a, tw, co = corner
    u = np.array([0.7, -1.1, 0.9])
    moved = M.wall_forces_moving(*a, tw, *co, np.broadcast_to(u, (3, 3)))
    shifted = M.wall_forces_moving(*a, tw - np.concatenate([u, np.zeros(3)]), *co, np.zeros((3, 3)))
    still = M.wall_forces_moving(*a, tw, *co, np.zeros((3, 3)))
    scale = np.abs(still["f"]).max()
    for k in ("f", "torque", "wall_out"):
        assert np.abs(moved[k] - shifted[k]).max() <= 1e-14 * max(scale, np.abs(still[k]).max()), k
    assert np.abs(moved["f"] - still["f"]).max() > 1e-2 * scale          # the velocity did matter
    # frame indifference: particle and walls translating together, no spin
    co_t = (co[0], co[1], co[2], co[3], co[4], co[5])
    common = M.wall_forces_moving(*a, np.array([[*u, 0.0, 0.0, 0.0]]), *co_t, np.broadcast_to(u, (3, 3)))
    rest = M.wall_forces_moving(*a, np.zeros((1, 6)), *co_t, np.zeros((3, 3)))
    for k in ("f", "torque", "wall_out"):
        assert np.array_equal(common[k], rest[k]), k
    assert all(not c[5].any() for c in common["contacts"])               # no v_rel: no friction


def test_a_tangential_velocity_never_moves_the_plane():
    planes = np.array([[0.0, 0, 1, 0.25], [S3, S3, S3, -1.5], [1.0, 0, 0, 2.0]])
    vel = np.array([[-1.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.0, 3.0, -2.0]])
    assert not M.normal_speed(planes, vel).any()
    assert np.array_equal(M.advance(planes, vel, 1e-4, 1000), planes)
    # a normal part moves it by the accumulation, which is k dt (n.u) to k roundings
    vel[1] = [0.3, -0.2, 0.5]
    out = M.advance(planes, vel, 1e-4, 1000)
    assert np.array_equal(out[:, :3], planes[:, :3]) and out[0, 3] == planes[0, 3] and out[2, 3] == planes[2, 3]
    nu = S3 * 0.6
    assert abs(out[1, 3] - (-1.5 + 1000 * 1e-4 * nu)) <= 1e-15 * 1000 * 1.5


def test_displacing_the_plane_along_u_changes_the_volume_at_minus_sn_dot_u(oracle):
    """The kinematic claim of §2.12 on the oblique L = 6 case of tests/test_wall_ref.py at n_q = 32: the central difference
    of V under a plane displacement eps (n.u) n against -S_n.u, at the bar that file uses for S_n.n against dV/dh (1e-2
    relative: the sharp rule's S_n carries a tangential part of relative size ~2e-3 that a plane's true V does not see).
    u has a normal and a tangential part of order 1."""
    anm = shapes.random_shape(6, 3, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    rng = np.random.default_rng(1)
    q, n, ax = unit(rng.normal(size=4)), unit(rng.normal(size=3)), unit(rng.normal(size=3))
    h0, nq, e = 0.85 * rm, 32, 1e-4
    u = 0.8 * n + 0.6 * unit(np.cross(n, ax))
    vol = lambda eps: W.wall_sums(6, anm, rm, n * h0, q, (*n, eps * (n @ u)), nq)
    V, S, T, st = vol(0.0)
    dV = (vol(e)[0] - vol(-e)[0]) / (2 * e)
    print("-S.u %.6f  dV/deps %.6f  rel %.2e" % (-S @ u, dV, abs(-S @ u / dV - 1)))
    assert st == 1 and V > 0 and dV > 0            # the wall advances into the particle: the overlap grows
    assert abs(-S @ u / dV - 1) <= 1e-2
