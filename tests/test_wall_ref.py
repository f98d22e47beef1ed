"""CPU pins of tests/wall_ref.py, the numpy restatement of docs/SPEC.md §2.9 that the GPU wall tests compare against:
closed forms for a sphere, the divergence-theorem identities (S_n.n = dV/dh, T_n.a = dV/dtheta), a Monte-Carlo volume,
signs, limits and invariances.  Passes on any tree by construction: it pins the yardstick, not the kernels."""
import numpy as np
import pytest

import wall_ref as W
from shpair import shapes


def qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


@pytest.fixture(scope="module")
def rough(oracle):
    """A random L = 6 shape, random orientation, oblique normal, h = 0.85 Rmax."""
    anm = shapes.random_shape(6, 3, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    rng = np.random.default_rng(1)
    q = unit(rng.normal(size=4))
    n = unit(rng.normal(size=3))
    ax = unit(rng.normal(size=3))
    return dict(anm=anm, rm=rm, q=q, n=n, ax=ax, h0=0.85 * rm)


def test_sphere_closed_forms(oracle):
    """Unit sphere, Rmax = 1.01, h in {0.8, 0.85, 0.9, 0.95}, n_q in {16, 32}: V = pi (R-h)^2 (2R+h)/3, A_c = pi (R^2-h^2).
    Measured worst over this grid: |V/V_exact - 1| = 5.8e-4 (h = 0.95, n_q = 16), ||S_n.n|/A_c - 1| = 1.08e-2 (h = 0.9,
    n_q = 16; the sharp rule is first order and not monotone in n_q), tangential S_n and T_n 2.1e-17.  Bars 2e-3, 2e-2,
    1e-14."""
    a = shapes.sphere(1.0)
    worst = [0.0, 0.0, 0.0]
    for h in (0.8, 0.85, 0.9, 0.95):
        for nq in (16, 32):
            V, S, T, st = W.wall_sums(0, a, 1.01, np.array([0.2, -0.1, h + 0.3]), (1, 0, 0, 0), (0, 0, 1, 0.3), nq)
            assert st == 1
            Ve, Ae = np.pi * (1 - h) ** 2 * (2 + h) / 3, np.pi * (1 - h * h)
            worst[0] = max(worst[0], abs(V / Ve - 1))
            worst[1] = max(worst[1], abs(-S[2] / Ae - 1))
            worst[2] = max(worst[2], np.abs(S[:2]).max(), np.abs(T).max())
    print("sphere worst: V %.2e  S %.2e  vanishing parts %.2e" % tuple(worst))
    assert worst[0] <= 2e-3 and worst[1] <= 2e-2 and worst[2] <= 1e-14


def test_force_is_minus_energy_gradient(rough):
    """S_n.n against the central difference of V in h (step 1e-4) at n_q = 32: measured 2.0e-3 relative, bar 1e-2."""
    r, nq, e = rough, 32, 1e-4
    f = lambda h: W.wall_sums(6, r["anm"], r["rm"], r["n"] * h, r["q"], (*r["n"], 0.0), nq)
    V, S, T, _ = f(r["h0"])
    dV = (f(r["h0"] + e)[0] - f(r["h0"] - e)[0]) / (2 * e)
    print("S.n %.6f  dV/dh %.6f  rel %.2e" % (S @ r["n"], dV, abs(S @ r["n"] / dV - 1)))
    assert V > 0 and dV < 0
    assert abs(S @ r["n"] / dV - 1) <= 1e-2


def test_torque_is_minus_energy_gradient(rough):
    """tau.a = -dE/dtheta for a rotation of the particle about a random axis a through x_i; with kn = m = 1 this is
    T_n.a = dV/dtheta.  Central difference with step 1e-4 at n_q = 32: measured 3.3e-4 relative (1.9e-3 with step 1e-3),
    same bar as the force check, 1e-2."""
    r, nq, e = rough, 32, 1e-4
    def vol(th):
        dq = np.array([np.cos(th / 2), *(np.sin(th / 2) * r["ax"])])
        return W.wall_sums(6, r["anm"], r["rm"], r["n"] * r["h0"], qmul(dq, r["q"]), (*r["n"], 0.0), nq)
    V, S, T, _ = vol(0.0)
    dV = (vol(e)[0] - vol(-e)[0]) / (2 * e)
    F, tau, E = W.force_law(V, S, T, 1.0, 1.0)
    print("tau.a %.6e  -dE/dtheta %.6e  rel %.2e" % (tau @ r["ax"], -dV, abs(tau @ r["ax"] / -dV - 1)))
    assert abs(dV) > 0.1 * np.linalg.norm(T)   # the axis is not nearly orthogonal to the torque
    assert abs(tau @ r["ax"] / -dV - 1) <= 1e-2


def test_volume_against_monte_carlo(oracle, rough):
    """V against the Monte-Carlo volume of {p inside the particle, n.p < c}: 3 standard errors + 2e-3 relative
    (2e5 samples of a box around the cap of the bounding ball: one standard error is 3.6 % of V)."""
    r = rough
    V = W.wall_sums(6, r["anm"], r["rm"], r["n"] * r["h0"], r["q"], (*r["n"], 0.0), 32)[0]
    rng = np.random.default_rng(5)
    N = 200000
    # sample the slab of the bounding ball behind the plane: a box around the cap, in a frame with z along -n
    R = W.quat_to_mat(r["q"])
    rm, h = r["rm"], r["h0"]
    half = np.sqrt(rm * rm - h * h)
    depth = rm - h
    ez = -r["n"]
    ex = unit(np.cross(ez, [1.0, 0.0, 0.0]))
    ey = np.cross(ez, ex)
    p = (rng.uniform(-half, half, N)[:, None] * ex + rng.uniform(-half, half, N)[:, None] * ey +
         (h + rng.uniform(0, depth, N))[:, None] * ez)   # relative to x_i; all of them behind the plane
    d = np.linalg.norm(p, axis=1)
    hits = sum(1 for k in np.nonzero(d < rm)[0] if d[k] < oracle.sh_eval(6, r["anm"], R.T @ (p[k] / d[k])))
    box = (2 * half) ** 2 * depth
    frac = hits / N
    mc, se = box * frac, box * np.sqrt(frac * (1 - frac) / N)
    print("V %.6e  MC %.6e +- %.1e" % (V, mc, se))
    assert abs(V - mc) <= 3 * se + 2e-3 * V


def test_signs_and_limits(rough):
    r = rough
    # a particle resting on a floor is pushed along +n
    V, S, T, st = W.wall_sums(6, r["anm"], r["rm"], [0.3, 0.4, 0.8 * r["rm"]], r["q"], (0, 0, 1, 0.0), 16)
    F, tau, E = W.force_law(V, S, T, 1000.0, 1.25)
    assert st == 1 and V > 0 and F[2] > 0 and abs(F[2]) > 10 * np.abs(F[:2]).max() and E > 0
    # out of reach: zeros; at or behind the plane: nothing, flagged
    for h, want in ((r["rm"], 0), (1.5 * r["rm"], 0), (0.0, -1), (-0.2, -1), (np.nan, -1)):
        V, S, T, st = W.wall_sums(6, r["anm"], r["rm"], [0.0, 0.0, h], r["q"], (0, 0, 1, 0.0), 16)
        assert st == want and V == 0 and not S.any() and not T.any()


def test_translation_and_rotation_invariance(rough):
    """Shifting particle and plane together, or rotating both by the same rotation, changes V by no more than 1e-13 and
    rotates F, tau with it."""
    r, nq = rough, 16
    x = r["n"] * r["h0"] + np.array([0.3, -0.2, 0.1])
    c = r["n"] @ np.array([0.3, -0.2, 0.1])
    V, S, T, _ = W.wall_sums(6, r["anm"], r["rm"], x, r["q"], (*r["n"], c), nq)
    sh = np.array([1.7, -2.3, 0.9])
    V2, S2, T2, _ = W.wall_sums(6, r["anm"], r["rm"], x + sh, r["q"], (*r["n"], c + r["n"] @ sh), nq)
    assert abs(V2 - V) <= 1e-13 and np.abs(S2 - S).max() <= 1e-13 and np.abs(T2 - T).max() <= 1e-13
    # a rotation about the wall normal by a multiple of the azimuth step pi / n_q maps the node set onto itself: 1e-13
    th = 5 * np.pi / nq
    g = np.array([np.cos(th / 2), *(np.sin(th / 2) * r["n"])])
    G = W.quat_to_mat(g)
    V3, S3, T3, _ = W.wall_sums(6, r["anm"], r["rm"], G @ x, qmul(g, r["q"]), (*(G @ r["n"]), c), nq)
    assert abs(V3 - V) <= 1e-13 and np.abs(S3 - G @ S).max() <= 1e-13 and np.abs(T3 - G @ T).max() <= 1e-13
    # any other rotation: the frame of SPEC §2.3 is a function of c alone, not covariant, so the rotated configuration
    # places its azimuths elsewhere on the same rings: another quadrature of the same integrals.  It agrees at the
    # quadrature error (the sphere bars above: 2e-3 on V, 2e-2 on S_n), not at rounding.  Measured at n_q = 64:
    # dV/V 6.4e-6, dS 6.4e-3, dT 1.2e-3 of |S_n|.
    g = unit([0.9, 0.1, -0.3, 0.25])
    G = W.quat_to_mat(g)
    Va, Sa, Ta, _ = W.wall_sums(6, r["anm"], r["rm"], x, r["q"], (*r["n"], c), 64)
    Vb, Sb, Tb, _ = W.wall_sums(6, r["anm"], r["rm"], G @ x, qmul(g, r["q"]), (*(G @ r["n"]), c), 64)
    print("rotation: dV/V %.2e  dS %.2e  dT %.2e" % (abs(Vb / Va - 1), np.abs(Sb - G @ Sa).max() / np.abs(Sa).max(),
                                                    np.abs(Tb - G @ Ta).max() / np.abs(Sa).max()))
    assert abs(Vb / Va - 1) <= 2e-3 and np.abs(Sb - G @ Sa).max() <= 2e-2 * np.abs(Sa).max()
    assert np.abs(Tb - G @ Ta).max() <= 2e-2 * np.abs(Sa).max()
