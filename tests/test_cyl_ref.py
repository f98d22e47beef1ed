"""CPU pins of tests/cyl_ref.py, the numpy restatement of docs/SPEC.md §2.18 that the GPU cylinder tests compare against:
the plane as the limit Rc -> infinity (sums and friction), the divergence-theorem identities in the cylinder's own
coordinates, a Monte-Carlo volume, the symmetries of the surface and the cap bound.  Passes on any tree that has the
reference: it pins the yardstick, not the kernels."""
import numpy as np
import pytest

import cyl_ref as Cy
import friction_ref as Fr
import wall_ref as W
from shpair import shapes


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def frame_e1(ch):
    """e1 of the frame rule of SPEC §2.3 about ch."""
    s = np.copysign(1.0, ch[2])
    a = -1.0 / (s + ch[2])
    return np.array([1 + s * ch[0] ** 2 * a, s * ch[0] * ch[1] * a, -s * ch[0]])


@pytest.fixture(scope="module")
def rough(oracle):
    """A random L = 6 shape, random orientation, an oblique axis, Rc = 2.5 Rmax, h = Rc - d = 0.7 Rmax."""
    anm = shapes.random_shape(6, 3, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    rng = np.random.default_rng(1)
    q = unit(rng.normal(size=4))
    ax = unit(rng.normal(size=3))
    ch = unit(np.cross(ax, rng.normal(size=3)))   # a radial direction
    a = np.array([0.4, -0.3, 0.2])
    Rc = 2.5 * rm
    return dict(anm=anm, rm=rm, q=q, ax=ax, ch=ch, a=a, Rc=Rc, d0=Rc - 0.7 * rm, cyl=np.array([*a, *ax, Rc]))


def at(r, d, along=0.0):
    return r["a"] + d * r["ch"] + along * r["ax"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_plane_is_the_limit_of_a_large_cylinder(oracle, seed):
    """Rc = 1e8 R_i and the same h: V, S_n, T_n agree with wall_ref.wall_sums to 1e-6 relative (the curvature scale R_i / Rc
    is 1e-8: a margin of 100).  The axis is the e1 of the plane's frame, so both rules place the same azimuths; no node of
    these seeds sits within 1e-5 of the boundary (checked), so none changes sides."""
    rng = np.random.default_rng(seed)
    anm = shapes.random_shape(6, 10 + seed, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    q, n = unit(rng.normal(size=4)), unit(rng.normal(size=3))
    h, nq = 0.7 * rm, 16
    x = n * h
    Vw, Sw, Tw, st = W.wall_sums(6, anm, rm, x, q, (*n, 0.0), nq)
    Rc = 1e8 * rm
    cyl = np.array([*(Rc * n), *frame_e1(-n), Rc])
    margin = []
    V, S, T, st2 = Cy.cyl_sums(6, anm, rm, x, q, cyl, nq, boundary=margin)
    assert st == 1 and st2 == 1 and Vw > 0
    print("seed %d: nearest node to the boundary %.2e; dV %.2e dS %.2e dT %.2e" %
          (seed, min(margin), abs(V / Vw - 1), np.abs(S - Sw).max() / np.abs(Sw).max(), np.abs(T - Tw).max() / np.abs(Tw).max()))
    assert min(margin) > 1e-5
    assert abs(V / Vw - 1) <= 1e-6
    assert np.abs(S - Sw).max() <= 1e-6 * np.abs(Sw).max() and np.abs(T - Tw).max() <= 1e-6 * np.abs(Tw).max()


def test_force_is_minus_energy_gradient(rough):
    """kn = m = 1, so E = V and F = -S_n: F.c^ against -dE/dd, the central difference of V in d (step 1e-4), at n_q = 32.
    Measured 6.28e-4 relative; bar 1.3e-3 (twice that).  The plane's figure (tests/test_wall_ref.py) is 2.0e-3."""
    r, nq, e = rough, 32, 1e-4
    f = lambda d: Cy.cyl_sums(6, r["anm"], r["rm"], at(r, d), r["q"], r["cyl"], nq)
    V, S, T, st = f(r["d0"])
    dV = (f(r["d0"] + e)[0] - f(r["d0"] - e)[0]) / (2 * e)
    F = Cy.contact_wrench(V, S, T, at(r, r["d0"]), r["cyl"], 1.0, 1.0)[0]
    rel = abs(F @ r["ch"] / -dV - 1)
    print("F.c %.6f  -dE/dd %.6f  rel %.2e" % (F @ r["ch"], -dV, rel))
    assert st == 1 and V > 0 and dV > 0   # deeper as d grows, and the wall pushes back towards the axis
    assert rel <= 1.3e-3


def test_torque_is_minus_energy_gradient(rough):
    """tau.a^ = -dE/dtheta for a rotation of the particle about the axis direction through x_i; with kn = m = 1 this is
    T_n.a^ = dV/dtheta.  Central difference with step 1e-4 at n_q = 32: measured 2.92e-9 relative; bar 6e-9 (twice that).
    No node changes sides within the step here and r_in does not depend on theta, so T_n.a^ is the exact derivative of
    the discrete sum and what is left is the truncation of the difference; the plane's figure, 3.3e-4, has a crossing."""
    r, nq, e = rough, 32, 1e-4
    def vol(th):
        dq = np.array([np.cos(th / 2), *(np.sin(th / 2) * r["ax"])])
        return Cy.cyl_sums(6, r["anm"], r["rm"], at(r, r["d0"]), qmul(dq, r["q"]), r["cyl"], nq)
    V, S, T, _ = vol(0.0)
    dV = (vol(e)[0] - vol(-e)[0]) / (2 * e)
    rel = abs(T @ r["ax"] / dV - 1)
    print("T.a %.6e  dV/dtheta %.6e  rel %.2e  |T| %.3e" % (T @ r["ax"], dV, rel, np.linalg.norm(T)))
    assert abs(dV) > 0.1 * np.linalg.norm(T)   # the axis is not nearly orthogonal to the torque
    assert rel <= 6e-9


def test_volume_against_monte_carlo(oracle, rough):
    """V against the Monte-Carlo volume of {p inside the particle, outside the cylinder}, within 3 standard errors (2e5
    samples of a box around the cap of the bounding ball)."""
    r = rough
    x = at(r, r["d0"])
    V = Cy.cyl_sums(6, r["anm"], r["rm"], x, r["q"], r["cyl"], 32)[0]
    rng = np.random.default_rng(5)
    N = 200000
    R = W.quat_to_mat(r["q"])
    rm, h = r["rm"], r["Rc"] - r["d0"]
    # the wall curves towards the particle, so the overlap is NOT confined to c^-coordinates beyond h; the cap is what
    # bounds it: every point of it lies in a direction with u.c^ >= cos alpha, within R_i
    ca = Cy.cap_cos(r["Rc"], r["d0"], rm)
    half = rm * np.sqrt(1 - ca * ca)
    h, depth = rm * ca, rm * (1 - ca)
    ez, ex = r["ch"], r["ax"]
    ey = np.cross(ez, ex)
    p = (rng.uniform(-half, half, N)[:, None] * ex + rng.uniform(-half, half, N)[:, None] * ey +
         (h + rng.uniform(0, depth, N))[:, None] * ez)   # relative to x_i
    y = (x - r["a"]) + p
    rad = np.linalg.norm(y - (y @ r["ax"])[:, None] * r["ax"], axis=1)
    dist = np.linalg.norm(p, axis=1)
    cand = np.nonzero((dist < rm) & (rad > r["Rc"]))[0]
    hits = sum(1 for k in cand if dist[k] < oracle.sh_eval(6, r["anm"], R.T @ (p[k] / dist[k])))
    box = (2 * half) ** 2 * depth
    frac = hits / N
    mc, se = box * frac, box * np.sqrt(frac * (1 - frac) / N)
    print("V %.6e  MC %.6e +- %.1e (%d hits)" % (V, mc, se, hits))
    assert hits > 100 and abs(V - mc) <= 3 * se


def test_sphere_has_no_axial_force_and_no_torque(rough):
    """A unit sphere (Rmax 1.01) in an oblique cylinder: the force is radial: its axial part and the torque are 0 to 1e-12
    of |F|."""
    r = rough
    cyl = np.array([*r["a"], *r["ax"], 3.0])
    for h in (0.8, 0.9, 0.95):
        x = r["a"] + (3.0 - h) * r["ch"] + 0.7 * r["ax"]
        V, S, T, st = Cy.cyl_sums(0, shapes.sphere(1.0), 1.01, x, (1, 0, 0, 0), cyl, 16)
        F, tau, E, _ = Cy.contact_wrench(V, S, T, x, cyl, 1000.0, 1.25)
        fn = np.linalg.norm(F)
        print("h %.2f: |F| %.4g  axial %.1e  torque %.1e" % (h, fn, abs(F @ r["ax"]) / fn, np.abs(tau).max() / fn))
        assert st == 1 and V > 0 and F @ r["ch"] < 0
        assert abs(F @ r["ax"]) <= 1e-12 * fn and np.abs(tau).max() <= 1e-12 * fn


def test_screw_motion_about_the_axis_rotates_the_wrench(rough):
    """The surface is invariant under a translation along the axis and a rotation about it, and the frame (a^, c^ x a^, c^)
    moves with the particle: the moved particle has the rotated wrench to 1e-12."""
    r, nq = rough, 16
    x = at(r, r["d0"], along=0.3)
    V, S, T, _ = Cy.cyl_sums(6, r["anm"], r["rm"], x, r["q"], r["cyl"], nq)
    F, tau, E, _ = Cy.contact_wrench(V, S, T, x, r["cyl"], 1000.0, 1.25)
    th = 0.7391
    g = np.array([np.cos(th / 2), *(np.sin(th / 2) * r["ax"])])
    G = W.quat_to_mat(g)
    x2 = r["a"] + G @ (x - r["a"]) - 1.7 * r["ax"]
    V2, S2, T2, _ = Cy.cyl_sums(6, r["anm"], r["rm"], x2, qmul(g, r["q"]), r["cyl"], nq)
    F2, tau2, E2, _ = Cy.contact_wrench(V2, S2, T2, x2, r["cyl"], 1000.0, 1.25)
    sc = np.linalg.norm(F)
    print("screw: dE %.1e dF %.1e dtau %.1e" % (abs(E2 / E - 1), np.abs(F2 - G @ F).max() / sc, np.abs(tau2 - G @ tau).max() / sc))
    assert abs(E2 / E - 1) <= 1e-12 and np.abs(F2 - G @ F).max() <= 1e-12 * sc and np.abs(tau2 - G @ tau).max() <= 1e-12 * sc


def test_no_direction_outside_the_cap_reaches_the_wall():
    """10^4 random directions with u.c^ < cos alpha, at r = R_i, over random (Rc, d, R_i): (q r + 2 b) r > g never holds.
    And the plane's h / R_i is no bound: directions between the two caps do reach the wall."""
    rng = np.random.default_rng(7)
    tried = beyond_plane_cap = 0
    while tried < 10000:
        R = rng.uniform(0.5, 2.0)
        Rc = R * rng.uniform(0.6, 6.0)
        d = rng.uniform(max(0.0, Rc - R), Rc) * (1 - 1e-9)
        if not Rc - d < R:
            continue
        ca = Cy.cap_cos(Rc, d, R)
        g = (Rc - d) * (Rc + d)
        u = unit(rng.normal(size=3))          # c^ = z, a^ = x
        inside = ((1 - u[0] ** 2) * R + 2 * d * u[2]) * R > g
        if u[2] < ca:
            tried += 1
            assert not inside, (Rc, d, R, u)
        elif inside and u[2] < (Rc - d) / R:
            beyond_plane_cap += 1
    print("directions inside the wall but outside the plane's cap h / R_i: %d" % beyond_plane_cap)
    assert beyond_plane_cap > 0


def _wall_law(V, S, T, n, h, tw, mu, gt):
    """tests/friction_ref.py's wall law on given sums (kn 1000, m 1.25, gamma 3)."""
    p = 1000.0 * 1.25 * V ** 0.25
    pt = max(0.0, p + 3.0 * (S @ tw[:3] + T @ tw[3:]))
    ri = Fr.wall_contact_point(S, T, n, h)
    vrel = tw[:3] + np.cross(tw[3:], ri)
    Ft, _, capped = Fr.capped(vrel - (vrel @ n) * n, pt * np.linalg.norm(S), mu, gt)
    return -pt * S + Ft, -pt * T + np.cross(ri, Ft), Ft, ri, capped


def test_friction_is_the_wall_law_in_the_limit_of_a_large_cylinder(oracle):
    """Rc = 1e8 R_i: the contact point, F_t and the torque of §2.18 reproduce tests/friction_ref.py's wall law at the same
    contact to 1e-6, viscous and capped.  The two laws agree in the limit where S_n is along the wall normal: the plane
    drops r_perp onto the wall along n^, the cylinder follows the line of action along S^.  So the contacts are (a) a
    spinning unit sphere with its own sums (S_n along n^ by symmetry, to rounding) and (b) a rough L = 6 shape whose S_n is
    replaced by its normal part, T_n and V kept: r_perp, the cap and both branches are exercised.  (c) With the rough
    shape's own S_n the two contact points differ by (h + n^.r_perp) tan(phi) in the wall, phi the angle between S^ and the
    normal (quadrature noise; measured 7.4e-3 |r_i|); that distance is asserted instead."""
    rng = np.random.default_rng(11)
    tw = np.array([0.3, -0.2, 0.1, 0.5, 0.4, -0.6])
    seen = set()
    for label in ("sphere", "rough"):
        lmax, anm = (0, shapes.sphere(1.0)) if label == "sphere" else (6, shapes.random_shape(6, 12, amp=0.1))
        rm = 1.01 if label == "sphere" else oracle.shape_rmax(6, anm)
        q, n = unit(rng.normal(size=4)), unit(rng.normal(size=3))
        h, nq = 0.7 * rm, 16
        x = n * h
        Rc = 1e8 * rm
        cyl = np.array([*(Rc * n), *frame_e1(-n), Rc])
        V, S0, T, st = Cy.cyl_sums(lmax, anm, rm, x, q, cyl, nq)
        assert st == 1 and V > 0
        S = S0 if label == "sphere" else (S0 @ n) * n
        for mu, gt in ((0.5, 2.0), (0.5, 2000.0), (0.01, 2000.0)):
            F, tau, E, det = Cy.contact_wrench(V, S, T, x, cyl, 1000.0, 1.25, tw, gamma=3.0, mu=mu, gt=gt)
            Fw, tauw, Ft, ri, capped = _wall_law(V, S, T, n, h, tw, mu, gt)
            seen.add(capped)
            err = (np.abs(det["ri"] - ri).max() / np.linalg.norm(ri), np.abs(det["Ft"] - Ft).max() / np.linalg.norm(Ft),
                   np.abs(F - Fw).max() / np.linalg.norm(Fw), np.abs(tau - tauw).max() / max(np.linalg.norm(tauw), np.linalg.norm(Fw)))
            print("%s mu %g gamma_t %g capped %s: dri %.1e dFt %.1e dF %.1e dtau %.1e" % (label, mu, gt, capped, *err))
            assert det["capped"] == capped and np.linalg.norm(Ft) > 0
            assert max(err) <= 1e-6
        if label == "rough":   # (c)
            F, tau, E, det = Cy.contact_wrench(V, S0, T, x, cyl, 1000.0, 1.25, tw, gamma=3.0, mu=0.5, gt=2.0)
            ri = Fr.wall_contact_point(S0, T, n, h)
            rp = np.cross(S0, T) / (S0 @ S0)
            cosphi = -(S0 @ n) / np.linalg.norm(S0)
            want = (h + n @ rp) * np.sqrt(1 - cosphi ** 2) / cosphi
            got = np.linalg.norm(det["ri"] - ri)
            print("rough, own S_n: |dri| %.6e, (h + n.r_perp) tan phi %.6e, of |r_i| %.1e" % (got, want, got / np.linalg.norm(ri)))
            assert abs(got - want) <= 1e-6 * np.linalg.norm(ri) and abs((det["ri"] - ri) @ n) <= 1e-6 * np.linalg.norm(ri)
    assert seen == {True, False}


def test_signs_limits_and_the_axis(rough):
    r = rough
    # out of reach: zeros; at or outside the wall: nothing, flagged
    for d, want in ((r["Rc"] - 1.0001 * r["rm"], 0), (0.2 * r["rm"], 0), (r["Rc"], -1), (1.2 * r["Rc"], -1), (np.nan, -1)):
        V, S, T, st = Cy.cyl_sums(6, r["anm"], r["rm"], at(r, d), r["q"], r["cyl"], 16)
        assert st == want and V == 0 and not S.any() and not T.any(), d
    # a centre exactly on the axis of a narrow cylinder (Rmax > Rc): the whole sphere is the cap, the fallback frame is
    # perpendicular to the axis, and a unit sphere feels no net force
    cyl = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.9])
    rho, d, ch = Cy.foot([0.0, 0.0, 2.5], cyl)
    assert d == 0 and abs(ch @ cyl[3:6]) <= 1e-15 and abs(np.linalg.norm(ch) - 1) <= 1e-15
    assert Cy.cap_cos(0.9, 0.0, 1.01) == -1.0
    V, S, T, st = Cy.cyl_sums(0, shapes.sphere(1.0), 1.01, [0.0, 0.0, 2.5], (1, 0, 0, 0), cyl, 16)
    assert st == 1 and V > 0 and np.abs(S).max() <= 1e-12 * V and np.abs(T).max() <= 1e-12 * V
