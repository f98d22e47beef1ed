"""CPU pins of tests/cone_ref.py, the numpy restatement of docs/SPEC.md §2.22 that the GPU cone tests compare against:
the cylinder as the limit theta -> 0 with the apex far away (sums and friction), the plane as the limit theta -> pi/2, the
energy gradients of an oblique cone, a Monte-Carlo volume, the symmetries of the surface, the cap bound and the exit
root.  Passes on any tree that has the reference: it pins the yardstick, not the kernels."""
import numpy as np
import pytest

import cone_ref as Co
import cyl_ref as Cy
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


def place(co, ch, t, d):
    """The point at axial coordinate t and radius d along the radial direction ch."""
    return co[:3] + t * co[3:6] + d * ch


@pytest.fixture(scope="module")
def rough(oracle):
    """A random L = 6 shape, random orientation, an oblique axis, theta = 30 degrees, local radius 2.5 Rmax (the radius of
    the cone at the centre's axial coordinate), h = 0.7 Rmax."""
    anm = shapes.random_shape(6, 3, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    rng = np.random.default_rng(1)
    q = unit(rng.normal(size=4))
    ax = unit(rng.normal(size=3))
    ch = unit(np.cross(ax, rng.normal(size=3)))   # a radial direction
    th = np.pi / 6
    co = Co.cone([0.4, -0.3, 0.2], ax, th)
    t0 = 2.5 * rm / np.tan(th)
    d0 = (np.sin(th) * t0 - 0.7 * rm) / np.cos(th)
    gen, _, nh = Co.frame(co, ch)
    return dict(anm=anm, rm=rm, q=q, ax=ax, ch=ch, co=co, th=th, t0=t0, d0=d0, nh=nh, x0=place(co, ch, t0, d0))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_cylinder_is_the_limit_of_a_slender_cone(oracle, seed):
    """theta = 2.5e-8 and the apex 1e8 R_i down the axis, so the local radius is 2.5 R_i; the same axis, radial direction
    and h = 0.7 R_i: V, S_n, T_n agree with cyl_ref.cyl_sums to 1e-6 relative (the taper over the particle is 2.5e-8 and
    the coordinates of the centre carry 1e8 R_i, whose rounding moves it by 1e-8 R_i; measured at most 3.7e-7 for the sums and 4.6e-7 for the
    laws: a margin of 2), and so does the friction law, viscous and capped, with Omega != 0.  No node of these seeds sits within 1e-5 of the boundary."""
    rng = np.random.default_rng(seed)
    anm = shapes.random_shape(6, 10 + seed, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    q, ax = unit(rng.normal(size=4)), unit(rng.normal(size=3))
    ch = unit(np.cross(ax, rng.normal(size=3)))
    th, nq = 2.5e-8, 16
    t0 = 1e8 * rm
    Rc = t0 * np.tan(th)
    co = Co.cone(-t0 * ax, ax, th)
    cyl = np.array([0.0, 0.0, 0.0, *ax, Rc])
    x = (Rc - 0.7 * rm) * ch
    margin = []
    V, S, T, st = Co.cone_sums(6, anm, rm, x, q, co, nq, boundary=margin)
    Vc, Sc, Tc, st2 = Cy.cyl_sums(6, anm, rm, x, q, cyl, nq)
    assert st == 1 and st2 == 1 and Vc > 0
    errs = (abs(V / Vc - 1), np.abs(S - Sc).max() / np.abs(Sc).max(), np.abs(T - Tc).max() / np.abs(Tc).max())
    print("seed %d: nearest node to the boundary %.2e; dV %.2e dS %.2e dT %.2e" % (seed, min(margin), *errs))
    assert min(margin) > 1e-5
    assert max(errs) <= 1e-6
    tw = np.array([0.3, -0.2, 0.1, 0.5, 0.4, -0.6])
    seen = set()
    for mu, gt in ((0.5, 2.0), (0.01, 2000.0)):
        F, tau, E, det = Co.contact_wrench(V, S, T, x, co, 1000.0, 1.25, tw, gamma=3.0, mu=mu, gt=gt, omega=1.7)
        Fc, tauc, Ec, detc = Cy.contact_wrench(Vc, Sc, Tc, x, cyl, 1000.0, 1.25, tw, gamma=3.0, mu=mu, gt=gt, omega=1.7)
        seen.add(det["capped"])
        fn = np.linalg.norm(Fc)
        err = (np.abs(det["ri"] - detc["ri"]).max() / np.linalg.norm(detc["ri"]), np.abs(det["Ft"] - detc["Ft"]).max() / np.linalg.norm(detc["Ft"]),
               np.abs(F - Fc).max() / fn, np.abs(tau - tauc).max() / max(np.linalg.norm(tauc), fn), abs(E / Ec - 1))
        print("  mu %g gamma_t %g capped %s: dri %.1e dFt %.1e dF %.1e dtau %.1e dE %.1e" % (mu, gt, det["capped"], *err))
        assert det["capped"] == detc["capped"] and np.linalg.norm(detc["Ft"]) > 0
        assert max(err) <= 1e-6
    assert seen == {True, False}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_plane_is_the_limit_of_a_wide_cone(oracle, seed):
    """theta = pi/2 - 1e-8: the cone opens to the half-space beyond the plane through the apex normal to the axis.  The
    apex lies one R_i to the side, along minus the e1 of the plane's frame, so that g^ -> c^ is that e1 and both rules
    place the same azimuths; the centre's axial coordinate is set so that h is the plane's.  V, S_n, T_n agree with
    wall_ref.wall_sums to 1e-6 relative (the curvature scale R_i / P is 1e-8; measured at most 4.3e-8: a margin of 20)."""
    rng = np.random.default_rng(seed)
    anm = shapes.random_shape(6, 10 + seed, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    q, n = unit(rng.normal(size=4)), unit(rng.normal(size=3))
    h, nq = 0.7 * rm, 16
    Vw, Sw, Tw, st = W.wall_sums(6, anm, rm, n * h, q, (*n, 0.0), nq)
    th = np.pi / 2 - 1e-8
    e1 = frame_e1(-n)
    co = Co.cone(-rm * e1, n, th)
    x = n * (h + np.cos(th) * rm) / np.sin(th)
    margin = []
    V, S, T, st2 = Co.cone_sums(6, anm, rm, x, q, co, nq, boundary=margin)
    assert st == 1 and st2 == 1 and Vw > 0
    errs = (abs(V / Vw - 1), np.abs(S - Sw).max() / np.abs(Sw).max(), np.abs(T - Tw).max() / np.abs(Tw).max())
    print("seed %d: h %.17g against %.17g; nearest node to the boundary %.2e; dV %.2e dS %.2e dT %.2e" %
          (seed, Co.foot(x, co)[4], h, min(margin), *errs))
    assert min(margin) > 1e-5
    assert max(errs) <= 1e-6


def test_force_is_minus_energy_gradient(rough):
    """kn = m = 1, so E = V and F = -S_n: F.n^ against -dE/dn, the central difference of V along the outward normal n^ of
    the nearest generator (step 1e-4), at n_q = 32.  Measured 3.06e-4 relative; bar 6.2e-4 (twice that).  The cylinder's
    figure (tests/test_cyl_ref.py) is 6.28e-4, the plane's 2.0e-3."""
    r, nq, e = rough, 32, 1e-4
    f = lambda s: Co.cone_sums(6, r["anm"], r["rm"], r["x0"] + s * r["nh"], r["q"], r["co"], nq)
    V, S, T, st = f(0.0)
    dV = (f(e)[0] - f(-e)[0]) / (2 * e)
    F = Co.contact_wrench(V, S, T, r["x0"], r["co"], 1.0, 1.0)[0]
    rel = abs(F @ r["nh"] / -dV - 1)
    print("F.n %.6f  -dE/dn %.6f  rel %.2e" % (F @ r["nh"], -dV, rel))
    assert st == 1 and V > 0 and dV > 0   # deeper as the centre moves towards the wall, and the wall pushes back
    assert rel <= 6.2e-4


def test_torque_is_minus_energy_gradient(rough):
    """tau.a^ = -dE/dphi for a rotation of the particle about the axis direction through x_i; with kn = m = 1 this is
    T_n.a^ = dV/dphi.  Central difference with step 1e-4 at n_q = 32: measured 2.77e-9 relative; bar 5.6e-9 (twice that).  As
    at the cylinder no node changes sides within the step and lambda1 does not depend on phi, so T_n.a^ is the exact
    derivative of the discrete sum and what is left is the truncation of the difference."""
    r, nq, e = rough, 32, 1e-4
    def vol(th):
        dq = np.array([np.cos(th / 2), *(np.sin(th / 2) * r["ax"])])
        return Co.cone_sums(6, r["anm"], r["rm"], r["x0"], qmul(dq, r["q"]), r["co"], nq)
    V, S, T, _ = vol(0.0)
    dV = (vol(e)[0] - vol(-e)[0]) / (2 * e)
    rel = abs(T @ r["ax"] / dV - 1)
    print("T.a %.6e  dV/dphi %.6e  rel %.2e  |T| %.3e" % (T @ r["ax"], dV, rel, np.linalg.norm(T)))
    assert abs(dV) > 0.1 * np.linalg.norm(T)   # the axis is not nearly orthogonal to the torque
    assert rel <= 5.6e-9


def test_volume_against_monte_carlo(oracle, rough):
    """V against the Monte-Carlo volume of {p inside the particle, outside the cone}, within 3 standard errors (2e5
    samples of a box around the cap of the bounding ball)."""
    r = rough
    x, co = r["x0"], r["co"]
    V = Co.cone_sums(6, r["anm"], r["rm"], x, r["q"], co, 32)[0]
    rng = np.random.default_rng(5)
    N = 200000
    R = W.quat_to_mat(r["q"])
    rm = r["rm"]
    ca = Co.cap_cos(co, r["t0"], r["d0"], rm)
    half = rm * np.sqrt(1 - ca * ca) if ca > 0 else rm
    lo, depth = rm * ca, rm * (1 - ca)
    gen, e2, nh = Co.frame(co, r["ch"])
    p = (rng.uniform(-half, half, N)[:, None] * gen + rng.uniform(-half, half, N)[:, None] * e2 +
         (lo + rng.uniform(0, depth, N))[:, None] * nh)   # relative to x_i
    y = (x - co[:3]) + p
    t = y @ r["ax"]
    rad = np.linalg.norm(y - t[:, None] * r["ax"], axis=1)
    dist = np.linalg.norm(p, axis=1)
    cand = np.nonzero((dist < rm) & ~(co[7] * t - co[6] * rad > 0))[0]
    hits = sum(1 for k in cand if dist[k] < oracle.sh_eval(6, r["anm"], R.T @ (p[k] / dist[k])))
    box = (2 * half) ** 2 * depth
    frac = hits / N
    mc, se = box * frac, box * np.sqrt(frac * (1 - frac) / N)
    print("V %.6e  MC %.6e +- %.1e (%d hits, %.2f standard errors)" % (V, mc, se, hits, abs(V - mc) / se))
    assert hits > 100 and abs(V - mc) <= 3 * se


def test_sphere_on_the_axis_has_an_axial_force_and_no_torque():
    """A unit sphere (Rmax 1.01) on the axis of a 30-degree cone (the axis along z, so that d = 0 as computed): the cap is
    the whole sphere about the axis, the nodes keep the symmetry of the contact, and the force is along the axis, towards
    the opening: no component of force or torque off the axis above 1e-12 |F|."""
    co = Co.cone([0.4, -0.3, 0.2], [0.0, 0.0, 1.0], np.pi / 6)
    ax = co[3:6]
    for h in (0.8, 0.9, 0.95):
        x = co[:3] + (h / co[7]) * ax
        assert Co.foot(x, co)[2] == 0.0
        V, S, T, st = Co.cone_sums(0, shapes.sphere(1.0), 1.01, x, (1, 0, 0, 0), co, 16)
        F, tau, E, _ = Co.contact_wrench(V, S, T, x, co, 1000.0, 1.25)
        fn = np.linalg.norm(F)
        off = F - (F @ ax) * ax
        print("h %.2f: |F| %.4g  off-axis %.1e  torque %.1e" % (h, fn, np.abs(off).max() / fn, np.abs(tau).max() / fn))
        assert st == 1 and V > 0 and F @ ax > 0
        assert np.abs(off).max() <= 1e-12 * fn and np.abs(tau).max() <= 1e-12 * fn


def test_rotation_about_the_axis_rotates_the_wrench(rough):
    """The surface is invariant under a rotation about its axis, and the frame (g^, c^ x a^, n^) moves with the particle:
    the rotated state has the rotated wrench to 1e-12, friction and a turning cone included."""
    r, nq = rough, 16
    x, co = r["x0"], r["co"]
    tw = np.array([0.3, -0.2, 0.1, 0.5, 0.4, -0.6])
    V, S, T, _ = Co.cone_sums(6, r["anm"], r["rm"], x, r["q"], co, nq)
    F, tau, E, det = Co.contact_wrench(V, S, T, x, co, 1000.0, 1.25, tw, gamma=3.0, mu=0.5, gt=2.0, omega=1.7)
    th = 0.7391
    g = np.array([np.cos(th / 2), *(np.sin(th / 2) * r["ax"])])
    G = W.quat_to_mat(g)
    x2 = co[:3] + G @ (x - co[:3])
    tw2 = np.concatenate([G @ tw[:3], G @ tw[3:]])
    V2, S2, T2, _ = Co.cone_sums(6, r["anm"], r["rm"], x2, qmul(g, r["q"]), co, nq)
    F2, tau2, E2, _ = Co.contact_wrench(V2, S2, T2, x2, co, 1000.0, 1.25, tw2, gamma=3.0, mu=0.5, gt=2.0, omega=1.7)
    sc = np.linalg.norm(F)
    print("rotation: dE %.1e dF %.1e dtau %.1e" % (abs(E2 / E - 1), np.abs(F2 - G @ F).max() / sc, np.abs(tau2 - G @ tau).max() / sc))
    assert np.linalg.norm(det["Ft"]) > 0
    assert abs(E2 / E - 1) <= 1e-12 and np.abs(F2 - G @ F).max() <= 1e-12 * sc and np.abs(tau2 - G @ tau).max() <= 1e-12 * sc


def test_no_direction_outside_the_cap_reaches_the_wall():
    """20 random centres in random cones (theta between 3 and 87 degrees), among them ones with h = 0.05 R_i and ones
    within 2 R_i of the apex; 10^4 random directions with u.n^ < cos alpha for each centre with a cap smaller than the
    sphere: the point at R_i along none of them is outside the cone (the interior is convex, so no nearer point is
    either).  And the plane's h / R_i is no bound: directions between the two caps do reach the wall."""
    rng = np.random.default_rng(7)
    centres = whole = beyond_plane_cap = 0
    while centres < 20:
        R = rng.uniform(0.5, 2.0)
        th = np.radians(rng.uniform(3.0, 87.0))
        co = Co.cone([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], th)
        kind = centres % 4
        h = 0.05 * R if kind == 0 else R * rng.uniform(0.05, 1.0)
        if kind == 1:      # within 2 R_i of the apex
            s = rng.uniform(0.0, 2.0) * R
        else:
            s = rng.uniform(0.0, 8.0) * R
        # the centre from its place s along the generator and its distance h from it
        t, d = np.cos(th) * s + np.sin(th) * h, np.sin(th) * s - np.cos(th) * h
        if d < 0 or not h < R:
            continue
        ca = Co.cap_cos(co, t, d, R)
        centres += 1
        if ca == -1.0:
            whole += 1
            continue
        ch = np.array([1.0, 0.0, 0.0])
        gen, e2, nh = Co.frame(co, ch)
        # 10^4 directions uniform over the sphere outside the cap, and as many over the whole sphere for the plane's cap
        un = rng.uniform(-1.0, ca, 10000)
        psi = rng.uniform(0, 2 * np.pi, 10000)
        sg = np.sqrt(1 - un * un)
        u = (sg * np.cos(psi))[:, None] * gen + (sg * np.sin(psi))[:, None] * e2 + un[:, None] * nh
        y = np.array([d, 0.0, t]) + R * u
        outside = ~(co[7] * y[:, 2] - co[6] * np.hypot(y[:, 0], y[:, 1]) > 0)
        assert not outside.any(), (th, t, d, R, ca)
        u = rng.normal(size=(10000, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        un = u @ nh
        y = np.array([d, 0.0, t]) + R * u
        outside = ~(co[7] * y[:, 2] - co[6] * np.hypot(y[:, 0], y[:, 1]) > 0)
        beyond_plane_cap += int((outside & (un < h / R)).sum())
    print("centres whose cap is the whole sphere: %d of 20; directions inside the wall but outside the plane's cap h / R_i: %d"
          % (whole, beyond_plane_cap))
    assert whole < 10 and beyond_plane_cap > 0


def test_the_exit_root_against_numpy_roots():
    """lambda1 = G / (B + sqrt(B^2 + A G)) against the roots of A lambda^2 + 2 B lambda - G = 0 from numpy.roots, for rays
    with A > 0 (the positive root), A < 0 and u.a^ < 0 (the smaller of two positive roots: the exit from the nappe towards
    the apex) and A < 0 and u.a^ > 0 (steeper than the generators, into the opening: never leaves); the exit point lies on
    the nappe, and every point before it inside."""
    rng = np.random.default_rng(3)
    seen = {"A>0": 0, "A<0 down": 0, "A<0 up": 0}
    th = np.radians(35.0)
    co = Co.cone([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], th)
    ct, st = co[6], co[7]
    while min(seen.values()) < 50:
        t = rng.uniform(0.5, 3.0)
        d = rng.uniform(0.0, 0.98) * t * np.tan(th)
        u = unit(rng.normal(size=3))
        ua, uc, ue = u[2], u[0], -u[1]   # c^ = x, a^ = z, c^ x a^ = -y
        lam, (A, B, G, den) = Co.exit_root(co, t, d, ua, uc, ue)
        y = lambda s: np.array([d, 0.0, t]) + s * u
        form = lambda p: st * p[2] - ct * np.hypot(p[0], p[1])
        if A > 0:
            roots = np.roots([A, 2 * B, -G])
            want = roots[roots > 0]
            assert len(want) == 1 and lam is not None and abs(lam / want[0] - 1) <= 1e-9
            seen["A>0"] += 1
        elif ua > 0:
            assert lam is None
            assert all(form(y(s)) > 0 for s in (0.1, 1.0, 10.0, 1e3))
            seen["A<0 up"] += 1
            continue
        else:
            roots = np.roots([A, 2 * B, -G])
            assert not np.iscomplex(roots).any(), (t, d, u)   # from inside, towards the apex: the nappe is always left
            assert (roots.real > 0).all() and lam is not None and abs(lam / roots.real.min() - 1) <= 1e-9
            seen["A<0 down"] += 1
        p = y(lam)
        assert abs(form(p)) <= 1e-12 * max(1.0, np.linalg.norm(p)) and p[2] > -1e-12
        assert all(form(y(f * lam)) > 0 for f in (0.0, 0.25, 0.5, 0.75, 0.999))
        assert not form(y(1.001 * lam)) > 0
    print(seen)


def test_signs_limits_and_the_axis(rough):
    r = rough
    co, rm = r["co"], r["rm"]
    tan = co[7] / co[6]
    # out of reach: zeros; at or outside the wall, behind the apex, not a number: nothing, flagged
    for t, d, want in ((r["t0"], r["d0"] - 0.31 * rm / co[6], 0), (r["t0"], 0.0, 0), (r["t0"], r["t0"] * tan, -1),
                       (r["t0"], 1.2 * r["t0"] * tan, -1), (-0.5, 0.0, -1), (0.0, 0.0, -1), (np.nan, 0.1, -1)):
        V, S, T, st = Co.cone_sums(6, r["anm"], rm, place(co, r["ch"], t, d), r["q"], co, 16)
        assert st == want and V == 0 and not S.any() and not T.any(), (t, d)
    # a centre exactly on the axis: the fallback frame is perpendicular to the axis, the inscribed sphere's centre IS the
    # particle's and the cap the whole sphere
    zc = Co.cone([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], np.pi / 6)
    t, rho, d, ch, h = Co.foot([0.0, 0.0, 1.7], zc)
    assert d == 0 and abs(ch @ zc[3:6]) <= 1e-15 and abs(np.linalg.norm(ch) - 1) <= 1e-15 and abs(h - 0.85) <= 1e-15
    assert Co.cap_cos(zc, t, d, 1.01) == -1.0
    # within R_i of the apex the whole sphere, just beyond it the bound
    assert Co.cap_cos(zc, 0.9, 0.3, 1.01) == -1.0 and 0.9 ** 2 + 0.3 ** 2 < 1.01 ** 2
    assert -1.0 < Co.cap_cos(zc, 3.0, 1.5, 1.01) < 1.0
