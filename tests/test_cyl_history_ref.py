"""CPU pins of tests/cyl_history_ref.py, the numpy restatement of docs/SPEC.md §2.19 that the GPU tests of the cylinder
springs compare against: the planar spring law of §2.15 as the limit Rc -> infinity, invariance of (xi_a, xi_theta)
under a screw motion of the whole state about the axis, co-rotation with the drum, and the bookkeeping of a pass (look,
reset, a cylinder without a spring).  Passes on any tree that has the reference: it pins the yardstick, not the kernels."""
import numpy as np

import cyl_history_ref as CH
import cyl_ref as Cy
import friction_ref as Fr
import wall_history_ref as WH
import wall_ref as W
from shpair import shapes
from test_cyl_ref import frame_e1, qmul, unit


def test_the_planar_spring_law_is_the_limit_of_a_large_cylinder(oracle):
    """Rc = 1e8 R_i: F_t and the new xi, mapped to the space frame with (a^, t^_c) of the contact point, reproduce
    wall_history_ref.spring_law at the tangent plane to 1e-6, sticking and sliding, over two consecutive passes.  The
    contacts are those of the friction law's test in the same limit (tests/test_cyl_ref.py): a spinning unit sphere with
    its own sums, and a rough L = 6 shape whose S_n is replaced by its normal part.  The bar is that test's: the
    contact-point geometry is the same, and the curvature scale R_i / Rc is 1e-8."""
    rng = np.random.default_rng(11)
    tw = np.array([0.3, -0.2, 0.1, 0.5, 0.4, -0.6])
    seen, worst = set(), 0.0
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
        for mu, gt, kt, dt in ((0.5, 2.0, 4e3, 1e-3), (0.5, 0.0, 4e3, 1e-3), (0.01, 2.0, 4e5, 1e-2)):
            xi2, xi3 = np.zeros(2), np.zeros(3)
            for step in range(2):
                F, tau, E, d = CH.contact_history(V, S, T, x, cyl, 1000.0, 1.25, tw, 3.0, mu, gt, 0.0, kt, xi2, dt)
                p = 1000.0 * 1.25 * V ** 0.25
                N = max(0.0, p + 3.0 * (S @ tw[:3] + T @ tw[3:])) * np.linalg.norm(S)
                ri = Fr.wall_contact_point(S, T, n, h)
                vrel = tw[:3] + np.cross(tw[3:], ri)
                Ftw, xi3, kind = WH.spring_law(xi3, vrel - (vrel @ n) * n, n, N, mu, gt, kt, dt)
                xi2 = d["xi"]
                xs = xi2[0] * d["ea"] + xi2[1] * d["et"]
                err = (np.abs(d["Ft"] - Ftw).max() / np.linalg.norm(Ftw), np.abs(xs - xi3).max() / np.linalg.norm(xi3))
                print("%s mu %g gamma_t %g k_t %g step %d %s: dFt %.1e dxi %.1e" % (label, mu, gt, kt, step, kind, *err))
                assert d["kind"] == kind and np.linalg.norm(Ftw) > 0
                assert max(err) <= 1e-6
                seen.add(kind)
                worst = max(worst, *err)
    print("plane limit of the spring law: largest deviation %.1e (bar 1e-6)" % worst)
    assert seen == {CH.STICK, CH.SLIDE}


def _rough_state(oracle):
    anm = shapes.random_shape(6, 3, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    rng = np.random.default_rng(1)
    q, ax = unit(rng.normal(size=4)), unit(rng.normal(size=3))
    ch = unit(np.cross(ax, rng.normal(size=3)))
    a = np.array([0.4, -0.3, 0.2])
    Rc = 2.5 * rm
    return dict(anm=anm, rm=rm, q=q, ax=ax, a=a, Rc=Rc, cyl=np.array([*a, *ax, Rc]), x=a + (Rc - 0.7 * rm) * ch + 0.3 * ax)


def _one(r, x, q, tw, omega, xi, dt, mu=0.5, gt=2.0, kt=4e3, nq=16):
    return CH.cyl_forces_history([(6, r["anm"], r["rm"])], nq, x[None], q[None], [0], tw[None], [r["cyl"]], [1000.0], [1.25], 3.0,
                                 mu, gt, omega, kt, xi, np.any(np.asarray(xi) != 0, axis=-1), dt)


def test_a_screw_motion_of_the_whole_state_leaves_the_surface_coordinates_unchanged(oracle):
    """x, quat and the twists rotated by theta about the axis and shifted along it, the cylinder's Omega as it was: the
    (xi_a, xi_theta) coming out are unchanged and the wrench is rotated, to the 1e-12 of §2.18's screw test; sticking and
    sliding."""
    r = _rough_state(oracle)
    tw = np.array([0.3, -0.2, 0.1, 0.5, 0.4, -0.6])
    th = 0.83
    g = np.array([np.cos(th / 2), *(np.sin(th / 2) * r["ax"])])
    G = W.quat_to_mat(g)
    x2 = r["a"] + G @ (r["x"] - r["a"]) - 1.7 * r["ax"]
    tw2 = np.concatenate([G @ tw[:3], G @ tw[3:]])
    seen = set()
    for mu, xi in ((0.5, [[[2e-3, -1e-3]]]), (0.01, [[[2e-3, -1e-3]]]), (0.5, [[[0.0, 0.0]]])):
        o1 = _one(r, r["x"], r["q"], tw, 0.7, xi, 1e-3, mu=mu)
        o2 = _one(r, x2, qmul(g, r["q"]), tw2, 0.7, xi, 1e-3, mu=mu)
        sc, xs = np.linalg.norm(o1["f"]), np.abs(o1["xi"]).max()
        err = (np.abs(o2["xi"] - o1["xi"]).max() / xs, np.abs(o2["f"][0] - G @ o1["f"][0]).max() / sc,
               np.abs(o2["torque"][0] - G @ o1["torque"][0]).max() / sc, abs(o2["cyl_out"][0, 4] - o1["cyl_out"][0, 4]) / sc)
        print("screw, mu %g %s: dxi %.1e dF %.1e dtau %.1e dM_ax %.1e" % (mu, o1["kind"][0, 0], *err))
        assert o1["kind"][0, 0] == o2["kind"][0, 0] != CH.RESET and xs > 0
        assert max(err) <= 1e-12
        seen.add(o1["kind"][0, 0])
    assert seen == {CH.STICK, CH.SLIDE}


def test_a_particle_carried_round_by_the_drum_keeps_its_spring(oracle):
    """The particle turns rigidly with the drum, w = Omega a^ x (x - a), omega = Omega a^, x and quat turned by Omega dt per
    pass: v_t = 0 at the contact point, so (xi_a, xi_theta) stay what they were given over 8 passes (1e-12 relative) and the
    tangential force only rotates.  The space-frame vector of §2.15 with a projection would lose 1 - cos(Omega dt) of its
    length per pass."""
    r = _rough_state(oracle)
    Om, dt = 2.0, 0.05
    xi = np.array([[[2e-3, -1e-3]]])
    x, q = r["x"].copy(), r["q"].copy()
    g = np.array([np.cos(Om * dt / 2), *(np.sin(Om * dt / 2) * r["ax"])])
    G = W.quat_to_mat(g)
    f0 = None
    for k in range(8):
        tw = np.concatenate([Om * np.cross(r["ax"], x - r["a"]), Om * r["ax"]])
        o = _one(r, x, q, tw, Om, xi, dt)
        assert o["kind"][0, 0] == CH.STICK
        assert np.abs(o["xi"] - xi).max() <= 1e-12 * np.abs(xi).max()
        if f0 is None:
            f0, Gk = o["f"][0], np.eye(3)
        assert np.abs(o["f"][0] - Gk @ f0).max() <= 1e-12 * np.linalg.norm(f0)
        xi, x, q, Gk = o["xi"], r["a"] + G @ (x - r["a"]), qmul(g, q), G @ Gk
    assert 1 - np.cos(Om * dt) > 1e-3


def test_look_reset_and_a_cylinder_without_a_spring(oracle):
    r = _rough_state(oracle)
    tw = np.array([0.3, -0.2, 0.1, 0.5, 0.4, -0.6])
    xi = np.array([[[2e-3, -1e-3]]])
    look = _one(r, r["x"], r["q"], tw, 0.7, xi, 0.0)
    assert np.array_equal(look["xi"], xi) and look["live"].all() and look["kind"][0, 0] == CH.STICK
    # at rest and well inside the cap the contact carries F_t = -k_t (xi_a a^ + xi_theta t^_c)
    rest = _one(r, r["x"], r["q"], np.zeros(6), 0.0, xi, 0.0)
    (_, _, Ft, ri, rc, vt, N, kind, ratio), = rest["contacts"]
    ea, et = CH.surface_frame(r["ax"], rc, r["Rc"])
    assert kind == CH.STICK and ratio < 0.5 and np.allclose(Ft, -4e3 * (2e-3 * ea - 1e-3 * et), rtol=0, atol=1e-15 * 4e3)
    assert abs(np.linalg.norm(et) - 1) <= 1e-12 and abs(ea @ et) <= 1e-12 and abs(et @ rc) <= 1e-12
    # out of reach: reset, and the state is gone; no k_t: tests/cyl_ref.py's law, kind none, no state
    far = _one(r, r["a"] + 0.1 * r["ax"], r["q"], tw, 0.7, xi, 1e-3)
    assert far["kind"][0, 0] == CH.RESET and not far["live"].any() and not far["xi"].any() and not far["f"].any()
    off = _one(r, r["x"], r["q"], tw, 0.7, np.zeros((1, 1, 2)), 1e-3, kt=0.0)
    ref = Cy.cyl_forces([(6, r["anm"], r["rm"])], 16, r["x"][None], r["q"][None], [0], [r["cyl"]], [1000.0], [1.25], tw=tw[None],
                        gamma=3.0, mu=0.5, gt=2.0, omega=0.7)
    assert off["kind"][0, 0] == CH.NONE and not off["live"].any()
    assert np.array_equal(off["f"], ref["f"]) and np.array_equal(off["torque"], ref["torque"]) and np.array_equal(off["cyl_out"], ref["cyl_out"])
