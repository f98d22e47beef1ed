"""CPU-only checks of tests/conic_roll_ref.py, the numpy restatement of docs/SPEC.md §2.24: the properties the section
states, on random contacts; both branches of both kinds occur; the cylinder of §2.21 as the limit of a slender cone and
the plane of §2.17 as the limit of a wide one; the per-contact power identity; and the five hand-made wrong variants of
the reference module (Omega_k not subtracted, the cylinder's normal, the wall's rotation counted as rolling only, a
missing cap, a sign flip) are each rejected by one of these checks, by more than 100 bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cone_ref as Co           # noqa: E402
import conic_history_ref as CH  # noqa: E402
import conic_roll_ref as KR     # noqa: E402

EPS = 1e-12     # relative: a few roundings of products of O(1) factors
LIMIT_BAR = 1e-6
AXIS = np.array([2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0])
APEX = np.array([0.4, -0.3, 0.2])
THETA = np.pi / 6


def _contacts(seed=5, n=400):
    """Random contacts inside an oblique 30-degree cone: the centre 0.3 to 0.9 from the wall, an S_n up to ~25 degrees
    off n^ (the quadrature's error and an asymmetric grain, exaggerated), the row's force -F_i = p_tot S_n + a tangential
    friction part, omega over three decades, Omega_k, coefficients."""
    rng = np.random.default_rng(seed)
    co = Co.cone(APEX, AXIS, THETA)
    ct, st = co[6], co[7]
    out = []
    for k in range(n):
        r = rng.normal(size=3)
        r -= (r @ AXIS) * AXIS
        r /= np.linalg.norm(r)
        s, h = rng.uniform(5.0, 8.0), rng.uniform(0.3, 0.9)
        x = APEX + (ct * s + st * h) * AXIS + (st * s - ct * h) * r
        nh = KR.normal(x, co)
        S = nh * rng.uniform(0.05, 0.5) + 0.1 * rng.normal(size=3) * rng.uniform(0.05, 0.5)
        pt = rng.uniform(50.0, 500.0) if k % 9 else 0.0        # every ninth one clamped
        t = rng.normal(size=3)
        t -= (t @ nh) * nh
        Fw = pt * S + (0.3 * pt * np.linalg.norm(S)) * t
        if k % 11 == 0:
            Fw = -Fw                                            # a row that pulls: N = 0
        om = rng.normal(size=3) * 10.0 ** rng.uniform(-2, 1)
        out.append(dict(Fw=Fw, x=x, co=co, nh=nh, omega=om, Ok=rng.normal() * 2, mur=0.05, gr=3.0, mutw=0.03, gtw=2.0))
    return out


def _law(variant=None):
    return lambda c, omega=None, **kw: KR.couple(kw.get("Fw", c["Fw"]), kw.get("x", c["x"]), c["co"], c["omega"] if omega is None else omega,
                                                 kw.get("Ok", c["Ok"]), kw.get("mur", c["mur"]), kw.get("gr", c["gr"]),
                                                 kw.get("mutw", c["mutw"]), kw.get("gtw", c["gtw"]), variant=variant)


def _rel(c):
    return c["omega"] - c["Ok"] * AXIS


def _loaded(c):
    return c["nh"] @ c["Fw"] > 0


# ---- the properties of §2.24, each a function of the law and of a multiple of its bar, so that the variants can be held
# ---- to them too: check(law, 100) passing would mean the variant is not rejected by more than 100 bars

def check_power(law, bars=1):
    """M.Omega_rel <= 0, and M.omega_i = -P_roll + Omega_k (a^.M) with P_roll >= 0, to 1e-12 of the largest term."""
    for c in _contacts():
        M, P, W, _, N, _ = law(c)
        Or = _rel(c)
        assert M @ Or <= bars * EPS * (np.linalg.norm(M) * np.linalg.norm(Or) + 1e-300)
        big = max(P, abs(W), abs(M @ c["omega"]), 1e-300)
        assert P >= 0 and abs(M @ Or + P) <= bars * EPS * big
        assert abs(M @ c["omega"] + P - W) <= bars * EPS * big


def check_caps(law, bars=1):
    for c in _contacts():
        M = law(c)[0]
        N = max(0.0, c["nh"] @ c["Fw"])                         # the load of the section, not the law's own
        Mn = (M @ c["nh"]) * c["nh"]
        assert np.linalg.norm(M - Mn) <= c["mur"] * N * (1 + bars * EPS) + 1e-300
        assert np.linalg.norm(Mn) <= c["mutw"] * N * (1 + bars * EPS) + 1e-300


def check_rigid_co_rotation_is_exactly_zero(law, bars=1):
    """Carried round by the cone, omega_i = Omega_k a^ by the same product: exactly nothing.  (An exact statement: its bar
    is 0, and so is every multiple of it.)"""
    for c in _contacts():
        M, P, W, _, _, _ = law(c, omega=c["Ok"] * AXIS)
        assert not M.any() and P == 0.0 and W == 0.0


def check_the_two_spins_meet_one_couple_each(law, bars=1):
    """A spin about n^ meets only twisting, a spin in the tangent plane only rolling: the other kind's part is 0, and the
    couple along the spin, to 1e-12 of gamma |omega| (the other part of the spin is a rounding residue of relative size
    2^-53, and its coefficient is at most its gamma: the scale is the uncapped couple, not the capped one)."""
    for c in (c for c in _contacts() if _loaded(c)):
        w = np.linalg.norm(c["omega"])
        sc = max(c["gr"], c["gtw"]) * w
        M, _, _, _, _, (Mr, Mt) = law(c, omega=w * c["nh"], Ok=0.0)
        assert M.any() and np.linalg.norm(Mr) <= bars * EPS * sc
        assert np.linalg.norm(np.cross(M, c["nh"])) <= bars * EPS * sc
        t = np.cross(c["nh"], [1.0, 0.3, -0.2])
        t *= w / np.linalg.norm(t)
        M, _, _, _, _, (Mr, Mt) = law(c, omega=t, Ok=0.0)
        assert M.any() and np.linalg.norm(Mt) <= bars * EPS * sc
        assert abs(M @ c["nh"]) <= bars * EPS * sc


def check_the_cone_twists_and_rolls(law, bars=1):
    """Omega_k a^ alone, on the viscous branches (small gammas): the couple on a grain at rest is gamma_tw (-Omega_k s) n^
    . (-1) + gamma_r Omega_k c g^, that is a twisting part proportional to sin theta and a rolling part proportional to
    cos theta, to 1e-12."""
    for c in (c for c in _contacts() if _loaded(c)):
        co = c["co"]
        ct, st = co[6], co[7]
        gen = Co.frame(co, Co.foot(c["x"], co)[3])[0]
        gr, gtw = 1e-3, 2e-3
        M = law(c, omega=np.zeros(3), gr=gr, gtw=gtw)[0]
        want_tw, want_r = -gtw * (c["Ok"] * st), gr * (c["Ok"] * ct)     # M.n^ and M.g^: M = -kappa (0 - Omega_k a^) parts
        sc = max(abs(want_tw), abs(want_r))
        assert abs(M @ c["nh"] - want_tw) <= bars * EPS * sc and abs(M @ gen - want_r) <= bars * EPS * sc
        assert abs(M @ np.cross(c["nh"], gen)) <= bars * EPS * sc


def check_a_rotation_about_the_axis_rotates_the_couple(law, bars=1):
    """The whole state turned about the axis: M turns with it, to 1e-12."""
    for k, c in enumerate(_contacts()):
        phi = 0.1 + 0.37 * k
        K = np.array([[0, -AXIS[2], AXIS[1]], [AXIS[2], 0, -AXIS[0]], [-AXIS[1], AXIS[0], 0]])
        R = np.eye(3) + np.sin(phi) * K + (1 - np.cos(phi)) * K @ K
        M = law(c)[0]
        M2 = law(c, omega=R @ c["omega"], x=APEX + R @ (c["x"] - APEX), Fw=R @ c["Fw"])[0]
        assert np.abs(M2 - R @ M).max() <= bars * EPS * max(np.abs(M).max(), 1e-300)


CHECKS = (check_power, check_caps, check_rigid_co_rotation_is_exactly_zero, check_the_two_spins_meet_one_couple_each,
          check_the_cone_twists_and_rolls, check_a_rotation_about_the_axis_rotates_the_couple)


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_the_law_has_the_stated_properties(check):
    check(_law())


def test_both_branches_of_both_kinds_occur_and_a_dead_load_adds_nothing():
    got = {}
    for k, c in enumerate(_contacts()):
        M, P, W, br, N, _ = _law()(c)
        got[(k, 0)] = br
        if not N > 0:
            assert not M.any() and P == 0.0 and W == 0.0 and br == (KR.NONE, KR.NONE)
    counts = KR.branch_counts(got)
    print(counts)
    assert all(v >= 20 for v in counts.values()), counts
    c = next(c for c in _contacts() if _loaded(c))              # a kind needs both of its coefficients
    assert not _law()(c, mur=0.0, mutw=0.0)[0].any() and not _law()(c, gr=0.0, gtw=0.0)[0].any()
    assert _law()(c, mur=0.0)[3][0] == KR.NONE and _law()(c, gtw=0.0)[3][1] == KR.NONE


# which check rejects which wrong law
REJECTED_BY = {"omega_k_kept": check_rigid_co_rotation_is_exactly_zero, "cylinder_normal": check_the_two_spins_meet_one_couple_each,
               "rotation_only_rolls": check_the_cone_twists_and_rolls, "no_cap": check_caps, "sign_flip": check_power}


@pytest.mark.parametrize("variant", KR.VARIANTS)
def test_a_wrong_variant_is_rejected_by_more_than_100_bars(variant):
    assert set(REJECTED_BY) == set(KR.VARIANTS)
    REJECTED_BY[variant](_law(), 1)                             # the law itself passes at one bar ...
    with pytest.raises(AssertionError):
        REJECTED_BY[variant](_law(variant), 100)                # ... and the wrong one fails at a hundred


def test_the_pass_sums_the_cones_of_a_particle_and_leaves_the_force_alone(oracle):
    """conic_roll on a sphere in reach of two cones and one at rest against them: the couple is the sum over the cones, f
    and entries 0..3 of cone_out are those of the same pass with every coefficient of §2.24 at 0, M_ax differs by -a^.M,
    and the load along n^ is p_tot |S_n| up to the quadrature (a sphere, friction off)."""
    from shpair import shapes
    anm = shapes.sphere(1.0)
    c0 = Co.cone(APEX, AXIS, THETA)
    c1 = Co.cone(APEX - 0.05 * AXIS, AXIS, THETA + 0.004)
    cones = np.stack([c0, c1])
    ct, st = c0[6], c0[7]
    e1 = CH.axis_frame(AXIS)[0]
    x = np.stack([APEX + (ct * 6.0 + st * 0.7) * AXIS + (st * 6.0 - ct * 0.7) * e1,
                  APEX + (ct * 7.0 + st * 0.75) * AXIS - (st * 7.0 - ct * 0.75) * e1])
    q = np.array([[1.0, 0, 0, 0]] * 2)
    tw = np.array([[0.1, -0.2, 0.05, 0.7, -0.4, 2.0], [0, 0, 0, 0.0, 0.0, 0.0]])
    sums = KR.reach_sums([(0, anm, 1.01)], 8, x, q, np.zeros(2, int), cones)
    assert set(sums) == {(0, 0), (0, 1), (1, 0), (1, 1)} and all(v[0] > 0 for v in sums.values())
    mur, gr, mutw, gtw = np.array([0.05, 0.02]), np.array([3.0, 500.0]), np.array([0.0, 0.03]), np.array([2.0, 2.0])
    on = KR.conic_roll(sums, 2, x, tw, cones, 1e4, 1.25, mur, gr, mutw, gtw, gamma=500.0)
    off = KR.conic_roll(sums, 2, x, tw, cones, 1e4, 1.25, 0.0, 0.0, 0.0, 0.0, gamma=500.0)
    assert np.array_equal(on["f"], off["f"]) and np.array_equal(on["cone_out"][:, :4], off["cone_out"][:, :4])
    assert not off["couple"].any() and on["couple"][0].any() and not on["couple"][1].any()        # omega = 0, Omega_k = 0: exactly nothing
    assert np.array_equal(on["torque0"], off["torque"])
    assert np.array_equal(off["cone_out"][:, 4], off["max0"]) and np.array_equal(on["max0"], off["max0"])
    assert on["branch"][(0, 0)][1] == KR.NONE and on["branch"][(0, 1)] == (KR.CAPPED, KR.VISCOUS)  # the kinds follow the cones
    # friction off: F_w = p_tot S_n, so N = p_tot n^.S_n <= p_tot |S_n|; a cone's wall curves more towards the apex, so even a
    # sphere's S_n tilts along the generator, by an angle of the order of the cap's width over the slant distance: the gap
    # 1 - cos is below (R_i / s)^2 / 2 with s >= 6 R_i here
    for k in sums:
        gap = (on["NS"][k] - on["N"][k]) / on["NS"][k]
        print(f"{k}: N {on['N'][k]:.6g} p_tot |S_n| {on['NS'][k]:.6g} gap {gap:.2e}")
        assert -1e-14 <= gap <= 0.5 / 36.0
    # a turning cone moves a particle at rest: Omega_rel = -Omega_k a^, and cone 1 both twists and rolls it
    turn = KR.conic_roll(sums, 2, x, tw, cones, 1e4, 1.25, mur, gr, mutw, gtw, gamma=500.0, omega=[0.0, 0.5])
    M = turn["couple"][1]
    nh = KR.normal(x[1], c1)
    assert turn["wroll"][1, 1] != 0 and turn["wroll"][1, 0] == 0 and abs(M @ nh) > 0 and np.linalg.norm(M - (M @ nh) * nh) > 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_cylinder_is_the_limit_of_a_slender_cone(oracle, seed):
    """§2.22's slender set-up (theta = 2.5e-8, the apex 1e8 R_i down the axis, local radius 2.5 R_i, h = 0.7 R_i), a rough
    L = 6 shape with damping and friction, Omega = 1.7, uncapped and capped: M, its power and N agree with
    tests/cyl_roll_ref.py within 1e-6.  Value reached: printed (see docs/SPEC.md §2.24)."""
    import cyl_ref as Cy
    import cyl_roll_ref as CR
    from shpair import shapes
    from test_cone_ref import unit
    rng = np.random.default_rng(seed)
    anm = shapes.random_shape(6, 10 + seed, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    q, ax = unit(rng.normal(size=4)), unit(rng.normal(size=3))
    ch = unit(np.cross(ax, rng.normal(size=3)))
    th, nq, Om = 2.5e-8, 16, 1.7
    t0 = 1e8 * rm
    Rc = t0 * np.tan(th)
    co = Co.cone(-t0 * ax, ax, th)
    cyl = np.array([0.0, 0.0, 0.0, *ax, Rc])
    x = (Rc - 0.7 * rm) * ch
    V, S, T, st = Co.cone_sums(6, anm, rm, x, q, co, nq)
    Vc, Sc, Tc, st2 = Cy.cyl_sums(6, anm, rm, x, q, cyl, nq)
    assert st == 1 and st2 == 1 and Vc > 0
    tw = np.concatenate([0.3 * rng.normal(size=3), 3.0 * rng.normal(size=3)])
    F = Co.contact_wrench(V, S, T, x, co, 1000.0, 1.25, tw, gamma=3.0, mu=0.5, gt=2.0, omega=Om)[0]
    Fc = Cy.contact_wrench(Vc, Sc, Tc, x, cyl, 1000.0, 1.25, tw, gamma=3.0, mu=0.5, gt=2.0, omega=Om)[0]
    worst, seen = 0.0, set()
    for mur, gr, mutw, gtw in ((0.05, 0.3, 0.03, 0.2), (1e-3, 300.0, 1e-3, 200.0)):
        M, P, W, br, N, _ = KR.couple(-F, x, co, tw[3:], Om, mur, gr, mutw, gtw)
        Mc, Pc, Wc, brc, Nc = CR.couple(-Fc, x, cyl, tw[3:], Om, mur, gr, mutw, gtw)
        err = max(np.abs(M - Mc).max() / np.abs(Mc).max(), abs(P - Pc) / Pc, abs(N - Nc) / Nc, abs(W - Wc) / max(abs(Wc), np.abs(Mc).max()))
        worst = max(worst, err)
        seen.add(br)
        print(f"seed {seed} {br}: cone M {M}, cylinder {Mc}, rel err {err:.1e}")
        assert br == brc and Mc.any() and err <= LIMIT_BAR
    print(f"value reached: {worst:.1e}")
    assert seen == {(KR.VISCOUS, KR.VISCOUS), (KR.CAPPED, KR.CAPPED)}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_plane_is_the_limit_of_a_wide_cone(oracle, seed):
    """theta = pi/2 - 1e-8 and Omega = 0, tests/test_cone_ref.py's set-up: M, its power and N of a rough L = 6 shape with
    damping and friction agree with tests/wall_roll_ref.py's couple for the plane within 1e-6.  Value reached: printed."""
    import wall_ref as W
    import wall_roll_ref as WR
    from shpair import shapes
    from test_cone_ref import unit
    from test_shell_ledger_ref import frame_e1
    rng = np.random.default_rng(seed)
    anm = shapes.random_shape(6, 10 + seed, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    q, n = unit(rng.normal(size=4)), unit(rng.normal(size=3))
    h, nq = 0.7 * rm, 16
    plane = np.array([*n, 0.0])
    xw = n * h
    Vw, Sw, Tw, st = W.wall_sums(6, anm, rm, xw, q, plane, nq)
    th = np.pi / 2 - 1e-8
    co = Co.cone(-rm * frame_e1(-n), n, th)
    x = n * (h + np.cos(th) * rm) / np.sin(th)
    V, S, T, st2 = Co.cone_sums(6, anm, rm, x, q, co, nq)
    assert st == 1 and st2 == 1 and Vw > 0
    tw = np.concatenate([0.3 * rng.normal(size=3), 3.0 * rng.normal(size=3)])
    F = Co.contact_wrench(V, S, T, x, co, 1000.0, 1.25, tw, gamma=3.0, mu=0.5, gt=2.0, omega=0.0)[0]
    Fp = WR.contact_force(Vw, Sw, Tw, xw, tw, plane, 1000.0, 1.25, 3.0, 0.5, 2.0)[0]
    worst, seen = 0.0, set()
    for mur, gr, mutw, gtw in ((0.05, 3.0, 0.03, 2.0), (1e-3, 300.0, 1e-3, 200.0)):
        M, P, Wd, br, N, _ = KR.couple(-F, x, co, tw[3:], 0.0, mur, gr, mutw, gtw)
        Mp, Pp, brp, Np = WR.couple(-Fp, n, tw[3:], mur, gr, mutw, gtw)
        err = max(np.abs(M - Mp).max() / np.abs(Mp).max(), abs(P - Pp) / Pp, abs(N - Np) / Np)
        worst = max(worst, err)
        seen.add(br)
        print(f"seed {seed} {br}: cone M {M}, plane {Mp}, rel err {err:.1e}")
        assert br == brp and Wd == 0.0 and Mp.any() and err <= LIMIT_BAR
    print(f"value reached: {worst:.1e}")
    assert seen == {(KR.VISCOUS, KR.VISCOUS), (KR.CAPPED, KR.CAPPED)}


def test_the_power_identity_holds_per_contact_on_real_sums(oracle):
    """(tau + M).omega_i - tau.omega_i = M.omega_i = -P_roll + Omega_k (a^.M) to 1e-12 of the largest term, on the sums of a
    rough shape against a 30-degree cone that turns, behind the elastic, the dissipative and the spring law; and the wall's
    share: M_ax changes by -a^.M, so Omega_k times that change is minus the work term."""
    from shpair import shapes
    anm = shapes.random_shape(6, 3, amp=0.1)
    rm = oracle.shape_rmax(6, anm)
    co = Co.cone(APEX, AXIS, THETA)
    ct, st = co[6], co[7]
    e1 = CH.axis_frame(AXIS)[0]
    x = (APEX + (ct * 6.0 + st * 0.7 * rm) * AXIS + (st * 6.0 - ct * 0.7 * rm) * e1)[None]
    q = np.array([[0.5, -0.5, 0.5, 0.5]])
    sums = KR.reach_sums([(6, anm, rm)], 16, x, q, [0], [co])
    assert sums[(0, 0)][0] > 0
    rng = np.random.default_rng(8)
    nroll, seen = 0, set()
    for name, (gamma, mu, gt, kt) in dict(elastic=(0, 0, 0, 0), dissipative=(3.0, 0.5, 2.0, 0), spring=(3.0, 0.5, 2.0, 4e3)).items():
        for _ in range(4):
            tw = np.concatenate([0.3 * rng.normal(size=3), rng.normal(size=3)])[None]
            mur, mutw = ((0.05, 0.03), (1e-3, 1e-3))[nroll % 2]      # mostly viscous, mostly capped
            r = KR.conic_roll(sums, 1, x, tw, [co], 1000.0, 1.25, mur, 3.0, mutw, 2.0, gamma=gamma, mu=mu, gt=gt, omega=1.7, kt=kt, dt=2e-3)
            M, Pr, Wr = r["couple"][0], r["proll"][0, 0], r["wroll"][0, 0]
            lhs = (r["torque"][0] - r["torque0"][0]) @ tw[0, 3:]
            err = abs(lhs + Pr - Wr) / max(abs(lhs), Pr, abs(Wr))
            dM = r["cone_out"][0, 4] - r["max0"][0]
            print(f"{name}: N {r['N'][(0, 0)]:.4g} branches {r['branch'][(0, 0)]} P_roll {Pr:.4g} W_roll {Wr:.4g} err {err:.1e}")
            assert err <= 1e-12 and Pr > 0 and M.any()
            assert abs(1.7 * dM + Wr) <= 1e-12 * abs(Wr)
            nroll += 1
            seen |= set(r["branch"][(0, 0)])
    assert nroll == 12 and seen == {KR.VISCOUS, KR.CAPPED}
