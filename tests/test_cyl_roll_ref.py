"""CPU-only checks of tests/cyl_roll_ref.py, the numpy restatement of docs/SPEC.md §2.21: the properties the section
states, on random contacts; both branches of both kinds occur; the plane of §2.17 as the limit of a wide cylinder; the
per-contact power identity of §2.20 with the couples in it; and the hand-made wrong variants of the reference module
(Omega_c not subtracted, the normal taken from S_n, a missing cap, a sign flip) are each rejected by one of these checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cyl_ref as Cy          # noqa: E402
import cyl_roll_ref as CR     # noqa: E402

EPS = 1e-12     # relative: a few roundings of products of O(1) factors
AXIS = np.array([2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0])


def _contacts(seed=5, n=400):
    """Random contacts inside an oblique cylinder: the centre, an S_n up to ~25 degrees off c^ (the quadrature's error and an
    asymmetric grain, exaggerated), the row's force -F_i = p_tot S_n + a tangential friction part, omega over three
    decades, Omega_c, coefficients."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        cyl = np.array([0.4, -0.3, 0.2, *AXIS, 4.0])
        t = rng.normal(size=3)
        t -= (t @ AXIS) * AXIS
        x = cyl[:3] + rng.uniform(2.5, 3.5) * t / np.linalg.norm(t) + rng.uniform(-2, 2) * AXIS
        ch = Cy.foot(x, cyl)[2]
        S = ch * rng.uniform(0.05, 0.5) + 0.1 * rng.normal(size=3) * rng.uniform(0.05, 0.5)
        pt = rng.uniform(50.0, 500.0) if k % 9 else 0.0        # every ninth one clamped
        t = rng.normal(size=3)
        t -= (t @ ch) * ch
        Fw = pt * S + (0.3 * pt * np.linalg.norm(S)) * t
        if k % 11 == 0:
            Fw = -Fw                                            # a row that pulls: N = 0
        om = rng.normal(size=3) * 10.0 ** rng.uniform(-2, 1)
        out.append(dict(Fw=Fw, x=x, cyl=cyl, ch=ch, S=S, omega=om, Oc=rng.normal() * 2, mur=0.05, gr=3.0, mutw=0.03, gtw=2.0))
    return out


def _law(variant=None):
    return lambda c, omega=None, **kw: CR.couple(kw.get("Fw", c["Fw"]), kw.get("x", c["x"]), c["cyl"], c["omega"] if omega is None else omega,
                                                 kw.get("Oc", c["Oc"]), kw.get("mur", c["mur"]), kw.get("gr", c["gr"]),
                                                 kw.get("mutw", c["mutw"]), kw.get("gtw", c["gtw"]), variant=variant, S=c["S"])


def _rel(c):
    return c["omega"] - c["Oc"] * AXIS


# ---- the properties of §2.21, each a function of the law, so that the variants can be held to them too --------------------

def check_power(law):
    for c in _contacts():
        M, P, W, _, N = law(c)
        Or = _rel(c)
        assert M @ Or <= EPS * (np.linalg.norm(M) * np.linalg.norm(Or) + 1e-300)
        assert P >= 0 and abs(M @ Or + P) <= 1e-9 * max(P, 1e-300)
        # M.omega_i = -P_roll + Wdot_roll
        assert abs(M @ c["omega"] + P - W) <= 1e-9 * max(P, abs(W), 1e-300)


def check_caps(law):
    for c in _contacts():
        M = law(c)[0]
        N = max(0.0, c["ch"] @ c["Fw"])                         # the load of the section, not the law's own
        Mn = (M @ c["ch"]) * c["ch"]
        assert np.linalg.norm(M - Mn) <= c["mur"] * N * (1 + 1e-9) + 1e-300
        assert np.linalg.norm(Mn) <= c["mutw"] * N * (1 + 1e-9) + 1e-300


def check_rigid_co_rotation_is_exactly_zero(law):
    for c in _contacts():
        M, P, W, _, _ = law(c, omega=c["Oc"] * AXIS)            # carried round by the drum: the same product
        assert not M.any() and P == 0.0 and W == 0.0


def check_the_two_spins_meet_one_couple_each(law):
    for c in _contacts():
        if not c["ch"] @ c["Fw"] > 0:
            continue
        w = np.linalg.norm(c["omega"])
        about = law(c, omega=w * c["ch"], mur=0.0, Oc=0.0)[0]   # twisting only: the law with rolling switched off ...
        both = law(c, omega=w * c["ch"], Oc=0.0)[0]
        assert np.abs(both - about).max() <= 1e-9 * (np.abs(both).max() + 1e-300) and both.any()     # ... is the whole law
        t = np.cross(c["ch"], [1.0, 0.3, -0.2])
        t *= w / np.linalg.norm(t)
        inplane = law(c, omega=t, mutw=0.0, Oc=0.0)[0]
        both = law(c, omega=t, Oc=0.0)[0]
        assert np.abs(both - inplane).max() <= 1e-9 * (np.abs(both).max() + 1e-300) and both.any()


def check_the_drum_only_rolls(law):
    """a^ is normal to c^: another Omega_c changes the twisting couple by no more than 1e-12 of the couple."""
    for c in _contacts():
        if not c["ch"] @ c["Fw"] > 0:
            continue
        a, b = law(c, gtw=1e-3)[0], law(c, gtw=1e-3, Oc=c["Oc"] + 1.3)[0]      # (a small gamma_tw: the viscous branch, where M_tw follows Omega_n)
        assert abs((a - b) @ c["ch"]) <= 1e-12 * max(np.linalg.norm(a), np.linalg.norm(b))
        assert np.abs(a - b).max() > 0                          # ... and the rolling couple does follow it


def check_a_screw_motion_rotates_the_couple(law):
    """The whole state turned about the axis and moved along it: M turns with it, to 1e-12."""
    for k, c in enumerate(_contacts()):
        phi, z = 0.1 + 0.37 * k, 0.3 * np.sin(k)
        K = np.array([[0, -AXIS[2], AXIS[1]], [AXIS[2], 0, -AXIS[0]], [-AXIS[1], AXIS[0], 0]])
        R = np.eye(3) + np.sin(phi) * K + (1 - np.cos(phi)) * K @ K
        a = c["cyl"][:3]
        M = law(c)[0]
        M2 = law(c, omega=R @ c["omega"], x=a + R @ (c["x"] - a) + z * AXIS, Fw=R @ c["Fw"])[0]
        assert np.abs(M2 - R @ M).max() <= 1e-12 * max(np.abs(M).max(), 1e-300)


CHECKS = (check_power, check_caps, check_rigid_co_rotation_is_exactly_zero, check_the_two_spins_meet_one_couple_each,
          check_the_drum_only_rolls, check_a_screw_motion_rotates_the_couple)


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_the_law_has_the_stated_properties(check):
    check(_law())


def test_both_branches_of_both_kinds_occur_and_a_dead_load_adds_nothing():
    got = {}
    for k, c in enumerate(_contacts()):
        M, P, W, br, N = _law()(c)
        got[(k, 0)] = br
        if not N > 0:
            assert not M.any() and P == 0.0 and W == 0.0 and br == (CR.NONE, CR.NONE)
    counts = CR.branch_counts(got)
    print(counts)
    assert all(v >= 20 for v in counts.values()), counts
    c = next(c for c in _contacts() if c["ch"] @ c["Fw"] > 0)   # a kind needs both of its coefficients
    assert not _law()(c, mur=0.0, mutw=0.0)[0].any() and not _law()(c, gr=0.0, gtw=0.0)[0].any()
    assert _law()(c, mur=0.0)[3][0] == CR.NONE and _law()(c, gtw=0.0)[3][1] == CR.NONE


# which check rejects which wrong law
REJECTED_BY = {"omega_c_kept": check_rigid_co_rotation_is_exactly_zero, "normal_from_S": check_the_two_spins_meet_one_couple_each,
               "no_cap": check_caps, "sign_flip": check_power}


@pytest.mark.parametrize("variant", CR.VARIANTS)
def test_a_wrong_variant_is_rejected(variant):
    assert set(REJECTED_BY) == set(CR.VARIANTS)
    with pytest.raises(AssertionError):
        REJECTED_BY[variant](_law(variant))


def test_the_pass_sums_the_cylinders_of_a_particle_and_leaves_the_force_alone(oracle):
    """cyl_roll on a sphere in reach of two crossing cylinders and one at rest against one: the couple is the sum over the
    cylinders, f and entries 0..3 of cyl_out are those of the same pass with every coefficient of §2.21 at 0, M_ax differs
    by -a^.M, and the radial load is p_tot |S_n| up to the quadrature (a sphere, friction off)."""
    from shpair import shapes
    anm = shapes.sphere(1.0)
    cyls = np.array([[0, 0, 0, 0, 0, 1.0, 3.0], [0, 0, 0, 1.0, 0, 0, 3.0]])
    x, q = np.array([[0.0, 2.07, 0.3], [0.2, 2.05, 0.0]]), np.array([[1.0, 0, 0, 0]] * 2)
    tw = np.array([[0.1, -0.2, 0.05, 0.7, -0.4, 2.0], [0, 0, 0, 0.0, 0.0, 0.0]])
    sums = CR.reach_sums([(0, anm, 1.01)], 8, x, q, np.zeros(2, int), cyls)
    assert set(sums) == {(0, 0), (0, 1), (1, 0), (1, 1)} and all(v[0] > 0 for v in sums.values())
    mur, gr, mutw, gtw = np.array([0.05, 0.02]), np.array([3.0, 500.0]), np.array([0.0, 0.03]), np.array([2.0, 2.0])
    on = CR.cyl_roll(sums, 2, x, tw, cyls, 1e4, 1.25, mur, gr, mutw, gtw, gamma=500.0)
    off = CR.cyl_roll(sums, 2, x, tw, cyls, 1e4, 1.25, 0.0, 0.0, 0.0, 0.0, gamma=500.0)
    assert np.array_equal(on["f"], off["f"]) and np.array_equal(on["cyl_out"][:, :4], off["cyl_out"][:, :4])
    assert not off["couple"].any() and on["couple"][0].any() and not on["couple"][1].any()        # omega = 0, Omega_c = 0: exactly nothing
    assert np.abs(on["torque"] - on["couple"] - off["torque"]).max() <= 1e-14 * np.abs(on["torque"]).max()
    assert np.array_equal(off["cyl_out"][:, 4], off["max0"]) and np.array_equal(on["max0"], off["max0"])
    assert on["branch"][(0, 0)][1] == CR.NONE and on["branch"][(0, 1)] == (CR.CAPPED, CR.VISCOUS)  # the kinds follow the cylinders
    for k in sums:
        assert abs(on["N"][k] - on["NS"][k]) <= 1e-9 * on["NS"][k]
    # a turning drum moves a particle at rest: Omega_rel = -Omega_c a^
    turn = CR.cyl_roll(sums, 2, x, tw, cyls, 1e4, 1.25, mur, gr, mutw, gtw, gamma=500.0, omega=[0.5, 0.0])
    assert turn["couple"][1].any() and turn["wroll"][1, 0] != 0 and turn["wroll"][1, 1] == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_plane_is_the_limit_of_a_wide_cylinder(oracle, seed):
    """Rc = 1e8 R_i, Omega_c = 0, the axis the e1 of the plane's frame: M of a unit sphere with damping and friction agrees
    with tests/wall_roll_ref.py's couple for the plane to 1e-6, the bar of §2.18 to §2.20 in this limit.  Value reached:
    printed (1.1e-8 at worst over the three seeds)."""
    import wall_ref as W
    import wall_roll_ref as WR
    import shell_ledger_ref as SL
    from shpair import shapes
    from test_shell_ledger_ref import frame_e1, unit
    rng = np.random.default_rng(seed)
    anm, rm, nq = shapes.sphere(1.0), 1.01, 16
    q, n = unit(rng.normal(size=4)), unit(rng.normal(size=3))
    x = n * 0.7 * rm
    Rc = 1e8 * rm
    cyl = np.array([*(Rc * n), *frame_e1(-n), Rc])
    plane = np.array([*n, 0.0])
    tw = np.concatenate([rng.normal(size=3), 3.0 * rng.normal(size=3)])
    V, S, T, st = Cy.cyl_sums(0, anm, rm, x, q, cyl, nq)
    Vp, Sp, Tp, stp = W.wall_sums(0, anm, rm, x, q, plane, nq)
    assert st == 1 and V > 0 and stp == 1 and Vp > 0
    worst, seen = 0.0, set()
    for mur, gr, mutw, gtw in ((0.05, 3.0, 0.03, 2.0), (1e-3, 300.0, 1e-3, 200.0)):
        d = SL.contact_powers(V, S, T, x, cyl, 1000.0, 1.25, tw, 3.0, 0.5, 2.0, 0.0)
        Fp = WR.contact_force(Vp, Sp, Tp, x, tw, plane, 1000.0, 1.25, 3.0, 0.5, 2.0)[0]
        M, P, Wd, br, N = CR.couple(-d["F"], x, cyl, tw[3:], 0.0, mur, gr, mutw, gtw)
        Mp, Pp, brp, Np = WR.couple(-Fp, n, tw[3:], mur, gr, mutw, gtw)
        err = max(np.abs(M - Mp).max() / np.abs(Mp).max(), abs(P - Pp) / Pp, abs(N - Np) / Np)
        worst = max(worst, err)
        seen.add(br)
        print(f"seed {seed} {br}: cylinder M {M}, plane {Mp}, rel err {err:.1e}")
        assert br == brp and Wd == 0.0 and Mp.any() and err <= 1e-6
    print(f"value reached: {worst:.1e}")
    assert seen == {(CR.VISCOUS, CR.VISCOUS), (CR.CAPPED, CR.CAPPED)}


@pytest.mark.parametrize("label", ["sphere", "rough"])
def test_the_power_identity_holds_per_contact_with_the_couples(oracle, label):
    """F.w + (tau + M).omega = -p Vdot - P_d - (P_f + P_roll) + (Wdot_c + Wdot_roll) to 1e-12 of the largest term, for
    tests/test_shell_ledger_ref.py's five laws of the contact, Omega = 1.7; and the work entry is -Omega times the friction
    part and the rolling part of M_ax together."""
    import shell_ledger_ref as SL
    from test_shell_ledger_ref import LAWS, contact
    lmax, anm, rm, x, q, cyl, V, S, T = contact(label)
    a, ax = cyl[:3], cyl[3:6]
    rng = np.random.default_rng(8)
    nroll = 0
    for name, (scale, gamma, mu, gt, kt, xi) in LAWS.items():
        for _ in range(4):
            tw = scale * np.concatenate([rng.normal(size=3), 0.5 * rng.normal(size=3)])
            d = SL.contact_powers(V, S, T, x, cyl, 1000.0, 1.25, tw, gamma, mu, gt, 1.7, kt, (0.0, 0.0) if xi is None else xi, 2e-3)
            M, Pr, Wr, br, N = CR.couple(-d["F"], x, cyl, tw[3:], 1.7, 0.05, 3.0, 0.03, 2.0)
            Pd, Pf, Wc = d["P"]
            lhs = d["F"] @ tw[:3] + (d["tau"] + M) @ tw[3:]
            terms = (-d["p"] * d["vd"], -Pd, -(Pf + Pr), Wc + Wr)
            err = abs(lhs - sum(terms)) / max(abs(t) for t in terms + (lhs,))
            print(f"{label} {name}: N {N:.4g} branches {br} P_roll {Pr:.4g} W_roll {Wr:.4g} err {err:.1e}")
            assert err <= 1e-12 and Pr >= 0
            nroll += Pr > 0
            if d["friction"]:
                Mf = ax @ (np.cross(x - a, -d["Ft"]) - np.cross(d["ri"], d["Ft"])) - ax @ M
                assert abs((Wc + Wr) + 1.7 * Mf) <= 1e-12 * max(abs(Wc), abs(Wr), abs(1.7 * Mf))
            else:
                assert not M.any() or N > 0
    assert nroll >= 12


def test_the_balance_of_a_thrown_sphere_closes_to_first_order_with_the_couples_on(oracle):
    """tests/shell_ledger_ref.py's thrown sphere with both couples on, at dt and dt / 2: the residual
    |Delta E_mech - (W_shell - D_shell)| halves (7.02e-2 and 3.45e-2, ratio 0.491; the couples dissipate 0.376 of
    D_f = 21.5).  These are the figures tests/test_gpu_cyl_roll.py's closure test is chosen on."""
    import shell_ledger_ref as SL
    r1, r2 = CR.thrown_sphere(1), CR.thrown_sphere(2)
    R1, R2 = SL.residual(r1), SL.residual(r2)
    print(f"R(dt) {R1:.3e} R(dt/2) {R2:.3e} ratio {R2 / R1:.3f}; D_roll {r1['D_roll']:.4f} of D_f {r1['D_f']:.4f}; contact steps {r1['ncontact']}")
    assert not r1["touching"] and r1["h"] > 1.01 and r1["ncontact"] > 100 and r1["D_roll"] > 0.1
    assert R2 <= 0.6 * R1 and R2 >= 0.4 * R1
