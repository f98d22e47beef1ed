"""CPU tests of tests/shell_ledger_ref.py, the numpy restatement of docs/SPEC.md §2.20 (the cylinder entries of the
energy ledger): the per-contact power identity, the signs, the drive work against the friction part of M_ax, the plane as
the limit of a large cylinder, and the closure of the balance for a sphere thrown at the shell of a rotating drum."""
import functools

import numpy as np
import pytest

import cyl_history_ref as CH
import cyl_ref as Cy
import ledger_ref as Lg
import shell_ledger_ref as SL
from shpair import shapes


def unit(v):
    return np.asarray(v, float) / np.linalg.norm(v)


def frame_e1(ch):
    """The e1 of the frame rule of SPEC §2.3 about ch."""
    s = np.copysign(1.0, ch[2])
    a = -1.0 / (s + ch[2])
    return np.array([1 + s * ch[0] ** 2 * a, s * ch[0] * ch[1] * a, -s * ch[0]])


OBLIQUE_AXIS = np.array([2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0])


@functools.lru_cache(maxsize=None)
def contact(label):
    """(lmax, anm, rmax, x, q, cyl, V, S, T) of a unit sphere or a random L = 6 shape 0.7 Rmax from the wall of an oblique
    cylinder of radius 2.5 Rmax, n_q = 16."""
    from oracle import oracle as O
    lmax, anm = (0, shapes.sphere(1.0)) if label == "sphere" else (6, shapes.random_shape(6, 3, amp=0.1))
    rm = 1.01 if label == "sphere" else O.shape_rmax(6, anm)
    rng = np.random.default_rng(5)
    q = unit(rng.normal(size=4))
    ch = unit(np.cross(OBLIQUE_AXIS, rng.normal(size=3)))
    a = np.array([0.4, -0.3, 0.2])
    Rc = 2.5 * rm
    x = a + (Rc - 0.7 * rm) * ch + 0.3 * OBLIQUE_AXIS
    cyl = np.array([*a, *OBLIQUE_AXIS, Rc])
    V, S, T, st = Cy.cyl_sums(lmax, anm, rm, x, q, cyl, 16)
    assert st == 1 and V > 0
    return lmax, anm, rm, x, q, cyl, V, S, T


# twist scale, gamma, mu, gamma_t, k_t, xi going in: what each is meant to be is asserted from the reference's own answer
LAWS = {"viscous": (1.0, 3.0, 0.5, 2.0, 0.0, None), "capped": (1.0, 3.0, 0.01, 2000.0, 0.0, None),
        "clamped": (1.0, 1e6, 0.5, 2.0, 0.0, None), "stick": (1e-3, 3.0, 0.5, 2.0, 4e3, (1e-4, -2e-4)),
        "slide": (1.0, 3.0, 0.05, 2.0, 4e3, (3e-2, 1e-2))}


@pytest.mark.parametrize("label", ["sphere", "rough"])
def test_the_power_identity_holds_per_contact(oracle, label):
    """F.w + tau.omega = -p Vdot - P_d - P_f + Wdot_c to 1e-12 of the largest term, for a viscous, a capped, a clamped, a
    sticking and a sliding contact, Omega = 1.7, an oblique axis."""
    lmax, anm, rm, x, q, cyl, V, S, T = contact(label)
    rng = np.random.default_rng(8)
    seen = set()
    for name, (scale, gamma, mu, gt, kt, xi) in LAWS.items():
        for _ in range(4):
            tw = scale * np.concatenate([rng.normal(size=3), 0.5 * rng.normal(size=3)])
            if name == "clamped" and S @ tw[:3] + T @ tw[3:] > 0:
                tw = -tw                        # receding fast: p + gamma Vdot < 0
            d = SL.contact_powers(V, S, T, x, cyl, 1000.0, 1.25, tw, gamma, mu, gt, 1.7, kt, (0.0, 0.0) if xi is None else xi, 2e-3)
            Pd, Pf, Wc = d["P"]
            lhs = d["F"] @ tw[:3] + d["tau"] @ tw[3:]
            terms = (-d["p"] * d["vd"], -Pd, -Pf, Wc)
            err = abs(lhs - sum(terms)) / max(abs(t) for t in terms + (lhs,))
            kind = ("clamped" if d["pt"] == 0 else d["kind"] if kt else "capped" if d.get("capped") else "viscous")
            seen.add(kind)
            print(f"{label} {name}: kind {kind} P_d {Pd:.4g} P_f {Pf:.4g} W {Wc:.4g} lhs {lhs:.6g} err {err:.1e}")
            assert kind == name
            assert err <= 1e-12
            assert Pd >= 0.0 and (kt != 0 or Pf >= 0.0)
            if name == "clamped":               # p |Vdot|, and no normal load: the friction is dropped, with its power and work
                assert Pd == d["p"] * abs(d["vd"]) and Pf == 0.0 and Wc == 0.0 and not d["F"].any()
            else:
                assert Pf != 0.0 and Wc != 0.0
    assert seen == {"viscous", "capped", "clamped", CH.STICK, CH.SLIDE}


def test_signs_and_the_drive_work_is_minus_omega_times_the_friction_moment(oracle):
    """Over random twists, without a spring: P_d >= 0 and P_f >= 0; Wdot_c = 0 at Omega = 0; Wdot_c = -Omega M_ax,f with
    M_ax,f = a^.[(x_i - a) x (-F_t) - r_i x F_t], the friction part of the row's M_ax, to 1e-12; and the whole M_ax is another
    number: the normal wrench's axial moment, quadrature noise of the sharp rule, is not zero for the rough shape."""
    rng = np.random.default_rng(3)
    for label in ("sphere", "rough"):
        lmax, anm, rm, x, q, cyl, V, S, T = contact(label)
        a, ax = cyl[:3], cyl[3:6]
        worst = 0.0
        for k in range(40):
            tw = 10.0 ** rng.uniform(-2, 1) * np.concatenate([rng.normal(size=3), 0.5 * rng.normal(size=3)])
            mu, gt = (0.5, 2.0) if k % 2 else (0.02, 900.0)
            om = rng.normal() * 2
            d = SL.contact_powers(V, S, T, x, cyl, 1000.0, 1.25, tw, 3.0, mu, gt, om)
            assert d["P"][0] >= 0.0 and d["P"][1] >= 0.0
            still = SL.contact_powers(V, S, T, x, cyl, 1000.0, 1.25, tw, 3.0, mu, gt, 0.0)
            assert still["P"][2] == 0.0 and still["P"][1] > 0.0
            if d["pt"] == 0:
                continue
            Mf = ax @ (np.cross(x - a, -d["Ft"]) - np.cross(d["ri"], d["Ft"]))
            worst = max(worst, abs(d["P"][2] + om * Mf) / abs(om * Mf))
            assert abs(Mf + d["Ft"] @ np.cross(ax, d["rc"])) <= 1e-12 * abs(Mf)   # M_ax,f = -Rc F_t.t^_c, t^_c = a^ x rho_c / Rc
        Mn = ax @ (np.cross(x - a, d["pt"] * S) + d["pt"] * T)
        print(f"{label}: worst |W + Omega M_ax,f| / |Omega M_ax,f| {worst:.1e}; axial moment of the normal wrench {Mn:.3e} "
              f"of a friction moment {Mf:.3e}")
        assert worst <= 1e-12
        if label == "rough":
            assert abs(Mn) > 1e-6 * abs(d["pt"]) * np.linalg.norm(T)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_moving_plane_is_the_limit_of_a_large_rotating_cylinder(oracle, seed):
    """Rc = 1e8 R_i, Omega = u / Rc, the axis the e1 of the plane's frame: P_d, P_f and Wdot_c of a unit sphere agree with
    tests/ledger_ref.py's wall powers and work rate -F_w.u_w for the plane moving tangentially at u = Omega a x rho_c, to
    1e-6 (the bar of §2.18 and §2.19 in this limit), viscous and capped.  Value reached: 8.3e-8 (printed; seeds 1 and 3 reach 1.8e-9).  A sphere, whose
    S_n is along the normal to rounding: for a rough shape the two laws place the contact point apart (tests/test_cyl_ref.py)."""
    rng = np.random.default_rng(seed)
    anm, rm, nq, u = shapes.sphere(1.0), 1.01, 16, 0.9
    q, n = unit(rng.normal(size=4)), unit(rng.normal(size=3))
    h = 0.7 * rm
    x = n * h
    Rc = 1e8 * rm
    ax = frame_e1(-n)
    cyl = np.array([*(Rc * n), *ax, Rc])
    vel = (u / Rc) * np.cross(ax, -Rc * n)           # Omega a x rho_c at the contact
    tw = np.concatenate([rng.normal(size=3), 0.5 * rng.normal(size=3)])
    V, S, T, st = Cy.cyl_sums(0, anm, rm, x, q, cyl, nq)
    assert st == 1 and V > 0
    seen, worst = set(), 0.0
    for mu, gt in ((0.5, 2.0), (0.01, 2000.0)):
        d = SL.contact_powers(V, S, T, x, cyl, 1000.0, 1.25, tw, 3.0, mu, gt, u / Rc)
        P, Fw = Lg.wall_powers([(0, anm, rm)], nq, x[None], q[None], [0], tw[None], [(*n, 0.0)], [1000.0], [1.25], [3.0], [mu], [gt], [vel])
        want = np.array([P[0, 0, 0], P[0, 0, 1], -(Fw[0, 0] @ vel)])
        err = np.abs(d["P"] - want) / np.abs(want)
        seen.add(d["capped"])
        worst = max(worst, err.max())
        print(f"seed {seed} mu {mu} gamma_t {gt} capped {d['capped']}: cylinder {d['P']}, plane {want}, rel err {err}")
        assert (np.abs(want) > 0).all() and err.max() <= 1e-6
    print(f"value reached: {worst:.1e}")
    assert seen == {True, False}


@functools.lru_cache(maxsize=None)
def throw(k, elastic=False):
    return SL.thrown_sphere(k, elastic)


def test_the_balance_of_a_thrown_sphere_closes_to_first_order_in_dt(oracle):
    """shell_ledger_ref.THROW: a unit sphere thrown obliquely at the shell of a drum with gamma_c, mu_c, gamma_t,c and
    Omega = 1.5, no gravity; it meets the wall and parts again, so E_mech is kinetic at both ends.  R = |Delta E_mech -
    (W_shell - D_shell)| on the reference's own sharp-rule sums at n_q = 8: R(dt) = 6.845e-2, R(dt/2) = 3.360e-2, ratio
    0.491; elastic R0 = 2.1e-3 and 5.6e-5 (0.031 R and 0.0017 R).  The inputs are chosen here so that the reference alone meets
    tests/test_gpu_ledger.py's conditions for the planar collision: R(dt/2) <= 0.75 R(dt) and R0 <= 0.1 R."""
    R, R0 = [], []
    for k in (1, 2):
        r, e = throw(k), throw(k, True)
        R.append(SL.residual(r))
        R0.append(abs(e["E1"] - e["E0"]))
        print(f"dt/{k}: E0 {r['E0']:.6f} E1 {r['E1']:.6f} D_d {r['D_d']:.6f} D_f {r['D_f']:.6f} W {r['W']:.6f} R {R[-1]:.3e} "
              f"elastic R0 {R0[-1]:.3e}, {r['ncontact']} steps in contact, final h {r['h']:.3f}")
        assert r["ncontact"] > 100 and not r["touching"] and r["h"] > 1.01 and r["mono"]      # they met and parted
        assert e["ncontact"] > 100 and not e["touching"] and e["D_d"] == 0 and e["D_f"] == 0 and e["W"] == 0
        assert r["D_d"] > 0 and r["D_f"] > 0 and r["W"] > 0                                     # the drum drives the sphere
    print(f"R(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert R0[0] <= 0.1 * R[0] and R0[1] <= 0.1 * R[1]
    assert R[1] <= 0.75 * R[0]
