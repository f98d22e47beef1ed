"""CPU-only checks of tests/wall_roll_ref.py, the numpy restatement of docs/SPEC.md §2.17: the properties the section states,
on random contacts; both branches of both kinds occur; and the hand-made wrong variants of the reference module (the
normal taken from S_n, a missing cap, a sign flip, u_w subtracted from Omega) are each rejected by one of these checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wall_roll_ref as WR   # noqa: E402

EPS = 1e-12     # relative: a few roundings of products of O(1) factors


def _contacts(seed=5, n=400):
    """Random contacts: a unit normal, an S_n up to ~25 degrees off -n (the quadrature's error, exaggerated), the row's
    force -F_i = p_tot S_n + an in-plane friction part, omega over three decades, a wall velocity, coefficients."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        S = -nrm * rng.uniform(0.05, 0.5) + 0.1 * rng.normal(size=3) * rng.uniform(0.05, 0.5)
        pt = rng.uniform(50.0, 500.0) if k % 9 else 0.0        # every ninth one clamped
        t = rng.normal(size=3)
        t -= (t @ nrm) * nrm
        Fw = pt * S + (0.3 * pt * np.linalg.norm(S)) * t
        if k % 11 == 0:
            Fw = -Fw                                            # a row that pulls: N = 0
        om = rng.normal(size=3) * 10.0 ** rng.uniform(-2, 1)
        out.append(dict(Fw=Fw, nrm=nrm, S=S, omega=om, uw=rng.normal(size=3), mur=0.05, gr=3.0, mutw=0.03, gtw=2.0))
    return out


def _law(variant=None):
    return lambda c, omega=None, **kw: WR.couple(c["Fw"], c["nrm"], c["omega"] if omega is None else omega,
                                                 kw.get("mur", c["mur"]), kw.get("gr", c["gr"]), kw.get("mutw", c["mutw"]),
                                                 kw.get("gtw", c["gtw"]), variant=variant, S=c["S"], uw=c["uw"])


# ---- the properties of §2.17, each a function of the law, so that the variants can be held to them too --------------------

def check_power(law):
    for c in _contacts():
        M, P, _, N = law(c)
        assert M @ c["omega"] <= EPS * (np.linalg.norm(M) * np.linalg.norm(c["omega"]) + 1e-300)
        assert P >= 0 and abs(M @ c["omega"] + P) <= 1e-9 * max(P, 1e-300)


def check_caps(law):
    for c in _contacts():
        M, _, _, _ = law(c)
        N = max(0.0, -(c["nrm"] @ c["Fw"]))                     # the load of the section, not the law's own
        Mn = (M @ c["nrm"]) * c["nrm"]
        assert np.linalg.norm(M - Mn) <= c["mur"] * N * (1 + 1e-9) + 1e-300
        assert np.linalg.norm(Mn) <= c["mutw"] * N * (1 + 1e-9) + 1e-300


def check_rest_is_exactly_zero(law):
    for c in _contacts():
        M, P, _, _ = law(c, omega=np.zeros(3))
        assert not M.any() and P == 0.0


def check_the_two_spins_meet_one_couple_each(law):
    for c in _contacts():
        N = max(0.0, -(c["nrm"] @ c["Fw"]))
        if not N > 0:
            continue
        w = np.linalg.norm(c["omega"])
        about = law(c, omega=w * c["nrm"], mur=0.0)[0]          # twisting only: the law with rolling switched off ...
        both = law(c, omega=w * c["nrm"])[0]
        assert np.abs(both - about).max() <= 1e-9 * (np.abs(both).max() + 1e-300) and both.any()     # ... is the whole law
        t = np.cross(c["nrm"], [1.0, 0.3, -0.2])
        t *= w / np.linalg.norm(t)
        inplane = law(c, omega=t, mutw=0.0)[0]
        both = law(c, omega=t)[0]
        assert np.abs(both - inplane).max() <= 1e-9 * (np.abs(both).max() + 1e-300) and both.any()


CHECKS = (check_power, check_caps, check_rest_is_exactly_zero, check_the_two_spins_meet_one_couple_each)


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_the_law_has_the_stated_properties(check):
    check(_law())


def test_both_branches_of_both_kinds_occur_and_a_dead_load_adds_nothing():
    got = {}
    for k, c in enumerate(_contacts()):
        M, P, br, N = _law()(c)
        got[(k, 0)] = br
        if not N > 0:
            assert not M.any() and P == 0.0 and br == (WR.NONE, WR.NONE)
    counts = WR.branch_counts(got)
    print(counts)
    assert all(v >= 20 for v in counts.values()), counts
    # a kind needs both of its coefficients
    c = next(c for c in _contacts() if -(c["nrm"] @ c["Fw"]) > 0)
    assert not _law()(c, mur=0.0, mutw=0.0)[0].any() and not _law()(c, gr=0.0, gtw=0.0)[0].any()
    assert _law()(c, mur=0.0)[2][0] == WR.NONE and _law()(c, gtw=0.0)[2][1] == WR.NONE


# which check rejects which wrong law
REJECTED_BY = {"normal_from_S": check_the_two_spins_meet_one_couple_each, "no_cap": check_caps, "sign_flip": check_power,
               "minus_uw": check_rest_is_exactly_zero}


@pytest.mark.parametrize("variant", WR.VARIANTS)
def test_a_wrong_variant_is_rejected(variant):
    assert set(REJECTED_BY) == set(WR.VARIANTS)
    with pytest.raises(AssertionError):
        REJECTED_BY[variant](_law(variant))


def test_the_pass_sums_the_walls_of_a_particle_and_leaves_the_force_alone(oracle):
    """wall_roll on a corner contact of a sphere (three walls): the couple is the sum of the three, f and wall_out are those
    of the same pass with every coefficient of §2.17 at 0, and the load from the row is p_tot |S_n| up to the quadrature."""
    from shpair import shapes
    anm = shapes.sphere(1.0)
    planes = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    x, q = np.array([[0.93, 0.95, 0.9], [5.0, 5.0, 0.99]]), np.array([[1.0, 0, 0, 0]] * 2)
    tw = np.array([[0.1, -0.2, 0.05, 0.7, -0.4, 2.0], [0, 0, 0, 0.0, 0.0, 0.0]])
    sums = WR.reach_sums([(0, anm, 1.01)], 8, x, q, np.zeros(2, int), planes)
    assert set(sums) == {(0, 0), (0, 1), (0, 2), (1, 2)}
    kn, m, z = np.full(3, 1e4), np.full(3, 1.25), np.zeros(3)
    mur, gr, mutw, gtw = np.array([0.05, 0.0, 0.02]), np.array([3.0, 3.0, 500.0]), np.array([0.0, 0.03, 0.03]), np.array([2.0, 2.0, 2.0])
    on = WR.wall_roll(sums, 2, x, tw, planes, kn, m, mur, gr, mutw, gtw, gamma=np.full(3, 500.0), mu=np.full(3, 0.3), gt=np.full(3, 20.0))
    off = WR.wall_roll(sums, 2, x, tw, planes, kn, m, z, z, z, z, gamma=np.full(3, 500.0), mu=np.full(3, 0.3), gt=np.full(3, 20.0))
    assert np.array_equal(on["f"], off["f"]) and np.array_equal(on["wall_out"], off["wall_out"])
    assert not off["couple"].any() and on["couple"][0].any() and not on["couple"][1].any()        # omega = 0: exactly nothing
    assert np.abs(on["torque"] - on["couple"] - off["torque"]).max() <= 1e-14 * np.abs(on["torque"]).max()
    assert on["branch"][(0, 0)][1] == WR.NONE and on["branch"][(0, 1)][0] == WR.NONE              # the kinds follow the walls
    assert on["branch"][(0, 2)][0] == WR.CAPPED
    for k in sums:
        assert abs(on["N"][k] - on["NS"][k]) <= 1e-9 * on["NS"][k]                                # a sphere: S_n is along n_w
