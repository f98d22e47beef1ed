"""tests/pair_ref.py (numpy, exact inner radii) pinned on known answers, the committed fixtures pinned on it, and the CPU
oracle held to the fixtures: the integrals that depend on no root at docs/SPEC.md §4's 1e-9, the ones that do at 1.5 x the
deviation tests/golden/root_shortcut.json records for the oracle's own search (tests/golden/make_pair_ref.py)."""
import numpy as np
import pytest

import pair_ref
from mixed_common import MIN_MIXED_SLOTS, slot_classes
from shpair import shapes

GATE = 1e-9          # SPEC §4
MARGIN = 1.5         # on a recorded figure: truncation error of one fixed search path; more is another path


@pytest.mark.parametrize("lmax", [0, 3, 6, 12, 14])
def test_gradient_against_central_differences_and_the_oracle(oracle, lmax):
    a = shapes.random_shape(lmax, 40 + lmax, amp=0.3)
    rng = np.random.default_rng(lmax)
    u = rng.normal(size=(24, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[0], u[1], u[2] = (0, 0, 1), (0, 0, -1), (1, 0, 0)          # poles and the equator
    g = pair_ref.sh_gradient(lmax, a, u)
    h = 1e-5
    fd = np.stack([(shapes.sh_radius_np(lmax, a, u + h * e) - shapes.sh_radius_np(lmax, a, u - h * e)) / (2 * h)
                   for e in np.eye(3)], axis=1)
    # F is a polynomial of degree lmax with coefficients of order amp: h^2/6 |F'''| <= ~1e-10 lmax^3, rounding 1e-16 / h
    assert np.abs(g - fd).max() < 1e-6 * (1.0 + np.abs(g).max())
    go = np.array([oracle.sh_eval(lmax, a, v, grad=True)[1] for v in u])
    assert np.abs(g - go).max() <= 1e-12 * max(1.0, np.abs(go).max())


@pytest.mark.parametrize("R,r,d", [(1.0, 1.0, 1.9), (1.0, 0.7, 1.5), (0.8, 1.3, 1.9), (1.0, 1.0, 1.5)])
def test_spheres_with_exact_bounding_radius_give_the_lens_volume(R, r, d):
    """rho^2 >= R_i^2 + R_j^2: every ray that crosses the lens ends inside j, V is exact (SPEC §2.5) and every cap node is
    inside, so the rule is spectrally accurate.  Cases and bars of the oracle's own lens test."""
    rng = np.random.default_rng(1)
    c = rng.normal(size=3)
    c /= np.linalg.norm(c)
    xi = rng.normal(size=3)
    qi = np.array([np.cos(0.35), *(np.sin(0.35) * np.array([1, 2, 3]) / np.sqrt(14))])
    qj = np.array([np.cos(0.95), *(np.sin(0.95) * np.array([3, 1, -2]) / np.sqrt(14))])
    o = pair_ref.pair_slot((0, shapes.sphere(R), R), (0, shapes.sphere(r), r), xi, qi, xi + d * c, qj, 24)
    lens = np.pi * (R + r - d) ** 2 * (d * d + 2 * d * (R + r) - 3 * (R - r) ** 2) / (12 * d)
    a2 = R * R - ((d * d + R * R - r * r) / (2 * d)) ** 2
    assert o["nin"] == 2 * 24 * 24 and o["branch"] == 2 and not o["multi"] and o["resid"] < 1e-12
    assert abs(o["V"] - lens) < 1e-8 * lens
    assert np.abs(o["S"] - np.pi * a2 * c).max() < 1e-12
    assert np.abs(o["T"]).max() < 1e-13


def test_cap_branches_and_the_centre_inside_branch():
    sph = lambda R: (0, shapes.sphere(R), R)
    q0 = np.array([1.0, 0, 0, 0])
    far = pair_ref.pair_slot(sph(1.0), sph(1.0), [0, 0, 0], q0, [0, 0, 2.0], q0, 8)
    assert far["branch"] == -1 and far["nin"] == 0 and far["V"] == 0.0
    same = pair_ref.pair_slot(sph(1.0), sph(1.0), [1, 2, 3], q0, [1, 2, 3], q0, 8)
    assert same["branch"] == -1 and not same["S"].any()
    cone = pair_ref.pair_slot(sph(1.0), sph(1.0), [0, 0, 0], q0, [0, 0, 1.2], q0, 32)
    assert cone["branch"] == 1 and 0 < cone["nin"] < 2 * 32 * 32
    assert abs(cone["S"][2] - np.pi * (1 - 0.36)) < 0.02 * np.pi * (1 - 0.36)
    # the whole of a small particle inside a big sphere: V = integral r^3 / 3, the closed surface has no vector area
    small = shapes.random_shape(4, 2, amp=0.2)
    rs = 1.01 * shapes.sh_radius_np(4, small, shapes._sphere_grid(32)[0]).max()
    full = pair_ref.pair_slot((4, small, rs), sph(2.02), [0, 0, 0], q0, [0.5, 0, 0], q0, 16)
    u, wg, _, _ = shapes._sphere_grid(24)
    vol = np.sum(shapes.sh_radius_np(4, small, u) ** 3 / 3.0 * wg)
    assert full["branch"] == 0 and full["rin0"] and full["nin"] == 2 * 16 * 16
    assert abs(full["V"] - vol) < 1e-3 * vol and np.abs(full["S"]).max() < 1e-3


def test_assemble_newton_rule_and_momentum_balance():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(4, 3))
    pairs = dict(V=np.array([0.02, 0.0, 0.01]), S=rng.normal(size=(3, 3)), T=rng.normal(size=(3, 3)))
    nlist = (np.array([0, 1]), np.array([0, 2, 3]), np.array([1, 3, 2]))
    ty = np.array([1, 2, 1, 2])
    K, E = pair_ref.kn_table(2, 1.25)
    f, tq, e = pair_ref.assemble(pairs, nlist, x, ty, K, E, 4, True)
    assert np.abs(f.sum(0)).max() < 1e-12 and np.abs((tq + np.cross(x, f)).sum(0)).max() < 1e-12
    assert not f[3].any()                                    # V = 0: the slot does not touch
    p0 = 1500.0 * 1.25 * 0.02 ** 0.25                       # types 1 and 2: kn = 500 (1 + 2)
    assert np.allclose(f[0], -p0 * pairs["S"][0]) and np.allclose(tq[0], -p0 * pairs["T"][0])
    assert np.isclose(e, 1500.0 * (0.02 ** 1.25 + 0.01 ** 1.25))
    f2, tq2, e2 = pair_ref.assemble(pairs, nlist, x, ty, K, E, 2, False)     # atoms 2, 3 are ghosts
    assert np.array_equal(f2[:2], f[:2]) and not f2[2:].any() and not tq2[2:].any()
    assert np.isclose(e2, 1500.0 * (0.02 ** 1.25 + 0.5 * 0.01 ** 1.25))


@pytest.fixture(scope="module")
def shortcut():
    return pair_ref.load_shortcut()


@pytest.mark.parametrize("name", pair_ref.CASES)
def test_fixture_meets_the_recorder_s_conditions(name, shortcut):
    g = pair_ref.load_fixture(name)
    touch = g["V"] > 0
    flagged = touch & g["multi"]
    if name == "soup":
        assert min((touch & (g["branch"] == b)).sum() for b in (0, 1, 2)) >= 3 and (touch & g["rin0"]).sum() >= 3
    else:
        assert touch.sum() >= 40
    assert len(g["x"]) <= 80 and (g["resid"] <= 1e-12 * g["rmax"][g["shtype"][g["jlist"]]]).all()
    assert flagged.sum() <= 0.05 * touch.sum()
    if "own_lmax" in g:          # shapes of several orders: both mixed orientations among the touching slots
        cls = slot_classes(g["own_lmax"], g["shtype"], *g["nlist"], touch)
        print(name, cls)
        assert g["lmax"] == g["own_lmax"].max() and cls["low-high"] >= MIN_MIXED_SLOTS and cls["high-low"] >= MIN_MIXED_SLOTS, cls
        for l, a in zip(g["own_lmax"], g["a_nm"]):
            assert not a[(l + 1) * (l + 2):].any()
    rec = shortcut[name]
    assert (rec["n_slots"], rec["n_touching"], rec["n_flagged"]) == (touch.size, touch.sum(), flagged.sum())


@pytest.mark.parametrize("name", pair_ref.CASES)
def test_fixture_rows_are_the_reference_s(name):
    """Six seeded touching slots per fixture, recomputed."""
    g = pair_ref.load_fixture(name)
    slots = np.sort(np.random.default_rng(7).choice(np.flatnonzero(g["V"] > 0), 6, replace=False))
    r = pair_ref.pair_list(g["shape_table"], g["nq"], g["x"], g["quat"], g["shtype"], *g["nlist"], slots=slots)
    for k in ("nin", "branch", "rin0", "multi"):
        assert np.array_equal(r[k], g[k][slots]), k
    assert np.abs(r["V"] - g["V"][slots]).max() <= 1e-13 * g["V"][slots].max()
    for k in ("S", "T"):
        assert (np.abs(r[k] - g[k][slots]).max(axis=1) <= 1e-13 * np.abs(g[k][slots]).max(axis=1)).all(), k


@pytest.mark.parametrize("name", pair_ref.CASES)
def test_oracle_against_the_exact_root_reference(oracle, shortcut, name):
    g = pair_ref.load_fixture(name)
    rec = shortcut[name]
    newton = bool(g["newton"])
    touch = g["V"] > 0
    flagged = touch & g["multi"]
    args = (g["nq"], g["nlocal"], g["x"], g["quat"], g["type"], g["shtype"])
    K, E = pair_ref.kn_table(g["ntypes"], 1.0)
    o = oracle.compute(g["shape_table"], K, E, *args, *g["nlist"], newton_pair=newton, force_volume=True, want_pairs=True)
    got = o["pairs"]
    # what depends on no root: classification, surface sums, the m = 1 wrench and its assembly -- every slot
    assert np.array_equal(got[:, 0] > 0, touch) and o["counts"][2] == touch.sum()
    assert np.abs(got[:, 1:4] - g["S"]).max() <= GATE * np.abs(g["S"]).max()
    assert np.abs(got[:, 4:7] - g["T"]).max() <= GATE * np.abs(g["T"]).max()
    f, tq, _ = pair_ref.assemble(g, g["nlist"], g["x"], g["type"], K, E, g["nlocal"], newton)
    df, dt = pair_ref.deviations(o["f"], o["torque"], f, tq)
    assert df <= GATE and dt <= GATE
    if not newton:
        assert not o["f"][g["nlocal"]:].any() and not f[g["nlocal"]:].any()
    # what depends on the accepted roots
    cmp_v = touch & ~flagged
    vdev = np.abs(got[cmp_v, 0] - g["V"][cmp_v]) / g["V"][cmp_v]
    print(name, "V", vdev.max(), "recorded", rec["v_dev_max"])
    assert vdev.max() <= MARGIN * rec["v_dev_max"]
    short = pair_ref.without_slots(g["nlist"], flagged)
    for m in (1.25, 2.0):
        K, E = pair_ref.kn_table(g["ntypes"], m)
        o = oracle.compute(g["shape_table"], K, E, *args, *short, newton_pair=newton, force_volume=True, eflag=True)
        f, tq, e = pair_ref.assemble(g, g["nlist"], g["x"], g["type"], K, E, g["nlocal"], newton, skip=flagged)
        df, dt = pair_ref.deviations(o["f"], o["torque"], f, tq)
        print(name, m, "F", df, "tau", dt, "recorded", rec["f_dev"][repr(m)], rec["tau_dev"][repr(m)])
        assert df <= MARGIN * rec["f_dev"][repr(m)] and dt <= MARGIN * rec["tau_dev"][repr(m)]
        assert abs(o["eng_virial"][0] - e) <= MARGIN * rec["v_dev_max"] * m * e
