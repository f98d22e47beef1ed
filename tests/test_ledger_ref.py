"""CPU checks of tests/ledger_ref.py, the numpy restatement of docs/SPEC.md §2.13, on the small beds of
dissipation_common.bed_case with the ORACLE's integrals: the identity the energy ledger rests on — the powers it counts
are minus the power of the dissipative wrench — for pairs and for moving walls, their sign, a common rigid motion, and
the first-order closure of the balance on a two-sphere collision, where the inputs of the GPU closure test are chosen."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import damp_ref as D  # noqa: E402
import friction_ref as F  # noqa: E402
import ledger_ref as LR  # noqa: E402
import wall_move_ref as M  # noqa: E402
import wall_ref as W  # noqa: E402
from common import coeff_tables, oracle_compute  # noqa: E402
from dissipation_common import NQ, bed_case, motion, _rigid_motion  # noqa: E402

TOL = 1e-12      # rounding only: of the largest term of the sum
GAMMA = {(1, 1): 300.0, (1, 2): 900.0, (2, 2): 1800.0}                          # tests/test_gpu_friction.py's
FRIC = {(1, 1): (2.0, 300.0), (1, 2): (1.5, 400.0), (2, 2): (2.5, 250.0)}
# the collision of the closure tests (here and tests/test_gpu_ledger.py): chosen on the two references below
COLLISION = dict(gamma=2e4, kn=1e4, m=1.25, vrel=6.0, dt=1e-4, nsteps=1400, nq=32)


def table(coef, k=None):
    G = np.zeros((3, 3))
    for (a, b), g in coef.items():
        G[a, b] = G[b, a] = g if k is None else g[k]
    return G


def _pair_inputs(oracle, n, seed, v, L, expo=1.25):
    case = bed_case(oracle, n, seed)
    K, E = coeff_tables(2, lambda i, j: 1000.0 + 100.0 * (i + j), expo)
    b = case["bed"]
    o = oracle_compute(oracle, case, NQ, K, E, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], case["offsets"], case["jlist"])
    if v is None:
        v, L = motion(case, 8)
    elif v == "rigid":
        v, L = _rigid_motion(case, np.array([0.3, -0.2, 0.5]), np.array([0.4, 0.7, -0.5]))
    tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
    return (o["pairs"], pi, pj, b["x"], tw, b["type"], b["shtype"], case["rmax"], K, E), case


def test_pair_powers_are_minus_the_power_of_the_dissipative_wrench(oracle):
    for n, seed, expo in ((12, 2, 1.25), (60, 1, 1.25), (60, 1, 1.0)):
        for gamma, fric in ((GAMMA, {}), ({}, FRIC), (GAMMA, FRIC)):
            a, case = _pair_inputs(oracle, n, seed, None, None, expo)
            tabs = (table(gamma), table(fric, 0), table(fric, 1))
            P = LR.pair_powers(*a, *tabs, case["n"], shared=False)
            f, tq, _ = F.pair_friction(*a, *tabs, case["n"])
            tw = a[4]
            terms = np.concatenate([(f * tw[:, :3]).ravel(), (tq * tw[:, 3:]).ravel()])
            assert (P >= 0).all() and P.sum() > 0
            assert bool(gamma) == bool(P[:, 0].any()) and bool(fric) == bool(P[:, 1].any())
            assert abs(P.sum() + terms.sum()) <= TOL * max(np.abs(terms).max(), P.max()) * np.sqrt(terms.size)
            # with every share 1 the shared rows are the rows; newton off and a ghost j: half of it
            assert np.array_equal(LR.pair_powers(*a, *tabs, case["n"]), P)
            half = LR.pair_powers(*a, *tabs, case["n"] // 2, newton_pair=False)
            ghost = a[2] >= case["n"] // 2
            assert ghost.any() and np.array_equal(half[ghost], 0.5 * P[ghost]) and np.array_equal(half[~ghost], P[~ghost])


def test_pair_powers_of_a_common_rigid_motion_vanish(oracle):
    a, case = _pair_inputs(oracle, 60, 1, "rigid", None)
    tabs = (table(GAMMA), table(FRIC, 0), table(FRIC, 1))
    P = LR.pair_powers(*a, *tabs, case["n"])
    moving = LR.pair_powers(*_pair_inputs(oracle, 60, 1, None, None)[0], *tabs, case["n"])
    # exactly 0 in exact arithmetic; Vdot and v_t are differences of O(1) velocities, the powers their squares
    print(f"rigid motion: largest power {P.max():.3e} against {moving.max():.3e} of a random motion")
    assert (P >= 0).all() and P.max() <= 1e-24 * moving.max()


def _wall_inputs(oracle):
    """The bed of bed_case(12) on a floor that rises and slides, beside a belt: both touched, and by some particles both."""
    case = bed_case(oracle, 12, 2)
    b = case["bed"]
    shapes = [(4, a, r) for a, r in zip(case["shapes"], case["rmax"])]
    x = b["x"]
    planes = np.array([[0.0, 0, 1, x[:, 2].min() - 0.8], [1.0, 0, 0, x[:, 0].min() - 0.85]])
    vel = np.array([[0.3, 0.0, 0.5], [0.0, 1.0, 0.0]])
    co = (np.array([1000.0, 800.0]), np.array([1.25, 1.0]), np.array([400.0, 250.0]), np.array([0.5, 0.3]), np.array([200.0, 400.0]))
    return case, shapes, planes, vel, co


def test_wall_powers_are_minus_the_power_of_the_dissipative_wrench_against_the_moving_wall(oracle):
    case, shapes, planes, vel, co = _wall_inputs(oracle)
    b = case["bed"]
    kn, expo, gamma, mu, gt = co
    for v, L in (motion(case, 8), _rigid_motion(case, np.array([0.3, -0.2, 0.5]), np.zeros(3))):
        tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
        for u in (vel, np.zeros((2, 3))):
            a = (shapes, NQ, b["x"], b["quat"], b["shtype"])
            P, Fw = LR.wall_powers(*a, tw, planes, kn, expo, gamma, mu, gt, u)
            full = M.wall_forces_moving(*a, tw, planes, kn, expo, gamma, mu, gt, u)
            el = W.wall_forces(*a, planes, kn, expo)
            assert ((P > 0).any(axis=(0, 2))).all() and ((P[:, 0] > 0).any(axis=1) & (P[:, 1] > 0).any(axis=1)).any()   # both walls; one particle at both
            assert (P >= 0).all()
            assert np.abs(Fw.sum(axis=0) - full["wall_out"][:, 1:]).max() <= TOL * np.abs(full["wall_out"]).max()
            # per wall the identity needs the per-wall wrench; summed over the walls it is the rows' (w - u_w differs per
            # wall, so the reference is evaluated one wall at a time)
            for w in range(2):
                one = lambda r: (r[w:w + 1],)
                fw = M.wall_forces_moving(*a, tw, planes[w:w + 1], kn[w:w + 1], expo[w:w + 1], gamma[w:w + 1], mu[w:w + 1], gt[w:w + 1], u[w:w + 1])
                ew = W.wall_forces(*a, planes[w:w + 1], kn[w:w + 1], expo[w:w + 1])
                df, dt_ = fw["f"] - ew["f"], fw["torque"] - ew["torque"]
                terms = np.concatenate([(df * (tw[:, :3] - u[w])).ravel(), (dt_ * tw[:, 3:]).ravel()])
                assert abs(P[:, w].sum() + terms.sum()) <= TOL * max(np.abs(terms).max(), P.max()) * np.sqrt(terms.size), w
            per, tot = LR.wall_ledger(P, Fw, u, dt=0.5)
            assert np.array_equal(tot, per.sum(axis=0)) and (per[:, 2] == 0).all() == (not u.any())
    # a bed that translates with a wall and does not spin: no power at that wall
    u = np.array([[0.3, -0.2, 0.5], [0.0, 0.0, 0.0]])
    v, L = _rigid_motion(case, u[0], np.zeros(3))
    tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
    P, _ = LR.wall_powers(shapes, NQ, b["x"], b["quat"], b["shtype"], tw, planes, kn, expo, gamma, mu, gt, u)
    assert P[:, 0].max() <= 1e-24 * P[:, 1].max() and P[:, 1].max() > 0


def _closure(integrals=None):
    c = COLLISION
    R, R0, out = [], [], []
    for k in (1, 2):
        kw = dict(vrel=c["vrel"], dt=c["dt"] / k, nsteps=c["nsteps"] * k, integrals=integrals)
        E0, E1, Dd, mono, s = LR.sphere_collision_ledger(c["gamma"], c["kn"], c["m"], **kw)
        e0, e1, d0, _, s0 = LR.sphere_collision_ledger(0.0, c["kn"], c["m"], **kw)
        # they met and parted again (beyond the bounding spheres), D never fell, and a substantial part of the energy went
        assert mono and d0 == 0.0 and s > 2.02 and s0 > 2.02 and 0.3 * E0 < Dd < E0
        R.append(abs(E1 - E0 + Dd))
        R0.append(abs(e1 - e0))
        out.append(f"dt {c['dt'] / k:g}: E0 {E0:.6f} D {Dd:.6f} R {R[-1]:.4e} R/D {R[-1] / Dd:.2e} R0 {R0[-1]:.2e}")
    print("\n".join(out), f"\nR(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert 0.4 <= R[1] / R[0] <= 0.6
    assert R0[0] <= 0.1 * R[0] and R0[1] <= 0.1 * R[1]


def test_two_sphere_collision_closes_the_balance_to_first_order_in_dt():
    """R(dt) = |E_mech(end) - E_mech(0) + D| of the head-on collision COLLISION (two unit spheres, L = 0, closed-form lens,
    the loop's time levels) at dt = 1e-4 (1400 steps) and 5e-5 (2800 steps).  Reference values: E_mech(0) = 37.699112;
    gamma = 2e4: D = 35.96278 / 35.85916, R = 2.0757e-1 / 1.0336e-1, ratio 0.498, R / D = 5.8e-3 / 2.9e-3;
    gamma = 0: R0 = 2.2e-5 / 1.8e-6.  The GPU closure test (tests/test_gpu_ledger.py) runs these inputs."""
    _closure()


def test_the_collision_clears_the_sharp_rules_stepping_force(oracle):
    """The same run with the ORACLE's integrals at the n_q of the GPU test in place of the closed-form lens: what the
    kernels integrate.  Head-on, S_n steps whenever a ring of nodes enters or leaves the cap, and the leapfrog turns every
    step of the force into an energy error of order dt |jump| v with no fixed sign: an elastic-only residual R0 that the
    closed-form lens does not have and that falls with dt only on average (at gamma = 1e4, v = 2, dt = 4e-4 / 2e-4 it is
    8.3e-4 / 5.9e-3 against R = 1.27e-2 / 6.2e-3: the condition R0 <= 0.1 R cannot hold there).  R grows with gamma v,
    the steps of the force do not know gamma: so the inputs are a fast, heavily damped collision.  Reference values at
    n_q = 32: D = 35.96841 / 35.86349, R = 2.1070e-1 / 1.0584e-1, ratio 0.502, R0 = 2.0e-3 / 1.2e-3 (1 % of R)."""
    _closure(LR.oracle_sphere_integrals(COLLISION["nq"]))
