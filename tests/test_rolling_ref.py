"""CPU checks of tests/rolling_ref.py, the numpy restatement of docs/SPEC.md §2.16, on a small bed of random integrals and
random motion: the properties the SPEC states for the two resisting couples (a pure couple, frame indifference,
dissipation, the two caps) and the closed form of two spheres."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import friction_ref as F  # noqa: E402
import rolling_ref as R  # noqa: E402


def _bed(seed, n=40, npairs=150, ntypes=2, gamma_scale=0.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 6, (n, 3))
    pi = rng.integers(0, n - 1, npairs)
    pj = np.array([rng.integers(i + 1, n) for i in pi])
    pairs = np.zeros((npairs, 7))
    pairs[:, 0] = rng.uniform(1e-4, 1e-2, npairs)
    pairs[:, 1:] = rng.normal(size=(npairs, 6)) * 0.1
    pairs[::7] = 0.0   # slots that did not touch
    type_ = 1 + rng.integers(0, ntypes, n)
    K = np.zeros((ntypes + 1, ntypes + 1))
    E, G, MUR, GR, MUTW, GTW = (np.ones_like(K),) + tuple(np.zeros_like(K) for _ in range(5))
    for a in range(1, ntypes + 1):
        for b in range(a, ntypes + 1):
            K[a, b] = K[b, a] = rng.uniform(500, 2000)
            E[a, b] = E[b, a] = rng.choice([1.0, 1.25, 2.0])
            G[a, b] = G[b, a] = gamma_scale * rng.uniform(0.5, 2.0)
            MUR[a, b] = MUR[b, a] = rng.uniform(0.02, 0.06)
            GR[a, b] = GR[b, a] = rng.uniform(1.0, 4.0)
            MUTW[a, b] = MUTW[b, a] = rng.uniform(0.01, 0.03)
            GTW[a, b] = GTW[b, a] = rng.uniform(1.0, 4.0)
    tw = rng.normal(size=(n, 6))
    return dict(x=x, pi=pi, pj=pj, pairs=pairs, ty=type_, K=K, E=E, G=G, MUR=MUR, GR=GR, MUTW=MUTW, GTW=GTW, tw=tw)


def _run(c, tw=None, **kw):
    return R.pair_rolling(c["pairs"], c["pi"], c["pj"], c["x"], c["tw"] if tw is None else tw, c["ty"], c["K"], c["E"], c["G"],
                          c["MUR"], c["GR"], c["MUTW"], c["GTW"], kw.pop("nlocal", len(c["x"])), **kw)


def test_a_pure_couple_the_torques_sum_to_zero_and_no_force_is_added():
    for seed in range(3):
        for gs in (0.0, 3000.0):     # alone, and with the p_tot of a damped contact
            c = _bed(seed, gamma_scale=gs)
            tq, det = _run(c)        # (the reference returns torques only: there is no force to return)
            assert det["live"].sum() > 50 and np.abs(tq).sum() > 0      # (a damped bed clamps about half)
            # sum tau = 0 and no force: linear momentum and angular momentum about ANY point are conserved
            assert np.abs(tq.sum(axis=0)).max() <= 1e-13 * np.abs(tq).sum()
            if gs:
                assert det["clamped"].any()


def test_common_rigid_motion_gives_exactly_zero():
    c = _bed(20, gamma_scale=3000.0)
    rng = np.random.default_rng(5)
    v0, Om = rng.normal(size=3), rng.normal(size=3)
    x = c["x"]
    tw = np.concatenate([v0 + np.cross(Om, x), np.broadcast_to(Om, x.shape)], axis=1)
    tq, det = _run(c, tw)
    assert det["live"].sum() > 50
    assert not tq.any() and not det["M"][det["live"]].any()      # Omega = 0: no unit vector was formed


def test_power_is_never_positive_and_both_couples_stay_under_their_caps():
    for seed in range(3):
        c = _bed(10 + seed)
        tq, det = _run(c)
        ok = det["live"]
        tw = c["tw"]
        Om = tw[c["pi"], 3:] - tw[c["pj"], 3:]
        per_slot = (det["M"][ok] * Om[ok]).sum(axis=1)               # M.Omega = -kappa_r |Omega_r|^2 - kappa_tw |Omega_n|^2
        assert ok.sum() > 80 and (per_slot <= 0).all() and (per_slot < 0).any()
        assert np.abs(per_slot + det["power"][ok]).max() <= 1e-13 * det["power"][ok].max()
        assert abs((tq * tw[:, 3:]).sum() - per_slot.sum()) <= 1e-12 * np.abs(per_slot).sum()
        S = c["pairs"][ok, 1:4]
        Sh = S / np.linalg.norm(S, axis=1)[:, None]
        Mn = (det["M"][ok] * Sh).sum(axis=1)[:, None] * Sh           # the twisting part is along S_n, the rolling part normal to it
        Mr = det["M"][ok] - Mn
        nMr, nMn = np.linalg.norm(Mr, axis=1), np.linalg.norm(Mn, axis=1)
        assert (nMr <= det["cap_r"][ok] * (1 + 1e-12)).all() and (nMn <= det["cap_tw"][ok] * (1 + 1e-12)).all()
        for cp, nM, cap, visc in ((det["capped_r"][ok], nMr, det["cap_r"][ok], det["visc_r"][ok]),
                                  (det["capped_tw"][ok], nMn, det["cap_tw"][ok], det["visc_tw"][ok])):
            assert cp.any() and (~cp).any()                          # both branches of kappa
            assert np.abs(nM[cp] - cap[cp]).max() <= 1e-12 * cap.max()
            assert np.abs(nM[~cp] - visc[~cp]).max() <= 1e-12 * visc.max()


def test_clamped_untouched_and_half_set_pairs_add_nothing():
    x = np.array([[0.0, 0, 0], [1.5, 0.2, -0.1]])
    pairs = np.array([[2e-3, 0.11, 0.02, -0.01, 0.004, -0.03, 0.02]])
    one = lambda v: np.array([[0, 0], [0, v]])
    tw = np.zeros((2, 6))
    tw[1, :3] = [3.0, 0.5, 0]      # j runs away along S_n ...
    tw[0, 3:] = [0.3, -0.2, 0.5]   # ... and i spins
    args = (pairs, [0], [1], x, tw, [1, 1], one(1000.0), np.array([[1, 1], [1, 1.25]]))
    tq, det = R.pair_rolling(*args, one(5e4), one(0.05), one(2.0), one(0.02), one(2.0), 2)
    assert det["clamped"][0] and det["N"][0] == 0.0 and not tq.any()
    tq, det = R.pair_rolling(*args, one(0.0), one(0.05), one(2.0), one(0.02), one(2.0), 2)
    assert det["live"][0] and tq[0].any() and (tq[1] == -tq[0]).all()
    for mu, g in ((0.0, 2.0), (0.05, 0.0)):     # a kind counts iff both of its coefficients are non-zero
        tq, det = R.pair_rolling(*args, one(0.0), one(mu), one(g), one(mu), one(g), 2)
        assert not det["live"][0] and not tq.any()
    tq, det = R.pair_rolling(np.zeros((1, 7)), *args[1:], one(0.0), one(0.05), one(2.0), one(0.02), one(2.0), 2)
    assert not det["touched"][0] and not tq.any()
    # x enters only through Vdot: with every gamma_ij = 0 another x gives the same bits
    a = R.pair_rolling(*args, one(0.0), one(0.05), one(2.0), one(0.02), one(2.0), 2)[0]
    b = R.pair_rolling(args[0], [0], [1], x + [[0.3, 0.1, 0.0], [-1.0, 2.0, 0.5]], *args[4:], one(0.0), one(0.05), one(2.0), one(0.02),
                       one(2.0), 2)[0]
    assert (a == b).all()


def test_two_unit_spheres_match_the_closed_form():
    """Centres 1.9 apart along x: S_n along x, N = |F_elastic| = kn m V^(m-1) |S_n|.  i spinning about x twists
    (M = -kappa_tw omega on i, +kappa_tw omega on j), about z rolls (the same with kappa_r); one rate in each branch."""
    kn, m = 1000.0, 1.25
    io = F.lens_integrals(1.0, 1.9)
    N = kn * m * io[0] ** (m - 1) * io[1]
    x = np.array([[0.0, 0, 0], [1.9, 0, 0]])
    one = lambda v: np.array([[0, 0], [0, v]])
    mur, gr, mutw, gtw = 0.05, 2.0, 0.02, 3.0
    for axis, mu, g in ((0, mutw, gtw), (2, mur, gr)):
        branch = mu * N / g
        for om, k in ((0.5 * branch, g), (4.0 * branch, mu * N / (4.0 * branch))):
            tw = np.zeros((2, 6))
            tw[0, 3 + axis] = om
            tq, det = R.pair_rolling(io[None], [0], [1], x, tw, [1, 1], one(kn), one(m), one(0.0), one(mur), one(gr), one(mutw),
                                     one(gtw), 2)
            want = np.zeros(3)
            want[axis] = -k * om
            assert abs(det["N"][0] - N) <= 1e-15 * N
            assert np.abs(tq[0] - want).max() <= 1e-15 * abs(k * om) and (tq[1] == -tq[0]).all()
            assert bool(det["capped_tw" if axis == 0 else "capped_r"][0]) == (om > branch)


def test_newton_off_keeps_ghost_rows_clean():
    c = _bed(30)
    nlocal = 25
    tq, _ = _run(c, nlocal=nlocal, newton_pair=False)
    ghost_only = np.setdiff1d(np.arange(nlocal, len(c["x"])), c["pi"])
    assert ghost_only.size and not tq[ghost_only].any()
