"""CPU checks of tests/friction_ref.py, the numpy restatement of docs/SPEC.md §2.11, on random integrals: the properties
the SPEC states for the friction wrench (momentum, angular momentum, frame indifference, dissipation, Coulomb's cap, the
contact point)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import friction_ref as F  # noqa: E402


def _random_pairs(seed, n=40, npairs=150, ntypes=2, gamma_scale=0.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 6, (n, 3))
    pi = rng.integers(0, n - 1, npairs)
    pj = np.array([rng.integers(i + 1, n) for i in pi])
    pairs = np.zeros((npairs, 7))
    pairs[:, 0] = rng.uniform(1e-4, 1e-2, npairs)
    pairs[:, 1:] = rng.normal(size=(npairs, 6)) * 0.1
    pairs[::7] = 0.0   # slots that did not touch
    type_ = 1 + rng.integers(0, ntypes, n)
    shtype = rng.integers(0, 2, n)
    rmax = np.array([1.0, 1.3])
    K = np.zeros((ntypes + 1, ntypes + 1))
    E, G, MU, GT = np.ones_like(K), np.zeros_like(K), np.zeros_like(K), np.zeros_like(K)
    for a in range(1, ntypes + 1):
        for b in range(a, ntypes + 1):
            K[a, b] = K[b, a] = rng.uniform(500, 2000)
            E[a, b] = E[b, a] = rng.choice([1.0, 1.25, 2.0])
            G[a, b] = G[b, a] = gamma_scale * rng.uniform(0.5, 2.0)
            MU[a, b] = MU[b, a] = rng.uniform(0.2, 0.6)
            GT[a, b] = GT[b, a] = rng.uniform(10.0, 40.0)
    tw = rng.normal(size=(n, 6))
    return dict(x=x, pi=pi, pj=pj, pairs=pairs, ty=type_, sh=shtype, rmax=rmax, K=K, E=E, G=G, MU=MU, GT=GT, tw=tw)


def _run(c, tw=None, **kw):
    return F.pair_friction(c["pairs"], c["pi"], c["pj"], c["x"], c["tw"] if tw is None else tw, c["ty"], c["sh"], c["rmax"],
                           c["K"], c["E"], c["G"], c["MU"], c["GT"], kw.pop("nlocal", len(c["x"])), **kw)


def test_momentum_and_angular_momentum_are_conserved():
    for seed in range(3):
        for gs in (0.0, 3000.0):     # friction alone, and with damping
            c = _random_pairs(seed, gamma_scale=gs)
            f, tq, det = _run(c)
            x = c["x"]
            scale = np.abs(f).sum()
            assert scale > 0 and det["fric"].sum() > 100
            assert np.abs(f.sum(axis=0)).max() <= 1e-13 * scale
            assert np.abs((np.cross(x, f) + tq).sum(axis=0)).max() <= 1e-13 * (np.abs(np.cross(x, f)).sum() + np.abs(tq).sum())


def test_common_rigid_motion_gives_no_force():
    c = _random_pairs(20, gamma_scale=3000.0)
    rng = np.random.default_rng(5)
    v0, Om = rng.normal(size=3), rng.normal(size=3)
    x = c["x"]
    tw = np.concatenate([v0 + np.cross(Om, x), np.broadcast_to(Om, x.shape)], axis=1)
    f, tq, det = _run(c, tw)
    ok = det["fric"]
    assert ok.sum() > 100
    # |r_i| of random integrals is not small: the cancellation is in v_rel, at rounding size of the velocities
    arm = np.abs(det["ri"][ok]).max()
    assert np.abs(det["vrel"][ok]).max() <= 1e-13 * np.abs(tw).max() * (1 + arm)
    assert np.abs(f).max() <= 1e-12 * c["GT"].max() * np.abs(tw).max() * (1 + arm)


def test_power_is_never_positive_and_the_force_stays_under_coulombs_cap():
    for seed in range(3):
        c = _random_pairs(10 + seed)
        f, tq, det = _run(c)
        ok = det["fric"]
        per_slot = (det["Ft"][ok] * det["vrel"][ok]).sum(axis=1)      # F_t.v_rel = -kappa |v_t|^2
        assert ok.sum() > 100 and (per_slot <= 0).all() and (per_slot < 0).any()
        tw = c["tw"]
        power = (f * tw[:, :3]).sum() + (tq * tw[:, 3:]).sum()        # every gamma_ij = 0: the pass is friction alone
        assert power < 0 and abs(power - per_slot.sum()) <= 1e-12 * np.abs(per_slot).sum()
        Ft = np.linalg.norm(det["Ft"][ok], axis=1)
        assert (Ft <= det["cap"][ok] * (1 + 1e-14)).all()
        cp = det["capped"][ok]
        assert cp.any() and (~cp).any()                               # both branches of kappa
        assert np.abs(Ft[cp] - det["cap"][ok][cp]).max() <= 1e-14 * det["cap"][ok].max()
        assert np.abs(Ft[~cp] - det["visc"][ok][~cp]).max() <= 1e-14 * det["visc"][ok].max()
        # tangential: no component along S_n
        S = c["pairs"][ok, 1:4]
        assert np.abs((det["Ft"][ok] * S).sum(axis=1)).max() <= 1e-13 * (Ft * np.linalg.norm(S, axis=1)).max()


def test_a_clamped_contact_and_a_pair_at_rest_have_no_friction():
    x = np.array([[0.0, 0, 0], [1.5, 0.2, -0.1]])
    pairs = np.array([[2e-3, 0.11, 0.02, -0.01, 0.004, -0.03, 0.02]])
    one = lambda v: np.array([[0, 0], [0, v]])
    tw = np.zeros((2, 6))
    tw[1, :3] = [3.0, 0.5, 0]      # j runs away along S_n and slides
    args = (pairs, [0], [1], x, tw, [1, 1], [0, 0], [1.0], one(1000.0), np.array([[1, 1], [1, 1.25]]))
    f, tq, det = F.pair_friction(*args, one(5e4), one(0.5), one(20.0), 2)
    assert det["N"][0] == 0.0 and not det["Ft"][0].any()
    f, tq, det = F.pair_friction(*args, one(0.0), one(0.5), one(20.0), 2)
    assert det["N"][0] > 0 and det["Ft"][0].any()
    f, tq, det = F.pair_friction(pairs, [0], [1], x, np.zeros((2, 6)), [1, 1], [0, 0], [1.0], one(1000.0), one(1.25), one(0.0), one(0.5),
                                 one(20.0), 2)
    assert not f.any() and not tq.any()                   # v_t = 0: exactly zero, no unit tangent was formed
    # mu or gamma_t zero: no friction
    for mu, gt in ((0.0, 20.0), (0.5, 0.0)):
        f, tq, det = F.pair_friction(*args, one(0.0), one(mu), one(gt), 2)
        assert not det["fric"][0] and not f.any()


def test_sphere_pair_contact_point_is_the_midpoint():
    for dist in (1.9, 1.7):
        io = F.lens_integrals(1.0, dist)
        d = np.array([dist, 0.0, 0.0])
        ri = F.contact_point(io[1:4], io[4:7], d, 1.01, 1.01)
        assert np.abs(ri - d / 2).max() <= 4e-16 * dist      # to rounding of (d.S) S / |S|^2
    # unequal bounding radii, S_n along d (what two bounding spheres give): exactly on their radical plane
    d = np.array([1.8, 0.4, -0.3])
    S = 0.3 * d
    T = np.cross(np.array([0.2, -0.1, 0.4]), S)           # a wrench through the point (0.2, -0.1, 0.4)
    Ri, Rj = 1.0, 1.4
    ri = F.contact_point(S, T, d, Ri, Rj)
    assert abs((ri @ ri - Ri ** 2) - ((ri - d) @ (ri - d) - Rj ** 2)) <= 1e-14 * 4        # equal power w.r.t. both spheres ...
    assert np.abs(np.cross(ri, S) - T).max() <= 1e-15                                        # ... on the line of action
    # S_n oblique to d: still on the line of action, at the fraction t of d.S_n along it
    S = np.array([0.3, 0.1, -0.2])
    T = np.cross(np.array([0.2, -0.1, 0.4]), S)
    ri = F.contact_point(S, T, d, Ri, Rj)
    t = 0.5 * (1 + (Ri ** 2 - Rj ** 2) / (d @ d))
    assert np.abs(np.cross(ri, S) - T).max() <= 1e-15 and abs(ri @ S - t * (d @ S)) <= 1e-15


def test_wall_contact_point_is_on_the_plane():
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        x, c = rng.normal(size=3), rng.normal()
        S, T = rng.normal(size=3), rng.normal(size=3)
        ri = F.wall_contact_point(S, T, n, n @ x - c)
        assert abs(n @ (x + ri) - c) <= 1e-13 * (1 + np.abs(ri).max() + np.abs(x).max())
        rp = np.cross(S, T) / (S @ S)
        assert np.abs(np.cross(ri - rp, n)).max() <= 1e-13 * (1 + np.abs(ri).max())   # dropped along the wall normal


def test_newton_off_keeps_ghost_rows_clean():
    c = _random_pairs(30)
    nlocal = 25
    f, tq, _ = _run(c, nlocal=nlocal, newton_pair=False)
    ghost_only = np.setdiff1d(np.arange(nlocal, len(c["x"])), c["pi"])
    assert ghost_only.size and not f[ghost_only].any() and not tq[ghost_only].any()
