"""CPU checks of tests/damp_ref.py, the numpy restatement of docs/SPEC.md §2.10, on random integrals: the properties the
SPEC states for the damping wrench (momentum, angular momentum, dissipation, frame indifference, no pull)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import damp_ref as D  # noqa: E402


def _random_pairs(seed, n=40, npairs=150, ntypes=2, gamma_scale=3000.0):
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
    E = np.ones_like(K)
    G = np.zeros_like(K)
    for a in range(1, ntypes + 1):
        for b in range(a, ntypes + 1):
            K[a, b] = K[b, a] = rng.uniform(500, 2000)
            E[a, b] = E[b, a] = rng.choice([1.0, 1.25, 2.0])
            G[a, b] = G[b, a] = gamma_scale * rng.uniform(0.5, 2.0)
    tw = rng.normal(size=(n, 6))
    return x, pi, pj, pairs, type_, K, E, G, tw


def test_momentum_and_angular_momentum_are_conserved():
    for seed in range(3):
        x, pi, pj, pairs, ty, K, E, G, tw = _random_pairs(seed)
        f, tq = D.pair_damping(pairs, pi, pj, x, tw, ty, K, E, G, len(x))
        scale = np.abs(f).sum()
        assert scale > 0
        assert np.abs(f.sum(axis=0)).max() <= 1e-13 * scale
        assert np.abs((np.cross(x, f) + tq).sum(axis=0)).max() <= 1e-13 * (np.abs(np.cross(x, f)).sum() + np.abs(tq).sum())


def test_power_is_never_positive_and_equals_minus_delta_vdot():
    for seed in range(3):
        x, pi, pj, pairs, ty, K, E, G, tw = _random_pairs(10 + seed)
        f, tq, det = D.pair_damping(pairs, pi, pj, x, tw, ty, K, E, G, len(x), details=True)
        ok = ~np.isnan(det[:, 0])
        per_slot = -det[ok, 0] * det[ok, 1]
        assert ok.sum() > 100 and (per_slot <= 0).all() and (per_slot < 0).any()
        power = (f * tw[:, :3]).sum() + (tq * tw[:, 3:]).sum()
        assert power < 0 and abs(power - per_slot.sum()) <= 1e-12 * np.abs(per_slot).sum()
        # both branches of the clamp occur in this input
        clamped = det[ok, 0] == -det[ok, 2]
        assert clamped.any() and (~clamped).any()


def test_common_rigid_motion_is_not_damped():
    x, pi, pj, pairs, ty, K, E, G, _ = _random_pairs(20)
    rng = np.random.default_rng(5)
    v0, Om = rng.normal(size=3), rng.normal(size=3)
    tw = np.concatenate([v0 + np.cross(Om, x), np.broadcast_to(Om, x.shape)], axis=1)
    f, tq, det = D.pair_damping(pairs, pi, pj, x, tw, ty, K, E, G, len(x), details=True)
    ok = ~np.isnan(det[:, 0])
    elastic = (det[ok, 2][:, None] * np.abs(pairs[ok, 1:4])).max()
    assert np.abs(det[ok, 1]).max() <= 1e-13 * np.abs(pairs[:, 1:]).max() * np.abs(tw).max() * 10
    assert np.abs(f).max() <= 1e-12 * elastic and np.abs(tq).max() <= 1e-12 * elastic


def test_clamped_contact_carries_exactly_no_force():
    """A pair that separates fast enough: p_tot = 0, and elastic + damping is exactly zero — the contact never pulls."""
    x = np.array([[0.0, 0, 0], [1.5, 0.2, -0.1]])
    pairs = np.array([[2e-3, 0.11, 0.02, -0.01, 0.004, -0.03, 0.02]])
    K, E, G = np.array([[0, 0], [0, 1000.0]]), np.array([[1, 1], [1, 1.25]]), np.array([[0, 0], [0, 5e4]])
    tw = np.zeros((2, 6))
    tw[1, :3] = [3.0, 0, 0]      # j runs away along S_n: Vdot = -S_n.w_j < 0
    f, tq, det = D.pair_damping(pairs, [0], [1], x, tw, [1, 1], K, E, G, 2, details=True)
    delta, vd, p = det[0]
    assert vd < 0 and p + G[1, 1] * vd < 0 and delta == -p
    S, T = pairs[0, 1:4], pairs[0, 4:7]
    assert np.array_equal(-p * S + f[0], np.zeros(3)) and np.array_equal(-p * T + tq[0], np.zeros(3))
    assert np.array_equal(p * S + f[1], np.zeros(3))
    # and one that approaches is pushed harder
    tw[1, :3] = [-3.0, 0, 0]
    _, _, det = D.pair_damping(pairs, [0], [1], x, tw, [1, 1], K, E, G, 2, details=True)
    assert det[0, 1] > 0 and det[0, 0] == max(0.0, det[0, 2] + G[1, 1] * det[0, 1]) - det[0, 2] > 0


def test_newton_off_keeps_ghost_rows_clean_and_untouched_slots_add_nothing():
    x, pi, pj, pairs, ty, K, E, G, tw = _random_pairs(30)
    nlocal = 25
    f, tq = D.pair_damping(pairs, pi, pj, x, tw, ty, K, E, G, nlocal, newton_pair=False)
    ghost_only = np.setdiff1d(np.arange(nlocal, len(x)), pi)
    assert ghost_only.size and not f[ghost_only].any() and not tq[ghost_only].any()
    zero = np.zeros_like(pairs)
    f0, t0 = D.pair_damping(zero, pi, pj, x, tw, ty, K, E, G, len(x))
    assert not f0.any() and not t0.any()
    # forces-only integrals (V not computed, exponent 1): S_n != 0 decides, p = kn
    nov = pairs.copy()
    nov[:, 0] = 0.0
    f1, _, det = D.pair_damping(nov, pi, pj, x, tw, ty, K, np.ones_like(E), G, len(x), needv=False, details=True)
    ok = ~np.isnan(det[:, 0])
    assert f1.any() and np.array_equal(det[ok, 2], K[ty[pi[ok]], ty[pj[ok]]])
