"""CPU tests of tests/history_ref.py, the numpy restatement of docs/SPEC.md §2.14, against closed form: two equal spheres
(friction_ref.lens_integrals) under a constant tangential velocity stick, then slide, then hold a load at rest; with every
k_t = 0 the reference is friction_ref.pair_friction bit for bit; the carry by key against a brute-force dictionary."""
import numpy as np

import friction_ref as F
import history_ref as H

R, DIST, KN, EXPO = 1.0, 1.9, 1e4, 1.25
MU, KT, GT, DT = 0.4, 1.0e4, 30.0, 1e-3
VT = np.array([0.0, 0.3, -0.4])                      # |v_t| = 0.5, normal to d = +x


def two_spheres(vt):
    pairs = F.lens_integrals(R, DIST)[None, :]
    x = np.array([[0.0, 0, 0], [DIST, 0, 0]])
    tw = np.zeros((2, 6))
    tw[0, :3] = vt
    t = lambda v: np.array([[0.0, 0.0], [0.0, v]])   # (ntypes+1)^2 tables of one type
    return pairs, x, tw, t


def one_pass(xi, vt, dt=DT, kt=KT, gt=GT):
    pairs, x, tw, t = two_spheres(vt)
    return H.pair_history(pairs, [0], [1], x, tw, [1, 1], [0, 0], [1.01], t(KN), t(EXPO), t(0.0), t(MU), t(gt), t(kt), xi, dt, 2)


def normal_load():
    V, S = F.lens_integrals(R, DIST)[0], F.lens_integrals(R, DIST)[1]
    return KN * EXPO * V ** (EXPO - 1) * S


def test_stick_then_slide_then_hold_in_closed_form():
    N = normal_load()
    xi = np.zeros((1, 3))
    kslip = None
    for k in range(1, 400):
        f, tq, xn, det = one_pass(xi, VT)
        trial = -KT * (k * DT * VT) - GT * VT if kslip is None else None
        if kslip is None and np.linalg.norm(trial) <= MU * N:
            assert det["kind"][0] == H.STICK
            assert np.abs(xn[0] - k * DT * VT).max() <= 1e-14 * np.abs(k * DT * VT).max()
            assert np.abs(f[0] - trial).max() <= 1e-13 * np.abs(trial).max()
        else:
            kslip = kslip or k
            assert det["kind"][0] == H.SLIDE
            assert abs(np.linalg.norm(f[0]) - MU * N) <= 1e-14 * MU * N
            # xi no longer grows: it holds what the capped force leaves the spring, (mu N - gamma_t |v_t|) / k_t
            hold = (MU * N - GT * np.linalg.norm(VT)) / KT
            assert abs(np.linalg.norm(xn[0]) - hold) <= 1e-13 * hold
        assert np.array_equal(f[1], -f[0])                       # the pair's forces cancel
        assert np.abs(np.cross([DIST / 2, 0, 0], f[0]) - tq[0]).max() <= 1e-13 * MU * N   # both at the mid point
        assert np.abs(tq[1] - tq[0]).max() <= 1e-13 * MU * N      # tau_j = -r_j x F_t, r_j = -d/2
        xi = xn
    assert kslip is not None and 10 < kslip < 390                 # both regimes were well inside the sequence
    # a pass at rest: the spring holds -k_t xi, which history-free friction cannot
    f, tq, xn, det = one_pass(xi, np.zeros(3))
    assert det["kind"][0] == H.STICK
    assert np.abs(f[0] + KT * xi[0]).max() <= 1e-14 * KT * np.abs(xi).max() and np.linalg.norm(f[0]) > 0.5 * MU * N
    assert np.array_equal(xn, xi)
    # ... and a look (dt = 0) at the same state gives the same force and leaves xi alone
    f0, _, x0, _ = one_pass(xi, np.zeros(3), dt=0.0)
    assert np.array_equal(f0, f) and np.array_equal(x0, xi)
    # gamma_t = 0 is still a history pair
    assert one_pass(xi, VT, gt=0.0)[3]["kind"][0] in (H.STICK, H.SLIDE)


def test_separated_spheres_lose_their_spring():
    pairs, x, tw, t = two_spheres(VT)
    pairs = np.zeros_like(pairs)
    f, tq, xn, det = H.pair_history(pairs, [0], [1], x, tw, [1, 1], [0, 0], [1.01], t(KN), t(EXPO), t(0.0), t(MU), t(GT), t(KT),
                                    np.ones((1, 3)), DT, 2)
    assert det["kind"][0] == H.RESET_UNTOUCHED and not xn.any() and not f.any() and not tq.any()


def random_bed(rng, n=40, ns=150):
    pi = np.sort(rng.integers(0, n - 1, ns))
    pj = np.array([rng.integers(i + 1, n) for i in pi])
    pairs = np.abs(rng.normal(size=(ns, 7))) * np.array([0.01, 1, 1, 1, 0.1, 0.1, 0.1]) * rng.choice([-1, 1], size=(ns, 7))
    pairs[:, 0] = np.abs(pairs[:, 0])
    pairs[rng.random(ns) < 0.2] = 0.0
    x = rng.uniform(0, 6, (n, 3))
    tw = rng.normal(size=(n, 6))
    ty = rng.integers(1, 3, n)
    sh = rng.integers(0, 2, n)
    tab = lambda a, b, c: np.array([[0, 0, 0], [0, a, b], [0, b, c]], float)
    return pi, pj, pairs, x, tw, ty, sh, tab


def test_without_a_spring_the_reference_is_the_friction_reference_bit_for_bit():
    rng = np.random.default_rng(5)
    pi, pj, pairs, x, tw, ty, sh, tab = random_bed(rng)
    K, E, G = tab(1000, 1200, 1400), tab(1.25, 1.25, 1.25), tab(300, 0, 900)
    MUt, GTt = tab(2.0, 1.5, 0.0), tab(300, 400, 250)
    xi = 0.05 * rng.normal(size=(len(pi), 3))
    for newton, nlocal in ((True, 40), (False, 30)):
        a = F.pair_friction(pairs, pi, pj, x, tw, ty, sh, [1.1, 1.3], K, E, G, MUt, GTt, nlocal, newton_pair=newton)
        b = H.pair_history(pairs, pi, pj, x, tw, ty, sh, [1.1, 1.3], K, E, G, MUt, GTt, tab(0, 0, 0), xi, 1e-3, nlocal, newton_pair=newton)
        assert np.abs(a[0]).max() > 0
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert not b[2].any() and not b[3]["kind"].any()          # no history pair: every xi is zeroed, no slot has a kind
    # a k_t on one type pair changes those slots and no other
    c = H.pair_history(pairs, pi, pj, x, tw, ty, sh, [1.1, 1.3], K, E, G, MUt, GTt, tab(0, 5e3, 0), xi, 1e-3, 40)
    mixed = (ty[pi] != ty[pj])
    assert (c[3]["kind"][mixed] != H.NONE).all() and (c[3]["kind"][~mixed] == H.NONE).all()
    assert set(c[3]["kind"][mixed]) >= {H.STICK, H.SLIDE, H.RESET_UNTOUCHED}
    live = np.isin(c[3]["kind"], (H.STICK, H.SLIDE))
    assert (np.linalg.norm(c[3]["Ft"][live], axis=1) <= c[3]["cap"][live] * (1 + 1e-14)).all()       # |F_t| <= mu N
    S = pairs[live, 1:4]
    assert np.abs(np.einsum("ij,ij->i", c[2][live], S)).max() <= 1e-12 * np.abs(c[2][live]).max() * np.abs(S).max()   # xi is tangential


def test_carry_by_key_against_a_dictionary():
    rng = np.random.default_rng(11)
    n = 50

    def rows(keep):
        offs, keys = [0], []
        for i in range(n):
            ks = [k for k in range(i + 1, n) if keep(i, k)]
            keys += ks
            offs.append(len(keys))
        return np.array(offs), np.array(keys)

    old_offs, old_keys = rows(lambda i, k: rng.random() < 0.15)
    old_xi = rng.normal(size=(len(old_keys), 3))
    new_offs, new_keys = rows(lambda i, k: rng.random() < 0.15)
    book = {}
    for i in range(n):
        for w in range(old_offs[i], old_offs[i + 1]):
            book[(i, old_keys[w])] = old_xi[w]
    got = H.carry(old_offs, old_keys, old_xi, new_offs, new_keys)
    kept = new = 0
    for i in range(n):
        for w in range(new_offs[i], new_offs[i + 1]):
            want = book.get((i, new_keys[w]))
            if want is None:
                assert not got[w].any()
                new += 1
            else:
                assert np.array_equal(got[w], want)
                kept += 1
    assert kept >= 10 and new >= 10 and len(book) - kept >= 10


def test_owner_tags():
    pj = np.array([1, 4, 5, 2])
    assert np.array_equal(H.owner_tags(pj, 4, gowner=[2, 0]), [1, 2, 0, 2])           # no tags: rows, ghosts through their owners
    assert np.array_equal(H.owner_tags(pj, 4, tag=np.array([10, 11, 12, 13, 12, 10])), [11, 12, 10, 12])
