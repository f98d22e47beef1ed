"""Builders for the tests of contexts that mix shapes of different orders (CPU and GPU): beds and pair soups like those
of tests/common.py with one order per shape, the zero-padding of a coefficient vector, and the count of touching slots
by (order of i, order of j).

One rule for every comparison: the references evaluate each shape at its OWN order, the library gets each shape at its
own order, and both get the same explicit bounding radius (the default radius comes from a sample grid that depends on
the order, so it is never left to either side)."""
import numpy as np

from shpair import shapes, bed


def pad_anm(l, L, anm):
    """The coefficients of an order-l shape as an order-L vector: the storage is n-major (docs/SPEC.md §1), so the
    padding is a tail of exact zeros."""
    a = np.asarray(anm, dtype=np.float64).ravel()
    assert L >= l and a.size == (l + 1) * (l + 2)
    out = np.zeros((L + 1) * (L + 2))
    out[:a.size] = a
    return out


def mixed_shapes(orders, seed, amp):
    return [shapes.sphere(1.0) if l == 0 else shapes.random_shape(l, 1000 * seed + 17 * s + l, amp=amp)
            for s, l in enumerate(orders)]


def make_mixed_case(n, orders, seed=0, amp=0.1, spacing=1.9, ntypes=1, skin=0.1, rmax_fn=None):
    """make_case of tests/common.py with a tuple of orders, one per shape.  rmax_fn(l, anm) at the shape's own order."""
    orders = tuple(int(l) for l in orders)
    shp = mixed_shapes(orders, seed, amp)
    rmax = [rmax_fn(l, a) for l, a in zip(orders, shp)]
    b = bed.make_bed(n, rmax, len(orders), spacing=spacing, seed=bed.SEED0 + seed)
    if ntypes > 1:
        b["type"] = (1 + np.arange(n) % ntypes).astype(np.int32)
    il, of, jl = bed.half_neighbor_list(b["x"], b["shtype"], rmax, skin=skin)
    return dict(lmax=max(orders), orders=orders, shapes=shp, rmax=rmax, bed=b, ilist=il, offsets=of, jlist=jl, ntypes=ntypes, n=n)


def make_mixed_soup(orders, rmax_fn, npair=400, seed=None, far=2.6):
    """make_soup of tests/common.py with one order per shape: isolated random pairs from deep overlap (centre of i inside
    j, full-sphere cap, tangent-cone cap) to grazing.  Atoms 2p, 2p + 1 are pair p; row 2p holds the one slot.  far: the
    largest separation (make_soup's 2.6 leaves few of the far pairs touching; a smaller one keeps more of the lens branch)."""
    orders = tuple(int(l) for l in orders)
    rng = np.random.default_rng(1000 + sum(orders) if seed is None else seed)
    shp = [shapes.random_shape(l, 300 + s, amp=0.35) for s, l in enumerate(orders)]
    rmax = [rmax_fn(l, a) for l, a in zip(orders, shp)]
    x = np.zeros((2 * npair, 3))
    q = rng.normal(size=(2 * npair, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    sh = rng.integers(0, len(orders), size=2 * npair).astype(np.int32)
    sep = np.concatenate([rng.uniform(0.15, 0.9, npair // 4), rng.uniform(0.9, 1.6, npair // 4),
                          rng.uniform(1.6, far, npair - 2 * (npair // 4))])
    for p in range(npair):
        d = rng.normal(size=3)
        d *= sep[p] / np.linalg.norm(d)
        x[2 * p] = (20.0 * p, 0.0, 0.0)
        x[2 * p + 1] = x[2 * p] + d
    il = np.arange(2 * npair, dtype=np.int32)
    of = np.zeros(2 * npair + 1, np.int32)
    of[1::2] = np.arange(1, npair + 1)
    of[2::2] = np.arange(1, npair + 1)
    jl = (2 * np.arange(npair) + 1).astype(np.int32)
    ty = np.ones(2 * npair, np.int32)
    return dict(lmax=max(orders), orders=orders, shapes=shp, rmax=rmax, x=x, quat=q, type=ty, shtype=sh, sep=sep, ilist=il,
                offsets=of, jlist=jl, npair=npair)


def own_tuples(case):
    """[(l, anm, rmax)] for the references: every shape at its own order."""
    return [(l, a, r) for l, a, r in zip(case["orders"], case["shapes"], case["rmax"])]


def padded_tuples(case):
    """The same shapes zero-padded to the largest order, the same radii."""
    L = case["lmax"]
    return [(L, pad_anm(l, L, a), r) for l, a, r in zip(case["orders"], case["shapes"], case["rmax"])]


def mixed_oracle_compute(O, case, nq, K, E, padded=False, **kw):
    b = case["bed"]
    nlocal = kw.pop("nlocal", case["n"])
    return O.compute(padded_tuples(case) if padded else own_tuples(case), K, E, nq, nlocal, b["x"], b["quat"], b["type"],
                     b["shtype"], case["ilist"], case["offsets"], case["jlist"], **kw)


def slot_rows(ilist, offsets):
    """The atom i of every slot of a CSR list."""
    return np.repeat(np.asarray(ilist), np.diff(np.asarray(offsets)))


def slot_classes(orders, shtype, ilist, offsets, jlist, touching):
    """Touching slots by (order of i, order of j) against the largest order: dict with the keys "low-low", "low-high",
    "high-low", "high-high".  touching: one flag per slot, from a reference's per-slot volumes alone."""
    o = np.asarray(orders)
    hi = o == o.max()
    sh = np.asarray(shtype)
    i = slot_rows(ilist, offsets)
    j = np.asarray(jlist) & 0x1FFFFFFF
    t = np.asarray(touching, dtype=bool)
    assert i.size == j.size == t.size
    hi_i, hi_j = hi[sh[i]], hi[sh[j]]
    return {"low-low": int((t & ~hi_i & ~hi_j).sum()), "low-high": int((t & ~hi_i & hi_j).sum()),
            "high-low": int((t & hi_i & ~hi_j).sum()), "high-high": int((t & hi_i & hi_j).sum())}


def mixed_ctx(case, nq, K, E, padded=False, neighbors=True):
    """A context with every shape at its own order (padded: zero-padded to the largest by the caller) and the case's
    explicit bounding radii, which the library must keep as they are."""
    from shpair import ShPair
    sp = ShPair(0)
    sp.settings(nq)
    nt = K.shape[0] - 1
    sp.set_ntypes(nt, len(case["shapes"]))
    for s, (l, a, r) in enumerate(padded_tuples(case) if padded else own_tuples(case)):
        sp.set_shape(s, l, a, r)
        assert sp.rmax(s) == r
    for i in range(1, nt + 1):
        for j in range(1, nt + 1):
            sp.coeff(i, j, K[i, j], E[i, j])
    if neighbors:
        sp.set_neighbors_csr(case["ilist"], case["offsets"], case["jlist"])
    return sp


# The beds of the bed-level tests: name -> (orders, n_q, particles, keyword arguments of make_mixed_case).  Seeds, sizes
# and spacing were chosen on the CPU so that the oracle finds at least 30 touching slots in each of low-high and high-low
# (asserted where a bed is used); 150 particles where n_q >= 24.
BEDS = {
    "o0_6": ((0, 6), 16, 260, dict(seed=601)),
    "o4_6_2": ((4, 6, 2), 16, 260, dict(seed=602)),
    "o0_4": ((0, 4), 10, 260, dict(seed=603)),
    "o3_12_q32": ((3, 12), 32, 150, dict(seed=604)),
    "o3_12_q20": ((3, 12), 20, 260, dict(seed=605)),
    "o5_9": ((5, 9), 12, 260, dict(seed=606, ntypes=2)),
    "o3_6": ((3, 6), 7, 260, dict(seed=607)),
    "o12_13": ((12, 13), 8, 260, dict(seed=608)),
    "o0_20": ((0, 20), 24, 150, dict(seed=609)),
    "o2_6": ((2, 6), 16, 260, dict(seed=610)),
    "o4_6": ((4, 6), 16, 260, dict(seed=611)),
}
MIN_MIXED_SLOTS = 30


def bed_case(name, rmax_fn):
    orders, nq, n, kw = BEDS[name]
    return make_mixed_case(n, orders, rmax_fn=rmax_fn, **kw), nq


def assert_mixed_slots(case, pairs, nrows=None):
    """At least MIN_MIXED_SLOTS touching slots with a low-order i on a high-order j and as many the other way round,
    counted from a reference's per-slot volumes.  Returns the four counts."""
    cls = slot_classes(case["orders"], case["bed"]["shtype"], case["ilist"][:nrows],
                       case["offsets"][:None if nrows is None else nrows + 1], case["jlist"][:len(pairs)], pairs[:, 0] > 0)
    assert cls["low-high"] >= MIN_MIXED_SLOTS and cls["high-low"] >= MIN_MIXED_SLOTS, cls
    return cls


# ---- walls: orders (0, 4, 6), 200 particles, three planes (a floor, a side wall and an oblique plane, as the box of
# tests/test_gpu_wall.py has them)
WALL_ORDERS = (0, 4, 6)
WALL_NQ = 16


def wall_case(rmax_fn, n=200, seed=77, edge=4.0, margin=0.35):
    s3 = 1.0 / np.sqrt(3.0)
    planes = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [s3, s3, s3, 2.5]], dtype=np.float64)
    rng = np.random.default_rng(seed)
    x = np.zeros((0, 3))
    while x.shape[0] < n:
        p = rng.uniform(0, edge, size=(4 * n, 3))
        h = p @ planes[:, :3].T - planes[:, 3]
        x = np.concatenate([x, p[(h >= margin).all(axis=1)]])
    x = x[:n].copy()
    shp = mixed_shapes(WALL_ORDERS, 70, 0.1)
    rmax = [rmax_fn(l, a) for l, a in zip(WALL_ORDERS, shp)]
    return dict(lmax=max(WALL_ORDERS), orders=WALL_ORDERS, shapes=shp, rmax=rmax, x=x, quat=bed.random_quaternions(n, rng),
                shtype=rng.integers(0, len(WALL_ORDERS), n).astype(np.int32), planes=planes, n=n,
                kn=np.array([1000.0, 800.0, 1200.0]), expo=np.array([1.0, 1.25, 2.0]))


def soup_branches(soup, pairs):
    """Touching pairs of a soup by the cap branch of docs/SPEC.md §2.2 (0: rho <= R_j, the full sphere; 1: the tangent
    cone of j's bounding sphere; 2: the lens of the two bounding spheres) and by orientation (order of i below / above
    the order of j): a [3][2] table of counts.  pairs: a reference's per-slot rows (touching: V > 0)."""
    o = np.asarray(soup["orders"])
    r = np.asarray(soup["rmax"])
    si, sj = soup["shtype"][0::2], soup["shtype"][1::2]
    Ri, Rj, rho = r[si], r[sj], soup["sep"]
    branch = np.where(rho <= Rj, 0, np.where(rho * rho - Rj * Rj <= Ri * Ri, 1, 2))
    touching = np.asarray(pairs)[:, 0] > 0
    out = np.zeros((3, 2), dtype=int)
    for b in range(3):
        out[b, 0] = (touching & (branch == b) & (o[si] < o[sj])).sum()
        out[b, 1] = (touching & (branch == b) & (o[si] > o[sj])).sum()
    return out


# The soup of the cap-branch tests: 400 isolated pairs of the orders (1, 5, 9); seed and largest separation chosen on the
# CPU so that the oracle finds at least 20 touching pairs in every cap branch and orientation (asserted where it is used).
SOUP_ORDERS = (1, 5, 9)
MIN_BRANCH_PAIRS = 20


def soup_case(rmax_fn):
    return make_mixed_soup(SOUP_ORDERS, rmax_fn, npair=400, seed=11, far=2.2)


# ---- the whole step: 24 particles of the orders (2, 4) at n_q = 8 on two hcp layers above a floor, periodic in x, with
# gravity and drag, pair damping, history-free friction, rolling and twisting, every seventh row frozen (frozen=True) and
# the ledger on.  The bed drifts along +x fast enough for one rebuild in STEP_NSTEPS steps.  The whole-step reference
# (tests/traj_ref.py) takes one order, so it gets the shapes zero-padded to the largest; the library gets each shape at
# its own order and the scene's bounding radii.
STEP_ORDERS = (2, 4)
STEP_NQ = 8
STEP_NSTEPS = 10
STEP_MARGIN = 1.0e-6          # of a rebuild decision, as tests/golden/make_traj_ref.py asks
STEP_BAR_FACTOR = 10.0        # bar = 10 D_q, as there
STEP_NOISE_SEED = 20261020
MIN_CROSS_MIXED = 5           # slots in contact that join a low-order and a high-order row of different ranks


def step_scene(frozen):
    import traj_ref as TR
    L, spacing = max(STEP_ORDERS), 1.9
    own = [shapes.random_shape(l, 8100 + 17 * s, amp=0.2) for s, l in enumerate(STEP_ORDERS)]
    shp = [pad_anm(l, L, a) for l, a in zip(STEP_ORDERS, own)]
    dx, dy, dz = spacing, spacing * np.sqrt(3.0) / 2.0, spacing * np.sqrt(2.0 / 3.0)
    k, j, i = (a.ravel() for a in np.meshgrid(np.arange(2), np.arange(3), np.arange(4), indexing="ij"))
    pts = np.stack([(i + 0.5 * (j % 2) + 0.5 * (k % 2)) * dx, (j + (k % 2) / 3.0) * dy, k * dz], axis=1)
    hi_x = 4 * dx                                # two bricks of 3.8 along x, each wider than the ghost cutoff
    pts[:, 0] = np.mod(pts[:, 0] + 0.9, hi_x)
    n = len(pts)
    rng = np.random.default_rng(4712)
    x = pts + rng.uniform(-0.05, 0.05, pts.shape)
    lo = np.array([0.0, x[:, 1].min() - 3.0, x[:, 2].min() - 3.0])
    hi = np.array([hi_x, x[:, 1].max() + 3.0, x[:, 2].max() + 3.0])
    quat = bed.random_quaternions(n, rng)
    shtype = (np.arange(n) % 2).astype(np.int32)
    rng.shuffle(shtype)
    type_ = (1 + rng.integers(0, 2, n)).astype(np.int32)
    mask = np.ones(n, np.int32)
    if frozen:
        mask[::7] = 4                            # outside the group: frozen
    v = np.array([9.0, 0.0, 0.0]) + 1.5 * rng.normal(size=(n, 3))
    ang = 1.2 * rng.normal(size=(n, 3))
    v[mask == 4], ang[mask == 4] = 0.0, 0.0
    K, E = np.zeros((3, 3)), np.ones((3, 3))
    K[1:, 1:], E[1:, 1:] = [[1000.0, 1500.0], [1500.0, 2000.0]], [[1.25, 1.5], [1.5, 1.25]]
    sc = TR.scene(L, STEP_NQ, shp, [1.3, 0.8], x, v, quat, ang, type_, shtype, lo, hi, (1, 0, 0), 0.3, 2.0e-3, K, E, mask=mask,
                  gravity=(0.0, 0.0, -9.81), gamma_t=0.05, gamma_r=0.02, pair_damping={(1, 1): 30.0, (2, 2): 800.0},
                  pair_friction={(1, 1): (0.5, 20.0), (1, 2): (0.4, 40.0)}, pair_rolling={(1, 1): (0.02, 2.0), (1, 2): (0.03, 1.0)},
                  pair_twisting={(1, 2): (0.02, 1.5), (2, 2): (0.03, 1.0)}, planes=[[0.0, 0.0, 1.0, x[:, 2].min() - 0.93]],
                  wall_kn=[2000.0], wall_expo=[1.25], wall_damping=[3000.0], wall_mu=[0.5], wall_gt=[20.0], ledger=True)
    sc["own_lmax"] = np.array(STEP_ORDERS, np.int32)
    return sc


def step_reference(frozen, grid=(2, 1, 1)):
    """The reference run of step_scene, and everything the tests take from it alone: dict with the scene `sc`, the last
    snapshot `last`, the set-up snapshot `setup`, per step `rebuilt` and `margin`, the deviation `D` of the reference from
    itself with every integral scaled by 1 + 1e-12 eta, the bars 10 D, and `cross_mixed`: the slots (i, owner of j) found
    in contact in some force pass that join a low-order and a high-order row owned by different bricks of `grid`
    (traj_ref.brick_owner on the rows of the latest build)."""
    import traj_ref as TR
    sc = step_scene(frozen)
    order = sc["own_lmax"][sc["shtype"]]
    cross = set()

    def tally(st):
        n = len(st["x"])
        brick = TR.brick_owner(st["xhold"], sc["lo"], sc["hi"], sc["periodic"], grid)
        owner = np.concatenate([np.arange(n), st["own"]])
        i = np.repeat(np.arange(n), np.diff(st["offs"]))
        j = owner[st["jl"]]
        hit = st["touch"] & (order[i] != order[j]) & (brick[i] != brick[j]).any(axis=1)
        cross.update(zip(i[hit].tolist(), j[hit].tolist()))

    st = TR.setup(sc)
    tally(st)
    setup, recs = TR.snapshot(st), []
    for _ in range(STEP_NSTEPS):
        recs.append(TR.step(sc, st))
        tally(st)
    last = TR.snapshot(st)
    noisy, nrecs = TR.run(sc, STEP_NSTEPS, noise=np.random.default_rng(STEP_NOISE_SEED))
    assert [r["rebuilt"] for r in nrecs] == [r["rebuilt"] for r in recs]
    D = TR.deviation(noisy[f"step{STEP_NSTEPS}"], last)
    return dict(sc=sc, setup=setup, last=last, rebuilt=[r["rebuilt"] for r in recs], margin=[r["margin"] for r in recs],
                touching=[r["counts"]["touching"] for r in recs], D=D, bar={q: STEP_BAR_FACTOR * D[q] for q in D},
                cross_mixed=sorted(cross))


def assert_step_conditions(ref, frozen):
    """The conditions on the whole-step scene, from the reference alone: 24 particles of both orders, a rebuild within the
    run whose decision margins are at least STEP_MARGIN, contacts throughout, every ledger column filled, frozen rows as
    asked, and at least MIN_CROSS_MIXED slots in contact that join a low-order and a high-order row of different bricks."""
    sc = ref["sc"]
    assert len(sc["x"]) == 24 and int(sc["lmax"]) == max(STEP_ORDERS) and np.bincount(sc["shtype"]).min() >= 8
    assert sum(ref["rebuilt"]) >= 1 and min(ref["margin"]) >= STEP_MARGIN
    assert min(ref["touching"]) >= 40 and ref["last"]["ledger"][:4].min() > 0
    assert frozen == bool((sc["mask"] != 1).any())
    assert len(ref["cross_mixed"]) >= MIN_CROSS_MIXED, ref["cross_mixed"]
