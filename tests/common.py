"""Shared builders for the bed-level tests (CPU and GPU)."""
import numpy as np

from shpair import shapes, bed


def make_case(n, lmax, nshapes, seed=0, amp=0.1, spacing=1.9, ntypes=1, skin=0.1, rmax_fn=None):
    """Synthetic bed + half list. rmax_fn(lmax, anm) -> bounding radius (oracle or library helper)."""
    shp = [shapes.random_shape(lmax, 1000 * seed + 17 * s + lmax, amp=amp) for s in range(nshapes)]
    rmax = [rmax_fn(lmax, a) for a in shp]
    b = bed.make_bed(n, rmax, nshapes, spacing=spacing, seed=bed.SEED0 + seed)
    if ntypes > 1:
        b["type"] = (1 + np.arange(n) % ntypes).astype(np.int32)
    il, of, jl = bed.half_neighbor_list(b["x"], b["shtype"], rmax, skin=skin)
    return dict(lmax=lmax, shapes=shp, rmax=rmax, bed=b, ilist=il, offsets=of, jlist=jl, ntypes=ntypes, n=n)


def make_soup(lmax, rmax_fn, npair=240):
    """Isolated random pairs from deep overlap (centre of i inside j, full-sphere cap, tangent-cone cap) to grazing:
    a quarter of the separations in [0.15, 0.9), a quarter in [0.9, 1.6), half in [1.6, 2.6).  Atoms 2p, 2p + 1 are
    pair p; three shapes."""
    rng = np.random.default_rng(1000 + lmax)
    shp = [shapes.random_shape(lmax, 300 + s, amp=0.35) for s in range(3)]
    rmax = [rmax_fn(lmax, a) for a in shp]
    x = np.zeros((2 * npair, 3))
    q = rng.normal(size=(2 * npair, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    sh = rng.integers(0, 3, size=2 * npair).astype(np.int32)
    sep = np.concatenate([rng.uniform(0.15, 0.9, npair // 4), rng.uniform(0.9, 1.6, npair // 4),
                          rng.uniform(1.6, 2.6, npair - 2 * (npair // 4))])
    for p in range(npair):
        d = rng.normal(size=3)
        d *= sep[p] / np.linalg.norm(d)
        x[2 * p] = (20.0 * p, 0.0, 0.0)
        x[2 * p + 1] = x[2 * p] + d
    il = np.arange(2 * npair, dtype=np.int32)
    of = np.zeros(2 * npair + 1, np.int32)
    of[1:] = np.repeat(np.arange(1, npair + 1), 2)
    of[1::2] = np.arange(1, npair + 1)
    of[2::2] = np.arange(1, npair + 1)
    jl = (2 * np.arange(npair) + 1).astype(np.int32)
    ty = np.ones(2 * npair, np.int32)
    return dict(lmax=lmax, shapes=shp, rmax=rmax, x=x, quat=q, type=ty, shtype=sh, sep=sep, ilist=il, offsets=of, jlist=jl,
                npair=npair)


def coeff_tables(ntypes, kn=1000.0, expo=1.0):
    """(ntypes+1)^2 tables; kn/expo scalars or symmetric functions of (i,j)."""
    K = np.zeros((ntypes + 1, ntypes + 1))
    E = np.ones((ntypes + 1, ntypes + 1))
    for i in range(1, ntypes + 1):
        for j in range(1, ntypes + 1):
            K[i, j] = kn(i, j) if callable(kn) else kn
            E[i, j] = expo(i, j) if callable(expo) else expo
    return K, E


def oracle_compute(O, case, nq, K, E, **kw):
    b = case["bed"]
    nlocal = kw.pop("nlocal", case["n"])
    return O.compute([(case["lmax"], a, r) for a, r in zip(case["shapes"], case["rmax"])], K, E, nq, nlocal,
                     b["x"], b["quat"], b["type"], b["shtype"], case["ilist"], case["offsets"], case["jlist"], **kw)


def rel_err(a, b, scale=None):
    scale = scale if scale is not None else np.abs(b).max()
    return np.abs(np.asarray(a) - np.asarray(b)).max() / scale


def random_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def random_boxes(rmax, ntrials=40, seed=2026):
    """The boxes of the property tests of SPEC §7: any mix of periodic / open directions, edges down to the minimum
    2 c_max, particles outside open faces, one to a few hundred particles, dense and dilute.  Yields one dict per trial
    (trial, periodic, skin, cmax, edge, lo, hi, n, x, quat, type, shtype); rmax: bounding radii of the two shapes."""
    rng = np.random.default_rng(seed)
    for trial in range(ntrials):
        periodic = tuple(int(v) for v in rng.integers(0, 2, 3))
        skin = float(rng.choice([0.0, 0.05, 0.4]))
        cmax = 2 * rmax.max() + skin
        edge = np.where(np.array(periodic, bool), rng.uniform(2.0 * cmax + 1e-9, 5 * cmax, 3), rng.uniform(0.3, 6 * cmax, 3))
        lo = rng.uniform(-5, 5, 3)
        hi = lo + edge
        n = int(rng.choice([1, 2, 7, 60, 300]))
        x = lo + rng.uniform(-0.2, 1.2, (n, 3)) * edge      # some outside: wrapped if periodic, clamped into edge cells if not
        if trial % 5 == 0:
            x[: n // 2] = x[0] + rng.normal(0, 0.3, (n // 2, 3))   # a dense clump: long rows
        yield dict(trial=trial, periodic=periodic, skin=skin, cmax=cmax, edge=edge, lo=lo, hi=hi, n=n, x=x,
                   quat=random_quats(rng, n), type=np.ones(n, np.int32), shtype=rng.integers(0, 2, n).astype(np.int32))
