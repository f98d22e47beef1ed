"""Helpers of the multi-rank GPU tests (tests/test_gpu_mrank.py, tests/test_gpu_mrank_damp.py,
tests/test_gpu_mrank_friction.py): the ranks are host threads on the one GPU that share an in-process hub.  The bed of
the dissipation tests: L = 4, n_q = 8, two random shapes (amp 0.2), periodic_hcp(3000, 1.9) with jitter 0.15, skin 0.2,
kn = 400, m = 1.25, random v (|v| ~ 0.3) and angmom drawn per tag."""
import threading

import numpy as np

LMAX, NQ, SKIN = 4, 8, 0.2
GAMMA = 2000.0        # static tests: both branches of max(0, p + gamma Vdot) on the bed at rest speeds
GAMMA_LOOP = 40.0     # the loops at dt = 2e-3
NBED = 3000
DT = 2e-3


def _ctx(lmax, shp, nq, kn=400.0, expo=1.25):
    from shpair import ShPair
    sp = ShPair(0)
    sp.settings(nq)
    sp.set_ntypes(1, len(shp))
    for s, a in enumerate(shp):
        sp.set_shape(s, lmax, a)
    sp.coeff(1, 1, kn, expo)
    return sp


def _bed(n_target, periodic, nshapes=2, jitter=0.15, seed=9):
    from shpair import bed
    pts, lo, hi = bed.periodic_hcp(n_target, 1.9, periodic)
    rng = np.random.default_rng(seed)
    n = pts.shape[0]
    x = pts + rng.uniform(-jitter, jitter, pts.shape)
    quat = bed.random_quaternions(n, rng)
    sht = rng.integers(0, nshapes, n).astype(np.int32) if nshapes > 1 else np.zeros(n, np.int32)
    return x, quat, sht, np.arange(n, dtype=np.int32), lo, hi, rng


def _run_ranks(world, body):
    """body(rank) in one thread per rank; re-raises the first failure."""
    out, errs = [None] * world, []

    def work(r):
        try:
            out[r] = body(r)
        except BaseException as e:  # noqa: BLE001
            import traceback
            errs.append((r, repr(e), traceback.format_exc()))
    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs[0]
    return out


def _distribute(grid, lo, hi, periodic, cut, x):
    from shpair import mrank
    g0 = mrank.plan_geometry(grid, lo, hi, periodic, cut, 0)
    return mrank.plan_owner(g0, x)   # (wrapped x, owner)


def _shapes():
    from shpair import shapes
    return [shapes.random_shape(LMAX, 400 + s, amp=0.2) for s in range(2)]


def _motion(n):
    """v (|v| ~ 0.3) and angmom of every particle, by tag."""
    rng = np.random.default_rng(77)
    return 0.3 / np.sqrt(3.0) * rng.normal(size=(n, 3)), 0.1 * rng.normal(size=(n, 3))


def _masses(shp):
    sp = _ctx(LMAX, shp, NQ)
    m = np.array([sp.body(s)[0] for s in range(len(shp))])
    sp.close()
    return m


def _wrap(dx, lo, hi, periodic):
    for d in range(3):
        if periodic[d]:
            dx[:, d] -= (hi[d] - lo[d]) * np.round(dx[:, d] / (hi[d] - lo[d]))
    return dx


def _setup(grid, periodic, nbed=NBED):
    from shpair import mrank
    shp = _shapes()
    x, quat, sht, tag, lo, hi, _ = _bed(nbed, periodic)
    sp0 = _ctx(LMAX, shp, NQ)
    cut = 2.0 * max(sp0.rmax(s) for s in range(2)) + SKIN
    sp0.close()
    xw, owner = _distribute(grid, lo, hi, periodic, cut, x)
    world = int(np.prod(grid))
    hub = mrank.Hub(world) if world > 1 else None
    v, L = _motion(x.shape[0])
    return dict(shp=shp, x=x, xw=xw, quat=quat, sht=sht, tag=tag, lo=lo, hi=hi, owner=owner, world=world, hub=hub, v=v, L=L,
                grid=grid, periodic=periodic)


def _rank_run(S, sp, rank, **kw):
    from shpair import mrank
    halo = mrank.Halo(sp, rank, S["world"], S["grid"], S["lo"], S["hi"], S["periodic"], SKIN, hub=S["hub"])
    mine = S["owner"] == rank
    run = mrank.RankRun(sp, halo, S["xw"][mine], S["quat"][mine], S["sht"][mine], S["tag"][mine], v=S["v"][mine],
                        angmom=S["L"][mine], **kw)
    return halo, run


def _gather(parts, n, keys):
    tg = np.concatenate([p["tag"] for p in parts])
    o = np.argsort(tg)
    assert np.array_equal(tg[o], np.arange(n)), "atoms lost or duplicated"
    return [np.concatenate([p[k] for p in parts])[o] for k in keys]
