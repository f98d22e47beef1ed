"""The prescribed motions of tests/test_gpu_cyl_history.py and their reference trajectories (tests/cyl_history_ref.py),
computed once per case and shared: x, quat and the twists of every pass are given, not integrated, so the device and the
reference see the same inputs and differ only in how they carry (xi_a, xi_theta).

Every case is built so that the reference alone shows at least one sticking, one sliding and one reset contact, and no
contact whose |F*| / (mu N) lies within 1e-6 of 1: no branch can flip inside the 1e-9 gate (check_conditions)."""
import functools

import numpy as np

import cyl_history_ref as CH

OBLIQUE = np.array([0.3, -0.2, 0.5, 2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0, 4.0])   # a, a unit axis with rational components, Rc
NPASS, DT = 4, 2e-3
KN, EXPO, GAMMA = 1000.0, 1.25, 3.0


def _perp(ax):
    e1 = np.cross(ax, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(ax, e1)


def _ring(rng, n, rmax, cyl, lo, hi):
    """n centres inside cylinder `cyl` with depth margins h = Rc - d uniform in [lo, hi] rmax."""
    a, ax, Rc = cyl[:3], cyl[3:6], cyl[6]
    e1, e2 = _perp(ax)
    d = Rc - rng.uniform(lo, hi, n) * rmax
    phi, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(-3, 3, n)
    return a + d[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2) + z[:, None] * ax


def geometry(name, rmax):
    """(cyls [nc][7], mu, gamma_t, k_t, Omega per cylinder, a function rng -> x [n][3]) of a named geometry."""
    if name == "oblique":      # one cylinder, an oblique axis, a rotating wall
        return np.array([OBLIQUE]), [0.5], [2.0], [4e3], [0.7], lambda rng: _ring(rng, 14, rmax, OBLIQUE, 0.5, 0.95)
    if name == "two":          # two cylinders in reach of most particles; the second has no k_t and keeps §2.18's friction
        e1, _ = _perp(OBLIQUE[3:6])
        second = np.array([*(OBLIQUE[:3] + 0.12 * e1), *OBLIQUE[3:6], 4.1])
        return (np.array([OBLIQUE, second]), [0.5, 0.4], [0.0, 30.0], [4e3, 0.0], [0.0, 0.5],
                lambda rng: _ring(rng, 14, rmax, OBLIQUE, 0.5, 0.85))
    if name == "axis":         # a narrow cylinder (Rmax > Rc): a centre exactly on the axis, the others just off it
        cyl = np.array([0.5, -0.25, 0.0, 0.0, 0.0, 1.0, 0.9 * rmax])
        def place(rng):
            x = _ring(rng, 8, rmax, cyl, 0.45, 0.85)
            x[0] = [0.5, -0.25, 2.5]
            return x
        return np.array([cyl]), [0.5], [2.0], [4e3], [0.4], place
    raise KeyError(name)


# the seeds for which check_conditions holds (seed 0 of (4, 1, "axis") has no sliding contact)
SEEDS = {(4, 1, "axis"): 4}


@functools.lru_cache(maxsize=None)
def case(lmax, nq, name, seed=None):
    """The inputs of NPASS consecutive advancing passes and the reference's trajectory through them."""
    from oracle import oracle as O
    from shpair import bed, shapes
    anm = shapes.random_shape(lmax, 40 + lmax, amp=0.1)
    rmax = O.shape_rmax(lmax, anm)
    cyls, mu, gt, kt, om, place = geometry(name, rmax)
    seed = SEEDS.get((lmax, nq, name), 0) if seed is None else seed
    rng = np.random.default_rng(1000 * lmax + 10 * nq + len(name) + seed)
    x0 = place(rng)
    n = len(x0)
    quat = bed.random_quaternions(n, rng)
    # twists over five decades, so that both branches of the cap are taken, most contacts well away from it
    scale = 10.0 ** rng.uniform(-2.5, 2.5, n)
    xs, tws, masks = [], [], []
    for k in range(NPASS):
        tw = rng.normal(size=(n, 6)) * scale[:, None]
        x = x0 + DT * k * 0.05 * rng.normal(size=(n, 3))
        if k == 2:             # the last particle leaves the reach of every cylinder for one pass and comes back
            a, ax = cyls[0][:3], cyls[0][3:6]
            y = x[-1] - a
            x[-1] = a + (y @ ax) * ax + 0.02 * (y - (y @ ax) * ax)
        mask = np.ones(n, np.int32)
        if k == 2 and name == "axis":   # nothing inside a narrow cylinder is out of its reach: the particle leaves the group instead
            x[-1] = x0[-1]
            mask[-1] = 2
        xs.append(x)
        masks.append(mask)
        tws.append(tw)
    shp = [(lmax, anm, rmax)]
    sht = np.zeros(n, np.int32)
    xi, live = np.zeros((n, len(cyls), 2)), np.zeros((n, len(cyls)), bool)
    refs = []
    for k in range(NPASS):
        r = CH.cyl_forces_history(shp, nq, xs[k], quat, sht, tws[k], cyls, [KN] * len(cyls), [EXPO] * len(cyls), GAMMA, mu, gt, om,
                                  kt, xi, live, DT, mask=masks[k])
        xi, live = r["xi"], r["live"]
        refs.append(r)
    return dict(lmax=lmax, nq=nq, anm=anm, rmax=rmax, cyls=cyls, mu=mu, gt=gt, kt=kt, om=om, n=n, quat=quat, shtype=sht, xs=xs,
                tws=tws, masks=masks, refs=refs)


def check_conditions(c):
    """Read from the reference alone: every kind occurs, no contact sits on the cap, and the state is not trivial."""
    kinds = [k for r in c["refs"] for k in r["kind"].ravel()]
    ratios = np.array([d[8] for r in c["refs"] for d in r["contacts"]])
    counts = {k: kinds.count(k) for k in (CH.STICK, CH.SLIDE, CH.RESET, CH.NONE)}
    margin = np.abs(ratios - 1).min()
    print("kinds %s, closest |F*|/(mu N) to 1: %.2e, max|xi| %.3e" % (counts, margin, np.abs(c["refs"][-1]["xi"]).max()))
    assert counts[CH.STICK] > 0 and counts[CH.SLIDE] > 0 and counts[CH.RESET] > 0
    assert margin > 1e-6
    assert np.abs(c["refs"][-1]["xi"]).max() > 0
    return counts
