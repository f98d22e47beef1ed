"""The bed of tests/test_gpu_cyl_roll.py and its reference (tests/cyl_roll_ref.py), computed once per (L, n_q) and shared.

Eight cylinders through one point, so that bit 7 of the mask is used: 0 is tests/test_gpu_cylinder.py's oblique cylinder, 1
crosses it at a right angle (some particles reach both), 2..6 are wide and out of everybody's reach, 7 is cylinder 0 shifted
and a little wider (most particles at the shell of 0 reach it too).  Cylinder 1 has rolling resistance alone, cylinder 7
twisting alone, cylinder 0 both; cylinders 0 and 7 turn.  A sub-bed is the same particles against a subset of the
cylinders: the sums of a (particle, cylinder) do not depend on the other cylinders.

The bed, its motion and the coefficients were chosen on the CPU, with the reference alone, so that the condition
test_the_bed_takes_every_branch asserts on the INPUTS holds at both (L, n_q)."""
import functools

import numpy as np

import cyl_roll_ref as CR

NBED = 301            # two blocks of 256 rows, the second one ragged
KN, EXPO, DT = 1000.0, 1.25, 1e-3
CONFIGS = [(4, 10), (6, 16)]
CENTRE = np.array([0.3, -0.2, 0.5])
AXIS0 = np.array([2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0])   # a unit axis with rational components
NCYL = 8
# rolling on cylinders 0 and 1, twisting on 0 and 7: one cylinder with each kind alone; the wide ones carry coefficients too
MUR, GR = np.array([0.05, 0.04, 0.05, 0.05, 0.0, 0.0, 0.05, 0.0]), np.array([4.0, 3.0, 4.0, 4.0, 4.0, 0.0, 4.0, 4.0])
MUTW, GTW = np.array([0.03, 0.0, 0.03, 0.0, 0.03, 0.0, 0.03, 0.04]), np.array([2.5, 2.5, 2.5, 0.0, 2.5, 0.0, 2.5, 2.0])
OMEGA = np.array([0.7, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0, -0.5])
# the contact's own coefficients, per instance of the contact kernel (None: elastic)
GAMMA = np.array([60.0, 40.0, 0.0, 0.0, 0.0, 0.0, 0.0, 50.0])
MU, GT = np.array([0.4, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5]), np.array([30.0, 20.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
KT = np.array([0.0, 3e3, 0.0, 0.0, 0.0, 0.0, 0.0, 4e3])
INSTANCES = {                                 # name: (coefficients of the contact, dt or None for the force call, both ledgers)
    "elastic": (None, None, False),
    "dissipative": (dict(gamma=GAMMA, mu=MU, gt=GT), None, False),
    "spring": (dict(gamma=GAMMA, mu=MU, gt=GT, kt=KT), DT, False),
    "spring-look": (dict(gamma=GAMMA, mu=MU, gt=GT, kt=KT), 0.0, False),
    "ledger-dissipative": (dict(gamma=GAMMA, mu=MU, gt=GT), None, True),
    "ledger-spring": (dict(gamma=GAMMA, mu=MU, gt=GT, kt=KT), DT, True),
    "ledger-elastic": (None, None, True),
}


def perp(ax):
    e1 = np.cross(ax, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(ax, e1)


@functools.lru_cache(maxsize=None)
def shape(lmax):
    from shpair import shapes
    return shapes.random_shape(lmax, 21, amp=0.15)


@functools.lru_cache(maxsize=None)
def rmax(lmax):
    from shpair import capi
    return capi.shape_default_rmax(lmax, shape(lmax))


def cylinders():
    e1, e2 = perp(AXIS0)
    cyls = np.zeros((NCYL, 7))
    cyls[0] = [*CENTRE, *AXIS0, 4.0]
    cyls[1] = [*CENTRE, *e1, 4.0]
    for k in range(2, 7):
        ax = np.roll(AXIS0, k)
        cyls[k] = [*(CENTRE + 0.1 * k * e2), *ax, 30.0 + k]
    cyls[7] = [*(CENTRE + 0.12 * e1), *AXIS0, 4.1]
    return cyls


@functools.lru_cache(maxsize=None)
def bed():
    """NBED particles inside all eight cylinders: 64 at the shell of cylinder 0 (most of them in reach of 7 too, a dozen
    just within reach, where V <= 0 occurs), 24 near the two lines where the shells of 0 and 1 meet, the rest in the bulk,
    out of every reach.  Every 7th particle is outside the group, every 5th has omega = 0; |omega| and |w| spread over three
    decades, so that both branches of both caps are taken and some contacts recede fast enough to be clamped."""
    from shpair import bed as B
    rng = np.random.default_rng(23)
    e1, e2 = perp(AXIS0)
    rm = 1.3                                      # at least the bounding radius of either shape (asserted by the tests)
    u = rng.normal(size=(NBED, 3))
    x = CENTRE + u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(0.0, 2.0, NBED)[:, None]
    ring = np.arange(NBED)[(np.arange(NBED) % 3 == 1)][:88]
    for n_, i in enumerate(ring):
        h = rng.uniform(0.5, 0.85) * rm
        if n_ % 5 == 4:
            h = rng.uniform(0.93, 1.0) * rm       # just within reach
        d = 4.0 - h
        if n_ < 64:
            phi, z = rng.uniform(0, 2 * np.pi), rng.uniform(-1.2, 1.2)
        else:                                     # where the two shells meet: d sin(phi) and z put it h1 from shell 1 as well
            h1 = rng.uniform(0.5, 0.9) * rm
            z = rng.choice([-1.0, 1.0]) * rng.uniform(1.0, 2.0)
            s = np.sqrt(max(0.0, (4.0 - h1) ** 2 - z * z)) / d
            phi = np.arcsin(min(1.0, s)) * rng.choice([-1.0, 1.0]) + rng.choice([0.0, np.pi])
        x[i] = CENTRE + d * (np.cos(phi) * e1 + np.sin(phi) * e2) + z * AXIS0
    quat = B.random_quaternions(NBED, rng)
    tw = np.concatenate([rng.normal(size=(NBED, 3)) * 10.0 ** rng.uniform(-2, 1, size=(NBED, 1)),
                         rng.normal(size=(NBED, 3)) * 10.0 ** rng.uniform(-2, 1, size=(NBED, 1))], axis=1)
    tw[::5, 3:] = 0.0
    mask = np.ones(NBED, np.int32)
    mask[::7] = 2                                 # another group's bit
    return x, quat, tw, mask


@functools.lru_cache(maxsize=None)
def sums(lmax, nq):
    """The per-(particle, cylinder) sums of the bed from the reference: computed once per (L, n_q), shared by every test."""
    x, quat, _, mask = bed()
    return CR.reach_sums([(lmax, shape(lmax), rmax(lmax))], nq, x, quat, np.zeros(NBED, int), cylinders(), mask=mask)


def reference(lmax, nq, name="elastic", n=NBED, cyl_ids=None, mask=None, roll=True, **kw):
    """The reference's pass over the first n particles against the cylinders cyl_ids (all eight by default) behind the
    contact-kernel instance `name`; mask: a narrower group than the bed's."""
    x, _, tw, m0 = bed()
    ids = list(range(NCYL)) if cyl_ids is None else list(cyl_ids)
    coef, dt, _ = INSTANCES[name]
    s = {(i, ids.index(c)): v for (i, c), v in sums(lmax, nq).items() if i < n and c in ids and (mask is None or mask[i] & 1)}
    pick = lambda a: np.asarray(a, float)[ids]
    z = np.zeros(len(ids))
    args = dict(gamma=z, mu=z, gt=z, kt=z) if coef is None else {k: pick(v) for k, v in coef.items()}
    args.update(kw)
    on = 1.0 if roll else 0.0
    return CR.cyl_roll(s, n, x, tw, cylinders()[ids], KN, EXPO, on * pick(MUR), pick(GR), on * pick(MUTW), pick(GTW), omega=pick(OMEGA),
                       dt=dt or 0.0, **args)
