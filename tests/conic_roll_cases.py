"""The bed of the cone-rolling tests (docs/SPEC.md §2.24), shared by tests/test_gpu_conic_roll.py's CPU condition on the
inputs and its GPU parity tests: 40 particles in 8 cones on one oblique axis, as tests/test_gpu_conic_history.py's crowd,
with the coefficients of the three contact-kernel instances and of the two couples.  The reference is computed once per
(L, n_q) and shared.

Cones 0..6 have their apexes 0.04 apart down the axis and half-angles near 30 degrees, so that most particles reach
several of them; cone 7 is wider (60 degrees), with its apex at the origin, 3 up the axis.  Particle 39 sits at the unit
axis vector itself: exactly on the axis of cone 7 as both the reference and the kernel compute it (d = 0: foot_is_exact
shows it), within its reach and out of reach of the others.  Particle 5 is outside the group.

Kinds: cones 0, 3, 7 have both, 1 and 5 rolling only, 2 twisting only, 4 and 6 neither (4 a gamma_r without a mu_r, 6 a
mu_r without a gamma_r)."""
import functools
from fractions import Fraction

import numpy as np

import cone_ref as Co
import conic_history_cases as H
import conic_roll_ref as KR

# tests/conic_history_cases.py's axis with its middle component two units in the last place up: still a unit vector to
# 1e-16, and a.a rounds to exactly 1 in the order of numpy's dot and in that of the kernel's fused multiply-adds, so that a
# centre at the axis vector itself has rho = 0 exactly in both
AXIS = np.array([H.AXIS[0], np.nextafter(np.nextafter(H.AXIS[1], 1.0), 1.0), H.AXIS[2]])
NBED, NK, KN, EXPO, DT = 40, 8, 1000.0, 1.25, 5e-3
ON_AXIS, OUTSIDE = 39, 5
CONFIGS = [(4, 10), (6, 16)]

GAMMA = np.array([3.0, 0.0, 2.0, 3.0, 1.0, 0.0, 3.0, 2.0])
MU = np.array([0.5, 0.4, 0.05, 0.5, 0.0, 0.3, 0.02, 0.3])
GT = np.array([2.0, 3.0, 2.0, 0.0, 0.0, 300.0, 2.0, 2.0])
KT = np.array([4e3, 0.0, 3e3, 5e3, 2e3, 0.0, 4e3, 0.0])
OMEGA = np.array([1.7, 0.0, -0.8, 0.5, 0.3, 1.1, 0.0, 0.6])
MUR = np.array([0.05, 0.02, 0.0, 0.05, 0.0, 1e-3, 0.05, 0.04])
GR = np.array([3.0, 500.0, 0.0, 3.0, 2.0, 300.0, 0.0, 3.0])
MUTW = np.array([0.03, 0.0, 0.03, 1e-3, 0.0, 0.0, 0.0, 0.03])
GTW = np.array([2.0, 0.0, 2.0, 200.0, 0.0, 2.0, 0.0, 2.0])
ROLL_KIND = (MUR != 0) & (GR != 0)
TWIST_KIND = (MUTW != 0) & (GTW != 0)

# name: (coefficients of the contact law or None, dt of the pass: None for the call without a time step)
Z = np.zeros(NK)
INSTANCES = {"elastic": (None, None),
             "dissipative": (dict(gamma=GAMMA, mu=MU, gt=GT), None),
             "spring": (dict(gamma=GAMMA, mu=MU, gt=GT, kt=KT), DT),
             "spring-look": (dict(gamma=GAMMA, mu=MU, gt=GT, kt=KT), 0.0)}


@functools.lru_cache(maxsize=None)
def shape(lmax):
    from shpair import shapes
    return shapes.random_shape(lmax, 40 + lmax, amp=0.1)


@functools.lru_cache(maxsize=None)
def rmax(lmax):
    from oracle import oracle as O
    return O.shape_rmax(lmax, shape(lmax))


def cones():
    return np.stack([Co.cone(-(3.0 + 0.04 * k) * AXIS, AXIS, np.pi / 6 + 0.004 * (k % 3)) for k in range(NK - 1)] +
                    [Co.cone(np.zeros(3), AXIS, np.pi / 3)])


@functools.lru_cache(maxsize=None)
def bed(lmax):
    """x, quat, twist, mask.  The angular velocities span three decades; every eighth particle does not spin."""
    from shpair import bed as B
    rng = np.random.default_rng(31)
    co, rm = cones(), rmax(lmax)
    x = np.stack([H.centre(co[0], rng.uniform(0, 2 * np.pi), rng.uniform(6.0, 9.0), rng.uniform(0.55, 1.1) * rm) for _ in range(NBED)])
    x[ON_AXIS] = AXIS
    quat = B.random_quaternions(NBED, rng)
    tw = np.concatenate([rng.normal(size=(NBED, 3)) * 0.4, rng.normal(size=(NBED, 3)) * 10.0 ** rng.uniform(-2, 1, (NBED, 1))], axis=1)
    tw[::8, 3:] = 0.0
    tw[ON_AXIS, 3:] = [0.7, -0.4, 1.1]
    mask = np.ones(NBED, np.int32)
    mask[OUTSIDE] = 2
    return x, quat, tw, mask


def foot_is_exact():
    """d of particle 39 against cone 7 as the reference computes it, and as cone_foot of csrc/cone_kernels.hpp does (its
    fused multiply-adds in exact rational arithmetic, rounded once each)."""
    x, C = AXIS, cones()[7]
    fma = lambda a, b, c: float(Fraction(a) * Fraction(b) + Fraction(c))
    y = [float(x[j] - C[j]) for j in range(3)]
    t = fma(y[0], C[3], fma(y[1], C[4], y[2] * C[5]))
    r = [fma(-t, C[3 + j], y[j]) for j in range(3)]
    d_dev = float(np.sqrt(fma(r[0], r[0], fma(r[1], r[1], r[2] * r[2]))))
    return Co.foot(x, C)[2], d_dev


@functools.lru_cache(maxsize=None)
def sums(lmax, nq):
    x, quat, _, mask = bed(lmax)
    return KR.reach_sums([(lmax, shape(lmax), rmax(lmax))], nq, x, quat, np.zeros(NBED, int), cones(), mask=mask)


@functools.lru_cache(maxsize=None)
def reference(lmax, nq, name="elastic", roll=True):
    x, _, tw, _ = bed(lmax)
    coef, dt = INSTANCES[name]
    c = {**dict(gamma=Z, mu=Z, gt=Z, kt=Z), **(coef or {})}
    on = (MUR, GR, MUTW, GTW) if roll else (0.0, 0.0, 0.0, 0.0)
    return KR.conic_roll(sums(lmax, nq), NBED, x, tw, cones(), KN, EXPO, *on, gamma=c["gamma"], mu=c["mu"], gt=c["gt"], omega=OMEGA,
                         kt=c["kt"], dt=dt or 0.0)
