"""Prescribed motions for the cone-history tests (docs/SPEC.md §2.23), shared by tests/test_conic_history_ref.py and
tests/test_gpu_conic_history.py: the placement of a centre by its azimuth about the axis, rigid rotations about an axis,
and a driver that carries the state of one particle against one surface through a sequence of passes of a reference."""
import numpy as np

import cone_ref as Co
import conic_history_ref as CH
from wall_ref import quat_to_mat

AXIS = np.array([2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0])   # a unit axis with rational components
APEX = np.array([0.4, -0.3, 0.2])


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def turn(ax, ang):
    """(quaternion, matrix) of the rotation by ang about the unit vector ax."""
    g = np.array([np.cos(ang / 2), *(np.sin(ang / 2) * np.asarray(ax, float))])
    return g, quat_to_mat(g)


def radial(ax, phi):
    """The unit vector normal to the axis at azimuth phi of the frame CH.axis_frame gives."""
    e1, e2 = CH.axis_frame(ax)
    return np.cos(phi) * e1 + np.sin(phi) * e2


def centre(co, phi, s, h):
    """The centre at distance h from the wall of cone co whose foot point lies at slant distance s from the apex, at
    azimuth phi."""
    ct, st = co[6], co[7]
    t, d = ct * s + st * h, st * s - ct * h
    assert d > 0
    return co[:3] + t * co[3:6] + d * radial(co[3:6], phi)


def motion(co, phis, ss, hs):
    return np.stack([centre(co, p, s, h) for p, s, h in zip(phis, ss, hs)])


def follow(shape, nq, co, xs, quats, tws, coef, dt, law=CH.EXACT, state=None, live=False):
    """One particle against one cone through len(xs) advancing passes of conic_history_ref; coef = dict(kn, m, gamma, mu, gt,
    omega, kt).  Returns the list of pass results, each with the state (xi_g, xi_theta, phi_c) coming out."""
    xi = np.zeros((1, 1, 3)) if state is None else np.asarray(state, float).reshape(1, 1, 3)
    lv = np.array([[bool(live)]])
    out = []
    for x, q, tw in zip(xs, quats, tws):
        r = CH.cone_forces_history([shape], nq, x[None], np.asarray(q)[None], [0], np.asarray(tw)[None], [co], coef["kn"], coef["m"],
                                   coef["gamma"], coef["mu"], coef["gt"], coef["omega"], coef["kt"], xi, lv, dt, law=law)
        xi, lv = r["xi"], r["live"]
        out.append(r)
    return out


def tangential_force(r):
    """F_t of the one contact of a pass result (zeros where the contact was reset)."""
    return r["contacts"][0][2] if r["contacts"] else np.zeros(3)


def spring_vector(r, co):
    """xi_g g^_c + xi_theta t^_c of the one contact of a pass result, in the space frame."""
    (_, _, Ft, ri, rc, vt, N, kind, ratio), = r["contacts"]
    eg, et = CH.surface_frame(co, rc)
    return r["xi"][0, 0, 0] * eg + r["xi"][0, 0, 1] * et
