"""numpy restatement of docs/SPEC.md §2.12 (planar walls that translate at a constant velocity): the yardstick of the
moving-wall tests.

The per-contact sums come from tests/wall_ref.py (wall_sums), the capped friction law and the contact point from
tests/friction_ref.py (capped, wall_contact_point); what §2.12 adds is written out here: u_w leaves the linear part of the
particle's twist before Vdot and v_rel are formed, and the plane position is the per-step accumulation c += dt (n.u).
Shares no code with the kernels (the MOVE instances and the advance kernel of csrc/wall_kernels.hpp).
"""
import numpy as np

import friction_ref as F
import wall_ref as W


def wall_forces_moving(shapes, nq, x, quat, shtype, tw, planes, kn, expo, gamma, mu, gt, vel):
    """The wall pass of §2.10 + §2.11 against walls moving at vel [nw][3]: f, torque [n][3], wall_out [nw][4] (E_w = kn V^m,
    force ON the wall), per-contact details (i, w, p, p_tot, N, F_t[3], r_i[3], capped) — the layout of
    friction_ref.wall_forces_friction, which this is for vel = 0."""
    n, nw = len(x), len(planes)
    vel = np.asarray(vel, float).reshape(nw, 3)
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nw, 4))
    det = []
    for i in range(n):
        lmax, anm, rmax = shapes[int(shtype[i])]
        for w in range(nw):
            V, S, T, st = W.wall_sums(lmax, anm, rmax, x[i], quat[i], planes[w], nq)
            if st <= 0 or not V > 0:
                continue
            nrm = np.asarray(planes[w][:3], float)
            wl = tw[i, :3] - vel[w]                    # the SH origin's velocity relative to the wall
            p = kn[w] * expo[w] * V ** (expo[w] - 1)
            pt = max(0.0, p + gamma[w] * (S @ wl + T @ tw[i, 3:]))
            Fi, tau = -pt * S, -pt * T
            N = pt * np.linalg.norm(S)
            Ft, ri, cp = np.zeros(3), np.full(3, np.nan), False
            if mu[w] != 0 and gt[w] != 0 and S @ S > 0:
                ri = F.wall_contact_point(S, T, nrm, nrm @ x[i] - planes[w][3])
                vrel = wl + np.cross(tw[i, 3:], ri)
                vt = vrel - (vrel @ nrm) * nrm
                Ft, _, cp = F.capped(vt, N, mu[w], gt[w])
                Fi, tau = Fi + Ft, tau + np.cross(ri, Ft)
            det.append((i, w, p, pt, N, Ft, ri, cp))
            f[i] += Fi
            tq[i] += tau
            out[w, 0] += kn[w] * V ** expo[w]
            out[w, 1:] -= Fi
    return dict(f=f, torque=tq, wall_out=out, contacts=det)


def normal_speed(planes, vel):
    """n_w.u_w, formed once (as the library forms it when the velocity is set)."""
    pl, u = np.asarray(planes, float), np.asarray(vel, float)
    u = np.broadcast_to(u, (len(pl), 3))
    return pl[:, 0] * u[:, 0] + pl[:, 1] * u[:, 1] + pl[:, 2] * u[:, 2]


def advance(planes, vel, dt, k):
    """The planes after k advances by dt: c += dt (n.u), one product and one sum per step, each rounded — the plane
    position is DEFINED as this accumulation, not as c_0 + k dt (n.u)."""
    pl = np.array(planes, dtype=np.float64)
    step = np.float64(dt) * normal_speed(pl, vel)
    for _ in range(int(k)):
        pl[:, 3] = pl[:, 3] + step
    return pl
