"""numpy restatement of docs/SPEC.md §2.15 (tangential contact springs with history at planar walls): the yardstick of
the wall-history tests.

The per-contact sums come from tests/wall_ref.py (wall_sums), the contact point and the history-free law of the walls
without a spring from tests/friction_ref.py (wall_contact_point, capped), the wall-relative twist is that of
tests/wall_move_ref.py; what §2.15 adds is written out here: xi_iw and its live bit per (particle, wall), the reset, the
advance and the projection with the exact wall normal, the trial force and its cap.  Shares no code with the kernels (the
HIST instances and the sweep of csrc/wall_kernels.hpp).
"""
import numpy as np

import friction_ref as F
import wall_ref as W

STICK, SLIDE, RESET, NONE = "stick", "slide", "reset", "none"


def spring_law(xi, vt, nrm, N, mu, gt, kt, dt):
    """(F_t, new xi, kind) of one live contact of a history wall: advance, project, trial, cap."""
    xp = xi + dt * vt
    xp = xp - (xp @ nrm) * nrm
    Fs = -kt * xp - gt * vt
    fn = np.linalg.norm(Fs)
    if fn <= mu * N:
        return Fs, xp, STICK
    Ft = Fs * (mu * N / fn)
    return Ft, -(Ft + gt * vt) / kt, SLIDE


def wall_forces_history(shapes, nq, x, quat, shtype, tw, planes, kn, expo, gamma, mu, gt, kt, vel, xi, live, dt):
    """One wall pass of §2.10-§2.12 + §2.15 with the time step dt >= 0.  xi [n][nw][3] and live [n][nw] (bool) are the
    state going in; a xi that is not live counts as 0.  Returns f, torque [n][3], wall_out [nw][4] (E_w = kn V^m, force
    ON the wall), the state coming out (xi, live: the state going in, untouched, for dt = 0: a look), kind [n][nw] (stick,
    slide, reset for a history wall — reset also where the wall is out of reach —, none for a wall without history),
    and per-contact details in the layout of wall_move_ref.wall_forces_moving with the kind appended and `capped` true for
    a sliding contact: (i, w, p, p_tot, N, F_t[3], r_i[3], capped, kind, v_t[3])."""
    n, nw = len(x), len(planes)
    vel = np.asarray(vel, float).reshape(nw, 3)
    xi, live = np.asarray(xi, float).reshape(n, nw, 3), np.asarray(live, bool).reshape(n, nw)
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nw, 4))
    xi1, live1 = np.zeros((n, nw, 3)), np.zeros((n, nw), bool)
    kind = np.full((n, nw), NONE, dtype=object)
    det = []
    for i in range(n):
        lmax, anm, rmax = shapes[int(shtype[i])]
        for w in range(nw):
            hist = mu[w] != 0 and kt[w] != 0
            if hist:
                kind[i, w] = RESET                      # until the contact passes every guard
            V, S, T, st = W.wall_sums(lmax, anm, rmax, x[i], quat[i], planes[w], nq)
            if st <= 0 or not V > 0:
                continue
            nrm = np.asarray(planes[w][:3], float)
            wl = tw[i, :3] - vel[w]                    # the SH origin's velocity relative to the wall
            p = kn[w] * expo[w] * V ** (expo[w] - 1)
            pt = max(0.0, p + gamma[w] * (S @ wl + T @ tw[i, 3:]))
            Fi, tau = -pt * S, -pt * T
            N = pt * np.linalg.norm(S)
            Ft, ri, vt, cp = np.zeros(3), np.full(3, np.nan), np.full(3, np.nan), False
            if hist:
                if S @ S > 0 and N > 0:
                    ri = F.wall_contact_point(S, T, nrm, nrm @ x[i] - planes[w][3])
                    vrel = wl + np.cross(tw[i, 3:], ri)
                    vt = vrel - (vrel @ nrm) * nrm
                    Ft, xi1[i, w], kind[i, w] = spring_law(xi[i, w] if live[i, w] else np.zeros(3), vt, nrm, N, mu[w], gt[w],
                                                           kt[w], dt)
                    live1[i, w], cp = True, kind[i, w] == SLIDE
                    Fi, tau = Fi + Ft, tau + np.cross(ri, Ft)
            elif mu[w] != 0 and gt[w] != 0 and S @ S > 0:
                ri = F.wall_contact_point(S, T, nrm, nrm @ x[i] - planes[w][3])
                vrel = wl + np.cross(tw[i, 3:], ri)
                vt = vrel - (vrel @ nrm) * nrm
                Ft, _, cp = F.capped(vt, N, mu[w], gt[w])
                Fi, tau = Fi + Ft, tau + np.cross(ri, Ft)
            det.append((i, w, p, pt, N, Ft, ri, cp, kind[i, w], vt))
            f[i] += Fi
            tq[i] += tau
            out[w, 0] += kn[w] * V ** expo[w]
            out[w, 1:] -= Fi
    if dt == 0:
        xi1, live1 = xi.copy(), live.copy()
    else:
        xi1[~live1] = 0.0
    return dict(f=f, torque=tq, wall_out=out, xi=xi1, live=live1, kind=kind, contacts=det)
