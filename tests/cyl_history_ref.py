"""numpy restatement of docs/SPEC.md §2.19 (tangential contact springs with history at the cylinders of §2.18): the
yardstick of the cylinder-history tests.

The per-contact sums and the contact point come from tests/cyl_ref.py (cyl_sums, contact_point, foot), and a cylinder
without a spring keeps that file's law (contact_wrench); what §2.19 adds is written out here, in the space frame:
(xi_a, xi_theta) and the live bit per (particle, cylinder), the reset, the advance in the cylinder's own surface
coordinates, the trial force and its cap.  Shares no code with the kernels (cyl_spring_kernel and the sweep of
csrc/cylinder_kernels.hpp) and mirrors tests/wall_history_ref.py.
"""
import numpy as np

import cyl_ref as Cy

STICK, SLIDE, RESET, NONE = "stick", "slide", "reset", "none"


def surface_frame(ax, rho_c, Rc):
    """(a^, t^_c) at a contact point: the axis, and t^_c = a^ x rho_c / Rc, the direction the wall moves for Omega > 0."""
    ax = np.asarray(ax, float)
    return ax, np.cross(ax, rho_c) / Rc


def spring_law(xi, vt, ea, et, N, mu, gt, kt, dt):
    """(F_t, new (xi_a, xi_theta), kind, |F*| / (mu N)) of one contact of a history cylinder: advance, trial, cap."""
    xa, xt = xi[0] + dt * (vt @ ea), xi[1] + dt * (vt @ et)
    Fs = -kt * (xa * ea + xt * et) - gt * vt
    fn = np.linalg.norm(Fs)
    if fn <= mu * N:
        return Fs, np.array([xa, xt]), STICK, fn / (mu * N)
    Ft = Fs * (mu * N / fn)
    h = -(Ft + gt * vt) / kt
    return Ft, np.array([h @ ea, h @ et]), SLIDE, fn / (mu * N)


def contact_history(V, S, T, x, cyl, kn, m, tw, gamma, mu, gt, omega, kt, xi, dt):
    """(F_i, tau_i, E, details) of one contact with V > 0 of a history cylinder (mu != 0, kt != 0) on given sums; xi is
    the live (xi_a, xi_theta) going in, or zeros.  details is None where a guard resets the contact (|S_n| = 0, N = 0,
    A = 0, D < 0), else a dict Ft, ri, rc, vt, N, xi (coming out), kind, ratio = |F*| / (mu N), ea, et."""
    a, ax, Rc = np.asarray(cyl[:3], float), np.asarray(cyl[3:6], float), float(cyl[6])
    p = kn * m * V ** (m - 1)
    pt = max(0.0, p + gamma * (S @ tw[:3] + T @ tw[3:]))
    Fi, tau, E = -pt * S, -pt * T, kn * V ** m
    N = pt * np.linalg.norm(S)
    cp = Cy.contact_point(S, T, Cy.foot(x, cyl)[0], ax, Rc) if (S @ S > 0 and N > 0) else None
    if cp is None:
        return Fi, tau, E, None
    ri, rc = cp
    nrm = -rc / Rc
    vrel = tw[:3] + np.cross(tw[3:], ri) - omega * np.cross(ax, rc)
    vt = vrel - (vrel @ nrm) * nrm
    ea, et = surface_frame(ax, rc, Rc)
    Ft, xi1, kind, ratio = spring_law(np.asarray(xi, float), vt, ea, et, N, mu, gt, kt, dt)
    return Fi + Ft, tau + np.cross(ri, Ft), E, dict(Ft=Ft, ri=ri, rc=rc, vt=vt, N=N, xi=xi1, kind=kind, ratio=ratio, ea=ea, et=et)


def cyl_forces_history(shapes, nq, x, quat, shtype, tw, cyls, kn, expo, gamma, mu, gt, omega, kt, xi, live, dt, mask=None,
                       groupbit=1):
    """One cylinder pass of §2.18 + §2.19 with the time step dt >= 0.  xi [n][nc][2] and live [n][nc] (bool) are the state
    going in; a xi that is not live counts as 0.  Returns f, torque [n][3], cyl_out [nc][5] (E_c, the force ON the wall,
    M_ax), the state coming out (xi, live: the state going in, untouched, for dt = 0: a look), kind [n][nc] (stick, slide,
    reset for a history cylinder — reset also where the cylinder is out of reach —, none for a cylinder without
    history), ncontacts, and per contact of a history cylinder that passed every guard
    (i, c, F_t[3], r_i[3], rho_c[3], v_t[3], N, kind, |F*| / (mu N))."""
    n, nc = len(x), len(cyls)
    kn, expo, gamma, mu, gt, omega, kt = (np.broadcast_to(np.asarray(v, float), (nc,)) for v in (kn, expo, gamma, mu, gt, omega, kt))
    xi, live = np.asarray(xi, float).reshape(n, nc, 2), np.asarray(live, bool).reshape(n, nc)
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nc, 5))
    xi1, live1 = np.zeros((n, nc, 2)), np.zeros((n, nc), bool)
    kind = np.full((n, nc), NONE, dtype=object)
    det, ncon = [], 0
    for i in range(n):
        lmax, anm, rmax = shapes[int(shtype[i])]
        grouped = mask is None or bool(int(mask[i]) & groupbit)
        for c in range(nc):
            hist = mu[c] != 0 and kt[c] != 0
            if hist:
                kind[i, c] = RESET                      # until the contact passes every guard
            if not grouped:
                continue
            V, S, T, st = Cy.cyl_sums(lmax, anm, rmax, x[i], quat[i], cyls[c], nq)
            if st <= 0 or not V > 0:
                continue
            a, ax, Rc = np.asarray(cyls[c][:3], float), np.asarray(cyls[c][3:6], float), float(cyls[c][6])
            if not hist:
                Fi, tau, E, _ = Cy.contact_wrench(V, S, T, x[i], cyls[c], kn[c], expo[c], tw[i], gamma[c], mu[c], gt[c], omega[c])
            else:
                Fi, tau, E, d = contact_history(V, S, T, x[i], cyls[c], kn[c], expo[c], tw[i], gamma[c], mu[c], gt[c], omega[c],
                                                kt[c], xi[i, c] if live[i, c] else np.zeros(2), dt)
                if d is not None:
                    xi1[i, c], kind[i, c], live1[i, c] = d["xi"], d["kind"], True
                    det.append((i, c, d["Ft"], d["ri"], d["rc"], d["vt"], d["N"], d["kind"], d["ratio"]))
            f[i] += Fi
            tq[i] += tau
            out[c, 0] += E
            out[c, 1:4] -= Fi
            out[c, 4] += ax @ (np.cross(x[i] - a, -Fi) - tau)
            ncon += 1
    if dt == 0:
        xi1, live1 = xi.copy(), live.copy()
    else:
        xi1[~live1] = 0.0
    return dict(f=f, torque=tq, cyl_out=out, xi=xi1, live=live1, kind=kind, ncontacts=ncon, contacts=det)
