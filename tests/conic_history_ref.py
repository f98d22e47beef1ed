"""numpy restatement of docs/SPEC.md §2.23 (tangential contact springs with history at the cones of §2.22): the
yardstick of the cone-history tests.

The per-contact sums, the contact point and the law of a cone without a spring come from tests/cone_ref.py (cone_sums,
contact_point, contact_wrench, foot); what §2.23 adds is written out here, in the space frame: (xi_g, xi_theta, phi_c)
and the live bit per (particle, cone), the reset, the transport of the two components through the change of azimuth
against the wall's material, the advance, the trial force and its cap.  Shares no code with the kernels
(conic_spring_kernel and the sweep of csrc/cone_kernels.hpp) and mirrors tests/cyl_history_ref.py.

`law` selects the transport: EXACT is §2.23's; the others are the wrong laws the tests must be able to tell from it.
"""
import numpy as np

import cone_ref as Co

STICK, SLIDE, RESET, NONE = "stick", "slide", "reset", "none"
EXACT, NO_TRANSPORT, FULL_ANGLE, OPPOSITE, NO_OMEGA = "exact", "no transport", "dphi for sin(theta) dphi", "opposite sign", "ignores Omega dt"
WRONG_LAWS = (NO_TRANSPORT, FULL_ANGLE, OPPOSITE, NO_OMEGA)


def axis_frame(ax):
    """(e1, e2) normal to the axis: e1 is the vector the frame rule of §2.3 gives about a^ (the one §2.22 uses for c^ on
    the axis), e2 = a^ x e1."""
    ax = np.asarray(ax, float)
    s = np.copysign(1.0, ax[2])
    k = -1.0 / (s + ax[2])
    e1 = np.array([1 + s * ax[0] ** 2 * k, s * ax[0] * ax[1] * k, -s * ax[0]])
    return e1, np.cross(ax, e1)


def azimuth(co, rho_c):
    """phi_c = atan2(rho_c.e2, rho_c.e1)."""
    e1, e2 = axis_frame(co[3:6])
    return float(np.arctan2(rho_c @ e2, rho_c @ e1))


def surface_frame(co, rho_c):
    """(g^_c, t^_c) at a contact point: the generator away from the apex, s c^_c + c a^, and t^_c = a^ x c^_c, the direction
    the wall moves for Omega > 0; g^_c x t^_c is the inward normal n^_c = s a^ - c c^_c."""
    ax, ct, st = np.asarray(co[3:6], float), float(co[6]), float(co[7])
    ch = rho_c / np.sqrt(rho_c @ rho_c)
    return st * ch + ct * ax, np.cross(ax, ch)


def wrap(d):
    """d into (-pi, pi]."""
    if d > np.pi:
        return d - 2 * np.pi
    if d <= -np.pi:
        return d + 2 * np.pi
    return d


def transport_angle(dphi, st, omega, dt, law=EXACT):
    """Delta beta = sin theta (Delta phi - Omega dt): the polar angle of the developed cone is beta = sin theta phi, and the
    wall's material turns by Omega dt."""
    if law == EXACT:
        return st * (dphi - omega * dt)
    if law == NO_TRANSPORT:
        return 0.0
    if law == FULL_ANGLE:
        return dphi - omega * dt
    if law == OPPOSITE:
        return -st * (dphi - omega * dt)
    if law == NO_OMEGA:
        return st * dphi
    raise ValueError(law)


def transported(state, phi1, st, omega, dt, law=EXACT):
    """(xi_g, xi_theta) of a live state (xi_g, xi_theta, phi_c) carried to the azimuth phi1."""
    db = transport_angle(wrap(phi1 - state[2]), st, omega, dt, law)
    c, s = np.cos(db), np.sin(db)
    return np.array([state[0] * c + state[1] * s, -state[0] * s + state[1] * c])


def spring_law(xi, vt, eg, et, N, mu, gt, kt, dt):
    """(F_t, new (xi_g, xi_theta), kind, |F*| / (mu N)) of one contact of a history cone on the transported xi: advance,
    trial, cap."""
    xg, xt = xi[0] + dt * (vt @ eg), xi[1] + dt * (vt @ et)
    Fs = -kt * (xg * eg + xt * et) - gt * vt
    fn = np.linalg.norm(Fs)
    if fn <= mu * N:
        return Fs, np.array([xg, xt]), STICK, fn / (mu * N)
    Ft = Fs * (mu * N / fn)
    h = -(Ft + gt * vt) / kt
    return Ft, np.array([h @ eg, h @ et]), SLIDE, fn / (mu * N)


def contact_history(V, S, T, x, co, kn, m, tw, gamma, mu, gt, omega, kt, state, live, dt, law=EXACT):
    """(F_i, tau_i, E, details) of one contact with V > 0 of a history cone (mu != 0, kt != 0) on given sums; state is
    (xi_g, xi_theta, phi_c) going in and counts only where `live`.  details is None where a guard resets the contact
    (|S_n| = 0, N = 0, D < 0, S^ never leaves, t_c <= 0, rho_c = 0), else a dict Ft, ri, rc, vt, N, state (coming out),
    kind, ratio = |F*| / (mu N), eg, et."""
    ax, ct, st = np.asarray(co[3:6], float), float(co[6]), float(co[7])
    p = kn * m * V ** (m - 1)
    pt = max(0.0, p + gamma * (S @ tw[:3] + T @ tw[3:]))
    Fi, tau, E = -pt * S, -pt * T, kn * V ** m
    N = pt * np.linalg.norm(S)
    cp = None
    if S @ S > 0 and N > 0:
        t, rho = Co.foot(x, co)[:2]
        cp = Co.contact_point(S, T, t, rho, co)
    if cp is None:
        return Fi, tau, E, None
    ri, rc, tc = cp
    nrm = st * ax - ct * rc / np.sqrt(rc @ rc)
    vrel = tw[:3] + np.cross(tw[3:], ri) - omega * np.cross(ax, rc)
    vt = vrel - (vrel @ nrm) * nrm
    eg, et = surface_frame(co, rc)
    phi = azimuth(co, rc)
    xi = transported(state, phi, st, omega, dt, law) if live else np.zeros(2)
    Ft, xi1, kind, ratio = spring_law(xi, vt, eg, et, N, mu, gt, kt, dt)
    return Fi + Ft, tau + np.cross(ri, Ft), E, dict(Ft=Ft, ri=ri, rc=rc, vt=vt, N=N, state=np.array([xi1[0], xi1[1], phi]), kind=kind,
                                                    ratio=ratio, eg=eg, et=et)


def cone_forces_history(shapes, nq, x, quat, shtype, tw, cones, kn, expo, gamma, mu, gt, omega, kt, xi, live, dt, mask=None,
                        groupbit=1, law=EXACT):
    """One cone pass of §2.22 + §2.23 with the time step dt >= 0.  xi [n][nk][3] = (xi_g, xi_theta, phi_c) and live [n][nk]
    (bool) are the state going in; a row that is not live counts as 0.  Returns f, torque [n][3], cone_out [nk][5] (E_k,
    the force ON the wall, M_ax), the state coming out (xi, live: the state going in, untouched, for dt = 0: a look), kind
    [n][nk] (stick, slide, reset for a history cone — reset also where the cone is out of reach —, none for a cone
    without history), ncontacts, and per contact of a history cone that passed every guard
    (i, c, F_t[3], r_i[3], rho_c[3], v_t[3], N, kind, |F*| / (mu N))."""
    n, nk = len(x), len(cones)
    kn, expo, gamma, mu, gt, omega, kt = (np.broadcast_to(np.asarray(v, float), (nk,)) for v in (kn, expo, gamma, mu, gt, omega, kt))
    xi, live = np.asarray(xi, float).reshape(n, nk, 3), np.asarray(live, bool).reshape(n, nk)
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nk, 5))
    xi1, live1 = np.zeros((n, nk, 3)), np.zeros((n, nk), bool)
    kind = np.full((n, nk), NONE, dtype=object)
    det, ncon = [], 0
    for i in range(n):
        lmax, anm, rmax = shapes[int(shtype[i])]
        grouped = mask is None or bool(int(mask[i]) & groupbit)
        for c in range(nk):
            hist = mu[c] != 0 and kt[c] != 0
            if hist:
                kind[i, c] = RESET                      # until the contact passes every guard
            if not grouped:
                continue
            V, S, T, st = Co.cone_sums(lmax, anm, rmax, x[i], quat[i], cones[c], nq)
            if st <= 0 or not V > 0:
                continue
            a, ax = np.asarray(cones[c][:3], float), np.asarray(cones[c][3:6], float)
            if not hist:
                Fi, tau, E, _ = Co.contact_wrench(V, S, T, x[i], cones[c], kn[c], expo[c], tw[i], gamma[c], mu[c], gt[c], omega[c])
            else:
                Fi, tau, E, d = contact_history(V, S, T, x[i], cones[c], kn[c], expo[c], tw[i], gamma[c], mu[c], gt[c], omega[c],
                                                kt[c], xi[i, c], live[i, c], dt, law)
                if d is not None:
                    xi1[i, c], kind[i, c], live1[i, c] = d["state"], d["kind"], True
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
    return dict(f=f, torque=tq, cone_out=out, xi=xi1, live=live1, kind=kind, ncontacts=ncon, contacts=det)
