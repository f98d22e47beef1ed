"""numpy restatement of docs/SPEC.md §2.22 (contact of an SH particle with the inside of a one-nappe circular cone that
may rotate about its axis): the yardstick of the cone tests.

r_i and its gradient come from the CPU oracle's sh_eval, the Gauss-Legendre nodes from the oracle; the foot point, the
cap, the frame, the nodes, the exit root, the sums, the force law, damping and friction are written out here, in the
space frame, the per-node loop taken literally.  Shares no code with the kernels (csrc/cone_kernels.hpp).

A cone is 8 doubles: the apex a, the unit axis a^ from the apex into the opening, cos theta, sin theta of the half-angle.
"""
import numpy as np

from oracle import oracle as O
from wall_ref import quat_to_mat

ALMOST_ONE = np.nextafter(1.0, 0.0)


def cone(apex, axis, theta):
    """The record of a cone from its half-angle."""
    return np.array([*np.asarray(apex, float), *np.asarray(axis, float), np.cos(theta), np.sin(theta)])


def foot(x, co):
    """(t, rho, d, c^, h): the axial coordinate of x - a, its part normal to the axis, that part's length, the radial
    direction rho / d (on the axis, d = 0 as computed, the e1 of the frame rule of §2.3 about the axis) and the centre's
    distance to the wall, h = sin theta t - cos theta d."""
    a, ax, ct, st = np.asarray(co[:3], float), np.asarray(co[3:6], float), float(co[6]), float(co[7])
    y = np.asarray(x, float) - a
    t = y @ ax
    rho = y - t * ax
    d = np.sqrt(rho @ rho)
    h = st * t - ct * d
    if d > 0:
        return t, rho, d, rho / d, h
    s = np.copysign(1.0, ax[2])
    k = -1.0 / (s + ax[2])
    return t, rho, d, np.array([1 + s * ax[0] ** 2 * k, s * ax[0] * ax[1] * k, -s * ax[0]]), h


def cap_cos(co, t, d, R):
    """cos alpha about n^, the inscribed sphere's bound: with h = s t - c d and P = (s d + c t) s / c, the radius of the
    sphere about the axis that touches the cone along the circle through the foot point, (h (2 P - h) - R^2) / (2 (P - h) R)
    clamped to [-1, 1), formed without dividing where it is clamped; the whole sphere within R of the apex and on the
    axis (d = 0 as computed, where P = h)."""
    ct, st = float(co[6]), float(co[7])
    if d * d + t * t <= R * R or not d > 0:
        return -1.0
    h = st * t - ct * d
    P = (st * d + ct * t) * st / ct
    num, den = h * (2.0 * P - h) - R * R, 2.0 * (P - h) * R
    if num <= -den:
        return -1.0
    if num >= den:
        return ALMOST_ONE
    return num / den


def exit_root(co, t, d, ua, uc, ue):
    """lambda1 where the ray from a centre (t, d) inside the cone, in a direction with u.a^ = ua, u.c^ = uc and
    u.(c^ x a^) = ue, leaves the cone, or None where it never does; and (A, B, G, den) of the quadratic
    A lambda^2 + 2 B lambda - G = 0 and of lambda1 = G / den.  The discriminant B^2 + A G is formed as the sum of squares
    it is, c^2 [s^2 (uc t - ua d)^2 + ue^2 G]: the plain form cancels to nothing as theta -> pi/2."""
    ct, st = float(co[6]), float(co[7])
    q = 1 - ua * ua
    A = ct * ct * q - st * st * ua * ua
    B = ct * ct * d * uc - st * st * t * ua
    G = (st * t - ct * d) * (st * t + ct * d)
    w = uc * t - ua * d
    den = B + ct * np.sqrt(st * st * w * w + ue * ue * G)
    if not den > 0:
        return None, (A, B, G, den)
    return G / den, (A, B, G, den)


def frame(co, ch, whole=False):
    """(g^, c^ x a^, n^): the generator direction, the azimuthal one and the outward wall normal at the nearest generator.
    Where the cap is the whole sphere (`whole`) its pole is free and the frame is about the axis, (c^, a^ x c^, a^): the
    nodes keep the symmetry of the contact and map onto themselves when the centre crosses the axis."""
    ax, ct, st = np.asarray(co[3:6], float), float(co[6]), float(co[7])
    if not whole:
        return st * ch + ct * ax, np.cross(ch, ax), ct * ch - st * ax
    return ch, np.cross(ax, ch), ax


def cone_sums(lmax, anm, rmax, x, q, co, nq, boundary=None):
    """(V, S_n, T_n, status) of one particle against one cone.  status: 0 out of reach, 1 evaluated, -1 centre at or
    outside the wall or behind the apex (input error: contributes nothing).
    boundary: a list that receives |r den - G| / G of every node whose ray leaves, for the tests that need to know that
    no node sits on the boundary."""
    ct, st = float(co[6]), float(co[7])
    t, rho, d, ch, h = foot(x, co)
    if not h > 0:
        return 0.0, np.zeros(3), np.zeros(3), -1
    if h >= rmax:
        return 0.0, np.zeros(3), np.zeros(3), 0
    ca = cap_cos(co, t, d, rmax)
    whole = ca == -1.0
    e1, e2, nh = frame(co, ch, whole)
    ax = np.asarray(co[3:6], float)
    gt, w = O.gauss_legendre(nq)
    R = quat_to_mat(q)
    V, S, T = 0.0, np.zeros(3), np.zeros(3)
    for k in range(nq):
        mu = 0.5 * (1 + ca) + 0.5 * (1 - ca) * gt[k]
        sg = np.sqrt(max(0.0, 1 - mu * mu))
        om = 0.5 * (1 - ca) * w[k] * 2 * np.pi / (2 * nq)
        for l in range(2 * nq):
            psi = 2 * np.pi * (l + 0.5) / (2 * nq)
            cp, sp = sg * np.cos(psi), sg * np.sin(psi)
            u = cp * e1 + sp * e2 + mu * nh
            ub = R.T @ u
            r, gr = O.sh_eval(lmax, anm, ub, grad=True)
            ua, uc = ((ct * cp - st * mu, st * cp + ct * mu) if not whole else (mu, cp))   # u.a^, u.c^
            lam, (A, B, G, den) = exit_root(co, t, d, ua, uc, sp)
            if lam is None:
                continue
            if boundary is not None:
                boundary.append(abs(r * den - G) / G)
            if not r * den > G:
                continue
            Ai = R @ (r * r * ub - r * (gr - (ub @ gr) * ub))
            V += om * (r ** 3 - lam ** 3) / 3
            S += om * Ai
            T += om * np.cross(r * u, Ai)
    return V, S, T, 1


def contact_point(S, T, t, rho, co):
    """(r_i from x_i, rho_c, t_c) where the line x_i + S x T / |S|^2 + s S^ leaves the cone, or None: the quadratic of the
    nodes with the base point's (rho0, t0) and S^.  A > 0: the larger root; else the smaller one, which needs G > 0 and a
    positive denominator.  No root, t_c <= 0 or rho_c = 0: None."""
    ax, ct, st = np.asarray(co[3:6], float), float(co[6]), float(co[7])
    q = S @ S
    rp, sh = np.cross(S, T) / q, S / np.sqrt(q)
    ra, sa = rp @ ax, sh @ ax
    t0 = t + ra
    r0 = rho + rp - ra * ax
    sp = sh - sa * ax
    A = ct * ct * (sp @ sp) - st * st * sa * sa
    B = ct * ct * (r0 @ sp) - st * st * t0 * sa
    G = st * st * t0 * t0 - ct * ct * (r0 @ r0)
    D = B * B + A * G
    if not D >= 0:
        return None
    sq = np.sqrt(D)
    if A > 0:
        s = G / (B + sq) if B > 0 else (sq - B) / A
    elif G > 0 and B + sq > 0:
        s = G / (B + sq)
    else:
        return None
    rc, tc = r0 + s * sp, t0 + s * sa
    if not (tc > 0 and rc @ rc > 0):
        return None
    return rp + s * sh, rc, tc


def contact_wrench(V, S, T, x, co, kn, m, tw=None, gamma=0.0, mu=0.0, gt=0.0, omega=0.0):
    """(F_i, tau_i, E, details) of one contact with V > 0: force law, damping, friction."""
    ax, ct, st = np.asarray(co[3:6], float), float(co[6]), float(co[7])
    p = kn * m * V ** (m - 1)
    pt = p
    if tw is not None:
        pt = max(0.0, p + gamma * (S @ tw[:3] + T @ tw[3:]))
    F, tau = -pt * S, -pt * T
    det = dict(p=p, pt=pt, N=pt * np.linalg.norm(S), Ft=np.zeros(3), ri=None, capped=False)
    if tw is not None and mu != 0 and gt != 0 and S @ S > 0 and det["N"] > 0:
        t, rho = foot(x, co)[:2]
        cp = contact_point(S, T, t, rho, co)
        if cp is not None:
            ri, rc, tc = cp
            nc = st * ax - ct * rc / np.sqrt(rc @ rc)
            vrel = tw[:3] + np.cross(tw[3:], ri) - omega * np.cross(ax, rc)
            vt = vrel - (vrel @ nc) * nc
            s = np.linalg.norm(vt)
            kappa, capped = (gt, False) if gt * s <= mu * det["N"] else (mu * det["N"] / s, True)
            Ft = -kappa * vt
            F, tau = F + Ft, tau + np.cross(ri, Ft)
            det.update(Ft=Ft, ri=ri, capped=capped, vt=vt, nc=nc, rc=rc, tc=tc)
    return F, tau, kn * V ** m, det


def cone_forces(shapes, nq, x, quat, shtype, cones, kn, expo, mask=None, groupbit=1, tw=None, gamma=None, mu=None, gt=None,
                omega=None):
    """shapes: [(lmax, anm, rmax)]; cones [nk][8].  tw [n][6] with gamma, mu, gt, omega [nk] gives the dissipative pass.
    Returns dict f, torque [n][3], cone_out [nk][5] (E_k, the force ON the wall, M_ax), ncontacts, noutside, contacts."""
    n, nk = len(x), len(cones)
    z = np.zeros(nk)
    gamma, mu, gt, omega = (z if v is None else np.broadcast_to(np.asarray(v, float), (nk,)) for v in (gamma, mu, gt, omega))
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nk, 5))
    ncon = nout = 0
    det = []
    for i in range(n):
        if mask is not None and not (int(mask[i]) & groupbit):
            continue
        lmax, anm, rmax = shapes[int(shtype[i])]
        for c in range(nk):
            V, S, T, st = cone_sums(lmax, anm, rmax, x[i], quat[i], cones[c], nq)
            if st < 0:
                nout += 1
            if st <= 0 or not V > 0:
                continue
            F, tau, E, d = contact_wrench(V, S, T, x[i], cones[c], kn[c], expo[c], None if tw is None else tw[i], gamma[c], mu[c],
                                          gt[c], omega[c])
            f[i] += F
            tq[i] += tau
            a, ax = np.asarray(cones[c][:3], float), np.asarray(cones[c][3:6], float)
            out[c, 0] += E
            out[c, 1:4] -= F
            out[c, 4] += ax @ (np.cross(x[i] - a, -F) - tau)
            ncon += 1
            det.append((i, c, d))
    return dict(f=f, torque=tq, cone_out=out, ncontacts=ncon, noutside=nout, contacts=det)
