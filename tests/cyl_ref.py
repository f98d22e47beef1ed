"""numpy restatement of docs/SPEC.md §2.18 (contact of an SH particle with the inside of a circular cylinder that may
rotate about its axis): the yardstick of the cylinder tests.

r_i and its gradient come from the CPU oracle's sh_eval, the Gauss-Legendre nodes from the oracle; the foot point, the
cap, the frame, the nodes, the sums, the force law, damping and friction are written out here, in the space frame.
Shares no code with the kernels (csrc/cylinder_kernels.hpp).
"""
import numpy as np

from oracle import oracle as O
from wall_ref import quat_to_mat

ALMOST_ONE = np.nextafter(1.0, 0.0)


def foot(x, cyl):
    """(rho, d, c^): the part of x - a normal to the axis, its length, and the cap direction: rho / d, or, on the axis
    (d = 0 as computed), the e1 of the frame rule of §2.3 about the axis."""
    a, ax = np.asarray(cyl[:3], float), np.asarray(cyl[3:6], float)
    y = np.asarray(x, float) - a
    rho = y - (y @ ax) * ax
    d = np.sqrt(rho @ rho)
    if d > 0:
        return rho, d, rho / d
    s = np.copysign(1.0, ax[2])
    k = -1.0 / (s + ax[2])
    return rho, d, np.array([1 + s * ax[0] ** 2 * k, s * ax[0] * ax[1] * k, -s * ax[0]])


def cap_cos(Rc, d, R):
    """cos alpha = (Rc^2 - d^2 - R^2) / (2 d R), clamped to [-1, 1), formed without dividing where it is clamped."""
    num, den = (Rc - d) * (Rc + d) - R * R, 2.0 * d * R
    if num <= -den:
        return -1.0
    if num >= den:
        return ALMOST_ONE
    return num / den


def cyl_sums(lmax, anm, rmax, x, q, cyl, nq, boundary=None):
    """(V, S_n, T_n, status) of one particle against one cylinder (a[3], axis[3], Rc).  status: 0 out of reach,
    1 evaluated, -1 centre at or outside the cylinder (input error: contributes nothing).
    boundary: a list that receives |(q r + 2 b) r - g| / g of every node, for the tests that need to know that no node
    sits on the boundary."""
    ax, Rc = np.asarray(cyl[3:6], float), float(cyl[6])
    rho, d, ch = foot(x, cyl)
    if not d < Rc:
        return 0.0, np.zeros(3), np.zeros(3), -1
    if Rc - d >= rmax:
        return 0.0, np.zeros(3), np.zeros(3), 0
    ca = cap_cos(Rc, d, rmax)
    g = (Rc - d) * (Rc + d)
    e1, e2 = ax, np.cross(ch, ax)
    t, w = O.gauss_legendre(nq)
    R = quat_to_mat(q)
    V, S, T = 0.0, np.zeros(3), np.zeros(3)
    for k in range(nq):
        mu = 0.5 * (1 + ca) + 0.5 * (1 - ca) * t[k]
        sg = np.sqrt(max(0.0, 1 - mu * mu))
        om = 0.5 * (1 - ca) * w[k] * 2 * np.pi / (2 * nq)
        for l in range(2 * nq):
            psi = 2 * np.pi * (l + 0.5) / (2 * nq)
            cp = sg * np.cos(psi)
            u = cp * e1 + sg * np.sin(psi) * e2 + mu * ch
            ub = R.T @ u
            r, gr = O.sh_eval(lmax, anm, ub, grad=True)
            qq, b = 1 - cp * cp, d * mu
            if boundary is not None:
                boundary.append(abs((qq * r + 2 * b) * r - g) / g)
            if not (qq * r + 2 * b) * r > g:
                continue
            A = R @ (r * r * ub - r * (gr - (ub @ gr) * ub))
            rin = g / (b + np.sqrt(b * b + qq * g))
            V += om * (r ** 3 - rin ** 3) / 3
            S += om * A
            T += om * np.cross(r * u, A)
    return V, S, T, 1


def contact_point(S, T, rho, ax, Rc):
    """(r_i from x_i, rho_c) where the line x_i + S x T / |S|^2 + s S^ leaves the cylinder (the larger root), or None
    where S^ is along the axis or the line misses the cylinder."""
    q = S @ S
    rp, sh = np.cross(S, T) / q, S / np.sqrt(q)
    r0 = rho + rp - (rp @ ax) * ax
    sp = sh - (sh @ ax) * ax
    A, B, C = sp @ sp, r0 @ sp, r0 @ r0 - Rc * Rc
    D = B * B - A * C
    if not (A > 0 and D >= 0):
        return None
    s = -C / (B + np.sqrt(D)) if B > 0 else (np.sqrt(D) - B) / A
    return rp + s * sh, r0 + s * sp


def contact_wrench(V, S, T, x, cyl, kn, m, tw=None, gamma=0.0, mu=0.0, gt=0.0, omega=0.0):
    """(F_i, tau_i, E, details) of one contact with V > 0: force law, damping, friction."""
    ax, Rc = np.asarray(cyl[3:6], float), float(cyl[6])
    p = kn * m * V ** (m - 1)
    pt = p
    if tw is not None:
        pt = max(0.0, p + gamma * (S @ tw[:3] + T @ tw[3:]))
    F, tau = -pt * S, -pt * T
    det = dict(p=p, pt=pt, N=pt * np.linalg.norm(S), Ft=np.zeros(3), ri=None, capped=False)
    if tw is not None and mu != 0 and gt != 0 and S @ S > 0 and det["N"] > 0:
        rho = foot(x, cyl)[0]
        cp = contact_point(S, T, rho, ax, Rc)
        if cp is not None:
            ri, rc = cp
            nc = -rc / Rc
            vrel = tw[:3] + np.cross(tw[3:], ri) - omega * np.cross(ax, rc)
            vt = vrel - (vrel @ nc) * nc
            s = np.linalg.norm(vt)
            kappa, capped = (gt, False) if gt * s <= mu * det["N"] else (mu * det["N"] / s, True)
            Ft = -kappa * vt
            F, tau = F + Ft, tau + np.cross(ri, Ft)
            det.update(Ft=Ft, ri=ri, capped=capped, vt=vt, nc=nc)
    return F, tau, kn * V ** m, det


def cyl_forces(shapes, nq, x, quat, shtype, cyls, kn, expo, mask=None, groupbit=1, tw=None, gamma=None, mu=None, gt=None,
               omega=None):
    """shapes: [(lmax, anm, rmax)]; cyls [nc][7].  tw [n][6] with gamma, mu, gt, omega [nc] gives the dissipative pass.
    Returns dict f, torque [n][3], cyl_out [nc][5] (E_c, the force ON the wall, M_ax), ncontacts, noutside, contacts."""
    n, nc = len(x), len(cyls)
    z = np.zeros(nc)
    gamma, mu, gt, omega = (z if v is None else np.broadcast_to(np.asarray(v, float), (nc,)) for v in (gamma, mu, gt, omega))
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nc, 5))
    ncon = nout = 0
    det = []
    for i in range(n):
        if mask is not None and not (int(mask[i]) & groupbit):
            continue
        lmax, anm, rmax = shapes[int(shtype[i])]
        for c in range(nc):
            V, S, T, st = cyl_sums(lmax, anm, rmax, x[i], quat[i], cyls[c], nq)
            if st < 0:
                nout += 1
            if st <= 0 or not V > 0:
                continue
            F, tau, E, d = contact_wrench(V, S, T, x[i], cyls[c], kn[c], expo[c], None if tw is None else tw[i], gamma[c], mu[c],
                                          gt[c], omega[c])
            f[i] += F
            tq[i] += tau
            a, ax = np.asarray(cyls[c][:3], float), np.asarray(cyls[c][3:6], float)
            out[c, 0] += E
            out[c, 1:4] -= F
            out[c, 4] += ax @ (np.cross(x[i] - a, -F) - tau)
            ncon += 1
            det.append((i, c, d))
    return dict(f=f, torque=tq, cyl_out=out, ncontacts=ncon, noutside=nout, contacts=det)
