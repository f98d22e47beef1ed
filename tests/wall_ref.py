"""numpy restatement of docs/SPEC.md §2.9 (contact of an SH particle with fixed planes): the yardstick of the wall tests.

r_i and its gradient come from the CPU oracle's sh_eval, the Gauss-Legendre nodes from the oracle; the frame, the nodes
and the sums are written out here.  Shares no code with the kernels (csrc/wall_kernels.hpp).
"""
import numpy as np

from oracle import oracle as O


def quat_to_mat(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def wall_sums(lmax, anm, rmax, x, q, plane, nq):
    """(V, S_n, T_n, status) of one particle against one plane (nx, ny, nz, c).  status: 0 out of reach, 1 evaluated,
    -1 centre at or behind the plane (input error: contributes nothing)."""
    n = np.asarray(plane[:3], float)
    h = n @ np.asarray(x, float) - plane[3]
    if not h > 0:
        return 0.0, np.zeros(3), np.zeros(3), -1
    if h >= rmax:
        return 0.0, np.zeros(3), np.zeros(3), 0
    ch, ca = -n, h / rmax
    s = np.copysign(1.0, ch[2])
    a = -1.0 / (s + ch[2])
    b = ch[0] * ch[1] * a
    e1 = np.array([1 + s * ch[0] ** 2 * a, s * b, -s * ch[0]])
    e2 = np.array([b, s + ch[1] ** 2 * a, -ch[1]])
    t, w = O.gauss_legendre(nq)
    R = quat_to_mat(q)
    V, S, T = 0.0, np.zeros(3), np.zeros(3)
    for k in range(nq):
        mu = 0.5 * (1 + ca) + 0.5 * (1 - ca) * t[k]
        sg = np.sqrt(1 - mu * mu)
        om = 0.5 * (1 - ca) * w[k] * 2 * np.pi / (2 * nq)
        for l in range(2 * nq):
            psi = 2 * np.pi * (l + 0.5) / (2 * nq)
            u = sg * (np.cos(psi) * e1 + np.sin(psi) * e2) + mu * ch
            ub = R.T @ u
            r, g = O.sh_eval(lmax, anm, ub, grad=True)
            if not r * mu > h:
                continue
            A = R @ (r * r * ub - r * (g - (ub @ g) * ub))
            V += om * (r ** 3 - (h / mu) ** 3) / 3
            S += om * A
            T += om * np.cross(r * u, A)
    return V, S, T, 1


def force_law(V, S, T, kn, m):
    """(F_i, tau_i, E) of SPEC §2.7 with the wall's kn, m."""
    if not V > 0:
        return np.zeros(3), np.zeros(3), 0.0
    pn = kn * m * V ** (m - 1)
    return -pn * S, -pn * T, kn * V ** m


def wall_forces(shapes, nq, x, quat, shtype, planes, kn, expo, mask=None, groupbit=1):
    """shapes: [(lmax, anm, rmax)]; planes [nw][4].  Returns dict f, torque [n][3], wall_out [nw][4] (E_w and the force
    ON the wall), ncontacts, nbehind."""
    n, nw = len(x), len(planes)
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nw, 4))
    nc = nb = 0
    for i in range(n):
        if mask is not None and not (int(mask[i]) & groupbit):
            continue
        lmax, anm, rmax = shapes[int(shtype[i])]
        for w in range(nw):
            V, S, T, st = wall_sums(lmax, anm, rmax, x[i], quat[i], planes[w], nq)
            if st < 0:
                nb += 1
            if st <= 0:
                continue
            F, tau, E = force_law(V, S, T, kn[w], expo[w])
            f[i] += F
            tq[i] += tau
            out[w, 0] += E
            out[w, 1:] -= F
            nc += V > 0
    return dict(f=f, torque=tq, wall_out=out, ncontacts=int(nc), nbehind=nb)
