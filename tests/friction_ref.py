"""numpy restatement of docs/SPEC.md §2.11 (Coulomb-capped viscous friction, no history): the yardstick of the friction
tests.

Input as for tests/damp_ref.py — the per-pair integrals (V, S_n, T_n) in the space frame, positions, twists, the expanded
list and the coefficient tables — plus the bounding radii; output: the damping AND friction force and torque (the pass
adds both), and per-slot details.  The wall part takes its per-contact sums from tests/wall_ref.py.  Shares no code with
the kernels (csrc/dissipation_kernels.hpp, the friction instance of csrc/wall_kernels.hpp).
"""
import numpy as np

import damp_ref as D
import wall_ref as W


def contact_point(S, T, d, Ri, Rj):
    """r_i from x_i: the point of the line {S x T / q + s S} nearest the radical plane of the bounding spheres."""
    q = S @ S
    t = 0.5 * (1.0 + (Ri ** 2 - Rj ** 2) / (d @ d))
    return np.cross(S, T) / q + t * (d @ S) * S / q


def capped(vt, N, mu, gt):
    """(F_t, kappa, capped?) of F_t = -kappa v_t."""
    s = np.linalg.norm(vt)
    if gt * s <= mu * N:
        return -gt * vt, gt, False
    k = mu * N / s
    return -k * vt, k, True


def pair_friction(pairs, pi, pj, x, tw, type_, shtype, rmax, K, E, G, MU, GT, nlocal, newton_pair=True, needv=True):
    """dF, dtau [nall][3] of the dissipation pass (damping of §2.10 + friction of §2.11) and per-slot details: a dict of
    arrays with NaN / False for the slots that take no part in friction — Ft[3], vt[3], ri[3], N, cap (mu N), visc
    (gamma_t |v_t|), capped, touched, delta."""
    nall, ns = len(x), len(pi)
    f, tq = np.zeros((nall, 3)), np.zeros((nall, 3))
    det = dict(Ft=np.full((ns, 3), np.nan), vt=np.full((ns, 3), np.nan), ri=np.full((ns, 3), np.nan), vrel=np.full((ns, 3), np.nan),
               N=np.full(ns, np.nan), cap=np.full(ns, np.nan), visc=np.full(ns, np.nan), capped=np.zeros(ns, bool),
               touched=np.zeros(ns, bool), fric=np.zeros(ns, bool), delta=np.zeros(ns))
    for s, (i, j) in enumerate(zip(pi, pj)):
        V, S, T = pairs[s, 0], pairs[s, 1:4], pairs[s, 4:7]
        ti, tj = int(type_[i]), int(type_[j])
        touched, p = D.pressure(V, S, K[ti, tj], E[ti, tj], needv)
        g, mu, gt = G[ti, tj], MU[ti, tj], GT[ti, tj]
        fric = mu != 0 and gt != 0
        det["touched"][s] = touched
        if not touched or (g == 0 and not fric):
            continue
        d = x[j] - x[i]
        A = T - np.cross(d, S)
        ptot = p
        if g != 0:
            vd = S @ (tw[i, :3] - tw[j, :3]) + T @ tw[i, 3:] - A @ tw[j, 3:]
            ptot = max(0.0, p + g * vd)
        delta = ptot - p
        det["delta"][s] = delta
        Fi, Ti, Tj = -delta * S, -delta * T, delta * A
        q = S @ S
        if fric and q > 0:
            det["fric"][s] = True
            N = ptot * np.sqrt(q)
            ri = contact_point(S, T, d, rmax[int(shtype[i])], rmax[int(shtype[j])])
            rj = ri - d
            vrel = (tw[i, :3] + np.cross(tw[i, 3:], ri)) - (tw[j, :3] + np.cross(tw[j, 3:], rj))
            vt = vrel - (vrel @ S) * S / q
            Ft, _, cp = capped(vt, N, mu, gt)
            det["Ft"][s], det["vt"][s], det["ri"][s], det["vrel"][s] = Ft, vt, ri, vrel
            det["N"][s], det["cap"][s], det["visc"][s], det["capped"][s] = N, mu * N, gt * np.linalg.norm(vt), cp
            Fi = Fi + Ft
            Ti = Ti + np.cross(ri, Ft)
            Tj = Tj - np.cross(rj, Ft)
        f[i] += Fi
        tq[i] += Ti
        if newton_pair or j < nlocal:
            f[j] -= Fi
            tq[j] += Tj
    return f, tq, det


def wall_contact_point(S, T, n, h):
    """r_i from x_i: S x T / q dropped onto the plane n.(x_i + r) = c, h = n.x_i - c."""
    rp = np.cross(S, T) / (S @ S)
    return rp - (h + n @ rp) * n


def wall_forces_friction(shapes, nq, x, quat, shtype, tw, planes, kn, expo, gamma, mu, gt):
    """The wall pass of §2.10 + §2.11: f, torque [n][3], wall_out [nw][4] (E_w = kn V^m, force ON the wall), per-contact
    details (i, w, p, p_tot, N, F_t[3], r_i[3], capped)."""
    n, nw = len(x), len(planes)
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nw, 4))
    det = []
    for i in range(n):
        lmax, anm, rmax = shapes[int(shtype[i])]
        for w in range(nw):
            V, S, T, st = W.wall_sums(lmax, anm, rmax, x[i], quat[i], planes[w], nq)
            if st <= 0 or not V > 0:
                continue
            nrm = np.asarray(planes[w][:3], float)
            p = kn[w] * expo[w] * V ** (expo[w] - 1)
            pt = max(0.0, p + gamma[w] * (S @ tw[i, :3] + T @ tw[i, 3:]))
            F, tau = -pt * S, -pt * T
            N = pt * np.linalg.norm(S)
            Ft, ri, cp = np.zeros(3), np.full(3, np.nan), False
            if mu[w] != 0 and gt[w] != 0 and S @ S > 0:
                ri = wall_contact_point(S, T, nrm, nrm @ x[i] - planes[w][3])
                vrel = tw[i, :3] + np.cross(tw[i, 3:], ri)
                vt = vrel - (vrel @ nrm) * nrm
                Ft, _, cp = capped(vt, N, mu[w], gt[w])
                F, tau = F + Ft, tau + np.cross(ri, Ft)
            det.append((i, w, p, pt, N, Ft, ri, cp))
            f[i] += F
            tq[i] += tau
            out[w, 0] += kn[w] * V ** expo[w]
            out[w, 1:] -= F
    return dict(f=f, torque=tq, wall_out=out, contacts=det)


def lens_integrals(R, dist):
    """(V, S_n, T_n) of two equal spheres of radius R, centres `dist` apart along +x from i to j: the lens volume, the
    projected cap area along d, no moment."""
    dp = 2 * R - dist
    if dp <= 0:
        return np.zeros(7)
    V = np.pi * dp * dp * (6 * R - dp) / 12
    a2 = R * R - (dist / 2) ** 2
    return np.array([V, np.pi * a2, 0.0, 0.0, 0.0, 0.0, 0.0])
