"""numpy restatement of docs/SPEC.md §2.14 (tangential contact springs with history for SH pairs): the yardstick of the
history tests, built on tests/friction_ref.py.

Two functions: the per-slot law (one pass with a time step over the expanded list: forces, torques, the new xi and
per-slot details) and the carry of xi across a rebuild by key (i, owner tag of j).  Shares no code with the kernels
(csrc/history_kernels.hpp).
"""
import numpy as np

import damp_ref as D
import friction_ref as F

NONE, STICK, SLIDE, RESET_UNTOUCHED, RESET_GUARD = 0, 1, 2, 3, 4


def spring(xi, vt, S, N, mu, kt, gt, dt):
    """(F_t, new xi, slides?) of one live history slot: advance, project, trial force, cap."""
    xp = xi + dt * vt
    xp = xp - (xp @ S) * S / (S @ S)
    Fs = -kt * xp - gt * vt
    fn = np.linalg.norm(Fs)
    if fn <= mu * N:
        return Fs, xp, False
    Ft = Fs * (mu * N / fn)
    return Ft, -(Ft + gt * vt) / kt, True


def pair_history(pairs, pi, pj, x, tw, type_, shtype, rmax, K, E, G, MU, GT, KT, xi, dt, nlocal, newton_pair=True, needv=True):
    """dF, dtau [nall][3] of the contact pass (damping of §2.10, friction of §2.11 for the type pairs without a k_t, the
    springs of §2.14 for those with one), the xi [nslots][3] the pass leaves (the input where dt = 0: a look writes
    nothing) and per-slot details: kind (NONE: the type pair has no history; STICK, SLIDE, RESET_UNTOUCHED, RESET_GUARD),
    Ft, vt, N, cap (mu N), trial (|F*|), power (-F_t.v_t, before the slot's share)."""
    nall, ns = len(x), len(pi)
    f, tq = np.zeros((nall, 3)), np.zeros((nall, 3))
    xn = np.zeros((ns, 3))
    det = dict(kind=np.zeros(ns, int), Ft=np.full((ns, 3), np.nan), vt=np.full((ns, 3), np.nan), N=np.full(ns, np.nan),
               cap=np.full(ns, np.nan), trial=np.full(ns, np.nan), power=np.zeros(ns))
    for s, (i, j) in enumerate(zip(pi, pj)):
        V, S, T = pairs[s, 0], pairs[s, 1:4], pairs[s, 4:7]
        ti, tj = int(type_[i]), int(type_[j])
        touched, p = D.pressure(V, S, K[ti, tj], E[ti, tj], needv)
        g, mu, gt, kt = G[ti, tj], MU[ti, tj], GT[ti, tj], KT[ti, tj]
        hist = mu != 0 and kt != 0
        fric = hist or (mu != 0 and gt != 0)
        if hist:
            det["kind"][s] = RESET_UNTOUCHED
        if not touched or (g == 0 and not fric):
            continue
        d = x[j] - x[i]
        A = T - np.cross(d, S)
        ptot = p
        if g != 0:
            vd = S @ (tw[i, :3] - tw[j, :3]) + T @ tw[i, 3:] - A @ tw[j, 3:]
            ptot = max(0.0, p + g * vd)
        delta = ptot - p
        Fi, Ti, Tj = -delta * S, -delta * T, delta * A
        q = S @ S
        if hist:
            det["kind"][s] = RESET_GUARD
            N = ptot * np.sqrt(q)
            if q > 0 and d @ d > 0 and N > 0:
                ri = F.contact_point(S, T, d, rmax[int(shtype[i])], rmax[int(shtype[j])])
                rj = ri - d
                vrel = (tw[i, :3] + np.cross(tw[i, 3:], ri)) - (tw[j, :3] + np.cross(tw[j, 3:], rj))
                vt = vrel - (vrel @ S) * S / q
                Ft, xn[s], slid = spring(xi[s], vt, S, N, mu, kt, gt, dt)
                det["kind"][s] = SLIDE if slid else STICK
                det["Ft"][s], det["vt"][s], det["N"][s], det["cap"][s] = Ft, vt, N, mu * N
                xp = xi[s] + dt * vt
                det["trial"][s] = np.linalg.norm(-kt * (xp - (xp @ S) * S / q) - gt * vt)
                det["power"][s] = -(Ft @ vt)
                Fi = Fi + Ft
                Ti = Ti + np.cross(ri, Ft)
                Tj = Tj - np.cross(rj, Ft)
        elif fric and q > 0:
            N = ptot * np.sqrt(q)
            ri = F.contact_point(S, T, d, rmax[int(shtype[i])], rmax[int(shtype[j])])
            rj = ri - d
            vrel = (tw[i, :3] + np.cross(tw[i, 3:], ri)) - (tw[j, :3] + np.cross(tw[j, 3:], rj))
            vt = vrel - (vrel @ S) * S / q
            Ft, _, cp = F.capped(vt, N, mu, gt)
            Fi = Fi + Ft
            Ti = Ti + np.cross(ri, Ft)
            Tj = Tj - np.cross(rj, Ft)
        f[i] += Fi
        tq[i] += Ti
        if newton_pair or j < nlocal:
            f[j] -= Fi
            tq[j] += Tj
    if dt == 0:
        xn = np.array(xi, dtype=float, copy=True)
    return f, tq, xn, det


def owner_tags(pj, nlocal, tag=None, gowner=None):
    """The key of every slot: the tag of j's owner.  tag None: the tag is the row index, and ghost row nlocal + g belongs to
    gowner[g]; with tags a ghost row holds its owner's."""
    pj = np.asarray(pj)
    if tag is not None:
        return np.asarray(tag)[pj]
    own = np.where(pj < nlocal, pj, np.asarray(gowner)[np.maximum(pj - nlocal, 0)] if gowner is not None and len(gowner) else pj)
    return own


def carry(old_offsets, old_keys, old_xi, new_offsets, new_keys):
    """xi of the new slots: row i's new slot with owner tag k takes the xi of row i's old slot with owner tag k, or zero.
    Row by row, the first old slot with the key (a row holds a key at most once: SPEC §7's edge >= 2 c_max)."""
    out = np.zeros((len(new_keys), 3))
    for i in range(len(new_offsets) - 1):
        a, b = old_offsets[i], old_offsets[i + 1]
        for w in range(new_offsets[i], new_offsets[i + 1]):
            hit = np.flatnonzero(np.asarray(old_keys[a:b]) == new_keys[w])
            if hit.size:
                out[w] = old_xi[a + hit[0]]
    return out
