"""numpy restatement of docs/SPEC.md §2.16 (rolling and twisting resistance of SH pairs, no history): the yardstick of
the rolling tests.

Input as for tests/damp_ref.py — the per-pair integrals (V, S_n, T_n) in the space frame, positions, twists, the expanded
list and the coefficient tables; output: the torques the pass adds (it adds no force) and per-slot details.  p_tot is the
one of damp_ref.pair_damping.  Shares no code with the kernels (csrc/rolling_kernels.hpp).
"""
import numpy as np

import damp_ref as D


def kappa(norm, N, mu, gamma):
    """(kappa, capped?) of one of the two couples: gamma while gamma |Omega| <= mu N, mu N / |Omega| beyond."""
    if gamma * norm <= mu * N:
        return gamma, False
    return mu * N / norm, True


def pair_rolling(pairs, pi, pj, x, tw, type_, K, E, G, MUR, GR, MUTW, GTW, nlocal, newton_pair=True, needv=True):
    """dtau [nall][3] of the rolling pass and per-slot details: a dict of arrays with NaN / False for the slots that take
    no part — touched, live (a slot that enters the law: touched, a coefficient set, q > 0, N > 0), clamped (N = 0 under a
    gamma_ij), N, M[3], Or[3], On[3], nr = |Omega_r|, nn = |Omega_n|, cap_r = mu_r N, cap_tw = mu_tw N, visc_r = gamma_r nr,
    visc_tw = gamma_tw nn, roll / twist (the kind is set for the type pair), capped_r, capped_tw, power (>= 0, the
    dissipated one)."""
    nall, ns = len(x), len(pi)
    tq = np.zeros((nall, 3))
    nan = lambda *sh: np.full((ns,) + sh, np.nan)
    det = dict(touched=np.zeros(ns, bool), live=np.zeros(ns, bool), clamped=np.zeros(ns, bool), N=nan(), M=nan(3), Or=nan(3),
               On=nan(3), nr=nan(), nn=nan(), cap_r=nan(), cap_tw=nan(), visc_r=nan(), visc_tw=nan(), roll=np.zeros(ns, bool),
               twist=np.zeros(ns, bool), capped_r=np.zeros(ns, bool), capped_tw=np.zeros(ns, bool), power=np.zeros(ns))
    for s, (i, j) in enumerate(zip(pi, pj)):
        V, S, T = pairs[s, 0], pairs[s, 1:4], pairs[s, 4:7]
        ti, tj = int(type_[i]), int(type_[j])
        touched, p = D.pressure(V, S, K[ti, tj], E[ti, tj], needv)
        det["touched"][s] = touched
        roll = MUR[ti, tj] != 0 and GR[ti, tj] != 0
        twist = MUTW[ti, tj] != 0 and GTW[ti, tj] != 0
        q = S @ S
        if not touched or not (roll or twist) or not q > 0:
            continue
        det["roll"][s], det["twist"][s] = roll, twist
        g, ptot = G[ti, tj], p
        if g != 0:
            d = x[j] - x[i]
            A = T - np.cross(d, S)
            vd = S @ (tw[i, :3] - tw[j, :3]) + T @ tw[i, 3:] - A @ tw[j, 3:]
            ptot = max(0.0, p + g * vd)
        N = ptot * np.sqrt(q)
        det["N"][s] = N
        if not N > 0:
            det["clamped"][s] = True
            continue
        det["live"][s] = True
        Om = tw[i, 3:] - tw[j, 3:]
        On = (Om @ S) * S / q
        Or = Om - On
        nr, nn = np.linalg.norm(Or), np.linalg.norm(On)
        kr, cr = kappa(nr, N, MUR[ti, tj], GR[ti, tj]) if roll else (0.0, False)
        kt, ct = kappa(nn, N, MUTW[ti, tj], GTW[ti, tj]) if twist else (0.0, False)
        M = -kr * Or - kt * On
        det["M"][s], det["Or"][s], det["On"][s], det["nr"][s], det["nn"][s] = M, Or, On, nr, nn
        det["cap_r"][s], det["cap_tw"][s] = MUR[ti, tj] * N, MUTW[ti, tj] * N
        det["visc_r"][s], det["visc_tw"][s] = GR[ti, tj] * nr, GTW[ti, tj] * nn
        det["capped_r"][s], det["capped_tw"][s] = cr, ct
        det["power"][s] = kr * nr * nr + kt * nn * nn
        tq[i] += M
        if newton_pair or j < nlocal:
            tq[j] -= M
    return tq, det
