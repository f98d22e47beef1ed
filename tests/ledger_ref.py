"""numpy restatement of docs/SPEC.md §2.13 (the energy ledger): the yardstick of the ledger tests.

Per list slot and per (particle, wall) the power a contact dissipates, and per wall the rate of work -F_w.u_w, from the
definitions of the SPEC: P_d = delta Vdot, P_f = kappa |v_t|^2 with the velocities the force law saw.  The clamp, the
contact points and the capped law come from tests/damp_ref.py and tests/friction_ref.py, the per-contact sums of a wall
from tests/wall_ref.py; what §2.13 adds is written out here.  Shares no code with the kernels (the LEDGER instances of
csrc/dissipation_kernels.hpp and csrc/wall_kernels.hpp, csrc/ledger_kernels.hpp).
"""
import numpy as np

import damp_ref as D
import friction_ref as F
import wall_ref as W


def share(j, nlocal, newton_pair):
    """The share of a slot in a rank's tally: 1 with newton_pair, else a half for i and a half for an owned j."""
    return 1.0 if newton_pair else 0.5 + 0.5 * (j < nlocal)


def pair_powers(pairs, pi, pj, x, tw, type_, shtype, rmax, K, E, G, MU, GT, nlocal, newton_pair=True, needv=True, shared=True):
    """[nslots][2]: P_d, P_f of every slot (zeros for a slot that takes no part), times the slot's share if `shared`."""
    out = np.zeros((len(pi), 2))
    for s, (i, j) in enumerate(zip(pi, pj)):
        V, S, T = pairs[s, 0], pairs[s, 1:4], pairs[s, 4:7]
        ti, tj = int(type_[i]), int(type_[j])
        touched, p = D.pressure(V, S, K[ti, tj], E[ti, tj], needv)
        g, mu, gt = G[ti, tj], MU[ti, tj], GT[ti, tj]
        if not touched:
            continue
        d = x[j] - x[i]
        ptot = p
        if g != 0:
            A = T - np.cross(d, S)
            vd = S @ (tw[i, :3] - tw[j, :3]) + T @ tw[i, 3:] - A @ tw[j, 3:]
            ptot = max(0.0, p + g * vd)
            out[s, 0] = (ptot - p) * vd            # gamma Vdot^2, or p |Vdot| for a clamped contact
        q = S @ S
        if mu != 0 and gt != 0 and q > 0:
            ri = F.contact_point(S, T, d, rmax[int(shtype[i])], rmax[int(shtype[j])])
            vrel = (tw[i, :3] + np.cross(tw[i, 3:], ri)) - (tw[j, :3] + np.cross(tw[j, 3:], ri - d))
            vt = vrel - (vrel @ S) * S / q
            _, kappa, _ = F.capped(vt, ptot * np.sqrt(q), mu, gt)
            out[s, 1] = kappa * (vt @ vt)
        if shared:
            out[s] *= share(j, nlocal, newton_pair)
    return out


def wall_powers(shapes, nq, x, quat, shtype, tw, planes, kn, expo, gamma, mu, gt, vel):
    """Per (particle, wall): P [n][nw][2] = P_d, P_f of the wall-relative twist, and Fw [n][nw][3], the whole force ON the
    wall (damping and friction included).  tw may be None where no wall has a coefficient (the elastic contact)."""
    n, nw = len(x), len(planes)
    vel = np.zeros((nw, 3)) if vel is None else np.asarray(vel, float).reshape(nw, 3)
    P, Fw = np.zeros((n, nw, 2)), np.zeros((n, nw, 3))
    for i in range(n):
        lmax, anm, rmax = shapes[int(shtype[i])]
        for w in range(nw):
            V, S, T, st = W.wall_sums(lmax, anm, rmax, x[i], quat[i], planes[w], nq)
            if st <= 0 or not V > 0:
                continue
            nrm = np.asarray(planes[w][:3], float)
            p = pt = kn[w] * expo[w] * V ** (expo[w] - 1)
            fric = mu[w] != 0 and gt[w] != 0 and S @ S > 0
            Ft = np.zeros(3)
            if gamma[w] != 0 or fric:
                wl, om = tw[i, :3] - vel[w], tw[i, 3:]
                vd = S @ wl + T @ om
                pt = max(0.0, p + gamma[w] * vd)
                P[i, w, 0] = (pt - p) * vd
                if fric:
                    ri = F.wall_contact_point(S, T, nrm, nrm @ x[i] - planes[w][3])
                    vrel = wl + np.cross(om, ri)
                    vt = vrel - (vrel @ nrm) * nrm
                    Ft, kappa, _ = F.capped(vt, pt * np.linalg.norm(S), mu[w], gt[w])
                    P[i, w, 1] = kappa * (vt @ vt)
            Fw[i, w] = pt * S - Ft
    return P, Fw


def wall_ledger(P, Fw, vel, dt=1.0):
    """One fold of a wall pass: per_wall [nw][3] = dt (sum P_d, sum P_f, -F_w.u_w), and the three wall totals."""
    nw = P.shape[1]
    vel = np.zeros((nw, 3)) if vel is None else np.asarray(vel, float).reshape(nw, 3)
    per = np.zeros((nw, 3))
    per[:, :2] = dt * P.sum(axis=0)
    per[:, 2] = -dt * (Fw.sum(axis=0) * vel).sum(axis=1)
    return per, per.sum(axis=0)


def oracle_sphere_integrals(nq, R=1.0, rmax=1.01):
    """s -> (V, S_n.x) of two spheres of radius R (bounding radius rmax) with centres s apart along x, by the ORACLE's
    sharp rule at n_q: the integrals the contact kernels form.  Head-on, a whole ring of nodes enters or leaves the cap at
    once, so S_n steps as s changes where the closed-form lens is smooth."""
    from oracle import oracle as O
    from shpair import shapes
    anm = shapes.sphere(R)
    il, of, jl = np.array([0], np.int32), np.array([0, 1], np.int32), np.array([1], np.int32)
    q, ty, sh = np.array([[1.0, 0, 0, 0]] * 2), np.ones(2, np.int32), np.zeros(2, np.int32)
    K, E = np.array([[0.0, 0.0], [0.0, 1.0]]), np.ones((2, 2))      # the integrals do not depend on the force law

    def integrals(s):
        if s >= 2 * rmax:
            return 0.0, 0.0
        o = O.compute([(0, anm, rmax)], K, E, nq, 2, np.array([[0.0, 0, 0], [s, 0, 0]]), q, ty, sh, il, of, jl, force_volume=True,
                      want_pairs=True)
        return o["pairs"][0, 0], o["pairs"][0, 1]
    return integrals


def sphere_collision_ledger(gamma, kn, m, R=1.0, gap=0.02, vrel=2.0, dt=2e-4, nsteps=700, integrals=None):
    """damp_ref.sphere_collision_1d with the ledger: two equal spheres (unit density, L = 0) head-on, the closed-form lens
    of friction_ref.lens_integrals (or integrals(s) -> (V, S_n.x), e.g. oracle_sphere_integrals), the run loop's leapfrog;
    the power of a step is delta Vdot at x(t + dt) with the half-step velocity, as the loop forms it.  Returns (E_mech
    before, E_mech after, D, D never decreased, final distance) with E_mech = KE + kn V^m."""
    mu = 0.5 * 4.0 / 3.0 * np.pi * R ** 3      # reduced mass; s = distance of the centres
    s, sd = 2 * R + gap, -vrel

    def contact(s, sd):
        V, S = integrals(s) if integrals else F.lens_integrals(R, s)[:2]
        if not V > 0:
            return 0.0, 0.0, 0.0
        p = kn * m * V ** (m - 1)
        vd = S * (-sd)                             # Vdot = S_n.(w_i - w_j), S_n along +x from i to j
        pt = max(0.0, p + gamma * vd)
        return pt * S, (pt - p) * vd, kn * V ** m  # repulsion on the separation, power, elastic energy

    F0, _, U = contact(s, sd)
    E0, Dsum, mono = 0.5 * mu * sd * sd + U, 0.0, True
    for _ in range(nsteps):
        sd += 0.5 * dt * F0 / mu
        s += dt * sd
        F0, P, U = contact(s, sd)
        mono = mono and P >= 0.0
        Dsum += dt * P
        sd += 0.5 * dt * F0 / mu
    return E0, 0.5 * mu * sd * sd + U, Dsum, mono, s
