"""numpy restatement of docs/SPEC.md §2.17 (rolling and twisting resistance at planar walls, no history): the yardstick of
the wall-rolling tests.

The per-contact sums come from tests/wall_ref.py (wall_sums), the force of a contact — the whole force the wall pass leaves
in its (particle, wall) row — from the pieces of tests/friction_ref.py (wall_contact_point, capped) and
tests/wall_history_ref.py (spring_law), put together per contact as those modules do; what §2.17 adds is written out here:
the normal load from the row along the exact wall normal, the split of omega_i, the two caps, the couple and its power.
Shares no code with the kernels (csrc/wall_roll_kernels.hpp).

VARIANTS are hand-made WRONG laws, kept here only (never in the library) so that tests/test_wall_roll_ref.py can show
that its property checks reject them.
"""
import numpy as np

import friction_ref as F
import wall_history_ref as H
import wall_ref as W

VISCOUS, CAPPED, NONE = "viscous", "capped", "none"
# the normal taken from S_n, a missing cap, a sign flip, u_w subtracted from Omega
VARIANTS = ("normal_from_S", "no_cap", "sign_flip", "minus_uw")


def couple(Fw, nrm, omega, mur, gr, mutw, gtw, variant=None, S=None, uw=None):
    """One (particle, wall) of §2.17.  Fw: the row's force ON the wall (minus the whole force on the particle), nrm: the
    wall's unit normal, omega: omega_i.  Returns (M, power >= 0, (rolling branch, twisting branch), N).
    variant: one of VARIANTS (S: the contact's S_n for "normal_from_S", uw: the wall's velocity for "minus_uw")."""
    nrm, Om = np.asarray(nrm, float), np.asarray(omega, float)
    if variant == "normal_from_S":
        nrm = -np.asarray(S, float) / np.linalg.norm(S)
    if variant == "minus_uw":
        Om = Om - np.asarray(uw, float)
    N = max(0.0, -(nrm @ np.asarray(Fw, float)))
    roll, twist = mur != 0 and gr != 0, mutw != 0 and gtw != 0
    if not N > 0 or not (roll or twist):
        return np.zeros(3), 0.0, (NONE, NONE), N
    On = (Om @ nrm) * nrm
    Or = Om - On
    nr, nn = np.linalg.norm(Or), np.linalg.norm(On)
    kr = kt = 0.0
    br = bt = NONE
    if roll:
        kr, br = (gr, VISCOUS) if gr * nr <= mur * N or variant == "no_cap" else (mur * N / nr, CAPPED)
    if twist:
        kt, bt = (gtw, VISCOUS) if gtw * nn <= mutw * N or variant == "no_cap" else (mutw * N / nn, CAPPED)
    M = -kr * Or - kt * On
    if variant == "sign_flip":
        M = -M
    return M, kr * nr * nr + kt * nn * nn, (br, bt), N


def reach_sums(shapes, nq, x, quat, shtype, planes, mask=None, groupbit=1):
    """{(i, w): (V, S_n, T_n)} for every owned particle of the group and every wall in its mask of the candidate pass
    (0 < h < R), V <= 0 included.  The expensive part of the reference: compute once, share."""
    out = {}
    for i in range(len(x)):
        if mask is not None and not (int(mask[i]) & groupbit):
            continue
        lmax, anm, rmax = shapes[int(shtype[i])]
        for w in range(len(planes)):
            V, S, T, st = W.wall_sums(lmax, anm, rmax, x[i], quat[i], planes[w], nq)
            if st == 1:
                out[(i, w)] = (V, S, T)
    return out


def contact_force(V, S, T, xi_, twi, plane, kn, m, gamma=0.0, mu=0.0, gt=0.0, kt=0.0, uw=(0.0, 0.0, 0.0), dt=0.0):
    """(F_i, tau_i, p_tot, P_d, P_f) of one contact under §2.9-§2.12 and §2.15, the spring starting from nothing live."""
    if not V > 0:
        return np.zeros(3), np.zeros(3), 0.0, 0.0, 0.0
    nrm = np.asarray(plane[:3], float)
    wl = twi[:3] - np.asarray(uw, float)
    p = kn * m * V ** (m - 1)
    vd = S @ wl + T @ twi[3:]
    pt = max(0.0, p + gamma * vd)
    Fi, tau, Pf = -pt * S, -pt * T, 0.0
    N = pt * np.linalg.norm(S)
    hist = mu != 0 and kt != 0
    if (hist or (mu != 0 and gt != 0)) and S @ S > 0 and (N > 0 or not hist):
        ri = F.wall_contact_point(S, T, nrm, nrm @ xi_ - plane[3])
        vrel = wl + np.cross(twi[3:], ri)
        vt = vrel - (vrel @ nrm) * nrm
        if hist:
            Ft = H.spring_law(np.zeros(3), vt, nrm, N, mu, gt, kt, dt)[0]
        else:
            Ft = F.capped(vt, N, mu, gt)[0]
        Fi, tau, Pf = Fi + Ft, tau + np.cross(ri, Ft), -(Ft @ vt)
    return Fi, tau, pt, (pt - p) * vd, Pf


def wall_roll(sums, n, x, tw, planes, kn, expo, mur, gr, mutw, gtw, gamma=None, mu=None, gt=None, kt=None, vel=None, dt=0.0,
              variant=None):
    """One wall pass with §2.17 on, from reach_sums' table.  Returns f, torque (the whole pass), couple [n][3] (what §2.17
    adds), wall_out [nw][4], power [n][nw] (>= 0, of the couples), pd / pf [n][nw] (the contact's own damping and friction
    power), branch {(i, w): (rolling, twisting)}, N and NS {(i, w)}: the load from the row and p_tot |S_n|."""
    nw = len(planes)
    z = np.zeros(nw)
    gamma, mu, gt, kt = (z if a is None else np.asarray(a, float) for a in (gamma, mu, gt, kt))
    vel = np.zeros((nw, 3)) if vel is None else np.asarray(vel, float).reshape(nw, 3)
    f, tq, cpl, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nw, 4))
    power, pd, pf = np.zeros((n, nw)), np.zeros((n, nw)), np.zeros((n, nw))
    branch, Ns, NS = {}, {}, {}
    for (i, w) in sorted(sums):                       # particle by particle, the walls in index order
        V, S, T = sums[(i, w)]
        Fi, tau, pt, pd[i, w], pf[i, w] = contact_force(V, S, T, x[i], tw[i], planes[w], kn[w], expo[w], gamma[w], mu[w], gt[w],
                                                        kt[w], vel[w], dt)
        M, power[i, w], branch[(i, w)], Ns[(i, w)] = couple(-Fi, planes[w][:3], tw[i, 3:], mur[w], gr[w], mutw[w], gtw[w],
                                                            variant=variant, S=S if V > 0 else planes[w][:3] * -1.0, uw=vel[w])
        NS[(i, w)] = pt * np.linalg.norm(S) if V > 0 else 0.0
        f[i] += Fi
        tq[i] += tau
        cpl[i] += M
        if V > 0:
            out[w, 0] += kn[w] * V ** expo[w]
        out[w, 1:] -= Fi
    return dict(f=f, torque=tq + cpl, couple=cpl, wall_out=out, power=power, pd=pd, pf=pf, branch=branch, N=Ns, NS=NS)


def branch_counts(branch):
    """How many contacts took each of the four branches."""
    c = {("roll", VISCOUS): 0, ("roll", CAPPED): 0, ("twist", VISCOUS): 0, ("twist", CAPPED): 0}
    for br, bt in branch.values():
        if br != NONE:
            c[("roll", br)] += 1
        if bt != NONE:
            c[("twist", bt)] += 1
    return c
