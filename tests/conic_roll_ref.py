"""numpy restatement of docs/SPEC.md §2.24 (rolling and twisting resistance at conical walls, no history): the
yardstick of the cone-rolling tests.

The per-contact sums and the force of a cone without a spring come from tests/cone_ref.py (cone_sums, contact_wrench,
foot, frame), the spring law from tests/conic_history_ref.py (contact_history); what §2.24 adds is written out here, in
the space frame: the load along the geometric normal from the row, the angular velocity in the cone's frame, its split
along that normal, the two caps, the couple, its axial moment on the wall and its power.  Shares no code with the
kernel (csrc/conic_roll_kernels.hpp) and mirrors tests/cyl_roll_ref.py.

VARIANTS are hand-made WRONG laws, kept here only (never in the library) so that tests/test_conic_roll_ref.py can show
that its property checks reject them.
"""
import numpy as np

import cone_ref as Co
import conic_history_ref as CH

VISCOUS, CAPPED, NONE = "viscous", "capped", "none"
# Omega_k not subtracted from omega_i, the cylinder's normal -c^ in place of n^, the wall's rotation counted as rolling
# only (its twisting part -Omega_k s n^ left out), a missing cap, a sign flip
VARIANTS = ("omega_k_kept", "cylinder_normal", "rotation_only_rolls", "no_cap", "sign_flip")


def normal(x, co):
    """n^ = cos theta c^ - sin theta a^, the outward wall normal at the nearest generator (c^ on the axis: Co.foot's e1)."""
    ax, ct, st = np.asarray(co[3:6], float), float(co[6]), float(co[7])
    return ct * Co.foot(x, co)[3] - st * ax


def couple(Fw, x, co, omega, Omega_k, mur, gr, mutw, gtw, variant=None):
    """One (particle, cone) of §2.24.  Fw: the row's force ON the wall (minus the whole force on the particle), x: the
    particle's centre, co: the cone's 8 doubles, omega: omega_i, Omega_k: the cone's angular velocity about its axis.
    Returns (M, P_roll >= 0, Wdot = Omega_k a^.M, (rolling branch, twisting branch), N, (M_r, M_tw))."""
    ax = np.asarray(co[3:6], float)
    nh = normal(x, co)
    if variant == "cylinder_normal":
        nh = -Co.foot(x, co)[3]
    z = np.zeros(3)
    N = max(0.0, nh @ np.asarray(Fw, float))
    roll, twist = mur != 0 and gr != 0, mutw != 0 and gtw != 0
    if not N > 0 or not (roll or twist):
        return z, 0.0, 0.0, (NONE, NONE), N, (z, z)
    carried = Omega_k * ax                       # rounded on its own: omega_i = Omega_k a^ gives exactly 0
    Om = np.asarray(omega, float) - (0.0 if variant == "omega_k_kept" else carried)
    On = (Om @ nh) * nh
    Or = Om - On
    if variant == "rotation_only_rolls":         # the drum's rule at a cone: Omega_k a^ taken out of the tangential part alone
        On = (np.asarray(omega, float) @ nh) * nh
        Or = Om - (Om @ nh) * nh
    nr, nn = np.linalg.norm(Or), np.linalg.norm(On)
    kr = kt = 0.0
    br = bt = NONE
    if roll:
        kr, br = (gr, VISCOUS) if gr * nr <= mur * N or variant == "no_cap" else (mur * N / nr, CAPPED)
    if twist:
        kt, bt = (gtw, VISCOUS) if gtw * nn <= mutw * N or variant == "no_cap" else (mutw * N / nn, CAPPED)
    Mr, Mt = -kr * Or, -kt * On
    if variant == "sign_flip":
        Mr, Mt = -Mr, -Mt
    M = Mr + Mt
    return M, kr * nr * nr + kt * nn * nn, Omega_k * (ax @ M), (br, bt), N, (Mr, Mt)


def reach_sums(shapes, nq, x, quat, shtype, cones, mask=None, groupbit=1):
    """{(i, c): (V, S_n, T_n)} for every owned particle of the group and every cone in its mask of the candidate pass
    (0 < h < R), V <= 0 included.  The expensive part of the reference: compute once, share."""
    out = {}
    for i in range(len(x)):
        if mask is not None and not (int(mask[i]) & groupbit):
            continue
        lmax, anm, rmax = shapes[int(shtype[i])]
        for c in range(len(cones)):
            V, S, T, st = Co.cone_sums(lmax, anm, rmax, x[i], quat[i], cones[c], nq)
            if st == 1:
                out[(i, c)] = (V, S, T)
    return out


def conic_roll(sums, n, x, tw, cones, kn, expo, mur, gr, mutw, gtw, gamma=0.0, mu=0.0, gt=0.0, omega=0.0, kt=0.0, dt=0.0,
               variant=None):
    """One cone pass with §2.24 on, from reach_sums' table; the springs of §2.23 start from nothing live.  Coefficients
    are scalars or [nk].  Returns f, torque (the whole pass), torque0 (without §2.24), couple [n][3] (what §2.24 adds),
    cone_out [nk][5] (M_ax with -a^.M), max0 [nk] (M_ax without it), proll, wroll [n][nk], branch {(i, c): (rolling,
    twisting)}, N and NS {(i, c)}: the load from the row and p_tot |S_n|, rows {(i, c)}: F_w, d {(i, c)}: the distance of
    the centre from the axis as computed, ncontacts."""
    nk = len(cones)
    kn, expo, mur, gr, mutw, gtw, gamma, mu, gt, omega, kt = (np.broadcast_to(np.asarray(v, float), (nk,)) for v in
                                                              (kn, expo, mur, gr, mutw, gtw, gamma, mu, gt, omega, kt))
    f, tq, cpl, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nk, 5))
    max0 = np.zeros(nk)
    proll, wroll = np.zeros((n, nk)), np.zeros((n, nk))
    branch, Ns, NS, rows, ds = {}, {}, {}, {}, {}
    ncon = 0
    for (i, c) in sorted(sums):                      # particle by particle, the cones in index order
        V, S, T = sums[(i, c)]
        a, ax = np.asarray(cones[c][:3], float), np.asarray(cones[c][3:6], float)
        Fi, tau, NS[(i, c)] = np.zeros(3), np.zeros(3), 0.0
        if V > 0:
            if mu[c] != 0 and kt[c] != 0:
                Fi, tau, E, _ = CH.contact_history(V, S, T, x[i], cones[c], kn[c], expo[c], tw[i], gamma[c], mu[c], gt[c], omega[c],
                                                   kt[c], np.zeros(3), False, dt)
                pt = max(0.0, kn[c] * expo[c] * V ** (expo[c] - 1) + gamma[c] * (S @ tw[i, :3] + T @ tw[i, 3:]))
            else:
                Fi, tau, E, det = Co.contact_wrench(V, S, T, x[i], cones[c], kn[c], expo[c], tw[i], gamma[c], mu[c], gt[c], omega[c])
                pt = det["pt"]
            NS[(i, c)] = pt * np.linalg.norm(S)
            out[c, 0] += E
            ncon += 1
        M, proll[i, c], wroll[i, c], branch[(i, c)], Ns[(i, c)], _ = couple(-Fi, x[i], cones[c], tw[i, 3:], omega[c], mur[c], gr[c],
                                                                           mutw[c], gtw[c], variant=variant)
        rows[(i, c)] = -Fi
        ds[(i, c)] = Co.foot(x[i], cones[c])[2]
        f[i] += Fi
        tq[i] += tau
        cpl[i] += M
        out[c, 1:4] -= Fi
        m0 = ax @ (np.cross(x[i] - a, -Fi) - tau)
        max0[c] += m0
        out[c, 4] += m0 - ax @ M
    return dict(f=f, torque=tq + cpl, torque0=tq, couple=cpl, cone_out=out, max0=max0, proll=proll, wroll=wroll, branch=branch,
                N=Ns, NS=NS, rows=rows, d=ds, ncontacts=ncon)


def branch_counts(branch):
    """How many (particle, cone) took each of the four branches."""
    c = {("roll", VISCOUS): 0, ("roll", CAPPED): 0, ("twist", VISCOUS): 0, ("twist", CAPPED): 0}
    for br, bt in branch.values():
        if br != NONE:
            c[("roll", br)] += 1
        if bt != NONE:
            c[("twist", bt)] += 1
    return c


def load_gap(r):
    """max |N - p_tot |S_n|| / N over the (particle, cone) with N > 0: what the load along n^ costs (SPEC §2.24)."""
    return max((abs(r["N"][k] - r["NS"][k]) / r["N"][k] for k in r["N"] if r["N"][k] > 0), default=0.0)
