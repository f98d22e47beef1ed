"""numpy restatement of docs/SPEC.md §2.21 (rolling and twisting resistance at cylindrical walls, no history): the
yardstick of the cylinder-rolling tests.

The per-contact sums come from tests/cyl_ref.py (cyl_sums, foot), the force of a contact — the whole force the cylinder
pass leaves in its (particle, cylinder) row — and its three powers from tests/shell_ledger_ref.py (contact_powers, which
takes the spring law from tests/cyl_history_ref.py); what §2.21 adds is written out here, in the space frame: the radial
load from the row, the angular velocity in the drum's frame, its split along the radial direction, the two caps, the couple,
its axial moment on the shell and its two powers.  Shares no code with the kernels (csrc/cyl_roll_kernels.hpp).

VARIANTS are hand-made WRONG laws, kept here only (never in the library) so that tests/test_cyl_roll_ref.py can show that
its property checks reject them.
"""
import numpy as np

import cyl_ref as Cy
import shell_ledger_ref as SL

VISCOUS, CAPPED, NONE = "viscous", "capped", "none"
# Omega_c not subtracted from omega_i, the normal taken from S_n, a missing cap, a sign flip
VARIANTS = ("omega_c_kept", "normal_from_S", "no_cap", "sign_flip")


def couple(Fw, x, cyl, omega, Omega_c, mur, gr, mutw, gtw, variant=None, S=None):
    """One (particle, cylinder) of §2.21.  Fw: the row's force ON the wall (minus the whole force on the particle), x: the
    particle's centre, cyl: a[3], axis[3], Rc, omega: omega_i, Omega_c: the cylinder's angular velocity about its axis.
    Returns (M, P_roll >= 0, Wdot_roll, (rolling branch, twisting branch), N).
    variant: one of VARIANTS (S: the contact's S_n for "normal_from_S")."""
    ax = np.asarray(cyl[3:6], float)
    ch = Cy.foot(x, cyl)[2]
    if variant == "normal_from_S":
        ch = np.asarray(S, float) / np.linalg.norm(S)
    N = max(0.0, ch @ np.asarray(Fw, float))
    roll, twist = mur != 0 and gr != 0, mutw != 0 and gtw != 0
    if not N > 0 or not (roll or twist):
        return np.zeros(3), 0.0, 0.0, (NONE, NONE), N
    carried = Omega_c * ax                       # rounded on its own: omega_i = Omega_c a^ gives exactly 0
    Om = np.asarray(omega, float) - (0.0 if variant == "omega_c_kept" else carried)
    On = (Om @ ch) * ch
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
    return M, kr * nr * nr + kt * nn * nn, Omega_c * (ax @ M), (br, bt), N


def reach_sums(shapes, nq, x, quat, shtype, cyls, mask=None, groupbit=1):
    """{(i, c): (V, S_n, T_n)} for every owned particle of the group and every cylinder in its mask of the candidate pass
    (0 < Rc - d < R), V <= 0 included.  The expensive part of the reference: compute once, share."""
    out = {}
    for i in range(len(x)):
        if mask is not None and not (int(mask[i]) & groupbit):
            continue
        lmax, anm, rmax = shapes[int(shtype[i])]
        for c in range(len(cyls)):
            V, S, T, st = Cy.cyl_sums(lmax, anm, rmax, x[i], quat[i], cyls[c], nq)
            if st == 1:
                out[(i, c)] = (V, S, T)
    return out


def cyl_roll(sums, n, x, tw, cyls, kn, expo, mur, gr, mutw, gtw, gamma=0.0, mu=0.0, gt=0.0, omega=0.0, kt=0.0, dt=0.0, variant=None,
             xi=None, live=None):
    """One cylinder pass with §2.21 on, from reach_sums' table; the springs of §2.19 start from nothing live, or from xi
    [n][nc][2] where live [n][nc] (a pass in the middle of a run: tests/traj_ref.py).  Coefficients are scalars or [nc].  Returns f, torque (the whole pass), couple [n][3] (what §2.21 adds), cyl_out [nc][5] (M_ax with
    -a^.M), max0 [nc] (M_ax without it), P [n][nc][3] (the power rows of §2.20 with P_roll and Wdot_roll added), P0 (without),
    proll, wroll [n][nc], branch {(i, c): (rolling, twisting)}, N and NS {(i, c)}: the radial load from the row and
    p_tot |S_n|, rows {(i, c)}: F_w, the row's force ON the wall, ncontacts."""
    nc = len(cyls)
    kn, expo, mur, gr, mutw, gtw, gamma, mu, gt, omega, kt = (np.broadcast_to(np.asarray(v, float), (nc,)) for v in
                                                              (kn, expo, mur, gr, mutw, gtw, gamma, mu, gt, omega, kt))
    f, tq, cpl, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nc, 5))
    max0 = np.zeros(nc)
    P, proll, wroll = np.zeros((n, nc, 3)), np.zeros((n, nc)), np.zeros((n, nc))
    branch, Ns, NS, rows = {}, {}, {}, {}
    ncon = 0
    for (i, c) in sorted(sums):                      # particle by particle, the cylinders in index order
        V, S, T = sums[(i, c)]
        a, ax = np.asarray(cyls[c][:3], float), np.asarray(cyls[c][3:6], float)
        Fi, tau, NS[(i, c)] = np.zeros(3), np.zeros(3), 0.0
        if V > 0:
            d = SL.contact_powers(V, S, T, x[i], cyls[c], kn[c], expo[c], tw[i], gamma[c], mu[c], gt[c], omega[c], kt[c],
                                  (0.0, 0.0) if live is None or not live[i][c] else xi[i][c], dt)
            Fi, tau, P[i, c] = d["F"], d["tau"], d["P"]
            NS[(i, c)] = d["pt"] * np.linalg.norm(S)
            out[c, 0] += d["E"]
            ncon += 1
        M, proll[i, c], wroll[i, c], branch[(i, c)], Ns[(i, c)] = couple(-Fi, x[i], cyls[c], tw[i, 3:], omega[c], mur[c], gr[c],
                                                                         mutw[c], gtw[c], variant=variant, S=S if V > 0 else None)
        rows[(i, c)] = -Fi
        f[i] += Fi
        tq[i] += tau
        cpl[i] += M
        out[c, 1:4] -= Fi
        m0 = ax @ (np.cross(x[i] - a, -Fi) - tau)
        max0[c] += m0
        out[c, 4] += m0 - ax @ M
    P0 = P.copy()
    P[:, :, 1] += proll
    P[:, :, 2] += wroll
    return dict(f=f, torque=tq + cpl, torque0=tq, couple=cpl, cyl_out=out, max0=max0, P=P, P0=P0, proll=proll, wroll=wroll,
                branch=branch, N=Ns, NS=NS, rows=rows, ncontacts=ncon)


def branch_counts(branch):
    """How many (particle, cylinder) took each of the four branches."""
    c = {("roll", VISCOUS): 0, ("roll", CAPPED): 0, ("twist", VISCOUS): 0, ("twist", CAPPED): 0}
    for br, bt in branch.values():
        if br != NONE:
            c[("roll", br)] += 1
        if bt != NONE:
            c[("twist", bt)] += 1
    return c


def load_gap(r):
    """max |N - p_tot |S_n|| / N over the (particle, cylinder) with N > 0: what the radial load costs (SPEC §2.21)."""
    return max((abs(r["N"][k] - r["NS"][k]) / r["N"][k] for k in r["N"] if r["N"][k] > 0), default=0.0)


# ---- the closure trajectory: tests/shell_ledger_ref.py's thrown sphere with the two couples on -----------------------------

THROW_ROLL, THROW_TWIST = (0.05, 3.0), (0.03, 2.0)   # (mu_r, gamma_r), (mu_tw, gamma_tw) of the drum's shell


def thrown_sphere(k=1, roll=THROW_ROLL, twist=THROW_TWIST):
    """SL.thrown_sphere (the run loop's explicit velocity Verlet at dt / k on the reference's own sums) with §2.21 on: the
    couple joins the torque, P_roll the friction entry and Wdot_roll the work entry.  Returns dict E0, E1, D_d, D_f, W, h,
    ncontact, D_roll (the part of D_f the couples dissipated)."""
    from shpair import shapes
    c = SL.THROW
    anm = shapes.sphere(1.0)
    mass = 4.0 / 3.0 * np.pi
    inertia = 0.4 * mass
    cyl = np.array(c["cyl"])
    dt = c["dt"] / k
    x, v, w = np.array(c["x0"], float), np.array(c["v0"], float), np.array(c["w0"], float)
    q = np.array([1.0, 0.0, 0.0, 0.0])

    def force(x, v, w):
        V, S, T, st = Cy.cyl_sums(0, anm, 1.01, x, q, cyl, c["nq"])
        assert st >= 0
        if st == 0 or not V > 0:
            return np.zeros(3), np.zeros(3), np.zeros(3), 0.0, False
        d = SL.contact_powers(V, S, T, x, cyl, c["kn"], c["m"], np.concatenate([v, w]), c["gamma"], c["mu"], c["gt"], c["omega"])
        M, Pr, Wr, _, _ = couple(-d["F"], x, cyl, w, c["omega"], roll[0], roll[1], twist[0], twist[1])
        return d["F"], d["tau"] + M, d["P"] + np.array([0.0, Pr, Wr]), Pr, True

    ke = lambda: 0.5 * mass * (v @ v) + 0.5 * inertia * (w @ w)
    F, tau, _, _, touching = force(x, v, w)
    assert not touching
    E0, acc, droll, ncontact = ke(), np.zeros(3), 0.0, 0
    for _ in range(c["nsteps"] * k):
        v = v + 0.5 * dt * F / mass
        w = w + 0.5 * dt * tau / inertia
        x = x + dt * v
        F, tau, P, Pr, touching = force(x, v, w)
        acc += dt * P
        droll += dt * Pr
        ncontact += touching
        v = v + 0.5 * dt * F / mass
        w = w + 0.5 * dt * tau / inertia
    return dict(E0=E0, E1=ke(), D_d=acc[0], D_f=acc[1], W=acc[2], h=cyl[6] - Cy.foot(x, cyl)[1], ncontact=ncontact, D_roll=droll,
                touching=touching)
