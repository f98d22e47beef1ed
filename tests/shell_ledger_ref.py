"""numpy restatement of docs/SPEC.md §2.20 (the cylinder entries of the energy ledger): the yardstick of the shell-ledger
tests.

Per (particle, cylinder) the three powers (P_d, P_f, Wdot_c) from the definitions of the SPEC, with the quantities the
force law formed: the per-contact sums, the contact point and the law of a cylinder without a spring come from
tests/cyl_ref.py, the spring law from tests/cyl_history_ref.py; what §2.20 adds is written out here, in the space frame.
Shares no code with the kernels (csrc/cyl_power_kernels.hpp and the LEDGER instances of csrc/cylinder_kernels.hpp).
"""
import numpy as np

import cyl_history_ref as CH
import cyl_ref as Cy


def contact_powers(V, S, T, x, cyl, kn, m, tw, gamma, mu, gt, omega, kt=0.0, xi=(0.0, 0.0), dt=0.0):
    """One contact with V > 0: dict F, tau (on the particle), E, P = (P_d, P_f, Wdot_c), p, vd = Vdot, Ft, kind, ratio and
    xi (the spring coming out; None where the cylinder has no history or a guard resets it)."""
    ax, Rc = np.asarray(cyl[3:6], float), float(cyl[6])
    p = kn * m * V ** (m - 1)
    vd = S @ tw[:3] + T @ tw[3:]
    pt = max(0.0, p + gamma * vd)
    out = dict(p=p, vd=vd, pt=pt, Ft=np.zeros(3), kind=CH.NONE, ratio=None, xi=None, friction=False)
    Pd, Pf, Wc = (pt - p) * vd, 0.0, 0.0
    if mu != 0 and kt != 0:                      # a history cylinder (§2.19): P_f = -F_t.v_t
        F, tau, E, d = CH.contact_history(V, S, T, x, cyl, kn, m, tw, gamma, mu, gt, omega, kt, xi, dt)
        out["kind"] = CH.RESET
        if d is not None:
            Pf = -(d["Ft"] @ d["vt"])
            Wc = omega * (d["Ft"] @ np.cross(ax, d["rc"]))
            out.update(Ft=d["Ft"], kind=d["kind"], ratio=d["ratio"], xi=d["xi"], friction=True, rc=d["rc"], ri=d["ri"], vt=d["vt"])
    else:                                        # §2.18: P_f = kappa |v_t|^2
        F, tau, E, d = Cy.contact_wrench(V, S, T, x, cyl, kn, m, tw, gamma, mu, gt, omega)
        if d["ri"] is not None:
            vt, N = d["vt"], d["N"]
            kappa = mu * N / np.linalg.norm(vt) if d["capped"] else gt
            rc = -Rc * d["nc"]
            Pf = kappa * (vt @ vt)
            Wc = omega * (d["Ft"] @ np.cross(ax, rc))
            out.update(Ft=d["Ft"], friction=True, rc=rc, ri=d["ri"], vt=vt, capped=d["capped"])
    out.update(F=F, tau=tau, E=E, P=np.array([Pd, Pf, Wc]))
    return out


def shell_pass(shapes, nq, x, quat, shtype, tw, cyls, kn, expo, gamma, mu, gt, omega, kt=0.0, xi=None, live=None, dt=0.0, mask=None,
               groupbit=1):
    """One cylinder pass of §2.18 + §2.19 with the powers of §2.20.  Coefficients are scalars or [nc].  Returns f, torque
    [n][3], cyl_out [nc][5], P [n][nc][3] (zeros where nothing is in contact or a guard drops the term), xi, live (the
    state coming out; the state going in for dt = 0), ncontacts, and ratios: |F*| / (mu N) of the history contacts."""
    n, nc = len(x), len(cyls)
    kn, expo, gamma, mu, gt, omega, kt = (np.broadcast_to(np.asarray(v, float), (nc,)) for v in (kn, expo, gamma, mu, gt, omega, kt))
    xi = np.zeros((n, nc, 2)) if xi is None else np.asarray(xi, float).reshape(n, nc, 2)
    live = np.zeros((n, nc), bool) if live is None else np.asarray(live, bool).reshape(n, nc)
    f, tq, out, P = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nc, 5)), np.zeros((n, nc, 3))
    xi1, live1 = np.zeros((n, nc, 2)), np.zeros((n, nc), bool)
    ncon, ratios, kinds = 0, [], []
    for i in range(n):
        if mask is not None and not (int(mask[i]) & groupbit):
            continue
        lmax, anm, rmax = shapes[int(shtype[i])]
        for c in range(nc):
            V, S, T, st = Cy.cyl_sums(lmax, anm, rmax, x[i], quat[i], cyls[c], nq)
            if st <= 0 or not V > 0:
                continue
            d = contact_powers(V, S, T, x[i], cyls[c], kn[c], expo[c], tw[i], gamma[c], mu[c], gt[c], omega[c], kt[c],
                               xi[i, c] if live[i, c] else np.zeros(2), dt)
            f[i] += d["F"]
            tq[i] += d["tau"]
            P[i, c] = d["P"]
            a, ax = np.asarray(cyls[c][:3], float), np.asarray(cyls[c][3:6], float)
            out[c, 0] += d["E"]
            out[c, 1:4] -= d["F"]
            out[c, 4] += ax @ (np.cross(x[i] - a, -d["F"]) - d["tau"])
            ncon += 1
            kinds.append(d["kind"])
            if d["xi"] is not None:
                xi1[i, c], live1[i, c] = d["xi"], True
                ratios.append(d["ratio"])
    if dt == 0:
        xi1, live1 = xi.copy(), live.copy()
    return dict(f=f, torque=tq, cyl_out=out, P=P, xi=xi1, live=live1, ncontacts=ncon, ratios=np.array(ratios), kinds=kinds)


def shell_fold(P, dt=1.0):
    """One fold of a pass: per_cylinder [nc][3] = dt (sum P_d, sum P_f, sum Wdot_c), and the three totals."""
    per = dt * P.sum(axis=0)
    return per, per.sum(axis=0)


# ---- the closure trajectory: one unit sphere thrown obliquely at the shell of a rotating drum ----------------------------

# A drum along y through (4, 4, 4) in the box [0, 8]^3; the sphere (L = 0, R = 1, bounding radius 1.01, unit density)
# starts 0.03 inside the wall's reach, moving outwards, along the axis and across, with a spin; no gravity.
THROW = dict(nq=8, kn=2000.0, m=1.25, Rc=3.0, gamma=60.0, mu=0.4, gt=25.0, omega=1.5, dt=4e-4, nsteps=600,
             x0=(4.0, 4.0, 4.0 - (3.0 - 1.04)), v0=(0.8, 0.5, -1.6), w0=(0.6, -0.9, 0.4))
THROW["cyl"] = (4.0, 4.0, 4.0, 0.0, 1.0, 0.0, THROW["Rc"])


def thrown_sphere(k=1, elastic=False, c=THROW):
    """The run loop's explicit velocity Verlet at dt / k on the reference's own sums: half kick, drift, force at x(t + dt) with
    the half-step twist, fold, half kick.  Returns dict E0, E1 (kinetic energy: the sphere starts and ends out of contact),
    D_d, D_f, W (the shell ledger), h (the final depth margin Rc - d), steps in contact, P_d >= 0 throughout."""
    from shpair import shapes
    anm = shapes.sphere(1.0)
    mass = 4.0 / 3.0 * np.pi
    inertia = 0.4 * mass
    cyl = np.array(c["cyl"])
    gamma, mu, gt = (0.0, 0.0, 0.0) if elastic else (c["gamma"], c["mu"], c["gt"])
    dt = c["dt"] / k
    x, v, w = np.array(c["x0"], float), np.array(c["v0"], float), np.array(c["w0"], float)
    q = np.array([1.0, 0.0, 0.0, 0.0])           # a sphere: the orientation enters no sum

    def force(x, v, w):
        V, S, T, st = Cy.cyl_sums(0, anm, 1.01, x, q, cyl, c["nq"])
        assert st >= 0
        if st == 0 or not V > 0:
            return np.zeros(3), np.zeros(3), np.zeros(3), False
        d = contact_powers(V, S, T, x, cyl, c["kn"], c["m"], np.concatenate([v, w]), gamma, mu, gt, c["omega"])
        return d["F"], d["tau"], d["P"], True

    ke = lambda: 0.5 * mass * (v @ v) + 0.5 * inertia * (w @ w)
    F, tau, _, touching = force(x, v, w)
    assert not touching
    E0, acc, ncontact, mono = ke(), np.zeros(3), 0, True
    for _ in range(c["nsteps"] * k):
        v = v + 0.5 * dt * F / mass
        w = w + 0.5 * dt * tau / inertia
        x = x + dt * v
        F, tau, P, touching = force(x, v, w)
        acc += dt * P
        ncontact += touching
        mono = mono and P[0] >= 0.0 and P[1] >= 0.0
        v = v + 0.5 * dt * F / mass
        w = w + 0.5 * dt * tau / inertia
    return dict(E0=E0, E1=ke(), D_d=acc[0], D_f=acc[1], W=acc[2], h=cyl[6] - Cy.foot(x, cyl)[1], ncontact=ncontact, mono=mono,
                touching=touching)


def residual(r):
    """|Delta E_mech - (W_shell - D_shell)| of a thrown_sphere result."""
    return abs(r["E1"] - r["E0"] - (r["W"] - r["D_d"] - r["D_f"]))
