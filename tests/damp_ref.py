"""numpy restatement of docs/SPEC.md §2.10 (volume-rate contact damping): the yardstick of the damping tests.

Input: the per-pair integrals (V, S_n, T_n) in the space frame, positions, twists, the expanded list and the coefficient
tables; output: the damping force and torque alone.  The wall part takes its per-contact sums from tests/wall_ref.py.
The twists come from the oracle's mass properties.  Shares no code with the kernels (csrc/dissipation_kernels.hpp).
"""
import numpy as np

import wall_ref as W


def expand(ilist, offsets, jlist):
    """(pair_i, pair_j), one entry per CSR slot."""
    cnt = np.diff(np.asarray(offsets))
    return np.repeat(np.asarray(ilist), cnt).astype(np.int64), np.asarray(jlist).astype(np.int64)


def twists(massprops, density, v, quat, angmom, shtype):
    """[n][6]: w = v - omega x (R c), omega = R I^-1 R^T L.  massprops[s] = oracle.mass_props of shape s (unit density)."""
    n = len(v)
    out = np.zeros((n, 6))
    for i in range(n):
        mp, rho = np.asarray(massprops[int(shtype[i])]), float(density[int(shtype[i])])
        xx, yy, zz, xy, xz, yz = rho * mp[4:10]
        J = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
        R = W.quat_to_mat(quat[i])
        om = R @ np.linalg.solve(J, R.T @ angmom[i])
        out[i, :3] = v[i] - np.cross(om, R @ mp[1:4])
        out[i, 3:] = om
    return out


def pressure(V, S, kn, m, needv=True):
    """(touched, p) as the contact kernels' epilogue decides: V > 0, or S_n != 0 where the volume is not computed (m = 1)."""
    if V > 0:
        return True, kn * m * V ** (m - 1)
    if not needv and np.any(S != 0):
        return True, kn
    return False, 0.0


def pair_damping(pairs, pi, pj, x, tw, type_, K, E, G, nlocal, newton_pair=True, needv=True, details=False):
    """dF, dtau [nall][3] of the damping pass.  pairs[slot] = V, S_n[3], T_n[3]; K, E, G: (ntypes+1)^2 tables of kn, exponent,
    gamma.  details: also the per-slot (delta, Vdot, p) with NaN for the slots that take no part."""
    nall = len(x)
    f, tq = np.zeros((nall, 3)), np.zeros((nall, 3))
    det = np.full((len(pi), 3), np.nan)
    for s, (i, j) in enumerate(zip(pi, pj)):
        V, S, T = pairs[s, 0], pairs[s, 1:4], pairs[s, 4:7]
        ti, tj = int(type_[i]), int(type_[j])
        touched, p = pressure(V, S, K[ti, tj], E[ti, tj], needv)
        g = G[ti, tj]
        if not touched or g == 0:
            continue
        d = x[j] - x[i]
        A = T - np.cross(d, S)
        vd = S @ (tw[i, :3] - tw[j, :3]) + T @ tw[i, 3:] - A @ tw[j, 3:]
        delta = max(0.0, p + g * vd) - p
        det[s] = delta, vd, p
        f[i] -= delta * S
        tq[i] -= delta * T
        if newton_pair or j < nlocal:
            f[j] += delta * S
            tq[j] += delta * A
    return (f, tq, det) if details else (f, tq)


def wall_forces_damped(shapes, nq, x, quat, shtype, tw, planes, kn, expo, gamma):
    """The wall pass of §2.10: f, torque [n][3], wall_out [nw][4] (E_w = kn V^m, force ON the wall), per-contact details."""
    n, nw = len(x), len(planes)
    f, tq, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((nw, 4))
    det = []
    for i in range(n):
        lmax, anm, rmax = shapes[int(shtype[i])]
        for w in range(nw):
            V, S, T, st = W.wall_sums(lmax, anm, rmax, x[i], quat[i], planes[w], nq)
            if st <= 0 or not V > 0:
                continue
            p = kn[w] * expo[w] * V ** (expo[w] - 1)
            vd = S @ tw[i, :3] + T @ tw[i, 3:]
            pt = max(0.0, p + gamma[w] * vd)
            det.append((i, w, p, pt, vd))
            f[i] -= pt * S
            tq[i] -= pt * T
            out[w, 0] += kn[w] * V ** expo[w]
            out[w, 1:] += pt * S
    return dict(f=f, torque=tq, wall_out=out, contacts=det)


def sphere_collision_1d(gamma, kn, m, R=1.0, gap=0.02, vrel=2.0, dt=2e-4, nsteps=700):
    """Two equal spheres (unit density) head-on, §2.10 in one dimension with the exact lens volume
    V = pi d^2 (6R - d) / 12 of overlap depth d, the run loop's leapfrog and half-step velocities.
    Returns (separation speed, kinetic energy after / before)."""
    mu = 0.5 * 4.0 / 3.0 * np.pi * R ** 3      # reduced mass; s = distance of the centres
    s, sd = 2 * R + gap, -vrel

    def force(s, sd):
        d = 2 * R - s
        if d <= 0:
            return 0.0
        V, dV = np.pi * d * d * (6 * R - d) / 12, np.pi * d * (4 * R - d) / 4
        return max(0.0, kn * m * V ** (m - 1) + gamma * dV * (-sd)) * dV

    F = force(s, sd)
    for _ in range(nsteps):
        sd += 0.5 * dt * F / mu
        s += dt * sd
        F = force(s, sd)
        sd += 0.5 * dt * F / mu
    return sd, (sd / vrel) ** 2
