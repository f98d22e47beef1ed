"""numpy restatement of docs/SPEC.md §2 steps 1-7 for a whole neighbour list, with EXACT inner radii: the yardstick of the
pair-path tests that does not follow §2.6's search.

Gauss nodes come from numpy, r from shapes.sh_radius_np; the gradient of the polynomial F, the cap, the frame, the
nodes, the inside test, the sums and the force law are written out here.  The inner radius of step 6 is the root of g
in the SPEC's bracket, bisected until the bracket is 4 ulp wide -- no extrapolation, no acceptance threshold.  Shares no
code with csrc/ and none with oracle/ (tests/test_pair_ref.py cross-checks the gradient against the oracle's, nothing
else).

Cap branch codes of a slot: -1 not a contact pair, 0 rho <= R_j (full sphere), 1 tangent cone of B_j, 2 rim of the lens.
"""
import json
import os

import numpy as np

from shpair import shapes

HERE = os.path.dirname(os.path.abspath(__file__))
EXPONENTS = (1.0, 1.25, 2.0)
CASES = ("l4_shallow", "l6_shallow", "l6_deep", "l6_rough", "l12_shallow", "l9_general", "l3_body", "l14_loop", "ghosts",
         "soup", "l3_9_mixed")


def quat_to_mat(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def sh_gradient(lmax, anm, u):
    """Cartesian gradient of the polynomial F(x, y, z) of SPEC §1 at u[..., 3]: the recurrence of shapes.sh_radius_np
    with its derivative in z carried along, E_{m-1} kept for the x and y parts."""
    a = np.asarray(anm, dtype=np.float64).reshape(-1, 2)
    u = np.asarray(u, dtype=np.float64)
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    gx, gy, gz = np.zeros_like(z), np.zeros_like(z), np.zeros_like(z)
    cm, sm = np.ones_like(z), np.zeros_like(z)          # E_m
    cp, sp = np.zeros_like(z), np.zeros_like(z)         # E_{m-1}
    pmm = np.sqrt(1.0 / (4.0 * np.pi))
    for m in range(lmax + 1):
        if m > 0:
            pmm = -pmm * np.sqrt((2.0 * m + 1.0) / (2.0 * m))
        fac = 1.0 if m == 0 else 2.0
        p2, p1 = np.zeros_like(z), np.full_like(z, pmm)
        d2, d1 = np.zeros_like(z), np.zeros_like(z)
        k = m * (m + 1) // 2 + m
        wr, wi = a[k, 0] * p1, a[k, 1] * p1
        zr, zi = np.zeros_like(z), np.zeros_like(z)
        for n in range(m + 1, lmax + 1):
            al = np.sqrt((4.0 * n * n - 1.0) / (n * n - m * m))
            be = 0.0 if n - m < 2 else np.sqrt(((2.0 * n + 1.0) * (n + m - 1.0) * (n - m - 1.0)) /
                                               ((n - m) * (n + m) * (2.0 * n - 3.0)))
            p = al * z * p1 - be * p2
            dp = al * (p1 + z * d1) - be * d2
            k = n * (n + 1) // 2 + m
            wr, wi = wr + a[k, 0] * p, wi + a[k, 1] * p
            zr, zi = zr + a[k, 0] * dp, zi + a[k, 1] * dp
            p2, p1, d2, d1 = p1, p, d1, dp
        gz = gz + fac * (zr * cm - zi * sm)
        if m > 0:                                       # dE_m/dx = m E_{m-1}, dE_m/dy = i m E_{m-1}
            gx = gx + fac * m * (wr * cp - wi * sp)
            gy = gy - fac * m * (wr * sp + wi * cp)
        cp, sp = cm, sm
        cm, sm = cp * x - sp * y, cp * y + sp * x
    return np.stack([gx, gy, gz], axis=-1)


def cap(rho, Ri, Rj):
    """(cos alpha, branch) of step 2."""
    if rho <= Rj:
        return -1.0, 0
    if rho * rho - Rj * Rj <= Ri * Ri:
        return np.sqrt(rho * rho - Rj * Rj) / rho, 1
    return (rho * rho + Ri * Ri - Rj * Rj) / (2.0 * rho * Ri), 2


def cap_nodes(nq, cosa, c):
    """Directions u[nq][2 nq][3] and solid-angle weights omega[nq][2 nq] of steps 3-4."""
    s = np.copysign(1.0, c[2])
    a = -1.0 / (s + c[2])
    b = c[0] * c[1] * a
    e1 = np.array([1.0 + s * c[0] ** 2 * a, s * b, -s * c[0]])
    e2 = np.array([b, s + c[1] ** 2 * a, -c[1]])
    t, w = np.polynomial.legendre.leggauss(nq)
    mu = 0.5 * (1.0 + cosa) + 0.5 * (1.0 - cosa) * t
    sig = np.sqrt(np.maximum(0.0, 1.0 - mu * mu))
    psi = 2.0 * np.pi * (np.arange(2 * nq) + 0.5) / (2 * nq)
    ring = np.cos(psi)[:, None] * e1 + np.sin(psi)[:, None] * e2
    u = sig[:, None, None] * ring[None] + mu[:, None, None] * c
    om = np.repeat((0.5 * (1.0 - cosa) * w * 2.0 * np.pi / (2 * nq))[:, None], 2 * nq, axis=1)
    return u, om


def g_ray(lj, anmj, Rj, Rmj, u, d, lam):
    """g(lambda) of step 6 on the rays u[N][3]; lam[..., N]."""
    q = (lam[..., None] * u - d) @ Rmj                  # R_j^T (lam u - d)
    s = np.linalg.norm(q, axis=-1)
    s1 = np.where(s > 0.0, s, 1.0)
    return np.where(s > 0.0, s - shapes.sh_radius_np(lj, anmj, q / s1[..., None]), -Rj)


def exact_roots(lj, anmj, Rj, Rmj, u, d, rho, ri):
    """Roots of g in the bracket of step 6 for the inside nodes u[N][3] of a pair whose centre of i is outside j.
    Returns (r_in, |g(r_in)|, sign changes of g on 64 equal sub-intervals of the bracket)."""
    bp = u @ d
    if rho < Rj:
        a = np.zeros_like(ri)
    else:
        a = bp - np.sqrt(np.maximum(0.0, bp * bp - (rho * rho - Rj * Rj)))
    b = ri.copy()
    lam = a + (b - a) * np.linspace(0.0, 1.0, 65)[:, None]
    pos = g_ray(lj, anmj, Rj, Rmj, u, d, lam) >= 0.0
    pos[0], pos[-1] = True, False                       # g(a) >= 0 by construction, g(r_i) < 0: the node is inside
    changes = (pos[1:] != pos[:-1]).sum(axis=0)
    for _ in range(400):
        todo = (b - a) > 4.0 * np.spacing(np.maximum(np.abs(a), np.abs(b)))
        if not todo.any():
            break
        mid = 0.5 * (a + b)
        up = g_ray(lj, anmj, Rj, Rmj, u, d, mid) >= 0.0
        a = np.where(todo & up, mid, a)
        b = np.where(todo & ~up, mid, b)
    else:
        raise RuntimeError("bisection did not reach 4 ulp")
    rin = 0.5 * (a + b)
    return rin, np.abs(g_ray(lj, anmj, Rj, Rmj, u, d, rin)), changes


def pair_slot(shape_i, shape_j, xi, qi, xj, qj, nq):
    """One list slot, i integrated.  shape = (lmax, anm, rmax).  Returns dict V, S[3], T[3], nin (inside nodes),
    branch, rin0 (the r_in = 0 branch was taken), multi (some bracket holds more than one sign change of g),
    resid (largest |g| at an accepted root)."""
    (li, ai, Ri), (lj, aj, Rj) = shape_i, shape_j
    out = dict(V=0.0, S=np.zeros(3), T=np.zeros(3), nin=0, branch=-1, rin0=False, multi=False, resid=0.0)
    d = np.asarray(xj, float) - np.asarray(xi, float)
    rho = np.sqrt(d @ d)
    if rho >= Ri + Rj or not rho > 0.0:                 # step 1: separated, or no line of centres
        return out
    cosa, out["branch"] = cap(rho, Ri, Rj)
    u, om = cap_nodes(nq, cosa, d / rho)
    u, om = u.reshape(-1, 3), om.ravel()
    Rmi, Rmj = quat_to_mat(qi), quat_to_mat(qj)
    ub = u @ Rmi                                        # R_i^T u
    ri = shapes.sh_radius_np(li, ai, ub)
    q = (ri[:, None] * u - d) @ Rmj
    s = np.linalg.norm(q, axis=1)
    s1 = np.where(s > 0.0, s, 1.0)
    rj = np.where(s > 0.0, shapes.sh_radius_np(lj, aj, q / s1[:, None]), Rj)
    ins = (s < Rj) & ((s < rj) | (s == 0.0))
    out["nin"] = int(ins.sum())
    if not ins.any():
        return out
    u, om, ub, ri = u[ins], om[ins], ub[ins], ri[ins]
    grad = sh_gradient(li, ai, ub)
    tang = grad - np.sum(ub * grad, axis=1)[:, None] * ub
    A = (ri[:, None] ** 2 * ub - ri[:, None] * tang) @ Rmi.T       # R_i A_i
    out["S"] = np.sum(om[:, None] * A, axis=0)
    out["T"] = np.sum(om[:, None] * np.cross(ri[:, None] * u, A), axis=0)
    if rho < Rj and g_ray(lj, aj, Rj, Rmj, np.zeros((1, 3)), d, np.zeros(1))[0] <= 0.0:
        rin = np.zeros_like(ri)                         # the centre of i lies inside j
        out["rin0"] = True
    else:
        rin, resid, changes = exact_roots(lj, aj, Rj, Rmj, u, d, rho, ri)
        out["resid"] = float(resid.max())
        out["multi"] = bool((changes > 1).any())
    out["V"] = float(np.sum(om * (ri ** 3 - rin ** 3) / 3.0))
    return out


FIELDS = ("V", "S", "T", "nin", "branch", "rin0", "multi", "resid")


def pair_list(shape_table, nq, x, quat, shtype, ilist, offsets, jlist, slots=None):
    """Every slot of a CSR half list (or the given slot numbers): dict of arrays over slots, fields as pair_slot."""
    rows = []
    want = None if slots is None else set(int(p) for p in slots)
    for ii, i in enumerate(ilist):
        for p in range(offsets[ii], offsets[ii + 1]):
            if want is not None and p not in want:
                continue
            j = int(jlist[p]) & 0x1FFFFFFF
            rows.append(pair_slot(shape_table[shtype[i]], shape_table[shtype[j]], x[i], quat[i], x[j], quat[j], nq))
    return {k: np.array([r[k] for r in rows]) for k in FIELDS}


def assemble(pairs, nlist, x, type_, K, E, nlocal, newton=True, skip=None):
    """Step 7 on the per-slot integrals pairs = dict(V, S, T): returns (f[nall][3], torque[nall][3], energy).  nlist =
    (ilist, offsets, jlist); K, E the (ntypes + 1)^2 tables.  A slot touches iff V > 0.  skip: bool per slot, left out."""
    ilist, offsets, jlist = nlist
    f, tq, eng = np.zeros((len(x), 3)), np.zeros((len(x), 3)), 0.0
    for ii, i in enumerate(ilist):
        for p in range(offsets[ii], offsets[ii + 1]):
            V = pairs["V"][p]
            if not V > 0.0 or (skip is not None and skip[p]):
                continue
            j = int(jlist[p]) & 0x1FFFFFFF
            kn, m = K[type_[i], type_[j]], E[type_[i], type_[j]]
            pn = kn if m == 1.0 else kn * m * V ** (m - 1.0)
            Fi, Ti = -pn * pairs["S"][p], -pn * pairs["T"][p]
            f[i] += Fi
            tq[i] += Ti
            if newton or j < nlocal:
                Fj = -Fi
                f[j] += Fj
                tq[j] += -Ti - np.cross(x[j] - x[i], Fj)
            eng += (1.0 if newton or j < nlocal else 0.5) * kn * V ** m
    return f, tq, eng


# ---- the committed fixtures (tests/golden/pair_ref_<name>.npz, root_shortcut.json; recorder: golden/make_pair_ref.py)

def kn_table(ntypes, m):
    """The coefficient tables every comparison with the fixtures uses: kn = 500 (ti + tj), one exponent."""
    K = np.zeros((ntypes + 1, ntypes + 1))
    for a in range(1, ntypes + 1):
        for b in range(1, ntypes + 1):
            K[a, b] = 500.0 * (a + b)
    return K, np.full((ntypes + 1, ntypes + 1), float(m))


def load_fixture(name):
    g = dict(np.load(os.path.join(HERE, "golden", f"pair_ref_{name}.npz")))
    for k in ("lmax", "nq", "nlocal", "ntypes", "newton"):
        g[k] = int(g[k])
    g["shape_table"] = [(g["lmax"], a, r) for a, r in zip(g["a_nm"], g["rmax"])]
    g["nlist"] = (g["ilist"], g["offsets"], g["jlist"])
    return g


def load_shortcut():
    with open(os.path.join(HERE, "golden", "root_shortcut.json")) as fh:
        return json.load(fh)


def without_slots(nlist, drop):
    """The CSR list with the slots drop[p] = True removed (same rows)."""
    ilist, offsets, jlist = nlist
    keep = ~np.asarray(drop, bool)
    csum = np.concatenate([[0], np.cumsum(keep)])
    return ilist, csum[offsets].astype(np.int32), jlist[keep]


def deviations(f, tq, f_ref, tq_ref):
    """(max |dF| / max|F|, max |dtau| / max(|F|, |tau|)) of SPEC §4, components."""
    fs = np.abs(f_ref).max()
    ts = max(fs, np.abs(tq_ref).max())
    return np.abs(f - f_ref).max() / fs, np.abs(tq - tq_ref).max() / ts
