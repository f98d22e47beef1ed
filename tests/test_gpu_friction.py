"""GPU tests of the Coulomb-capped friction of docs/SPEC.md §2.11 (csrc/dissipation_kernels.hpp, the friction instance of
csrc/wall_kernels.hpp, through the C ABI of include/shstep.h) against tests/friction_ref.py fed by the ORACLE's per-pair
integrals: forces and torques at SPEC §4's gate (1e-9 of the largest force), the invariants the SPEC states, the
deterministic mode, the run loop and the walls.  The pass does not depend on the order: L = 4, n_q = 8 unless stated.

The coefficients and motion seeds below were chosen on the CPU, with the oracle and the reference alone, so that the
conditions the parity test asserts on its INPUTS hold (both branches of kappa well populated, a clamped slot wherever a
gamma_ij is set, no slot near the branch point, a friction part that is not small)."""
import os
import sys

import numpy as np
import pytest

from common import coeff_tables, oracle_compute
from dissipation_common import (NQ, dev, bed_case, motion, ctx, gpu_forces, _rigid_motion, periodic_run, _total_energy, _wall_ctx,
                                _wall_pass)

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-9
GAMMA = {(1, 1): 300.0, (1, 2): 900.0, (2, 2): 1800.0}
FRIC = {(1, 1): (2.0, 300.0), (1, 2): (1.5, 400.0), (2, 2): (2.5, 250.0)}      # (mu, gamma_t)


def table(ntypes, coef, k=None):
    G = np.zeros((ntypes + 1, ntypes + 1))
    for (a, b), g in coef.items():
        if a <= ntypes and b <= ntypes:
            G[a, b] = G[b, a] = g if k is None else g[k]
    return G


def reference(oracle, case, K, E, gamma, fric, v, L, nlocal=None, newton=True):
    import damp_ref as D
    import friction_ref as F
    b, n = case["bed"], case["n"]
    nlocal = n if nlocal is None else nlocal
    o = oracle_compute(oracle, case, NQ, K, E, nlocal=nlocal, newton_pair=newton, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], case["offsets"], case["jlist"])
    tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
    f, tq, det = F.pair_friction(o["pairs"], pi, pj, b["x"], tw, b["type"], b["shtype"], case["rmax"], K, E, table(2, gamma),
                                 table(2, fric, 0), table(2, fric, 1), nlocal, newton_pair=newton)
    fd, td = D.pair_damping(o["pairs"], pi, pj, b["x"], tw, b["type"], K, E, table(2, gamma), nlocal, newton_pair=newton)
    return dict(elastic_f=o["f"], elastic_t=o["torque"], f=f, torque=tq, twist=tw, det=det, fric_f=f - fd, fric_t=tq - td)


def input_conditions(ref, damped):
    """The conditions of the parity test on its inputs (not measurements of the code under test)."""
    det = ref["det"]
    ok = det["fric"] & det["touched"]
    live = ok & (det["N"] > 0)
    cp = det["capped"][live]
    near = np.abs(det["visc"][live] - det["cap"][live]) / det["cap"][live]
    scale = np.abs(ref["elastic_f"] + ref["f"]).max()
    return dict(touched=int(ok.sum()), ncapped=int(cp.sum()), capped=float(cp.mean()), viscous=float((~cp).mean()), clamped=int((det["N"][ok] == 0).sum()),
                nearest=float(near.min()), fric_share=float(np.abs(ref["fric_f"]).max() / scale), scale=scale, damped=damped)


def assert_input_conditions(c):
    assert c["capped"] >= 0.1 and c["viscous"] >= 0.1, c         # at least 10 % of the touched slots in each branch of kappa
    assert c["ncapped"] >= 5, c                                  # and at least five slots at the cap mu N
    # RELAXED against the issue for one case: a clamped slot (N = 0) needs p_tot = 0 < p, that is a gamma_ij, so in the case
    # with every gamma_ij = 0 none can exist and the condition is waived there; it holds in the six damped cases
    assert c["clamped"] >= 1 or not c["damped"], c
    assert c["nearest"] > 1e-6, c                                # no slot within 1e-6 relative of the branch point
    assert c["fric_share"] > 0.05, c                             # the friction part exceeds 5 % of the largest force


# ---- 1. against the reference --------------------------------------------------------------------------------------

PARITY = [
    # n, bed seed, exponent, nlocal, newton, damping too?, motion seed
    (12, 2, 1.25, None, True, True, 9),        # fewer than 64 slots
    (60, 1, 1.25, None, True, True, 8),
    (60, 1, 1.0, None, True, True, 8),
    (60, 1, 1.25, None, True, False, 8),       # friction with every gamma_ij = 0
    (60, 3, 1.25, 40, False, True, 10),
    (60, 3, 1.25, 40, True, True, 10),
    (150, 4, 1.25, None, True, True, 11),      # more than 256 slots, no multiple of 64 or 256
    (60, 1, 1.75, None, True, True, 8),        # exponents whose V^(m-1) is pow() in the pass (m - 1 = 0.75, 1.5, 0.3): it
    (60, 1, 2.5, None, True, True, 8),         # feeds the damping clamp and the cap mu N
    (60, 1, 1.3, None, True, True, 8),
]


@pytest.mark.parametrize("n,seed,expo,nlocal,newton,damped,mseed", PARITY)
def test_friction_wrench_matches_the_reference_on_oracle_integrals(oracle, n, seed, expo, nlocal, newton, damped, mseed):
    case = bed_case(oracle, n, seed, nlocal)
    npairs = case["jlist"].size
    assert npairs % 64 != 0 and npairs % 256 != 0 and npairs > 10
    assert (npairs < 64) == (n == 12) and (n != 150 or npairs > 256)
    K, E = coeff_tables(2, lambda i, j: 1000.0 + 100.0 * (i + j), expo)
    gamma = GAMMA if damped else {}
    v, L = motion(case, mseed)
    ref = reference(oracle, case, K, E, gamma, FRIC, v, L, nlocal, newton)
    cond = input_conditions(ref, damped)
    print(f"n={n} m={expo} nlocal={nlocal} newton={newton} damped={damped}: {npairs} slots, inputs {cond}")
    assert_input_conditions(cond)
    sp = ctx(case, K, E)
    f0, t0, _ = gpu_forces(sp, case, v, L, nlocal, newton)   # every coefficient 0: the pass launches nothing
    for (a, b), g in gamma.items():
        sp.pair_damping(a, b, g)
    for (a, b), (mu, gt) in FRIC.items():
        sp.pair_friction(a, b, mu, gt)
    f1, t1, tw = gpu_forces(sp, case, v, L, nlocal, newton)
    sp.close()
    scale = cond["scale"]
    tscale = max(scale, np.abs(ref["elastic_t"] + ref["torque"]).max())
    ef, et = np.abs((f1 - f0) - ref["f"]).max() / scale, np.abs((t1 - t0) - ref["torque"]).max() / tscale
    e0 = np.abs(f0 - ref["elastic_f"]).max() / scale
    etw = np.abs(tw - ref["twist"]).max() / np.abs(ref["twist"]).max()
    print(f"  max|F| {scale:.4g}, max|F_fric| {np.abs(ref['fric_f']).max():.4g}, rel err dF {ef:.1e} dtau {et:.1e} elastic {e0:.1e} "
          f"twist {etw:.1e}")
    assert etw <= 1e-12
    assert e0 <= TOL and ef <= TOL and et <= TOL
    if nlocal is not None and not newton:
        assert not f1[nlocal:].any() and not t1[nlocal:].any()
    if nlocal is not None and newton:
        assert np.abs(f1[nlocal:] - f0[nlocal:]).max() > 0           # ghost j rows got their share


# ---- 2. closed form, no oracle ---------------------------------------------------------------------------------------

def _sphere_ctx(det=1, nq=NQ, kn=1e4, expo=1.25):
    from shpair import ShPair, shapes
    sp = ShPair(0)
    sp.settings(nq)
    sp.set_ntypes(1, 1)
    sp.set_shape(0, 0, shapes.sphere(1.0), 1.01)
    sp.coeff(1, 1, kn, expo)
    if det:
        sp.set_option("deterministic", 1)
    return sp


@pytest.mark.parametrize("wz,branch", [(5.0, "viscous"), (40.0, "capped")])
def test_spinning_sphere_against_a_sphere_at_rest_in_closed_form(oracle, wz, branch):
    """Two unit spheres 1.9 apart along x, one spinning about z: r_i = d/2, v_t = omega x d/2, N = p |S_n| from the
    elastic force itself, F_t = -kappa omega x d/2 on the spinner, torques -(+-d/2) x F_t... with §2.11's signs:
    tau_i = r_i x F_t, tau_j = -r_j x F_t = (d/2) x F_t."""
    mu, gt = 0.4, 30.0
    case = dict(n=2, lmax=0, shapes=None, bed=dict(x=np.array([[0.0, 0, 0], [1.9, 0, 0]]), quat=np.array([[1.0, 0, 0, 0]] * 2),
                                                     type=np.ones(2, np.int32), shtype=np.zeros(2, np.int32)))
    sp = _sphere_ctx(det=0)
    sp.set_neighbors_csr(np.array([0], np.int32), np.array([0, 1], np.int32), np.array([1], np.int32))
    Iz = sp.body(0)[2][2]                                    # inertia (xx, yy, zz, ...) of the unit sphere
    v, L = np.zeros((2, 3)), np.array([[0.0, 0, Iz * wz], [0, 0, 0]])
    f0, t0, _ = gpu_forces(sp, case, v, L)
    sp.pair_friction(1, 1, mu, gt)
    f1, t1, tw = gpu_forces(sp, case, v, L)
    sp.close()
    # (the quadrature puts the sphere's centre of mass at rounding distance from its SH origin: w is not exactly 0)
    assert np.abs(tw[0, 5] - wz) <= 1e-14 * wz and not tw[1].any() and np.abs(tw[0, :5]).max() <= 1e-15 * wz
    N = abs(f0[0, 0])                                        # p |S_n|: the elastic force of the pair, along x
    half = np.array([0.95, 0.0, 0.0])
    vt = np.cross([0.0, 0.0, wz], half)
    kappa = gt if gt * np.linalg.norm(vt) <= mu * N else mu * N / np.linalg.norm(vt)
    assert (kappa == gt) == (branch == "viscous")
    Ft = -kappa * vt
    # the sphere's own T_n is rounding of the quadrature: |r_perp| = |T_n| / |S_n| enters r_i
    tn = max(np.abs(t0).max() / N, 1e-16)
    tol = TOL * N + np.abs(Ft).max() * 10 * tn + gt * wz * tn * 10
    df, dt = f1 - f0, t1 - t0
    print(f"omega_z {wz} ({branch}): N {N:.6g}, |F_t| {np.abs(Ft).max():.6g} (mu N {mu * N:.6g}), err f {np.abs(df[0] - Ft).max():.2e}, "
          f"tau_i {np.abs(dt[0] - np.cross(half, Ft)).max():.2e}, tau_j {np.abs(dt[1] - np.cross(half, Ft)).max():.2e}, tol {tol:.2e}")
    assert np.abs(Ft).max() > 1e-3 * N
    assert np.abs(df[0] - Ft).max() <= tol and np.abs(df[1] + Ft).max() <= tol
    assert np.abs(dt[0] - np.cross(half, Ft)).max() <= tol        # tau_i = r_i x F_t
    assert np.abs(dt[1] - np.cross(half, Ft)).max() <= tol        # tau_j = -r_j x F_t, r_j = -d/2
    assert abs(df[0, 0]) <= tol                                   # the normal part is unchanged


# ---- 3. invariants on the GPU result ---------------------------------------------------------------------------------

def test_gpu_friction_conserves_momentum_and_angular_momentum(oracle):
    case = bed_case(oracle, 60, 1)
    K, E = coeff_tables(2, 1000.0, 1.25)
    v, L = motion(case, 11)
    sp = ctx(case, K, E)
    f0, t0, _ = gpu_forces(sp, case, v, L)
    for (a, b), (mu, gt) in FRIC.items():
        sp.pair_friction(a, b, mu, gt)
    f1, t1, _ = gpu_forces(sp, case, v, L)
    sp.close()
    df, dt = f1 - f0, t1 - t0
    x = case["bed"]["x"]
    tot = np.abs(df).sum()
    assert tot > 0
    print(f"net friction force {np.abs(df.sum(axis=0)).max():.2e}, net moment {np.abs((np.cross(x, df) + dt).sum(axis=0)).max():.2e}, sum|dF| {tot:.4g}")
    assert np.abs(df.sum(axis=0)).max() <= 1e-12 * tot
    assert np.abs((np.cross(x, df) + dt).sum(axis=0)).max() <= 1e-12 * tot


def test_rigid_motion_of_a_bed_has_no_friction(oracle):
    case = bed_case(oracle, 60, 1)
    K, E = coeff_tables(2, 1000.0, 1.25)
    v, L = _rigid_motion(case, np.array([0.3, -0.2, 0.5]), np.array([0.4, 0.7, -0.5]))
    sp = ctx(case, K, E)
    f0, t0, _ = gpu_forces(sp, case, v, L)
    for (a, b), (mu, gt) in FRIC.items():
        sp.pair_friction(a, b, mu, gt)
    f1, t1, _ = gpu_forces(sp, case, v, L)
    sp.close()
    fel = np.abs(f0).max()
    print(f"rigid motion: max|dF| {np.abs(f1 - f0).max():.2e}, max|dtau| {np.abs(t1 - t0).max():.2e}, max|F_elastic| {fel:.4g}")
    assert fel > 0 and np.abs(v).max() > 1
    assert np.abs(f1 - f0).max() <= 1e-12 * fel and np.abs(t1 - t0).max() <= 1e-12 * fel


def _periodic_run(fric, v, L=None, det=1):
    return periodic_run(v, L, det, pair_friction=fric)


def test_translation_of_a_periodic_bed_has_no_friction_and_momentum_is_conserved_over_ghost_pairs(oracle):
    import torch
    v0 = np.array([1.5, -0.7, 0.9])
    sp0, r0 = _periodic_run(None, v0)
    f0, t0 = r0.f[:r0.n].cpu().numpy(), r0.tq[:r0.n].cpu().numpy()
    sp0.close()
    sp, r = _periodic_run(FRIC, v0)
    n, ng = r.n, r.nghost
    f1, t1 = r.f[:n].cpu().numpy(), r.tq[:n].cpu().numpy()
    fel = np.abs(f0).max()
    print(f"periodic translation: {n} owned, {ng} ghosts, {r.npairs} slots, max|dF| {np.abs(f1 - f0).max():.2e}, max|F_elastic| {fel:.4g}")
    assert ng > 0 and fel > 0
    assert np.array_equal(f1, f0) and np.array_equal(t1, t0)         # v_rel is exactly 0: ghosts carry their owners' twists
    rng = np.random.default_rng(2)
    r.v[:] = dev(rng.normal(size=(n, 3)))
    r.L[:] = dev(0.3 * rng.normal(size=(n, 3)))
    r.force()
    torch.cuda.synchronize()
    df = r.f[:n].cpu().numpy() - f0
    offs, jl = sp.copy_neighbors(n, r.npairs)
    assert (jl >= n).any()                                             # pairs across the faces
    print(f"periodic random motion: max|dF| {np.abs(df).max():.4g}, net {np.abs(df.sum(axis=0)).max():.2e}")
    assert np.abs(df).max() > 0.05 * fel and np.abs(df.sum(axis=0)).max() <= 1e-12 * np.abs(df).sum()
    sp.close()


# ---- 4. deterministic mode -------------------------------------------------------------------------------------------

def test_deterministic_mode_is_bitwise_reproducible_and_agrees_with_the_atomics(oracle):
    case = bed_case(oracle, 60, 1)
    K, E = coeff_tables(2, 1000.0, 1.25)
    v, L = motion(case, 8)
    runs = []
    for det in (1, 1, 0):
        sp = ctx(case, K, E, det=det, gamma=GAMMA, fric=FRIC)
        f, tq, _ = gpu_forces(sp, case, v, L)
        if det and not runs:
            f2, tq2, _ = gpu_forces(sp, case, v, L)   # the same context again
            assert np.array_equal(f, f2) and np.array_equal(tq, tq2)
        runs.append((f, tq))
        sp.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    scale = np.abs(runs[2][0]).max()
    assert scale > 0
    assert np.abs(runs[0][0] - runs[2][0]).max() <= TOL * scale and np.abs(runs[0][1] - runs[2][1]).max() <= TOL * scale
    sp = ctx(case, K, E, det=1, gamma=GAMMA)          # the friction-free deterministic result
    f0, _, _ = gpu_forces(sp, case, v, L)
    sp.close()
    assert np.abs(runs[0][0] - f0).max() > 0.05 * scale


# ---- 5. off means off ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("damped,det", [(False, 0), (False, 1), (True, 1)])
def test_without_friction_the_dissipation_pass_is_the_damping_pass_bit_for_bit(oracle, damped, det):
    """ONE compute, then the old and the new call each on a copy of its f / torque.  With damping on the comparison is made
    in deterministic mode: the atomic scatter's order is not fixed, so there even two runs of the old call need not agree
    in the last bit."""
    import torch
    case = bed_case(oracle, 60, 1)
    K, E = coeff_tables(2, 1000.0, 1.25)
    v, L = motion(case, 8)
    sp = ctx(case, K, E, det=det, gamma=GAMMA if damped else None)
    sp.pair_friction(1, 2, 0.0, 5.0)          # coefficients that leave every pair without friction
    sp.pair_friction(1, 1, 0.5, 0.0)
    b, n = case["bed"], case["n"]
    x, q, ty, sh = dev(b["x"]), dev(b["quat"]), dev(b["type"].astype(np.int32)), dev(b["shtype"].astype(np.int32))
    f, tq, tw = dev(np.zeros((n, 3))), dev(np.zeros((n, 3))), dev(np.zeros((n, 6)))
    sp.compute_device(n, 0, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f.data_ptr(), tq.data_ptr())
    sp.twist_device(n, 0, dev(v).data_ptr(), q.data_ptr(), dev(L).data_ptr(), sh.data_ptr(), tw.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    fa, ta, fb, tb = f.clone(), tq.clone(), f.clone(), tq.clone()
    sp.pair_damping_device(n, 0, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), fa.data_ptr(), ta.data_ptr())
    sp.pair_dissipation_device(n, 0, x.data_ptr(), ty.data_ptr(), sh.data_ptr(), tw.data_ptr(), fb.data_ptr(), tb.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    sp.close()
    assert torch.equal(fa, fb) and torch.equal(ta, tb)
    assert torch.equal(fa, f) != damped       # damping off: nothing was launched; on: the pass added its wrench


# ---- 6. the run loop -------------------------------------------------------------------------------------------------

def _oblique(fric, use_graph=False, nsteps=0):
    """Two unit spheres, relative velocity 2 along x, centres offset by 1.0 along y (impact plane x-y, normal z)."""
    from shpair.run import DeviceRun
    sp = _sphere_ctx()
    x = np.array([[3.12, 3.5, 4.0], [4.88, 4.5, 4.0]])       # 2.024 apart: just outside each other's bounding spheres
    v = np.array([[1.0, 0, 0], [-1.0, 0, 0]])
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]] * 2), np.zeros(2, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, dt=2e-4,
                  pair_friction=fric)
    r.v[:] = dev(v)
    r.force()
    if nsteps:
        r.run_native(nsteps, use_graph=use_graph)
    return sp, r


def _collide(fric, nsteps=500):
    sp, r = _oblique(fric)
    mass = sp.body(0)[0]
    E, p, J, Ls = [_total_energy(sp, r)], [], [], []
    for _ in range(nsteps):
        r.run_native(1)
        E.append(_total_energy(sp, r))
        x, v, L = r.x[:2].cpu().numpy(), r.v.cpu().numpy(), r.L.cpu().numpy()
        p.append(mass * v.sum(axis=0))
        J.append((np.cross(x, mass * v) + L).sum(axis=0))      # the unit sphere's centre of mass is its SH origin
        Ls.append(L.copy())
    gap = float(np.linalg.norm((r.x[1] - r.x[0]).cpu().numpy()))
    sp.close()
    return np.array(E), np.array(p), np.array(J), np.array(Ls), gap, mass


def test_oblique_impact_in_the_run_loop_spins_both_spheres_up_and_conserves_momenta(oracle):
    E0, p0, J0, L0, gap0, mass = _collide(None)
    drift = np.abs(E0 - E0[0]).max()
    Jscale = np.abs(J0[0]).max()
    print(f"no friction: E0 {E0[0]:.6f}, drift {drift:.3e}, max|L| {np.abs(L0).max():.2e}, gap {gap0:.3f}")
    assert gap0 > 2.02 and np.ptp(E0) > 0 and Jscale > 1.0       # they met and parted; the orbital moment is not small
    assert np.abs(L0).max() <= 1e-12 * Jscale                       # no friction: no spin beyond rounding
    E1, p1, J1, L1, gap1, _ = _collide({(1, 1): (0.5, 50.0)})
    print(f"friction: E end / E0 {E1[-1] / E1[0]:.4f}, L_z {L1[-1][:, 2]}, largest rise {np.diff(E1).max():.3e}, momentum {np.abs(p1).max():.2e}, "
          f"angular momentum change {np.abs(J1 - J1[0]).max():.2e}")
    assert gap1 > 2.02
    Lz = L1[-1][:, 2]
    assert (np.abs(Lz) > 1e-3 * Jscale).all() and Lz[0] * Lz[1] > 0          # both spin up, the same way, about z
    assert np.abs(L1[-1][:, :2]).max() <= 1e-12 * Jscale                      # ... and about z only
    assert np.abs(p1).max() <= 1e-12 * mass * 2.0 and np.abs(p0).max() <= 1e-12 * mass * 2.0
    assert np.abs(J1 - J1[0]).max() <= 1e-12 * Jscale and np.abs(J0 - J0[0]).max() <= 1e-12 * Jscale
    assert (np.diff(E1) <= drift).all()       # never rises step to step beyond the frictionless run's measured drift


def test_graph_replay_and_plain_launches_give_the_same_bits(oracle):
    import torch
    out = []
    for use_graph in (False, True):
        sp, r = _oblique({(1, 1): (0.5, 50.0)}, use_graph, 500)
        torch.cuda.synchronize()
        out.append([t.cpu().numpy().copy() for t in (r.x[:2], r.v, r.q[:2], r.L, r.f[:2], r.tq[:2])])
        sp.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[0][3][:, 2]).min() > 0                       # the contact happened: both spin


# ---- 7. walls, parity --------------------------------------------------------------------------------------------------

S3 = 1.0 / np.sqrt(3.0)


WALL_CASES = {
    # one oblique plane: approaching (pushed harder), and leaving fast enough for the clamp
    "oblique_in": (np.array([[S3, S3, S3, 0.0]]), np.array([0.5, 0.45, 0.4]), np.array([-0.4, -0.3, -0.5, 0.3, -0.2, 0.4]), "live"),
    "oblique_out": (np.array([[S3, S3, S3, 0.0]]), np.array([0.5, 0.45, 0.4]), np.array([4.0, 3.0, 5.0, 0.3, -0.2, 0.4]), "clamped"),
    # three walls in a corner, a random twist
    "corner": (np.array([[1.0, 0, 0, 0.0], [0, 1.0, 0, 0.0], [0, 0, 1.0, 0.0]]), np.array([0.8, 0.9, 0.7]),
               np.array([0.35, -0.6, -0.25, 0.5, 0.8, -0.7]), "live"),
}
WALL_MU, WALL_GT = np.array([0.5, 0.1, 0.6]), np.array([200.0, 400.0, 100.0])
_WALL_KN, _WALL_EXPO, _WALL_GAM = np.array([1000.0, 800.0, 1200.0]), np.array([1.25, 1.0, 2.0]), np.array([400.0, 250.0, 600.0])
_wall_refs = {}


def _wall_reference(name, rmax):
    """(with friction, damped only, elastic) of a wall case from the numpy references: computed once, shared."""
    import damp_ref as D
    import friction_ref as F
    import wall_ref as W
    from shpair import shapes
    if name not in _wall_refs:
        planes, x0, tw0, _ = WALL_CASES[name]
        nw = len(planes)
        sh = [(6, shapes.random_shape(6, 3, amp=0.1), rmax)]
        a = (sh, 16, x0[None, :], np.array([[0.5, 0.5, -0.5, 0.5]]), np.zeros(1, np.int32))
        kn, expo, gam = _WALL_KN[:nw], _WALL_EXPO[:nw], _WALL_GAM[:nw]
        _wall_refs[name] = (F.wall_forces_friction(*a, tw0[None, :], planes, kn, expo, gam, WALL_MU[:nw], WALL_GT[:nw]),
                            D.wall_forces_damped(*a, tw0[None, :], planes, kn, expo, gam), W.wall_forces(*a, planes, kn, expo))
    return _wall_refs[name]


@pytest.mark.parametrize("name", list(WALL_CASES))
def test_wall_pass_with_friction_matches_the_reference(oracle, name):
    from shpair import shapes
    from shpair.capi import ShPairError
    planes, x0, tw0, kind = WALL_CASES[name]
    shp = [(6, shapes.random_shape(6, 3, amp=0.1))]
    nw = len(planes)
    kn, expo, gam, mu, gt = _WALL_KN[:nw], _WALL_EXPO[:nw], _WALL_GAM[:nw], WALL_MU[:nw], WALL_GT[:nw]
    x, quat, tw = x0[None, :], np.array([[0.5, 0.5, -0.5, 0.5]]), tw0[None, :]
    sp = _wall_ctx(shp, 16)
    sp.set_walls(planes, kn, expo)
    sp.wall_damping(gam)
    damped = _wall_pass(sp, x, quat, tw, nw)
    sp.wall_friction(np.zeros(nw), gt)                     # no wall has friction: today's damped pass, the same bits
    assert all(np.array_equal(a, b) for a, b in zip(damped, _wall_pass(sp, x, quat, tw, nw)))
    sp.wall_friction(mu, gt)
    f, tq, out = _wall_pass(sp, x, quat, tw, nw)
    nc = sp.wall_stats()
    sp.wall_damping(np.zeros(nw))                          # friction alone refuses the twist-less call too
    with pytest.raises(ShPairError, match="wall friction needs the twist form") as e:
        _wall_pass(sp, x, quat, tw, nw, damped=False)
    assert e.value.code == -1
    ref, nofr, elastic = _wall_reference(name, sp.rmax(0))
    sp.close()
    scale = max(np.abs(elastic["f"]).max(), np.abs(ref["f"]).max())
    tscale = max(scale, np.abs(elastic["torque"]).max(), np.abs(ref["torque"]).max())
    ef, et = np.abs(f - ref["f"]).max() / scale, np.abs(tq - ref["torque"]).max() / tscale
    eo = np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() / scale
    ee = np.abs(out[:, 0] - ref["wall_out"][:, 0]).max() / np.abs(ref["wall_out"][:, 0]).max()
    print(f"{name}: contacts {nc}, N / |F_t| / capped {[(round(c[4], 2), round(float(np.linalg.norm(c[5])), 3), c[7]) for c in ref['contacts']]}, "
          f"max|F| {scale:.4g}, rel err f {ef:.1e} torque {et:.1e} wall force {eo:.1e} wall energy {ee:.1e}")
    assert nc == len(ref["contacts"]) == nw and scale > 0
    assert ef <= TOL and et <= TOL and eo <= TOL and ee <= TOL
    assert np.abs(f.sum(axis=0) + out[:, 1:].sum(axis=0)).max() <= TOL * scale   # the force on the wall is -F_i
    if kind == "clamped":
        assert all(c[3] == 0.0 for c in ref["contacts"]) and not f.any() and not tq.any()    # a clamped contact adds no friction
        return
    assert all(c[3] > 0 and np.linalg.norm(c[5]) > 0.02 * scale for c in ref["contacts"])    # live contacts, friction not small
    # the friction force of the GPU result, wall by wall: what the wall's row of wall_out gains over today's damped pass
    # (p_tot is the same in both), with no component along that wall's normal
    for w in range(nw):
        dF = -(out[w, 1:] - damped[2][w, 1:])
        assert np.linalg.norm(dF) > 0.02 * scale and abs(dF @ planes[w, :3]) <= 1e-12 * np.linalg.norm(dF)
    assert np.abs((f[0] - damped[0][0]) + (out[:, 1:] - damped[2][:, 1:]).sum(axis=0)).max() <= TOL * scale
    for c in ref["contacts"]:
        assert abs(c[5] @ planes[c[1], :3]) <= 1e-12 * np.linalg.norm(c[5])


def test_wall_cases_cover_both_branches_of_kappa(oracle):
    """A condition on the inputs, read from the references alone."""
    from shpair import ShPair, shapes
    sp = _wall_ctx([(6, shapes.random_shape(6, 3, amp=0.1))], 16)
    rmax = sp.rmax(0)
    sp.close()
    branches = {bool(c[7]) for name in WALL_CASES for c in _wall_reference(name, rmax)[0]["contacts"] if c[3] > 0}
    assert branches == {True, False}


# ---- 8. walls, run loop ------------------------------------------------------------------------------------------------

def test_sphere_sliding_on_the_floor_slows_down_and_starts_to_roll(oracle):
    import torch
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 16, kn=1e4, expo=1.25, rmax=[1.01])
    # centre near the height at which the floor carries the weight: it settles under gamma_w while it slides along +x
    r = DeviceRun(sp, np.array([[0.0, 0.0, 0.9945]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-5, -5, 0), (50, 5, 10),
                  (0, 0, 0), 0.5, dt=1e-4, gravity=(0.0, 0.0, -9.81), walls=([[0, 0, 1, 0.0]], 1e4, 1.25), wall_damping=1000.0,
                  wall_friction=(0.3, 200.0))
    r.v[:] = dev(np.array([[1.0, 0.0, 0.0]]))
    vx, Ly = [1.0], [0.0]
    for _ in range(30):
        r.run_native(50, use_graph=True)
        vx.append(float(r.v[0, 0].item()))
        Ly.append(float(r.L[0, 1].item()))
    sp.synchronize()
    vx, Ly = np.array(vx), np.array(Ly)
    print(f"v_x {vx[0]:.4f} -> {vx[-1]:.4f}, L_y 0 -> {Ly[-1]:.4f}, contacts {sp.wall_stats()}")
    assert (np.diff(vx) <= 0).all() and vx[-1] < vx[0] - 1e-3            # the horizontal speed never increases
    # rolling along +x on a floor below: omega = (0, +w, 0) (v = omega x r, r = +z from the contact point)
    assert (np.diff(Ly) >= 0).all() and Ly[-1] > 1e-3
    assert abs(float(r.L[0, 0].item())) <= 1e-12 and abs(float(r.L[0, 2].item())) <= 1e-12
    sp.close()


# ---- 9. argument checks ------------------------------------------------------------------------------------------------

def test_argument_checks(oracle):
    from shpair import mrank
    from shpair.capi import ShPairError, HaloArrays, HaloRunParams
    case = bed_case(oracle, 12, 2)
    K, E = coeff_tables(2, 1000.0, 1.25)
    sp = ctx(case, K, E)
    for a, b, mu, gt in ((1, 1, -1.0, 1.0), (1, 1, 1.0, -1.0), (1, 2, np.nan, 1.0), (1, 2, 1.0, np.nan), (1, 1, np.inf, 1.0),
                         (1, 1, 1.0, np.inf), (0, 1, 1.0, 1.0), (1, 3, 1.0, 1.0)):
        with pytest.raises(ShPairError) as e:
            sp.pair_friction(a, b, mu, gt)
        assert e.value.code == -1
    sp.set_walls([[0, 0, 1, -10.0]], 1000.0, 1.25)
    for mu, gt in (([1.0, 2.0], [1.0, 2.0]), ([-1.0], [1.0]), ([1.0], [-1.0]), ([np.nan], [1.0]), ([1.0], [np.inf])):
        with pytest.raises(ShPairError) as e:
            sp.wall_friction(mu, gt)
        assert e.value.code == -1
    # the dissipation pass ahead of any compute
    sp.pair_friction(1, 2, 0.5, 10.0)
    n = case["n"]
    x, ty, sh, tw = dev(case["bed"]["x"]), dev(case["bed"]["type"].astype(np.int32)), dev(case["bed"]["shtype"].astype(np.int32)), dev(np.zeros((n, 6)))
    f, tq = dev(np.zeros((n, 3))), dev(np.zeros((n, 3)))
    with pytest.raises(ShPairError, match="no compute has run") as e:
        sp.pair_dissipation_device(n, 0, x.data_ptr(), ty.data_ptr(), sh.data_ptr(), tw.data_ptr(), f.data_ptr(), tq.data_ptr())
    assert e.value.code == -1
    # the damping call refuses while a pair has friction, and names the new call
    with pytest.raises(ShPairError, match="shstep_pair_dissipation_device") as e:
        sp.pair_damping_device(n, 0, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), f.data_ptr(), tq.data_ptr())
    assert e.value.code == -1
    # the twist-less wall call refuses while a wall has friction
    sp.wall_friction(0.5, 10.0)
    q, m = dev(case["bed"]["quat"]), dev(np.ones(n, np.int32))
    with pytest.raises(ShPairError, match="wall friction needs the twist form") as e:
        sp.wall_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    assert e.value.code == -1
    # the loop over several ranks refuses without halo_twists while a coefficient is set, pair or wall
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    for pair_mu, wall_mu in ((0.5, 0.0), (0.0, 0.5)):
        sp.pair_friction(1, 2, pair_mu, 10.0)
        sp.wall_friction(wall_mu, 10.0)
        with pytest.raises(ShPairError, match="contact friction is not supported") as e:
            halo.run(HaloArrays(), HaloRunParams(), 1, 0)
        assert e.value.code == -1
    halo.close()
    sp.close()
