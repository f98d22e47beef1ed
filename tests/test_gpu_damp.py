"""GPU tests of the volume-rate contact damping of docs/SPEC.md §2.10 (csrc/dissipation_kernels.hpp, the DAMP instance of
csrc/wall_kernels.hpp, through the C ABI of include/shstep.h) against tests/damp_ref.py fed by the ORACLE's per-pair
integrals: forces and torques at SPEC §4's gate (1e-9 of the largest force), the invariants the SPEC states, the
deterministic mode, the run loop and the walls.  The kernels do not depend on the order: L = 4, n_q = 8 unless stated."""
import os
import sys

import numpy as np
import pytest

import dissipation_common
from common import coeff_tables, oracle_compute
from dissipation_common import NQ, dev, bed_case, motion, ctx, _rigid_motion, periodic_run, _total_energy, _wall_ctx, _wall_pass

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-9
GAMMA = {(1, 1): 300.0, (1, 2): 900.0, (2, 2): 1800.0}


def gamma_table(ntypes, gam):
    G = np.zeros((ntypes + 1, ntypes + 1))
    for (a, b), g in gam.items():
        if a <= ntypes and b <= ntypes:
            G[a, b] = G[b, a] = g
    return G


def gpu_forces(sp, case, v, L, nlocal=None, newton=True):
    """compute + twists + damping pass (the entry point without shape indices) on fresh arrays: f, torque [n][3], twist [n][6]."""
    return dissipation_common.gpu_forces(sp, case, v, L, nlocal, newton, old_call=True)


def set_gamma(sp, gam, ntypes=2):
    for (a, b), g in gam.items():
        if a <= ntypes and b <= ntypes:
            sp.pair_damping(a, b, g)


def reference(oracle, case, K, E, G, v, L, nlocal=None, newton=True):
    import damp_ref as D
    b, n = case["bed"], case["n"]
    nlocal = n if nlocal is None else nlocal
    o = oracle_compute(oracle, case, NQ, K, E, nlocal=nlocal, newton_pair=newton, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], case["offsets"], case["jlist"])
    tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
    f, tq, det = D.pair_damping(o["pairs"], pi, pj, b["x"], tw, b["type"], K, E, G, nlocal, newton_pair=newton, details=True)
    return dict(elastic_f=o["f"], elastic_t=o["torque"], f=f, torque=tq, twist=tw, det=det)


# ---- 1. against the reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,seed,expo,nlocal,newton", [(60, 1, 1.25, None, True), (60, 1, 1.0, None, True), (12, 2, 1.25, None, True),
                                                       (60, 3, 1.25, 40, False), (60, 3, 1.25, 40, True),
                                                       # exponents whose V^(m-1) is pow() in the pass (m - 1 = 0.75, 1.5, 0.3)
                                                       (60, 1, 1.75, None, True), (60, 1, 2.5, None, True), (60, 1, 1.3, None, True)])
def test_damping_wrench_matches_the_reference_on_oracle_integrals(oracle, n, seed, expo, nlocal, newton):
    case = bed_case(oracle, n, seed, nlocal)
    npairs = case["jlist"].size
    assert npairs % 64 != 0 and ((npairs < 64) == (n == 12)) and npairs > 10
    K, E = coeff_tables(2, lambda i, j: 1000.0 + 100.0 * (i + j), expo)
    G = gamma_table(2, GAMMA)
    v, L = motion(case, 7 + seed)
    sp = ctx(case, K, E)
    for s in range(2):
        assert np.abs(sp.body(s)[1]).max() > 1e-3   # centres of mass off the SH origin: w != v
    f0, t0, _ = gpu_forces(sp, case, v, L, nlocal, newton)   # every gamma = 0: the pass launches nothing
    set_gamma(sp, GAMMA)
    f1, t1, tw = gpu_forces(sp, case, v, L, nlocal, newton)
    sp.close()
    ref = reference(oracle, case, K, E, G, v, L, nlocal, newton)
    ok = ~np.isnan(ref["det"][:, 0])
    clamped = ref["det"][ok, 0] == -ref["det"][ok, 2]
    scale = np.abs(ref["elastic_f"] + ref["f"]).max()
    tscale = max(scale, np.abs(ref["elastic_t"] + ref["torque"]).max())
    ef, et = np.abs((f1 - f0) - ref["f"]).max() / scale, np.abs((t1 - t0) - ref["torque"]).max() / tscale
    e0 = np.abs(f0 - ref["elastic_f"]).max() / scale
    etw = np.abs(tw - ref["twist"]).max() / np.abs(ref["twist"]).max()
    print(f"n={n} m={expo} nlocal={nlocal} newton={newton}: {npairs} slots, {ok.sum()} damped ({clamped.sum()} clamped), max|F| {scale:.4g}, "
          f"max|dF| {np.abs(ref['f']).max():.4g}, rel err dF {ef:.1e} dtau {et:.1e} elastic {e0:.1e} twist {etw:.1e}")
    assert scale > 0 and np.abs(ref["f"]).max() > 0.05 * scale     # the damping part is not a rounding-size effect
    assert clamped.any() and (~clamped).any()                        # both branches of max(0, p + gamma Vdot)
    if expo not in (1.0, 1.25):
        assert clamped.sum() >= 5 and (~clamped).sum() >= 5          # counted from the reference alone
    assert etw <= 1e-12
    assert e0 <= TOL and ef <= TOL and et <= TOL
    if nlocal is not None and not newton:
        assert not f1[nlocal:].any() and not t1[nlocal:].any()
    if nlocal is not None and newton:
        assert np.abs(f1[nlocal:] - f0[nlocal:]).max() > 0           # ghost j rows got their share


# ---- 2. invariants on the GPU result -------------------------------------------------------------------------------

def test_gpu_damping_conserves_momentum_and_angular_momentum(oracle):
    case = bed_case(oracle, 60, 1)
    K, E = coeff_tables(2, 1000.0, 1.25)
    v, L = motion(case, 11)
    sp = ctx(case, K, E)
    f0, t0, _ = gpu_forces(sp, case, v, L)
    set_gamma(sp, GAMMA)
    f1, t1, _ = gpu_forces(sp, case, v, L)
    sp.close()
    df, dt = f1 - f0, t1 - t0
    x = case["bed"]["x"]
    tot = np.abs(df).sum()
    assert tot > 0
    print(f"net damping force {np.abs(df.sum(axis=0)).max():.2e}, net moment {np.abs((np.cross(x, df) + dt).sum(axis=0)).max():.2e}, sum|F| {tot:.4g}")
    assert np.abs(df.sum(axis=0)).max() <= 1e-12 * tot
    assert np.abs((np.cross(x, df) + dt).sum(axis=0)).max() <= 1e-12 * tot


def test_rigid_rotation_of_a_bed_is_not_damped(oracle):
    case = bed_case(oracle, 60, 1)
    K, E = coeff_tables(2, 1000.0, 1.25)
    v, L = _rigid_motion(case, np.array([0.3, -0.2, 0.5]), np.array([0.4, 0.7, -0.5]))
    sp = ctx(case, K, E)
    f0, t0, _ = gpu_forces(sp, case, v, L)
    set_gamma(sp, GAMMA)
    f1, t1, _ = gpu_forces(sp, case, v, L)
    sp.close()
    fel = np.abs(f0).max()
    print(f"rigid rotation: max|dF| {np.abs(f1 - f0).max():.2e}, max|dtau| {np.abs(t1 - t0).max():.2e}, max|F_elastic| {fel:.4g}")
    assert fel > 0 and np.abs(v).max() > 1
    assert np.abs(f1 - f0).max() <= 1e-12 * fel and np.abs(t1 - t0).max() <= 1e-12 * fel


def _periodic_run(oracle, gam, v, L=None, det=1):
    return periodic_run(v, L, det, pair_damping=gam)


def test_translation_of_a_periodic_bed_is_not_damped_and_its_ghosts_carry_their_owners_twists(oracle):
    v0 = np.array([1.5, -0.7, 0.9])
    sp0, r0 = _periodic_run(oracle, None, v0)
    f0, t0 = r0.f[:r0.n].cpu().numpy(), r0.tq[:r0.n].cpu().numpy()
    sp0.close()
    sp, r = _periodic_run(oracle, GAMMA, v0)
    n, ng = r.n, r.nghost
    f1, t1 = r.f[:n].cpu().numpy(), r.tq[:n].cpu().numpy()
    tw = r.twist.cpu().numpy()
    owner_of_ghost_pairs = r.npairs
    fel = np.abs(f0).max()
    print(f"periodic translation: {n} owned, {ng} ghosts, {owner_of_ghost_pairs} slots, max|dF| {np.abs(f1 - f0).max():.2e}, max|F_elastic| {fel:.4g}")
    assert ng > 0 and fel > 0
    assert np.array_equal(tw[n:n + ng, :3], np.broadcast_to(v0, (ng, 3))) and not tw[:n + ng, 3:].any()
    assert np.abs(f1 - f0).max() <= 1e-12 * fel and np.abs(t1 - t0).max() <= 1e-12 * fel
    # ... and with a random motion the ghost rows' shares come home: momentum is conserved over the periodic bed
    rng = np.random.default_rng(2)
    r.v[:] = dev(rng.normal(size=(n, 3)))
    r.L[:] = dev(0.3 * rng.normal(size=(n, 3)))
    r.force()
    import torch
    torch.cuda.synchronize()
    df = r.f[:n].cpu().numpy() - f0
    tw = r.twist.cpu().numpy()
    offs, jl = sp.copy_neighbors(n, r.npairs)
    ghost_j = jl[jl >= n]
    assert ghost_j.size > 0 and np.abs(tw[ghost_j]).min(axis=1).max() > 0    # pairs across the faces, with live twists
    print(f"periodic random motion: max|dF| {np.abs(df).max():.4g}, net {np.abs(df.sum(axis=0)).max():.2e}")
    assert np.abs(df).max() > 0.05 * fel and np.abs(df.sum(axis=0)).max() <= 1e-12 * np.abs(df).sum()
    sp.close()


# ---- 3. deterministic mode -----------------------------------------------------------------------------------------

def test_deterministic_mode_is_bitwise_reproducible_and_agrees_with_the_atomics(oracle):
    case = bed_case(oracle, 60, 1)
    K, E = coeff_tables(2, 1000.0, 1.25)
    v, L = motion(case, 8)
    runs = []
    for det in (1, 1, 0):
        sp = ctx(case, K, E, det=det)
        set_gamma(sp, GAMMA)
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
    # untouched slots wrote zeros: a deterministic run with every gamma = 0 differs by exactly the damping part
    sp = ctx(case, K, E, det=1)
    f0, _, _ = gpu_forces(sp, case, v, L)
    sp.close()
    assert np.abs(runs[0][0] - f0).max() > 0.05 * scale


# ---- 4. the run loop ------------------------------------------------------------------------------------------------

def _two_spheres(gamma, periodic, det=1):
    """Two unit spheres (mass 4.19) head-on at relative speed 2, kn = 1e4, m = 1.25, dt = 2e-4; periodic: they meet across
    the x face of the box."""
    from shpair import ShPair, shapes
    from shpair.run import DeviceRun
    sp = ShPair(0)
    sp.settings(NQ)
    sp.set_ntypes(1, 1)
    sp.set_shape(0, 0, shapes.sphere(1.0), 1.01)
    sp.coeff(1, 1, 1e4, 1.25)
    if det:
        sp.set_option("deterministic", 1)
    if periodic:
        x = np.array([[0.99, 4.0, 4.0], [7.97, 4.0, 4.0]])      # 0.99 + (9 - 7.97) = 2.02 apart across the face
        v = np.array([[-1.0, 0, 0], [1.0, 0, 0]])
        lo, hi, per = (0, 0, 0), (9, 8, 8), (1, 0, 0)
    else:
        x = np.array([[2.99, 4.0, 4.0], [5.01, 4.0, 4.0]])
        v = np.array([[1.0, 0, 0], [-1.0, 0, 0]])
        lo, hi, per = (0, 0, 0), (8, 8, 8), (0, 0, 0)
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]] * 2), np.zeros(2, np.int32), lo, hi, per, 0.3, dt=2e-4,
                  pair_damping={(1, 1): gamma})
    r.v[:] = dev(v)
    r.force()
    return sp, r


def _collide(gamma, nsteps=700):
    sp, r = _two_spheres(gamma, periodic=False)
    mass = sp.body(0)[0]
    E, p = [_total_energy(sp, r)], []
    for _ in range(nsteps):
        r.run_native(1)
        E.append(_total_energy(sp, r))
        p.append(mass * r.v.sum(dim=0).cpu().numpy())
    v = r.v.cpu().numpy()
    gap = float((r.x[1, 0] - r.x[0, 0]).item())
    sp.close()
    return np.array(E), np.array(p), v, gap, mass


def test_head_on_collision_in_the_run_loop_dissipates_energy_and_conserves_momentum(oracle):
    E0, p0, v0, gap0, mass = _collide(0.0)
    drift = np.abs(E0 - E0[0]).max()
    print(f"gamma = 0: E0 {E0[0]:.6f}, drift {drift:.3e}, separation speed {v0[1, 0] - v0[0, 0]:.6f}, gap {gap0:.3f}")
    assert gap0 > 2.02 and E0.max() - E0.min() > 0     # they met, and parted again
    # The undamped loop conserves energy.  While the spheres overlap the books are kept by two quadratures that agree
    # only to the sharp rule's error — the force integrates S_n, the energy V: 2.7e-2 of the stored energy at n_q = 8
    # (SPEC §2.8's table) — so that is the bound during the contact; once they have parted only the kinetic energy is
    # left and what remains is that error over the closed path and the leapfrog's (dt = 2e-4, ~350 steps in contact).
    assert drift <= 2.7e-2 * E0[0] and abs(E0[-1] - E0[0]) <= 1e-2 * E0[0]
    assert abs((v0[1, 0] - v0[0, 0]) - 2.0) <= 1e-2     # restitution 1 without damping
    E1, p1, v1, gap1, _ = _collide(1000.0)
    sep = v1[1, 0] - v1[0, 0]
    print(f"gamma = 1000: E end / E0 {E1[-1] / E1[0]:.4f}, separation speed {sep:.6f}, largest step-to-step rise {np.diff(E1).max():.3e}, "
          f"momentum {np.abs(p1).max():.2e}")
    assert gap1 > 2.02
    assert (np.diff(E1) <= drift).all()                 # non-increasing step by step beyond the measured drift
    # ... and really dissipated: what a 1-D integration of SPEC §2.10 with the exact lens volume loses (8.3 % of E0 at
    # gamma = 1000; tests/damp_ref.py).  The loss is quadratic in S_n, whose sharp-rule error at n_q = 8 is 2.7e-2 (SPEC
    # §2.8's table), so twice that of the loss, plus what the undamped run itself is off by from end to end.
    import damp_ref as D
    sep_1d, ke_1d = D.sphere_collision_1d(1000.0, 1e4, 1.25)
    loss, loss_1d = E1[0] - E1[-1], (1.0 - ke_1d) * E1[0]
    print(f"energy lost {loss:.5f}, 1-D model {loss_1d:.5f}; separation speed 1-D {sep_1d:.6f}")
    assert loss_1d > 0.05 * E1[0]
    assert abs(loss - loss_1d) <= 5.4e-2 * loss_1d + abs(E0[-1] - E0[0])
    assert 0 < sep < 2.0 - 1e-2                         # slower apart than together
    assert np.abs(p1).max() <= 1e-12 * mass * 2.0 and np.abs(p0).max() <= 1e-12 * mass * 2.0


@pytest.mark.parametrize("periodic", [False, True])
def test_graph_replay_and_plain_launches_give_the_same_bits(oracle, periodic):
    import torch
    out = []
    for use_graph in (False, True):
        sp, r = _two_spheres(1000.0, periodic)
        r.run_native(500, use_graph=use_graph)
        torch.cuda.synchronize()
        out.append([t.cpu().numpy().copy() for t in (r.x[:2], r.v, r.q[:2], r.L, r.f[:2], r.tq[:2])] + [r.nghost])
        sp.close()
    for a, b in zip(out[0][:-1], out[1][:-1]):
        assert np.array_equal(a, b)
    v = out[0][1]
    sep = abs(v[1, 0] - v[0, 0])
    print(f"periodic={periodic}: ghosts {out[0][-1]}, separation speed {sep:.6f}, net momentum {np.abs(v.sum(axis=0)).max():.2e}")
    assert (out[0][-1] > 0) == periodic
    assert np.sign(v[1, 0]) == (-1.0 if periodic else 1.0)       # they bounced
    assert 0.5 < sep < 2.0 - 1e-2                                # ... with a restitution below 1
    assert np.abs(v.sum(axis=0)).max() <= 1e-12 * 2.0


# ---- 5. walls --------------------------------------------------------------------------------------------------------

S3 = 1.0 / np.sqrt(3.0)


WALL_CASES = {
    # one oblique plane: approaching (pushed harder), and leaving fast enough for the clamp
    "oblique_in": (np.array([[S3, S3, S3, 0.0]]), np.array([0.5, 0.45, 0.4]), np.array([-0.4, -0.3, -0.5, 0.3, -0.2, 0.4]), "damped"),
    "oblique_out": (np.array([[S3, S3, S3, 0.0]]), np.array([0.5, 0.45, 0.4]), np.array([4.0, 3.0, 5.0, 0.3, -0.2, 0.4]), "clamped"),
    # three walls in a corner, a random twist
    "corner": (np.array([[1.0, 0, 0, 0.0], [0, 1.0, 0, 0.0], [0, 0, 1.0, 0.0]]), np.array([0.8, 0.9, 0.7]),
               np.array([0.35, -0.6, -0.25, 0.5, 0.8, -0.7]), "damped"),
}


@pytest.mark.parametrize("name", list(WALL_CASES))
def test_damped_wall_pass_matches_the_reference(oracle, name):
    import damp_ref as D
    import wall_ref as W
    from shpair import shapes
    planes, x0, tw0, kind = WALL_CASES[name]
    shp = [(6, shapes.random_shape(6, 3, amp=0.1))]
    nw = len(planes)
    kn, expo, gam = np.array([1000.0, 800.0, 1200.0])[:nw], np.array([1.25, 1.0, 2.0])[:nw], np.array([400.0, 250.0, 600.0])[:nw]
    x, quat, tw = x0[None, :], np.array([[0.5, 0.5, -0.5, 0.5]]), tw0[None, :]
    sp = _wall_ctx(shp, 16)
    sp.set_walls(planes, kn, expo)
    el = _wall_pass(sp, x, quat, tw, nw, damped=False)
    same = _wall_pass(sp, x, quat, tw, nw, damped=True)        # every gamma_w = 0: the same kernel, the same bits
    assert all(np.array_equal(a, b) for a, b in zip(el, same))
    sp.wall_damping(gam)
    f, tq, out = _wall_pass(sp, x, quat, tw, nw)
    from shpair.capi import ShPairError
    with pytest.raises(ShPairError, match="wall damping needs the twist form") as e:
        _wall_pass(sp, x, quat, tw, nw, damped=False)
    assert e.value.code == -1
    ref = D.wall_forces_damped([(6, shp[0][1], sp.rmax(0))], 16, x, quat, np.zeros(1, np.int32), tw, planes, kn, expo, gam)
    elastic = W.wall_forces([(6, shp[0][1], sp.rmax(0))], 16, x, quat, np.zeros(1, np.int32), planes, kn, expo)
    nc = sp.wall_stats()
    sp.close()
    scale = max(np.abs(elastic["f"]).max(), np.abs(ref["f"]).max())
    tscale = max(scale, np.abs(elastic["torque"]).max())
    ef, et = np.abs(f - ref["f"]).max() / scale, np.abs(tq - ref["torque"]).max() / tscale
    eo = np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() / scale
    ee = np.abs(out[:, 0] - ref["wall_out"][:, 0]).max() / np.abs(ref["wall_out"][:, 0]).max()
    print(f"{name}: contacts {nc}, p / p_tot {[(round(c[2], 1), round(c[3], 1)) for c in ref['contacts']]}, max|F| {scale:.4g}, "
          f"rel err f {ef:.1e} torque {et:.1e} wall force {eo:.1e} wall energy {ee:.1e}")
    assert nc == len(ref["contacts"]) == nw and scale > 0
    if kind == "clamped":
        assert all(c[3] == 0.0 for c in ref["contacts"]) and not f.any() and not tq.any()    # the wall does not pull
    else:
        assert all(c[3] > 0 and abs(c[3] - c[2]) > 0.02 * c[2] for c in ref["contacts"])
    assert np.abs(out[:, 0] - el[2][:, 0]).max() <= 1e-14 * np.abs(el[2][:, 0]).max()     # E_w stays kn V^m
    assert ef <= TOL and et <= TOL and eo <= TOL and ee <= TOL
    assert np.abs(f.sum(axis=0) + out[:, 1:].sum(axis=0)).max() <= TOL * scale   # the force on the wall is -F_i


def test_dropped_sphere_rebounds_lower_on_each_of_three_bounces(oracle):
    """The unit sphere of tests/test_gpu_wall.py's bounce test (kn = 1e4, m = 1.25, g = 9.81, centre 1.5 above the floor, dt = 1e-4,
    n_q = 16), now with gamma_w = 1000, in the run loop with graph replay: each rebound peaks strictly below the one before."""
    import torch
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 16, kn=1e4, expo=1.25, rmax=[1.01])
    r = DeviceRun(sp, np.array([[0.0, 0.0, 1.5]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-5, -5, 0), (5, 5, 10),
                  (0, 0, 0), 0.5, dt=1e-4, gravity=(0.0, 0.0, -9.81), walls=([[0, 0, 1, 0.0]], 1e4, 1.25), wall_damping=1000.0)
    zs = []
    for _ in range(200):      # 2 s, sampled every 100 steps (0.01 s: the centre moves 1.2e-4 in the 0.005 s either side of a peak)
        r.run_native(100, use_graph=True)
        zs.append(r.x[0, 2].clone())
    z = torch.stack(zs).cpu().numpy()
    sp.synchronize()
    contact = z < 1.0
    starts = [k for k in range(1, len(z)) if contact[k] and not contact[k - 1]]
    peaks = [z[a:b].max() for a, b in zip(starts, starts[1:] + [len(z)])]
    print(f"contacts begin at samples {starts}, rebound peaks {[round(float(p), 4) for p in peaks]}")
    assert len(starts) >= 4 or (len(starts) == 3 and np.argmax(z[starts[2]:]) < len(z) - starts[2] - 1)
    assert peaks[0] < 1.5 - 1e-3 and peaks[1] < peaks[0] - 1e-3 and peaks[2] < peaks[1] - 1e-3
    assert peaks[2] > 1.0     # still bouncing: the drag did not simply stop it
    sp.close()


# ---- 6. argument checks ---------------------------------------------------------------------------------------------

def test_argument_checks(oracle):
    import ctypes as C
    from shpair import mrank
    from shpair.capi import ShPairError, HaloArrays, HaloRunParams
    case = bed_case(oracle, 12, 2)
    K, E = coeff_tables(2, 1000.0, 1.25)
    sp = ctx(case, K, E)
    for a, b, g in ((1, 1, -1.0), (1, 2, np.nan), (1, 1, np.inf), (0, 1, 1.0), (1, 3, 1.0)):
        with pytest.raises(ShPairError) as e:
            sp.pair_damping(a, b, g)
        assert e.value.code == -1
    sp.set_walls([[0, 0, 1, -10.0]], 1000.0, 1.25)
    for g in ([1.0, 2.0], [-1.0], [np.nan]):
        with pytest.raises(ShPairError) as e:
            sp.wall_damping(g)
        assert e.value.code == -1
    # the damping pass ahead of any compute
    sp.pair_damping(1, 2, 10.0)
    n = case["n"]
    x, ty, tw = dev(case["bed"]["x"]), dev(case["bed"]["type"].astype(np.int32)), dev(np.zeros((n, 6)))
    f, tq = dev(np.zeros((n, 3))), dev(np.zeros((n, 3)))
    with pytest.raises(ShPairError, match="no compute has run") as e:
        sp.pair_damping_device(n, 0, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), f.data_ptr(), tq.data_ptr())
    assert e.value.code == -1
    # the loop over several ranks refuses while a coefficient is set, pair or wall
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    for pair_g, wall_g in ((10.0, 0.0), (0.0, 5.0)):
        sp.pair_damping(1, 2, pair_g)
        sp.wall_damping(wall_g)
        with pytest.raises(ShPairError, match="contact damping is not supported") as e:
            halo.run(HaloArrays(), HaloRunParams(), 1, 0)
        assert e.value.code == -1
    halo.close()
    sp.close()
