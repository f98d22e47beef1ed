"""GPU tests of the translating planar walls of docs/SPEC.md §2.12 (the MOVE instances and the advance kernel of
csrc/wall_kernels.hpp, through the C ABI of include/shstep.h) against tests/wall_move_ref.py: parity of the wall pass,
Galilean invariance at pass level, nothing changes while nothing moves, the advance, the three step loops, a piston and a
belt against their mirror experiments on fixed walls, a wall that runs over a particle, two ranks, argument checks.

The wall velocities of the parity test were chosen on the CPU, with the reference alone, so that the conditions the test
asserts on its INPUTS hold at every (L, n_q) it runs: the live contacts cover both branches of kappa, and one contact
(the corner's third wall) is live with u = 0 and clamped with it."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dissipation_common import dev, _wall_ctx, _wall_pass   # noqa: E402

TOL = 1e-9            # tests/test_gpu_friction.py's
S3 = 1.0 / np.sqrt(3.0)
# per case of test_gpu_friction.WALL_CASES: one velocity per wall, normal and tangential parts of order 1
WALL_VEL = {
    "oblique_in": np.array([[-1.2, -0.3, -0.9]]),
    "oblique_out": np.array([[1.5, 0.8, 1.9]]),
    "corner": np.array([[0.9, -0.7, 0.4], [0.6, -1.1, 0.8], [-0.5, 0.9, -1.2]]),
}
QUAT = np.array([[0.5, 0.5, -0.5, 0.5]])
_refs = {}


def _coefficients(nw):
    import test_gpu_friction as G
    return G._WALL_KN[:nw], G._WALL_EXPO[:nw], G._WALL_GAM[:nw], G.WALL_MU[:nw], G.WALL_GT[:nw]


def _shape(lmax):
    from shpair import shapes
    return shapes.random_shape(lmax, 3, amp=0.1)


def _reference(lmax, nq, name, rmax):
    """(moving, the same walls at rest, the same walls without a coefficient) from tests/wall_move_ref.py: computed once,
    shared."""
    import test_gpu_friction as G
    import wall_move_ref as M
    key = (lmax, nq, name)
    if key not in _refs:
        planes, x0, tw0, _ = G.WALL_CASES[name]
        nw = len(planes)
        a = ([(lmax, _shape(lmax), rmax)], nq, x0[None, :], QUAT, np.zeros(1, np.int32))
        co = (planes, *_coefficients(nw))
        _refs[key] = (M.wall_forces_moving(*a, tw0[None, :], *co, WALL_VEL[name]),
                      M.wall_forces_moving(*a, tw0[None, :], *co, np.zeros((nw, 3))),
                      M.wall_forces_moving(*a, tw0[None, :], planes, co[1], co[2], *np.zeros((3, nw)), WALL_VEL[name]))
    return _refs[key]


# ---- 1. against the reference --------------------------------------------------------------------------------------

CONFIGS = [(6, 16), (4, 10), (4, 1)]      # n_q = 1: two nodes per cap, one live lane or two in a wave


@pytest.mark.parametrize("lmax,nq", CONFIGS)
@pytest.mark.parametrize("name", ["oblique_in", "oblique_out", "corner"])
def test_moving_wall_pass_matches_the_reference(oracle, name, lmax, nq):
    import test_gpu_friction as G
    planes, x0, tw0, _ = G.WALL_CASES[name]
    nw = len(planes)
    kn, expo, gam, mu, gt = _coefficients(nw)
    sp = _wall_ctx([(lmax, _shape(lmax))], nq)
    sp.set_walls(planes, kn, expo)
    sp.wall_damping(gam)
    sp.wall_friction(mu, gt)
    sp.wall_velocity(WALL_VEL[name])
    f, tq, out = _wall_pass(sp, x0[None, :], QUAT, tw0[None, :], nw)
    nc = sp.wall_stats()
    ref, rest, elastic = _reference(lmax, nq, name, sp.rmax(0))
    sp.close()
    scale = max(np.abs(elastic["f"]).max(), np.abs(ref["f"]).max())
    tscale = max(scale, np.abs(elastic["torque"]).max(), np.abs(ref["torque"]).max())
    ef, et = np.abs(f - ref["f"]).max() / scale, np.abs(tq - ref["torque"]).max() / tscale
    eo = np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() / scale
    ee = np.abs(out[:, 0] - ref["wall_out"][:, 0]).max() / np.abs(ref["wall_out"][:, 0]).max()
    print(f"L={lmax} nq={nq} {name}: contacts {nc}, p_tot / |F_t| / capped "
          f"{[(round(c[3], 1), round(float(np.linalg.norm(c[5])), 2), c[7]) for c in ref['contacts']]}, max|F| {scale:.4g}, "
          f"rel err f {ef:.1e} torque {et:.1e} wall force {eo:.1e} wall energy {ee:.1e}")
    assert nc == len(ref["contacts"]) == nw and scale > 0
    assert ef <= TOL and et <= TOL and eo <= TOL and ee <= TOL
    assert np.abs(f.sum(axis=0) + out[:, 1:].sum(axis=0)).max() <= TOL * scale      # the force on the wall is -F_i
    if name != "oblique_out":
        assert np.abs(ref["f"] - rest["f"]).max() > 0.05 * scale                    # the velocity is not a small change


@pytest.mark.parametrize("lmax,nq", CONFIGS)
def test_parity_inputs_cover_both_branches_and_a_clamp_that_only_the_velocity_causes(oracle, lmax, nq):
    """Conditions on the inputs, read from the reference alone."""
    sp = _wall_ctx([(lmax, _shape(lmax))], nq)
    rmax = sp.rmax(0)
    sp.close()
    pairs = [(c1, c0) for name in WALL_VEL for c1, c0 in zip(*[r["contacts"] for r in _reference(lmax, nq, name, rmax)[:2]])]
    assert all(c1[:2] == c0[:2] for c1, c0 in pairs)
    assert {bool(c1[7]) for c1, _ in pairs if c1[3] > 0} == {True, False}          # live contacts: viscous and capped
    assert any(c0[3] > 0 and c1[3] == 0.0 for c1, c0 in pairs)                     # live at rest, clamped by u_w


# ---- 2. Galilean invariance of the pass -------------------------------------------------------------------------------

def test_common_wall_velocity_equals_a_shifted_particle_velocity_on_the_gpu(oracle):
    from test_gpu_wall import box_case
    lmax, nq, n = 4, 8, 40
    case = box_case(100 + lmax, n, 4.0, 1)
    planes = case["planes"][:6]
    from shpair import shapes
    shp = [(lmax, shapes.random_shape(lmax, 900 + lmax, amp=0.1))]
    rng = np.random.default_rng(5)
    tw = np.concatenate([rng.normal(size=(n, 3)), 0.5 * rng.normal(size=(n, 3))], axis=1)
    u = np.array([0.7, -1.1, 0.9])
    res = []
    for moving in (True, False):
        sp = _wall_ctx(shp, nq)
        sp.set_walls(planes, 1000.0, 1.25)
        sp.wall_damping(300.0)
        sp.wall_friction(0.4, 150.0)
        if moving:
            sp.wall_velocity(u)
        twist = tw if moving else tw - np.concatenate([u, np.zeros(3)])
        res.append(_wall_pass(sp, case["x"], case["quat"], twist, 6) + (sp.wall_stats(),))
        if moving:                                    # ... and against the same walls at rest: the velocity matters
            sp.wall_velocity(np.zeros(3))
            rest = _wall_pass(sp, case["x"], case["quat"], tw, 6)
        sp.close()
    (f1, t1, o1, n1), (f0, t0, o0, n0) = res
    scale = np.abs(f0).max()
    print(f"contacts {n1}, max|F| {scale:.4g}, |df| {np.abs(f1 - f0).max() / scale:.1e} |dtau| {np.abs(t1 - t0).max() / scale:.1e} "
          f"|dwall| {np.abs(o1 - o0).max() / scale:.1e}; against walls at rest {np.abs(f1 - rest[0]).max() / scale:.2f}")
    assert n1 == n0 and n1 >= 5 and scale > 0
    assert np.abs(f1 - f0).max() <= 1e-12 * scale and np.abs(t1 - t0).max() <= 1e-12 * scale and np.abs(o1 - o0).max() <= 1e-12 * scale
    assert np.abs(f1 - rest[0]).max() > 0.05 * scale


# ---- 3. nothing changes when nothing moves ------------------------------------------------------------------------------

def _corner_passes(prepare):
    """The elastic, damped and friction passes of the corner case on a context that `prepare` touched after set_walls."""
    import test_gpu_friction as G
    planes, x0, tw0, _ = G.WALL_CASES["corner"]
    kn, expo, gam, mu, gt = _coefficients(3)
    sp = _wall_ctx([(6, _shape(6))], 16)
    sp.set_walls(planes, kn, expo)
    prepare(sp)
    x, tw = x0[None, :], tw0[None, :]
    out = [_wall_pass(sp, x, QUAT, tw, 3, damped=False), _wall_pass(sp, x, QUAT, tw, 3)]   # elastic, by both calls
    sp.wall_damping(gam)
    out.append(_wall_pass(sp, x, QUAT, tw, 3))
    sp.wall_friction(mu, gt)
    out.append(_wall_pass(sp, x, QUAT, tw, 3))
    sp.close()
    return out


def test_zero_velocity_and_zero_coefficients_change_no_bit(oracle):
    never = _corner_passes(lambda sp: None)
    zero = _corner_passes(lambda sp: sp.wall_velocity(np.zeros((3, 3))))
    assert np.abs(never[0][0]).max() > 0 and not np.array_equal(never[2][0], never[0][0]) and not np.array_equal(never[3][0], never[2][0])
    for a, b in zip(never, zero):
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    # u != 0 with every coefficient 0: the elastic pass, by either call
    moving = _corner_passes(lambda sp: sp.wall_velocity(WALL_VEL["corner"]))
    for k in (0, 1):
        assert all(np.array_equal(p, q) for p, q in zip(never[0], moving[k]))
    assert not np.array_equal(never[2][0], moving[2][0])                      # ... and with one it matters


def test_a_belt_leaves_the_planes_where_they_are(oracle):
    planes = np.array([[0.0, 0, 1, 0.25], [S3, S3, S3, -1.5], [1.0, 0, 0, 2.0]])
    from shpair import shapes
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 8)
    sp.set_walls(planes, 1000.0, 1.25)
    assert np.array_equal(sp.get_walls(), planes)
    sp.wall_velocity([[-1.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.0, 3.0, -2.0]])
    for _ in range(10):
        sp.advance_walls_device(1e-2)
    assert np.array_equal(sp.get_walls(), planes)
    sp.close()


# ---- 4. the advance ---------------------------------------------------------------------------------------------------

def test_a_thousand_advances_match_the_accumulation(oracle):
    import wall_move_ref as M
    k, dt = 1000, 1e-4
    planes = np.array([[1.0, 0, 0, 0.05], [0, 1.0, 0, -0.04], [S3, S3, S3, 0.4]])
    vel = np.array([[0.5, 0.3, -0.2], [0.1, -0.4, 0.2], [0.2, 0.3, 0.1]])
    kn, expo = np.array([1000.0, 800.0, 1200.0]), np.array([1.25, 1.0, 2.0])
    x, tw = np.array([[0.8, 0.9, 0.7]]), np.zeros((1, 6))
    sp = _wall_ctx([(6, _shape(6))], 16)
    sp.set_walls(planes, kn, expo)
    sp.wall_velocity(vel)
    st = sp.own_stream()
    for _ in range(k):
        sp.advance_walls_device(dt, stream=st)
    got = sp.get_walls()
    ref = M.advance(planes, vel, dt, k)
    cmax = np.maximum(np.abs(planes[:, 3]), np.abs(ref[:, 3]))
    print(f"c after {k} advances {got[:, 3]}, reference {ref[:, 3]}, difference {np.abs(got[:, 3] - ref[:, 3])}")
    assert (np.abs(ref[:, 3] - planes[:, 3]) > 0.01).all()
    assert (np.abs(got[:, 3] - ref[:, 3]) <= 1e-15 * k * cmax).all()
    assert np.array_equal(got[:, :3], planes[:, :3])                 # the normals: not a bit
    # kn and m: the elastic pass on the advanced planes is the pass of a fresh context given those planes and kn, m
    moved = _wall_pass(sp, x, QUAT, tw, 3, damped=False)
    sp2 = _wall_ctx([(6, _shape(6))], 16)
    sp2.set_walls(got, kn, expo)
    fresh = _wall_pass(sp2, x, QUAT, tw, 3, damped=False)
    sp2.close()
    assert np.abs(moved[2][:, 0]).min() > 0 and all(np.array_equal(a, b) for a, b in zip(moved, fresh))
    # set_walls resets position and velocity
    sp.set_walls(planes, kn, expo)
    assert np.array_equal(sp.get_walls(), planes)
    sp.advance_walls_device(dt, stream=st)
    assert np.array_equal(sp.get_walls(), planes) and not sp.move_walls
    sp.close()


# ---- 5. the three loops -------------------------------------------------------------------------------------------------

def test_run_loops_with_a_rising_floor_and_a_belt_are_bitwise_identical(oracle):
    import torch
    import wall_move_ref as M
    from shpair import shapes
    from shpair.run import DeviceRun
    from test_gpu_wall import _settling_case, _state, box_planes, ctx
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    L, nsteps, dt = 8.4, 50, 5e-4
    x, quat = _settling_case(4, L)
    x[:, 2] -= 0.15
    sht = np.zeros(x.shape[0], np.int32)
    planes = box_planes(L, cut=-10.0)[:6]
    vel = np.zeros((6, 3))
    vel[4] = [0.0, 0.0, 0.2]          # the floor rises
    vel[0] = [0.0, 1.0, 0.0]          # the wall x = 0 is a belt along y

    def go(mode, vel):
        sp = ctx(shp, 10, kn=2000.0, deterministic=1)
        r = DeviceRun(sp, x, quat, sht, (0, 0, 0), (L, L, L), (0, 0, 0), 0.3, dt=dt, gravity=(0.0, 0.0, -9.81), gamma_t=0.2,
                      gamma_r=0.1, walls=(planes, 2000.0, 1.25), wall_damping=50.0, wall_friction=(0.3, 20.0), wall_velocity=vel)
        if mode == "python":
            r.run(nsteps)
        else:
            r.run_native(nsteps, use_graph=(mode == "graph"))
        torch.cuda.synchronize()
        st, nc, pl = _state(r), sp.wall_stats(), sp.get_walls()
        sp.close()
        return st, nc, pl
    ref, nc, pl = go("python", vel)
    assert nc > 0 and np.abs(ref[1]).max() > 0
    for mode in ("plain", "graph"):
        got, nc2, pl2 = go(mode, vel)
        assert nc2 == nc and np.array_equal(pl2, pl), mode
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), mode
    want = M.advance(planes, vel, dt, nsteps)
    cmax = np.maximum(np.abs(planes[:, 3]), np.abs(want[:, 3]))
    print(f"floor at {pl[4, 3]!r}, reference {want[4, 3]!r}")
    assert pl[4, 3] > 0.004 and (np.abs(pl[:, 3] - want[:, 3]) <= 1e-15 * nsteps * cmax).all() and np.array_equal(pl[:, :3], planes[:, :3])
    assert np.array_equal(pl[[0, 1, 2, 3, 5]], planes[[0, 1, 2, 3, 5]])
    still, _, _ = go("graph", None)
    assert not np.array_equal(still[0], ref[0])        # ... and the motion of the walls did act


# ---- 6. a piston ----------------------------------------------------------------------------------------------------------

def _one_sphere(v, wall_velocity, nsteps, **kw):
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 16, kn=1e4, expo=1.25, rmax=[1.01])
    r = DeviceRun(sp, np.array([[0.0, 0.0, 1.5]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-5, -5, 0), (5, 5, 10),
                  (0, 0, 0), 0.5, dt=1e-4, walls=([[0, 0, 1, 0.4]], 1e4, 1.25), wall_velocity=wall_velocity, **kw)
    r.v[:] = dev(np.array([v]))
    r.force()
    r.run_native(nsteps, use_graph=True, check_every=50)
    sp.synchronize()           # no error bit
    out = r.x[0].cpu().numpy(), r.v[0].cpu().numpy(), sp.get_walls()[0, 3]
    sp.close()
    return out


def test_a_piston_launches_a_sphere_as_the_mirror_experiment_says(oracle):
    """A floor 1.1 below a sphere at rest (clear of its bounding sphere, 1.01) rises at 1 and meets it after ~900 steps; the
    mirror experiment — existing behaviour — is the sphere falling at -1 onto the fixed floor, leaving at +u'.  The piston
    run must end at 1 + u' within 1e-9 (issue: accumulated rounding of c over <= 1e4 steps <= 2e-12, against a contact
    depth of ~0.05 that is ~4e-11 relative in the force; the bar leaves 25x), and u' is within 1e-2 of 1 (the bar of the
    drop test of tests/test_gpu_wall.py)."""
    nsteps = 3000
    xm, vm, cm = _one_sphere([0.0, 0.0, -1.0], None, nsteps)
    xp, vp, cp = _one_sphere([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], nsteps)
    print(f"mirror: leaves at {vm[2]:.12f}, height over the floor {xm[2] - cm:.9f}; piston: {vp[2]:.12f}, {xp[2] - cp:.9f} "
          f"(floor at {cp:.6f}); difference {abs(vp[2] - (1.0 + vm[2])):.2e}")
    assert cm == 0.4 and abs(cp - (0.4 + nsteps * 1e-4)) <= 1e-12
    assert xm[2] - cm > 1.01 and xp[2] - cp > 1.01 and vm[2] > 0      # they met and parted
    assert abs(vp[2] - (1.0 + vm[2])) <= 1e-9
    assert abs(vm[2] - 1.0) <= 1e-2
    assert np.abs(vp[:2]).max() <= 1e-12 and np.abs(vm[:2]).max() <= 1e-12      # (rounding of the sphere's tangential S_n)


# ---- 7. a belt --------------------------------------------------------------------------------------------------------------

def _floor_run(v, wall_velocity):
    """The sphere of test_sphere_sliding_on_the_floor_slows_down_and_starts_to_roll (tests/test_gpu_friction.py), 30 samples
    of 50 steps.  The forces of the start are computed again once v is set, so that the run with a belt and the run on a
    fixed floor start from mirrored states (friction acts in the first half kick of both)."""
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 16, kn=1e4, expo=1.25, rmax=[1.01])
    r = DeviceRun(sp, np.array([[0.0, 0.0, 0.9945]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-5, -5, 0), (50, 5, 10),
                  (0, 0, 0), 0.5, dt=1e-4, gravity=(0.0, 0.0, -9.81), walls=([[0, 0, 1, 0.0]], 1e4, 1.25), wall_damping=1000.0,
                  wall_friction=(0.3, 200.0), wall_velocity=wall_velocity)
    r.v[:] = dev(np.array([v]))
    r.force()
    rows = []
    for _ in range(30):
        r.run_native(50, use_graph=True)
        rows.append((float(r.v[0, 0].item()), float(r.L[0, 1].item()), float(r.x[0, 0].item())))
    sp.synchronize()
    pl = sp.get_walls()
    sp.close()
    return np.array(rows), pl


def test_a_sphere_at_rest_on_a_belt_is_the_sliding_sphere_seen_from_the_belt(oracle):
    ref, _ = _floor_run([1.0, 0.0, 0.0], None)
    got, pl = _floor_run([0.0, 0.0, 0.0], [-1.0, 0.0, 0.0])
    t = 1e-4 * 50 * np.arange(1, 31)
    dv, dL, dx = np.abs(got[:, 0] + 1.0 - ref[:, 0]).max(), np.abs(got[:, 1] - ref[:, 1]).max(), np.abs(got[:, 2] + t - ref[:, 2]).max()
    print(f"reference v_x {ref[0, 0]:.6f} -> {ref[-1, 0]:.6f}, L_y -> {ref[-1, 1]:.6f}; belt run: |d v_x| {dv:.2e} |d L_y| {dL:.2e} |d x| {dx:.2e}")
    assert ref[-1, 0] < 1.0 - 1e-3 and ref[-1, 1] > 1e-3              # the reference slowed down and rolls
    assert dv <= 1e-10 and dL <= 1e-10 and dx <= 1e-10
    assert np.array_equal(pl, np.array([[0.0, 0.0, 1.0, 0.0]]))


# ---- 8. a wall that runs over a particle -----------------------------------------------------------------------------------

def test_a_wall_run_over_a_particle_is_reported_and_the_rest_is_right(oracle):
    """An input error the library must report, not a device fault: the floor rises by 0.1 per step, faster than its
    contact force can push sphere 0 away, and passes its centre; sphere 1 rests against a side wall out of the floor's
    reach."""
    import torch
    import wall_ref as W
    from shpair import shapes
    from shpair.capi import ShPairError
    from shpair.run import DeviceRun
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 16, kn=1e3, expo=1.25, rmax=[1.01])
    planes = np.array([[0.0, 0, 1, 0.5], [1.0, 0, 0, 0.0]])
    x = np.array([[5.0, 5.0, 1.55], [0.9, 5.0, 7.0]])
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]] * 2), np.zeros(2, np.int32), (0, 0, 0), (10, 10, 10), (0, 0, 0), 0.5, dt=1e-3,
                  walls=(planes, 1e3, 1.25), wall_velocity=[[0.0, 0.0, 100.0], [0.0, 0.0, 0.0]])
    with pytest.raises(ShPairError, match="particle centre behind a wall") as e:
        r.run_native(20)
    assert e.value.code == -1
    torch.cuda.synchronize()
    sp.synchronize()                     # the error word was read and cleared
    pl = sp.get_walls()
    xe, qe, f, tq = r.x[:2].cpu().numpy(), r.q[:2].cpu().numpy(), r.f[:2].cpu().numpy(), r.tq[:2].cpu().numpy()
    ref = W.wall_forces([(0, shapes.sphere(1.0), 1.01)], 16, xe, qe, np.zeros(2, np.int32), pl, [1e3] * 2, [1.25] * 2)
    scale = np.abs(ref["f"]).max()
    print(f"floor at {pl[0, 3]:.3f}, sphere 0 at z {xe[0, 2]:.3f}; force on sphere 1 {f[1]}, reference {ref['f'][1]}")
    assert abs(pl[0, 3] - 2.5) <= 1e-12 and xe[0, 2] < pl[0, 3] and ref["nbehind"] == 1
    assert scale > 0 and ref["f"][1, 0] > 0 and not ref["f"][0].any()
    assert np.abs(f - ref["f"]).max() <= TOL * scale and np.abs(tq - ref["torque"]).max() <= TOL * scale
    sp.close()


# ---- 9. two ranks -------------------------------------------------------------------------------------------------------------

def test_two_ranks_with_a_rising_damped_floor_match_the_single_domain():
    """Thread pattern and bed of test_two_ranks_with_a_floor_match_the_single_domain (tests/test_gpu_wall.py); K = 4 steps of
    shhalo_run_device.  The baseline is the same run with u = 0 (the parent's behaviour): its grid-to-grid deviation d0
    sets the bar of the moving run, 4 max(d0, 1e-12 max|F|) — the 4 for the one extra rounding per wall per step."""
    from shpair import shapes, mrank, bed
    from mrank_common import _run_ranks, _distribute
    from test_gpu_wall import ctx
    lmax, nq, skin, K, dt = 4, 8, 0.2, 4, 2e-3
    shp = [(lmax, shapes.random_shape(lmax, 400 + s, amp=0.2)) for s in range(2)]
    periodic = (1, 1, 0)
    pts, lo, hi = bed.periodic_hcp(1500, 1.9, periodic)
    rng = np.random.default_rng(9)
    n = pts.shape[0]
    x = pts + rng.uniform(-0.15, 0.15, pts.shape)
    quat = bed.random_quaternions(n, rng)
    sht = rng.integers(0, 2, n).astype(np.int32)
    tag = np.arange(n, dtype=np.int32)
    zmin, zmax = x[:, 2].min(), x[:, 2].max()
    planes = np.array([[0, 0, 1, zmin - 0.7], [0, 0, -1, -(zmax + 0.7)]])
    sp0 = ctx(shp, nq, kn=400.0)
    cut = 2.0 * max(sp0.rmax(s) for s in range(2)) + skin
    sp0.close()

    def run(grid, vel):
        world = int(np.prod(grid))
        xw, owner = _distribute(grid, lo, hi, periodic, cut, x)
        hub = mrank.Hub(world) if world > 1 else None

        def body(rank):
            sp = ctx(shp, nq, kn=400.0)
            sp.set_option("halo_twists", 1)
            sp.set_walls(planes, 400.0, 1.25)
            sp.wall_damping(500.0)
            halo = mrank.Halo(sp, rank, world, grid, lo, hi, periodic, skin, hub=hub)
            mine = owner == rank
            r = mrank.RankRun(sp, halo, xw[mine], quat[mine], sht[mine], tag[mine], dt=dt, wall_velocity=vel)
            r.run(K)
            t, _, _, _, f, tq = r.owned()
            res = (t, f, tq, sp.wall_stats(), sp.get_walls())
            halo.close()
            sp.close()
            return res
        parts = _run_ranks(world, body)
        if hub is not None:
            hub.close()
        f = np.zeros((n, 3))
        for t, pf, _, _, _ in parts:
            f[t] = pf
        return f, sum(p[3] for p in parts), [p[4] for p in parts]
    vel = np.array([[0.3, 0.0, 0.5], [0.0, 0.0, 0.0]])       # the floor rises (and slides: damping sees the normal part only)
    out = {(g, m): run(g, vel if m else None) for g in ((1, 1, 1), (2, 1, 1)) for m in (False, True)}
    f1, c1, w1 = out[((1, 1, 1), True)]
    f2, c2, w2 = out[((2, 1, 1), True)]
    scale = np.abs(f1).max()
    d0 = np.abs(out[((1, 1, 1), False)][0] - out[((2, 1, 1), False)][0]).max()
    d1 = np.abs(f1 - f2).max()
    print(f"wall contacts {c1} / {c2}, max|F| {scale:.4g}, grid-to-grid deviation: walls at rest {d0:.2e}, rising floor {d1:.2e}")
    assert c1 == c2 and c1 > 0
    assert all(np.array_equal(w, w1[0]) for w in w1 + w2)                            # every rank, every grid: the same planes
    assert w1[0][0, 3] > planes[0, 3] + 0.9 * K * dt * 0.5 and w1[0][1, 3] == planes[1, 3]
    assert np.abs(f1 - out[((1, 1, 1), False)][0]).max() > 1e-6 * scale                 # the rising floor acted
    assert d1 <= 4.0 * max(d0, 1e-12 * scale)


# ---- 10. argument checks --------------------------------------------------------------------------------------------------------

def test_argument_checks():
    import ctypes
    from shpair import shapes
    from shpair.capi import ShPairError
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 8)
    with pytest.raises(ShPairError, match="after shstep_set_walls") as e:       # before set_walls
        sp.wall_velocity([[0.0, 0.0, 1.0]])
    assert e.value.code == -1
    sp.set_walls([[0, 0, 1, 0.0], [1, 0, 0, 0.0]], 1000.0, 1.25)
    for u in ([[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]] * 3, [[np.nan, 0, 0], [0, 0, 0]], [[0, 0, 0], [0, np.inf, 0]], [[0, 0, -np.inf], [0, 0, 0]]):
        with pytest.raises(ShPairError) as e:
            sp.wall_velocity(u)
        assert e.value.code == -1
    assert sp._lib.shstep_set_wall_velocity(sp._h, 2, None) == -1                # a null pointer with nwalls > 0
    assert not sp.move_walls
    with pytest.raises(ShPairError, match="dt is not finite") as e:
        sp.advance_walls_device(np.nan)
    assert e.value.code == -1
    p = (ctypes.c_double * 4)()
    assert sp._lib.shstep_get_walls(sp._h, 1, p) == -1                           # a count mismatch
    assert sp._lib.shstep_get_walls(sp._h, 2, None) == -1
    sp.wall_velocity([1.0, 2.0, 3.0])                                            # one vector for every wall
    sp.advance_walls_device(0.5)
    assert np.array_equal(sp.get_walls(), np.array([[0, 0, 1, 1.5], [1, 0, 0, 0.5]]))
    sp.close()
