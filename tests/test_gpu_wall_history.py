"""GPU tests of the tangential contact springs with history at planar walls of docs/SPEC.md §2.15 (the HIST instances and
the sweep of csrc/wall_kernels.hpp, through the C ABI of include/shstep.h) against tests/wall_history_ref.py: parity of
one advancing pass, a load at rest, a look, stale rows, off is off, the three loops, a restart, a belt against its mirror
experiment, the ledger, refusals.

K_T, DT and XI0 of the parity test were chosen on the CPU, with the reference alone, so that the condition its companion
asserts on the INPUTS holds at every (L, n_q): one sticking, one sliding and one reset contact, with and without the wall
velocities."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dissipation_common import dev, _wall_ctx, _wall_pass   # noqa: E402

TOL = 1e-9            # tests/test_gpu_friction.py's and tests/test_gpu_wall_move.py's
QUAT = np.array([[0.5, 0.5, -0.5, 0.5]])
DT = 1e-3
# per case of test_gpu_friction.WALL_CASES; the corner has history on two walls and plain friction on the third
K_T = {"oblique_in": np.array([2000.0]), "oblique_out": np.array([2000.0]), "corner": np.array([2000.0, 2000.0, 0.0])}
XI0 = {"oblique_in": np.array([[0.01, -0.02, 0.015]]), "oblique_out": np.array([[0.01, -0.02, 0.015]]),
       "corner": np.array([[0.0, 0.004, -0.003], [0.3, 0.0, -0.2], [0.1, 0.1, 0.0]])}
_refs = {}


def _cases():
    import test_gpu_friction as G
    import test_gpu_wall_move as MV
    return G.WALL_CASES, MV.WALL_VEL, MV.CONFIGS, MV._coefficients, MV._shape


def _contact_pass(sp, x, quat, tw, nwalls, dt):
    """One shstep_wall_contact_device call on fresh arrays: f, torque [n][3], wall_out [nw][4]."""
    import torch
    n = len(x)
    xd, qd, sh, m, twd = dev(x), dev(quat), dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32)), dev(tw)
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    out = torch.zeros(nwalls, 4, dtype=torch.float64, device="cuda:0")
    sp.wall_contact_device(n, xd.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), twd.data_ptr(), dt,
                           wall_out=out.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy()


def _reference(lmax, nq, name, moving, rmax, dt=DT):
    """(with the springs, the same walls without any coefficient) from tests/wall_history_ref.py: computed once, shared."""
    import wall_history_ref as H
    cases, wall_vel, _, coefficients, shape = _cases()
    key = (lmax, nq, name, moving, dt)
    if key not in _refs:
        planes, x0, tw0, _ = cases[name]
        nw = len(planes)
        a = ([(lmax, shape(lmax), rmax)], nq, x0[None, :], QUAT, np.zeros(1, np.int32), tw0[None, :], planes)
        kn, expo, gam, mu, gt = coefficients(nw)
        vel = wall_vel[name] if moving else np.zeros((nw, 3))
        live = XI0[name].any(axis=1)[None, :]
        z = np.zeros(nw)
        _refs[key] = (H.wall_forces_history(*a, kn, expo, gam, mu, gt, K_T[name], vel, XI0[name][None], live, dt),
                      H.wall_forces_history(*a, kn, expo, z, z, z, z, vel, XI0[name][None], live, dt))
    return _refs[key]


def _spring_ctx(lmax, nq, name, moving):
    cases, wall_vel, _, coefficients, shape = _cases()
    planes = cases[name][0]
    nw = len(planes)
    kn, expo, gam, mu, gt = coefficients(nw)
    sp = _wall_ctx([(lmax, shape(lmax))], nq)
    sp.set_walls(planes, kn, expo)
    sp.wall_damping(gam)
    sp.wall_friction(mu, gt)
    sp.set_wall_tangential_spring(K_T[name])
    if moving:
        sp.wall_velocity(wall_vel[name])
    return sp, nw


# ---- 1. parity of one advancing pass -------------------------------------------------------------------------------------

@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("lmax,nq", [(6, 16), (4, 10), (4, 1)])
@pytest.mark.parametrize("name", ["oblique_in", "oblique_out", "corner"])
def test_advancing_pass_matches_the_reference(oracle, name, lmax, nq, moving):
    cases = _cases()[0]
    _, x0, tw0, _ = cases[name]
    sp, nw = _spring_ctx(lmax, nq, name, moving)
    sp.set_wall_history(1, XI0[name][None])
    f, tq, out = _contact_pass(sp, x0[None, :], QUAT, tw0[None, :], nw, DT)
    xi = sp.wall_history(1)
    nc = sp.wall_stats()
    ref, elastic = _reference(lmax, nq, name, moving, sp.rmax(0))
    sp.close()
    scale = max(np.abs(elastic["f"]).max(), np.abs(ref["f"]).max())
    tscale = max(scale, np.abs(elastic["torque"]).max(), np.abs(ref["torque"]).max())
    ef, et = np.abs(f - ref["f"]).max() / scale, np.abs(tq - ref["torque"]).max() / tscale
    eo = np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() / scale
    ee = np.abs(out[:, 0] - ref["wall_out"][:, 0]).max() / np.abs(ref["wall_out"][:, 0]).max()
    xs = np.abs(ref["xi"]).max()
    ex = np.abs(xi - ref["xi"]).max()
    print(f"L={lmax} nq={nq} {name} moving={moving}: contacts {nc}, kinds {list(ref['kind'][0])}, max|F| {scale:.4g}, rel err f {ef:.1e} "
          f"torque {et:.1e} wall force {eo:.1e} wall energy {ee:.1e}; max|xi| {xs:.3e}, err xi {ex:.1e}")
    assert nc == len(ref["contacts"]) == nw and scale > 0
    assert ef <= TOL and et <= TOL and eo <= TOL and ee <= TOL
    assert ex <= TOL * xs
    assert np.array_equal(xi.any(axis=2), ref["live"])                           # the live bits, through the copy


@pytest.mark.parametrize("lmax,nq", [(6, 16), (4, 10), (4, 1)])
def test_parity_inputs_hold_a_stick_a_slide_and_a_reset(oracle, lmax, nq):
    """A condition on the inputs, read from the reference alone."""
    import wall_history_ref as H
    _, _, configs, _, shape = _cases()
    assert (lmax, nq) in configs
    sp = _wall_ctx([(lmax, shape(lmax))], nq)
    rmax = sp.rmax(0)
    sp.close()
    for moving in (False, True):
        kinds = {k for name in K_T for k in _reference(lmax, nq, name, moving, rmax)[0]["kind"][0]}
        assert {H.STICK, H.SLIDE, H.RESET} <= kinds, (moving, kinds)


# ---- 2. a contact at rest carries a load ---------------------------------------------------------------------------------

def test_a_contact_at_rest_carries_a_tangential_load(oracle):
    cases, _, _, coefficients, shape = _cases()
    planes, x0, _, _ = cases["oblique_in"]
    kn, expo, _, mu, gt = coefficients(1)
    n = planes[0, :3]
    xi0 = np.array([2e-3, -1e-3, 3e-3])
    tw = np.zeros((1, 6))
    sp = _wall_ctx([(6, shape(6))], 16)
    sp.set_walls(planes, kn, expo)
    elastic = _wall_pass(sp, x0[None, :], QUAT, tw, 1, damped=False)
    sp.wall_friction(mu, gt)
    plain = _wall_pass(sp, x0[None, :], QUAT, tw, 1)                 # k_t = 0: at v_t = 0 the friction of §2.11 is exactly 0
    assert all(np.array_equal(a, b) for a, b in zip(elastic, plain))
    sp.set_wall_tangential_spring(K_T["oblique_in"])
    sp.set_wall_history(1, xi0[None, None, :])
    f, tq, out = _contact_pass(sp, x0[None, :], QUAT, tw, 1, DT)
    xi = sp.wall_history(1)[0, 0]
    sp.close()
    want = -K_T["oblique_in"][0] * (xi0 - (xi0 @ n) * n)
    scale = np.abs(elastic[0]).max()
    Ft = f[0] - elastic[0][0]
    print(f"F_t {Ft}, -k_t xi {want}, max|F| {scale:.4g}, mu N {mu[0] * scale:.4g}")
    assert np.linalg.norm(want) > 1e-3 * scale and np.linalg.norm(want) < 0.5 * mu[0] * scale      # a load, well inside the cap
    assert np.abs(Ft - want).max() <= TOL * scale
    assert np.abs(out[0, 1:] + f[0]).max() <= TOL * scale                                            # the wall's row: minus the whole force
    assert np.abs(xi - (xi0 - (xi0 @ n) * n)).max() <= TOL * np.abs(xi0).max()                       # no motion: xi only loses its normal part


# ---- 3. a look writes nothing ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("moving", [False, True])
def test_a_look_writes_nothing_and_gives_the_reference_forces(oracle, moving):
    cases = _cases()[0]
    _, x0, tw0, _ = cases["corner"]
    sp, nw = _spring_ctx(6, 16, "corner", moving)
    sp.set_wall_history(1, XI0["corner"][None])
    f, tq, out = _contact_pass(sp, x0[None, :], QUAT, tw0[None, :], nw, 0.0)
    xi = sp.wall_history(1)
    rmax = sp.rmax(0)
    ref, elastic = _reference(6, 16, "corner", moving, rmax, dt=0.0)
    assert np.array_equal(xi, XI0["corner"][None])                    # every xi and, through the copy, every live bit
    f2, tq2, out2 = _contact_pass(sp, x0[None, :], QUAT, tw0[None, :], nw, 0.0)
    assert np.array_equal(f, f2) and np.array_equal(tq, tq2) and np.array_equal(out, out2)
    sp.close()
    scale = max(np.abs(elastic["f"]).max(), np.abs(ref["f"]).max())
    assert np.abs(f - ref["f"]).max() <= TOL * scale and np.abs(tq - ref["torque"]).max() <= TOL * scale
    assert np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() <= TOL * scale
    adv = _reference(6, 16, "corner", moving, rmax)[0]
    assert np.abs(ref["f"] - adv["f"]).max() > 1e-6 * scale           # the look is not the advancing pass


# ---- 4. stale rows die ---------------------------------------------------------------------------------------------------------

def test_a_particle_that_leaves_the_walls_reach_loses_its_xi(oracle):
    from shpair import shapes
    q1 = np.array([[1.0, 0.0, 0.0, 0.0]])
    near, far = np.array([[0.0, 0.0, 0.95]]), np.array([[0.0, 0.0, 1.5]])       # R = 1.01: h >= R at 1.5
    slide, rest = np.array([[0.4, -0.3, 0.0, 0.0, 0.0, 0.0]]), np.zeros((1, 6))

    def ctx():
        sp = _wall_ctx([(0, shapes.sphere(1.0))], 16, kn=1e4, expo=1.25, rmax=[1.01])
        sp.set_walls([[0, 0, 1, 0.0]], 1e4, 1.25)
        sp.wall_friction(0.5, 0.0)                                               # a history wall with gamma_t = 0
        sp.set_wall_tangential_spring(2e4)
        return sp
    sp = ctx()
    loaded = _contact_pass(sp, near, q1, slide, 1, DT)
    xi = sp.wall_history(1)
    assert np.abs(xi[0, 0, :2] - DT * slide[0, :2]).max() <= 1e-15 and np.abs(loaded[0][0, :2]).max() > 1.0     # loaded, sticking
    away = _contact_pass(sp, far, q1, rest, 1, DT)                               # straight out of reach: no pass at V = 0 between
    assert not away[0].any() and not sp.wall_history(1).any()
    back = _contact_pass(sp, near, q1, rest, 1, DT)
    assert not sp.wall_history(1).any()                                          # at rest from xi = 0: the bit is live, xi is 0
    sp.close()
    sp = ctx()
    fresh = _contact_pass(sp, near, q1, rest, 1, DT)                             # a context that never held a xi
    sp.close()
    assert all(np.array_equal(a, b) for a, b in zip(back, fresh)) and np.abs(fresh[0]).max() > 0
    assert np.abs(back[0][0, :2]).max() <= 1e-12 * np.abs(back[0]).max()         # nothing tangential beyond the sphere's own rounding


# ---- 5. off changes no bit -----------------------------------------------------------------------------------------------------

def test_without_a_spring_the_contact_call_is_the_damped_call_bit_for_bit(oracle):
    cases, wall_vel, _, coefficients, shape = _cases()
    planes, x0, tw0, _ = cases["corner"]
    kn, expo, gam, mu, gt = coefficients(3)
    sp = _wall_ctx([(6, shape(6))], 16)
    sp.set_walls(planes, kn, expo)
    sp.wall_damping(gam)
    sp.wall_friction(mu, gt)
    sp.set_wall_tangential_spring(np.zeros(3))
    sp.wall_velocity(wall_vel["corner"])
    assert not sp.has_wall_history
    old = _wall_pass(sp, x0[None, :], QUAT, tw0[None, :], 3)
    for dt in (0.0, DT, 7.0):
        new = _contact_pass(sp, x0[None, :], QUAT, tw0[None, :], 3, dt)
        assert all(np.array_equal(a, b) for a, b in zip(old, new)), dt
    assert np.abs(old[0]).max() > 0
    # a spring on wall 1 only: a particle that touches only wall 0 keeps the bits of the friction instance
    x = np.array([[0.8, 5.0, 5.0]])
    plain = _wall_pass(sp, x, QUAT, tw0[None, :], 3)
    sp.set_wall_tangential_spring([0.0, 2000.0, 0.0])
    assert sp.has_wall_history
    sprung = _contact_pass(sp, x, QUAT, tw0[None, :], 3, DT)
    print(f"one wall without a spring beside a sprung one: |df| {np.abs(plain[0] - sprung[0]).max():.1e} |dtau| {np.abs(plain[1] - sprung[1]).max():.1e} "
          f"|dwall| {np.abs(plain[2] - sprung[2]).max():.1e} of max|F| {np.abs(plain[0]).max():.4g}")
    assert sp.wall_stats() == 1 and np.abs(plain[0]).max() > 0 and not plain[2][1:].any()
    assert all(np.array_equal(a, b) for a, b in zip(plain, sprung))
    assert not sp.wall_history(1).any()
    sp.close()


# ---- 6. the loops agree --------------------------------------------------------------------------------------------------------

BED_MU, BED_KT = np.array([0.3, 0, 0, 0, 0.8, 0]), np.array([2000.0, 0, 0, 0, 300.0, 0])     # the belt x = 0 and the floor


def _bed_run(mode, nsteps, x, quat, planes, vel, v=None, shp=None, state=None):
    """A bed in the box of tests/test_gpu_wall.py with a sprung floor and a sprung belt (gamma_t = 0, no wall damping: N is a
    function of the positions alone).  state: (v, angmom, f, torque, xi) of a run to continue."""
    import torch
    from shpair.run import DeviceRun
    from test_gpu_wall import ctx
    sp = ctx(shp, 10, kn=2000.0, deterministic=1)
    L = 8.4
    r = DeviceRun(sp, x, quat, np.zeros(x.shape[0], np.int32), (0, 0, 0), (L, L, L), (0, 0, 0), 0.3, dt=5e-4, gravity=(0.0, 0.0, -9.81),
                  gamma_t=2.0, gamma_r=1.0, walls=(planes, 2000.0, 1.25), wall_friction=(BED_MU, np.zeros(6)), wall_spring=BED_KT,
                  wall_velocity=vel)
    if v is not None:
        r.v[:] = dev(v)
        r.force()
    if state is not None:
        r.v[:], r.L[:] = dev(state[0]), dev(state[1])
        r.f[:r.n], r.tq[:r.n] = dev(state[2]), dev(state[3])
        sp.set_wall_history(r.n, state[4])
        torch.cuda.synchronize()
    if mode == "python":
        r.run(nsteps)
    else:
        r.run_native(nsteps, use_graph=(mode == "graph"))
    torch.cuda.synchronize()
    sp.synchronize()
    n = r.n
    out = [t.cpu().numpy().copy() for t in (r.x[:n], r.v, r.q[:n], r.L, r.f[:n], r.tq[:n])] + [r.wall_history(), sp.get_walls()]
    sp.close()
    return out


def test_the_three_loops_carry_the_same_wall_history_bits(oracle):
    import wall_history_ref as H
    from shpair import shapes
    from test_gpu_wall import _settling_case, box_planes, ctx
    anm = shapes.random_shape(4, 21, amp=0.15)
    shp = [(4, anm)]
    L, nsteps = 8.4, 300
    x, quat = _settling_case(4, L)
    x[:, 2] -= 0.15
    planes = box_planes(L, cut=-10.0)[:6]
    vel = np.zeros((6, 3))
    vel[0] = [0.0, 1.0, 0.0]          # the wall x = 0 is a belt along y
    ref = _bed_run("python", nsteps, x, quat, planes, vel, shp=shp)
    for mode in ("plain", "graph"):
        got = _bed_run(mode, nsteps, x, quat, planes, vel, shp=shp)
        for k, (a, b) in enumerate(zip(ref, got)):
            assert np.array_equal(a, b), (mode, k)
    xe, qe, xi = ref[0], ref[2], ref[6]
    assert np.array_equal(ref[7], planes) and not xi[:, [1, 2, 3, 5]].any()
    # stuck and slid contacts, from the read-back xi against mu N / k_t at the final positions through the reference
    sp = ctx(shp, 10, kn=2000.0)
    rmax = sp.rmax(0)
    sp.close()
    n, z6 = len(xe), np.zeros(6)
    look = H.wall_forces_history([(4, anm, rmax)], 10, xe, qe, np.zeros(n, np.int32), np.zeros((n, 6)), planes, np.full(6, 2000.0),
                                 np.full(6, 1.25), z6, BED_MU, z6, BED_KT, vel, xi, xi.any(axis=2), 0.0)
    slid = stuck = 0
    for c in look["contacts"]:
        i, w, N = c[0], c[1], c[4]
        if BED_KT[w] == 0 or not N > 0:
            continue
        hold, have = BED_MU[w] * N / BED_KT[w], np.linalg.norm(xi[i, w])
        slid += abs(have - hold) <= 1e-9 * hold
        stuck += 0 < have < 0.99 * hold
    print(f"{len(look['contacts'])} wall contacts at the end: {slid} slid in the last step, {stuck} stuck; max|xi| {np.abs(xi).max():.3e}")
    assert slid >= 1 and stuck >= 1


# ---- 7. restart ------------------------------------------------------------------------------------------------------------------

def test_a_restart_from_the_planes_the_arrays_and_the_wall_history_continues_bitwise(oracle):
    """Four particles on the floor, clear of each other (no pair force: the continuation's fresh neighbour list cannot
    matter), one against the belt; the floor rises, so the planes must travel too."""
    from shpair import shapes
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    x = np.array([[0.9, 2.0, 0.95], [4.5, 2.0, 0.9], [2.6, 6.0, 0.95], [6.4, 6.0, 0.9]])
    from shpair import bed
    rng = np.random.default_rng(3)
    quat = bed.random_quaternions(4, rng)
    v = 0.5 * rng.normal(size=(4, 3))
    from test_gpu_wall import box_planes
    planes = box_planes(8.4, cut=-10.0)[:6]
    vel = np.zeros((6, 3))
    vel[0], vel[4] = [0.0, 1.0, 0.0], [0.0, 0.0, 0.05]
    whole = _bed_run("graph", 200, x, quat, planes, vel, v=v, shp=shp)
    half = _bed_run("graph", 100, x, quat, planes, vel, v=v, shp=shp)
    assert half[6].any() and not np.array_equal(half[7], planes)
    rest = _bed_run("graph", 100, half[0], half[2], half[7], vel, shp=shp, state=(half[1], half[3], half[4], half[5], half[6]))
    for k, (a, b) in enumerate(zip(whole, rest)):
        assert np.array_equal(a, b), k
    # ... and the history mattered: the same continuation from xi = 0 ends elsewhere
    bare = _bed_run("graph", 100, half[0], half[2], half[7], vel, shp=shp, state=(half[1], half[3], half[4], half[5], np.zeros_like(half[6])))
    print(f"continuation without its xi: |dx| {np.abs(bare[0] - whole[0]).max():.2e} |dv| {np.abs(bare[1] - whole[1]).max():.2e}")
    assert not np.array_equal(bare[1], whole[1])


# ---- 8. Galilean -----------------------------------------------------------------------------------------------------------------

def _floor_run(v, wall_velocity):
    """tests/test_gpu_wall_move.py's sphere on a floor with friction, with a tangential spring on the floor."""
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 16, kn=1e4, expo=1.25, rmax=[1.01])
    r = DeviceRun(sp, np.array([[0.0, 0.0, 0.9945]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-5, -5, 0), (50, 5, 10),
                  (0, 0, 0), 0.5, dt=1e-4, gravity=(0.0, 0.0, -9.81), walls=([[0, 0, 1, 0.0]], 1e4, 1.25), wall_damping=1000.0,
                  wall_friction=(0.3, 200.0), wall_spring=5e3, wall_velocity=wall_velocity)
    r.v[:] = dev(np.array([v]))
    r.force()
    rows = []
    for _ in range(30):
        r.run_native(50, use_graph=True)
        rows.append((float(r.v[0, 0].item()), float(r.L[0, 1].item()), float(r.x[0, 0].item()), *r.wall_history()[0, 0]))
    sp.synchronize()
    sp.close()
    return np.array(rows)


def test_a_sphere_at_rest_on_a_sprung_belt_is_the_moving_sphere_seen_from_the_belt(oracle):
    """Run A: at rest on a belt moving at u = (-1, 0, 0).  Run B: moving at -u on the same wall at rest.  The bar is that of
    test_a_sphere_at_rest_on_a_belt_is_the_sliding_sphere_seen_from_the_belt: 1e-10."""
    ref = _floor_run([1.0, 0.0, 0.0], None)
    got = _floor_run([0.0, 0.0, 0.0], [-1.0, 0.0, 0.0])
    t = 1e-4 * 50 * np.arange(1, 31)
    dv, dL, dx = np.abs(got[:, 0] + 1.0 - ref[:, 0]).max(), np.abs(got[:, 1] - ref[:, 1]).max(), np.abs(got[:, 2] + t - ref[:, 2]).max()
    dxi = np.abs(got[:, 3:] - ref[:, 3:]).max()
    print(f"reference v_x {ref[0, 0]:.6f} -> {ref[-1, 0]:.6f}, L_y -> {ref[-1, 1]:.6f}, xi_x -> {ref[-1, 3]:.4e}; belt run: |d v_x| {dv:.2e} "
          f"|d L_y| {dL:.2e} |d x| {dx:.2e} |d xi| {dxi:.2e}")
    assert ref[-1, 0] < 1.0 - 1e-3 and ref[-1, 1] > 1e-3 and np.abs(ref[:, 3]).max() > 1e-5      # it slowed down, rolls, and xi is loaded
    assert dv <= 1e-10 and dL <= 1e-10 and dx <= 1e-10 and dxi <= 1e-10


# ---- 9. the ledger ---------------------------------------------------------------------------------------------------------------

def _impact(k, dissipative):
    """A unit sphere with spin hits a floor obliquely and leaves it; dt = 1e-4 / k."""
    import torch
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 32, kn=1e4, expo=1.25, rmax=[1.01], deterministic=1)   # n_q = 32: see the test
    kw = dict(wall_damping=8000.0, wall_friction=(0.5, 20.0), wall_spring=2e4) if dissipative else {}
    r = DeviceRun(sp, np.array([[0.0, 0.0, 1.5]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-5, -5, 0), (5, 5, 10), (0, 0, 0),
                  0.5, dt=1e-4 / k, walls=([[0, 0, 1, 0.4]], 1e4, 1.25), ledger=True, **kw)
    r.v[:] = dev(np.array([[0.7, 0.0, -1.0]]))
    r.L[:] = dev(np.array([[0.0, -0.4, 0.3]]))
    r.force()
    torch.cuda.synchronize()
    e = r.energies()
    E0 = e[1] + e[2]
    seen = 0.0
    for _ in range(30):
        r.run_native(100 * k, use_graph=True, check_every=50)
        if dissipative:
            seen = max(seen, float(np.abs(r.wall_history()).max()))
    led = r.ledger()
    e = r.energies()
    E1 = e[1] + e[2]
    gap = float(r.x[0, 2].item()) - 0.4
    xi = r.wall_history() if dissipative else np.zeros((1, 1, 3))
    sp.close()
    return E0, E1, led["dissipated"], led["work"], led["wall_friction"], gap, xi, seen


def test_the_balance_of_an_oblique_spinning_impact_on_a_sprung_floor_closes_to_first_order_in_dt(oracle):
    """The bounds are those of the pair-history ledger test of tests/test_gpu_history.py: the elastic residual is at most a
    tenth of the dissipative one, and the dissipative one falls to at most 0.75 of itself at dt / 2.  The sphere starts and
    ends clear of the floor, so E_mech is the kinetic energy; the floor is at rest, W = 0.
    n_q = 32: the elastic residual is the quadrature noise of the sharp rule at a wall (nodes crossing the plane), which does
    not fall with dt but does with n_q; at n_q = 16 it is 1.6e-4 at dt and 8.2e-4 at dt / 2, beside the first-order term.
    Measured on an MI355X: R = 9.401e-3 and 4.752e-3 (ratio 0.506), R0 = 5.17e-4 and 3.22e-4, D = 1.208 of E0 = 3.195."""
    R, R0 = [], []
    for k in (1, 2):
        E0, E1, D, W, Pf, gap, xi, seen = _impact(k, True)
        e0, e1, d0, _, _, gap0, _, _ = _impact(k, False)
        R.append(abs(E1 - E0 - W + D))
        R0.append(abs(e1 - e0))
        print(f"dt/{k}: E0 {E0:.6f} E1 {E1:.6f} D {D:.6f} (wall friction row {Pf:.6f}) W {W:.3e} R {R[-1]:.3e} R/D {R[-1] / D:.2e} elastic R0 "
              f"{R0[-1]:.3e} gap {gap:.3f} largest |xi| {seen:.3e}")
        assert gap > 1.01 and gap0 > 1.01 and d0 == 0.0 and W == 0.0      # it met the floor and left it
        assert seen > 0 and not xi.any()                                    # the spring was loaded, and leaving the reach dropped it
        assert Pf > 0 and 0.3 * E0 < D < E0                               # (the input condition of the pair test)
    print(f"R(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert R0[0] <= 0.1 * R[0] and R0[1] <= 0.1 * R[1]
    assert R[1] <= 0.75 * R[0]


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals(oracle):
    import torch
    from shpair import mrank, shapes
    from shpair.capi import ShPairError, HaloArrays, HaloRunParams
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 8)
    with pytest.raises(ShPairError, match="after shstep_set_walls") as e:       # before set_walls
        sp.set_wall_tangential_spring([1.0])
    assert e.value.code == -1
    sp.set_walls([[0, 0, 1, 0.0], [1, 0, 0, 0.0]], 1000.0, 1.25)
    for kt in ([1.0], [1.0, 2.0, 3.0], [-1.0, 0.0], [np.nan, 1.0], [1.0, np.inf]):
        with pytest.raises(ShPairError) as e:
            sp.set_wall_tangential_spring(kt)
        assert e.value.code == -1
    assert sp._lib.shstep_set_wall_tangential_spring(sp._h, 2, None) == -1
    assert not sp.has_wall_history
    with pytest.raises(ShPairError, match="no wall tangential spring") as e:    # no history to copy
        sp.wall_history(1)
    assert e.value.code == -4
    sp.set_wall_tangential_spring([2000.0, 0.0])
    sp.wall_friction([0.5, 0.0], [0.0, 0.0])                                     # spring first, mu second: a history wall with gamma_t = 0
    assert sp.has_wall_history and not sp.fric_walls
    n = 2
    x, q = dev(np.array([[5.0, 5.0, 0.9], [0.9, 5.0, 5.0]])), dev(np.array([[1.0, 0, 0, 0]] * 2))
    sh, m, tw = dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32)), dev(np.zeros((n, 6)))
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    # the three older wall calls refuse while a spring is set, and name the new one
    with pytest.raises(ShPairError, match="shstep_wall_contact_device") as e:
        sp.wall_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    assert e.value.code == -1
    with pytest.raises(ShPairError, match="shstep_wall_contact_device") as e:
        sp.wall_force_damped_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), tw.data_ptr())
    assert e.value.code == -1
    with pytest.raises(ShPairError, match="shstep_wall_contact_device") as e:
        sp.wall_force(np.array([[5.0, 5.0, 0.9]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32))
    assert e.value.code == -1
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ShPairError, match="dt") as e:
            sp.wall_contact_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), tw.data_ptr(), bad)
        assert e.value.code == -1
    with pytest.raises(ShPairError, match="null twist") as e:
        sp.wall_contact_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), None, DT)
    assert e.value.code == -1
    assert not f.any() and not tq.any()
    # a wrong nlocal in copy and set
    sp.wall_contact_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), tw.data_ptr(), DT)
    sp.synchronize()
    assert sp.wall_history(n).shape == (2, 2, 3)
    for wrong in (n + 1, 1, -1):
        xi = np.zeros(6 * max(wrong, n)).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert sp._lib.shstep_copy_wall_history(sp._h, wrong, xi) == -1
    for wrong in (0, -1):
        assert sp._lib.shstep_set_wall_history(sp._h, wrong, xi) == -1
    assert sp._lib.shstep_set_wall_history(sp._h, n, None) == -1
    # the loop over several ranks, and its Python driver
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    with pytest.raises(ShPairError, match="wall tangential history is single-rank") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -4
    with pytest.raises(ShPairError, match="wall tangential history is single-rank") as e:
        mrank.RankRun.force(type("R", (), dict(sp=sp, a=None, stream=None, halo=None))())
    assert e.value.code == -4
    sp.set_walls([[0, 0, 1, 0.0]], 1000.0, 1.25)                                  # set_walls drops the spring and the refusals
    assert not sp.has_wall_history
    sp.wall_force_device(1, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    sp.synchronize()
    halo.close()
    sp.close()
