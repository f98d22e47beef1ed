"""GPU tests of the planar walls of docs/SPEC.md §2.9 (csrc/wall_kernels.hpp through the C ABI of include/shstep.h)
against tests/wall_ref.py: forces, torques and per-wall totals at SPEC §4's gate (1e-9 of the largest force), every
order and both ends of the n_q range, masks, errors, reproducibility, the step loops and two ranks on one GPU."""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dissipation_common import _wall_ctx as ctx, dev  # noqa: E402

GATE = 1e-9
S3 = 1.0 / np.sqrt(3.0)


def ref_shapes(sp, shp):
    return [(lmax, a, sp.rmax(s)) for s, (lmax, a) in enumerate(shp)]


def box_planes(L, cut=2.5):
    """Six walls of the box [0, L]^3 and one oblique plane that cuts the corner at the origin."""
    return np.array([[1, 0, 0, 0], [-1, 0, 0, -L], [0, 1, 0, 0], [0, -1, 0, -L], [0, 0, 1, 0], [0, 0, -1, -L],
                     [S3, S3, S3, cut]], dtype=np.float64)


def box_case(seed, n, L, nshapes, margin=0.35):
    """n jittered particles inside the planes of box_planes(L), every centre at least `margin` inside every plane."""
    from shpair import bed
    rng = np.random.default_rng(seed)
    pl = box_planes(L)
    x = np.zeros((0, 3))
    while x.shape[0] < n:
        p = rng.uniform(0, L, size=(4 * n, 3))
        h = p @ pl[:, :3].T - pl[:, 3]
        x = np.concatenate([x, p[(h >= margin).all(axis=1)]])
    x = x[:n].copy()
    return dict(x=x, quat=bed.random_quaternions(n, rng), shtype=rng.integers(0, nshapes, n).astype(np.int32), planes=pl, n=n)


def run_device(sp, case, kn, expo, mask=None, groupbit=1, f0=None, want_out=True):
    """One shstep_wall_force_device call on fresh device arrays. Returns f, torque, wall_out, ncontacts."""
    import torch
    n = case["n"]
    sp.set_walls(case["planes"], kn, expo)
    x, q, sh = dev(case["x"]), dev(case["quat"]), dev(case["shtype"])
    m = dev(np.ones(n, dtype=np.int32) if mask is None else mask.astype(np.int32))
    f = dev(np.zeros((n, 3)) if f0 is None else f0[0])
    tq = dev(np.zeros((n, 3)) if f0 is None else f0[1])
    out = torch.zeros(len(case["planes"]), 4, dtype=torch.float64, device="cuda:0")
    sp.wall_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(),
                         groupbit=groupbit, wall_out=out.data_ptr() if want_out else None)
    torch.cuda.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy(), sp.wall_stats()


def check_against_ref(got, ref, label):
    f, tq, out, nc = got
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ef, et = np.abs(f - ref["f"]).max() / scale, np.abs(tq - ref["torque"]).max() / tscale
    eo = np.abs(out[:, 1:] - ref["wall_out"][:, 1:]).max() / np.abs(ref["wall_out"][:, 1:]).max()
    ee = np.abs(out[:, 0] - ref["wall_out"][:, 0]).max() / np.abs(ref["wall_out"][:, 0]).max()
    print(f"{label}: contacts {nc}, max|F| {scale:.4g}, rel err f {ef:.1e} torque {et:.1e} wall force {eo:.1e} wall energy {ee:.1e}")
    assert scale > 0 and nc == ref["ncontacts"] and nc > 0
    assert ef <= GATE and et <= GATE and eo <= GATE and ee <= GATE
    # momentum: what the particles receive the walls give; and the energies add up
    assert np.abs(f.sum(axis=0) + out[:, 1:].sum(axis=0)).max() <= GATE * scale * max(1, nc)
    assert abs(out[:, 0].sum() - ref["wall_out"][:, 0].sum()) <= GATE * abs(ref["wall_out"][:, 0].sum())


@pytest.mark.parametrize("lmax,nq,nshapes,n", [(4, 10, 1, 300), (6, 16, 1, 300), (6, 16, 4, 300), (12, 32, 1, 100)])
def test_box_with_oblique_plane_matches_reference(oracle, lmax, nq, nshapes, n):
    """The BASELINE shapes in a 6-wall box plus a plane that cuts a corner; the walls carry the exponents 1, 1.25, 2."""
    import wall_ref as W
    from shpair import shapes
    shp = [(lmax, shapes.random_shape(lmax, 500 + 7 * s + lmax, amp=0.1)) for s in range(nshapes)]
    case = box_case(lmax + nshapes, n, 7.0, nshapes)
    kn = np.array([1000.0, 800.0, 1200.0, 1000.0, 2000.0, 500.0, 900.0])
    expo = np.array([1.0, 1.25, 2.0, 1.0, 1.25, 2.0, 1.25])
    sp = ctx(shp, nq, deterministic=1)
    got = run_device(sp, case, kn, expo)
    ref = W.wall_forces(ref_shapes(sp, shp), nq, case["x"], case["quat"], case["shtype"], case["planes"], kn, expo)
    assert ref["nbehind"] == 0
    check_against_ref(got, ref, f"L={lmax} nq={nq} shapes={nshapes}")
    # reproducibility: a second call on the same state gives the same bits (f, torque, and the per-wall totals)
    again = run_device(sp, case, kn, expo)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]) and np.array_equal(got[2], again[2])
    # the host-pointer form computes the same
    fh, th, oh = sp.wall_force(case["x"], case["quat"], case["shtype"])
    assert np.array_equal(fh, got[0]) and np.array_equal(th, got[1]) and np.array_equal(oh, got[2])
    sp.close()
    # without the deterministic option the per-particle rows are the same bits as well (no atomics on f)
    sp2 = ctx(shp, nq)
    plain = run_device(sp2, case, kn, expo)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])
    sp2.close()


@pytest.mark.parametrize("lmax", list(range(13)) + [15, 20])
def test_every_order(oracle, lmax):
    """Every compiled order 0..12 and the run-time orders 15 and 20 on a small case."""
    import wall_ref as W
    from shpair import shapes
    shp = [(lmax, shapes.random_shape(lmax, 900 + lmax, amp=0.1))]
    case = box_case(100 + lmax, 40, 4.0, 1)
    sp = ctx(shp, 8)
    got = run_device(sp, case, 1000.0, 1.25)
    ref = W.wall_forces(ref_shapes(sp, shp), 8, case["x"], case["quat"], case["shtype"], case["planes"], [1000.0] * 7, [1.25] * 7)
    check_against_ref(got, ref, f"L={lmax}")
    sp.close()


@pytest.mark.parametrize("nq,n", [(1, 40), (2, 40), (128, 4)])
def test_both_ends_of_the_nq_range(oracle, nq, n):
    import wall_ref as W
    from shpair import shapes
    shp = [(4, shapes.random_shape(4, 77, amp=0.1))]
    case = box_case(200 + nq, n, 2.6, 1)
    sp = ctx(shp, nq)
    got = run_device(sp, case, 1000.0, 1.25)
    ref = W.wall_forces(ref_shapes(sp, shp), nq, case["x"], case["quat"], case["shtype"], case["planes"], [1000.0] * 7, [1.25] * 7)
    check_against_ref(got, ref, f"nq={nq}")
    sp.close()


def test_particle_in_a_corner_touches_three_walls(oracle):
    import wall_ref as W
    from shpair import shapes
    shp = [(6, shapes.random_shape(6, 3, amp=0.1))]
    pl = box_planes(10.0, cut=-5.0)[:6]
    case = dict(x=np.array([[0.8, 0.9, 0.7], [5.0, 5.0, 5.0]]), quat=np.array([[0.5, 0.5, -0.5, 0.5], [1.0, 0, 0, 0]]),
                shtype=np.zeros(2, np.int32), planes=pl, n=2)
    sp = ctx(shp, 16)
    got = run_device(sp, case, 1000.0, 1.25)
    ref = W.wall_forces(ref_shapes(sp, shp), 16, case["x"], case["quat"], case["shtype"], pl, [1000.0] * 6, [1.25] * 6)
    assert ref["ncontacts"] == 3 and (got[0][0] > 0).all() and not got[0][1].any()
    check_against_ref(got, ref, "corner")
    sp.close()


@pytest.mark.parametrize("lmax,nq", [(4, 10), (6, 16)])
def test_three_walls_whose_exponents_take_pow(oracle, lmax, nq):
    """The walls x = 0, y = 0, z = 0 with m_w = 1.75, 2.5, 1.3: V^(m-1) of the wall pass is pow(V, 0.75 / 1.5 / 0.3), which
    the exponents 1, 1.25 and 2 of the other cases never reach with these arguments.  Every wall has contacts, counted
    from the reference."""
    import wall_ref as W
    from shpair import shapes
    shp = [(lmax, shapes.random_shape(lmax, 640 + 7 * s + lmax, amp=0.1)) for s in range(2)]
    case = box_case(60 + lmax, 150, 4.0, 2)
    case["planes"] = case["planes"][[0, 2, 4]]
    kn, expo = np.array([900.0, 1500.0, 700.0]), np.array([1.75, 2.5, 1.3])
    sp = ctx(shp, nq, deterministic=1)
    got = run_device(sp, case, kn, expo)
    rs = ref_shapes(sp, shp)
    ref = W.wall_forces(rs, nq, case["x"], case["quat"], case["shtype"], case["planes"], kn, expo)
    per_wall = [W.wall_forces(rs, nq, case["x"], case["quat"], case["shtype"], case["planes"][w:w + 1], kn[w:w + 1],
                              expo[w:w + 1])["ncontacts"] for w in range(3)]
    print(f"contacts per wall (reference) {per_wall}")
    assert ref["nbehind"] == 0 and min(per_wall) >= 5 and sum(per_wall) == ref["ncontacts"]
    check_against_ref(got, ref, f"L={lmax} nq={nq} m_w={expo.tolist()}")
    sp.close()


def test_groupbit_masks_particles_and_far_bed_is_untouched(oracle):
    import wall_ref as W
    from shpair import shapes
    shp = [(4, shapes.random_shape(4, 11, amp=0.1))]
    case = box_case(5, 200, 6.0, 1)
    rng = np.random.default_rng(3)
    mask = np.where(rng.uniform(size=200) < 0.5, 1, 2).astype(np.int32)
    f0 = (rng.normal(size=(200, 3)), rng.normal(size=(200, 3)))
    sp = ctx(shp, 10)
    f, tq, out, nc = run_device(sp, case, 1000.0, 1.25, mask=mask, groupbit=2, f0=f0)
    ref = W.wall_forces(ref_shapes(sp, shp), 10, case["x"], case["quat"], case["shtype"], case["planes"], [1000.0] * 7, [1.25] * 7,
                        mask=mask, groupbit=2)
    off = mask == 1
    assert np.array_equal(f[off], f0[0][off]) and np.array_equal(tq[off], f0[1][off])   # masked rows: not a bit changed
    check_against_ref((f - f0[0], tq - f0[1], out, nc), ref, "groupbit")   # the forces are ADDED to what was there
    # a bed with no wall in reach: f untouched, no contact
    far = dict(case, planes=box_planes(6.0, cut=-30.0) + np.array([0, 0, 0, -20.0]))
    f, tq, out, nc = run_device(sp, far, 1000.0, 1.25, f0=f0)
    assert nc == 0 and np.array_equal(f, f0[0]) and np.array_equal(tq, f0[1]) and not out.any()
    sp.close()


def test_centre_behind_a_plane_is_an_error_and_the_rest_is_right(oracle):
    import torch
    import wall_ref as W
    from shpair import shapes
    from shpair.capi import ShPairError
    shp = [(4, shapes.random_shape(4, 11, amp=0.1))]
    case = box_case(6, 100, 5.0, 1)
    case["planes"] = case["planes"][:6]
    case["x"][17] = [-0.1, 2.0, 2.0]     # behind wall 0
    case["x"][18] = [2.0, 0.0, 0.4]      # exactly on wall 2, and touching the floor
    sp = ctx(shp, 10)
    n = case["n"]
    sp.set_walls(case["planes"], 1000.0, 1.25)
    x, q, sh, m = dev(case["x"]), dev(case["quat"]), dev(case["shtype"]), dev(np.ones(n, dtype=np.int32))
    f, tq = dev(np.zeros((n, 3))), dev(np.zeros((n, 3)))
    sp.wall_force_device(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    torch.cuda.synchronize()
    with pytest.raises(ShPairError, match="particle centre behind a wall") as e:
        sp.wall_stats()
    assert e.value.code == -1   # SHPAIR_EINVAL
    sp.synchronize()            # the error word was read and cleared
    ref = W.wall_forces(ref_shapes(sp, shp), 10, case["x"], case["quat"], case["shtype"], case["planes"], [1000.0] * 6, [1.25] * 6)
    assert ref["nbehind"] == 2 and ref["f"][18, 2] > 0
    scale = np.abs(ref["f"]).max()
    assert np.abs(f.cpu().numpy() - ref["f"]).max() <= GATE * scale and np.abs(tq.cpu().numpy() - ref["torque"]).max() <= GATE * scale
    # the host form reports it itself
    with pytest.raises(ShPairError, match="particle centre behind a wall"):
        sp.wall_force(case["x"], case["quat"], case["shtype"])
    sp.close()


def test_set_walls_argument_checks():
    from shpair import shapes
    from shpair.capi import ShPairError
    sp = ctx([(0, shapes.sphere(1.0))], 8)
    ok = [[0, 0, 1, 0.0]]
    for planes, kn, ex in (([[0, 0, 1.0 + 1e-9, 0.0]], 1.0, 1.0), ([[0, 0, 0, 0.0]], 1.0, 1.0), ([[0, 0, 1, np.nan]], 1.0, 1.0),
                           ([[np.inf, 0, 0, 0.0]], 1.0, 1.0), (ok, -1.0, 1.0), (ok, np.nan, 1.0), (ok, 1.0, 0.5), (ok, 1.0, np.inf),
                           (ok * 33, 1.0, 1.0)):
        with pytest.raises(ShPairError) as e:
            sp.set_walls(planes, kn, ex)
        assert e.value.code == -1
    sp.set_walls(ok * 32, 1.0, 1.0)
    assert sp.nwalls == 32
    sp.set_walls(None)
    assert sp.nwalls == 0 and sp.wall_stats() == 0
    sp.close()


# ---- steps ---------------------------------------------------------------------------------------------------------

def _settling_case(n_side, L):
    from shpair import bed
    rng = np.random.default_rng(12)
    g = (np.arange(n_side) + 0.5) * (L / n_side)
    x = np.stack(np.meshgrid(g, g, g[: max(1, n_side - 1)], indexing="ij"), axis=-1).reshape(-1, 3)
    x += rng.uniform(-0.05, 0.05, x.shape)
    return x, bed.random_quaternions(x.shape[0], rng)


def _state(r):
    n = r.n
    return [t.cpu().numpy().copy() for t in (r.x[:n], r.v, r.q[:n], r.L, r.f[:n], r.tq[:n])]


def test_run_loops_with_walls_are_bitwise_identical(oracle):
    """(a) shstep_run_device plain, with hipGraph replay, and the call-by-call Python loop: the same bits over 50 steps
    under the deterministic option.  (b) nwalls = 0 is bitwise a context on which shstep_set_walls was never called."""
    from shpair import shapes
    from shpair.run import DeviceRun
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    L = 8.4
    x, quat = _settling_case(4, L)
    x[:, 2] -= 0.15   # the lowest layer reaches into the floor, the outer columns into the side walls
    sht = np.zeros(x.shape[0], np.int32)
    walls = (box_planes(L, cut=-10.0)[:6], 2000.0, 1.25)

    def go(mode, walls):
        sp = ctx(shp, 10, kn=2000.0, deterministic=1)
        r = DeviceRun(sp, x, quat, sht, (0, 0, 0), (L, L, L), (0, 0, 0), 0.3, dt=5e-4, gravity=(0.0, 0.0, -9.81), gamma_t=0.2,
                      gamma_r=0.1, walls=walls)
        if mode == "python":
            r.run(50)
        else:
            r.run_native(50, use_graph=(mode == "graph"))
        import torch
        torch.cuda.synchronize()
        st, nc = _state(r), sp.wall_stats()
        sp.close()
        return st, nc
    ref, nc = go("python", walls)
    assert nc > 0 and np.abs(ref[1]).max() > 0
    for mode in ("plain", "graph"):
        got, nc2 = go(mode, walls)
        assert nc2 == nc
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), mode
    never, _ = go("graph", None)
    removed, _ = go("graph", (None, None, None))
    for a, b in zip(never, removed):
        assert np.array_equal(a, b)
    assert not np.array_equal(never[0], ref[0])   # ... and the walls did act in (a)


def test_sphere_bounces_back_to_its_drop_height(oracle):
    """(c) One unit sphere, kn = 1e4, m = 1.25, g = 9.81, dropped from rest with its centre 1.5 above a floor, dt = 1e-4,
    n_q = 16: the contact conserves energy, so the rebound peak recovers the drop height, (peak - 1)/(1.5 - 1) within
    1 % (a 1-D numpy prototype of this case: 1.00096), and the deepest centre height is 0.9503 within 1e-3."""
    import torch
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = ctx([(0, shapes.sphere(1.0))], 16, kn=1e4, expo=1.25, rmax=[1.01])
    r = DeviceRun(sp, np.array([[0.0, 0.0, 1.5]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (-5, -5, 0), (5, 5, 10),
                  (0, 0, 0), 0.5, dt=1e-4, gravity=(0.0, 0.0, -9.81), walls=([[0, 0, 1, 0.0]], 1e4, 1.25), check=False)
    zs = []
    for _ in range(9000):   # 0.9 s: fall 0.32 s, contact, rise 0.32 s, and past the peak
        r.step()
        zs.append(r.x[0, 2].clone())
    z = torch.stack(zs).cpu().numpy()
    sp.synchronize()        # no error bit
    kmin = int(np.argmin(z))
    peak = z[kmin:].max()
    print(f"deepest centre height {z[kmin]:.5f} at step {kmin}, rebound peak {peak:.5f}, recovered {(peak - 1) / 0.5:.5f}")
    assert kmin + 1 < np.argmax(z[kmin:]) + kmin < len(z) - 1   # the peak lies inside the run
    assert abs(z[kmin] - 0.9503) <= 1e-3
    assert abs((peak - 1.0) / 0.5 - 1.0) <= 1e-2
    sp.close()


def test_bed_settles_in_a_box_and_the_floor_carries_its_weight(oracle):
    """(d) 200 L = 4 particles released in a box with gravity and viscous damping: no error bit, every centre stays inside
    every plane, the kinetic energy ends below its peak, and once it has fallen below 1e-6 of the peak the summed normal
    force on the floor balances the total weight within 5 % (the bar is the static balance, the margin the residual motion).

    Why n_q = 128 and a drop of one unit.  The sharp rule leaves S_n a tangential part of relative size eps (SPEC §2.9:
    ~2e-3 at n_q = 16), so a particle at rest on a frictionless floor feels a steady sideways force eps m g and drifts at
    eps g / gamma under the drag gamma v, while the fall cannot be faster than g / gamma: the kinetic energy cannot sink
    below ~eps^2 of its peak.  Measured plateaus of KE / peak on this bed: 1.6e-4 at n_q = 16 (drop 0.3), 2.3e-6 at 48,
    6.9e-7 at 64, 3.2e-7 at 96 (drop 1.0, reached after ~20 000 steps of 5e-4).  One particle alone drifts at 1.9e-2
    (n_q = 16) and 1.5e-3 (n_q = 48).  The floor carried 0.995 ... 1.009 of the weight in every one of those runs."""
    import torch
    from shpair import shapes
    from shpair.run import DeviceRun
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    sp = ctx(shp, 128, kn=2e4, expo=1.25, deterministic=1)
    mass, rm = sp.body(0)[0], sp.rmax(0)
    rng = np.random.default_rng(8)
    a = 2.0 * rm + 0.1                        # no bounding spheres overlap at the start: nothing but gravity feeds the bed
    L = 15 * a                                # one layer, 200 sites of a 15 x 15 grid, released 1.0 above the floor
    g = (np.arange(15) + 0.5) * a
    x = np.stack(np.meshgrid(g, g, [rm + 1.0], indexing="ij"), axis=-1).reshape(-1, 3)[:200]
    x += rng.uniform(-0.04, 0.04, x.shape)
    n = x.shape[0]
    assert n == 200
    from shpair import bed
    quat = bed.random_quaternions(n, rng)
    planes = np.array([[1, 0, 0, 0], [-1, 0, 0, -L], [0, 1, 0, 0], [0, -1, 0, -L], [0, 0, 1, 0]], dtype=np.float64)
    r = DeviceRun(sp, x, quat, np.zeros(n, np.int32), (0, 0, 0), (L, L, 30.0), (0, 0, 0), 0.3, dt=5e-4, gravity=(0.0, 0.0, -9.81),
                  gamma_t=3.0 * mass, gamma_r=2.0 * mass, walls=(planes, 2e4, 1.25))
    out = torch.zeros(5, 4, dtype=torch.float64, device="cuda:0")

    def floor_force():
        out.zero_()
        f, tq = torch.zeros_like(r.f), torch.zeros_like(r.tq)
        torch.cuda.synchronize()
        sp.wall_force_device(n, r.x.data_ptr(), r.q.data_ptr(), r.sh.data_ptr(), r.mask.data_ptr(), f.data_ptr(), tq.data_ptr(),
                             wall_out=out.data_ptr(), stream=sp.own_stream())
        sp.synchronize()
        return -float(out[4, 3].item())   # the force ON the floor points down: its normal component, sign flipped
    ke_peak, ke, steps, reached = 0.0, 0.0, 0, None
    weight = n * mass * 9.81
    while steps < 30000:
        r.run_native(500, use_graph=True)
        steps += 500
        e = r.energies()
        ke = e[1] + e[2]
        ke_peak = max(ke_peak, ke)
        h = r.x[:n].cpu().numpy() @ planes[:, :3].T - planes[:, 3]
        assert (h > 0).all()
        if steps % 3000 == 0:
            vn = np.linalg.norm(r.v.cpu().numpy(), axis=1)
            print(f"  step {steps}: KE {ke:.3e} (rotational {e[2]:.1e}, peak {ke_peak:.3e}), max|v| {vn.max():.1e}, "
                  f"{(vn > 0.1 * vn.max()).sum()} particles above a tenth of it")
        if ke < 1e-6 * ke_peak:
            reached = steps
            break
    fz = floor_force()
    print(f"steps {steps}, KE/peak {ke / ke_peak:.2e}, floor force / weight {fz / weight:.4f}, wall contacts {sp.wall_stats()}")
    assert ke < ke_peak
    assert reached is not None, f"KE/peak only {ke / ke_peak:.2e} after {steps} steps; floor force / weight {fz / weight:.4f}"
    assert abs(fz / weight - 1.0) <= 0.05
    sp.close()


# ---- two ranks on one GPU ------------------------------------------------------------------------------------------

def test_two_ranks_with_a_floor_match_the_single_domain():
    """Two rank threads on one GPU (the pattern of tests/test_gpu_mrank.py), a floor and a lid under both domains:
    decomposed forces == single-domain forces at that file's tolerance (1e-12 of the largest force)."""
    from shpair import shapes, mrank, bed
    from mrank_common import _run_ranks, _distribute
    lmax, nq, skin = 4, 8, 0.2
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
    walls = (np.array([[0, 0, 1, zmin - 0.7], [0, 0, -1, -(zmax + 0.7)]]), 400.0, 1.25)
    sp0 = ctx(shp, nq, kn=400.0)
    cut = 2.0 * max(sp0.rmax(s) for s in range(2)) + skin
    sp0.close()
    res = {}
    for grid in ((1, 1, 1), (2, 1, 1)):
        world = int(np.prod(grid))
        xw, owner = _distribute(grid, lo, hi, periodic, cut, x)
        hub = mrank.Hub(world) if world > 1 else None

        def body(rank):
            sp = ctx(shp, nq, kn=400.0)
            halo = mrank.Halo(sp, rank, world, grid, lo, hi, periodic, skin, hub=hub)
            mine = owner == rank
            run = mrank.RankRun(sp, halo, xw[mine], quat[mine], sht[mine], tag[mine], dt=0.0, walls=walls)
            t, _, _, _, f, tq = run.owned()
            nc = sp.wall_stats()
            halo.close()
            sp.close()
            return t, f, tq, nc
        parts = _run_ranks(world, body)
        f, tq = np.zeros((n, 3)), np.zeros((n, 3))
        for t, pf, ptq, _ in parts:
            f[t], tq[t] = pf, ptq
        res[grid] = (f, tq, sum(p[3] for p in parts))
        if hub is not None:
            hub.close()
    (f1, t1, c1), (f2, t2, c2) = res[(1, 1, 1)], res[(2, 1, 1)]
    scale = np.abs(f1).max()
    print(f"wall contacts {c1} / {c2}, max|F| {scale:.4g}, decomposed vs single: f {np.abs(f1 - f2).max() / scale:.1e} torque {np.abs(t1 - t2).max() / scale:.1e}")
    assert c1 == c2 and c1 > 0
    assert np.abs(f1 - f2).max() <= 1e-12 * scale and np.abs(t1 - t2).max() <= 1e-12 * scale
