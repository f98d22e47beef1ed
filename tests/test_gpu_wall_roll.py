"""GPU tests of the rolling and twisting resistance at planar walls of docs/SPEC.md §2.17 (csrc/wall_roll_kernels.hpp,
through the C ABI of include/shstep.h) against tests/wall_roll_ref.py at the walls' bar: parity on a bed in a box of six
planes, the mask's top bit, one wall, stale rows, every instance of the contact kernel in turn, off is off, refusals, the
ledger, and the three run loops on a rolling and a spinning particle.

The bed, its motion and the coefficients were chosen on the CPU, with the reference alone, so that the condition
test_the_bed_takes_every_branch asserts on the INPUTS holds at both (L, n_q)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dissipation_common import dev, _wall_ctx   # noqa: E402

TOL = 1e-9            # tests/test_gpu_wall_history.py's
DT = 1e-3
NBED, LBOX = 301, 5.2   # two blocks of 256 rows, the second one ragged
KN, EXPO = 1000.0, 1.25
CONFIGS = [(4, 10), (6, 16)]
# per wall of the box: rolling on five of the six walls, twisting on five, one wall with each kind alone
MUR, GR = np.array([0.05, 0.05, 0.05, 0.0, 0.05, 0.05]), np.array([4.0, 4.0, 4.0, 4.0, 4.0, 4.0])
MUTW, GTW = np.array([0.03, 0.03, 0.0, 0.03, 0.03, 0.03]), np.array([2.5, 2.5, 2.5, 2.5, 2.5, 2.5])
_cache = {}


def _shape(lmax):
    from shpair import shapes
    return shapes.random_shape(lmax, 21, amp=0.15)


def _planes():
    from test_gpu_wall import box_planes
    return box_planes(LBOX)[:6]


def _bed():
    """NBED particles in the box [0, LBOX]^3, no centre nearer than 0.72 to a plane: a third of them near a face, a dozen in
    an edge (two planes) and a dozen in a corner (three planes), the rest in the bulk or just within reach (V <= 0 occurs).
    Every 7th particle is outside the group, every 5th has omega = 0; |omega| spreads over three decades."""
    if "bed" not in _cache:
        from shpair import bed
        rng = np.random.default_rng(17)
        x = rng.uniform(0.72, LBOX - 0.72, size=(NBED, 3))
        for k in range(12):                                      # edges and corners, at either end of the axes
            side = lambda: rng.uniform(0.74, 0.9) if rng.random() < 0.5 else LBOX - rng.uniform(0.74, 0.9)
            x[10 + k] = [side(), side(), rng.uniform(1.5, LBOX - 1.5)]
            x[40 + k] = [side(), side(), side()]
        quat = bed.random_quaternions(NBED, rng)
        tw = np.concatenate([0.3 * rng.normal(size=(NBED, 3)), rng.normal(size=(NBED, 3)) * 10.0 ** rng.uniform(-2, 1, size=(NBED, 1))],
                            axis=1)
        tw[::5, 3:] = 0.0
        mask = np.ones(NBED, np.int32)
        mask[::7] = 2                                            # another group's bit
        _cache["bed"] = (x, quat, tw, mask)
    return _cache["bed"]


def _rmax(lmax):
    from shpair import capi
    return capi.shape_default_rmax(lmax, _shape(lmax))


def _sums(lmax, nq):
    """The per-(particle, wall) sums of the bed from the reference: computed once per (L, n_q), shared by every test."""
    import wall_roll_ref as WR
    if ("sums", lmax, nq) not in _cache:
        x, quat, _, mask = _bed()
        _cache[("sums", lmax, nq)] = WR.reach_sums([(lmax, _shape(lmax), _rmax(lmax))], nq, x, quat, np.zeros(NBED, int), _planes(),
                                                   mask=mask)
    return _cache[("sums", lmax, nq)]


def _reference(lmax, nq, n=NBED, **kw):
    import wall_roll_ref as WR
    x, _, tw, _ = _bed()
    sums = {k: v for k, v in _sums(lmax, nq).items() if k[0] < n}
    nw = 6
    return WR.wall_roll(sums, n, x, tw, _planes(), np.full(nw, KN), np.full(nw, EXPO), kw.pop("mur", MUR), kw.pop("gr", GR),
                        kw.pop("mutw", MUTW), kw.pop("gtw", GTW), **kw)


def _ctx(lmax, nq, det=0, roll=True, planes=None):
    sp = _wall_ctx([(lmax, _shape(lmax))], nq, kn=KN, expo=EXPO, deterministic=det)
    sp.set_walls(_planes() if planes is None else planes, KN, EXPO)
    if roll:
        sp.wall_rolling(MUR, GR)
        sp.wall_twisting(MUTW, GTW)
    return sp


def _pass(sp, x, quat, tw, mask, nwalls, dt=None, want_out=True):
    """One wall pass on fresh arrays: f, torque [n][3], wall_out [nw][4] (zeros where it is not asked for)."""
    import torch
    n = len(x)
    xd, qd, sh, m, twd = dev(x), dev(quat), dev(np.zeros(n, np.int32)), dev(np.asarray(mask, np.int32)), dev(tw)
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    out = torch.zeros(nwalls, 4, dtype=torch.float64, device="cuda:0")
    a = (n, xd.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), twd.data_ptr())
    kw = dict(wall_out=out.data_ptr() if want_out else None)
    if dt is None:
        sp.wall_force_damped_device(*a, **kw)
    else:
        sp.wall_contact_device(*a, dt, **kw)
    torch.cuda.synchronize()
    sp.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy()


def _bed_pass(sp, n=NBED, **kw):
    x, quat, tw, mask = _bed()
    return _pass(sp, x[:n], quat[:n], tw[:n], mask[:n], 6, **kw)


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


# ---- 1. the inputs ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lmax,nq", CONFIGS)
def test_the_bed_takes_every_branch(oracle, lmax, nq):
    """A condition on the inputs, read from the reference alone: each of the four branches on at least 5 contacts, particles
    on two and on three planes, walls within reach with V <= 0, particles outside the group, particles at rest."""
    import wall_roll_ref as WR
    ref = _reference(lmax, nq)
    counts = WR.branch_counts(ref["branch"])
    sums = _sums(lmax, nq)
    touching = {}
    for (i, w), (V, _, _) in sums.items():
        touching[i] = touching.get(i, 0) + (V > 0)
    x, _, tw, mask = _bed()
    dry = sum(1 for v in sums.values() if not v[0] > 0)
    rel = max(abs(ref["N"][k] - ref["NS"][k]) / ref["N"][k] for k in sums if ref["N"][k] > 0)
    print(f"L={lmax} nq={nq}: {len(sums)} (particle, wall) rows, {sum(touching.values())} contacts, {dry} within reach with V <= 0, "
          f"{sum(v == 2 for v in touching.values())} particles on two planes, {sum(v == 3 for v in touching.values())} on three; "
          f"branches {counts}; max |N - p_tot|S_n|| / N = {rel:.3e}")
    assert all(v >= 5 for v in counts.values()), counts
    assert sum(v == 2 for v in touching.values()) >= 3 and sum(v == 3 for v in touching.values()) >= 3 and dry >= 3
    assert (mask == 2).sum() >= 20 and not any(mask[i] == 2 for i, _ in sums)
    assert sum(1 for i in touching if touching[i] and not tw[i, 3:].any()) >= 5
    assert rel <= 0.05                                          # the two definitions of the load differ by the quadrature only


# ---- 2. parity, off is off, deterministic ------------------------------------------------------------------------------------

@pytest.mark.parametrize("lmax,nq", CONFIGS)
def test_the_bed_matches_the_reference_and_the_force_keeps_its_bits(oracle, lmax, nq):
    ref = _reference(lmax, nq)
    sp = _ctx(lmax, nq, roll=False)
    assert sp.rmax(0) == _rmax(lmax)
    parent = _bed_pass(sp)                                      # no coefficient was ever set: the parent's pass
    sp.wall_rolling(MUR, GR)
    sp.wall_twisting(MUTW, GTW)
    assert sp.has_wall_rolling
    got = _bed_pass(sp)
    nc = sp.wall_stats()
    noout = _bed_pass(sp, want_out=False)                       # the pass keeps its rows whether or not wall_out is asked for
    sp.wall_rolling(0.0, 0.0)
    sp.wall_twisting(0.0, 0.0)
    assert not sp.has_wall_rolling
    back = _bed_pass(sp)
    sp.close()
    sp = _ctx(lmax, nq, det=1)
    det = _bed_pass(sp)
    sp.close()
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    et = np.abs(got[1] - ref["torque"]).max() / tscale
    ec = np.abs((got[1] - parent[1]) - ref["couple"]).max() / np.abs(ref["couple"]).max()
    print(f"L={lmax} nq={nq}: {nc} contacts, max|F| {scale:.4g} max|tau| {np.abs(ref['torque']).max():.4g} max|M| {np.abs(ref['couple']).max():.4g}; "
          f"rel err torque {et:.1e}, of the couple alone {ec:.1e}")
    assert nc == sum(1 for v in _sums(lmax, nq).values() if v[0] > 0) and scale > 0
    assert np.abs(parent[0] - ref["f"]).max() <= TOL * scale and np.abs(parent[2][:, 1:] - ref["wall_out"][:, 1:]).max() <= TOL * scale
    assert et <= TOL
    assert ec <= TOL * tscale / np.abs(ref["couple"]).max()     # (a difference of two torques: the bar, over max|M| / max|tau|)
    assert np.array_equal(got[0], parent[0]) and np.array_equal(got[2], parent[2])       # f and wall_out: bit for bit
    moved = (got[1] != parent[1]).any(axis=1)
    assert moved.sum() >= 20 and np.array_equal(moved, ref["couple"].any(axis=1))        # exactly the rows the reference moves
    assert np.array_equal(noout[0], got[0]) and np.array_equal(noout[1], got[1]) and not noout[2].any()
    assert _same(back, parent)                                  # set and zeroed again: the parent's bits
    assert _same(det, got)                                      # the same bits with and without "deterministic"


# ---- 3. the mask's top bit, one wall -------------------------------------------------------------------------------------------

def test_a_contact_on_wall_31_of_32_and_a_single_wall(oracle):
    import wall_roll_ref as WR
    lmax, nq = 4, 10
    floor = np.array([0.0, 0.0, 1.0, 0.0])
    x, q = np.array([[3.0, 3.0, 0.8], [6.0, 3.0, 0.85]]), np.array([[0.5, 0.5, -0.5, 0.5], [1.0, 0, 0, 0]])
    tw = np.array([[0.1, 0.0, -0.1, 0.3, -0.2, 0.8], [0.0, 0.2, 0.0, -5.0, 4.0, 9.0]])
    shp = [(lmax, _shape(lmax), _rmax(lmax))]
    for nw in (32, 1):
        planes = np.array([[0.0, 0.0, 1.0, -50.0 - k] for k in range(nw - 1)] + [floor])     # 31 planes far below, the floor last
        sums = WR.reach_sums(shp, nq, x, q, np.zeros(2, int), planes)
        assert set(sums) == {(0, nw - 1), (1, nw - 1)}
        z = np.zeros(nw)
        mur, gr, mutw, gtw = z + 0.05, z + 40.0, z + 0.03, z + 25.0
        ref = WR.wall_roll(sums, 2, x, tw, planes, z + KN, z + EXPO, mur, gr, mutw, gtw)
        sp = _ctx(lmax, nq, roll=False, planes=planes)
        parent = _pass(sp, x, q, tw, np.ones(2), nw)
        sp.wall_rolling(0.05, 40.0)                             # scalars: one value for every wall
        sp.wall_twisting(0.03, 25.0)
        got = _pass(sp, x, q, tw, np.ones(2), nw)
        sp.close()
        scale = max(np.abs(ref["f"]).max(), np.abs(ref["torque"]).max())
        assert ref["couple"][0].any() and ref["couple"][1].any()
        assert {b for br in ref["branch"].values() for b in br} == {WR.VISCOUS, WR.CAPPED}
        assert np.abs(got[1] - ref["torque"]).max() <= TOL * scale
        assert np.array_equal(got[0], parent[0]) and np.array_equal(got[2], parent[2]) and not np.array_equal(got[1], parent[1])


# ---- 4. stale rows ---------------------------------------------------------------------------------------------------------------

def test_rows_of_an_earlier_call_and_of_another_nlocal_are_never_read(oracle):
    """The same context sees the bed, then the bed with its lower half lifted out of the floor's reach, then its first 130 rows:
    each result has the bits of a context that saw nothing before."""
    lmax, nq = 4, 10
    x, quat, tw, mask = _bed()
    lifted = x.copy()
    low = x[:, 2] < 1.3
    lifted[low, 2] = 2.0 + 0.3 * (np.arange(NBED)[low] % 3)
    assert low.sum() >= 30
    calls = [(x, NBED), (lifted, NBED), (x, 130), (lifted, NBED)]
    sp = _ctx(lmax, nq)
    got = [_pass(sp, xx[:n], quat[:n], tw[:n], mask[:n], 6) for xx, n in calls]
    sp.close()
    for k, (xx, n) in enumerate(calls[1:], 1):
        sp = _ctx(lmax, nq)
        fresh = _pass(sp, xx[:n], quat[:n], tw[:n], mask[:n], 6)
        sp.close()
        assert _same(got[k], fresh), k
    assert not np.array_equal(got[0][1], got[1][1])
    ref = _reference(lmax, nq, n=130)
    assert np.abs(got[2][1] - ref["torque"]).max() <= TOL * max(np.abs(ref["f"]).max(), np.abs(ref["torque"]).max())


# ---- 5. N follows the row of every instance ----------------------------------------------------------------------------------------

NSUB = 60
INSTANCES = {
    "damping": dict(gamma=np.full(6, 900.0)),
    "friction": dict(gamma=np.full(6, 900.0), mu=np.full(6, 0.4), gt=np.full(6, 30.0)),
    "spring": dict(gamma=np.full(6, 900.0), mu=np.full(6, 0.4), gt=np.full(6, 5.0), kt=np.full(6, 2000.0), dt=DT),
    "moving": dict(gamma=np.full(6, 900.0), mu=np.full(6, 0.4), gt=np.full(6, 30.0),
                   vel=np.array([[0, 0.7, 0.2], [0.1, 0, 0], [0, 0, -0.5], [0, 0, 0], [0.6, -0.3, 0.15], [0.2, 0.2, -0.1]], float)),
    "moving_elastic": dict(vel=np.array([[0, 0.7, 0.2], [0.1, 0, 0], [0, 0, -0.5], [0, 0, 0], [0.6, -0.3, 0.15], [0.2, 0.2, -0.1]], float)),
}


@pytest.mark.parametrize("name", list(INSTANCES))
def test_the_load_follows_the_row_of_every_instance_and_u_w_stays_out_of_omega(oracle, name):
    lmax, nq = 4, 10
    opt = dict(INSTANCES[name])
    ref = _reference(lmax, nq, n=NSUB, **opt)
    plain = _reference(lmax, nq, n=NSUB)
    sp = _ctx(lmax, nq, roll=False)
    if "gamma" in opt:
        sp.wall_damping(opt["gamma"])
    if "mu" in opt:
        sp.wall_friction(opt["mu"], opt["gt"])
    if "kt" in opt:
        sp.set_wall_tangential_spring(opt["kt"])
    if "vel" in opt:
        sp.wall_velocity(opt["vel"])
    dt = opt.get("dt")
    off = _bed_pass(sp, n=NSUB, dt=dt)
    if dt is not None:
        sp.reset_wall_history()                                 # the second pass starts from nothing live too
    sp.wall_rolling(MUR, GR)
    sp.wall_twisting(MUTW, GTW)
    got = _bed_pass(sp, n=NSUB, dt=dt)
    sp.close()
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ef, et = np.abs(got[0] - ref["f"]).max() / scale, np.abs(got[1] - ref["torque"]).max() / tscale
    dN = max(abs(ref["N"][k] - plain["N"][k]) / plain["N"][k] for k in plain["N"] if plain["N"][k] > 0)
    print(f"{name}: rel err f {ef:.1e} torque {et:.1e}; the loads differ from the elastic ones by up to {dN:.2e}; "
          f"max|M| {np.abs(ref['couple']).max():.4g} against {np.abs(plain['couple']).max():.4g}")
    assert ef <= TOL and et <= TOL
    assert np.array_equal(got[0], off[0]) and np.array_equal(got[2], off[2])
    if name == "moving_elastic":                                # no coefficient reads u_w: the elastic rows, and Omega = omega_i
        assert np.array_equal(ref["couple"], plain["couple"])
    else:
        assert dN > 1e-3 and np.abs(ref["couple"] - plain["couple"]).max() > 1e-6 * np.abs(plain["couple"]).max()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(oracle):
    import torch
    from shpair import mrank, shapes
    from shpair.capi import ShPairError, HaloArrays, HaloRunParams
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 8)
    for setter in (sp.wall_rolling, sp.wall_twisting):
        with pytest.raises(ShPairError, match="after shstep_set_walls") as e:     # before set_walls
            setter([0.05], [1.0])
        assert e.value.code == -1
    sp.set_walls([[0, 0, 1, 0.0], [1, 0, 0, 0.0]], 1000.0, 1.25)
    for setter in (sp.wall_rolling, sp.wall_twisting):
        for a, b in (([1.0], [1.0]), ([-1.0, 0.0], [1.0, 1.0]), ([0.1, 0.1], [np.nan, 1.0]), ([np.inf, 0.1], [1.0, 1.0]), ([0.1, 0.1], [1.0, -2.0])):
            with pytest.raises(ShPairError) as e:
                setter(a, b)
            assert e.value.code == -1
    t = (np.zeros(2)).ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_double))
    assert sp._lib.shstep_set_wall_rolling(sp._h, 2, None, t) == -1 and sp._lib.shstep_set_wall_twisting(sp._h, 2, t, None) == -1
    assert not sp.has_wall_rolling
    n = 2
    x, q = dev(np.array([[5.0, 5.0, 0.9], [0.9, 5.0, 5.0]])), dev(np.array([[1.0, 0, 0, 0]] * 2))
    sh, m, tw = dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32)), dev(np.ones((n, 6)))
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    a = (n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    sp.wall_rolling([0.05, 0.0], [0.0, 3.0])                    # no wall has both: nothing is on, the old call runs
    assert not sp.has_wall_rolling
    sp.wall_force_device(*a)
    sp.synchronize()
    assert f.any()
    f.zero_(), tq.zero_()
    sp.wall_twisting([0.0, 0.03], [0.0, 3.0])
    assert sp.has_wall_rolling
    with pytest.raises(ShPairError, match="shstep_wall_force_damped_device") as e:
        sp.wall_force_device(*a)
    assert e.value.code == -4
    with pytest.raises(ShPairError, match="shstep_wall_force_damped_device") as e:
        sp.wall_force(np.array([[5.0, 5.0, 0.9]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32))
    assert e.value.code == -4
    with pytest.raises(ShPairError, match="null twist") as e:
        sp.wall_force_damped_device(*a, None)
    assert e.value.code == -1
    assert not f.any() and not tq.any()
    sp.wall_force_damped_device(*a, tw.data_ptr())
    sp.synchronize()
    assert f.any() and tq[1].any()
    # the loop over several ranks refuses without option "halo_twists", as for any wall coefficient
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    with pytest.raises(ShPairError, match="halo_twists") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -1
    sp.set_walls([[0, 0, 1, 0.0]], 1000.0, 1.25)                # set_walls drops the coefficients and the refusals
    assert not sp.has_wall_rolling
    sp.wall_force_device(1, *a[1:])
    sp.synchronize()
    halo.close()
    sp.close()


# ---- 7. the ledger -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["elastic", "friction"])
def test_the_couples_power_goes_into_the_wall_friction_entries(oracle, name):
    """One pass and one fold: with a friction instance writing the power rows, and with the elastic instance writing none."""
    lmax, nq = 4, 10
    opt = dict(INSTANCES["friction"]) if name == "friction" else {}
    ref = _reference(lmax, nq, n=NSUB, **opt)
    sp = _ctx(lmax, nq, roll=False)
    if opt:
        sp.wall_damping(opt["gamma"])
        sp.wall_friction(opt["mu"], opt["gt"])
    sp.set_energy_ledger(True)
    _bed_pass(sp, n=NSUB, want_out=False)
    sp.ledger_fold_device(DT)
    base, base_w = sp.energy_ledger()
    sp.reset_energy_ledger()
    sp.wall_rolling(MUR, GR)
    sp.wall_twisting(MUTW, GTW)
    _bed_pass(sp, n=NSUB, want_out=False)
    sp.ledger_fold_device(DT)
    sp.ledger_fold_device(DT)                                   # a pass is folded once
    tot, per = sp.energy_ledger()
    sp.close()
    want_w = DT * (ref["power"] + ref["pf"]).sum(axis=0)
    want_d = DT * ref["pd"].sum(axis=0)
    print(f"{name}: wall friction {tot[3]:.6e} (reference {want_w.sum():.6e}, of which the couples {DT * ref['power'].sum():.6e}), "
          f"without the resistance {base[3]:.6e}; wall damping {tot[2]:.6e} (reference {want_d.sum():.6e})")
    assert ref["power"].sum() > 0 and (ref["power"].sum(axis=0) > 0).sum() >= 4
    assert abs(tot[3] - want_w.sum()) <= TOL * want_w.sum() and np.abs(per[:, 1] - want_w).max() <= TOL * want_w.max()
    assert abs(tot[2] - want_d.sum()) <= TOL * max(abs(want_d.sum()), want_w.sum()) and tot[2] == base[2] and np.array_equal(per[:, 0], base_w[:, 0])
    assert abs(base[3] - DT * ref["pf"].sum()) <= TOL * want_w.sum() and (name == "friction" or base[3] == 0.0)
    assert tot[0] == 0.0 and tot[1] == 0.0 and tot[4] == 0.0


# ---- 8. the run loops ----------------------------------------------------------------------------------------------------------------

RUN_ROLL, RUN_TWIST = (0.3, 40.0), (0.2, 20.0)
RUN_DT, RUN_KN = 5e-4, 200.0


def _wall_energy(sp, r):
    """E_w = kn V^m of the wall contacts at the current positions: one look of the wall pass into scratch rows."""
    import torch
    out = torch.zeros(1, 4, dtype=torch.float64, device="cuda:0")
    f2, t2 = torch.zeros_like(r.f), torch.zeros_like(r.tq)
    sp.wall_contact_device(r.n, r.x.data_ptr(), r.q.data_ptr(), r.sh.data_ptr(), r.mask.data_ptr(), f2.data_ptr(), t2.data_ptr(),
                           r.twist.data_ptr(), 0.0, wall_out=out.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    return float(out[0, 0].item())


def _scene(mode, nsteps, resist, k=1, ledger=False, chunks=1, drop=False):
    """A near-spherical particle (L = 4, amplitude 0.01) on a floor under gravity, with wall damping, wall friction and a wall
    spring, started rolling without slipping along x; a second one, an exact sphere clear of the first, spins about the floor's
    normal.  Both start near their resting height (the weight of 41 is carried at an overlap of 0.07).  dt = RUN_DT / k;
    n_q = 32 keeps the quadrature noise of the sharp rule at a wall below the first-order term of the balance, as in
    tests/test_gpu_wall_history.py.  Returns omega of both per chunk (the twists of the state the chunk left), the
    state at the end, the ledger and (E_mech at the start, at the end).
    drop: both start clear of the floor, at 1.25, moving down at 1 with the same spins, so that they land on it within the run:
    a smooth roll leaves a first-order term of the balance too small to be told from the quadrature noise (measured on an
    MI355X at n_q = 32, 1500 steps: R = 3.04e-3 at dt and 3.62e-3 at dt / 2 of D = 6.01), an impact does not."""
    import torch
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = _wall_ctx([(4, shapes.random_shape(4, 21, amp=0.01)), (0, shapes.sphere(1.0))], 32, kn=RUN_KN, expo=1.25, rmax=[0.0, 1.01],
                   deterministic=1)
    kw = dict(wall_rolling=RUN_ROLL, wall_twisting=RUN_TWIST) if resist else {}
    h = 1.25 if drop else 0.93
    x = np.array([[2.0, 3.0, h], [6.0, 3.0, h]])
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]] * 2), np.array([0, 1], np.int32), (0, 0, 0), (12, 6, 6), (0, 0, 0), 0.5,
                  dt=RUN_DT / k, gravity=(0.0, 0.0, -9.81), walls=([[0, 0, 1, 0.0]], RUN_KN, 1.25), wall_damping=60.0,
                  wall_friction=(0.5, 5.0), wall_spring=4e3, ledger=ledger, **kw)
    I0, I1 = sp.body(0)[2], sp.body(1)[2]
    r.v[:] = dev(np.array([[1.0 * 0.93, 0.0, -1.0 if drop else 0.0], [0.0, 0.0, -1.0 if drop else 0.0]]))               # omega = (0, 1, 0) and v = omega x (0, 0, 0.93)
    r.L[:] = dev(np.array([[I0[3], I0[1], I0[5]], [0.0, 0.0, 2.0 * I1[2]]]))     # L = I omega: (xy, yy, yz) and 2 I_zz
    r.force()
    torch.cuda.synchronize()
    e = r.energies()
    E0 = e[1] + e[2] + e[3] + _wall_energy(sp, r)
    rows = []
    for _ in range(chunks):
        if mode == "python":
            r.run(nsteps * k // chunks)
        else:
            r.run_native(nsteps * k // chunks, use_graph=(mode == "graph"))
        torch.cuda.synchronize()
        # (the library's loop keeps its twists in the step state: form them here from the state the chunk left, for every mode)
        sp.twist_device(r.n, 0, r.v.data_ptr(), r.q.data_ptr(), r.L.data_ptr(), r.sh.data_ptr(), r.twist.data_ptr())
        torch.cuda.synchronize()
        sp.synchronize()
        tw = r.twist[:2].cpu().numpy()
        rows.append(np.concatenate([tw[0, 3:], tw[1, 3:]]))
    sp.synchronize()
    state = [t.cpu().numpy().copy() for t in (r.x[:2], r.v, r.q[:2], r.L, r.f[:2], r.tq[:2])]
    led = r.ledger() if ledger else None
    e = r.energies()
    E1 = e[1] + e[2] + e[3] + _wall_energy(sp, r)
    sp.close()
    return np.array(rows), state, led, (E0, E1)


def test_the_three_loops_agree_and_the_resistance_brings_both_particles_to_rest(oracle):
    """3000 steps of 5e-4.  The three loops run the same kernels in the same order on the same bits under "deterministic", so they are
    held to equality, which is inside every bar of tests/test_gpu_traj.py.  With the resistance both |omega| fall below 5 % of
    their start and the spinner's |Omega_n| never grows; without it neither particle comes to rest.
    Measured on an MI355X: roller |omega| 0.891 after the first 150 steps, 6.4e-3 at the end (1.047 without the resistance),
    spinner 1.660 and 3.0e-7 (2.000 without)."""
    on = {m: _scene(m, 3000, True, chunks=20) for m in ("python", "plain", "graph")}
    for m in ("plain", "graph"):
        for k, (a, b) in enumerate(zip(on["python"][1], on[m][1])):
            assert np.array_equal(a, b), (m, k)
        assert np.array_equal(on["python"][0], on[m][0]), m
    rows = on["graph"][0]
    off = _scene("graph", 3000, False, chunks=20)[0]
    wr, ws = np.linalg.norm(rows[:, :3], axis=1), np.linalg.norm(rows[:, 3:], axis=1)
    wr0, ws0 = np.linalg.norm(off[:, :3], axis=1), np.linalg.norm(off[:, 3:], axis=1)
    print(f"roller |omega| {wr[0]:.4f} -> {wr[-1]:.3e} (off: {wr0[-1]:.4f}); spinner |omega| {ws[0]:.4f} -> {ws[-1]:.3e} (off: {ws0[-1]:.4f}); "
          f"spinner Omega_z by chunk {np.array2string(rows[:, 5], precision=3)}")
    assert wr[-1] <= 0.05 * 1.0 and ws[-1] <= 0.05 * 2.0
    assert (np.diff(np.abs(rows[:, 5])) <= 1e-12).all()          # |Omega_n| of the spinner never increases
    assert wr0[-1] >= 0.5 * 1.0 and ws0[-1] >= 0.5 * 2.0         # nothing else takes the spin out


def test_the_ledger_is_the_same_under_plain_launches_and_graph_replay_and_the_balance_closes_to_first_order(oracle):
    """E_mech(t) - E_mech(0) = W - D with W = 0 (the floor is at rest): the residual is first order in dt.  The bounds on the
    ratio are those of tests/test_gpu_ledger.py and tests/test_gpu_wall_history.py: at most 0.75 at dt / 2.
    Measured on an MI355X: R = 6.820e-2 and 2.935e-2 (ratio 0.430) of D = 32.18 (wall friction 6.08, of E0 = 113.0)."""
    R = []
    for k in (1, 2):
        plain = _scene("plain", 1500, True, k=k, ledger=True, drop=True)
        graph = _scene("graph", 1500, True, k=k, ledger=True, drop=True)
        lp, lg = plain[2], graph[2]
        for key in ("pair_damping", "pair_friction", "wall_damping", "wall_friction", "wall_work"):
            assert lp[key] == lg[key], key
        assert np.array_equal(lp["per_wall"], lg["per_wall"])
        E0, E1 = graph[3]
        R.append(abs(E1 - E0 + lg["dissipated"] - lg["work"]))
        print(f"dt/{k}: E0 {E0:.6f} E1 {E1:.6f} D {lg['dissipated']:.6f} (wall friction {lg['wall_friction']:.6f}, wall damping "
              f"{lg['wall_damping']:.6f}) W {lg['work']:.3e} R {R[-1]:.3e}")
        assert lg["wall_friction"] > 0 and lg["work"] == 0.0 and lg["pair_damping"] == 0.0 and lg["pair_friction"] == 0.0
    print(f"R(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert R[1] <= 0.75 * R[0]
