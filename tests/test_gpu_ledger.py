"""GPU tests of the energy ledger of docs/SPEC.md §2.13 (the LEDGER instances of csrc/dissipation_kernels.hpp and
csrc/wall_kernels.hpp, csrc/ledger_kernels.hpp, through the C ABI of include/shstep.h) against tests/ledger_ref.py fed by
the ORACLE's per-pair integrals and tests/wall_ref.py's per-contact sums: the powers at the bar the wrench is held to
(1e-9, tests/test_gpu_friction.py — the power is a bilinear form of the same integrals), the ordered sums' bits, the three
loops, the wall work against the host's own sum, the closure of the balance, two ranks, and the ledger switched off."""
import functools
import os
import sys

import numpy as np
import pytest

from common import coeff_tables, oracle_compute
from dissipation_common import NQ, dev, bed_case, motion, ctx, gpu_forces, _total_energy, _wall_ctx

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-9            # tests/test_gpu_friction.py's
GAMMA = {(1, 1): 300.0, (1, 2): 900.0, (2, 2): 1800.0}
FRIC = {(1, 1): (2.0, 300.0), (1, 2): (1.5, 400.0), (2, 2): (2.5, 250.0)}
CHUNK = 2048          # kLedgerChunk: slots per block of the pair fold's first stage


def table(coef, k=None):
    G = np.zeros((3, 3))
    for (a, b), g in coef.items():
        G[a, b] = G[b, a] = g if k is None else g[k]
    return G


# ---- 1. pair powers against the reference ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pair_case(n, seed, expo, nlocal, newton, mseed):
    """The bed, its motion and the oracle's integrals, computed once per bed (the reference is shared and left alone)."""
    from oracle import oracle as O
    import damp_ref as D
    case = bed_case(O, n, seed, nlocal)
    K, E = coeff_tables(2, lambda i, j: 1000.0 + 100.0 * (i + j), expo)
    v, L = motion(case, mseed)
    b = case["bed"]
    o = oracle_compute(O, case, NQ, K, E, nlocal=n if nlocal is None else nlocal, newton_pair=newton, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], case["offsets"], case["jlist"])
    tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
    return case, K, E, v, L, (o["pairs"], pi, pj, b["x"], tw, b["type"], b["shtype"], case["rmax"], K, E)


PAIR = [
    # n, bed seed, exponent, nlocal, newton, which, deterministic, motion seed
    (12, 2, 1.25, None, True, "both", 0, 9),         # fewer than 256 slots
    (60, 1, 1.25, None, True, "damp", 0, 8),
    (60, 1, 1.0, None, True, "fric", 1, 8),
    (60, 1, 1.0, None, True, "both", 0, 8),
    (60, 3, 1.25, 40, False, "both", 0, 10),         # ghost j without newton: the half share
    (60, 3, 1.25, 40, True, "both", 1, 10),
    (1500, 4, 1.25, None, True, "both", 0, 11),      # more slots than one stage-1 block: two partial sums meet
    (1500, 4, 1.25, None, True, "both", 1, 11),
]


@pytest.mark.parametrize("n,seed,expo,nlocal,newton,which,det,mseed", PAIR)
def test_pair_powers_match_the_reference(oracle, n, seed, expo, nlocal, newton, which, det, mseed):
    import ledger_ref as LR
    case, K, E, v, L, a = _pair_case(n, seed, expo, nlocal, newton, mseed)
    npairs = case["jlist"].size
    assert (n != 12 or npairs < 256) and (npairs > CHUNK and npairs % CHUNK != 0) == (n == 1500), npairs
    gamma = GAMMA if which in ("damp", "both") else {}
    fric = FRIC if which in ("fric", "both") else {}
    P = LR.pair_powers(*a, table(gamma), table(fric, 0), table(fric, 1), n if nlocal is None else nlocal, newton_pair=newton)
    ref = P.sum(axis=0)
    sp = ctx(case, K, E, det=det, gamma=gamma, fric=fric)
    sp.set_energy_ledger(True)
    gpu_forces(sp, case, v, L, nlocal, newton)
    sp.ledger_fold_device(1.0)
    tot, _ = sp.energy_ledger()
    sp.ledger_fold_device(1.0)                       # nothing fresh: enqueues nothing
    again, _ = sp.energy_ledger()
    sp.reset_energy_ledger()
    gpu_forces(sp, case, v, L, nlocal, newton)
    sp.ledger_fold_device(1.0)
    second, _ = sp.energy_ledger()
    sp.close()
    scale = ref.sum()
    print(f"n={n} m={expo} nlocal={nlocal} newton={newton} {which} det={det}: {npairs} slots, reference P_d {ref[0]:.6g} P_f {ref[1]:.6g}, "
          f"ledger {tot[0]:.6g} {tot[1]:.6g}, rel err {np.abs(tot[:2] - ref).max() / scale:.1e}")
    assert scale > 0 and bool(gamma) == (ref[0] > 0) and bool(fric) == (ref[1] > 0)
    assert np.abs(tot[:2] - ref).max() <= TOL * scale
    assert not tot[2:].any()
    assert np.array_equal(again, tot) and np.array_equal(second, tot)    # folded once; the same rows give the same bits
    if nlocal is not None and not newton:
        full = LR.pair_powers(*a, table(gamma), table(fric, 0), table(fric, 1), n, newton_pair=True).sum()
        assert ref.sum() < 0.999 * full                                  # the half share did count


def test_deterministic_and_atomic_modes_give_the_same_ledger_bits(oracle):
    case, K, E, v, L, _ = _pair_case(1500, 4, 1.25, None, True, 11)
    out = []
    for det in (0, 1):
        sp = ctx(case, K, E, det=det, gamma=GAMMA, fric=FRIC)
        sp.set_energy_ledger(True)
        gpu_forces(sp, case, v, L)
        sp.ledger_fold_device(0.37)
        out.append(sp.energy_ledger()[0])
        sp.close()
    assert out[0][:2].all() and np.array_equal(out[0], out[1])


# ---- 2. wall powers and work against the reference -------------------------------------------------------------------

WALL_N = 17       # 17 x 17 = 289 particles in one layer over the floor: two blocks of the row reduce


@functools.lru_cache(maxsize=None)
def _wall_case():
    from oracle import oracle as O
    from shpair import shapes, bed
    import wall_ref as W
    anm = shapes.random_shape(4, 21, amp=0.15)
    rmax = O.shape_rmax(4, anm)
    rng = np.random.default_rng(5)
    g = np.arange(WALL_N) * 2.3
    x = np.stack(np.meshgrid(g + 0.8, g + 1.5, [0.8], indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.05, 0.05, (WALL_N ** 2, 3))
    n = x.shape[0]
    quat = bed.random_quaternions(n, rng)
    tw = np.concatenate([rng.normal(size=(n, 3)), 0.5 * rng.normal(size=(n, 3))], axis=1)
    planes = np.array([[0.0, 0, 1, 0.0], [1.0, 0, 0, 0.0]])
    cache = {}
    sums = W.wall_sums

    def cached(lmax, a, r, xi, qi, plane, nq):      # the per-contact sums do not depend on the coefficients: once per contact
        key = (xi.tobytes(), np.asarray(plane, float).tobytes(), nq)
        if key not in cache:
            cache[key] = sums(lmax, a, r, xi, qi, plane, nq)
        return cache[key]
    return dict(shp=[(4, anm)], shapes=[(4, anm, rmax)], x=x, quat=quat, tw=tw, planes=planes, n=n, sums=cached)


WALL = {
    # gamma_w, (mu_w, gamma_t,w), u_w
    "elastic_moving": (None, None, [[0.3, 0.0, 0.5], [0.2, 1.0, 0.0]]),
    "damped": ([400.0, 250.0], None, None),
    "friction": ([0.0, 250.0], ([0.5, 0.3], [200.0, 400.0]), None),
    "moving_damped": ([400.0, 250.0], None, [[0.3, 0.0, 0.5], [0.2, 1.0, 0.0]]),
    "moving_friction": ([400.0, 250.0], ([0.5, 0.3], [200.0, 400.0]), [[0.3, 0.0, 0.5], [0.2, 1.0, 0.0]]),
}
WALL_KN, WALL_EXPO, WALL_DT = np.array([1000.0, 800.0]), np.array([1.25, 1.0]), 0.5


def _wall_ledger(c, name, want_out, det=0):
    import torch
    gamma, fric, vel = WALL[name]
    sp = _wall_ctx(c["shp"], NQ, deterministic=det)
    sp.set_walls(c["planes"], WALL_KN, WALL_EXPO)
    if gamma is not None:
        sp.wall_damping(gamma)
    if fric is not None:
        sp.wall_friction(*fric)
    if vel is not None:
        sp.wall_velocity(vel)
    sp.set_energy_ledger(True)
    n = c["n"]
    xd, qd, sh, m, twd = dev(c["x"]), dev(c["quat"]), dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32)), dev(c["tw"])
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    out = torch.zeros(2, 4, dtype=torch.float64, device="cuda:0")
    sp.wall_force_damped_device(n, xd.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                twd.data_ptr() if sp.wall_reads_twists else None, wall_out=out.data_ptr() if want_out else None)
    sp.ledger_fold_device(WALL_DT)
    tot, per = sp.energy_ledger()
    nc = sp.wall_stats()
    sp.close()
    return tot, per, out.cpu().numpy(), f.cpu().numpy(), nc


@pytest.mark.parametrize("name", list(WALL))
def test_wall_powers_and_work_match_the_reference(oracle, name, monkeypatch):
    import ledger_ref as LR
    c = _wall_case()
    monkeypatch.setattr(LR.W, "wall_sums", c["sums"])
    gamma, fric, vel = WALL[name]
    g = np.zeros(2) if gamma is None else np.array(gamma)
    mu, gt = (np.zeros(2), np.zeros(2)) if fric is None else (np.array(fric[0]), np.array(fric[1]))
    P, Fw = LR.wall_powers(c["shapes"], NQ, c["x"], c["quat"], np.zeros(c["n"], np.int32), c["tw"], c["planes"], WALL_KN, WALL_EXPO, g, mu,
                           gt, vel)
    per_ref, tot_ref = LR.wall_ledger(P, Fw, vel, WALL_DT)
    z = np.zeros(2)
    _, Fe = LR.wall_powers(c["shapes"], NQ, c["x"], c["quat"], np.zeros(c["n"], np.int32), None, c["planes"], WALL_KN, WALL_EXPO, z, z, z, None)
    touched = (Fe != 0).any(axis=2)                 # the elastic contact: V > 0 (a clamped contact carries no force)
    assert touched[:, 0].sum() > 256 and touched[:, 1].sum() >= 10 and (touched[:, 0] & touched[:, 1]).sum() >= 10
    tot, per, out, f, nc = _wall_ledger(c, name, True)
    tot2, per2, _, f2, _ = _wall_ledger(c, name, False)
    tot3, per3, _, _, _ = _wall_ledger(c, name, False, det=1)
    # the bar of the wrench: 1e-9 of the largest force, times the velocity it works against and dt
    fscale = np.abs(Fw.sum(axis=0)).max()
    vscale = max(np.abs(c["tw"][:, :3]).max(), 1.0 if vel is None else np.abs(vel).max())
    scale = WALL_DT * fscale * vscale
    print(f"{name}: contacts {nc}, per wall (damping, friction, work) {per.tolist()}, reference {per_ref.tolist()}, "
          f"err {np.abs(per - per_ref).max():.2e} of bar {TOL * scale:.2e}")
    assert nc == touched.sum()
    assert np.abs(per - per_ref).max() <= TOL * scale and np.abs(tot[2:] - tot_ref).max() <= TOL * scale
    assert not tot[:2].any()
    assert (per_ref[:, 0] > 0).all() == (gamma is not None and all(gamma)) and (per_ref[:, 1] > 0).all() == (fric is not None)
    assert (per_ref[:, 2] != 0).all() == (vel is not None)
    assert np.array_equal(tot, tot2) and np.array_equal(per, per2) and np.array_equal(f, f2)      # wall_out or not: the same bits
    assert np.array_equal(tot, tot3) and np.array_equal(per, per3)                              # deterministic or not
    # the work is -dt F_w.u_w of the very force the caller reads in wall_out
    if vel is not None:
        w = -WALL_DT * (out[:, 1:] * np.array(vel)).sum(axis=1)
        assert np.abs(per[:, 2] - w).max() <= 1e-13 * np.abs(w).max()


def test_set_walls_resets_the_wall_entries_and_keeps_the_pair_entries(oracle):
    case, K, E, v, L, _ = _pair_case(60, 1, 1.25, None, True, 8)
    sp = ctx(case, K, E, gamma=GAMMA)
    sp.set_energy_ledger(True)
    gpu_forces(sp, case, v, L)
    planes = np.array([[0.0, 0, 1, case["bed"]["x"][:, 2].min() - 0.8]])
    sp.set_walls(planes, 1000.0, 1.25)
    sp.wall_damping(400.0)
    b, n = case["bed"], case["n"]
    import torch
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda:0")
    f, tq, tw = z(n, 3), z(n, 3), dev(np.concatenate([v, np.zeros((n, 3))], axis=1))
    xd, qd, sh, m = dev(b["x"]), dev(b["quat"]), dev(b["shtype"].astype(np.int32)), dev(np.ones(n, np.int32))
    sp.wall_force_damped_device(n, xd.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), tw.data_ptr())
    sp.ledger_fold_device(1.0)
    tot, per = sp.energy_ledger()
    assert tot[0] > 0 and tot[2] > 0 and per[0, 0] == tot[2]
    sp.set_walls(planes, 1000.0, 1.25)
    tot2, per2 = sp.energy_ledger()
    sp.close()
    assert tot2[0] == tot[0] and not tot2[2:].any() and not per2.any()


# ---- 3. + 4. the three loops, and the wall work against the host's own sum -------------------------------------------

class _WithWallOut:
    """A context whose wall pass also fills the caller's wall_out: everything else is the context's."""

    def __init__(self, sp, out):
        self._sp, self._out = sp, out

    def __getattr__(self, k):
        return getattr(self._sp, k)

    def wall_force_damped_device(self, *a, **kw):
        kw["wall_out"] = self._out.data_ptr()
        return self._sp.wall_force_damped_device(*a, **kw)


def _piston_bed(mode, nsteps=40, dt=5e-4):
    """The settling bed of tests/test_gpu_wall_move.py's loop test — gravity, a rising floor, a belt — with pair and wall
    damping and friction, started fast enough and with a skin small enough for a rebuild inside the run."""
    import torch
    from shpair import shapes
    from shpair.run import DeviceRun
    from test_gpu_wall import _settling_case, box_planes
    shp = [(4, shapes.random_shape(4, 21, amp=0.15))]
    L = 8.4
    x, quat = _settling_case(4, L)
    x[:, 2] -= 0.15
    n = x.shape[0]
    planes = box_planes(L, cut=-10.0)[:6]
    vel = np.zeros((6, 3))
    vel[4] = [0.0, 0.0, 0.2]          # the floor rises
    vel[0] = [0.0, 1.0, 0.0]          # the wall x = 0 is a belt along y
    sp = _wall_ctx(shp, 10, kn=2000.0, deterministic=1)
    r = DeviceRun(sp, x, quat, np.zeros(n, np.int32), (0, 0, 0), (L, L, L), (0, 0, 0), 0.02, dt=dt, gravity=(0.0, 0.0, -9.81),
                  gamma_t=0.2, gamma_r=0.1, ledger=True, walls=(planes, 2000.0, 1.25), wall_damping=50.0, wall_friction=(0.3, 20.0),
                  wall_velocity=vel, pair_damping={(1, 1): 40.0}, pair_friction={(1, 1): (0.4, 30.0)})
    rng = np.random.default_rng(3)
    r.v[:] = dev(rng.normal(size=(n, 3)) * 1.5)
    r.force()
    b0, host = r.builds, None
    if mode == "python":
        r.run(nsteps)
    elif mode == "wall_out":
        out = torch.zeros(6, 4, dtype=torch.float64, device="cuda:0")
        r.sp = _WithWallOut(sp, out)
        host = np.zeros(6)
        for _ in range(nsteps):
            out.zero_()
            r.step()
            host += -dt * (out.cpu().numpy()[:, 1:] * vel).sum(axis=1)
    else:
        r.run_native(nsteps, use_graph=(mode == "graph"))
    torch.cuda.synchronize()
    led = r.ledger()
    nc = sp.wall_stats()
    rebuilds = r.builds - b0
    sp.close()
    return led, rebuilds, nc, host


def test_the_three_loops_give_the_same_ledger_bits_and_the_work_is_the_hosts_own_sum(oracle):
    ref, reb, nc, _ = _piston_bed("python")
    print(f"rebuilds {reb}, wall contacts {nc}, ledger " + ", ".join(f"{k} {ref[k]:.6g}" for k in ("dissipated", "work")),
          ref["per_wall"].tolist())
    assert reb >= 1 and nc > 0
    terms = ("pair_damping", "pair_friction", "wall_damping", "wall_friction")
    assert all(ref[k] > 0 for k in terms) and ref["work"] != 0
    assert ref["per_wall"][4, 2] != 0 and ref["per_wall"][0, 2] != 0 and not ref["per_wall"][[1, 2, 3, 5], 2].any()
    for mode in ("plain", "graph", "wall_out"):
        got, reb2, _, host = _piston_bed(mode)
        assert reb2 == reb, mode
        for k in terms + ("work",):
            assert got[k] == ref[k], (mode, k)
        assert np.array_equal(got["per_wall"], ref["per_wall"]), mode
    work = ref["per_wall"][:, 2]
    print(f"wall work: ledger {work[[0, 4]].tolist()}, host {host[[0, 4]].tolist()}")
    assert np.abs(work - host).max() <= 1e-13 * np.abs(host).max()


# ---- 5. closure ----------------------------------------------------------------------------------------------------------

def _collision(gamma, k):
    """tests/test_ledger_ref.py's COLLISION through shstep_run_device at dt / k: E_mech before and after, D, D's samples."""
    from shpair import ShPair, shapes
    from shpair.run import DeviceRun
    from test_ledger_ref import COLLISION as c
    sp = ShPair(0)
    sp.settings(c["nq"])
    sp.set_ntypes(1, 1)
    sp.set_shape(0, 0, shapes.sphere(1.0), 1.01)
    sp.coeff(1, 1, c["kn"], c["m"])
    sp.set_option("deterministic", 1)
    x = np.array([[2.99, 4.0, 4.0], [5.01, 4.0, 4.0]])
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]] * 2), np.zeros(2, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, dt=c["dt"] / k,
                  ledger=True, pair_damping={(1, 1): gamma})
    r.v[:] = dev(np.array([[0.5 * c["vrel"], 0, 0], [-0.5 * c["vrel"], 0, 0]]))
    r.force()
    E0, Ds = _total_energy(sp, r), [0.0]
    for _ in range(14):
        r.run_native(c["nsteps"] * k // 14, use_graph=True)
        Ds.append(r.ledger()["dissipated"])
    E1 = _total_energy(sp, r)
    gap = float((r.x[1, 0] - r.x[0, 0]).item())
    sp.close()
    return E0, E1, np.array(Ds), gap


def test_the_balance_of_a_collision_closes_to_first_order_in_dt(oracle):
    """The inputs are tests/test_ledger_ref.py's COLLISION, chosen there on the closed-form lens and on the oracle's
    sharp-rule integrals (which predict R = 2.107e-1 / 1.058e-1, ratio 0.502, elastic R0 = 2.0e-3 / 1.2e-3 for this run)."""
    from test_ledger_ref import COLLISION
    R, R0 = [], []
    for k in (1, 2):
        E0, E1, Ds, gap = _collision(COLLISION["gamma"], k)
        e0, e1, d0, gap0 = _collision(0.0, k)
        R.append(abs(E1 - E0 + Ds[-1]))
        R0.append(abs(e1 - e0))
        print(f"dt/{k}: E0 {E0:.6f} E1 {E1:.6f} D {Ds[-1]:.6f} R {R[-1]:.3e} R/D {R[-1] / Ds[-1]:.2e} elastic R0 {R0[-1]:.3e}")
        assert gap > 2.02 and gap0 > 2.02 and not d0.any()          # they met and parted; no dissipation without a gamma
        assert (np.diff(Ds) >= 0).all() and 0.3 * E0 < Ds[-1] < E0
    print(f"R(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert R0[0] <= 0.1 * R[0] and R0[1] <= 0.1 * R[1]
    assert R[1] <= 0.75 * R[0]


# ---- 6. two ranks ----------------------------------------------------------------------------------------------------------

def test_the_ranks_ledgers_add_up_to_the_single_rank_ledger():
    from mrank_common import GAMMA_LOOP, DT, _setup, _rank_run, _run_ranks
    from test_gpu_mrank_damp import _damped_ctx
    K = 6

    def run(grid):
        S = _setup(grid, (1, 1, 1))

        def body(rank):
            sp = _damped_ctx(S["shp"], gamma=GAMMA_LOOP, det=1)
            sp.set_energy_ledger(True)
            halo, r = _rank_run(S, sp, rank, dt=DT)
            r.run(K)
            tot, _ = sp.energy_ledger()
            halo.close()
            sp.close()
            return tot
        parts = _run_ranks(S["world"], body)
        if S["hub"]:
            S["hub"].close()
        return parts
    one, two = run((1, 1, 1))[0], run((2, 1, 1))
    s = two[0] + two[1]
    print(f"pair damping over {K} steps: one rank {one[0]!r}, two ranks {two[0][0]!r} + {two[1][0]!r}, rel diff {abs(s[0] - one[0]) / one[0]:.1e}")
    assert one[0] > 0 and two[0][0] > 0 and two[1][0] > 0 and not one[1:].any()
    assert abs(s[0] - one[0]) <= 1e-12 * one[0]


# ---- 7. ledger off -----------------------------------------------------------------------------------------------------------

def test_with_the_ledger_off_the_fold_is_refused_and_the_passes_are_what_they_were(oracle):
    from shpair.capi import ShPairError
    case, K, E, v, L, _ = _pair_case(60, 1, 1.25, None, True, 8)
    c = _wall_case()
    out = []
    for toggle in (False, True):
        sp = ctx(case, K, E, det=1, gamma=GAMMA, fric=FRIC)
        if toggle:
            sp.set_energy_ledger(True)
            sp.set_energy_ledger(False)
        with pytest.raises(ShPairError) as e:
            sp.ledger_fold_device(1.0)
        assert e.value.code == -4 and "ledger" in str(e.value)            # SHPAIR_ESTATE
        f, tq, _ = gpu_forces(sp, case, v, L)
        sp.close()
        import torch
        spw = _wall_ctx(c["shp"], NQ)
        spw.set_walls(c["planes"], WALL_KN, WALL_EXPO)
        spw.wall_damping([400.0, 250.0])
        spw.wall_friction([0.5, 0.3], [200.0, 400.0])
        if toggle:
            spw.set_energy_ledger(True)
            spw.set_energy_ledger(False)
        n = c["n"]
        xd, qd, sh, m, twd = dev(c["x"]), dev(c["quat"]), dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32)), dev(c["tw"])
        fw, tw_ = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
        wo = torch.zeros(2, 4, dtype=torch.float64, device="cuda:0")
        spw.wall_force_damped_device(n, xd.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), fw.data_ptr(), tw_.data_ptr(),
                                     twd.data_ptr(), wall_out=wo.data_ptr())
        torch.cuda.synchronize()
        spw.synchronize()
        out.append((f, tq, fw.cpu().numpy(), tw_.cpu().numpy(), wo.cpu().numpy()))
        spw.close()
    assert np.abs(out[0][0]).max() > 0 and np.abs(out[0][2]).max() > 0
    for a, b in zip(*out):
        assert np.array_equal(a, b)
