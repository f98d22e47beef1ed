"""GPU tests of the rolling and twisting resistance of docs/SPEC.md §2.16 (csrc/rolling_kernels.hpp through the C ABI of
include/shstep.h) against tests/rolling_ref.py fed by the ORACLE's per-pair integrals: the added torque at SPEC §4's gate
(1e-9 of the larger of the largest force and the largest torque), f untouched bit for bit, the closed form of two
spheres, the deterministic mode, the pass alone and beside the other three laws, the run loop with its ledger, two
ranks, and the refusals.  The pass does not depend on the order: L = 4, n_q = 8 unless stated.

The coefficients and motion seeds below were chosen on the CPU, with the oracle and the reference alone, so that the
conditions the parity test asserts on its INPUTS hold (both branches of each kappa well populated, a clamped slot wherever
a gamma_ij is set, no slot near a branch point, an added torque that is not small)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import coeff_tables, oracle_compute  # noqa: E402
from dissipation_common import NQ, dev, bed_case, motion, ctx, _total_energy  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9
GAMMA = {(1, 1): 300.0, (1, 2): 900.0, (2, 2): 1800.0}                         # tests/test_gpu_friction.py's
FRIC = {(1, 1): (2.0, 300.0), (1, 2): (1.5, 400.0), (2, 2): (2.5, 250.0)}      # (mu, gamma_t), tests/test_gpu_friction.py's
ROLL = {(1, 1): (0.18, 120.0), (1, 2): (0.12, 90.0), (2, 2): (0.24, 150.0)}     # (mu_r, gamma_r)
TWIST = {(1, 1): (0.09, 180.0), (1, 2): (0.06, 135.0), (2, 2): (0.12, 210.0)}    # (mu_tw, gamma_tw)


def table(coef, k=None):
    G = np.zeros((3, 3))
    for (a, b), g in (coef or {}).items():
        G[a, b] = G[b, a] = g if k is None else g[k]
    return G


def bits(a):
    """The bit patterns of a double tensor / array: equality of these tells -0.0 from 0.0."""
    import torch
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _bed(n, seed, expo, nlocal, newton, mseed):
    """The bed, its motion and the oracle's integrals, computed once per bed (shared and left alone)."""
    from oracle import oracle as O
    import damp_ref as D
    O.build()
    case = bed_case(O, n, seed, nlocal)
    K, E = coeff_tables(2, lambda i, j: 1000.0 + 100.0 * (i + j), expo)
    v, L = motion(case, mseed)
    b = case["bed"]
    o = oracle_compute(O, case, NQ, K, E, nlocal=n if nlocal is None else nlocal, newton_pair=newton, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], case["offsets"], case["jlist"])
    tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
    return dict(case=case, K=K, E=E, v=v, L=L, o=o, pi=pi, pj=pj, tw=tw, nlocal=n if nlocal is None else nlocal, newton=newton)


def reference(c, gamma, roll, twist):
    """The torque the rolling pass adds, its details, and the forces / torques it is added to (elastic + damping)."""
    import damp_ref as D
    import rolling_ref as R
    b = c["case"]["bed"]
    a = (c["o"]["pairs"], c["pi"], c["pj"], b["x"], c["tw"], b["type"], c["K"], c["E"], table(gamma))
    tq, det = R.pair_rolling(*a, table(roll, 0), table(roll, 1), table(twist, 0), table(twist, 1), c["nlocal"], newton_pair=c["newton"])
    fd, td = D.pair_damping(*a, c["nlocal"], newton_pair=c["newton"])
    return dict(torque=tq, det=det, f0=c["o"]["f"] + fd, t0=c["o"]["torque"] + td)


def input_conditions(ref, damped, roll, twist):
    """The conditions of the parity test on its inputs (not measurements of the code under test)."""
    det = ref["det"]
    live = det["live"]
    out = dict(live=int(live.sum()), clamped=int(det["clamped"].sum()), damped=damped,
               share=float(np.abs(ref["torque"]).max() / np.abs(ref["t0"]).max()))
    for kind, on in (("r", bool(roll)), ("tw", bool(twist))):
        if on:
            cp = det["capped_" + kind][live]
            near = np.abs(det["visc_" + kind][live] - det["cap_" + kind][live]) / det["cap_" + kind][live]
            out["capped_" + kind], out["viscous_" + kind], out["nearest_" + kind] = float(cp.mean()), float((~cp).mean()), float(near.min())
    return out


def assert_input_conditions(c):
    for kind in ("r", "tw"):
        if "capped_" + kind in c:
            assert c["capped_" + kind] >= 0.1 and c["viscous_" + kind] >= 0.1, c     # 10 % of the live slots in each branch
            assert c["nearest_" + kind] > 1e-6, c                                    # no slot within 1e-6 relative of a branch point
    assert c["clamped"] >= 1 or not c["damped"], c        # a clamped slot in every case with a gamma_ij (none can exist without)
    assert c["share"] > 0.05, c                           # the added torque exceeds 5 % of the largest torque


def rolling_ctx(case, K, E, det=0, gamma=None, fric=None, roll=None, twist=None):
    sp = ctx(case, K, E, det=det, gamma=gamma, fric=fric)
    for (a, b), (mu, g) in (roll or {}).items():
        sp.pair_rolling(a, b, mu, g)
    for (a, b), (mu, g) in (twist or {}).items():
        sp.pair_twisting(a, b, mu, g)
    return sp


def gpu_pass(sp, case, v, L, nlocal=None, newton=True):
    """compute + twists + the pair pass where one runs, then the rolling pass: (f, torque) ahead of it and behind it,
    as tensors, and the twists."""
    import torch
    b, n = case["bed"], case["n"]
    nlocal = n if nlocal is None else nlocal
    x, q, ty, sh = dev(b["x"]), dev(b["quat"]), dev(b["type"].astype(np.int32)), dev(b["shtype"].astype(np.int32))
    vd, Ld = dev(v), dev(L)
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    tw = torch.zeros(n, 6, dtype=torch.float64, device="cuda:0")
    sp.compute_device(nlocal, n - nlocal, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f.data_ptr(), tq.data_ptr(),
                      newton_pair=newton)
    sp.twist_device(n, 0, vd.data_ptr(), q.data_ptr(), Ld.data_ptr(), sh.data_ptr(), tw.data_ptr())
    sp.pair_dissipation_device(nlocal, n - nlocal, x.data_ptr(), ty.data_ptr(), sh.data_ptr(), tw.data_ptr(), f.data_ptr(),
                               tq.data_ptr(), newton_pair=newton)
    torch.cuda.synchronize()
    sp.synchronize()
    f0, t0 = f.clone(), tq.clone()
    sp.pair_rolling_device(nlocal, n - nlocal, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), tq.data_ptr(), newton_pair=newton)
    torch.cuda.synchronize()
    sp.synchronize()
    return f0, t0, f, tq, tw


# ---- 1. against the reference --------------------------------------------------------------------------------------

PARITY = [
    # n, bed seed, exponent, nlocal, newton, damping too?, motion seed (the beds of tests/test_gpu_friction.py), which
    (12, 2, 1.25, None, True, True, 9, "both"),        # fewer than 64 slots
    (60, 1, 1.25, None, True, True, 8, "both"),
    (60, 1, 1.0, None, True, True, 8, "both"),
    (60, 1, 1.25, None, True, False, 8, "both"),       # every gamma_ij = 0
    (60, 1, 1.25, None, True, True, 8, "roll"),        # rolling alone ...
    (60, 1, 1.0, None, True, False, 8, "roll"),
    (60, 1, 1.25, None, True, False, 8, "twist"),      # ... twisting alone
    (60, 1, 1.0, None, True, True, 8, "twist"),
    (60, 3, 1.25, 40, False, True, 10, "both"),
    (60, 3, 1.25, 40, True, True, 10, "both"),
    (150, 4, 1.25, None, True, True, 11, "both"),      # more than 256 slots, no multiple of 64 or 256
    (60, 1, 1.75, None, True, True, 8, "both"),        # exponents whose V^(m-1) is pow() in the pass (m - 1 = 0.75, 1.5,
    (60, 1, 2.5, None, True, True, 8, "both"),         # 0.3): it feeds the clamp and the caps mu_r N, mu_tw N
    (60, 1, 1.3, None, True, True, 8, "both"),
]


@pytest.mark.parametrize("n,seed,expo,nlocal,newton,damped,mseed,which", PARITY)
def test_rolling_torque_matches_the_reference_on_oracle_integrals(oracle, n, seed, expo, nlocal, newton, damped, mseed, which):
    c = _bed(n, seed, expo, nlocal, newton, mseed)
    case = c["case"]
    npairs = case["jlist"].size
    assert npairs % 64 != 0 and npairs % 256 != 0 and npairs > 10
    assert (npairs < 64) == (n == 12) and (n != 150 or npairs > 256)
    gamma = GAMMA if damped else {}
    roll, twist = (ROLL if which != "twist" else {}), (TWIST if which != "roll" else {})
    ref = reference(c, gamma, roll, twist)
    cond = input_conditions(ref, damped, roll, twist)
    print(f"n={n} m={expo} nlocal={nlocal} newton={newton} damped={damped} {which}: {npairs} slots, inputs {cond}")
    assert_input_conditions(cond)
    sp = rolling_ctx(case, c["K"], c["E"], gamma=gamma, roll=roll, twist=twist)
    f0, t0, f1, t1, tw = gpu_pass(sp, case, c["v"], c["L"], nlocal, newton)
    sp.close()
    assert np.array_equal(bits(f0), bits(f1))                            # f is bitwise untouched by the pass
    f0, t0, t1, tw = f0.cpu().numpy(), t0.cpu().numpy(), t1.cpu().numpy(), tw.cpu().numpy()
    scale = max(np.abs(ref["f0"]).max(), np.abs(ref["t0"] + ref["torque"]).max())
    et = np.abs((t1 - t0) - ref["torque"]).max() / scale
    e0 = max(np.abs(f0 - ref["f0"]).max(), np.abs(t0 - ref["t0"]).max()) / scale
    etw = np.abs(tw - c["tw"]).max() / np.abs(c["tw"]).max()
    print(f"  max|F| {np.abs(ref['f0']).max():.4g}, max|tau| {np.abs(ref['t0']).max():.4g}, max|added tau| {np.abs(ref['torque']).max():.4g}, "
          f"rel err added tau {et:.1e}, what it is added to {e0:.1e}, twist {etw:.1e}")
    assert etw <= 1e-12
    assert e0 <= TOL and et <= TOL
    if nlocal is not None and not newton:
        assert not t1[nlocal:].any()
    if nlocal is not None and newton:
        assert np.abs(t1[nlocal:] - t0[nlocal:]).max() > 0                # ghost j rows got their share


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


SPHERES = dict(n=2, lmax=0, shapes=None, bed=dict(x=np.array([[0.0, 0, 0], [1.9, 0, 0]]), quat=np.array([[1.0, 0, 0, 0]] * 2),
                                                   type=np.ones(2, np.int32), shtype=np.zeros(2, np.int32)))


@pytest.mark.parametrize("axis,kind", [(0, "twisting"), (2, "rolling")])
def test_spinning_sphere_against_a_sphere_at_rest_in_closed_form(oracle, axis, kind):
    """Two unit spheres 1.9 apart along x.  i spinning about x: Omega_n = omega, M = -kappa_tw omega on i and +kappa_tw
    omega on j; about z: Omega_r = omega, the same with kappa_r.  N = |F_elastic|, read from the run without coefficients;
    one spin rate in each branch of kappa."""
    mur, gr, mutw, gtw = 0.05, 2.0, 0.02, 3.0
    mu, g = (mutw, gtw) if kind == "twisting" else (mur, gr)
    sp = _sphere_ctx(det=0)
    sp.set_neighbors_csr(np.array([0], np.int32), np.array([0, 1], np.int32), np.array([1], np.int32))
    I = sp.body(0)[2][axis]                                   # inertia (xx, yy, zz, ...) of the unit sphere
    fe, te, f_, t_, _ = gpu_pass(sp, SPHERES, np.zeros((2, 3)), np.zeros((2, 3)))
    assert np.array_equal(bits(te), bits(t_))                # no coefficient: nothing was launched
    fe = fe.cpu().numpy()
    N = abs(fe[0, 0])                                        # p |S_n|: the elastic force of the pair, along x
    sp.pair_rolling(1, 1, mur, gr)
    sp.pair_twisting(1, 1, mutw, gtw)
    branch = mu * N / g
    for om, want_branch in ((0.5 * branch, "viscous"), (4.0 * branch, "capped")):
        L = np.zeros((2, 3))
        L[0, axis] = I * om
        f0, t0, f1, t1, tw = gpu_pass(sp, SPHERES, np.zeros((2, 3)), L)
        tw = tw.cpu().numpy()
        assert abs(tw[0, 3 + axis] - om) <= 1e-14 * om and not tw[1].any()
        kappa = g if g * om <= mu * N else mu * N / om
        assert (kappa == g) == (want_branch == "viscous")
        M = np.zeros(3)
        M[axis] = -kappa * om
        dt = (t1 - t0).cpu().numpy()
        tol = TOL * max(N, abs(kappa * om))
        print(f"{kind}, omega {om:.4g} ({want_branch}): N {N:.6g}, |M| {abs(kappa * om):.6g} (cap {mu * N:.6g}), "
              f"err tau_i {np.abs(dt[0] - M).max():.2e} tau_j {np.abs(dt[1] + M).max():.2e}, tol {tol:.2e}")
        assert abs(kappa * om) > 1e-4 * N
        assert np.abs(dt[0] - M).max() <= tol and np.abs(dt[1] + M).max() <= tol
        assert np.array_equal(bits(f1), bits(fe)) and np.array_equal(bits(f0), bits(fe))    # forces: the run without coefficients
    sp.close()


# ---- 3. a common spin ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("det", [0, 1])
def test_both_spinning_alike_adds_exactly_nothing(oracle, det):
    sp = _sphere_ctx(det=det)
    sp.set_neighbors_csr(np.array([0], np.int32), np.array([0, 1], np.int32), np.array([1], np.int32))
    sp.pair_rolling(1, 1, 0.05, 2.0)
    sp.pair_twisting(1, 1, 0.02, 3.0)
    Ixx = sp.body(0)[2][0]
    om = np.array([0.7, -1.3, 2.1])
    v = np.array([[0.3, 0.1, -0.2], [-0.4, 0.2, 0.5]])       # (the linear motion does not enter: every gamma_ij = 0)
    f0, t0, f1, t1, tw = gpu_pass(sp, SPHERES, v, np.array([Ixx * om, Ixx * om]))
    sp.close()
    tw = tw.cpu().numpy()
    assert np.array_equal(tw[0, 3:], tw[1, 3:]) and np.abs(tw[0, 3:]).min() > 0.5
    assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(bits(f0), bits(f1))


# ---- 4. deterministic mode -------------------------------------------------------------------------------------------

def test_deterministic_mode_is_bitwise_reproducible_and_leaves_f_alone(oracle):
    c = _bed(60, 1, 1.25, None, True, 8)
    ref = reference(c, GAMMA, ROLL, TWIST)
    runs = []
    for det in (1, 1, 0):
        sp = rolling_ctx(c["case"], c["K"], c["E"], det=det, gamma=GAMMA, roll=ROLL, twist=TWIST)
        f0, t0, f1, t1, _ = gpu_pass(sp, c["case"], c["v"], c["L"])
        assert np.array_equal(bits(f0), bits(f1))            # f has the bits it had before the pass
        if det and not runs:
            _, _, f2, t2, _ = gpu_pass(sp, c["case"], c["v"], c["L"])   # the same context again
            assert np.array_equal(bits(f1), bits(f2)) and np.array_equal(bits(t1), bits(t2))
        runs.append((f1.cpu().numpy(), t1.cpu().numpy(), (t1 - t0).cpu().numpy()))
        sp.close()
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    scale = max(np.abs(ref["f0"]).max(), np.abs(ref["t0"] + ref["torque"]).max())
    assert np.abs(runs[0][1] - runs[2][1]).max() <= TOL * scale          # ... and agrees with the atomics
    assert np.abs(runs[0][2] - ref["torque"]).max() <= TOL * scale       # ... and with the reference
    assert np.abs(ref["torque"]).max() > 0.05 * np.abs(ref["t0"]).max()


# ---- 5. alone, and beside the others -----------------------------------------------------------------------------------

def test_with_rolling_alone_the_pair_passes_launch_nothing(oracle):
    """Only a rolling coefficient: the integrals are kept, but no table of the pair pass exists.  pair_dissipation_device
    and pair_contact_device return OK and leave f and torque as they are."""
    import torch
    c = _bed(60, 1, 1.25, None, True, 8)
    case = c["case"]
    sp = rolling_ctx(case, c["K"], c["E"], roll={(1, 2): (0.04, 30.0)})
    assert sp.keeps_integrals and sp.has_rolling and not sp.has_pair_pass
    b, n = case["bed"], case["n"]
    x, q, ty, sh = dev(b["x"]), dev(b["quat"]), dev(b["type"].astype(np.int32)), dev(b["shtype"].astype(np.int32))
    f, tq, tw = dev(np.zeros((n, 3))), dev(np.zeros((n, 3))), dev(np.zeros((n, 6)))
    sp.compute_device(n, 0, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f.data_ptr(), tq.data_ptr())
    sp.twist_device(n, 0, dev(c["v"]).data_ptr(), q.data_ptr(), dev(c["L"]).data_ptr(), sh.data_ptr(), tw.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    f0, t0 = f.clone(), tq.clone()
    a = (n, 0, x.data_ptr(), ty.data_ptr(), sh.data_ptr(), tw.data_ptr(), f.data_ptr(), tq.data_ptr())
    sp.pair_dissipation_device(*a)
    sp.pair_contact_device(*a, 1e-3)
    torch.cuda.synchronize()
    sp.synchronize()
    assert np.array_equal(bits(f), bits(f0)) and np.array_equal(bits(tq), bits(t0))
    sp.pair_rolling_device(n, 0, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), tq.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    sp.close()
    assert np.array_equal(bits(f), bits(f0)) and not np.array_equal(bits(tq), bits(t0))


def test_beside_damping_friction_and_a_spring_the_total_is_the_sum_of_the_references(oracle):
    """tests/test_gpu_history.py's bed, list, xi and dt = 0 reference (damping + friction + springs), with both kinds of
    resistance set too: the pair pass adds what it added there, the rolling pass adds tests/rolling_ref.py's torque."""
    import torch
    import damp_ref as D
    import rolling_ref as R
    from test_gpu_history import GAMMA as HG, NLOCAL, history_inputs, _bed_ctx, _Bed
    r = history_inputs(oracle, True)
    case, b = r["case"], r["case"]["bed"]
    pi, pj = D.expand(case["ilist"], r["offs"], r["jl"])
    tw = D.twists(case["massprops"], [1.0, 1.0], r["v"], b["quat"], r["L"], b["shtype"])
    rt, rdet = R.pair_rolling(r["o"]["pairs"], pi, pj, b["x"], tw, b["type"], r["K"], r["E"], table(HG), table(ROLL, 0), table(ROLL, 1),
                              table(TWIST, 0), table(TWIST, 1), NLOCAL, newton_pair=True)
    sp = _bed_ctx(case, r["K"], r["E"])
    for (a, c), (mu, g) in ROLL.items():
        sp.pair_rolling(a, c, mu, g)
    for (a, c), (mu, g) in TWIST.items():
        sp.pair_twisting(a, c, mu, g)
    bed = _Bed(sp, case, r["v"], r["L"], NLOCAL, True)
    assert np.array_equal(bed.offs, r["offs"]) and np.array_equal(bed.jl, r["jl"])
    sp.set_contact_history(NLOCAL, r["xi"])
    f, tq = bed.f.clone(), bed.tq.clone()
    a = (NLOCAL, bed.n - NLOCAL, bed.x.data_ptr(), bed.ty.data_ptr())
    sp.pair_contact_device(*a, bed.sh.data_ptr(), bed.tw.data_ptr(), f.data_ptr(), tq.data_ptr(), 0.0)
    sp.pair_rolling_device(*a, bed.tw.data_ptr(), tq.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    sp.close()
    df, dt = (f - bed.f).cpu().numpy(), (tq - bed.tq).cpu().numpy()
    lf, lt = r["look"][0], r["look"][1]
    scale = max(np.abs(r["o"]["f"] + lf).max(), np.abs(r["o"]["torque"] + lt + rt).max())
    print(f"beside the others: live {int(rdet['live'].sum())}, max|added tau| {np.abs(rt).max():.4g} beside {np.abs(lt).max():.4g}, "
          f"rel err dF {np.abs(df - lf).max() / scale:.1e} dtau {np.abs(dt - (lt + rt)).max() / scale:.1e}")
    assert rdet["live"].sum() > 100 and np.abs(rt).max() > 0.05 * np.abs(r["o"]["torque"] + lt).max()
    assert np.abs(df - lf).max() <= TOL * scale and np.abs(dt - (lt + rt)).max() <= TOL * scale


# ---- 6. the run loop ---------------------------------------------------------------------------------------------------

TWIST_RUN = dict(kn=1e4, m=1.25, vrel=6.0, dt=1e-4, nsteps=1400, nq=32, om=20.0, mu_tw=0.3, gamma_tw=10.0)


def _twisting_collision(coef, k=1, use_graph=True, ledger=True, samples=14):
    """tests/test_ledger_ref.py's head-on COLLISION of two unit spheres, elastic, with sphere 0 spinning about the line of
    centres: only twisting resistance can act on that spin.  dt / k.  Returns the samples of (omega_0x - omega_1x), of the
    total angular momentum about the origin, E_mech before and after, the ledger's samples, the final state."""
    import torch
    from shpair.run import DeviceRun
    c = TWIST_RUN
    sp = _sphere_ctx(det=1, nq=c["nq"], kn=c["kn"], expo=c["m"])
    x = np.array([[2.99, 4.0, 4.0], [5.01, 4.0, 4.0]])
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]] * 2), np.zeros(2, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, dt=c["dt"] / k,
                  ledger=ledger, pair_twisting=coef)
    mass, _, inertia = sp.body(0)
    r.v[:] = dev(np.array([[0.5 * c["vrel"], 0, 0], [-0.5 * c["vrel"], 0, 0]]))
    r.L[:] = dev(np.array([[inertia[0] * c["om"], 0, 0], [0, 0, 0]]))
    r.force()
    E0 = _total_energy(sp, r)
    spin, J, Ds = [c["om"]], [], [0.0]

    def momentum():
        X, V, L = r.x[:2].cpu().numpy(), r.v.cpu().numpy(), r.L.cpu().numpy()
        return (np.cross(X, mass * V) + L).sum(axis=0)           # the unit sphere's centre of mass is its SH origin
    J.append(momentum())
    for _ in range(samples):
        r.run_native(c["nsteps"] * k // samples, use_graph=use_graph)
        L = r.L.cpu().numpy()
        spin.append((L[0, 0] - L[1, 0]) / inertia[0])
        J.append(momentum())
        if ledger:
            Ds.append(r.ledger()["pair_friction"])
    E1 = _total_energy(sp, r)
    torch.cuda.synchronize()
    state = [t.cpu().numpy().copy() for t in (r.x[:2], r.v, r.q[:2], r.L, r.f[:2], r.tq[:2])]
    led = r.ledger() if ledger else None
    gap = float((r.x[1, 0] - r.x[0, 0]).item())
    sp.close()
    return dict(spin=np.array(spin), J=np.array(J), E0=E0, E1=E1, D=np.array(Ds), state=state, ledger=led, gap=gap, inertia=inertia[0])


def test_twisting_in_the_run_loop_takes_the_relative_spin_out_and_the_ledger_balances(oracle):
    """The band of the balance is tests/test_gpu_ledger.py's for its own collision: the elastic residual at most a tenth of
    the residual, and R(dt / 2) <= 0.75 R(dt).  The inputs were chosen on the closed-form lens in numpy (the loop's time
    levels): the contact visits both branches of kappa_tw, the relative spin falls 20 -> 13.8, D = 87.9,
    R = 4.72e-2 / 2.36e-2 (ratio 0.500), elastic R0 = 2.2e-5 / 1.7e-6."""
    c = TWIST_RUN
    coef = {(1, 1): (c["mu_tw"], c["gamma_tw"])}
    R, R0 = [], []
    for k in (1, 2):
        a = _twisting_collision(coef, k)
        e = _twisting_collision(None, k)
        R.append(abs(a["E1"] - a["E0"] + a["D"][-1]))
        R0.append(abs(e["E1"] - e["E0"]))
        print(f"dt/{k}: relative spin {a['spin'][0]:.4f} -> {a['spin'][-1]:.4f}, E0 {a['E0']:.6f} E1 {a['E1']:.6f} D {a['D'][-1]:.6f} "
              f"R {R[-1]:.3e} elastic R0 {R0[-1]:.3e}, |dJ| {np.abs(a['J'] - a['J'][0]).max():.2e}")
        assert a["gap"] > 2.02 and e["gap"] > 2.02                                  # they met and parted
        assert (np.diff(a["spin"]) <= 0).all() and a["spin"][-1] < 0.9 * a["spin"][0]   # the relative spin decays monotonically
        assert np.abs(e["spin"] - c["om"]).max() <= 1e-10 * c["om"]                 # without the coefficient nothing touches it
        assert not e["D"].any() and e["ledger"]["dissipated"] == 0.0
        Jscale = np.abs(a["J"][0]).max()
        assert Jscale > 1.0 and np.abs(a["J"] - a["J"][0]).max() <= 1e-12 * Jscale  # total angular momentum, to rounding
        assert (np.diff(a["D"]) >= 0).all() and a["D"][-1] > 0
        assert a["ledger"]["pair_friction"] == a["D"][-1] and a["ledger"]["dissipated"] == a["D"][-1]   # the friction entry, alone
    print(f"R(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert R0[0] <= 0.1 * R[0] and R0[1] <= 0.1 * R[1]
    assert R[1] <= 0.75 * R[0]


def test_graph_replay_and_plain_launches_give_the_same_bits(oracle):
    coef = {(1, 1): (TWIST_RUN["mu_tw"], TWIST_RUN["gamma_tw"])}
    out = [_twisting_collision(coef, 1, use_graph=g, samples=2) for g in (False, True)]
    for a, b in zip(out[0]["state"], out[1]["state"]):
        assert np.array_equal(bits(a), bits(b))
    assert out[0]["ledger"]["pair_friction"] == out[1]["ledger"]["pair_friction"] > 0
    assert out[0]["spin"][-1] < out[0]["spin"][0]


@pytest.mark.parametrize("mode", ["python", "plain", "graph"])
def test_the_first_steps_fold_holds_that_steps_power_alone(oracle, mode):
    """Twisting alone, ledger on, two unit spheres in contact and spinning: the force pass a driver runs at set-up leaves
    power rows that no fold follows.  The first step's fold must hold dt P of that step and nothing of the set-up pass:
    with no pair pass the rolling pass WRITES its rows.  P from the closed form: N = |F_elastic| at x(t + dt) (the pass
    adds no force), Omega the half-step relative spin L(t) + dt/2 tau(t) over the sphere's inertia."""
    import torch
    from shpair.run import DeviceRun
    mu, g, dt, om = 0.3, 10.0, 1e-4, 20.0
    sp = _sphere_ctx(det=1, nq=32, kn=1e4)
    x = np.array([[3.05, 4.0, 4.0], [4.95, 4.0, 4.0]])
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]] * 2), np.zeros(2, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, dt=dt,
                  ledger=True, pair_twisting={(1, 1): (mu, g)})
    I = sp.body(0)[2][0]
    r.L[:] = dev(np.array([[I * om, 0, 0], [0, 0, 0]]))
    r.force()                                                 # the set-up forces of the spinning pair: rows, no fold
    torch.cuda.synchronize()
    sp.synchronize()
    assert r.ledger()["dissipated"] == 0.0
    L0, tq0 = r.L.cpu().numpy().copy(), r.tq[:2].cpu().numpy().copy()
    assert abs(tq0[0, 0]) > 1.0                               # the set-up pass did act: its rows are not zeros
    if mode == "python":
        r.step()
    else:
        r.run_native(1, use_graph=(mode == "graph"))
    torch.cuda.synchronize()
    sp.synchronize()
    led = r.ledger()
    N = abs(float(r.f[0, 0].item()))
    Lh = L0 + 0.5 * dt * tq0
    Om = (Lh[0, 0] - Lh[1, 0]) / I
    kappa = g if g * abs(Om) <= mu * N else mu * N / abs(Om)
    want = dt * kappa * Om * Om
    sp.close()
    print(f"{mode}: N {N:.6g}, half-step relative spin {Om:.6f}, dt P {want:.9e}, ledger {led['pair_friction']:.9e}")
    assert want > 0 and abs(led["pair_friction"] - want) <= TOL * want
    assert led["dissipated"] == led["pair_friction"]


def test_beside_a_pair_pass_the_ledger_holds_both_powers(oracle):
    """Damping, friction and both kinds of resistance with the ledger on: the pair pass writes the power rows and the
    rolling pass ADDS its share.  The friction entry is tests/ledger_ref.py's friction power plus the sum of share times
    tests/rolling_ref.py's power; the damping entry is untouched.  Ghost j rows without newton_pair: the half share.
    A second compute + passes without a fold in between: the fold still takes the last passes once."""
    import ledger_ref as LR
    c = _bed(60, 3, 1.25, 40, False, 10)
    case, b, nlocal = c["case"], c["case"]["bed"], 40
    a = (c["o"]["pairs"], c["pi"], c["pj"], b["x"], c["tw"], b["type"], b["shtype"], case["rmax"], c["K"], c["E"])
    P = LR.pair_powers(*a, table(GAMMA), table(FRIC, 0), table(FRIC, 1), nlocal, newton_pair=False).sum(axis=0)
    det = reference(c, GAMMA, ROLL, TWIST)["det"]
    share = 0.5 + 0.5 * (c["pj"] < nlocal)
    Proll = float((share * det["power"]).sum())
    # (the resistance's power is a million gates wide: the test tells it from zero, from twice and from the half shares)
    assert (share == 0.5).any() and Proll > 1e6 * TOL * P.sum() and P[0] > 0 and P[1] > 0
    sp = rolling_ctx(case, c["K"], c["E"], gamma=GAMMA, fric=FRIC, roll=ROLL, twist=TWIST)
    sp.set_energy_ledger(True)
    gpu_pass(sp, case, c["v"], c["L"], nlocal, False)
    gpu_pass(sp, case, c["v"], c["L"], nlocal, False)         # no fold in between: these rows replace the first
    sp.ledger_fold_device(1.0)
    tot, _ = sp.energy_ledger()
    sp.close()
    scale = P.sum() + Proll
    print(f"pair damping {tot[0]:.6g} (reference {P[0]:.6g}), pair friction {tot[1]:.6g} (reference {P[1]:.6g} + {Proll:.6g}), "
          f"rel err {max(abs(tot[0] - P[0]), abs(tot[1] - P[1] - Proll)) / scale:.1e}")
    assert abs(tot[0] - P[0]) <= TOL * scale and abs(tot[1] - (P[1] + Proll)) <= TOL * scale
    assert not tot[2:].any()


# ---- 7. several ranks ------------------------------------------------------------------------------------------------------

MR_ROLL, MR_TWIST = (0.05, 50.0), (0.03, 50.0)


def _mrank_ctx(shp, twists=1):
    from mrank_common import LMAX, NQ as MNQ, GAMMA as MG, _ctx
    sp = _ctx(LMAX, shp, MNQ)
    sp.set_option("halo_twists", twists)
    sp.pair_damping(1, 1, MG)
    sp.pair_rolling(1, 1, *MR_ROLL)
    sp.pair_twisting(1, 1, *MR_TWIST)
    return sp


@functools.lru_cache(maxsize=None)
def _mrank_reference(periodic):
    """The whole box on one rank (shstep's own periodic images): forces and torques without and with the resistance."""
    import torch
    from shpair.run import DeviceRun
    from mrank_common import LMAX, NQ as MNQ, SKIN, NBED, GAMMA as MG, _bed as mbed, _ctx, _shapes, _motion
    shp = _shapes()
    x, quat, sht, tag, lo, hi, _ = mbed(NBED, periodic)
    n = x.shape[0]
    v, L = _motion(n)
    out = {}
    for name, on in (("damped", False), ("rolling", True)):
        sp = _ctx(LMAX, shp, MNQ)
        r = DeviceRun(sp, x, quat, sht, lo, hi, periodic, SKIN, dt=0.0, pair_damping={(1, 1): MG},
                      pair_rolling={(1, 1): MR_ROLL} if on else None, pair_twisting={(1, 1): MR_TWIST} if on else None)
        r.v[:] = torch.from_numpy(v).to(r.v.device)
        r.L[:] = torch.from_numpy(L).to(r.L.device)
        r.force()
        torch.cuda.synchronize()
        sp.synchronize()
        out[name] = (r.f[:n].cpu().numpy(), r.tq[:n].cpu().numpy())
        out["npairs"] = r.npairs
        sp.close()
    return out


def test_static_torques_over_two_ranks_match_the_single_domain():
    from mrank_common import _setup, _rank_run, _run_ranks, _gather
    grid, periodic = (2, 1, 1), (1, 1, 1)
    S = _setup(grid, periodic)

    def body(rank):
        sp = _mrank_ctx(S["shp"])
        halo, run = _rank_run(S, sp, rank, dt=0.0)
        t, _, _, _, f, tq = run.owned()
        res = dict(tag=t, f=f, tq=tq, npairs=run.npairs, fwd=halo.stats()["forward_bytes_per_step"])
        sp.pair_damping(1, 1, 0.0)           # rolling and twisting alone keep the wide exchange; with neither it is the narrow one
        res["fwd_rolling"] = halo.stats()["forward_bytes_per_step"]
        sp.pair_rolling(1, 1, 0.0, 0.0)
        sp.pair_twisting(1, 1, 0.0, 0.0)
        res["fwd_narrow"] = halo.stats()["forward_bytes_per_step"]
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(S["world"], body)
    ref = _mrank_reference(periodic)
    n = S["x"].shape[0]
    f, tq = _gather(parts, n, ("f", "tq"))
    fr, tr = ref["rolling"]
    fs = np.abs(fr).max()
    added = np.abs(tr - ref["damped"][1]).max()
    ef, et = np.abs(f - fr).max(), np.abs(tq - tr).max()
    print(f"grid {grid}: max|f| {fs:.4g}, max|tau| {np.abs(tr).max():.4g}, added torque {added:.4g}, |df| {ef:.2e} |dtau| {et:.2e} "
          f"(bar {1e-9 * fs:.2e})")
    assert np.array_equal(fr, ref["damped"][0]) or np.abs(fr - ref["damped"][0]).max() <= 1e-12 * fs    # no force is added
    assert added > 1e-2 * np.abs(tr).max()                    # the resistance is not negligible
    assert sum(p["npairs"] for p in parts) == ref["npairs"]
    assert fs > 0 and ef <= 1e-9 * fs and et <= 1e-9 * fs     # tests/test_gpu_mrank_friction.py's tolerance
    assert all(p["fwd_narrow"] > 0 and 7 * p["fwd"] == 13 * p["fwd_narrow"] and p["fwd_rolling"] == p["fwd"] for p in parts)
    if S["hub"]:
        S["hub"].close()


def test_the_loop_over_ranks_refuses_rolling_without_halo_twists(oracle):
    from shpair import mrank
    from shpair.capi import ShPairError, HaloArrays, HaloRunParams
    c = _bed(12, 2, 1.25, None, True, 9)
    sp = rolling_ctx(c["case"], c["K"], c["E"])
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    for roll, twist in (((0.05, 2.0), (0.0, 0.0)), ((0.0, 0.0), (0.02, 3.0))):
        sp.pair_rolling(1, 2, *roll)
        sp.pair_twisting(1, 2, *twist)
        with pytest.raises(ShPairError, match="contact rolling or twisting resistance is not supported.*set option halo_twists") as e:
            halo.run(HaloArrays(), HaloRunParams(), 1, 0)
        assert e.value.code == -1                             # as for friction (tests/test_gpu_friction.py)
    halo.close()
    sp.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals(oracle):
    import torch
    from shpair.capi import ShPairError
    c = _bed(12, 2, 1.25, None, True, 9)
    case = c["case"]
    sp = rolling_ctx(case, c["K"], c["E"])
    for setter in (sp.pair_rolling, sp.pair_twisting):
        for a, b, mu, g in ((1, 1, -1.0, 1.0), (1, 1, 1.0, -1.0), (1, 2, np.nan, 1.0), (1, 2, 1.0, np.nan), (1, 1, np.inf, 1.0),
                            (1, 1, 1.0, np.inf), (0, 1, 1.0, 1.0), (1, 3, 1.0, 1.0)):
            with pytest.raises(ShPairError) as e:
                setter(a, b, mu, g)
            assert e.value.code == -1
    assert not sp.has_rolling
    n = case["n"]
    b = case["bed"]
    x, q, ty, sh = dev(b["x"]), dev(b["quat"]), dev(b["type"].astype(np.int32)), dev(b["shtype"].astype(np.int32))
    f, tq, tw = dev(np.zeros((n, 3))), dev(np.zeros((n, 3))), dev(np.zeros((n, 6)))
    # neither kind set: OK and nothing launched, whatever the pointers
    sp.pair_rolling_device(n, 0, None, None, None, None)
    sp.pair_rolling(1, 2, 0.05, 2.0)
    # the pass ahead of any compute on the list
    with pytest.raises(ShPairError, match="no compute has run") as e:
        sp.pair_rolling_device(n, 0, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), tq.data_ptr())
    assert e.value.code == -1
    sp.compute_device(n, 0, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f.data_ptr(), tq.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    # a null torque (or any other null array)
    for a in ((x.data_ptr(), ty.data_ptr(), tw.data_ptr(), None), (None, ty.data_ptr(), tw.data_ptr(), tq.data_ptr()),
              (x.data_ptr(), None, tw.data_ptr(), tq.data_ptr()), (x.data_ptr(), ty.data_ptr(), None, tq.data_ptr())):
        with pytest.raises(ShPairError, match="null array pointer") as e:
            sp.pair_rolling_device(n, 0, *a)
        assert e.value.code == -1
    # a list that refers to atoms the caller does not have
    with pytest.raises(ShPairError, match="stale list") as e:
        sp.pair_rolling_device(n - 1, 0, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), tq.data_ptr())
    assert e.value.code == -1
    # the deterministic option set after the compute: no reverse index yet
    sp.set_option("deterministic", 1)
    with pytest.raises(ShPairError, match="deterministic option was set after") as e:
        sp.pair_rolling_device(n, 0, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), tq.data_ptr())
    assert e.value.code == -4
    sp.close()
