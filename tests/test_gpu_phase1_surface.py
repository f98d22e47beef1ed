"""The per-azimuth contact kernel forms the surface integrals S_n, T_n in PHASE 1 — for both nodes of a lane's pair
(k, l), (k, l + n_q) from one pass over the ring row — and its phase 2 is the volume search alone
(contact_kernel_azimuth.hpp).  Per-pair output (V, S_n, T_n) and per-atom force and torque against the CPU oracle at
the suite's 1e-9, on small beds chosen so that every path of that change runs:

  L = 6 / n_q = 16, specialised and general instance, spacing 1.9 (queued batches) and 1.6 (slabs that do not fit the
  queue: direct batches — 457 of 4 666 batches on the 1.6 bed and 184 of 2 621 on the 1.9 bed, with `spec` 1 and 0
  alike, counted with the work-counter build, make stats);
  L = 7 / 7 and L = 9 / 11 — the new path at odd order: the trig of the first order kept in the row of particle j's
  table, the gradient pass taken an order at a time, and a last slab with idle lanes (49 node pairs in one slab, 121
  in two) whose repeated pair must weigh 0;
  L = 4 / 10 and L = 3 / 7 (odd order, trig kept in the row, a last slab with idle lanes: orders that keep the tail of
  phase 2, SHP_SURFACE_PHASE1, behind the new phase-1 helper); L = 8 / 16 with two waves per pair; L = 12 / 32 in ring
  groups of 8 with one wave per pair (sums parked across table builds) and as the library runs it (two waves, which
  keep the tail as well); exponent 1 without energy (no phase 2 at all); and isolated
  pairs with no and with exactly one inside node, where every other lane's weight must contribute exactly 0.
"""
import numpy as np
import pytest

from common import make_case, coeff_tables, oracle_compute, rel_err
from test_gpu_parity import make_ctx

pytestmark = pytest.mark.gpu
TOL = 1e-9


def run_pairs(case, nq, K, E, opts, eflag=True):
    import torch
    sp = make_ctx(case, nq, K, E)
    for k, v in opts.items():
        sp.set_option(k, v)
    npairs = case["jlist"].size
    pairs = torch.zeros(max(npairs, 1), 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(pairs.data_ptr())
    b = case["bed"]
    f, tq, eng, _ = sp.compute(case["n"], b["x"], b["quat"], b["type"], b["shtype"], eflag=eflag)
    ki = sp.kernel_info()
    sp.set_pair_output(None)
    sp.close()
    return f, tq, eng, pairs.cpu().numpy()[:npairs], ki


def check_all(f, tq, pr, o, cols=slice(0, 7)):
    fs = np.abs(o["f"]).max()
    ts = max(fs, np.abs(o["torque"]).max())
    assert fs > 0 and o["counts"][2] > 0          # the bed has touching pairs
    assert np.all(np.isfinite(o["f"])) and np.all(np.isfinite(o["pairs"]))
    ef, et = rel_err(f, o["f"], fs), rel_err(tq, o["torque"], ts)
    scale = np.abs(o["pairs"]).max(axis=0) + 1e-300
    ep = (np.abs(pr - o["pairs"]) / scale)[:, cols].max()
    print(f"rel err f {ef:.2e} torque {et:.2e} pairs {ep:.2e}")
    assert ef < TOL and et < TOL and ep < TOL


@pytest.mark.parametrize("lmax,nq,n,spacing,expo,opts,waves", [
    (6, 16, 200, 1.9, 1.25, {"spec": 1}, 1), (6, 16, 200, 1.9, 1.25, {"spec": 0}, 1),
    (6, 16, 200, 1.6, 1.25, {"spec": 1}, 1), (6, 16, 200, 1.6, 1.25, {"spec": 0}, 1),
    (4, 10, 200, 1.9, 1.25, {}, 1), (3, 7, 200, 1.9, 1.25, {}, 1),
    (7, 7, 200, 1.9, 1.25, {"jpoly": 1}, 1), (9, 11, 200, 1.9, 1.25, {"jpoly": 1}, 1),
    (8, 16, 200, 1.9, 1.25, {"jpoly": 1, "split": 1}, 2),
    (12, 32, 24, 1.9, 1.25, {"jpoly": 1, "split": 0, "ring_rows": 8}, 1), (12, 32, 24, 1.9, 1.25, {}, 2)])
def test_pair_integrals_forces_and_torques(oracle, lmax, nq, n, spacing, expo, opts, waves):
    case = make_case(n, lmax, 2, seed=900 + lmax, spacing=spacing, rmax_fn=oracle.shape_rmax)
    K, E = coeff_tables(1, 1000.0, expo)
    o = oracle_compute(oracle, case, nq, K, E, eflag=True, want_pairs=True)
    f, tq, eng, pr, ki = run_pairs(case, nq, K, E, opts)
    assert ki["family"] == 1 and ki["waves_per_pair"] == waves and ki["scratch_bytes"] == 0, ki
    if "spec" in opts:
        assert ki["specialised"] == opts["spec"]
    if lmax == 12:
        assert 30 <= case["jlist"].size <= 120, case["jlist"].size
    check_all(f, tq, pr, o)
    assert abs(eng - o["eng_virial"][0]) < TOL * abs(o["eng_virial"][0])


def test_forces_only_instance_has_no_phase_2(oracle):
    """Exponent 1 and no energy: the NEEDV = false instance — phase 1 accumulates, the epilogue runs, nothing is queued.
    V is not computed there: S_n and T_n (columns 1..6), forces and torques."""
    case = make_case(200, 6, 2, seed=906, rmax_fn=oracle.shape_rmax)
    K, E = coeff_tables(1, 1000.0, 1.0)
    o = oracle_compute(oracle, case, 16, K, E, want_pairs=True)
    for spec in (1, 0):
        f, tq, _, pr, ki = run_pairs(case, 16, K, E, {"spec": spec}, eflag=False)
        assert ki["family"] == 1 and ki["specialised"] == spec
        check_all(f, tq, pr, o, cols=slice(1, 7))


def _isolated(oracle, lmax, nq, a, rmax, sep):
    """Two particles of shape `a` at distance `sep` along a fixed generic direction, one listed pair; the oracle's row."""
    d = np.array([0.36, -0.48, 0.8]) * sep
    x = np.array([[0.0, 0.0, 0.0], d])
    q = np.array([[0.9, 0.1, -0.3, 0.3], [0.2, -0.7, 0.5, 0.47]])
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    bd = dict(x=x, quat=q, type=np.ones(2, np.int32), shtype=np.zeros(2, np.int32))
    case = dict(lmax=lmax, shapes=[a], rmax=[rmax], bed=bd, n=2, ilist=np.array([0, 1], np.int32),
                offsets=np.array([0, 1, 1], np.int32), jlist=np.array([1], np.int32))
    K, E = coeff_tables(1, 1000.0, 1.25)
    return case, K, E, oracle_compute(oracle, case, nq, K, E, want_pairs=True)


def test_caps_with_no_and_with_one_inside_node(oracle):
    """One isolated pair whose bounding spheres overlap while no cap node is inside the neighbour, and one a hair closer:
    exactly one node inside (the separation at which the first node enters is bisected with the oracle; just below it
    S_n is one node's term and varies smoothly).  Every other lane of the slab has weight 0: S_n, T_n equal the oracle's
    — exactly 0 for the empty cap — and V has the oracle's sign."""
    from shpair import shapes
    lmax, nq = 6, 16
    a = shapes.random_shape(lmax, 4242, amp=0.2)
    rmax = oracle.shape_rmax(lmax, a)

    def snorm(sep):
        return np.abs(_isolated(oracle, lmax, nq, a, rmax, sep)[3]["pairs"][0, 1:4]).max()
    hi, lo = 2.0 * rmax * (1 - 1e-9), 1.2 * rmax      # hi: bounding spheres just overlap
    assert snorm(hi) == 0.0 and snorm(lo) > 0.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if snorm(mid) > 0.0 else (lo, mid)
    one = lo - 1e-6 * rmax
    s1, s2 = snorm(one), snorm(lo - 2e-6 * rmax)
    assert s1 > 0 and abs(s2 - s1) < 1e-2 * s1       # the same single node on both sides: no second one entered
    for sep, empty in ((hi, True), (one, False)):      # hi: the last separation without an inside node, spheres overlapping
        case, K, E, o = _isolated(oracle, lmax, nq, a, rmax, sep)
        for spec in (1, 0):
            f, tq, _, pr, _ = run_pairs(case, nq, K, E, {"spec": spec}, eflag=False)
            if empty:
                assert not o["pairs"].any() and not pr.any() and not f.any() and not tq.any()
            else:
                scale = np.abs(o["pairs"][0]).max()
                assert np.abs(pr[0, 1:] - o["pairs"][0, 1:]).max() < TOL * scale
                # (V itself is a node 1e-6 R deep: r_i^3 - r_in^3 carries the searches' tolerances of both sides at
                # ~1e-9 relative, and the force V^(m-1) S_n with it — the sign only)
                assert np.sign(pr[0, 0]) == np.sign(o["pairs"][0, 0]) == 1.0
