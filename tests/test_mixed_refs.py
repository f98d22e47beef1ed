"""CPU checks behind the tests of mixed orders (tests/test_gpu_mixed_orders.py): the references agree with themselves —
a shape at its own order gives what its zero-padded expansion gives — before they judge the kernels, every bed has the
touching slots of both mixed orientations the GPU tests need, and the library's stateless mass-properties entry point
agrees with the oracle at the orders one context mixes.

The gate of the self-comparisons is 1e-12 of the largest magnitude: the size of the perturbation the whole-step
reference uses for its own sensitivity D_q (tests/golden/make_traj_ref.py)."""
import numpy as np
import pytest

from common import coeff_tables
from mixed_common import (BEDS, WALL_NQ, bed_case, wall_case, pad_anm, own_tuples, padded_tuples, mixed_oracle_compute,
                          assert_mixed_slots, soup_case, soup_branches, MIN_BRANCH_PAIRS)

SELF_GATE = 1e-12


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def test_pad_anm_keeps_the_coefficients_and_appends_zeros():
    a = np.arange(1.0, 13.0)                       # order 2: 6 terms
    p = pad_anm(2, 5, a)
    assert p.size == 6 * 7 and np.array_equal(p[:12], a) and not p[12:].any()
    assert np.array_equal(pad_anm(2, 2, a), a)


@pytest.mark.parametrize("name", list(BEDS))
def test_oracle_own_order_equals_zero_padded(oracle, name):
    case, nq = bed_case(name, oracle.shape_rmax)
    K, E = coeff_tables(case["ntypes"], 1000.0, 1.25)
    kw = dict(eflag=True, vflag=True, want_pairs=True, nthreads=8)
    own = mixed_oracle_compute(oracle, case, nq, K, E, **kw)
    pad = mixed_oracle_compute(oracle, case, nq, K, E, padded=True, **kw)
    cls = assert_mixed_slots(case, own["pairs"])
    fs = np.abs(own["f"]).max()
    d = dict(f=np.abs(pad["f"] - own["f"]).max() / fs,
             torque=np.abs(pad["torque"] - own["torque"]).max() / max(fs, np.abs(own["torque"]).max()),
             energy=abs(pad["eng_virial"][0] - own["eng_virial"][0]) / abs(own["eng_virial"][0]),
             virial=rel(pad["eng_virial"][1:], own["eng_virial"][1:]),
             pairs=(np.abs(pad["pairs"] - own["pairs"]) / np.abs(own["pairs"]).max(axis=0)).max())
    print(f"{name}: slots {cls}, own order against padded {({k: float(f'{v:.1e}') for k, v in d.items()})}")
    assert fs > 0 and max(d.values()) < SELF_GATE
    assert np.array_equal(pad["counts"], own["counts"])


def test_soup_oracle_own_order_equals_zero_padded(oracle):
    soup = soup_case(oracle.shape_rmax)
    K, E = coeff_tables(1, 1000.0, 1.25)
    res = [oracle.compute(t, K, E, 16, 2 * soup["npair"], soup["x"], soup["quat"], soup["type"], soup["shtype"], soup["ilist"],
                          soup["offsets"], soup["jlist"], eflag=True, want_pairs=True, nthreads=8)
           for t in (own_tuples(soup), padded_tuples(soup))]
    d = (np.abs(res[1]["pairs"] - res[0]["pairs"]) / np.abs(res[0]["pairs"]).max(axis=0)).max()
    br = soup_branches(soup, res[0]["pairs"])
    print(f"soup (1, 5, 9): touching pairs by cap branch and orientation {br.tolist()}, own order against padded {d:.1e}")
    assert br.min() >= MIN_BRANCH_PAIRS
    assert d < SELF_GATE and rel(res[1]["f"], res[0]["f"]) < SELF_GATE


def test_wall_reference_own_order_equals_zero_padded(oracle):
    import wall_ref as W
    c = wall_case(oracle.shape_rmax)
    own = W.wall_forces(own_tuples(c), WALL_NQ, c["x"], c["quat"], c["shtype"], c["planes"], c["kn"], c["expo"])
    pad = W.wall_forces(padded_tuples(c), WALL_NQ, c["x"], c["quat"], c["shtype"], c["planes"], c["kn"], c["expo"])
    touching = np.abs(own["f"]).max(axis=1) > 0
    per_shape = np.bincount(c["shtype"][touching], minlength=3)
    d = dict(f=rel(pad["f"], own["f"]), torque=np.abs(pad["torque"] - own["torque"]).max() / np.abs(own["f"]).max(),
             wall=rel(pad["wall_out"], own["wall_out"]))
    print(f"walls: particles in contact per shape {per_shape.tolist()}, own order against padded {d}")
    assert own["nbehind"] == 0 and per_shape.min() >= 15
    assert max(d.values()) < SELF_GATE and own["ncontacts"] == pad["ncontacts"]


@pytest.mark.parametrize("l,L", [(0, 8), (3, 8), (8, 8), (2, 4), (4, 6), (12, 13), (0, 20)])
def test_mass_props_own_order_equals_zero_padded(oracle, l, L):
    from shpair import shapes
    a = shapes.random_shape(l, 40 + l, amp=0.3)
    own, pad = oracle.mass_props(l, a), oracle.mass_props(L, pad_anm(l, L, a))
    d = np.abs(pad - own).max() / np.abs(own).max()
    print(f"mass_props ({l} in {L}): {d:.1e}")
    assert d < SELF_GATE


def test_library_mass_props_at_the_orders_of_one_context(oracle):
    """shstep_shape_mass_props, the stateless form of the table a context builds per shape at the shape's own order
    (csrc/shstep_api.hip: mass_props(sh.lmax, ...)), at the orders (0, 3, 8): against the oracle at the own order, with
    the tolerance of tests/test_gpu_step.py::test_body_table_matches_oracle.  The table of a context itself needs a GPU:
    tests/test_gpu_mixed_orders.py::test_body_table_of_mixed_orders."""
    from shpair import capi, shapes
    for l in (0, 3, 8):
        a = shapes.random_shape(l, 31 + l, amp=0.3)
        mp = oracle.mass_props(l, a)
        assert np.abs(capi.shape_mass_props(l, a) - mp).max() < 1e-13
        assert np.abs(capi.shape_mass_props(8, pad_anm(l, 8, a)) - mp).max() < 1e-13


@pytest.mark.parametrize("frozen", [True, False], ids=["frozen-rows", "all-moving"])
def test_whole_step_scene_meets_its_conditions(frozen):
    """The scene of the whole-step GPU tests, from the reference alone: 24 particles of both orders, a rebuild within the
    run whose decision margins are at least 1e-6, every ledger column filled, and, for the two-rank run, at least 5 slots in
    contact that join a low-order and a high-order row owned by different bricks of a 2x1x1 grid."""
    from mixed_common import step_reference, assert_step_conditions
    ref = step_reference(frozen)
    print("rebuilt", ref["rebuilt"], "smallest margin", min(ref["margin"]), "touching", ref["touching"], "cross-rank mixed slots",
          len(ref["cross_mixed"]), "\nD", ref["D"])
    assert_step_conditions(ref, frozen)
    assert all(0 < ref["D"][q] < 1e-10 for q in ("x", "v", "quat", "angmom", "ledger"))
