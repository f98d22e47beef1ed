"""tests/step_ref.py (wrap properties, images by comparison, cKDTree half list, bin-grid rule) pinned against the CPU
oracle and against hand-computed grids, before the GPU tests of tests/test_gpu_step_scale.py rest on it."""
import numpy as np
import pytest

import step_ref
from common import random_boxes
from shpair import shapes


@pytest.fixture(scope="module")
def rmax2(oracle):
    # the two shapes of test_random_boxes_ghosts_and_lists_match_oracle (tests/test_gpu_step.py)
    return np.array([oracle.shape_rmax(3, shapes.random_shape(3, 70, amp=0.15)),
                     oracle.shape_rmax(3, shapes.random_shape(3, 71, amp=0.3))])


def test_images_and_half_list_equal_the_oracle_on_the_random_boxes(oracle, rmax2):
    nghost = npairs = 0
    seen_periodic = set()
    for case in random_boxes(rmax2):
        lo, hi, periodic, cmax, n = (case[k] for k in ("lo", "hi", "periodic", "cmax", "n"))
        xw = case["x"].copy()
        own, shift = oracle.borders(xw, lo, hi, periodic, cmax)
        assert step_ref.wrap_ok(case["x"], xw, lo, hi, periodic), step_ref.wrap_faults(case["x"], xw, lo, hi, periodic)
        r_own, r_code = step_ref.images(xw, lo, hi, periodic, cmax)
        assert np.array_equal(r_own, own), case["trial"]
        assert np.array_equal(step_ref.shift_of(r_code), shift), case["trial"]
        xa = np.concatenate([xw, xw[own] + shift * case["edge"]])
        tag = np.concatenate([np.arange(n), own]).astype(np.int32)
        sha = np.concatenate([case["shtype"], case["shtype"][own]])
        o_offs, o_jl = oracle.half_list(n, xa, sha, tag, rmax2, case["skin"])
        offs, jl = step_ref.half_list(n, xa, sha, tag, rmax2, case["skin"])
        assert offs.dtype == np.int32 and jl.dtype == np.int32
        assert np.array_equal(offs, o_offs) and np.array_equal(jl, o_jl), case["trial"]
        nghost += own.size
        npairs += jl.size
        seen_periodic.add(periodic)
    assert nghost > 1000 and npairs > 5000 and len(seen_periodic) >= 6


def test_half_list_follows_the_tags_and_skips_rows_with_nan(oracle):
    rng = np.random.default_rng(11)
    n, nlocal = 400, 300
    x = rng.uniform(0, 9, (n, 3))
    sh = rng.integers(0, 2, n).astype(np.int32)
    tag = rng.permutation(n).astype(np.int32) + 7
    rmax = np.array([0.5, 0.8])
    o = oracle.half_list(nlocal, x, sh, tag, rmax, 0.1)
    r = step_ref.half_list(nlocal, x, sh, tag, rmax, 0.1)
    assert np.array_equal(r[0], o[0]) and np.array_equal(r[1], o[1]) and r[1].size > nlocal
    x[5, 1] = np.nan
    o = oracle.half_list(nlocal, x, sh, tag, rmax, 0.1)
    r = step_ref.half_list(nlocal, x, sh, tag, rmax, 0.1)
    assert np.array_equal(r[0], o[0]) and np.array_equal(r[1], o[1])
    assert r[0][5] == r[0][6] and 5 not in r[1]
    e = step_ref.half_list(3, x[:1], sh[:1], tag[:1], rmax, 0.1)
    assert e[0].tolist() == [0, 0, 0, 0] and e[1].size == 0


def test_wrap_ok_rejects_wrong_wraps(oracle):
    rng = np.random.default_rng(12)
    lo, hi, periodic = np.array([-3.0, 1.0, 2.0]), np.array([5.0, 8.5, 6.0]), (1, 1, 0)
    box = hi - lo
    x = lo + rng.uniform(-1.5, 2.5, (200, 3)) * box
    x[7:9] = lo + 0.25 * box                          # two rows inside, with one coordinate each that no wrap may touch
    x[7, 0] = np.nan
    x[8, 1] = lo[1] + 2.5e6 * box[1]                 # too far: left alone
    xw = x.copy()
    oracle.borders(xw[:7], lo, hi, periodic, 1.0)   # views: wrapped in place, the NaN and the far row kept out of its loops
    oracle.borders(xw[9:], lo, hi, periodic, 1.0)
    assert step_ref.wrap_ok(x, xw, lo, hi, periodic), step_ref.wrap_faults(x, xw, lo, hi, periodic)
    moved = np.nonzero(xw[:, 0] != x[:, 0])[0]
    assert moved.size > 50
    bad = xw.copy()
    bad[moved[0], 0] = hi[0]                          # exactly at hi: outside [lo, hi)
    assert not step_ref.wrap_ok(x, bad, lo, hi, periodic)
    bad = xw.copy()
    r = moved[xw[moved, 0] < lo[0] + 0.5 * box[0]][0]
    bad[r, 0] += 0.5 * box[0]                         # inside the box, but half a box off
    assert lo[0] <= bad[r, 0] < hi[0]
    assert not step_ref.wrap_ok(x, bad, lo, hi, periodic)
    bad = xw.copy()
    bad[3, 2] = np.nextafter(bad[3, 2], np.inf)       # an open coordinate changed by one ulp
    assert not step_ref.wrap_ok(x, bad, lo, hi, periodic)
    # three more that a sloppy wrap could make: the NaN or the far coordinate touched, a coordinate inside moved a whole box
    bad = xw.copy()
    bad[7, 0] = lo[0]
    assert not step_ref.wrap_ok(x, bad, lo, hi, periodic)
    bad = xw.copy()
    bad[8, 1] = lo[1]
    assert not step_ref.wrap_ok(x, bad, lo, hi, periodic)
    # ... and one 4e-15 off where 2 ulp of max(|p|, |hi|) is 1.8e-15 (|p| < 8, hi = 5)
    small = moved[(np.abs(x[moved, 0]) < 8.0) & (xw[moved, 0] + 1e-14 < hi[0])][0]
    bad = xw.copy()
    bad[small, 0] += 4e-15
    assert not step_ref.wrap_ok(x, bad, lo, hi, periodic)


def test_cell_grid_on_hand_computed_cases():
    c = 2.5                                           # (k + 0.5) * 2.5 is exact in binary
    z3 = np.zeros(3)

    def grid(cells, periodic=(0, 0, 0)):
        return step_ref.cell_grid(z3, (np.array(cells) + 0.5) * c, periodic, c)
    # the table of tests/test_gpu_step_scale.py: floor((k + 0.5) c / c) = k cells per open direction
    assert grid([32, 32, 1]) == [32, 32, 1]                              # 1024 cells
    assert grid([41, 25, 1]) == [41, 25, 1]                              # 1025
    assert grid([1024, 1024, 1]) == [1024, 1024, 1]                      # 2^20
    assert grid([1024, 41, 25]) == [1024, 41, 25]                        # 2^20 + 1024
    assert grid([1024, 513, 2]) == [1024, 513, 2]                        # 1 050 624
    assert grid([1024, 1024, 3]) == [1024, 1024, 3]                      # 3 * 2^20
    # capped to 1024 per direction (2^30 cells), then halved x, y, z, x: 2^29, 2^28, 2^27, 2^26
    assert grid([1100, 1100, 1100]) == [256, 512, 512]
    assert grid([5000, 1100, 70000]) == [256, 512, 512]
    # a periodic direction carries a ghost layer on both sides: two more cells; an open edge shorter than c_max is one cell
    assert step_ref.cell_grid(z3, np.array([4.5 * c, 4.5 * c, 0.3 * c]), (1, 0, 0), c) == [6, 4, 1]
    assert step_ref.cell_grid(np.array([-7.0, 1.0, 2.0]), np.array([-7.0 + 2 * c, 1.0 + 3.75 * c, 2.0 + c]), (1, 1, 1), c) == [4, 5, 3]
    # halving rounds up and takes the first of equal directions: 1023 * 300 * 300 = 92 070 000 > 2^26 -> 512 * 300 * 300
    assert grid([1023, 300, 300]) == [512, 300, 300]
    assert grid([300, 1023, 300]) == [300, 512, 300]
    # 2^26 itself is allowed, one more cell per row is not: 1024 * 1024 * 64 stays, 1024 * 1024 * 65 -> 512 * 1024 * 65
    assert grid([1024, 1024, 64]) == [1024, 1024, 64]
    assert grid([1024, 1024, 65]) == [512, 1024, 65]
