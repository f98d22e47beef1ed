"""The index machinery of docs/SPEC.md §7 (wrap and image count, ghost fill, counting sort into bins, half list,
interior / boundary partition, and the three-pass exclusive scan under all of them) against tests/step_ref.py, at the
sizes where it takes another path: more than one chunk of the scan of the block sums (2^20 cells, rows or slots), the
cap and the halving of the bin grid, and row counts either side of a wave, a workgroup and a scan block.  Nothing here
goes through the oracle: wraps are checked as properties, ghosts by comparisons, lists against a cKDTree.

Which line, if wrong, fails which test (csrc/step_kernels.hpp, shstep_api.hip):
  - scan_sums_kernel, `sums[i] = carry + ex` / `carry += total`: without the carry the block sums of every chunk but
    the first start again at 0.  In the cell scan the start of cell 2^20 then equals that of cell 0: the clumps put into
    both (and either side of every further multiple of 2^20) share slots of the sorted atom array, one overwrites the
    other, and rows of the list lose or swap neighbours - the cases of 1025, 1026, 3072 and 65 536 blocks.  In the row
    scans the ghost offsets and list offsets of rows >= 2^20 fall back, `out[n]` (ghost count, pair count) comes out
    short: test_more_than_2_20_owned_rows fails at its first count; in the slot scan of the partition the interior
    slots behind slot 2^20 land on those in front: the forces of test_more_than_2_20_list_slots_and_the_partition.
  - its loop bounds (`base < nblocks`, `i < nblocks`, `base += kScanBlock`): 1024 blocks end the loop exactly, 1025
    leave one block for the second pass, `sums[nblocks]` is written behind a chunk boundary.
  - block_exclusive_scan's wave and workgroup seams, scan_local / scan_apply's `i < n`: 63 ... 2049 rows, 1024 and
    1025 cells.
  - step_refresh_box: the cap and the halving decide nc[], binv[] follows from them; cell_of and half_list_kernel
    must agree on the linear index (c_z n_y + c_y) n_x + c_x of a 256 x 512 x 512 grid and of grids with n_x != n_y
    != n_z (a transposed index passes on the cubic boxes of the other tests), and the clamp into the edge cells must
    keep particles beyond an open face next to their neighbours.
  - wrap_count_kernel's face corrections and image_wanted's `<` / `>=`: test_faces_of_the_wrap_and_the_image_thresholds
    puts a coordinate on every one of them and one ulp either side."""
import numpy as np
import pytest

import step_ref
from common import random_quats

pytestmark = pytest.mark.gpu

SCAN_BLOCK = 1024                   # entries per block of the scan; its middle pass walks 1024 block sums per chunk
CHUNK = SCAN_BLOCK * SCAN_BLOCK
LO = np.array([-1.0, 0.5, 2.0])     # no box here starts at 0, and |hi| > |lo| (the bound of step_ref.wrap_faults)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def make_ctx(shp, lmax, nq=8, kn=1000.0, expo=1.25):
    from shpair import ShPair
    sp = ShPair(0)
    sp.settings(nq)
    sp.set_ntypes(1, len(shp))
    for s, a in enumerate(shp):
        sp.set_shape(s, lmax, a)
    sp.coeff(1, 1, kn, expo)
    return sp, np.array([sp.rmax(s) for s in range(len(shp))])


@pytest.fixture(scope="module")
def shp3():
    from shpair import shapes
    return [shapes.random_shape(3, 70, amp=0.15), shapes.random_shape(3, 71, amp=0.3)]


# ---- a. the cell scan across chunk boundaries ---------------------------------------------------------------------

def _linear_cell(x, lo, hi, nc):
    """The bin of a position in an open box (clamped into the edge cells), for the tests' own preconditions."""
    w = (hi - lo) / np.array(nc)
    c = np.clip(np.floor((x - lo) / w), 0, np.array(nc) - 1).astype(np.int64)
    return (c[:, 2] * nc[1] + c[:, 1]) * nc[0] + c[:, 0]


def _clump_case(kedge, rmax, skin, seed):
    """Open box with edges (k + 0.5) c_max and a few hundred particles in clumps of 2 to 6 within the cut of each
    other.  Clump centres: the middle of cell 0, of the last cell, of the cells either side of every multiple of 2^20
    and of a few multiples of 1024 in the linear cell index, and of random cells; on faces between cells; a quarter of
    a cell in (after the halving of the grid: on a face of the unhalved cells); beyond and on the open faces."""
    rng = np.random.default_rng(seed)
    cmax = 2 * rmax.max() + skin
    lo = LO.copy()
    hi = lo + (np.array(kedge) + 0.5) * cmax
    nc = step_ref.cell_grid(lo, hi, (0, 0, 0), cmax)
    ncell = nc[0] * nc[1] * nc[2]
    w = (hi - lo) / np.array(nc)
    need = {0, ncell - 1}
    for m in range(1, ncell // CHUNK + 1):
        need |= {m * CHUNK - 1, min(m * CHUNK, ncell - 1)}
    nblk = ncell // SCAN_BLOCK
    for m in rng.choice(np.arange(1, nblk + 1), min(3, nblk), replace=False):
        need |= {int(m) * SCAN_BLOCK - 1, min(int(m) * SCAN_BLOCK, ncell - 1)}
    need = sorted(need)
    cells = np.array(need + rng.integers(0, ncell, max(12, 80 - len(need))).tolist(), dtype=np.int64)
    c3 = np.stack([cells % nc[0], (cells // nc[0]) % nc[1], cells // (nc[0] * nc[1])], axis=1)
    centres = [lo + (c3 + 0.5) * w]                                   # the middle of a cell
    for frac in (1.0, 0.25):                                          # on a face between two cells; a quarter in
        r3 = np.stack([rng.integers(0, max(1, nc[d] - 1), 6) for d in range(3)], axis=1)
        off = np.full((6, 3), 0.5)
        off[np.arange(6), rng.integers(0, 3, 6)] = frac
        off[:, np.array(nc) == 1] = 0.5                               # a direction of one cell has no inner face
        centres.append(lo + (r3 + off) * w)
    r3 = np.stack([rng.integers(0, nc[d], 8) for d in range(3)], axis=1)
    out = lo + (r3 + 0.5) * w
    d = rng.integers(0, 3, 8)
    up = rng.integers(0, 2, 8).astype(bool)
    dist = np.where(np.arange(8) < 6, rng.uniform(0.5, 4.0, 8), 0.0) * cmax     # six beyond an open face, two on it
    out[np.arange(8), d] = np.where(up, hi[d] + dist, lo[d] - dist)
    centres.append(out)
    centres = np.concatenate(centres)
    size = rng.integers(2, 7, centres.shape[0])
    if size.sum() > 560:                                              # many chunk boundaries: smaller clumps
        size = np.where(rng.uniform(size=size.size) < 0.1, 2, rng.integers(3, 5, size.size))
    reach = 0.4 * (2 * rmax.min() + skin)                             # any two of a clump are within the smallest cut
    x = []
    for ctr, k in zip(centres, size):
        v = rng.normal(size=(k, 3))
        v *= (reach * rng.uniform(0.2, 1.0, (k, 1)) / np.linalg.norm(v, axis=1, keepdims=True))
        v[:, np.array(nc) == 1] *= 0.2
        x.append(ctr + v)
    x = np.concatenate(x)
    x = x[rng.permutation(x.shape[0])]
    n = x.shape[0]
    return dict(n=n, x=x, lo=lo, hi=hi, nc=nc, ncell=ncell, need=need, skin=skin, cmax=cmax,
                shtype=rng.integers(0, len(rmax), n).astype(np.int32))


def _check_open_list(sp, case, rmax):
    """Preconditions on the CPU, then the device list of an open box (no ghosts) against the tree."""
    n, x, lo, hi = case["n"], case["x"], case["lo"], case["hi"]
    tag = np.arange(n, dtype=np.int32)
    r_offs, r_jl = step_ref.half_list(n, x, case["shtype"], tag, rmax, case["skin"])
    cell = _linear_cell(x, lo, hi, case["nc"])
    assert set(case["need"]) <= set(cell.tolist())
    assert 300 <= n <= 600 and r_jl.size > n
    ri = np.repeat(np.arange(n), np.diff(r_offs))
    assert (cell[ri] != cell[r_jl]).sum() >= 5                        # pairs across a cell face
    outside = ((x < lo) | (x >= hi)).any(axis=1)
    assert outside.sum() >= 10 and outside[ri].sum() >= 10            # beyond an open face, and listed
    sp.set_box(lo, hi, (0, 0, 0), case["skin"])
    xd, shd = dev(x), dev(case["shtype"])
    npairs = sp.neighbor_build_device(n, 0, xd.data_ptr(), shd.data_ptr())
    offs, jl = sp.copy_neighbors(n, npairs)
    print(f"cells {case['nc']} = {case['ncell']}, scan blocks {-(-case['ncell'] // SCAN_BLOCK)}, n {n}, npairs {npairs} "
          f"(reference {r_jl.size})")
    assert npairs == r_jl.size
    assert np.array_equal(offs, r_offs)
    assert np.array_equal(jl, r_jl)


@pytest.mark.parametrize("kedge,ncell,nblocks", [
    ((32, 32, 1), 1024, 1),
    ((41, 25, 1), 1025, 2),
    ((1024, 1024, 1), 1 << 20, 1024),             # one full chunk: the loop over the block sums ends exactly
    ((1024, 41, 25), (1 << 20) + 1024, 1025),     # the second chunk holds one block
    ((1024, 513, 2), 1050624, 1026),
    ((1024, 1024, 3), 3 << 20, 3072),             # three full chunks
])
def test_cell_scan_across_chunk_boundaries(shp3, kedge, ncell, nblocks):
    sp, rmax = make_ctx(shp3, 3)
    case = _clump_case(kedge, rmax, 0.1, 100 + nblocks)
    assert case["nc"] == list(kedge) and case["ncell"] == ncell and -(-ncell // SCAN_BLOCK) == nblocks
    try:
        _check_open_list(sp, case, rmax)
    finally:
        sp.close()


def test_capped_and_halved_grid_then_a_small_box_on_the_same_context(shp3):
    """Edges beyond 1024 c_max in all three directions: 1024 cells each, halved x, y, z, x down to 256 x 512 x 512 =
    2^26 cells, 65 536 scan blocks, 64 chunks; bins are 4.3 / 2.5 / 2.3 c_max wide.  Then a 3 x 3 x 3-cell box on the
    same context: the large buffers are reused with what the large grid left in them."""
    sp, rmax = make_ctx(shp3, 3)
    try:
        case = _clump_case((1100, 1300, 1200), rmax, 0.1, 200)
        assert case["nc"] == [256, 512, 512] and case["ncell"] == 1 << 26 and case["ncell"] // SCAN_BLOCK == 65536
        assert len(case["need"]) == 2 + 2 * 63 + 6
        # clumps that span two of the unhalved cells inside one halved cell
        n, x, lo, hi = case["n"], case["x"], case["lo"], case["hi"]
        r_offs, r_jl = step_ref.half_list(n, x, case["shtype"], np.arange(n), rmax, case["skin"])
        ri = np.repeat(np.arange(n), np.diff(r_offs))
        fine = _linear_cell(x, lo, hi, [1024, 1024, 1024])
        coarse = _linear_cell(x, lo, hi, case["nc"])
        assert ((fine[ri] != fine[r_jl]) & (coarse[ri] == coarse[r_jl])).sum() >= 5
        _check_open_list(sp, case, rmax)
        small = _clump_case((3, 3, 3), rmax, 0.1, 201)
        assert small["nc"] == [3, 3, 3]
        _check_open_list(sp, small, rmax)
    finally:
        sp.close()


# ---- b, c, d, e: periodic boxes -----------------------------------------------------------------------------------

def _lattice_case(m, nlocal, rmax, skin, seed, spacing=1.9, jitter=0.3, outside=3):
    """nlocal sites of an m^3 lattice bed (the bed of the periodic tests of tests/test_gpu_step.py), jittered, in
    random row order, the first few rows a box length outside."""
    rng = np.random.default_rng(seed)
    box = np.array([m, m, m]) * spacing
    g = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    assert nlocal <= g.shape[0]
    g = g[rng.permutation(g.shape[0])[:nlocal]]
    x = LO + (g + 0.5) * spacing + rng.uniform(-jitter, jitter, (nlocal, 3))
    x[:outside] -= box
    return dict(n=nlocal, lo=LO.copy(), hi=LO + box, periodic=(1, 1, 1), skin=skin, cmax=2 * rmax.max() + skin, x=x,
                quat=random_quats(rng, nlocal), type=np.ones(nlocal, dtype=np.int32),
                shtype=rng.integers(0, len(rmax), nlocal).astype(np.int32),
                tag=(rng.permutation(nlocal) + 1000).astype(np.int32))


class _Rows:
    """The caller's arrays on the device, nmax rows."""

    def __init__(self, case, nmax, with_tag):
        import torch
        n = case["n"]
        self.n, self.nmax = n, nmax
        self.x = torch.zeros(nmax, 3, dtype=torch.float64, device="cuda:0")
        self.q = torch.zeros(nmax, 4, dtype=torch.float64, device="cuda:0")
        self.ty = torch.zeros(nmax, dtype=torch.int32, device="cuda:0")
        self.sh = torch.zeros(nmax, dtype=torch.int32, device="cuda:0")
        self.tag = torch.zeros(nmax, dtype=torch.int32, device="cuda:0") if with_tag else None
        self.x[:n] = dev(case["x"]); self.q[:n] = dev(case["quat"])
        self.ty[:n] = dev(case["type"]); self.sh[:n] = dev(case["shtype"])
        if with_tag:
            self.tag[:n] = dev(case["tag"])

    def tag_ptr(self):
        return None if self.tag is None else self.tag.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check_borders(sp, case, rows):
    """borders_device against wrap properties and step_ref.images evaluated on the device's own wrapped positions.
    Returns (nghost, own, shift, all positions, all shape indices, all tags)."""
    n, lo, hi, periodic = case["n"], case["lo"], case["hi"], case["periodic"]
    ng = sp.borders_device(n, rows.nmax, rows.x.data_ptr(), rows.q.data_ptr(), rows.ty.data_ptr(), rows.sh.data_ptr(),
                           tag=rows.tag_ptr())
    xw = rows.x[:n].cpu().numpy()
    faults = step_ref.wrap_faults(case["x"], xw, lo, hi, periodic)
    assert not faults, faults
    own, code = step_ref.images(xw, lo, hi, periodic, case["cmax"])
    assert ng == own.size
    shift = step_ref.shift_of(code)
    xg, want = rows.x[n: n + ng].cpu().numpy(), xw[own] + shift * (hi - lo)
    assert np.array_equal(np.isnan(xg), np.isnan(want))
    if np.isfinite(want).any():
        assert np.nanmax(np.abs(xg - want)) <= 1e-13
    assert np.array_equal(_bits(rows.q[n: n + ng].cpu().numpy()), _bits(case["quat"][own]))
    assert np.array_equal(rows.sh[n: n + ng].cpu().numpy(), case["shtype"][own])
    assert np.array_equal(rows.ty[n: n + ng].cpu().numpy(), case["type"][own])
    if rows.tag is not None:
        assert np.array_equal(rows.tag[n: n + ng].cpu().numpy(), case["tag"][own])
        tags = np.concatenate([case["tag"], case["tag"][own]])
    else:
        tags = np.concatenate([np.arange(n), own]).astype(np.int32)       # without tags a ghost counts as its owner
    return ng, own, shift, rows.x[: n + ng].cpu().numpy(), np.concatenate([case["shtype"], case["shtype"][own]]), tags


def _check_list(sp, case, rows, ng, xa, sha, tags, rmax):
    n = case["n"]
    r_offs, r_jl = step_ref.half_list(n, xa, sha, tags, rmax, case["skin"])
    npairs = sp.neighbor_build_device(n, ng, rows.x.data_ptr(), rows.sh.data_ptr(), tag=rows.tag_ptr())
    offs, jl = sp.copy_neighbors(n, npairs)
    assert npairs == r_jl.size
    assert np.array_equal(offs, r_offs)
    assert np.array_equal(jl, r_jl)
    return r_offs, r_jl


@pytest.mark.parametrize("nlocal", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049])
def test_row_counts_at_wave_workgroup_and_scan_block_boundaries(shp3, nlocal):
    import torch
    sp, rmax = make_ctx(shp3, 3)
    try:
        m = int(np.ceil(nlocal ** (1 / 3) - 1e-9))
        case = _lattice_case(m, nlocal, rmax, 0.15, 300 + nlocal)
        n = nlocal
        sp.set_box(case["lo"], case["hi"], case["periodic"], case["skin"])
        rows = _Rows(case, 27 * n + 8, with_tag=nlocal % 2 == 1)
        ng, own, shift, xa, sha, tags = _check_borders(sp, case, rows)
        assert ng > n // 4 and (np.bincount(own) == 7).any()
        _, r_jl = _check_list(sp, case, rows, ng, xa, sha, tags, rmax)
        assert r_jl.size > n
        # forward: move the owners, ghosts follow; reverse: ghost forces fold into owners
        rows.x[:n] += 0.01
        rows.q[:n] = dev(random_quats(np.random.default_rng(1), n))
        sp.forward_device(rows.x.data_ptr(), rows.q.data_ptr())
        f = dev(np.random.default_rng(2).normal(size=(n + ng, 3)))
        t = dev(np.random.default_rng(3).normal(size=(n + ng, 3)))
        f0, t0 = f.cpu().numpy().copy(), t.cpu().numpy().copy()
        sp.reverse_device(f.data_ptr(), t.data_ptr())
        torch.cuda.synchronize()
        xs, qs = rows.x.cpu().numpy(), rows.q.cpu().numpy()
        assert np.abs(xs[n: n + ng] - (xs[own] + shift * (case["hi"] - case["lo"]))).max() <= 1e-13
        assert np.array_equal(_bits(qs[n: n + ng]), _bits(qs[:n][own]))
        fe, te = f0[:n].copy(), t0[:n].copy()
        np.add.at(fe, own, f0[n:])
        np.add.at(te, own, t0[n:])
        assert np.abs(f[:n].cpu().numpy() - fe).max() < 1e-13
        assert np.abs(t[:n].cpu().numpy() - te).max() < 1e-13
    finally:
        sp.close()


def _compute(sp, case, rows, ng):
    """One contact pass over the installed list; forces and torques of all rows, ghosts included."""
    import torch
    n = case["n"]
    f = torch.zeros(n + ng, 3, dtype=torch.float64, device="cuda:0")
    tq = torch.zeros_like(f)
    sp.compute_device(n, ng, rows.x.data_ptr(), rows.q.data_ptr(), rows.ty.data_ptr(), rows.sh.data_ptr(), f.data_ptr(),
                      tq.data_ptr())
    torch.cuda.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy()


def test_more_than_2_20_owned_rows(shp3):
    """102^3 = 1 061 208 particles, dilute: the scans over the owned rows (image counts, row lengths) and, in the
    deterministic mode, the scan over all rows that builds the reverse index take a second chunk."""
    sp, rmax = make_ctx(shp3, 3)
    try:
        m = 102
        case = _lattice_case(m, m ** 3, rmax, 0.1, 400, spacing=2.6, jitter=0.5, outside=1000)
        n = case["n"]
        assert n > CHUNK
        sp.set_box(case["lo"], case["hi"], case["periodic"], case["skin"])
        rows = _Rows(case, n + n // 8, with_tag=True)
        ng, own, shift, xa, sha, tags = _check_borders(sp, case, rows)
        assert (np.bincount(own) == 7).any() and own.max() > CHUNK
        r_offs, r_jl = _check_list(sp, case, rows, ng, xa, sha, tags, rmax)
        assert r_offs[CHUNK] < r_jl.size                              # rows behind the first chunk have entries
        print(f"n {n}, nghost {ng}, npairs {r_jl.size}")
        fa, ta = _compute(sp, case, rows, ng)
        sp.set_option("deterministic", 1)
        fd, td = _compute(sp, case, rows, ng)
        fd2, td2 = _compute(sp, case, rows, ng)
        fs = np.abs(fa).max()
        assert fs > 0 and (np.abs(fa[CHUNK:n]).max(axis=1) > 0).sum() > 100 and np.abs(fa[n:]).max() > 0
        assert np.abs(fd - fa).max() < 1e-12 * fs and np.abs(td - ta).max() < 1e-12 * fs
        assert np.array_equal(fd, fd2) and np.array_equal(td, td2)
    finally:
        sp.close()


def test_more_than_2_20_list_slots_and_the_partition():
    """57^3 particles at the spacing and jitter of the periodic tests, skin 0.2: about 5.8 slots per particle, so the scan
    over the slots that partitions the list (option "halo_overlap") takes a second chunk.  The context does not let
    Python read the interior count or the partitioned slots; the partition is held through the forces it produces."""
    from shpair import shapes
    shp = [shapes.random_shape(4, 50 + s, amp=0.2) for s in range(2)]
    got = []
    for overlap in (0, 2):
        sp, rmax = make_ctx(shp, 4)
        try:
            sp.set_option("halo_overlap", overlap)
            case = _lattice_case(57, 57 ** 3, rmax, 0.2, 70)
            n = case["n"]
            sp.set_box(case["lo"], case["hi"], case["periodic"], case["skin"])
            rows = _Rows(case, n + n // 2, with_tag=False)
            ng, own, shift, xa, sha, tags = _check_borders(sp, case, rows)
            if not got:
                ref = step_ref.half_list(n, xa, sha, tags, rmax, case["skin"])
                assert ref[1].size > CHUNK
                ninterior = int((ref[1] < n).sum())
                assert 0 < ninterior < ref[1].size and ref[1].size - ninterior > SCAN_BLOCK
                print(f"n {n}, nghost {ng}, npairs {ref[1].size}, interior {ninterior}")
            npairs = sp.neighbor_build_device(n, ng, rows.x.data_ptr(), rows.sh.data_ptr())
            offs, jl = sp.copy_neighbors(n, npairs)
            assert npairs == ref[1].size and np.array_equal(offs, ref[0]) and np.array_equal(jl, ref[1])
            got.append(_compute(sp, case, rows, ng))
        finally:
            sp.close()
    (f0, t0), (f2, t2) = got
    fs = np.abs(f0).max()
    assert fs > 0 and (np.abs(f0).max(axis=1) > 0).mean() > 0.5
    assert np.abs(f2 - f0).max() < 1e-12 * fs and np.abs(t2 - t0).max() < 1e-12 * fs


def test_faces_of_the_wrap_and_the_image_thresholds(shp3):
    """Coordinates at lo and hi, at the image thresholds lo + c_max and hi - c_max and one ulp either side of all four,
    999 999 and 1 000 001 box lengths away (the second is left alone), and one NaN."""
    sp, rmax = make_ctx(shp3, 3)
    try:
        skin = 0.15
        cmax = 2 * rmax.max() + skin
        rng = np.random.default_rng(500)
        lo = LO.copy()
        hi = lo + np.array([5.0, 6.5, 7.25]) * cmax
        box = hi - lo
        rows_x = []
        for d in range(3):
            faces = [lo[d], hi[d], lo[d] + cmax, hi[d] - cmax]
            vals = [v for f in faces for v in (np.nextafter(f, -np.inf), f, np.nextafter(f, np.inf))]
            vals += [lo[d] + s * k * box[d] + rng.uniform(0, 1) * box[d] for k in (999999, 1000001) for s in (1, -1)]
            vals += [lo[d] - box[d], hi[d] + box[d], lo[d] + 3 * box[d], np.nextafter(lo[d] - box[d], -np.inf)]
            for v in vals:
                p = lo + rng.uniform(0.3, 0.7, 3) * box           # the other two coordinates well inside
                p[d] = v
                rows_x.append(p)
        for u in (0, 1):                                          # corners: every coordinate at a face or a threshold
            for f in range(4):
                rows_x.append(np.array([(lo[d], hi[d], lo[d] + cmax, hi[d] - cmax)[(f + u * d) % 4] for d in range(3)]))
        nan_row = len(rows_x)
        rows_x.append(np.array([lo[0] + 0.1, np.nan, hi[2] - 0.1]))
        far = np.nonzero(np.abs((np.array(rows_x) - lo) / box) > 1.00000001e6)[0]
        rows_x += [lo + rng.uniform(0, 1, 3) * box for _ in range(40)]
        x = np.array(rows_x)
        n = x.shape[0]
        case = dict(n=n, lo=lo, hi=hi, periodic=(1, 1, 1), skin=skin, cmax=cmax, x=x, quat=random_quats(rng, n),
                    type=np.ones(n, dtype=np.int32), shtype=rng.integers(0, 2, n).astype(np.int32),
                    tag=(rng.permutation(n) + 50).astype(np.int32))
        sp.set_box(lo, hi, (1, 1, 1), skin)
        rows = _Rows(case, 27 * n + 8, with_tag=True)
        ng, own, shift, xa, sha, tags = _check_borders(sp, case, rows)
        xw = xa[:n]
        assert far.size == 6 and np.array_equal(_bits(xw[far]), _bits(x[far]))       # 1 000 001 lengths away: untouched
        assert np.isnan(xw[nan_row, 1]) and np.array_equal(xw[nan_row, ::2], x[nan_row, ::2])
        assert (np.bincount(own, minlength=n) == 7).sum() >= 2 and (own == nan_row).sum() == 3
        _check_list(sp, case, rows, ng, xa, sha, tags, rmax)
    finally:
        sp.close()
