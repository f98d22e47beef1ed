"""Reference for the index machinery of docs/SPEC.md §7 that does not go through the oracle: the wrap as properties,
the periodic images by comparisons alone, the half list from a scipy cKDTree, and the bin-grid rule restated.  Plain
numpy; the only arithmetic shared with the kernels is the cut test of the half list, written as §7 writes it."""
import numpy as np
from scipy.spatial import cKDTree

FAR_WRAPS = 1.0e6          # a coordinate further than this many box lengths away is left alone (like NaN)
MAX_CELLS_DIR = 1024       # bin-grid rule: cells per direction ...
MAX_CELLS = 1 << 26        # ... and in all


def wrap_faults(x_before, x_after, lo, hi, periodic):
    """What is wrong with a wrap, as a list of strings (empty: nothing).  Properties, not bits: the device may
    contract p - k*len into an FMA.
      - a periodic coordinate lies in [lo, hi) afterwards and differs from the input by an integer number of box
        lengths (hi - lo rounded to double, what both sides hold) to within 2 ulp of max(|p|, |hi|);
      - one already inside, an open coordinate, NaN, and anything further than 1e6 box lengths away keep their bits.
    The wrap count floor((p - lo) / len) is taken from a rounded quotient: within 1e-6 of the bound either answer is
    accepted."""
    xb, xa = np.asarray(x_before, dtype=np.float64), np.asarray(x_after, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    faults = []
    if xb.shape != xa.shape:
        return ["shapes differ"]
    same = xb.view(np.int64) == xa.view(np.int64)
    for d in range(3):
        b, a, eq = xb[:, d], xa[:, d], same[:, d]
        if not periodic[d]:
            if not eq.all():
                faults.append(f"dim {d}: open coordinate changed at rows {np.nonzero(~eq)[0][:5].tolist()}")
            continue
        ln = hi[d] - lo[d]
        with np.errstate(invalid="ignore", over="ignore"):
            q = (b - lo[d]) / ln
            inside = (b >= lo[d]) & (b < hi[d])
        # |floor(q)| < 1e6 is q in [-999 999, 1e6); the device's quotient may round the other way next to those two
        far = ~((q >= 1.0 - FAR_WRAPS) & (q < FAR_WRAPS))           # NaN counts as far
        either = (np.abs(q - FAR_WRAPS) < 1e-6) | (np.abs(q - (1.0 - FAR_WRAPS)) < 1e-6)
        keep = inside | (far & ~either)                             # must keep their bits
        if not eq[keep].all():
            faults.append(f"dim {d}: a coordinate inside the box, NaN or too far away changed at rows "
                          f"{np.nonzero(keep & ~eq)[0][:5].tolist()}")
        w = ~keep & ~(either & eq)                                  # must have been wrapped
        if not w.any():
            continue
        bw, aw = b[w], a[w]
        out = ~((aw >= lo[d]) & (aw < hi[d]))
        if out.any():
            faults.append(f"dim {d}: outside [lo, hi) after the wrap at rows {np.nonzero(w)[0][out][:5].tolist()}")
        # in extended precision, so that the check adds no rounding of its own at the scale of a double ulp
        diff = bw.astype(np.longdouble) - aw.astype(np.longdouble)
        m = np.rint(diff / np.longdouble(ln))
        resid = np.abs(diff - m * np.longdouble(ln)).astype(np.float64)
        tol = 2.0 * np.spacing(np.maximum(np.abs(bw), abs(hi[d])))
        bad = ~(resid <= tol)
        if bad.any():
            r = np.nonzero(w)[0][bad][:5]
            faults.append(f"dim {d}: not a whole number of box lengths at rows {r.tolist()} "
                          f"(off by {resid[bad][:5].tolist()}, allowed {tol[bad][:5].tolist()})")
    return faults


def wrap_ok(x_before, x_after, lo, hi, periodic):
    return not wrap_faults(x_before, x_after, lo, hi, periodic)


def images(xw, lo, hi, periodic, cmax):
    """§7 borders on wrapped positions, by comparisons only: (own[ng], code[ng]), owner-major, code ascending;
    code = (s_z+1)*9 + (s_y+1)*3 + (s_x+1)."""
    xw = np.asarray(xw, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    n = xw.shape[0]
    up = [bool(periodic[d]) & (xw[:, d] < lo[d] + cmax) for d in range(3)]      # an image one box length up exists
    down = [bool(periodic[d]) & (xw[:, d] >= hi[d] - cmax) for d in range(3)]
    want = np.zeros((n, 27), dtype=bool)
    for code in range(27):
        if code == 13:
            continue
        s = (code % 3 - 1, (code // 3) % 3 - 1, code // 9 - 1)
        ok = np.ones(n, dtype=bool)
        for d in range(3):
            if s[d] == 1:
                ok &= up[d]
            elif s[d] == -1:
                ok &= down[d]
        want[:, code] = ok
    own, code = np.nonzero(want)
    return own.astype(np.int32), code.astype(np.int32)


def shift_of(code):
    """(ng, 3) image shifts of shift codes."""
    code = np.asarray(code)
    return np.stack([code % 3 - 1, (code // 3) % 3 - 1, code // 9 - 1], axis=1)


def half_list(nlocal, x_all, shtype_all, tag_all, rmax, skin):
    """§7 half list from a non-periodic cKDTree over all rows (owned + ghost): (offs[nlocal+1], jl), int32.  (i, j) is
    listed iff i < nlocal, tag_i < tag_j and d2 < cut^2 with cut = (rmax_i + skin) + rmax_j; rows by i, entries by j."""
    x = np.asarray(x_all, dtype=np.float64)
    sh = np.asarray(shtype_all)
    tag = np.asarray(tag_all)
    rmax = np.asarray(rmax, dtype=np.float64)
    fin = np.nonzero(np.isfinite(x).all(axis=1))[0]        # a row with NaN is within the cut of nothing
    empty = np.zeros(nlocal + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if fin.size < 2:
        return empty
    reach = (2.0 * rmax.max() + skin) * (1.0 + 1e-9)        # the tree only proposes; the test below decides
    p = cKDTree(x[fin]).query_pairs(reach, output_type="ndarray")
    if p.shape[0] == 0:
        return empty
    a, b = fin[p[:, 0]], fin[p[:, 1]]
    i, j = np.concatenate([a, b]), np.concatenate([b, a])   # both orders: which one is listed is up to the tags
    keep = (i < nlocal) & (tag[i] < tag[j])
    i, j = i[keep], j[keep]
    dx, dy, dz = x[i, 0] - x[j, 0], x[i, 1] - x[j, 1], x[i, 2] - x[j, 2]
    cut = (rmax[sh[i]] + skin) + rmax[sh[j]]
    keep = dx * dx + dy * dy + dz * dz < cut * cut
    i, j = i[keep], j[keep]
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    offs = np.zeros(nlocal + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=nlocal), out=offs[1:])
    return offs.astype(np.int32), j.astype(np.int32)


def cell_grid(lo, hi, periodic, cmax):
    """The bin grid of §7: per direction floor(extent / c_max) cells (the extent of a periodic direction has a ghost
    layer of c_max on either side), at least 1 and at most 1024; then the direction with the most cells (the first of
    equals) is halved, rounding up, until there are at most 2^26 cells.  Returns [nx, ny, nz]."""
    nc = []
    for d in range(3):
        ext = float(hi[d]) - float(lo[d])
        if periodic[d]:
            ext += 2.0 * cmax
        n = np.floor(ext / cmax)
        nc.append(int(min(max(n, 1.0), MAX_CELLS_DIR)) if n == n else 1)
    while nc[0] * nc[1] * nc[2] > MAX_CELLS:
        d = nc.index(max(nc))
        nc[d] = (nc[d] + 1) // 2
    return nc
