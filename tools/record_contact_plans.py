"""Records the contact-kernel launch plan a build of libshpair chooses (shpair_get_kernel_info) over a grid of
(option set, L, n_q), one 2-particle compute per point: the fixture tests/golden/contact_plans.csv, which
tests/test_contact_plan.py checks the host planner (csrc/contact_plan.hpp) against on the CPU.
usage: python tools/record_contact_plans.py [lib.so] [--out FILE] [--lmax L ...]
lib.so is a file name in lammps-spherharm_amd/shpair (default libshpair.so), loaded the way tools/ab_libs.py does."""
import argparse
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-spherharm_amd"))

LMAX = list(range(13)) + [13, 16, 20]
NQ_FULL = list(range(1, 33)) + [40, 64, 128]
NQ_SHORT = [4, 10, 16, 24, 32]
# option set -> shpair_set_option settings; the full (L, n_q) grid for the first five, NQ_SHORT for the rest
OPTS = {
    "def": {}, "j0": {"jpoly": 0}, "s1": {"split": 1}, "s0": {"split": 0}, "r1": {"rule": 1},
    "qs0": {"queue_slack": 0}, "w2": {"waves_per_block": 2}, "w4": {"waves_per_block": 4},
    "rr4": {"ring_rows": 4}, "sp0": {"spec": 0}, "v1": {"variant": 1},
}
FULL = ("def", "j0", "s1", "s0", "r1")
FIELDS = ("family", "waves_per_pair", "ring_rows", "queue_entries", "lds_bytes_per_wave", "specialised")
HEADER = "opts,lmax,nq,rc," + ",".join(FIELDS)


def grid(lmaxes=LMAX):
    for name in OPTS:
        for L in lmaxes:
            for nq in (NQ_FULL if name in FULL else NQ_SHORT):
                yield name, L, nq


@functools.lru_cache(maxsize=None)
def _shape(shapes, L):
    return shapes.random_shape(L, 7)


def plan(capi, shapes, name, L, nq):
    """(rc, kernel_info fields) of one compute of a 2-particle bed; the fields are None when the compute failed."""
    sp = capi.ShPair(0)
    try:
        for k, v in OPTS[name].items():
            sp.set_option(k, v)
        sp.settings(nq)
        sp.set_ntypes(1, 1)
        sp.set_shape(0, L, _shape(shapes, L))
        sp.coeff("*", "*", 1000.0, 1.25)
        sp.set_neighbors_csr(np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([1], dtype=np.int32))
        x = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0]])
        q = np.array([[1.0, 0.0, 0.0, 0.0]] * 2)
        try:
            sp.compute(2, x, q, np.ones(2, dtype=np.int32), np.zeros(2, dtype=np.int32))
        except capi.ShPairError as e:
            return e.code, None
        k = sp.kernel_info()
        return 0, tuple(k[f] for f in FIELDS)
    finally:
        sp.close()


def row(name, L, nq, rc, fields):
    return f"{name},{L},{nq},{rc}," + (",".join(str(v) for v in fields) if fields else ",".join("" for _ in FIELDS))


def load_capi(lib):
    import torch  # noqa: F401  (binds the library to torch's HIP runtime, capi.load_library)
    from shpair import capi, shapes
    capi._LIB = None
    capi.library_path = lambda: os.path.join(ROOT, "lammps-spherharm_amd", "shpair", lib)
    return capi, shapes


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?", default="libshpair.so")
    ap.add_argument("--out", default=None, help="CSV file (default: stdout)")
    ap.add_argument("--lmax", type=int, nargs="*", default=LMAX)
    a = ap.parse_args()
    capi, shapes = load_capi(a.lib)
    lines = [HEADER] + [row(n, L, nq, *plan(capi, shapes, n, L, nq)) for n, L, nq in grid(a.lmax)]
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
