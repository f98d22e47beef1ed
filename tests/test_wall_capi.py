"""CPU-only checks of the wall entry points of include/shstep.h (docs/SPEC.md §2.9): the cross-compiled library exports
them, the ctypes binding lists them with the header's arity, the gfx950 code objects hold the wall kernels without
spills or scratch, and without a GPU they are unreachable like the rest (no context, no CPU fallback)."""
import ctypes
import importlib.util
import os
import re

import pytest

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALL = ("shstep_set_walls", "shstep_wall_force_device", "shstep_wall_force", "shstep_get_wall_stats")


def test_library_exports_the_wall_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in WALL:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]), name   # same number of arguments
    assert re.search(r"#define\s+SHSTEP_MAX_WALLS\s+32\b", txt)


def test_wall_kernels_are_in_the_code_object_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    for name in ("wall_candidates_kernel", "wall_contact_kernel", "wall_rows_partial_kernel", "wall_rows_final_kernel"):
        hit = [k for s, k in ks.items() if name in s]
        assert len(hit) == 1, (name, len(hit))   # one instance each: the contact kernel serves every order
        assert hit[0]["vgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0, hit[0]


def test_without_a_gpu_the_wall_calls_are_unreachable(gpu_available):
    if gpu_available:
        pytest.skip("GPU present: covered by tests/test_gpu_wall.py")
    with pytest.raises(capi.ShPairError):
        capi.ShPair(0)   # no context, hence no wall call: there is no CPU fallback
    lib = capi.load_library()
    n = ctypes.c_int(7)
    assert lib.shstep_set_walls(None, 0, None, None, None) != 0            # a null context is refused, not dereferenced
    assert lib.shstep_get_wall_stats(None, ctypes.byref(n)) != 0
    assert lib.shstep_wall_force(None, 0, None, None, None, None, 1, None, None, None) != 0
