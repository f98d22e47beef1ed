"""CPU-only checks of the translating-wall entry points of include/shstep.h (docs/SPEC.md §2.12): the cross-compiled
library exports them, the ctypes binding lists them with the header's arity, the gfx950 code object holds each new kernel
once without spills or scratch, and a null context is refused."""
import ctypes
import importlib.util
import os
import re

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVE = ("shstep_set_wall_velocity", "shstep_advance_walls_device", "shstep_get_walls")
KERNELS = ("wall_moving_damped_kernel", "wall_moving_friction_kernel", "wall_advance_kernel")


def test_library_exports_the_moving_wall_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in MOVE:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]), name   # same number of arguments
    for method in ("wall_velocity", "advance_walls_device", "get_walls"):
        assert callable(getattr(capi.ShPair, method))


def test_moving_wall_kernels_are_in_the_code_object_once_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    scr = M.scratch_instruction_counts(capi.library_path())
    for name in KERNELS:
        hit = [k for s, k in ks.items() if name in s]
        assert len(hit) == 1, (name, len(hit))
        assert hit[0]["vgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0 and scr.get(hit[0]["symbol"], 0) == 0, hit[0]
        # the names the older wall tests count must stay one each
        assert not any(old in hit[0]["symbol"] for old in ("wall_contact_kernel", "wall_candidates_kernel", "wall_rows_partial_kernel",
                                                           "wall_rows_final_kernel"))


def test_a_null_context_is_refused():
    lib = capi.load_library()
    v = (ctypes.c_double * 3)(0.0, 0.0, 1.0)
    p = (ctypes.c_double * 4)()
    assert lib.shstep_set_wall_velocity(None, 1, v) != 0            # refused, not dereferenced
    assert lib.shstep_advance_walls_device(None, 1e-3, None) != 0
    assert lib.shstep_get_walls(None, 1, p) != 0
