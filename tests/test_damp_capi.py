"""CPU-only checks of the damping entry points of include/shstep.h (docs/SPEC.md §2.10): the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the gfx950 code object holds the new kernels without
spills or scratch, and the argument checks that need no device refuse a null context."""
import ctypes
import importlib.util
import os
import re

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAMP = ("shstep_set_pair_damping", "shstep_set_wall_damping", "shstep_twist_device", "shstep_pair_damping_device",
        "shstep_wall_force_damped_device")


def test_library_exports_the_damping_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in DAMP:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]), name   # same number of arguments
    for method in ("pair_damping", "wall_damping", "twist_device", "pair_damping_device", "wall_force_damped_device"):
        assert callable(getattr(capi.ShPair, method))


def test_damping_kernels_are_in_the_code_object_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    for name in ("twist_kernel", "pair_damp_kernel", "wall_contact_damped_kernel"):
        hit = [k for s, k in ks.items() if name in s]
        assert len(hit) == 1, (name, len(hit))
        assert hit[0]["vgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0, hit[0]


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    g = (ctypes.c_double * 1)(1.0)
    assert lib.shstep_set_pair_damping(None, 1, 1, 1.0) == -1
    assert lib.shstep_set_wall_damping(None, 1, g) == -1
    assert lib.shstep_twist_device(None, 0, 0, None, None, None, None, None, None) == -1
    assert lib.shstep_pair_damping_device(None, 0, 0, None, None, None, 1, None, None, None) == -1
    assert lib.shstep_wall_force_damped_device(None, 0, None, None, None, None, 1, None, None, None, None, None) == -1
