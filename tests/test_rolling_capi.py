"""CPU-only checks of the rolling and twisting entry points of include/shstep.h (docs/SPEC.md §2.16): the cross-compiled
library exports them, the ctypes binding lists them with the header's arity, the gfx950 code object holds the new kernels
exactly once each without spills or scratch, and the argument checks that need no device refuse a null context."""
import ctypes
import importlib.util
import os
import re

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLING = ("shstep_set_pair_rolling", "shstep_set_pair_twisting", "shstep_pair_rolling_device")


def test_library_exports_the_rolling_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ROLLING:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]), name   # same number of arguments
    for method in ("pair_rolling", "pair_twisting", "pair_rolling_device"):
        assert callable(getattr(capi.ShPair, method))
    assert isinstance(capi.ShPair.has_rolling, property)


def test_rolling_kernels_are_in_the_code_object_once_each_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    for name in ("rolling_pair_kernel", "rolling_pair_ledger_kernel", "rolling_gather_kernel"):
        hit = [k for s, k in ks.items() if name in s]
        assert len(hit) == 1, (name, len(hit))
        assert hit[0]["vgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0, hit[0]


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    assert lib.shstep_set_pair_rolling(None, 1, 1, 0.1, 1.0) == -1
    assert lib.shstep_set_pair_twisting(None, 1, 1, 0.1, 1.0) == -1
    assert lib.shstep_pair_rolling_device(None, 0, 0, None, None, None, 1, None, None) == -1


def test_the_flag_shadow_follows_the_two_setters():
    """has_rolling / has_pair_pass / keeps_integrals / has_dissipation as shp_has_rolling, shp_has_pair_pass,
    shp_keeps_integrals and step_has_dissipation of the library: a kind counts iff both of its coefficients are non-zero,
    and the pair coefficients go with the type table."""
    sp = capi.ShPair.__new__(capi.ShPair)      # no context, no library: only what the object remembers
    sp._reset_shadow()
    state = lambda: (sp.has_rolling, sp.has_pair_pass, sp.keeps_integrals, sp.has_dissipation)
    assert state() == (False, False, False, False)
    sp._flags.pair_rolling(1, 2, 0.05, 0.0)
    sp._flags.pair_twisting(1, 1, 0.0, 2.0)
    assert state() == (False, False, False, False)
    sp._flags.pair_rolling(2, 1, 0.05, 2.0)
    assert state() == (True, False, True, True)
    sp._flags.pair_rolling(1, 2, 0.0, 0.0)      # symmetric: one pair
    assert state() == (False, False, False, False)
    sp._flags.pair_twisting(1, 1, 0.02, 2.0)
    sp._flags.pair_damping(1, 1, 5.0)
    assert state() == (True, True, True, True)
    sp._flags.pair_twisting(1, 1, 0.02, 0.0)
    assert state() == (False, True, True, True)
    sp._flags.pair_rolling(1, 1, 0.05, 2.0)
    sp._flags.set_ntypes()
    assert state() == (False, False, False, False)
