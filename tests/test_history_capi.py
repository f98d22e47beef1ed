"""CPU-only checks of the tangential-history entry points of include/shstep.h (docs/SPEC.md §2.14): the cross-compiled
library exports them, the ctypes binding lists them with the header's arity, the gfx950 code object holds the new kernels
without spills or scratch, and the argument checks that need no device refuse a null context."""
import ctypes
import importlib.util
import os
import re

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HISTORY = ("shstep_set_pair_tangential_spring", "shstep_pair_contact_device", "shstep_copy_contact_history",
           "shstep_set_contact_history", "shstep_reset_contact_history")
KERNELS = ("pair_history_kernel", "pair_history_ledger_kernel", "history_key_kernel", "history_carry_kernel")


def test_library_exports_the_history_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in HISTORY:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]), name   # same number of arguments
    for method in ("set_pair_tangential_spring", "pair_contact_device", "contact_history", "set_contact_history",
                   "reset_contact_history"):
        assert callable(getattr(capi.ShPair, method))
    from shpair.run import DeviceRun
    assert callable(DeviceRun.contact_history)


def test_history_kernels_are_in_the_code_object_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    for name in KERNELS:
        hit = [k for s, k in ks.items() if re.search(r"\d" + name + "E", s)]     # the mangled name holds <length><name>E
        assert len(hit) == 1, (name, len(hit))
        assert hit[0]["vgpr_spills"] == 0 and hit[0]["sgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0, hit[0]


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 3)()
    assert lib.shstep_set_pair_tangential_spring(None, 1, 1, 1.0) == -1
    assert lib.shstep_pair_contact_device(None, 0, 0, None, None, None, None, 1, 0.0, None, None, None) == -1
    assert lib.shstep_copy_contact_history(None, t) == -1
    assert lib.shstep_set_contact_history(None, t) == -1
    assert lib.shstep_reset_contact_history(None) == -1


def test_the_binding_keeps_the_librarys_flags():
    """The predicates the drivers decide by (no library call: a fresh shadow and the flag methods the setters call)."""
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    assert not sp.has_history and not sp.keeps_integrals
    sp._flags.pair_spring(2, 1, 5.0)
    assert sp.has_history and sp.keeps_integrals and sp.has_dissipation
    sp._flags.pair_spring(1, 2, 0.0)
    assert not sp.has_history and not sp.keeps_integrals
    sp._flags.pair_spring(1, 1, 5.0)
    sp._flags.set_ntypes()                       # shpair_set_ntypes resets the springs with the type table
    assert not sp.has_history
    sp._h = None
