"""CPU-only checks of the energy-ledger entry points of include/shstep.h (docs/SPEC.md §2.13): the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the gfx950 code object holds the new kernels without
spills or scratch, and the argument checks that need no device refuse a null context."""
import ctypes
import importlib.util
import os
import re

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER = ("shstep_set_energy_ledger", "shstep_ledger_fold_device", "shstep_get_energy_ledger", "shstep_reset_energy_ledger")
KERNELS = ("pair_damp_ledger_kernel", "pair_dissipation_ledger_kernel", "wall_ledger_damped_kernel", "wall_ledger_friction_kernel",
           "wall_ledger_moving_damped_kernel", "wall_ledger_moving_friction_kernel", "ledger_pair_partial_kernel",
           "ledger_wall_partial_kernel", "ledger_final_kernel")


def test_library_exports_the_ledger_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in LEDGER:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]), name   # same number of arguments
    for method in ("set_energy_ledger", "ledger_fold_device", "energy_ledger", "reset_energy_ledger"):
        assert callable(getattr(capi.ShPair, method))
    from shpair.run import DeviceRun
    assert callable(DeviceRun.ledger)


def test_ledger_kernels_are_in_the_code_object_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    for name in KERNELS:
        hit = [k for s, k in ks.items() if name in s]
        assert len(hit) == 1, (name, len(hit))
        assert hit[0]["vgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0, hit[0]


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 5)()
    assert lib.shstep_set_energy_ledger(None, 1) == -1
    assert lib.shstep_ledger_fold_device(None, 1.0, None) == -1
    assert lib.shstep_get_energy_ledger(None, t, 0, None) == -1
    assert lib.shstep_reset_energy_ledger(None) == -1
