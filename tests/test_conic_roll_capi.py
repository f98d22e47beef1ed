"""Checks of the cone-rolling entry points of include/shstep.h (docs/SPEC.md §2.24).  CPU: the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the methods, the property and the options exist, the
gfx950 code object holds the new kernel once without vector spills or scratch, a null context is refused, and the
binding's flag shadow follows the library's rules in either order of the setters.  (The refusals that need a context, and
so a device, are tests/test_gpu_conic_roll.py's.)"""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = ("shstep_set_rolling_con", "shstep_set_twisting_con")
KERNEL = "conic_roll_kernel"
# the substring searches of the older tests: the new kernel's symbol must match none of them
OLDER_SEARCHES = ("cone_contact", "cyl_", "wall_", "rolling_", "history_", "ledger_", "conic_spring_kernel", "conic_live_sweep_kernel")


def test_library_exports_the_cone_rolling_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in SETTERS:
        assert "cone" not in name and "conic" not in name       # the older tests pin those two sets of declarations
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]) == 4, name   # same number of arguments
    for method in ("conic_rolling", "conic_twisting"):
        assert callable(getattr(capi.ShPair, method))
        assert callable(getattr(capi._StepFlags, method))
    assert isinstance(capi.ShPair.has_conic_rolling, property)
    from shpair import step_pass
    par = inspect.signature(step_pass.apply_contact_options).parameters
    assert par["conic_rolling"].default is None and par["conic_twisting"].default is None
    names = list(par)
    assert names.index("conic_spring") < names.index("conic_rolling") < names.index("conic_twisting")


def test_the_conic_roll_kernel_is_in_the_code_object_once_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    scr = M.scratch_instruction_counts(capi.library_path())
    hit = [k for s, k in ks.items() if re.search(r"\d" + KERNEL + "E", s)]     # the mangled name holds <length><name>E
    assert len(hit) == 1, len(hit)
    assert hit[0]["vgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0 and scr.get(hit[0]["symbol"], 0) == 0, hit[0]
    assert not [w for w in OLDER_SEARCHES if w in hit[0]["symbol"]], hit[0]["symbol"]
    assert len([s for s in ks if "conic_roll" in s]) == 1                     # no ledger twin: cones keep no ledger entries


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 3)()
    assert lib.shstep_set_rolling_con(None, 1, t, t) == -1
    assert lib.shstep_set_twisting_con(None, 1, t, t) == -1


def test_the_flag_shadow_follows_the_two_setters_in_either_order_and_set_cones():
    """The predicates the drivers decide by (no library call: a fresh shadow and the flag methods the setters call)."""
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._flags.set_cones(3)
    assert not sp.has_conic_rolling and not sp.cone_reads_twists and not sp.has_dissipation
    sp._flags.conic_rolling([0.05, 0.0, 0.0], [0.0, 3.0, 0.0])            # a mu_r without a gamma_r on the same cone
    assert not sp.has_conic_rolling and not sp.cone_reads_twists
    sp._flags.conic_rolling([0.05, 0.0, 0.0], [2.0, 3.0, 0.0])
    assert sp.has_conic_rolling and sp.cone_reads_twists and sp.has_dissipation
    assert not sp.has_conic_history and not sp.has_cyl_rolling and not sp.has_wall_rolling and not sp.keeps_integrals
    assert not sp.cylinder_reads_twists and not sp.wall_reads_twists
    sp._flags.conic_rolling(np.zeros(3), np.zeros(3))
    assert not sp.has_conic_rolling and not sp.has_dissipation
    sp._flags.conic_twisting([0.0, 0.0, 0.03], [0.0, 0.0, 0.0])
    assert not sp.has_conic_rolling
    sp._flags.conic_twisting([0.0, 0.0, 0.03], [0.0, 0.0, 2.0])
    assert sp.has_conic_rolling and sp.cone_reads_twists
    sp._flags.conic_rolling([0.05, 0.05, 0.05], [1.0, 1.0, 1.0])          # twisting then rolling ...
    sp._flags.conic_twisting(np.zeros(3), np.zeros(3))
    assert sp.has_conic_rolling                                           # rolling still on
    sp._flags.set_cones(3)                                                # shstep_set_cones resets all four
    assert not sp.has_conic_rolling and not sp.cone_reads_twists and not sp.has_dissipation
    sp._flags.conic_rolling(0.05, 1.0)                                    # ... and rolling then twisting: the same state
    sp._flags.conic_twisting(0.03, 2.0)
    assert sp.has_conic_rolling and sp.cone_reads_twists and not sp.has_conic_history
    sp._flags.cone_friction(np.full(3, 0.5), np.zeros(3))                 # the spring's flags are not disturbed
    sp._flags.conic_spring(np.full(3, 4e3))
    assert sp.has_conic_history and sp.has_conic_rolling
    sp._flags.set_cones(0)
    assert not sp.has_conic_rolling and not sp.has_conic_history
    sp._h = None
