"""CPU-only checks of the wall-rolling entry points of include/shstep.h (docs/SPEC.md §2.17): the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the methods and properties exist, the gfx950 code
object holds each of the two new kernels once without vector spills or scratch, a null context is refused, and the
binding's flag shadow follows the library's rules: a kind is on iff both of its coefficients are non-zero on some wall."""
import ctypes
import importlib.util
import os
import re

import numpy as np

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = ("shstep_set_wall_rolling", "shstep_set_wall_twisting")
KERNELS = ("wall_roll_kernel", "wall_roll_ledger_kernel")
# the names the older *_capi.py files search the code object for, several of them by substring
OLDER = ("rolling_pair_kernel", "rolling_gather_kernel", "wall_ledger_", "wall_contact_kernel", "wall_candidates_kernel",
         "wall_rows_partial_kernel", "wall_rows_final_kernel", "wall_contact_damped_kernel", "wall_moving_damped_kernel",
         "wall_moving_friction_kernel", "wall_advance_kernel", "pair_history_", "history_key_kernel", "history_carry_kernel",
         "twist_kernel", "pair_damp_kernel", "ledger_final_kernel")


def test_library_exports_the_wall_rolling_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in SETTERS:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]) == 4, name   # same number of arguments
    for method in ("wall_rolling", "wall_twisting"):
        assert callable(getattr(capi.ShPair, method))
        assert callable(getattr(capi._StepFlags, method))
    assert isinstance(capi.ShPair.has_wall_rolling, property)
    import inspect
    from shpair import step_pass
    par = inspect.signature(step_pass.apply_contact_options).parameters
    assert par["wall_rolling"].default is None and par["wall_twisting"].default is None


def test_wall_roll_kernels_are_in_the_code_object_once_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    scr = M.scratch_instruction_counts(capi.library_path())
    for name in KERNELS:
        hit = [k for s, k in ks.items() if re.search(r"\d" + name + "E", s)]     # the mangled name holds <length><name>E
        assert len(hit) == 1, (name, len(hit))
        assert hit[0]["vgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0 and scr.get(hit[0]["symbol"], 0) == 0, hit[0]
        assert not any(old in hit[0]["symbol"] for old in OLDER), hit[0]["symbol"]


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 3)()
    assert lib.shstep_set_wall_rolling(None, 1, t, t) == -1
    assert lib.shstep_set_wall_twisting(None, 1, t, t) == -1


def test_the_flag_shadow_follows_the_two_setters_and_set_walls():
    """The predicates the drivers decide by (no library call: a fresh shadow and the flag methods the setters call)."""
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._flags.set_walls(np.eye(3))
    assert not sp.has_wall_rolling and not sp.wall_reads_twists and not sp.has_dissipation
    # a mu_r without a gamma_r on the same wall is no rolling resistance
    sp._flags.wall_rolling([0.05, 0.0, 0.0], [0.0, 3.0, 0.0])
    assert not sp.has_wall_rolling and not sp.wall_reads_twists
    sp._flags.wall_rolling([0.05, 0.0, 0.0], [2.0, 3.0, 0.0])
    assert sp.has_wall_rolling and sp.wall_reads_twists and sp.has_dissipation
    assert not sp.has_wall_history and not sp.fric_walls and not sp.keeps_integrals      # nothing else moves with it
    sp._flags.wall_rolling(np.zeros(3), np.zeros(3))
    assert not sp.has_wall_rolling and not sp.has_dissipation
    # twisting alone, and the two kinds are independent
    sp._flags.wall_twisting([0.0, 0.0, 0.03], [0.0, 0.0, 0.0])
    assert not sp.has_wall_rolling
    sp._flags.wall_twisting([0.0, 0.0, 0.03], [0.0, 0.0, 2.0])
    assert sp.has_wall_rolling and sp.wall_reads_twists
    sp._flags.wall_rolling([0.05, 0.05, 0.05], [1.0, 1.0, 1.0])
    sp._flags.wall_twisting(np.zeros(3), np.zeros(3))
    assert sp.has_wall_rolling                                                           # rolling still on
    sp._flags.set_walls(np.eye(3))                                                       # shstep_set_walls resets all four
    assert not sp.has_wall_rolling and not sp.wall_reads_twists and not sp.has_dissipation
    sp._h = None
