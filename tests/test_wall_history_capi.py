"""CPU-only checks of the wall-history entry points of include/shstep.h (docs/SPEC.md §2.15): the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the gfx950 code object holds each new kernel once
without vector spills or scratch (the bar of tests/test_wall_move_capi.py for the instances of this body), a null context is
refused, and the binding's flag shadow follows the library's rules."""
import ctypes
import importlib.util
import os
import re

import numpy as np

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HISTORY = ("shstep_set_wall_tangential_spring", "shstep_wall_contact_device", "shstep_copy_wall_history",
           "shstep_set_wall_history", "shstep_reset_wall_history")
KERNELS = ("wall_spring_kernel", "wall_spring_moving_kernel", "wall_spring_ledger_kernel", "wall_spring_moving_ledger_kernel",
           "wall_spring_sweep_kernel")
# the names the older *_capi.py files search the code object for, several of them by substring
OLDER = ("wall_contact_kernel", "wall_candidates_kernel", "wall_rows_partial_kernel", "wall_rows_final_kernel",
         "wall_contact_damped_kernel", "wall_moving_damped_kernel", "wall_moving_friction_kernel", "wall_advance_kernel",
         "wall_ledger_", "pair_history_", "history_key_kernel", "history_carry_kernel", "twist_kernel", "pair_damp_kernel",
         "ledger_final_kernel")


def test_library_exports_the_wall_history_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in HISTORY:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]), name   # same number of arguments
    for method in ("set_wall_tangential_spring", "wall_contact_device", "wall_history", "set_wall_history", "reset_wall_history"):
        assert callable(getattr(capi.ShPair, method))
    from shpair.run import DeviceRun
    assert callable(DeviceRun.wall_history)


def test_wall_history_kernels_are_in_the_code_object_once_without_spills():
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
    assert lib.shstep_set_wall_tangential_spring(None, 1, t) == -1
    assert lib.shstep_wall_contact_device(None, 0, None, None, None, None, 1, None, None, None, None, 0.0, None) == -1
    assert lib.shstep_copy_wall_history(None, 1, t) == -1
    assert lib.shstep_set_wall_history(None, 1, t) == -1
    assert lib.shstep_reset_wall_history(None) == -1


def test_the_binding_keeps_the_librarys_flags():
    """The predicates the drivers decide by (no library call: a fresh shadow and the flag methods the setters call)."""
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._flags.set_walls(np.eye(3))
    assert not sp.has_wall_history and not sp.wall_reads_twists and not sp.fric_walls
    # spring first, friction second: wall 0 has mu and k_t (gamma_t = 0), wall 1 has mu and gamma_t, wall 2 only a k_t
    sp._flags.wall_spring([5.0, 0.0, 7.0])
    assert not sp.has_wall_history and not sp.wall_reads_twists      # a k_t without a mu is no history
    sp._flags.wall_friction([0.5, 0.3, 0.0], [0.0, 10.0, 10.0])
    assert sp.has_wall_history and sp.wall_reads_twists and sp.has_dissipation and sp.fric_walls
    first = (sp.has_wall_history, sp.fric_walls, sp.wall_reads_twists)
    # ... and the other order gives the same state
    sp._flags.set_walls(np.eye(3))
    assert not sp.has_wall_history and not sp.fric_walls             # set_walls clears the spring and the friction
    sp._flags.wall_friction([0.5, 0.3, 0.0], [0.0, 10.0, 10.0])
    assert not sp.has_wall_history and sp.fric_walls
    sp._flags.wall_spring([5.0, 0.0, 7.0])
    assert (sp.has_wall_history, sp.fric_walls, sp.wall_reads_twists) == first
    # history with gamma_t = 0 everywhere: no friction instance, but the pass still reads twists
    sp._flags.wall_friction([0.5, 0.0, 0.0], [0.0, 0.0, 0.0])
    assert sp.has_wall_history and not sp.fric_walls and sp.wall_reads_twists
    sp._flags.wall_spring([0.0, 0.0, 0.0])                           # the last k_t gone
    assert not sp.has_wall_history and not sp.wall_reads_twists
    sp._flags.wall_spring(np.full(3, 2.0))
    sp._flags.set_walls(np.eye(3))                                   # shstep_set_walls resets every k_t,w
    assert not sp.has_wall_history
    sp._h = None
