"""Checks of the cylinder-rolling entry points of include/shstep.h (docs/SPEC.md §2.21).  CPU: the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the methods and properties exist, the gfx950 code
object holds each of the two new kernels once without vector spills or scratch, a null context is refused, and the
binding's flag shadow follows the library's rules.  On the GPU (a context needs a device): the argument refusals and their
words, the reset by shstep_set_cylinders, and the ledger refusals in both orders with their lifting by the shell ledger."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from shpair import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = ("shstep_set_rolling_cyl", "shstep_set_twisting_cyl")
KERNELS = ("cyl_roll_kernel", "cyl_roll_ledger_kernel")


def test_library_exports_the_cylinder_rolling_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in SETTERS:
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in include/shstep.h"
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]) == 4, name   # same number of arguments
    for method in ("cylinder_rolling", "cylinder_twisting"):
        assert callable(getattr(capi.ShPair, method))
        assert callable(getattr(capi._StepFlags, method))
    assert isinstance(capi.ShPair.has_cyl_rolling, property)
    import inspect
    from shpair import step_pass
    par = inspect.signature(step_pass.apply_contact_options).parameters
    assert par["cylinder_rolling"].default is None and par["cylinder_twisting"].default is None


def test_cyl_roll_kernels_are_in_the_code_object_once_without_spills():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    ks = {k["symbol"]: k for k in M.kernels(capi.library_path())}
    scr = M.scratch_instruction_counts(capi.library_path())
    for name in KERNELS:
        hit = [k for s, k in ks.items() if re.search(r"\d" + name + "E", s)]     # the mangled name holds <length><name>E
        assert len(hit) == 1, (name, len(hit))
        assert hit[0]["vgpr_spills"] == 0 and hit[0]["scratch_bytes"] == 0 and scr.get(hit[0]["symbol"], 0) == 0, hit[0]
        assert "wall_roll" not in hit[0]["symbol"]


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 3)()
    assert lib.shstep_set_rolling_cyl(None, 1, t, t) == -1
    assert lib.shstep_set_twisting_cyl(None, 1, t, t) == -1


def test_the_flag_shadow_follows_the_two_setters_and_set_cylinders():
    """The predicates the drivers decide by (no library call: a fresh shadow and the flag methods the setters call)."""
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._flags.set_cylinders(3)
    assert not sp.has_cyl_rolling and not sp.cylinder_reads_twists and not sp.has_dissipation
    sp._flags.cylinder_rolling([0.05, 0.0, 0.0], [0.0, 3.0, 0.0])        # a mu_r without a gamma_r on the same cylinder
    assert not sp.has_cyl_rolling and not sp.cylinder_reads_twists
    sp._flags.cylinder_rolling([0.05, 0.0, 0.0], [2.0, 3.0, 0.0])
    assert sp.has_cyl_rolling and sp.cylinder_reads_twists and sp.has_dissipation
    assert not sp.has_cyl_history and not sp.has_wall_rolling and not sp.wall_reads_twists and not sp.keeps_integrals
    sp._flags.cylinder_rolling(np.zeros(3), np.zeros(3))
    assert not sp.has_cyl_rolling and not sp.has_dissipation
    sp._flags.cylinder_twisting([0.0, 0.0, 0.03], [0.0, 0.0, 0.0])
    assert not sp.has_cyl_rolling
    sp._flags.cylinder_twisting([0.0, 0.0, 0.03], [0.0, 0.0, 2.0])
    assert sp.has_cyl_rolling and sp.cylinder_reads_twists
    sp._flags.cylinder_rolling([0.05, 0.05, 0.05], [1.0, 1.0, 1.0])
    sp._flags.cylinder_twisting(np.zeros(3), np.zeros(3))
    assert sp.has_cyl_rolling                                             # rolling still on
    sp._flags.set_cylinders(3)                                            # shstep_set_cylinders resets all four
    assert not sp.has_cyl_rolling and not sp.cylinder_reads_twists and not sp.has_dissipation
    sp._h = None


def _ctx():
    from dissipation_common import _wall_ctx
    from shpair import shapes
    return _wall_ctx([(0, shapes.sphere(1.0))], 8)


CYL = np.array([0.3, -0.2, 0.5, 2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0, 4.0])


@pytest.mark.gpu
def test_argument_refusals_their_words_and_the_reset_by_set_cylinders(oracle):
    from shpair.capi import ShPairError
    sp = _ctx()
    with pytest.raises(ShPairError, match=r"cylinder rolling resistance: 1 coefficients for 0 cylinders \(call it after shstep_set_cylinders\)") as e:
        sp._chk(sp._lib.shstep_set_rolling_cyl(sp._h, 1, (ctypes.c_double * 1)(0.1), (ctypes.c_double * 1)(1.0)))
    assert e.value.code == -1
    sp.set_cylinders([CYL, CYL], 1000.0, 1.25)
    with pytest.raises(ShPairError, match="cylinder twisting resistance: 3 coefficients for 2 cylinders"):
        sp.cylinder_twisting([0.1, 0.1, 0.1], [1.0, 1.0, 1.0])
    with pytest.raises(ShPairError, match="cylinder rolling resistance: null array pointer"):
        sp._chk(sp._lib.shstep_set_rolling_cyl(sp._h, 2, None, (ctypes.c_double * 2)(1.0, 1.0)))
    with pytest.raises(ShPairError, match=r"cylinder 1: rolling coefficient mu_r -0.5 must be finite and >= 0") as e:
        sp.cylinder_rolling([0.1, -0.5], [1.0, 1.0])
    assert e.value.code == -1
    with pytest.raises(ShPairError, match=r"cylinder 0: twisting coefficient gamma_tw nan must be finite"):
        sp.cylinder_twisting([0.1, 0.1], [np.nan, 1.0])
    with pytest.raises(ShPairError, match=r"cylinder 1: rolling coefficient gamma_r inf must be finite"):
        sp.cylinder_rolling([0.1, 0.1], [1.0, np.inf])
    assert not sp.has_cyl_rolling and not sp.cylinder_reads_twists       # a refused call changes nothing
    sp.cylinder_rolling([0.1, 0.0], [1.0, 0.0])
    sp.cylinder_twisting(0.03, 2.0)                                       # a scalar: every cylinder
    assert sp.has_cyl_rolling and sp.cylinder_reads_twists and sp.has_dissipation
    sp.set_cylinders([CYL], 1000.0, 1.25)                                 # resets all four
    assert not sp.has_cyl_rolling and not sp.cylinder_reads_twists
    sp.set_energy_ledger(True)                                            # the library agrees: no cylinder coefficient is set
    sp.set_energy_ledger(False)
    sp.close()


@pytest.mark.gpu
def test_the_ledger_refusals_in_both_orders_and_their_lifting_by_the_shell_ledger(oracle):
    from shpair.capi import ShPairError
    sp = _ctx()
    sp.set_cylinders([CYL], 1000.0, 1.25)
    # the energy ledger first: the setters refuse, with the words of every cylinder coefficient
    sp.set_energy_ledger(True)
    with pytest.raises(ShPairError, match="cylinder rolling resistance: the energy ledger is on and keeps no cylinder entries") as e:
        sp.cylinder_rolling(0.05, 3.0)
    assert e.value.code == -4 and not sp.has_cyl_rolling
    with pytest.raises(ShPairError, match="cylinder twisting resistance: the energy ledger is on and keeps no cylinder entries"):
        sp.cylinder_twisting(0.03, 2.0)
    sp.cylinder_rolling(0.05, 0.0)                                        # no kind: allowed
    sp.set_energy_ledger(False)
    # the coefficients first: the ledger refuses, with a message of its own while rolling or twisting is all that is set
    sp.cylinder_twisting(0.03, 2.0)
    with pytest.raises(ShPairError, match="energy ledger: cylinder rolling or twisting resistance is set and the ledger keeps no cylinder") as e:
        sp.set_energy_ledger(True)
    assert e.value.code == -4 and not sp.ledger_on
    sp.cylinder_damping(2.0)                                              # ... and the older words where an older coefficient is set too
    with pytest.raises(ShPairError, match="cylinder damping or friction coefficient is set and the ledger keeps no cylinder"):
        sp.set_energy_ledger(True)
    sp.cylinder_damping(0.0)
    sp.cylinder_friction(0.5, 0.0)
    sp.set_cyl_tangential_spring(4e3)
    with pytest.raises(ShPairError, match="cylinder tangential spring is set and the ledger keeps no cylinder"):
        sp.set_energy_ledger(True)
    sp.set_cyl_tangential_spring(0.0)
    # the shell ledger lifts both
    sp.set_shell_ledger(True)
    sp.set_energy_ledger(True)
    assert sp.ledger_on and sp.has_cyl_rolling
    sp.cylinder_rolling(0.05, 3.0)
    with pytest.raises(ShPairError, match="energy ledger is on and a cylinder coefficient"):   # off would recreate the refused state
        sp.set_shell_ledger(False)
    sp.cylinder_rolling(0.0, 0.0)
    sp.cylinder_twisting(0.0, 0.0)
    sp.set_shell_ledger(False)                                            # nothing is set: allowed, and the refusal is back
    with pytest.raises(ShPairError, match="cylinder twisting resistance: the energy ledger is on"):
        sp.cylinder_twisting(0.03, 2.0)
    sp.close()
