"""CPU-only checks of the shell-ledger entry points of include/shstep.h (docs/SPEC.md §2.20): the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the methods and options exist, the gfx950 code
object holds the four new kernels once each without vector spills or scratch and under names no older test matches, the
LEDGER instances take parameter structs of their own, a null context is refused, and the Python drivers set the switch
ahead of the coefficients and fold once per step."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np

from shpair import capi, run, step_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"shstep_set_shell_ledger": 2, "shstep_get_shell_ledger": 4}
KERNELS = ("cyl_power_dissipative_kernel", "cyl_power_spring_kernel", "cyl_power_partial_kernel", "cyl_power_final_kernel")
# the names the older tests search the code object for, several of them by substring
OLDER = ("cyl_contact", "cyl_spring_kernel", "ledger_", "wall_", "rolling_", "history_", "pair_contact", "twist_kernel", "pair_damp_kernel")


def test_library_exports_the_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(shstep_[a-z0-9_]*shell[a-z0-9_]*)\s*\(", txt))
    assert declared == set(ENTRY)
    for name, nargs in ENTRY.items():
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        assert "cylinder" not in name and "cyl_" not in name      # the older tests own those two families of names
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]) == nargs, name
    for method in ("set_shell_ledger", "shell_ledger"):
        assert callable(getattr(capi.ShPair, method)), method
    assert isinstance(capi.ShPair.shell_ledger_on, property)
    assert inspect.signature(step_pass.apply_contact_options).parameters["shell_ledger"].default is None
    assert inspect.signature(run.DeviceRun.__init__).parameters["shell_ledger"].default is None
    assert callable(run.DeviceRun.shell_ledger)


def test_the_new_kernels_are_in_the_code_object_once_without_spills():
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
    # parameter structs of their own: the arguments of the ordinary instances stay what they were
    assert "CylPowerParams" in [s for s in ks if "cyl_power_dissipative_kernel" in s][0]
    assert "CylPowerSpringParams" in [s for s in ks if "cyl_power_spring_kernel" in s][0]
    assert len([s for s in ks if "cyl_power_" in s]) == 4


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 27)()
    assert lib.shstep_set_shell_ledger(None, 1) == -1
    assert lib.shstep_get_shell_ledger(None, t, 0, t) == -1


class _Recorder:
    """A context stand-in that records the calls made on it; every unknown name is a callable."""

    def __init__(self, **flags):
        self.calls = []
        self.__dict__.update(flags)

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call


def test_the_switch_is_set_ahead_of_every_coefficient_and_none_leaves_it():
    sp = _Recorder()
    step_pass.apply_contact_options(sp, cylinders=([[0, 0, 0, 0, 0, 1, 2.0]], 1.0, 1.0), cylinder_damping=2.0, walls=(np.eye(3, 4), 1.0, 1.0),
                                    shell_ledger=True)
    names = [c[0] for c in sp.calls]
    assert names[0] == "set_shell_ledger" and sp.calls[0][1] == (True,) and names.index("cylinder_damping") > names.index("set_cylinders")
    sp = _Recorder()
    step_pass.apply_contact_options(sp, cylinder_damping=2.0)
    assert [c[0] for c in sp.calls] == ["cylinder_damping"]


def test_the_python_step_folds_once_behind_the_force_pass():
    """DeviceRun.step: first half kick, force pass, ONE fold (which takes the pair, wall and shell rows alike), second half
    kick, as step_after_reverse; no fold while the energy ledger is off, whatever the shell switch says."""
    for ledger in (True, False):
        sp = _Recorder(ledger_on=ledger, shell_ledger_on=True)
        r = run.DeviceRun.__new__(run.DeviceRun)
        r.sp, r.dt, r.check, r.steps, r.n = sp, 1e-3, False, 0, 4
        r._nve = lambda stage: sp.calls.append(("nve", (stage,), {}))
        r.force = lambda eflag=False, advance=False: sp.calls.append(("force", (advance,), {}))
        r.step()
        assert [c[0] for c in sp.calls] == (["nve", "force", "ledger_fold_device", "nve"] if ledger else ["nve", "force", "nve"])
        if ledger:
            assert sp.calls[2][1] == (1e-3,)


def test_the_shadow_of_a_fresh_context_has_the_switch_off():
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    assert sp.shell_ledger_on is False and sp.ledger_on is False
    assert capi.ShPair.SHELL_TERMS == ("damping", "friction", "work")
