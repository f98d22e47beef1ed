"""CPU-only checks of the cylinder-spring entry points of include/shstep.h (docs/SPEC.md §2.19): the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the methods and options exist, the gfx950 code
object holds the two new kernels once each without vector spills or scratch and under names no older test matches, the
two instances of §2.18 are still exactly two, a null context is refused, the binding's flag shadow follows the
library's rules, the shared force pass takes the call with a time step only while a spring is set, and the setter's
argument check (csrc/surface_coefficients.hpp) runs clean under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np

from shpair import capi, run, step_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
ENTRY = {"shstep_set_cyl_tangential_spring": 3, "shstep_cyl_contact_device": 13, "shstep_copy_cyl_history": 3,
         "shstep_set_cyl_history": 3, "shstep_reset_cyl_history": 1}
KERNELS = ("cyl_spring_kernel", "cyl_live_sweep_kernel")
# the names the older tests search the code object for, several of them by substring
OLDER = ("cyl_contact", "pair_contact", "wall_", "rolling_", "history_", "twist_kernel", "pair_damp_kernel", "ledger_")


def test_library_exports_the_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(shstep_[a-z0-9_]*cyl_[a-z0-9_]*)\s*\(", txt))
    assert declared == set(ENTRY)   # the binding below covers every entry point of §2.19
    for name, nargs in ENTRY.items():
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]) == nargs, name
    assert capi.SYMBOLS["shstep_cyl_contact_device"][1][-2] is ctypes.c_double   # dt
    for method in ("set_cyl_tangential_spring", "cyl_contact_device", "cyl_history", "set_cyl_history", "reset_cyl_history"):
        assert callable(getattr(capi.ShPair, method)), method
    assert isinstance(capi.ShPair.has_cyl_history, property)
    assert inspect.signature(step_pass.apply_contact_options).parameters["cylinder_spring"].default is None
    assert callable(run.DeviceRun.cylinder_history)


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
    assert "CylSpringParams" in [s for s in ks if "cyl_spring_kernel" in s][0]   # a parameter struct of its own
    assert sorted(s for s in ks if "cyl_contact" in s) == ["_ZN3shp18cyl_contact_kernelENS_9CylParamsE",
                                                           "_ZN3shp30cyl_contact_dissipative_kernelENS_9CylParamsE"]


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 4)()
    assert lib.shstep_set_cyl_tangential_spring(None, 1, t) == -1
    assert lib.shstep_cyl_contact_device(None, 0, None, None, None, None, 1, None, None, None, None, 0.0, None) == -1
    assert lib.shstep_copy_cyl_history(None, 1, t) == -1
    assert lib.shstep_set_cyl_history(None, 1, t) == -1
    assert lib.shstep_reset_cyl_history(None) == -1


def _shadow():
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._h = None
    return sp


def test_the_flag_shadow_follows_the_setters_in_either_order():
    sp = _shadow()
    assert not sp.has_cyl_history
    sp._flags.set_cylinders(2)
    sp._flags.cylinder_spring([4e3, 0.0])                    # a k_t without a mu is no history
    assert not sp.has_cyl_history and not sp.cylinder_reads_twists and not sp.has_dissipation
    sp._flags.cylinder_friction([0.0, 0.5], [0.0, 3.0])      # ... nor is a mu on the other cylinder
    assert not sp.has_cyl_history and sp.cylinder_reads_twists
    sp._flags.cylinder_friction([0.5, 0.0], [0.0, 0.0])      # mu and k_t on the same cylinder; gamma_t may be 0
    assert sp.has_cyl_history and sp.cylinder_reads_twists and sp.has_dissipation and not sp.has_wall_history
    sp._flags.cylinder_spring(np.zeros(2))                   # every k_t 0 drops it
    assert not sp.has_cyl_history and not sp.has_dissipation
    sp._flags.cylinder_spring([4e3, 4e3])                    # the spring behind the friction
    assert sp.has_cyl_history
    sp._flags.cylinder_friction(np.zeros(2), [1.0, 1.0])     # the mu of the last history cylinder to 0 drops it
    assert not sp.has_cyl_history
    sp._flags.cylinder_friction([0.5, 0.5], [1.0, 1.0])
    assert sp.has_cyl_history
    sp._flags.set_walls(np.eye(3))                           # the planes and the cylinders are independent
    assert sp.has_cyl_history
    sp._flags.set_cylinders(2)                               # shstep_set_cylinders resets every k_t,c
    assert not sp.has_cyl_history and not sp.cylinder_reads_twists


class _Recorder:
    """A context stand-in that records the calls of step_pass.force_pass; every unknown name is a callable, as in the
    stand-ins of the older tests."""

    def __init__(self, ncyl, hist):
        self.calls, self.ncylinders, self.cylinder_reads_twists, self.nwalls = [], ncyl, hist, 1
        self.keeps_integrals = self.has_pair_pass = self.has_rolling = self.has_history = self.has_wall_history = False
        self.has_dissipation, self.wall_reads_twists, self.walls_advance = hist, False, False
        if hist is not None:
            self.has_cyl_history = hist

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call


def test_the_shared_force_pass_hands_the_cylinder_pass_its_dt_only_while_a_spring_is_set():
    def order(ncyl, hist, advance, nlocal=5):
        sp = _Recorder(ncyl, hist)
        v = step_pass.StepView(nlocal, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 77, 1, 1e-3, (0.0, 0.0, -9.81), 0.0, 0.0, None)
        step_pass.force_pass(sp, v, lambda tw: None, lambda: None, 0, advance=advance)
        return sp.calls
    calls = order(2, True, True)
    names = [c[0] for c in calls]
    assert names[0] == "twist_device" and names[-3:] == ["wall_force_damped_device", "cyl_contact_device", "post_force_device"]
    assert "cylinder_force_device" not in names
    c = calls[-2]
    assert c[1] == (5, 1, 2, 6, 7, 8, 9, 77, 1e-3) and c[2]["groupbit"] == 1          # the step's twists and its dt
    assert order(2, True, False)[-2][1][-1] == 0.0                                        # the set-up pass: a look
    for hist in (False, None):   # no spring; and a stand-in without the predicate, which answers with a callable
        names = [c[0] for c in order(2, hist, True)]
        assert names[-3:] == ["wall_force_damped_device", "cylinder_force_device", "post_force_device"]
        assert "cyl_contact_device" not in names
    assert "cyl_contact_device" not in [c[0] for c in order(0, True, True)]              # no cylinder: no call
    assert "cyl_contact_device" not in [c[0] for c in order(2, True, True, nlocal=0)]


def test_the_argument_check_runs_clean_under_the_sanitizers(tmp_path):
    out = tmp_path / "test_cylinder_spring_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           f"-I{CSRC}", os.path.join(ROOT, "tests", "host", "test_cylinder_spring_check.cpp"), "-o", str(out)])
    res = subprocess.run([str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = dict(ln.split(": ", 1) for ln in res.stdout.strip().split("\n"))
    for ok in ("accepted", "none set"):
        assert lines[ok] == "ok", (ok, lines[ok])
    want = {"count": "3 coefficients for 2 cylinders", "count before any cylinder": "3 coefficients for 0 cylinders",
            "null": "null array pointer", "negative": "tangential spring k_t -0.5 must be finite and >= 0",
            "nan": "must be finite", "inf": "must be finite"}
    for label, part in want.items():
        assert part in lines[label], (label, lines[label])
