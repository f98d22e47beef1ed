"""CPU-only checks of the cylinder entry points of include/shstep.h (docs/SPEC.md §2.18): the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, the methods and options exist, the gfx950 code
object holds each of the five new kernels once without vector spills or scratch and under names no older test matches,
a null context is refused, the binding's flag shadow follows the library's rules, the two Python step drivers place
the pass, and the setters' argument checks (csrc/cylinder_check.hpp, csrc/surface_coefficients.hpp) run clean under
AddressSanitizer + UBSan in a stand-alone program."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np

from shpair import capi, step_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
ENTRY = {"shstep_set_cylinders": 5, "shstep_set_cylinder_damping": 3, "shstep_set_cylinder_friction": 4,
         "shstep_set_cylinder_rotation": 3, "shstep_cylinder_force_device": 12, "shstep_get_cylinder_stats": 2,
         "shstep_get_cylinders": 3}
KERNELS = ("cyl_candidates_kernel", "cyl_contact_kernel", "cyl_contact_dissipative_kernel", "cyl_rows_partial_kernel",
           "cyl_rows_final_kernel")
# the names the older tests search the code object for, several of them by substring
OLDER = ("pair_contact", "wall_", "rolling_", "history_", "twist_kernel", "pair_damp_kernel", "ledger_")


def test_library_exports_the_cylinder_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(shstep_[a-z0-9_]*cylinder[a-z0-9_]*)\s*\(", txt))
    assert declared == set(ENTRY)   # the binding below covers every cylinder entry point of the header
    for name, nargs in ENTRY.items():
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]) == nargs, name
    assert re.search(r"#define\s+SHSTEP_MAX_CYLINDERS\s+8\b", txt)
    for method in ("set_cylinders", "cylinder_damping", "cylinder_friction", "cylinder_rotation", "get_cylinders",
                   "cylinder_force_device", "cylinder_stats"):
        assert callable(getattr(capi.ShPair, method)), method
    assert isinstance(capi.ShPair.cylinder_reads_twists, property) and isinstance(capi.ShPair.ncylinders, property)
    par = inspect.signature(step_pass.apply_contact_options).parameters
    for opt in ("cylinders", "cylinder_damping", "cylinder_friction", "cylinder_rotation"):
        assert par[opt].default is None


def test_cylinder_kernels_are_in_the_code_object_once_without_spills():
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
    assert len([s for s in ks if "cyl_contact" in s]) == 2   # two instances only


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 7)()
    n = ctypes.c_int(7)
    assert lib.shstep_set_cylinders(None, 1, t, t, t) == -1
    assert lib.shstep_set_cylinder_damping(None, 1, t) == -1
    assert lib.shstep_set_cylinder_friction(None, 1, t, t) == -1
    assert lib.shstep_set_cylinder_rotation(None, 1, t) == -1
    assert lib.shstep_get_cylinders(None, 1, t) == -1
    assert lib.shstep_get_cylinder_stats(None, ctypes.byref(n)) == -1
    assert lib.shstep_cylinder_force_device(None, 0, None, None, None, None, 1, None, None, None, None, None) == -1


def _shadow():
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._h = None
    return sp


def test_the_flag_shadow_follows_the_setters():
    """The predicates the drivers decide by (no library call: a fresh shadow and the flag methods the setters call)."""
    sp = _shadow()
    assert sp.ncylinders == 0 and not sp.cylinder_reads_twists and not sp.has_dissipation
    sp._flags.set_cylinders(2)
    assert sp.ncylinders == 2 and not sp.cylinder_reads_twists and not sp.has_dissipation   # elastic: no twists
    sp._flags.cylinder_friction([0.5, 0.0], [0.0, 3.0])      # a mu without a gamma_t on the same cylinder is no friction
    assert not sp.cylinder_reads_twists
    sp._flags.cylinder_friction([0.5, 0.0], [2.0, 3.0])
    assert sp.cylinder_reads_twists and sp.has_dissipation and not sp.wall_reads_twists and not sp.keeps_integrals
    sp._flags.cylinder_friction(np.zeros(2), np.zeros(2))
    sp._flags.cylinder_damping([0.0, 1.5])
    assert sp.cylinder_reads_twists and sp.has_dissipation
    sp._flags.set_cylinders(2)                               # shstep_set_cylinders resets them
    assert not sp.cylinder_reads_twists and not sp.has_dissipation
    sp._flags.set_walls(np.eye(3))                           # the planes and the cylinders are independent
    sp._flags.cylinder_damping([1.0, 0.0])
    sp._flags.set_walls(np.eye(3))
    assert sp.cylinder_reads_twists and sp.nwalls == 3


class _Recorder:
    """A context stand-in that records the calls of step_pass.force_pass."""

    def __init__(self, ncyl, diss, nwalls):
        self.calls, self.ncylinders, self.cylinder_reads_twists, self.nwalls = [], ncyl, diss, nwalls
        self.keeps_integrals = self.has_pair_pass = self.has_rolling = self.has_history = self.has_wall_history = False
        self.has_dissipation, self.wall_reads_twists, self.walls_advance = diss, False, False

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call


def test_the_shared_force_pass_runs_the_cylinders_directly_behind_the_planes():
    def order(ncyl, diss, nwalls=1, nlocal=5):
        sp = _Recorder(ncyl, diss, nwalls)
        v = step_pass.StepView(nlocal, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 77, 1, 1e-3, (0.0, 0.0, -9.81), 0.0, 0.0, None)
        step_pass.force_pass(sp, v, lambda tw: None, lambda: None, 0, advance=True)
        return sp.calls
    names = [c[0] for c in order(2, False)]
    assert names[-3:] == ["wall_force_damped_device", "cylinder_force_device", "post_force_device"]
    assert "twist_device" not in names
    c = [c for c in order(2, False) if c[0] == "cylinder_force_device"][0]
    assert c[1][-1] is None and c[1][:7] == (5, 1, 2, 6, 7, 8, 9)              # elastic: no twist pointer
    names = [c[0] for c in order(2, True)]
    assert names[0] == "twist_device"
    c = [c for c in order(2, True, nwalls=0) if c[0] == "cylinder_force_device"][0]
    assert c[1][-1] == 77                                                      # a coefficient: the step's twists
    assert "cylinder_force_device" not in [c[0] for c in order(0, False)]      # no cylinder: no call
    assert "cylinder_force_device" not in [c[0] for c in order(2, False, nlocal=0)]


def test_argument_checks_run_clean_under_the_sanitizers(tmp_path):
    out = tmp_path / "test_cylinder_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           f"-I{CSRC}", os.path.join(ROOT, "tests", "host", "test_cylinder_check.cpp"), "-o", str(out)])
    res = subprocess.run([str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = dict(ln.split(": ", 1) for ln in res.stdout.strip().split("\n"))
    for ok in ("accepted", "coefficients accepted", "none set", "negative rotation"):
        assert lines[ok] == "ok", (ok, lines[ok])
    want = {"nine": "0..8 are accepted", "negative count": "0..8 are accepted", "null": "null array pointer",
            "axis length": "the axis has length", "zero axis": "the axis has length 0", "radius 0": "must be > 0",
            "radius < 0": "must be > 0", "radius nan": "not finite", "point inf": "not finite", "kn < 0": "kn -1 < 0",
            "kn nan": "not finite", "exponent < 1": "exponent 0.5 < 1", "exponent inf": "not finite",
            "count": "3 coefficients for 2 cylinders", "null table": "null array pointer", "negative": "must be finite and >= 0",
            "nan": "must be finite", "inf rotation": "must be finite"}
    for label, part in want.items():
        assert part in lines[label], (label, lines[label])
