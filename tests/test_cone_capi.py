"""CPU-only checks of the cone entry points of include/shstep.h (docs/SPEC.md §2.22): the cross-compiled library exports
them, the ctypes binding lists them with the header's arity, the methods and options exist, the gfx950 code object holds
each of the five new kernels once without vector spills or scratch and under names no older test matches, a null
context is refused, the binding's flag shadow follows the library's rules (set_cones resets every coefficient), and the
two Python step drivers place the pass behind the cylinders."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np

from shpair import capi, step_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"shstep_set_cones": 5, "shstep_set_cone_damping": 3, "shstep_set_cone_friction": 4, "shstep_set_cone_rotation": 3,
         "shstep_cone_force_device": 12, "shstep_get_cone_stats": 2, "shstep_get_cones": 3}
KERNELS = ("cone_candidates_kernel", "cone_contact_kernel", "cone_contact_dissipative_kernel", "cone_rows_partial_kernel",
           "cone_rows_final_kernel")
# the names the older tests search the code object for, several of them by substring
OLDER = ("pair_contact", "wall_", "rolling_", "history_", "twist_kernel", "pair_damp_kernel", "ledger_", "cyl_")


def test_library_exports_the_cone_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(shstep_[a-z0-9_]*cone[a-z0-9_]*)\s*\(", txt))
    assert declared == set(ENTRY)   # the binding below covers every cone entry point of the header
    for name, nargs in ENTRY.items():
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]) == nargs, name
    assert capi.SYMBOLS["shstep_cone_force_device"] == capi.SYMBOLS["shstep_cylinder_force_device"]   # the same argument list
    assert re.search(r"#define\s+SHSTEP_MAX_CONES\s+8\b", txt)
    for method in ("set_cones", "cone_damping", "cone_friction", "cone_rotation", "get_cones", "cone_force_device", "cone_stats"):
        assert callable(getattr(capi.ShPair, method)), method
    assert isinstance(capi.ShPair.cone_reads_twists, property) and isinstance(capi.ShPair.ncones, property)
    par = inspect.signature(step_pass.apply_contact_options).parameters
    for opt in ("cones", "cone_damping", "cone_friction", "cone_rotation"):
        assert par[opt].default is None
    rec = capi.cone_record([1.0, 2.0, 3.0], [0.0, 0.0, 1.0], np.pi / 6)
    assert rec.shape == (8,) and abs(rec[6] ** 2 + rec[7] ** 2 - 1) <= 4 * np.finfo(float).eps and rec[6] > rec[7] > 0


def test_cone_kernels_are_in_the_code_object_once_without_spills():
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
    assert len([s for s in ks if "cone_contact" in s]) == 2   # two instances only


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 8)()
    n = ctypes.c_int(7)
    assert lib.shstep_set_cones(None, 1, t, t, t) == -1
    assert lib.shstep_set_cone_damping(None, 1, t) == -1
    assert lib.shstep_set_cone_friction(None, 1, t, t) == -1
    assert lib.shstep_set_cone_rotation(None, 1, t) == -1
    assert lib.shstep_get_cones(None, 1, t) == -1
    assert lib.shstep_get_cone_stats(None, ctypes.byref(n)) == -1
    assert lib.shstep_cone_force_device(None, 0, None, None, None, None, 1, None, None, None, None, None) == -1


def _shadow():
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._h = None
    return sp


def test_the_flag_shadow_follows_the_setters_and_set_cones_resets_them():
    """The predicates the drivers decide by (no library call: a fresh shadow and the flag methods the setters call)."""
    sp = _shadow()
    assert sp.ncones == 0 and not sp.cone_reads_twists and not sp.has_dissipation
    sp._flags.set_cones(2)
    assert sp.ncones == 2 and not sp.cone_reads_twists and not sp.has_dissipation   # elastic: no twists
    sp._flags.cone_friction([0.5, 0.0], [0.0, 3.0])      # a mu without a gamma_t on the same cone is no friction
    assert not sp.cone_reads_twists
    sp._flags.cone_friction([0.5, 0.0], [2.0, 3.0])
    assert sp.cone_reads_twists and sp.has_dissipation and not sp.cylinder_reads_twists and not sp.wall_reads_twists
    sp._flags.cone_friction(np.zeros(2), np.zeros(2))
    sp._flags.cone_damping([0.0, 1.5])
    assert sp.cone_reads_twists and sp.has_dissipation
    sp._flags.set_cones(2)                               # shstep_set_cones resets them
    assert not sp.cone_reads_twists and not sp.has_dissipation
    sp._flags.cone_damping([1.0, 0.0])
    sp._flags.set_cylinders(3)                           # the cylinders and the cones are independent
    sp._flags.set_walls(np.eye(3))
    assert sp.cone_reads_twists and sp.ncylinders == 3 and sp.nwalls == 3 and sp.ncones == 2


class _Recorder:
    """A context stand-in that records the calls of step_pass.force_pass."""

    def __init__(self, ncones, diss, ncyl):
        self.calls, self.ncones, self.cone_reads_twists, self.ncylinders, self.nwalls = [], ncones, diss, ncyl, 1
        self.keeps_integrals = self.has_pair_pass = self.has_rolling = self.has_history = self.has_wall_history = False
        self.has_cyl_history = self.cylinder_reads_twists = False
        self.has_dissipation, self.wall_reads_twists, self.walls_advance = diss, False, False

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call


def test_the_shared_force_pass_runs_the_cones_directly_behind_the_cylinders():
    def order(ncones, diss, ncyl=1, nlocal=5):
        sp = _Recorder(ncones, diss, ncyl)
        v = step_pass.StepView(nlocal, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 77, 1, 1e-3, (0.0, 0.0, -9.81), 0.0, 0.0, None)
        step_pass.force_pass(sp, v, lambda tw: None, lambda: None, 0, advance=True)
        return sp.calls
    names = [c[0] for c in order(2, False)]
    assert names[-4:] == ["wall_force_damped_device", "cylinder_force_device", "cone_force_device", "post_force_device"]
    assert "twist_device" not in names
    c = [c for c in order(2, False) if c[0] == "cone_force_device"][0]
    assert c[1][-1] is None and c[1][:7] == (5, 1, 2, 6, 7, 8, 9)              # elastic: no twist pointer
    names = [c[0] for c in order(2, True)]
    assert names[0] == "twist_device"
    c = [c for c in order(2, True, ncyl=0) if c[0] == "cone_force_device"][0]
    assert c[1][-1] == 77                                                      # a coefficient: the step's twists
    assert "cone_force_device" not in [c[0] for c in order(0, False)]          # no cone: no call
    assert "cone_force_device" not in [c[0] for c in order(2, False, nlocal=0)]
