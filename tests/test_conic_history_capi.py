"""CPU-only checks of the cone-spring entry points of include/shstep.h (docs/SPEC.md §2.23): the cross-compiled library
exports them, the ctypes binding lists them with the header's arity, no shstep_*cone* name was added (the C names say
conic), the methods and options exist, the gfx950 code object holds the two new kernels once each without vector spills
or scratch, under a parameter struct of their own and under names no older test matches, the two instances of §2.22 are
still exactly two, a null context is refused, the binding's flag shadow follows the library's rules in both setter orders,
and the shared force pass takes the call with a time step only while a cone has history."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np

from shpair import capi, run, step_pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {"shstep_set_conic_tangential_spring": 3, "shstep_conic_contact_device": 13, "shstep_copy_conic_history": 3,
         "shstep_set_conic_history": 3, "shstep_reset_conic_history": 1}
# the cone entry points of §2.22, which tests/test_cone_capi.py pins: the set stays what it was
CONE = {"shstep_set_cones", "shstep_set_cone_damping", "shstep_set_cone_friction", "shstep_set_cone_rotation",
        "shstep_cone_force_device", "shstep_get_cone_stats", "shstep_get_cones"}
KERNELS = ("conic_spring_kernel", "conic_live_sweep_kernel")
# the names the older tests search the code object for, several of them by substring
OLDER = ("cone_contact", "cyl_", "pair_contact", "wall_", "rolling_", "history_", "twist_kernel", "pair_damp_kernel", "ledger_")


def test_library_exports_the_symbols_and_the_binding_lists_them():
    lib = ctypes.CDLL(capi.library_path())
    txt = open(os.path.join(ROOT, "include", "shstep.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(shstep_[a-z0-9_]*conic[a-z0-9_]*)\s*\(", txt))
    assert declared == set(ENTRY)   # the binding below covers every entry point of §2.23
    assert set(re.findall(r"\b(shstep_[a-z0-9_]*cone[a-z0-9_]*)\s*\(", txt)) == CONE   # no shstep_*cone* name was added
    for name, nargs in ENTRY.items():
        assert hasattr(lib, name), f"libshpair.so does not export {name}"
        assert name in capi.SYMBOLS
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", txt)
        assert len(m.group(1).split(",")) == len(capi.SYMBOLS[name][1]) == nargs, name
    assert capi.SYMBOLS["shstep_conic_contact_device"] == capi.SYMBOLS["shstep_cyl_contact_device"]   # dt placed as there
    assert capi.SYMBOLS["shstep_conic_contact_device"][1][-2] is ctypes.c_double
    for method in ("conic_spring", "conic_contact_device", "conic_history", "set_conic_history", "reset_conic_history"):
        assert callable(getattr(capi.ShPair, method)), method
    assert isinstance(capi.ShPair.has_conic_history, property)
    assert inspect.signature(step_pass.apply_contact_options).parameters["conic_spring"].default is None
    assert callable(run.DeviceRun.cone_history)


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
    assert "ConicSpringParams" in [s for s in ks if "conic_spring_kernel" in s][0]   # a parameter struct of its own
    assert sorted(s for s in ks if "cone_contact" in s) == ["_ZN3shp19cone_contact_kernelENS_10ConeParamsE",
                                                            "_ZN3shp31cone_contact_dissipative_kernelENS_10ConeParamsE"]


def test_a_null_context_is_refused_not_dereferenced():
    lib = capi.load_library()
    t = (ctypes.c_double * 4)()
    assert lib.shstep_set_conic_tangential_spring(None, 1, t) == -1
    assert lib.shstep_conic_contact_device(None, 0, None, None, None, None, 1, None, None, None, None, 0.0, None) == -1
    assert lib.shstep_copy_conic_history(None, 1, t) == -1
    assert lib.shstep_set_conic_history(None, 1, t) == -1
    assert lib.shstep_reset_conic_history(None) == -1


def _shadow():
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._h = None
    return sp


def test_the_flag_shadow_follows_the_setters_in_either_order_and_set_cones_resets_it():
    sp = _shadow()
    assert not sp.has_conic_history
    sp._flags.set_cones(2)
    sp._flags.conic_spring([4e3, 0.0])                   # a k_t without a mu is no history
    assert not sp.has_conic_history and not sp.cone_reads_twists and not sp.has_dissipation
    sp._flags.cone_friction([0.0, 0.5], [0.0, 3.0])      # ... nor is a mu on the other cone
    assert not sp.has_conic_history and sp.cone_reads_twists
    sp._flags.cone_friction([0.5, 0.0], [0.0, 0.0])      # mu and k_t on the same cone; gamma_t may be 0
    assert sp.has_conic_history and sp.cone_reads_twists and sp.has_dissipation
    assert not sp.has_cyl_history and not sp.has_wall_history
    sp._flags.conic_spring(np.zeros(2))                  # every k_t 0 drops it
    assert not sp.has_conic_history and not sp.has_dissipation
    sp._flags.conic_spring([4e3, 4e3])                   # the spring behind the friction
    assert sp.has_conic_history
    sp._flags.cone_friction(np.zeros(2), [1.0, 1.0])     # the mu of the last history cone to 0 drops it
    assert not sp.has_conic_history
    sp._flags.cone_friction([0.5, 0.5], [1.0, 1.0])
    assert sp.has_conic_history
    sp._flags.set_cylinders(2)                           # the cylinders and the cones are independent
    assert sp.has_conic_history and not sp.has_cyl_history
    sp._flags.set_cones(2)                               # shstep_set_cones resets every k_t,k
    assert not sp.has_conic_history and not sp.cone_reads_twists


class _Recorder:
    """A context stand-in that records the calls of step_pass.force_pass; every unknown name is a callable, as in the
    stand-ins of the older tests."""

    def __init__(self, ncones, hist):
        self.calls, self.ncones, self.cone_reads_twists, self.ncylinders, self.nwalls = [], ncones, bool(hist), 0, 1
        self.keeps_integrals = self.has_pair_pass = self.has_rolling = self.has_history = self.has_wall_history = False
        self.has_dissipation, self.wall_reads_twists, self.walls_advance = bool(hist), False, False
        if hist is not None:
            self.has_conic_history = hist

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call


def test_the_shared_force_pass_hands_the_cone_pass_its_dt_only_while_a_cone_has_history():
    def order(ncones, hist, advance, nlocal=5):
        sp = _Recorder(ncones, hist)
        v = step_pass.StepView(nlocal, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 77, 1, 1e-3, (0.0, 0.0, -9.81), 0.0, 0.0, None)
        step_pass.force_pass(sp, v, lambda tw: None, lambda: None, 0, advance=advance)
        return sp.calls
    calls = order(2, True, True)
    names = [c[0] for c in calls]
    assert names[0] == "twist_device" and names[-3:] == ["wall_force_damped_device", "conic_contact_device", "post_force_device"]
    assert "cone_force_device" not in names
    c = calls[-2]
    assert c[1] == (5, 1, 2, 6, 7, 8, 9, 77, 1e-3) and c[2]["groupbit"] == 1          # the step's twists and its dt
    assert order(2, True, False)[-2][1][-1] == 0.0                                        # the set-up pass: a look
    for hist in (False, None):   # no spring; and a stand-in without the predicate, which answers with a callable
        names = [c[0] for c in order(2, hist, True)]
        assert names[-3:] == ["wall_force_damped_device", "cone_force_device", "post_force_device"]
        assert "conic_contact_device" not in names
    assert "conic_contact_device" not in [c[0] for c in order(0, True, True)]            # no cone: no call
    assert "conic_contact_device" not in [c[0] for c in order(2, True, True, nlocal=0)]
