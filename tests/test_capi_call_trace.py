"""The call trace of the binding's three surface families (planar walls, cylinders, cones): what shpair/capi.py hands the
library, call by call, and what its predicates answer afterwards.  CPU: no GPU and no library: the library is a recorder.

Nothing is computed here, so the comparison is exact: tests/golden/capi_call_trace.json is the text this module prints
when it is run as a script,

    python tests/test_capi_call_trace.py > tests/golden/capi_call_trace.json

and it was made that way from the binding as it stood while every family had a hand-written copy of every method.  A change
that folds, renames or reorders the code behind the named methods must reproduce it byte for byte.

1. Per family: the geometry, every coefficient setter with scalars and with arrays, friction / spring and rolling /
   twisting in both orders, the geometry again (it resets), the two passes with positional and with keyword arguments,
   stats, read-back, the three history calls and a wrong-shape history, the geometry with None.
2. apply_contact_options with every option given, and force_pass over the real shadow for every combination of (absent,
   elastic, damped, with history) of the three families."""
import inspect
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(ROOT, "lammps-spherharm_amd"), ROOT]

from shpair import capi  # noqa: E402
from shpair.step_pass import StepView, apply_contact_options, force_pass  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_call_trace.json")
NLOCAL = 3


# ---- the recorder: the C contract's array lengths, written out from include/shstep.h -------------------------------------

def per(*widths):
    """One double* per width: count x width doubles, count being the call's first int argument."""
    return lambda n, count: [n * w for w in widths]


def history(geometry, xi):
    """[nlocal][surfaces of the family][xi]: nlocal is the call's first int argument."""
    return lambda n, count: [n * count[geometry] * xi]


DOUBLES = {
    "shstep_set_walls": per(4, 1, 1), "shstep_set_cylinders": per(7, 1, 1), "shstep_set_cones": per(8, 1, 1),
    "shstep_get_walls": per(4), "shstep_get_cylinders": per(7), "shstep_get_cones": per(8),
    "shstep_set_wall_damping": per(1), "shstep_set_cylinder_damping": per(1), "shstep_set_cone_damping": per(1),
    "shstep_set_wall_friction": per(1, 1), "shstep_set_cylinder_friction": per(1, 1), "shstep_set_cone_friction": per(1, 1),
    "shstep_set_cylinder_rotation": per(1), "shstep_set_cone_rotation": per(1),
    "shstep_set_wall_tangential_spring": per(1), "shstep_set_cyl_tangential_spring": per(1),
    "shstep_set_conic_tangential_spring": per(1),
    "shstep_set_wall_rolling": per(1, 1), "shstep_set_rolling_cyl": per(1, 1), "shstep_set_rolling_con": per(1, 1),
    "shstep_set_wall_twisting": per(1, 1), "shstep_set_twisting_cyl": per(1, 1), "shstep_set_twisting_con": per(1, 1),
    "shstep_set_wall_velocity": per(3),
    "shstep_copy_wall_history": history("shstep_set_walls", 3), "shstep_set_wall_history": history("shstep_set_walls", 3),
    "shstep_copy_cyl_history": history("shstep_set_cylinders", 2), "shstep_set_cyl_history": history("shstep_set_cylinders", 2),
    "shstep_copy_conic_history": history("shstep_set_cones", 3), "shstep_set_conic_history": history("shstep_set_cones", 3),
    "shstep_post_force_device": lambda n, count: [3],   # the gravity vector
}
GEOMETRY = ("shstep_set_walls", "shstep_set_cylinders", "shstep_set_cones")


def enc(a):
    """A scalar argument as the trace keeps it; bools as words, for JSON would let True pass for 1."""
    if isinstance(a, (bool, np.bool_)):
        return str(bool(a))
    if a is None or isinstance(a, (int, float, str)):
        return a
    return type(a).__name__       # byref(...) of an output scalar: CArgObject


class Library:
    """Stands in for libshpair.so: every symbol of capi.SYMBOLS is a callable that logs its arguments, the doubles behind
    every double* among them, and returns 0."""

    def __init__(self):
        self.log, self.count = [], {}

    def __getattr__(self, symbol):
        if symbol not in capi.SYMBOLS:
            raise AttributeError(symbol)

        def call(*args):
            assert len(args) == len(capi.SYMBOLS[symbol][1]), symbol
            n = next((a for a in args[1:] if isinstance(a, int)), None)
            pointers = [a for a in args if isinstance(a, capi._dp)]
            lengths = iter(DOUBLES[symbol](n, self.count)) if pointers else iter(())
            self.log.append([symbol] + [[a[i] for i in range(next(lengths))] if isinstance(a, capi._dp) else enc(a)
                                        for a in args])
            if symbol in GEOMETRY:
                self.count[symbol] = n
            return 0
        return call


# ---- the script ---------------------------------------------------------------------------------------------------------

STATE = ("keeps_integrals", "has_pair_pass", "has_rolling", "has_history", "pair_dissipation", "damp_pairs", "fric_pairs",
         "nwalls", "wall_reads_twists", "has_wall_rolling", "has_wall_history", "walls_advance", "damp_walls", "fric_walls",
         "move_walls", "ncylinders", "cylinder_reads_twists", "has_cyl_rolling", "has_cyl_history", "ncones",
         "cone_reads_twists", "has_conic_rolling", "has_conic_history", "has_dissipation", "shell_ledger_on")

WALLS = [[0.0, 0.0, 1.0, -0.5], [1.0, 0.0, 0.0, -2.0], [0.0, -1.0, 0.0, -3.25]]
CYLINDERS = [[0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 4.0], [1.0, 2.0, 3.0, 1.0, 0.0, 0.0, 2.5], [0.5, 0.0, -1.0, 0.0, 1.0, 0.0, 8.0]]
CONES = [[0.0, 0.0, -1.0, 0.0, 0.0, 1.0, 0.8, 0.6], [1.0, 2.0, 3.0, 1.0, 0.0, 0.0, 0.6, 0.8],
         [0.5, 0.0, -1.0, 0.0, 1.0, 0.0, 0.28, 0.96]]
# family -> (rows, xi width, set, damping, friction, rotation, spring, rolling, twisting, force pass, contact pass, the
# name of its output argument, history get / set / reset, stats, get)
FAMILIES = {
    "wall": (WALLS, 3, "set_walls", "wall_damping", "wall_friction", None, "set_wall_tangential_spring", "wall_rolling",
             "wall_twisting", "wall_force_damped_device", "wall_contact_device", "wall_out", "wall_history", "set_wall_history",
             "reset_wall_history", "wall_stats", "get_walls"),
    "cylinder": (CYLINDERS, 2, "set_cylinders", "cylinder_damping", "cylinder_friction", "cylinder_rotation",
                 "set_cyl_tangential_spring", "cylinder_rolling", "cylinder_twisting", "cylinder_force_device",
                 "cyl_contact_device", "cyl_out", "cyl_history", "set_cyl_history", "reset_cyl_history", "cylinder_stats",
                 "get_cylinders"),
    "cone": (CONES, 3, "set_cones", "cone_damping", "cone_friction", "cone_rotation", "conic_spring", "conic_rolling",
             "conic_twisting", "cone_force_device", "conic_contact_device", "cone_out", "conic_history", "set_conic_history",
             "reset_conic_history", "cone_stats", "get_cones"),
}
X, QUAT, V, L, TY, SH, MASK, FO, TQ, TW, OUT, STREAM = 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111, 77


def fresh():
    """An ShPair without a context: its shadow over the recorder."""
    sp = capi.ShPair.__new__(capi.ShPair)
    sp._reset_shadow()
    sp._h, sp._lib = "handle", Library()
    return sp


class Trace:
    def __init__(self, sp):
        self.sp, self.steps = sp, []

    def step(self, label, fn, *args, **kw):
        """One call of the binding: the library calls it made, what it returned (an array by its shape) or that it raised
        ValueError, and every predicate and count afterwards."""
        self.sp._lib.log.clear()
        entry = {"step": label}
        try:
            out = fn(*args, **kw)
            entry["returns"] = list(out.shape) if isinstance(out, np.ndarray) else enc(out)
        except ValueError:
            entry["raises"] = "ValueError"
        entry["calls"] = list(self.sp._lib.log)
        entry["state"] = [enc(getattr(self.sp, name)) for name in STATE] + [enc(self.sp.ledger_on)]
        self.steps.append(entry)


def drive_family(t, family):
    (rows, xi, set_, damping, friction, rotation, spring, rolling, twisting, force, contact, out_name, hist_get, hist_set,
     hist_reset, stats, get) = FAMILIES[family]

    def step(label, name, *args, **kw):
        t.step(f"{family}: {label}", getattr(t.sp, name), *args, **kw)
    step("geometry, scalar kn and exponent", set_, rows, 1000.0, 1.25)
    step("geometry, kn and exponent per surface", set_, np.array(rows), [1000.0, 2000.0, 500.0], [1.25, 1.5, 1.0])
    step("damping, scalar", damping, 2.0)
    step("damping, per surface", damping, [0.0, 1.5, 0.0])
    step("damping off", damping, 0.0)
    step("friction, scalars", friction, 0.5, 9.0)
    step("friction, per surface", friction, [0.5, 0.0, 0.25], [0.0, 3.0, 9.0])
    step("friction, array and scalar", friction, [0.5, 0.0, 0.25], 9.0)
    step("friction, scalar and array", friction, 0.5, [0.0, 0.0, 0.0])
    if rotation:
        step("rotation, scalar", rotation, 0.75)
        step("rotation, per surface", rotation, [0.75, -1.5, 0.0])
    step("spring behind friction, scalar", spring, 4000.0)
    step("spring, per surface", spring, [0.0, 4000.0, 0.0])
    step("spring off", spring, np.zeros(3))
    step("geometry again: resets", set_, rows, 1000.0, 1.25)
    step("spring ahead of friction", spring, [4000.0, 0.0, 0.0])
    step("friction behind spring, no common surface", friction, [0.0, 0.5, 0.0], [0.0, 3.0, 0.0])
    step("friction behind spring, a common surface", friction, [0.5, 0.5, 0.0], [0.0, 3.0, 0.0])
    step("rolling, scalars", rolling, 0.05, 2.0)
    step("twisting, scalars", twisting, 0.03, 1.0)
    step("rolling off, per surface", rolling, np.zeros(3), np.zeros(3))
    step("twisting off, per surface", twisting, [0.0, 0.0, 0.03], [0.0, 0.0, 0.0])
    step("geometry again: resets", set_, rows, 1000.0, 1.25)
    step("twisting ahead of rolling", twisting, [0.0, 0.0, 0.03], [0.0, 0.0, 2.0])
    step("rolling behind twisting", rolling, [0.05, 0.0, 0.0], [0.0, 3.0, 0.0])
    step("rolling, array and scalar", rolling, [0.05, 0.0, 0.0], 3.0)
    step("twisting, scalar and array", twisting, 0.03, [0.0, 0.0, 0.0])
    step("geometry again: resets", set_, rows, [1000.0, 2000.0, 500.0], 1.5)
    step("force pass, positional", force, NLOCAL, X, QUAT, SH, MASK, FO, TQ, TW, 2, OUT, STREAM)
    step("force pass, positional, defaults", force, NLOCAL, X, QUAT, SH, MASK, FO, TQ, *([None] if family == "wall" else []))
    step("force pass, keywords", force, nlocal=NLOCAL, x=X, quat=QUAT, shtype=SH, mask=MASK, f=FO, torque=TQ, twist=TW,
         groupbit=2, stream=STREAM, **{out_name: OUT})
    step("contact pass, positional", contact, NLOCAL, X, QUAT, SH, MASK, FO, TQ, TW, 1e-3, 2, OUT, STREAM)
    step("contact pass, positional, defaults", contact, NLOCAL, X, QUAT, SH, MASK, FO, TQ, TW, 0.0)
    step("contact pass, keywords", contact, nlocal=NLOCAL, x=X, quat=QUAT, shtype=SH, mask=MASK, f=FO, torque=TQ, twist=TW,
         dt=1e-3, groupbit=2, stream=STREAM, **{out_name: OUT})
    step("stats", stats)
    step("get", get)
    step("history get", hist_get, NLOCAL)
    step("history set", hist_set, NLOCAL, np.arange(NLOCAL * 3 * xi, dtype=np.float64).reshape(NLOCAL, 3, xi) / 8.0)
    step("history set, wrong shape", hist_set, NLOCAL, np.zeros((NLOCAL, 2, xi)))
    step("history set, flat", hist_set, NLOCAL, np.zeros(NLOCAL * 3 * xi))
    step("history reset", hist_reset)
    step("damping ahead of the removal", damping, 2.0)
    step("geometry None: removes", set_, None)
    step("geometry", set_, rows[:2], 1000.0, 1.25)
    step("geometry empty: removes", set_, [])
    step("geometry keywords", set_, **{{"wall": "planes", "cylinder": "cylinders", "cone": "cones"}[family]: rows[:1]},
         kn=[1000.0], exponent=[1.25])


ALL_OPTIONS = dict(
    walls=(WALLS, 1000.0, 1.25), pair_damping={(1, 2): 7.0, ("*", 1): 3.0}, wall_damping=[0.0, 4.0, 0.0],
    pair_friction={(1, "*"): (0.5, 20.0)}, wall_friction=(0.3, [9.0, 0.0, 9.0]), wall_velocity=[0.0, 0.0, 0.25],
    pair_spring={(2, 2): 5000.0}, wall_spring=4000.0, pair_rolling={(1, 1): (0.05, 2.0)}, pair_twisting={(1, 2): (0.02, 3.0)},
    wall_rolling=(0.05, 2.0), wall_twisting=([0.0, 0.03, 0.0], 1.0), cylinders=(CYLINDERS, [1000.0, 2000.0, 500.0], 1.5),
    cylinder_damping=2.0, cylinder_friction=([0.5, 0.0, 0.25], 9.0), cylinder_rotation=[0.75, -1.5, 0.0],
    cylinder_spring=[0.0, 4000.0, 4000.0], shell_ledger=True, cylinder_rolling=(0.05, 2.0),
    cylinder_twisting=(0.03, [0.0, 1.0, 0.0]), cones=(CONES, 1000.0, [1.25, 1.5, 1.0]), cone_damping=[0.0, 1.5, 0.0],
    cone_friction=(0.5, 9.0), cone_rotation=0.75, conic_spring=4000.0, conic_rolling=([0.05, 0.0, 0.0], [0.0, 3.0, 0.0]),
    conic_twisting=(0.03, 1.0))
MODES = ("absent", "elastic", "damped", "history")


def view(nlocal=NLOCAL):
    return StepView(nlocal, 2, X, QUAT, V, L, TY, SH, MASK, FO, TQ, TW, 2, 1e-3, np.array([0.0, 0.0, -9.81]), 0.0, 0.0, STREAM)


def drive_force_pass(t, modes, advance=True, nlocal=NLOCAL, pairs=False):
    """force_pass over a fresh shadow in which each family is absent, elastic, damped or has history."""
    sp = t.sp = fresh()
    sp.set_ntypes(2, 1)
    for family, mode in zip(FAMILIES, modes):
        rows, _, set_, damping, friction, _, spring = FAMILIES[family][:7]
        if mode != "absent":
            getattr(sp, set_)(rows, 1000.0, 1.25)
        if mode == "damped":
            getattr(sp, damping)(2.0)
        if mode == "history":
            getattr(sp, friction)(0.5, 0.0)
            getattr(sp, spring)(4000.0)
    if pairs:
        sp.pair_friction(1, 2, 0.5, 20.0)
        sp.set_pair_tangential_spring(1, 2, 5000.0)
        sp.pair_rolling(1, 1, 0.05, 2.0)
        sp.wall_velocity([0.0, 0.0, 0.25])
    log = sp._lib.log
    t.step(f"force_pass: {' '.join(modes)} advance={advance} nlocal={nlocal} pairs={pairs}", force_pass, sp, view(nlocal),
           lambda twist: log.append(["forward", twist]), lambda: log.append(["reverse"]), 2, advance=advance)
    sp._h = None


def make_trace():
    t = Trace(fresh())
    t.step("fresh", lambda: None)
    for family in FAMILIES:
        drive_family(t, family)
    t.sp._h = None
    t.sp = fresh()
    t.step("set_ntypes", t.sp.set_ntypes, 2, 1)
    assert sorted(ALL_OPTIONS) == sorted(list(inspect.signature(apply_contact_options).parameters)[1:])   # sp, then these
    t.step("apply_contact_options: every option",apply_contact_options, t.sp, **ALL_OPTIONS)
    t.step("apply_contact_options: none", apply_contact_options, t.sp)
    t.sp._h = None
    for w in MODES:
        for c in MODES:
            for k in MODES:
                drive_force_pass(t, (w, c, k))
    drive_force_pass(t, ("history", "history", "history"), advance=False)
    drive_force_pass(t, ("damped", "history", "elastic"), nlocal=0)
    drive_force_pass(t, ("elastic", "damped", "history"), pairs=True)
    return t.steps


def dumps(steps):
    return "[\n" + ",\n".join(json.dumps(s) for s in steps) + "\n]\n"


def test_the_state_list_names_every_public_property_of_the_binding():
    props = {n for n, p in vars(capi.ShPair).items() if isinstance(p, property) and not n.startswith("_")}
    assert props == set(STATE)


def test_the_binding_makes_the_recorded_calls_and_keeps_the_recorded_state():
    got = make_trace()
    with open(GOLDEN) as fh:
        text = fh.read()
    if dumps(got) != text:      # name the first step that differs before the whole text is compared
        for a, b in zip(got, json.loads(text)):
            assert json.dumps(a) == json.dumps(b), a["step"]
    assert dumps(got) == text


if __name__ == "__main__":
    sys.stdout.write(dumps(make_trace()))
