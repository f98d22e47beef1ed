"""CPU tests of what the two Python step drivers share (shpair/step_pass.py) and of the step predicates of the binding
(shpair/capi.py): no GPU and no library.

1. The force pass enqueues exactly what the library's loops enqueue, in the order of csrc/shhalo_run.cpp one_step (2b
   twists, 3 forward, 5 compute, 5b pair dissipation, 6 reverse) and csrc/shstep_run.cpp step_after_reverse (advance,
   wall pass, body forces).  The table below was written out from those two files, call by call.
2. The predicates keeps_integrals / wall_reads_twists / walls_advance / has_dissipation and the older names follow the
   setters as the flags of csrc/shpair_tables.cpp and csrc/shstep_walls.hip do."""
import numpy as np
import pytest

from shpair.capi import ShPair
from shpair.step_pass import StepView, apply_contact_options, force_pass

T, F, C, P, R, A, W, B = ("twist_device", "forward", "compute_device", "pair_dissipation_device", "reverse",
                          "advance_walls_device", "wall_force_damped_device", "post_force_device")
# (pair coefficient, wall coefficient, walls advance, body forces) -> the calls of one step's force pass, walls present
SEQUENCES = {
    (0, 0, 0, 0): [F, C, R, W],
    (0, 0, 0, 1): [F, C, R, W, B],
    (0, 0, 1, 0): [F, C, R, A, W],
    (0, 0, 1, 1): [F, C, R, A, W, B],
    (0, 1, 0, 0): [T, F, C, R, W],
    (0, 1, 0, 1): [T, F, C, R, W, B],
    (0, 1, 1, 0): [T, F, C, R, A, W],
    (0, 1, 1, 1): [T, F, C, R, A, W, B],
    (1, 0, 0, 0): [T, F, C, P, R, W],
    (1, 0, 0, 1): [T, F, C, P, R, W, B],
    (1, 0, 1, 0): [T, F, C, P, R, A, W],
    (1, 0, 1, 1): [T, F, C, P, R, A, W, B],
    (1, 1, 0, 0): [T, F, C, P, R, W],
    (1, 1, 0, 1): [T, F, C, P, R, W, B],
    (1, 1, 1, 0): [T, F, C, P, R, A, W],
    (1, 1, 1, 1): [T, F, C, P, R, A, W, B],
}
# device "pointers": any distinct ints
X, QUAT, V, L, TY, SH, MASK, FO, TQ, TW, EV = range(101, 112)


class Recorder:
    """Stands in for the context: the four predicates, nwalls and the six entry points the pass may call, which record
    (name, args, kwargs).  Any other attribute (a stray synchronize, say) is an AttributeError."""

    def __init__(self, pair, wall, adv, nwalls):
        self.keeps_integrals, self.wall_reads_twists, self.walls_advance, self.nwalls = bool(pair), bool(wall), bool(adv), nwalls
        self.has_dissipation = bool(pair or wall)
        self.calls = []

    def _rec(name):
        def call(self, *args, **kw):
            self.calls.append((name, args, kw))
        return call
    twist_device, compute_device, pair_dissipation_device = _rec(T), _rec(C), _rec(P)
    advance_walls_device, wall_force_damped_device, post_force_device = _rec(A), _rec(W), _rec(B)


def run_pass(pair, wall, adv, body, nwalls=3, nlocal=5, nghost=2, twist_ghosts=2, advance=True, eflag=False):
    sp = Recorder(pair, wall, adv, nwalls)
    v = StepView(nlocal, nghost, X, QUAT, V, L, TY, SH, MASK, FO, TQ, TW, 1, 1e-3, np.array([0.0, 0.0, -9.81 if body else 0.0]),
                 0.0, 0.0, 77)
    force_pass(sp, v, lambda twist: sp.calls.append((F, (twist,), {})), lambda: sp.calls.append((R, (), {})), twist_ghosts,
               eflag=eflag, ev=EV, advance=advance)
    return sp.calls


@pytest.mark.parametrize("combo", sorted(SEQUENCES))
def test_force_pass_enqueues_the_librarys_sequence(combo):
    assert [c[0] for c in run_pass(*combo)] == SEQUENCES[combo]


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("body", [0, 1])
def test_force_pass_without_walls(pair, body):
    """nwalls == 0: no wall pass and no advance; a wall coefficient cannot be set (shstep_set_walls resets them)."""
    want = ([T, F, C, P, R] if pair else [F, C, R]) + ([B] if body else [])
    assert [c[0] for c in run_pass(pair, 0, 0, body, nwalls=0)] == want


@pytest.mark.parametrize("nwalls", [0, 3])
@pytest.mark.parametrize("pair", [0, 1])
def test_forward_gets_the_twists_iff_a_pair_coefficient_is_set(nwalls, pair):
    for wall in ((0, 1) if nwalls else (0,)):
        calls = dict((c[0], c) for c in run_pass(pair, wall, 0, 0, nwalls=nwalls))
        assert calls[F][1] == ((TW,) if pair else (None,))
        if nwalls:   # ... and the wall pass iff a wall coefficient is set
            assert calls[W][1][-1] == (TW if wall else None)


@pytest.mark.parametrize("nwalls", [0, 3])
@pytest.mark.parametrize("twist_ghosts", [0, 2])
def test_twist_call_gets_the_drivers_ghost_row_count(nwalls, twist_ghosts):
    """DeviceRun passes its nghost (the twist kernel fills its periodic images), RankRun 0 (the exchange brings them)."""
    calls = run_pass(1, 0, 0, 0, nwalls=nwalls, nghost=2, twist_ghosts=twist_ghosts)
    assert calls[0] == (T, (5, twist_ghosts, V, QUAT, L, SH, TW), {"stream": 77})
    # the compute and the pair pass take the rank's ghost rows whatever the twist kernel fills
    assert calls[2][0] == C and calls[2][1][:2] == (5, 2) and calls[3][0] == P and calls[3][1][:2] == (5, 2)


@pytest.mark.parametrize("nwalls", [0, 3])
def test_force_pass_calls_nothing_but_the_recorded_set(nwalls):
    """Every call of every combination is one the stand-in records, on the view's stream; anything else, a synchronize
    or a zeroing among them, would have raised AttributeError in the stand-in."""
    for combo in SEQUENCES:
        if not nwalls and (combo[1] or combo[2]):
            continue
        for name, args, kw in run_pass(*combo, nwalls=nwalls, eflag=True):
            assert name in (T, F, C, P, R, A, W, B)
            assert name in (F, R) or kw["stream"] == 77
            if name == C:
                assert kw["eflag"] is True and kw["ev"] == EV
    with pytest.raises(AttributeError):
        Recorder(0, 0, 0, 0).synchronize()
    assert all(c[2]["ev"] is None for c in run_pass(0, 0, 0, 0) if c[0] == C)   # no eflag: no ev pointer


def test_advance_only_in_a_step_and_owned_rows_only():
    assert [c[0] for c in run_pass(1, 1, 1, 1, advance=False)] == [T, F, C, P, R, W, B]   # a constructor's or a test's pass
    # a rank that owns nothing still takes part in the exchanges and advances its planes; no wall pass, no body forces
    assert [c[0] for c in run_pass(1, 1, 1, 1, nlocal=0)] == [T, F, C, P, R, A]


# ---- the predicates of the binding -------------------------------------------------------------------------------------

FLOOR_AND_SIDE = [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]
NAMES = ("keeps_integrals", "wall_reads_twists", "walls_advance", "has_dissipation", "pair_dissipation", "damp_pairs",
         "fric_pairs", "damp_walls", "fric_walls", "move_walls", "nwalls")
# (what the setters record, in order) -> the names that are true afterwards, and nwalls
FLAG_CASES = [
    ([], set(), 0),
    ([("set_walls", FLOOR_AND_SIDE)], set(), 2),
    ([("pair_damping", 1, 2, 5.0)], {"keeps_integrals", "has_dissipation", "pair_dissipation", "damp_pairs"}, 0),
    ([("pair_damping", 2, 1, 5.0), ("pair_damping", 1, 2, 0.0)], set(), 0),                        # symmetric: one pair
    ([("pair_friction", 1, 1, 0.5, 20.0)], {"keeps_integrals", "has_dissipation", "pair_dissipation", "fric_pairs"}, 0),
    ([("pair_friction", 1, 1, 0.5, 0.0)], set(), 0),                                               # mu != 0, gamma_t == 0
    ([("pair_friction", 1, 1, 0.0, 20.0)], set(), 0),
    ([("pair_friction", 1, 1, 0.5, 20.0), ("pair_friction", 1, 1, 0.5, 0.0)], set(), 0),
    ([("pair_damping", 1, 1, 5.0), ("pair_friction", 1, 2, 0.5, 20.0), ("set_ntypes",)], set(), 0),  # the type table goes
    ([("set_walls", FLOOR_AND_SIDE), ("wall_damping", [0.0, 3.0])], {"wall_reads_twists", "has_dissipation", "damp_walls"}, 2),
    ([("set_walls", FLOOR_AND_SIDE), ("wall_damping", [0.0, 0.0])], set(), 2),
    ([("set_walls", FLOOR_AND_SIDE), ("wall_friction", [0.3, 0.0], [0.0, 9.0])], set(), 2),        # no wall has both
    ([("set_walls", FLOOR_AND_SIDE), ("wall_friction", [0.3, 0.0], [9.0, 0.0])],
     {"wall_reads_twists", "has_dissipation", "fric_walls"}, 2),
    ([("set_walls", FLOOR_AND_SIDE), ("wall_velocity", [[0.0, 0.0, 0.2], [0.0, 0.0, 0.0]])], {"move_walls", "walls_advance"}, 2),
    ([("set_walls", FLOOR_AND_SIDE), ("wall_velocity", [[1.0, -2.0, 0.0], [0.0, 3.0, 0.5]])], {"move_walls"}, 2),   # belts: u ⟂ n
    ([("set_walls", FLOOR_AND_SIDE), ("wall_velocity", [[0.0, 0.0, 0.2], [0.0, 0.0, 0.0]]),
      ("wall_velocity", [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])], set(), 2),
    # set_walls resets every wall coefficient and velocity, and leaves the pair coefficients
    ([("pair_damping", 1, 1, 5.0), ("set_walls", FLOOR_AND_SIDE), ("wall_damping", [1.0, 1.0]), ("wall_friction", [0.3, 0.3], [9.0, 9.0]),
      ("wall_velocity", [[0.0, 0.0, 0.2], [0.1, 0.0, 0.0]]), ("set_walls", [[0.0, 1.0, 0.0]])],
     {"keeps_integrals", "has_dissipation", "pair_dissipation", "damp_pairs"}, 1),
    ([("set_walls", FLOOR_AND_SIDE), ("wall_damping", [1.0, 1.0]), ("wall_velocity", [[0.0, 0.0, 0.2], [0.1, 0.0, 0.0]]),
      ("set_walls", np.zeros((0, 3)))], set(), 0),
]


@pytest.mark.parametrize("case", range(len(FLAG_CASES)))
def test_predicates_follow_the_setters(case):
    calls, true, nwalls = FLAG_CASES[case]
    sp = ShPair.__new__(ShPair)      # no context, no library: only what the object remembers
    sp._reset_shadow()
    for name, *args in calls:
        getattr(sp._flags, name)(*args)
    got = {n for n in NAMES[:-1] if getattr(sp, n)}
    assert all(isinstance(getattr(sp, n), bool) for n in NAMES[:-1])
    assert got == true and sp.nwalls == nwalls


def test_normal_velocity_is_formed_as_the_library_forms_it():
    """n[0]*u[0] + n[1]*u[1] + n[2]*u[2], summed in that order in doubles: (1 + 2^-53) - 1 is 0 (the first sum rounds to
    1) where the exact sum is not, and (1 - 1) + 2^-54 is not 0 where -1 + 2^-54 first would round to -1 and give 0."""
    sp = ShPair.__new__(ShPair)
    sp._reset_shadow()
    sp._flags.set_walls([[1.0, 1.0, 1.0]] * 2)     # (the library would refuse this normal; the record only multiplies)
    sp._flags.wall_velocity([[1.0, 2.0 ** -53, -1.0], [0.0, 0.0, 0.0]])
    assert sp.move_walls and not sp.walls_advance
    sp._flags.wall_velocity([[0.0, 0.0, 0.0], [1.0, -1.0, 2.0 ** -54]])
    assert sp.move_walls and sp.walls_advance


def test_contact_options_are_applied_in_the_constructors_order():
    class Ctx:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if name not in ("set_walls", "pair_damping", "wall_damping", "pair_friction", "wall_friction", "wall_velocity"):
                raise AttributeError(name)
            return lambda *a: self.calls.append((name,) + a)
    sp = Ctx()
    apply_contact_options(sp)
    assert sp.calls == []
    apply_contact_options(sp, wall_velocity=[0, 0, 1.0], wall_friction=(0.3, 9.0), pair_friction={(1, "*"): (0.5, 20.0)},
                          wall_damping=4.0, pair_damping={(1, 2): 7.0}, walls=("planes", 1000.0, 1.25))
    assert sp.calls == [("set_walls", "planes", 1000.0, 1.25), ("pair_damping", 1, 2, 7.0), ("wall_damping", 4.0),
                        ("pair_friction", 1, "*", 0.5, 20.0), ("wall_friction", 0.3, 9.0), ("wall_velocity", [0, 0, 1.0])]
