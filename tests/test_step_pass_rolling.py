"""CPU tests of where the Python force pass (shpair/step_pass.py) puts the rolling pass of docs/SPEC.md §2.16: behind the
pair pass and ahead of the reverse exchange, as step_dissipation_pass of csrc/shstep_run.cpp; alone, without any pair
pass; not at all while the predicate is false.  No GPU and no library."""
import numpy as np
import pytest

from shpair.step_pass import StepView, apply_contact_options, force_pass

T, F, C, P, H, RO, R, W = ("twist_device", "forward", "compute_device", "pair_dissipation_device", "pair_contact_device",
                           "pair_rolling_device", "reverse", "wall_force_damped_device")
X, QUAT, V, L, TY, SH, MASK, FO, TQ, TW, EV = range(101, 112)


class Recorder:
    """Stands in for the context, with the predicates of a binding that knows rolling; records (name, args, kwargs)."""

    def __init__(self, pair_pass, rolling, history=False, nwalls=0):
        self.has_pair_pass, self.has_rolling, self.has_history = bool(pair_pass), bool(rolling), bool(history)
        self.keeps_integrals = self.has_dissipation = bool(pair_pass or rolling)
        self.wall_reads_twists = self.walls_advance = False
        self.nwalls = nwalls
        self.calls = []

    def _rec(name):
        def call(self, *args, **kw):
            self.calls.append((name, args, kw))
        return call
    twist_device, compute_device, pair_dissipation_device, pair_contact_device = _rec(T), _rec(C), _rec(P), _rec(H)
    pair_rolling_device, wall_force_damped_device = _rec(RO), _rec(W)


def run_pass(pair_pass, rolling, history=False, nwalls=0, nlocal=5, nghost=2):
    sp = Recorder(pair_pass, rolling, history, nwalls)
    v = StepView(nlocal, nghost, X, QUAT, V, L, TY, SH, MASK, FO, TQ, TW, 1, 1e-3, np.zeros(3), 0.0, 0.0, 77)
    force_pass(sp, v, lambda twist: sp.calls.append((F, (twist,), {})), lambda: sp.calls.append((R, (), {})), nghost, advance=True)
    return sp.calls


def test_rolling_sits_between_the_pair_pass_and_reverse():
    assert [c[0] for c in run_pass(1, 1)] == [T, F, C, P, RO, R]
    assert [c[0] for c in run_pass(1, 1, history=True)] == [T, F, C, H, RO, R]
    assert [c[0] for c in run_pass(1, 1, nwalls=2)] == [T, F, C, P, RO, R, W]


def test_rolling_alone_has_no_pair_pass():
    calls = run_pass(0, 1)
    assert [c[0] for c in calls] == [T, F, C, RO, R]
    assert calls[1][1] == (TW,)          # the ghost rows need their owners' twists: the forward exchange is the wide one


def test_rolling_call_is_on_the_views_stream_with_the_views_arrays():
    call = [c for c in run_pass(0, 1) if c[0] == RO][0]
    assert call == (RO, (5, 2, X, TY, TW, TQ), {"stream": 77})      # torque only: the pass takes no f


@pytest.mark.parametrize("pair_pass", [0, 1])
def test_rolling_is_absent_while_the_predicate_is_false(pair_pass):
    assert [c[0] for c in run_pass(pair_pass, 0)] == ([T, F, C, P, R] if pair_pass else [F, C, R])


def test_contact_options_pass_the_two_kinds_through():
    class Ctx:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if name not in ("pair_friction", "pair_rolling", "pair_twisting"):
                raise AttributeError(name)
            return lambda *a: self.calls.append((name,) + a)
    sp = Ctx()
    apply_contact_options(sp, pair_twisting={(1, 1): (0.02, 3.0)}, pair_rolling={(1, "*"): (0.05, 2.0)},
                          pair_friction={(1, 2): (0.5, 20.0)})
    assert sp.calls == [("pair_friction", 1, 2, 0.5, 20.0), ("pair_rolling", 1, "*", 0.05, 2.0), ("pair_twisting", 1, 1, 0.02, 3.0)]
