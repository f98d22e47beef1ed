"""GPU tests that pin what the host layer of the two axial families says and keeps (csrc/shstep_cylinders.hip, csrc/shstep_cones.hip,
through the C ABI of include/shstep.h): every refusal of the coefficient setters, the passes, the read-backs and the history
calls by its whole message and its error code, and the state a set of coefficients leaves whatever order its setters came
in.  The same scenarios run for one cylinder and for one cone; the messages are written out here, per family, not formed
from the library's words.  Marked gpu because the first shstep_* call of a context needs a device; the refusals need no
particle, the passes take 2, the order test 4."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

gpu = pytest.mark.gpu
EINVAL, ESTATE = -1, -4
LMAX, NQ, KN, EXPO = 2, 4, 1000.0, 1.25
THETA = math.radians(30.0)


class Family:
    """The calls of one family by role, and its geometry: one surface about the z axis through the origin."""

    def __init__(self, name):
        self.name = name
        cyl = name == "cylinder"
        self.width, self.xi = (7, 2) if cyl else (8, 3)
        self.geometry = [0, 0, 0, 0, 0, 1, 5.0] if cyl else [0, 0, 0, 0, 0, 1, math.cos(THETA), math.sin(THETA)]
        self.c = dict(
            set="shstep_set_cylinders" if cyl else "shstep_set_cones", get="shstep_get_cylinders" if cyl else "shstep_get_cones",
            damping="shstep_set_cylinder_damping" if cyl else "shstep_set_cone_damping",
            friction="shstep_set_cylinder_friction" if cyl else "shstep_set_cone_friction",
            rotation="shstep_set_cylinder_rotation" if cyl else "shstep_set_cone_rotation",
            spring="shstep_set_cyl_tangential_spring" if cyl else "shstep_set_conic_tangential_spring",
            rolling="shstep_set_rolling_cyl" if cyl else "shstep_set_rolling_con",
            twisting="shstep_set_twisting_cyl" if cyl else "shstep_set_twisting_con",
            copy="shstep_copy_cyl_history" if cyl else "shstep_copy_conic_history",
            put="shstep_set_cyl_history" if cyl else "shstep_set_conic_history",
            stats="shstep_get_cylinder_stats" if cyl else "shstep_get_cone_stats")
        # the Python names of the same, for the passes and the order test
        self.py = dict(
            set="set_cylinders" if cyl else "set_cones", damping="cylinder_damping" if cyl else "cone_damping",
            friction="cylinder_friction" if cyl else "cone_friction", rotation="cylinder_rotation" if cyl else "cone_rotation",
            spring="set_cyl_tangential_spring" if cyl else "conic_spring", rolling="cylinder_rolling" if cyl else "conic_rolling",
            twisting="cylinder_twisting" if cyl else "conic_twisting", force="cylinder_force_device" if cyl else "cone_force_device",
            contact="cyl_contact_device" if cyl else "conic_contact_device", history="cyl_history" if cyl else "conic_history",
            stats="cylinder_stats" if cyl else "cone_stats", reads_twists="cylinder_reads_twists" if cyl else "cone_reads_twists",
            has_history="has_cyl_history" if cyl else "has_conic_history", has_rolling="has_cyl_rolling" if cyl else "has_conic_rolling",
            out="cyl_out" if cyl else "cone_out")

    def ctx(self, nsurf=1):
        from shpair import ShPair, shapes
        sp = ShPair(0)
        sp.settings(NQ)
        sp.set_ntypes(1, 1)
        sp.set_shape(0, LMAX, shapes.random_shape(LMAX, 7))
        sp.coeff(1, 1, KN, EXPO)
        if nsurf:
            getattr(sp, self.py["set"])([self.geometry] * nsurf, KN, EXPO)
        return sp

    def raw(self, sp, role, *args):
        """The C function of a role with ctypes arguments as they are; the error as the Python layer reports it."""
        sp._chk(getattr(sp._lib, self.c[role])(sp._h, *args))

    def centres(self, sp, n):
        """n centres 0.7 R_max from the surface (the shape's least radius is 0.88 of its largest), at n azimuths and heights."""
        h = 0.7 * sp.rmax(0)
        t = 6.0 + 0.25 * np.arange(n)
        d = 5.0 - h if self.name == "cylinder" else (math.sin(THETA) * t - h) / math.cos(THETA)
        phi = 0.3 + 2.0 * math.pi * np.arange(n) / n
        return np.stack([d * np.cos(phi), d * np.sin(phi), t], axis=1)


def _arr(*v):
    return (C.c_double * len(v))(*v)


def _refused(code, msg, call, *args, **kw):
    from shpair.capi import ShPairError
    with pytest.raises(ShPairError) as e:
        call(*args, **kw)
    assert e.value.code == code, str(e.value)
    assert str(e.value).endswith(" — " + msg), str(e.value)


FAMILIES = ["cylinder", "cone"]

# ---- the setters: count, null table, negative and non-finite values ------------------------------------------------------

# role: (tables, {scenario: message})
SETTER_MESSAGES = {
    "cylinder": {
        "damping": (1, {
            "count": "cylinder damping: 2 coefficients for 1 cylinders (call it after shstep_set_cylinders)",
            "null": "cylinder damping: null array pointer",
            "negative": ["cylinder 0: damping coefficient -1 must be finite and >= 0"],
            "nan": ["cylinder 0: damping coefficient nan must be finite"],
            "inf": ["cylinder 0: damping coefficient inf must be finite"]}),
        "friction": (2, {
            "count": "cylinder friction: 2 coefficients for 1 cylinders (call it after shstep_set_cylinders)",
            "null": "cylinder friction: null array pointer",
            "negative": ["cylinder 0: friction coefficient mu -1 must be finite and >= 0",
                         "cylinder 0: friction coefficient gamma_t -1 must be finite and >= 0"],
            "nan": ["cylinder 0: friction coefficient mu nan must be finite", "cylinder 0: friction coefficient gamma_t nan must be finite"],
            "inf": ["cylinder 0: friction coefficient mu inf must be finite", "cylinder 0: friction coefficient gamma_t inf must be finite"]}),
        "rotation": (1, {
            "count": "cylinder rotation: 2 coefficients for 1 cylinders (call it after shstep_set_cylinders)",
            "null": "cylinder rotation: null array pointer",
            "negative": [None],   # any sign
            "nan": ["cylinder 0: angular velocity nan must be finite"],
            "inf": ["cylinder 0: angular velocity inf must be finite"]}),
        "spring": (1, {
            "count": "cylinder tangential spring: 2 coefficients for 1 cylinders (call it after shstep_set_cylinders)",
            "null": "cylinder tangential spring: null array pointer",
            "negative": ["cylinder 0: tangential spring k_t -1 must be finite and >= 0"],
            "nan": ["cylinder 0: tangential spring k_t nan must be finite"],
            "inf": ["cylinder 0: tangential spring k_t inf must be finite"]}),
        "rolling": (2, {
            "count": "cylinder rolling resistance: 2 coefficients for 1 cylinders (call it after shstep_set_cylinders)",
            "null": "cylinder rolling resistance: null array pointer",
            "negative": ["cylinder 0: rolling coefficient mu_r -1 must be finite and >= 0",
                         "cylinder 0: rolling coefficient gamma_r -1 must be finite and >= 0"],
            "nan": ["cylinder 0: rolling coefficient mu_r nan must be finite", "cylinder 0: rolling coefficient gamma_r nan must be finite"],
            "inf": ["cylinder 0: rolling coefficient mu_r inf must be finite", "cylinder 0: rolling coefficient gamma_r inf must be finite"]}),
        "twisting": (2, {
            "count": "cylinder twisting resistance: 2 coefficients for 1 cylinders (call it after shstep_set_cylinders)",
            "null": "cylinder twisting resistance: null array pointer",
            "negative": ["cylinder 0: twisting coefficient mu_tw -1 must be finite and >= 0",
                         "cylinder 0: twisting coefficient gamma_tw -1 must be finite and >= 0"],
            "nan": ["cylinder 0: twisting coefficient mu_tw nan must be finite", "cylinder 0: twisting coefficient gamma_tw nan must be finite"],
            "inf": ["cylinder 0: twisting coefficient mu_tw inf must be finite", "cylinder 0: twisting coefficient gamma_tw inf must be finite"]}),
    },
    "cone": {
        "damping": (1, {
            "count": "cone damping: 2 coefficients for 1 cones (call it after shstep_set_cones)",
            "null": "cone damping: null array pointer",
            "negative": ["cone 0: damping coefficient -1 must be finite and >= 0"],
            "nan": ["cone 0: damping coefficient nan must be finite"],
            "inf": ["cone 0: damping coefficient inf must be finite"]}),
        "friction": (2, {
            "count": "cone friction: 2 coefficients for 1 cones (call it after shstep_set_cones)",
            "null": "cone friction: null array pointer",
            "negative": ["cone 0: friction coefficient mu -1 must be finite and >= 0",
                         "cone 0: friction coefficient gamma_t -1 must be finite and >= 0"],
            "nan": ["cone 0: friction coefficient mu nan must be finite", "cone 0: friction coefficient gamma_t nan must be finite"],
            "inf": ["cone 0: friction coefficient mu inf must be finite", "cone 0: friction coefficient gamma_t inf must be finite"]}),
        "rotation": (1, {
            "count": "cone rotation: 2 coefficients for 1 cones (call it after shstep_set_cones)",
            "null": "cone rotation: null array pointer",
            "negative": [None],   # any sign
            "nan": ["cone 0: angular velocity nan must be finite"],
            "inf": ["cone 0: angular velocity inf must be finite"]}),
        "spring": (1, {
            "count": "cone tangential spring: 2 coefficients for 1 cones (call it after shstep_set_cones)",
            "null": "cone tangential spring: null array pointer",
            "negative": ["cone 0: tangential spring k_t -1 must be finite and >= 0"],
            "nan": ["cone 0: tangential spring k_t nan must be finite"],
            "inf": ["cone 0: tangential spring k_t inf must be finite"]}),
        "rolling": (2, {
            "count": "cone rolling resistance: 2 coefficients for 1 cones (call it after shstep_set_cones)",
            "null": "cone rolling resistance: null array pointer",
            "negative": ["cone 0: rolling coefficient mu_r -1 must be finite and >= 0",
                         "cone 0: rolling coefficient gamma_r -1 must be finite and >= 0"],
            "nan": ["cone 0: rolling coefficient mu_r nan must be finite", "cone 0: rolling coefficient gamma_r nan must be finite"],
            "inf": ["cone 0: rolling coefficient mu_r inf must be finite", "cone 0: rolling coefficient gamma_r inf must be finite"]}),
        "twisting": (2, {
            "count": "cone twisting resistance: 2 coefficients for 1 cones (call it after shstep_set_cones)",
            "null": "cone twisting resistance: null array pointer",
            "negative": ["cone 0: twisting coefficient mu_tw -1 must be finite and >= 0",
                         "cone 0: twisting coefficient gamma_tw -1 must be finite and >= 0"],
            "nan": ["cone 0: twisting coefficient mu_tw nan must be finite", "cone 0: twisting coefficient gamma_tw nan must be finite"],
            "inf": ["cone 0: twisting coefficient mu_tw inf must be finite", "cone 0: twisting coefficient gamma_tw inf must be finite"]}),
    },
}
BAD = {"negative": -1.0, "nan": float("nan"), "inf": float("inf")}


@gpu
@pytest.mark.parametrize("role", ["damping", "friction", "rotation", "spring", "rolling", "twisting"])
@pytest.mark.parametrize("family", FAMILIES)
def test_a_setter_refuses_by_its_message_and_changes_nothing(family, role):
    F = Family(family)
    ntab, want = SETTER_MESSAGES[family][role]
    sp = F.ctx()
    good = _arr(0.5)
    # the count comes first: before the null pointer, and before the values
    _refused(EINVAL, want["count"], F.raw, sp, role, 2, *([None] * ntab))
    for k in range(ntab):   # a null table, each place
        _refused(EINVAL, want["null"], F.raw, sp, role, 1, *[None if j == k else good for j in range(ntab)])
    for kind, v in BAD.items():   # a bad value, each table; the other table is good
        for k in range(ntab):
            args = [_arr(v) if j == k else good for j in range(ntab)]
            if want[kind][k] is None:
                F.raw(sp, role, 1, *args)
                F.raw(sp, role, 1, *[_arr(0.0)] * ntab)
            else:
                _refused(EINVAL, want[kind][k], F.raw, sp, role, 1, *args)
    # a refused call changes nothing: the library still takes the pass without twists, and without a time step
    import torch
    from dissipation_common import dev
    n = 2
    x, q = dev(F.centres(sp, n)), dev(np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)))
    sh, m = dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32))
    f, tq = (torch.zeros(n, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
    getattr(sp, F.py["force"])(n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(), twist=None)
    torch.cuda.synchronize()
    assert f.cpu().numpy().any()
    # no surface set: the count of any call but 0 is wrong, and 0 is taken with null tables
    bare = F.ctx(nsurf=0)
    _refused(EINVAL, want["count"].replace("2 coefficients for 1", "1 coefficients for 0"), F.raw, bare, role, 1, *[good] * ntab)
    F.raw(bare, role, 0, *([None] * ntab))
    bare.close()
    sp.close()


# ---- the two ledgers, in both orders --------------------------------------------------------------------------------------

# setter first refused under a ledger: {ledger: {role: message or None (accepted)}}
UNDER_LEDGER = {
    "cylinder": {
        "energy": {
            "damping": "cylinder damping: the energy ledger is on and keeps no cylinder entries (docs/SPEC.md 2.18); switch it off "
                       "(shstep_set_energy_ledger) or leave every cylinder coefficient 0",
            "friction": "cylinder friction: the energy ledger is on and keeps no cylinder entries (docs/SPEC.md 2.18); switch it off "
                        "(shstep_set_energy_ledger) or leave every cylinder coefficient 0",
            "rotation": None,   # Omega alone is no coefficient, and does no work on an elastic contact
            "spring": "cylinder tangential spring: the energy ledger is on and keeps no cylinder entries (docs/SPEC.md 2.18); switch it off "
                      "(shstep_set_energy_ledger) or leave every cylinder coefficient 0",
            "rolling": "cylinder rolling resistance: the energy ledger is on and keeps no cylinder entries (docs/SPEC.md 2.18); switch it off "
                       "(shstep_set_energy_ledger) or leave every cylinder coefficient 0",
            "twisting": "cylinder twisting resistance: the energy ledger is on and keeps no cylinder entries (docs/SPEC.md 2.18); switch it "
                        "off (shstep_set_energy_ledger) or leave every cylinder coefficient 0"},
        "shell": {r: None for r in ("damping", "friction", "rotation", "spring", "rolling", "twisting")},
        "both": {r: None for r in ("damping", "friction", "rotation", "spring", "rolling", "twisting")}},
    "cone": {
        "energy": {
            "damping": "cone damping: the energy ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                       "(shstep_set_energy_ledger) or leave every cone coefficient and Omega 0",
            "friction": "cone friction: the energy ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                        "(shstep_set_energy_ledger) or leave every cone coefficient and Omega 0",
            "rotation": "cone rotation: the energy ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                        "(shstep_set_energy_ledger) or leave every cone coefficient and Omega 0",
            "spring": "cone tangential spring: the energy ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                      "(shstep_set_energy_ledger) or leave every cone coefficient and Omega 0",
            "rolling": "cone rolling resistance: the energy ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                       "(shstep_set_energy_ledger) or leave every cone coefficient and Omega 0",
            "twisting": "cone twisting resistance: the energy ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                        "(shstep_set_energy_ledger) or leave every cone coefficient and Omega 0"},
        "shell": {
            "damping": "cone damping: the shell ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                       "(shstep_set_shell_ledger) or leave every cone coefficient and Omega 0",
            "friction": "cone friction: the shell ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                        "(shstep_set_shell_ledger) or leave every cone coefficient and Omega 0",
            "rotation": "cone rotation: the shell ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                        "(shstep_set_shell_ledger) or leave every cone coefficient and Omega 0",
            "spring": "cone tangential spring: the shell ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                      "(shstep_set_shell_ledger) or leave every cone coefficient and Omega 0",
            "rolling": "cone rolling resistance: the shell ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                       "(shstep_set_shell_ledger) or leave every cone coefficient and Omega 0",
            "twisting": "cone twisting resistance: the shell ledger is on and keeps no cone entries (docs/SPEC.md 2.22); switch it off "
                        "(shstep_set_shell_ledger) or leave every cone coefficient and Omega 0"}},
}
UNDER_LEDGER["cone"]["both"] = UNDER_LEDGER["cone"]["energy"]   # the energy ledger's words while both are on

# coefficient first, the ledger refused: {role: {ledger: message or None}}
BEHIND_COEFFICIENT = {
    "cylinder": {
        "damping": {"energy": "energy ledger: a cylinder damping or friction coefficient is set and the ledger keeps no cylinder "
                              "entries (docs/SPEC.md 2.18); set every cylinder coefficient to 0 first", "shell": None},
        "friction": {"energy": "energy ledger: a cylinder damping or friction coefficient is set and the ledger keeps no cylinder "
                               "entries (docs/SPEC.md 2.18); set every cylinder coefficient to 0 first", "shell": None},
        "rotation": {"energy": None, "shell": None},
        "spring": {"energy": "energy ledger: a cylinder tangential spring is set and the ledger keeps no cylinder entries "
                             "(docs/SPEC.md 2.19); set every cylinder k_t to 0 first", "shell": None},
        "rolling": {"energy": "energy ledger: cylinder rolling or twisting resistance is set and the ledger keeps no cylinder "
                              "entries (docs/SPEC.md 2.21); set every cylinder rolling and twisting coefficient to 0 first", "shell": None},
        "twisting": {"energy": "energy ledger: cylinder rolling or twisting resistance is set and the ledger keeps no cylinder "
                               "entries (docs/SPEC.md 2.21); set every cylinder rolling and twisting coefficient to 0 first", "shell": None}},
    "cone": {
        role: {"energy": "energy ledger: a cone damping or friction coefficient or a cone rotation is set and the ledger keeps "
                         "no cone entries (docs/SPEC.md 2.22); set every cone coefficient and Omega to 0 first",
               "shell": "shell ledger: a cone damping or friction coefficient or a cone rotation is set and the ledger keeps "
                        "no cone entries (docs/SPEC.md 2.22); set every cone coefficient and Omega to 0 first"}
        for role in ("damping", "friction", "rotation", "rolling", "twisting")},
}
BEHIND_COEFFICIENT["cone"]["spring"] = {
    "energy": "energy ledger: a cone tangential spring is set and the ledger keeps no cone entries (docs/SPEC.md 2.23); set every "
              "cone k_t to 0 first",
    "shell": "shell ledger: a cone tangential spring is set and the ledger keeps no cone entries (docs/SPEC.md 2.23); set every "
             "cone k_t to 0 first"}
SHELL_OFF_UNDER_COEFFICIENT = ("shell ledger: the energy ledger is on and a cylinder coefficient or tangential spring is set "
                               "(docs/SPEC.md 2.20); switch the energy ledger off or set every cylinder coefficient to 0 first")


def _set(F, sp, role, on=True):
    """What switches a role's coefficient on (the spring takes its mu from the friction setter: gamma_t stays 0), or all off."""
    v = _arr(0.5 if on else 0.0)
    if role == "spring":
        F.raw(sp, "friction", 1, v, _arr(0.0))
    F.raw(sp, role, 1, *([v] * SETTER_MESSAGES[F.name][role][0]))
    if role == "spring" and not on:
        F.raw(sp, "friction", 1, v, v)


def _ledgers(sp, which, on):
    for name in (("energy", "shell") if which == "both" else (which,)):
        sp._chk(getattr(sp._lib, f"shstep_set_{name}_ledger")(sp._h, int(on)))


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_a_ledger_and_a_coefficient_refuse_each_other_in_either_order(family):
    F = Family(family)
    sp = F.ctx()
    roles = ("damping", "friction", "rotation", "spring", "rolling", "twisting")
    # the ledger first
    for which in ("energy", "shell", "both"):
        if family == "cylinder" and which == "both":
            _ledgers(sp, "shell", True)
            _ledgers(sp, "energy", True)
        else:
            _ledgers(sp, which, True)
        for role in roles:
            want = UNDER_LEDGER[family][which][role]
            if role == "spring":
                # mu alone switches nothing on: the friction setter is taken, the spring behind it is what is refused
                F.raw(sp, "friction", 1, _arr(0.5), _arr(0.0))
            v = [_arr(0.5)] * SETTER_MESSAGES[family][role][0]
            if want is None:
                F.raw(sp, role, 1, *v)
                if family == "cylinder" and which == "both" and role != "rotation":
                    _refused(ESTATE, SHELL_OFF_UNDER_COEFFICIENT, _ledgers, sp, "shell", False)   # off would recreate the refused state
            else:
                _refused(ESTATE, want, F.raw, sp, role, 1, *v)
            getattr(sp, F.py["set"])([F.geometry], KN, EXPO)   # every coefficient 0 again
        _ledgers(sp, "energy" if which == "both" else which, False)
        if which == "both":
            _ledgers(sp, "shell", False)
    # the coefficient first
    for role in roles:
        _set(F, sp, role)
        for which in ("energy", "shell"):
            want = BEHIND_COEFFICIENT[family][role][which]
            if want is None:
                _ledgers(sp, which, True)
                _ledgers(sp, which, False)
            else:
                _refused(ESTATE, want, _ledgers, sp, which, True)
        getattr(sp, F.py["set"])([F.geometry], KN, EXPO)
    sp.close()


# ---- the passes: null twist per switch, the call without a time step under a spring, a bad dt -----------------------------

PASS_MESSAGES = {
    "cylinder": {
        "nlocal": "nlocal -1 < 0", "null": "null array pointer",
        "damping": "cylinder damping: null twist pointer", "friction": "cylinder friction: null twist pointer",
        "spring": "cylinder tangential spring: null twist pointer",
        "rolling": "cylinder rolling or twisting resistance: null twist pointer",
        "twisting": "cylinder rolling or twisting resistance: null twist pointer",
        "old form": "a cylinder tangential spring is set: the cylinder pass needs the form with a time step (shstep_cyl_contact_device)",
        "dt negative": "cylinder contact: dt -1 must be finite and >= 0", "dt nan": "cylinder contact: dt nan must be finite and >= 0",
        "dt inf": "cylinder contact: dt inf must be finite and >= 0", "stats": "null output pointer"},
    "cone": {
        "nlocal": "nlocal -1 < 0", "null": "null array pointer",
        "damping": "cone damping: null twist pointer", "friction": "cone friction: null twist pointer",
        "spring": "cone tangential spring: null twist pointer",
        "rolling": "cone rolling or twisting resistance: null twist pointer",
        "twisting": "cone rolling or twisting resistance: null twist pointer",
        "old form": "a cone tangential spring is set: the cone pass needs the form with a time step (shstep_conic_contact_device)",
        "dt negative": "cone contact: dt -1 must be finite and >= 0", "dt nan": "cone contact: dt nan must be finite and >= 0",
        "dt inf": "cone contact: dt inf must be finite and >= 0", "stats": "null output pointer"},
}


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_a_pass_refuses_by_its_message_and_adds_nothing(family):
    import torch
    from dissipation_common import dev
    F = Family(family)
    want = PASS_MESSAGES[family]
    sp = F.ctx()
    n = 2
    x, q = dev(F.centres(sp, n)), dev(np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)))
    sh, m = dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32))
    f, tq = (torch.zeros(n, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
    tw = torch.zeros(n, 6, dtype=torch.float64, device="cuda:0")
    ptr = [x.data_ptr(), q.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr()]
    force, contact = getattr(sp, F.py["force"]), getattr(sp, F.py["contact"])
    _refused(EINVAL, want["nlocal"], force, -1, *ptr)
    _refused(EINVAL, want["nlocal"], contact, -1, *ptr, None, 0.0)
    for k in range(6):   # a null array, each place, either form
        holed = [None if j == k else p for j, p in enumerate(ptr)]
        _refused(EINVAL, want["null"], force, n, *holed)
        _refused(EINVAL, want["null"], contact, n, *holed, tw.data_ptr(), 0.0)
    for kind, dt in (("dt negative", -1.0), ("dt nan", float("nan")), ("dt inf", float("inf"))):
        _refused(EINVAL, want[kind], contact, n, *ptr, tw.data_ptr(), dt)
    for role in ("damping", "friction", "spring", "rolling", "twisting"):   # a null twist, per switch
        _set(F, sp, role)
        if role == "spring":   # ... and under a spring the form without a time step is refused ahead of everything else
            _refused(EINVAL, want["old form"], force, n, *ptr, twist=tw.data_ptr())
            _refused(EINVAL, want["old form"], force, -1, *([None] * 6))
        else:
            _refused(EINVAL, want[role], force, n, *ptr, twist=None)
        _refused(EINVAL, want[role], contact, n, *ptr, None, 1e-3)
        getattr(sp, F.py["set"])([F.geometry], KN, EXPO)
    # both kinds of coefficient: the damping's words while a gamma is set, the friction's otherwise
    _set(F, sp, "friction")
    _set(F, sp, "rolling")
    _refused(EINVAL, want["friction"], force, n, *ptr, twist=None)
    _set(F, sp, "damping")
    _refused(EINVAL, want["damping"], force, n, *ptr, twist=None)
    torch.cuda.synchronize()
    assert not f.any() and not tq.any()
    _refused(EINVAL, want["stats"], F.raw, sp, "stats", None)
    assert getattr(sp, F.py["stats"])() == 0   # no pass has run
    sp.close()


# ---- the read-back of the geometry and the history calls -------------------------------------------------------------------

STATE_MESSAGES = {
    "cylinder": {
        "get count": "get cylinders: room for 2 cylinders, 1 are set", "get null": "get cylinders: null output pointer",
        "copy off": "copy cylinder history: no cylinder tangential spring is set (shstep_set_cyl_tangential_spring)",
        "put off": "set cylinder history: no cylinder tangential spring is set (shstep_set_cyl_tangential_spring)",
        "copy negative": "copy cylinder history: nlocal -1, the history is held for -1 rows",
        "copy nlocal": "copy cylinder history: nlocal 3, the history is held for 2 rows",
        "copy null": "copy cylinder history: null output pointer",
        "put nlocal": "set cylinder history: nlocal 0 < 1", "put null": "set cylinder history: null array pointer",
        "put nan": "set cylinder history: particle 1, cylinder 0: a number that is not finite"},
    "cone": {
        "get count": "get cones: room for 2 cones, 1 are set", "get null": "get cones: null output pointer",
        "copy off": "copy cone history: no cone tangential spring is set (shstep_set_conic_tangential_spring)",
        "put off": "set cone history: no cone tangential spring is set (shstep_set_conic_tangential_spring)",
        "copy negative": "copy cone history: nlocal -1, the history is held for -1 rows",
        "copy nlocal": "copy cone history: nlocal 3, the history is held for 2 rows",
        "copy null": "copy cone history: null output pointer",
        "put nlocal": "set cone history: nlocal 0 < 1", "put null": "set cone history: null array pointer",
        "put nan": "set cone history: particle 1, cone 0: a number that is not finite"},
}


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_the_read_backs_and_the_history_calls_refuse_by_their_messages(family):
    F = Family(family)
    want = STATE_MESSAGES[family]
    sp = F.ctx()
    room = _arr(*([0.0] * 16))
    _refused(EINVAL, want["get count"], F.raw, sp, "get", 2, room)
    _refused(EINVAL, want["get null"], F.raw, sp, "get", 1, None)
    F.raw(sp, "get", 1, room)
    assert list(room[:F.width]) == [float(v) for v in F.geometry]
    bare = F.ctx(nsurf=0)
    F.raw(bare, "get", 0, None)   # nothing set: nothing is written
    bare.close()
    # no spring: the state's refusal comes ahead of every argument's
    xi = _arr(*([0.25] * (3 * F.xi)))
    _refused(ESTATE, want["copy off"], F.raw, sp, "copy", 2, xi)
    _refused(ESTATE, want["copy off"], F.raw, sp, "copy", -1, None)
    _refused(ESTATE, want["put off"], F.raw, sp, "put", 2, xi)
    _refused(ESTATE, want["put off"], F.raw, sp, "put", 0, None)
    _set(F, sp, "friction")   # mu and gamma_t, no k_t: still no spring
    _refused(ESTATE, want["copy off"], F.raw, sp, "copy", 2, xi)
    _set(F, sp, "spring")
    _refused(EINVAL, want["copy negative"], F.raw, sp, "copy", -1, xi)
    _refused(EINVAL, want["copy null"], F.raw, sp, "copy", 2, None)
    F.raw(sp, "copy", 0, None)
    _refused(EINVAL, want["put nlocal"], F.raw, sp, "put", 0, xi)
    _refused(EINVAL, want["put null"], F.raw, sp, "put", 2, None)
    bad = _arr(*([0.25] * F.xi + [float("nan")] + [0.25] * (F.xi - 1)))
    _refused(EINVAL, want["put nan"], F.raw, sp, "put", 2, bad)
    F.raw(sp, "copy", 3, xi)   # nothing live yet: any nlocal is taken, and reads as zeros
    assert not any(xi)
    xi = _arr(*([0.25] * (3 * F.xi)))
    F.raw(sp, "put", 2, xi)
    _refused(EINVAL, want["copy nlocal"], F.raw, sp, "copy", 3, xi)
    back = _arr(*([0.0] * (2 * F.xi)))
    F.raw(sp, "copy", 2, back)
    assert list(back) == [0.25] * (2 * F.xi)
    # a change of hist drops the history; the spring set again starts from nothing live
    F.raw(sp, "spring", 1, _arr(0.0))
    _refused(ESTATE, want["copy off"], F.raw, sp, "copy", 2, back)
    F.raw(sp, "spring", 1, _arr(0.5))
    F.raw(sp, "copy", 2, back)
    assert not any(back)
    sp.close()


# ---- the state a set of coefficients leaves, whatever order the setters came in --------------------------------------------

ORDERS = {"friction, spring": ("friction", "spring", "rolling", "twisting", "rotation", "damping"),
          "spring, friction": ("spring", "friction", "rolling", "twisting", "rotation", "damping"),
          "rolling, damping": ("rolling", "damping", "twisting", "rotation", "spring", "friction")}
VALUES = dict(damping=(3.0,), friction=(0.4, 2.0), spring=(150.0,), rolling=(0.05, 3.0), twisting=(0.03, 2.0), rotation=(0.7,))


def _one_pass(F, order):
    """The switches, f, torque, the row totals and xi of one advancing pass over 4 particles at the surface."""
    import torch
    from dissipation_common import dev
    sp = F.ctx()
    for role in order:
        getattr(sp, F.py[role])(*VALUES[role])
    switches = tuple(bool(getattr(sp, F.py[k])) for k in ("reads_twists", "has_history", "has_rolling"))
    n = 4
    rng = np.random.default_rng(5)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    x, qd, tw = dev(F.centres(sp, n)), dev(q), dev(rng.normal(size=(n, 6)))
    sh, m = dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32))
    f, tq = (torch.zeros(n, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
    out = torch.zeros(1, 5, dtype=torch.float64, device="cuda:0")
    ptr = (n, x.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    from shpair.capi import ShPairError
    with pytest.raises(ShPairError):   # the library's own switches: a spring is set, a coefficient is set
        getattr(sp, F.py["force"])(*ptr, twist=tw.data_ptr())
    with pytest.raises(ShPairError):
        getattr(sp, F.py["contact"])(*ptr, None, 1e-3)
    getattr(sp, F.py["contact"])(*ptr, tw.data_ptr(), 1e-3, **{F.py["out"]: out.data_ptr()})
    torch.cuda.synchronize()
    got = (f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy(), getattr(sp, F.py["history"])(n))
    ncontact = getattr(sp, F.py["stats"])()
    sp.close()
    return switches, got, ncontact


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_the_order_of_the_setters_leaves_the_same_state(family):
    F = Family(family)
    ref_switches, ref, ncontact = _one_pass(F, ORDERS["friction, spring"])
    assert ref_switches == (True, True, True) and ncontact == 4
    assert all(a.any() for a in ref)   # every output carries something
    assert ref[3].shape == (4, 1, F.xi) and (ref[3] != 0).any(axis=2).all()   # every spring is live
    for name in ("spring, friction", "rolling, damping"):
        switches, got, nc = _one_pass(F, ORDERS[name])
        assert switches == ref_switches and nc == ncontact, name
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), name
