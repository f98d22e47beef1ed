"""GPU tests of the rolling and twisting resistance at conical walls of docs/SPEC.md §2.24 (csrc/conic_roll_kernels.hpp,
through the C ABI of include/shstep.h) against tests/conic_roll_ref.py at the gate of SPEC §4 as tests/test_gpu_cyl_roll.py
applies it, 1e-9: parity on tests/conic_roll_cases.py's bed of 40 particles in eight cones behind every instance of the
contact kernel and through both forms of the call, off is off, stale rows, "deterministic", the physical cases, the three
run loops and the refusals.

The condition on the inputs (test_the_bed_takes_every_branch) needs no GPU: it reads the reference alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conic_roll_cases as K   # noqa: E402

gpu = pytest.mark.gpu
TOL = 1e-9
NBED, KN, EXPO = K.NBED, K.KN, K.EXPO


def _ctx(lmax, nq, name="elastic", det=0, roll=True):
    """A context with the bed's cones and the coefficients of a contact-kernel instance."""
    from dissipation_common import _wall_ctx
    coef = K.INSTANCES[name][0]
    sp = _wall_ctx([(lmax, K.shape(lmax))], nq, kn=KN, expo=EXPO, deterministic=det)
    sp.set_cones(K.cones(), KN, EXPO)
    sp.cone_rotation(K.OMEGA)
    if coef is not None:
        sp.cone_damping(coef["gamma"])
        sp.cone_friction(coef["mu"], coef["gt"])
        if "kt" in coef:
            sp.conic_spring(coef["kt"])
    if roll:
        sp.conic_twisting(K.MUTW, K.GTW)       # (the two setters in either order: twisting first here)
        sp.conic_rolling(K.MUR, K.GR)
    return sp


def _pass(sp, lmax, name="elastic", n=NBED, mask=None, want_out=True, tw=None):
    """One cone pass over the first n particles of the bed on fresh arrays: f, torque, cone_out."""
    from test_gpu_conic_history import Pass
    x, quat, tw0, m0 = K.bed(lmax)
    tw = tw0 if tw is None else tw
    dt = K.INSTANCES[name][1]
    if sp.has_conic_history:
        sp.reset_conic_history()                                # every pass here starts from nothing live, as the reference
    return Pass(sp, n).go(x[:n], quat[:n], tw[:n], dt or 0.0, mask=(m0 if mask is None else mask)[:n], old_call=dt is None, want_out=want_out)


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _errors(got, ref, plain=None):
    """Relative errors of f, torque, cone_out (M_ax against the torque scale) and, given the same pass with the kinds off,
    of the couple alone."""
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ro = ref["cone_out"]
    e = dict(f=np.abs(got[0] - ref["f"]).max() / scale, torque=np.abs(got[1] - ref["torque"]).max() / tscale,
             wall=np.abs(got[2][:, :4] - ro[:, :4]).max() / np.abs(ro[:, :4]).max(),
             M_ax=np.abs(got[2][:, 4] - ro[:, 4]).max() / max(tscale, np.abs(ro[:, 4]).max()))
    if plain is not None:
        e["couple"] = np.abs((got[1] - plain[1]) - ref["couple"]).max() / tscale
    return e


# ---- 1. the inputs (no GPU) ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lmax,nq", K.CONFIGS)
def test_the_bed_takes_every_branch(oracle, lmax, nq):
    """A condition on the inputs, read from the reference alone: rows with N = 0 for a cone in the mask, each couple viscous
    and capped at least five times, cones with one kind, both and neither within reach, a particle outside the group, and
    a centre with d = 0 as the reference and the kernel compute it, whose couple is not zero.  It also prints
    max |N - p_tot|S_n|| / N with friction off and on, with and without the ring contact on the axis (SPEC §2.24 records
    them; not a gate)."""
    import conic_roll_ref as KR
    s = K.sums(lmax, nq)
    x, _, tw, mask = K.bed(lmax)
    el, di, sg = (K.reference(lmax, nq, n) for n in ("elastic", "dissipative", "spring"))
    reach = {}
    for (i, c) in s:
        reach.setdefault(i, []).append(c)
    dead = sum(1 for k in s if di["N"][k] == 0.0)
    two = sum(len(v) >= 2 for v in reach.values())
    spot = lambda r: max(abs(r["N"][k] - r["NS"][k]) / r["N"][k] for k in r["N"] if r["N"][k] > 0 and k[0] != K.ON_AXIS)
    print(f"L={lmax} nq={nq}: {len(s)} (particle, cone) rows, {dead} with N = 0, {two} particles in reach of two cones or more; "
          f"branches elastic {KR.branch_counts(el['branch'])}, dissipative {KR.branch_counts(di['branch'])}; max |N - p_tot|S_n|| / N = "
          f"{spot(el):.3e} with friction off, {spot(di):.3e} with friction on, {spot(sg):.3e} with the springs; with the ring contact "
          f"on the axis {KR.load_gap(el):.3e}, {KR.load_gap(di):.3e}")
    for r in (el, di, sg):
        assert all(v >= 5 for v in KR.branch_counts(r["branch"]).values())
    assert dead >= 5 and two >= 20
    by_cone = {c: [k for k in s if k[1] == c and di["N"][k] > 0] for c in range(K.NK)}
    assert all(len(v) >= 1 for v in by_cone.values())           # every cone bears a load, bit 7 of the mask included
    for c, keys in by_cone.items():                             # ... and the kinds follow the cones
        for k in keys:
            br, bt = di["branch"][k]
            assert (br != KR.NONE) == bool(K.ROLL_KIND[c]) and (bt != KR.NONE) == bool(K.TWIST_KIND[c])
    both, one, none = K.ROLL_KIND & K.TWIST_KIND, K.ROLL_KIND ^ K.TWIST_KIND, ~(K.ROLL_KIND | K.TWIST_KIND)
    assert both.sum() == 3 and one.sum() == 3 and none.sum() == 2
    assert mask[K.OUTSIDE] == 2 and K.OUTSIDE not in reach and not di["couple"][K.OUTSIDE].any()
    assert K.foot_is_exact() == (0.0, 0.0) and reach[K.ON_AXIS] == [7] and di["d"][(K.ON_AXIS, 7)] == 0.0
    assert di["N"][(K.ON_AXIS, 7)] > 0 and di["branch"][(K.ON_AXIS, 7)] != (KR.NONE, KR.NONE) and di["couple"][K.ON_AXIS].any()
    assert sum(1 for i in reach if not tw[i, 3:].any()) >= 3
    assert spot(el) <= 0.05 and spot(sg) <= 0.2                 # a record, loosely bounded: SPEC §2.24 says what the gap is made of


# ---- 2. parity behind every instance and through both forms, off is off, deterministic ------------------------------------

@gpu
@pytest.mark.parametrize("lmax,nq", K.CONFIGS)
@pytest.mark.parametrize("name", ["elastic", "dissipative", "spring", "spring-look"])
def test_the_bed_matches_the_reference_and_the_force_keeps_its_bits(oracle, lmax, nq, name):
    """torque, M_ax and the other totals against the reference behind one instance of the contact kernel ("spring" and
    "spring-look" go through shstep_conic_contact_device); f and entries 0..3 of the rows (through their ordered totals) bit
    for bit those of the same pass with the kinds off; the rows are kept whether or not cone_out is asked for; set and zeroed
    again gives the bits of a context that never saw a coefficient; the same bits with "deterministic"."""
    ref = K.reference(lmax, nq, name)
    sp = _ctx(lmax, nq, name, roll=False)
    assert sp.rmax(0) == K.rmax(lmax) and not sp.has_conic_rolling
    plain = _pass(sp, lmax, name)                               # the kinds never set: the parent's pass
    sp.conic_rolling(K.MUR, K.GR)
    sp.conic_twisting(K.MUTW, K.GTW)
    assert sp.has_conic_rolling and sp.cone_reads_twists
    got = _pass(sp, lmax, name)
    nc = sp.cone_stats()
    noout = _pass(sp, lmax, name, want_out=False)
    sp.conic_rolling(0.0, 0.0)
    sp.conic_twisting(0.0, 0.0)
    assert not sp.has_conic_rolling
    back = _pass(sp, lmax, name)
    sp.close()
    sp = _ctx(lmax, nq, name, det=1)
    det = _pass(sp, lmax, name)
    sp.close()
    e = _errors(got, ref, plain)
    print(f"L={lmax} nq={nq} {name}: {nc} contacts, max|tau| {np.abs(ref['torque']).max():.4g} max|M| {np.abs(ref['couple']).max():.4g} "
          f"M_ax {ref['cone_out'][:, 4].tolist()} (without the couples {ref['max0'].tolist()}); rel err {e}")
    assert nc == ref["ncontacts"] > 40
    assert max(e.values()) <= TOL
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[2][:, :4], plain[2][:, :4])     # f, E_k and F_w: bit for bit
    moved = (got[1] != plain[1]).any(axis=1)
    assert moved.sum() >= 20 and np.array_equal(moved, ref["couple"].any(axis=1))                   # exactly the rows the reference moves
    assert moved[K.ON_AXIS] and not moved[K.OUTSIDE]
    changed = got[2][:, 4] != plain[2][:, 4]
    assert changed[[0, 1, 2, 3, 5, 7]].all() and not changed[[4, 6]].any()                           # the cones without a kind keep M_ax
    assert np.array_equal(noout[0], got[0]) and np.array_equal(noout[1], got[1]) and not noout[2].any()
    assert _same(back, plain)
    assert _same(det, got)


@gpu
def test_off_is_off_and_rows_of_an_earlier_call_or_another_nlocal_are_never_read(oracle):
    """The coefficients set and zeroed: bit for bit the pass of a context that never had them, and nothing reads twists.  A
    pass over fewer particles behind one over all of them, and a pass behind one whose masks were wider (a narrower group):
    bit for bit a fresh context's; nobody in the group: nothing is touched."""
    lmax, nq, name = 4, 10, "dissipative"
    fresh = _ctx(lmax, nq, roll=False)
    want = _pass(fresh, lmax)
    fresh.close()
    sp = _ctx(lmax, nq)
    sp.conic_rolling(0.0, 0.0)
    sp.conic_twisting(np.zeros(K.NK), np.zeros(K.NK))
    assert not sp.cone_reads_twists and not sp.has_dissipation
    assert _same(_pass(sp, lmax), want)
    sp.close()
    _, _, _, m0 = K.bed(lmax)
    narrow = m0.copy()
    narrow[1::2] = 2
    fresh = _ctx(lmax, nq, name)
    want_small = _pass(fresh, lmax, name, n=17)
    fresh.close()
    fresh = _ctx(lmax, nq, name)
    want_narrow = _pass(fresh, lmax, name, mask=narrow)
    fresh.close()
    sp = _ctx(lmax, nq, name)
    full = _pass(sp, lmax, name)
    assert max(_errors(full, K.reference(lmax, nq, name)).values()) <= TOL
    assert _same(_pass(sp, lmax, name, n=17), want_small) and want_small[1].any()
    assert _same(_pass(sp, lmax, name), full)
    assert _same(_pass(sp, lmax, name, mask=narrow), want_narrow) and not _same(want_narrow, full)
    none = _pass(sp, lmax, name, mask=np.full(NBED, 2, np.int32))     # nobody in the group: every mask is 0
    assert not none[0].any() and not none[1].any() and not none[2].any()
    sp.close()


# ---- 3. the physical cases ---------------------------------------------------------------------------------------------------

def _one_sphere(theta=np.pi / 6):
    """A unit sphere 0.7 from the wall of an oblique cone, 6 up its slant."""
    import cone_ref as Co
    import conic_history_cases as H
    co = Co.cone(H.APEX, H.AXIS, theta)
    return co, H.centre(co, 0.8, 6.0, 0.7), np.array([1.0, 0.0, 0.0, 0.0])


def _sphere_ctx(co, om, roll, twist):
    from dissipation_common import _wall_ctx
    from shpair import shapes
    sp = _wall_ctx([(0, shapes.sphere(1.0))], 10, rmax=[1.01])
    sp.set_cones([co], KN, EXPO)
    sp.cone_damping(3.0)
    sp.cone_rotation(om)
    if roll:
        sp.conic_rolling(*roll)
    if twist:
        sp.conic_twisting(*twist)
    return sp


@gpu
def test_a_carried_particle_feels_exactly_nothing(oracle):
    """omega_i = Omega_k a^ formed by the product the kernel forms, whatever the velocity: every bit of f, torque and cone_out
    is that of the pass with the kinds off; another omega_i moves the torque."""
    from test_gpu_conic_history import Pass
    co, x, q = _one_sphere()
    om = 1.7
    tw = np.concatenate([[0.3, -0.2, 0.1], om * co[3:6]])[None]
    off = _sphere_ctx(co, om, None, None)
    want = Pass(off, 1).go(x[None], q[None], tw, 0.0, old_call=True)
    off.close()
    sp = _sphere_ctx(co, om, (0.05, 3.0), (0.03, 2.0))
    got = Pass(sp, 1).go(x[None], q[None], tw, 0.0, old_call=True)
    assert want[0].any() and _same(got, want)
    tw[0, 3:] = 0.0                                              # at rest in the laboratory: the turning wall drags it
    got = Pass(sp, 1).go(x[None], q[None], tw, 0.0, old_call=True)
    assert np.array_equal(got[0], want[0]) and (got[1] != want[1]).any()
    sp.close()


@gpu
def test_a_sphere_at_rest_on_a_turning_cone_is_spun_about_the_normal_by_the_twisting_couple_alone(oracle):
    """omega_i = 0, Omega_k = 1.7, small gammas (both couples viscous): the couple is gamma_r Omega c g^ - gamma_tw Omega s n^.
    With rolling alone it has no part along n^, with twisting alone nothing else, to 1e-12 of gamma Omega; and over 20 steps
    of the run loop a frictionless sphere picks up angular momentum along -n^ with twisting on and none along n^ without."""
    import torch
    import cone_ref as Co
    import conic_roll_ref as KR
    from shpair.run import DeviceRun
    from test_gpu_conic_history import Pass
    co, x, q = _one_sphere()
    om, gr, gtw = 1.7, 1e-3, 2e-3
    nh = KR.normal(x, co)
    gen = Co.frame(co, Co.foot(x, co)[3])[0]
    tw = np.zeros((1, 6))
    couple = {}
    for label, roll, twist in (("off", None, None), ("rolling", (0.05, gr), None), ("twisting", None, (0.03, gtw)), ("both", (0.05, gr), (0.03, gtw))):
        sp = _sphere_ctx(co, om, roll, twist)
        couple[label] = Pass(sp, 1).go(x[None], q[None], tw, 0.0, old_call=True)[1][0]
        sp.close()
    Mr, Mt, Mb = (couple[k] - couple["off"] for k in ("rolling", "twisting", "both"))
    sc = max(gr, gtw) * om
    print(f"M rolling {Mr.tolist()} twisting {Mt.tolist()}; M_r.g {Mr @ gen:.6e} (gamma_r Omega c = {gr * om * co[6]:.6e}), "
          f"M_tw.n {Mt @ nh:.6e} (-gamma_tw Omega s = {-gtw * om * co[7]:.6e})")
    assert abs(Mr @ nh) <= 1e-12 * sc and abs(Mr @ gen - gr * om * co[6]) <= 1e-12 * sc and np.linalg.norm(Mr - (Mr @ gen) * gen) <= 1e-12 * sc
    assert abs(Mt @ nh + gtw * om * co[7]) <= 1e-12 * sc and np.linalg.norm(Mt - (Mt @ nh) * nh) <= 1e-12 * sc
    assert np.abs(Mb - Mr - Mt).max() <= 1e-12 * sc
    Ln = {}
    for label, extra in (("rolling", dict(conic_rolling=(0.05, 3.0))), ("twisting", dict(conic_twisting=(0.03, 2.0)))):
        sp = _sphere_ctx(co, om, None, None)
        r = DeviceRun(sp, x[None], q[None], np.zeros(1, np.int32), (-10, -10, -10), (10, 10, 10), (0, 0, 0), 0.5, dt=5e-4, **extra)
        r.run(20)
        torch.cuda.synchronize()
        L = r.L.cpu().numpy()[0]
        n1 = KR.normal(r.x[0].cpu().numpy(), co)
        Ln[label] = (L @ n1, np.linalg.norm(L - (L @ n1) * n1))
        assert sp.cone_stats() == 1
        sp.close()
    print(f"after 20 steps: L.n and |L - (L.n) n| with rolling alone {Ln['rolling']}, with twisting alone {Ln['twisting']}")
    assert Ln["twisting"][0] < 0 and Ln["twisting"][1] <= 1e-3 * abs(Ln["twisting"][0])   # (n^ turns by what the centre moves in 20 steps)
    assert Ln["rolling"][1] > 0 and abs(Ln["rolling"][0]) <= 1e-3 * Ln["rolling"][1]


@gpu
def test_a_spinning_sphere_in_a_hopper_at_rest_loses_its_spin_with_the_couples_and_keeps_it_without(oracle):
    """A frictionless unit sphere pressed into the wall of a hopper at rest, spinning about an oblique axis, 40 steps: |L|
    falls with both couples on, monotonically, and keeps its value to 1e-9 with them off (a sphere's normal wrench has no
    moment about its centre)."""
    import torch
    from dissipation_common import dev
    from shpair.run import DeviceRun
    co, x, q = _one_sphere()
    hist = {}
    for label, extra in (("off", {}), ("on", dict(conic_rolling=(0.05, 3.0), conic_twisting=(0.03, 2.0)))):
        sp = _sphere_ctx(co, 0.0, None, None)
        r = DeviceRun(sp, x[None], q[None], np.zeros(1, np.int32), (-10, -10, -10), (10, 10, 10), (0, 0, 0), 0.5, dt=5e-4, **extra)
        _, _, inertia = sp.body(0)
        r.L[:] = dev(np.array([[2.0, 5.0, -3.0]]) * inertia[0])
        norms = [float(torch.linalg.norm(r.L[0]))]
        for _ in range(4):
            r.run(10)
            norms.append(float(torch.linalg.norm(r.L[0])))
        hist[label] = norms
        assert sp.cone_stats() == 1
        sp.close()
    print(f"|L| every 10 steps: off {hist['off']}, on {hist['on']}")
    assert max(abs(v - hist["off"][0]) for v in hist["off"]) <= 1e-9 * hist["off"][0]
    assert all(b < a for a, b in zip(hist["on"], hist["on"][1:])) and hist["on"][-1] < 0.99 * hist["on"][0]


# ---- 4. the run loops --------------------------------------------------------------------------------------------------------

def _spinner(mode, nsteps=8, roll=True, det=1):
    """A near-sphere (L = 4, amplitude 0.02) resting on the wall of a hopper along z that turns at Omega = 0.8, spinning
    about an oblique axis, under gravity, with damping, friction, a spring and both couples."""
    import torch
    import cone_ref as Co
    from dissipation_common import _wall_ctx, dev
    from oracle import oracle as O
    from shpair import shapes
    from shpair.run import DeviceRun
    anm = shapes.random_shape(4, 5, amp=0.02)
    th = np.pi / 6
    co = Co.cone([4.0, 4.0, 0.5], [0.0, 0.0, 1.0], th)
    s, h = 6.0, 0.97
    t, d = np.cos(th) * s + np.sin(th) * h, np.sin(th) * s - np.cos(th) * h
    x = np.array([[4.0 + d * np.cos(0.3), 4.0 + d * np.sin(0.3), 0.5 + t]])
    sp = _wall_ctx([(4, anm)], 10, kn=2000.0, deterministic=det)
    extra = dict(conic_rolling=(0.05, 3.0), conic_twisting=(0.03, 2.0)) if roll else {}
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.5, dt=5e-4,
                  gravity=(0.0, 0.0, -9.81), cones=([co], 2000.0, 1.25), cone_damping=20.0, cone_friction=(0.4, 30.0), cone_rotation=0.8,
                  conic_spring=5e3, **extra)
    assert sp.has_conic_rolling == roll and sp.has_conic_history
    _, _, inertia = sp.body(0)
    r.L[:] = dev(np.array([[2.0, 5.0, -3.0]]) * inertia[0])
    r.force()
    if mode == "python":
        r.run(nsteps)
    else:
        r.run_native(nsteps, use_graph=(mode == "graph"))
    torch.cuda.synchronize()
    state = [t.cpu().numpy().copy() for t in (r.x[:1], r.v, r.q[:1], r.L, r.f[:1], r.tq[:1])] + [r.cone_history()]
    n = sp.cone_stats()
    sp.close()
    return state, n


@gpu
def test_the_three_loops_agree_bitwise_over_eight_steps(oracle):
    ref, n = _spinner("python")
    off, _ = _spinner("python", roll=False)
    print(f"spinner: contacts {n}, L {ref[3].tolist()} (without the couples {off[3].tolist()})")
    assert n == 1 and not np.array_equal(ref[3], off[3])
    for mode in ("plain", "graph"):
        got, _ = _spinner(mode)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), mode


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------

@gpu
def test_refusals_by_their_messages_and_both_forms_carry_the_couples(oracle):
    import ctypes
    import torch
    from shpair import mrank
    from shpair.capi import HaloArrays, HaloRunParams, ShPairError
    from test_gpu_conic_history import Pass
    lmax, nq = 4, 10
    sp = _ctx(lmax, nq)
    x, quat, tw, m0 = K.bed(lmax)
    n = 17
    P = Pass(sp, n)
    xd, qd, m = (torch.from_numpy(np.ascontiguousarray(a[:n])).cuda() for a in (x, quat, m0))
    f, tq = (torch.zeros(n, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
    args = (n, xd.data_ptr(), qd.data_ptr(), P.sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    with pytest.raises(ShPairError, match="cone rolling or twisting resistance: null twist pointer") as e:   # a null twist, either form
        sp.cone_force_device(*args, twist=None)
    assert e.value.code == -1
    with pytest.raises(ShPairError, match="cone rolling or twisting resistance: null twist pointer"):
        sp.conic_contact_device(*args, None, 1e-3)
    torch.cuda.synchronize()
    assert not f.any() and not tq.any()
    a = P.go(x[:n], quat[:n], tw[:n], 0.0, mask=m0[:n], old_call=True)
    b = P.go(x[:n], quat[:n], tw[:n], 0.0, mask=m0[:n])          # a look: the couples have no state
    c = P.go(x[:n], quat[:n], tw[:n], 1e-3, mask=m0[:n])
    assert _same(a, b) and _same(a, c) and (a[1] != P.go(x[:n], quat[:n], np.zeros((n, 6)), 0.0, mask=m0[:n])[1]).any()
    # either ledger, in either order: a kind is a cone coefficient like every other (on.any(), the words of SPEC §2.22's rule)
    sp.set_cones(K.cones(), KN, EXPO)                             # resets all four, and Omega
    assert not sp.has_conic_rolling and not sp.cone_reads_twists
    for kind in (sp.conic_rolling, sp.conic_twisting):            # a kind alone: nothing else is set, the cones are at rest
        kind(np.where(np.arange(K.NK) == 6, 0.05, 0.0), 3.0)
        assert sp.has_conic_rolling
        for switch, word, flag in ((sp.set_energy_ledger, "energy", "ledger_on"), (sp.set_shell_ledger, "shell", "shell_ledger_on")):
            with pytest.raises(ShPairError, match=f"{word} ledger: a cone damping or friction coefficient or a cone rotation is set and the "
                                                  "ledger keeps no cone entries") as e:
                switch(True)
            assert e.value.code == -4 and not getattr(sp, flag)
        kind(0.0, 0.0)
    assert not sp.has_conic_rolling
    for switch, word in ((sp.set_energy_ledger, "energy"), (sp.set_shell_ledger, "shell")):
        switch(True)
        with pytest.raises(ShPairError, match=f"cone rolling resistance: the {word} ledger is on and keeps no cone entries") as e:
            sp.conic_rolling(0.05, 3.0)
        assert e.value.code == -4 and not sp.has_conic_rolling
        with pytest.raises(ShPairError, match=f"cone twisting resistance: the {word} ledger is on and keeps no cone entries"):
            sp.conic_twisting(0.03, 2.0)
        sp.conic_rolling(0.05, 0.0)                               # no kind: allowed
        assert not sp.has_conic_rolling
        switch(False)
    # a wrong ncone, negative or non-finite values
    with pytest.raises(ShPairError, match=r"cone twisting resistance: 3 coefficients for 8 cones \(call it after shstep_set_cones\)") as e:
        sp.conic_twisting([0.1, 0.1, 0.1], [1.0, 1.0, 1.0])
    assert e.value.code == -1
    one = (ctypes.c_double * 8)(*([1.0] * 8))
    with pytest.raises(ShPairError, match="cone rolling resistance: null array pointer"):
        sp._chk(sp._lib.shstep_set_rolling_con(sp._h, 8, None, one))
    v = np.full(8, 0.1)
    bad = lambda k, val: np.where(np.arange(8) == k, val, v)
    with pytest.raises(ShPairError, match=r"cone 1: rolling coefficient mu_r -0.5 must be finite and >= 0") as e:
        sp.conic_rolling(bad(1, -0.5), v)
    assert e.value.code == -1
    with pytest.raises(ShPairError, match=r"cone 0: twisting coefficient gamma_tw nan must be finite"):
        sp.conic_twisting(v, bad(0, np.nan))
    with pytest.raises(ShPairError, match=r"cone 7: rolling coefficient gamma_r inf must be finite"):
        sp.conic_rolling(v, bad(7, np.inf))
    assert not sp.has_conic_rolling and not sp.cone_reads_twists  # a refused call changes nothing
    other = type(sp)(0)
    with pytest.raises(ShPairError, match=r"cone rolling resistance: 1 coefficients for 0 cones \(call it after shstep_set_cones\)"):
        other._chk(other._lib.shstep_set_rolling_con(other._h, 1, one, one))
    other.close()
    # several ranks: the loop over all ranks and its Python driver refuse any cone
    sp.conic_twisting(0.03, 2.0)
    assert sp.has_conic_rolling
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), (0, 0, 0), (20, 20, 20), (0, 0, 0), 0.2)
    stand_in = type("R", (), dict(sp=sp, a=None, stream=None, halo=None))()
    with pytest.raises(ShPairError, match="conical walls are single-rank") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -4
    with pytest.raises(ShPairError, match="conical walls are single-rank") as e:
        mrank.RankRun.force(stand_in)
    assert e.value.code == -4
    halo.close()
    sp.close()
