"""GPU tests of the rolling and twisting resistance at cylindrical walls of docs/SPEC.md §2.21 (csrc/cyl_roll_kernels.hpp,
through the C ABI of include/shstep.h) against tests/cyl_roll_ref.py at the bar of tests/test_gpu_wall_roll.py and
tests/test_gpu_cyl_history.py, 1e-9: parity on a bed of 301 particles inside eight cylinders behind every instance of the
contact kernel, one cylinder and two crossing ones, stale rows, the axis of a narrow cylinder, off is off, "deterministic",
the shell ledger, the three run loops and the closure of the ledger.

The condition on the inputs (test_the_bed_takes_every_branch) needs no GPU: it reads the reference alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cyl_roll_cases as K   # noqa: E402

gpu = pytest.mark.gpu
TOL = 1e-9
NBED, KN, EXPO = K.NBED, K.KN, K.EXPO


def _ctx(lmax, nq, name="elastic", det=0, roll=True, cyl_ids=None, ledger_first=False):
    """A context with the bed's cylinders (or a subset) and the coefficients of a contact-kernel instance."""
    from dissipation_common import _wall_ctx
    ids = list(range(K.NCYL)) if cyl_ids is None else list(cyl_ids)
    coef, _, ledger = K.INSTANCES[name]
    sp = _wall_ctx([(lmax, K.shape(lmax))], nq, kn=KN, expo=EXPO, deterministic=det)
    if ledger:
        sp.set_shell_ledger(True)
        if ledger_first:
            sp.set_energy_ledger(True)
    sp.set_cylinders(K.cylinders()[ids], KN, EXPO)
    sp.cylinder_rotation(K.OMEGA[ids])
    if coef is not None:
        sp.cylinder_damping(coef["gamma"][ids])
        sp.cylinder_friction(coef["mu"][ids], coef["gt"][ids])
        if "kt" in coef:
            sp.set_cyl_tangential_spring(coef["kt"][ids])
    if roll:
        sp.cylinder_rolling(K.MUR[ids], K.GR[ids])
        sp.cylinder_twisting(K.MUTW[ids], K.GTW[ids])
    if ledger and not ledger_first:
        sp.set_energy_ledger(True)
    return sp


def _pass(sp, name="elastic", n=NBED, mask=None, want_out=True, tw=None):
    """One cylinder pass over the first n particles of the bed on fresh arrays: f, torque, cyl_out."""
    from test_gpu_cyl_history import Pass
    x, quat, tw0, m0 = K.bed()
    tw = tw0 if tw is None else tw
    dt = K.INSTANCES[name][1]
    got = Pass(sp, n).go(x[:n], quat[:n], tw[:n], dt or 0.0, mask=(m0 if mask is None else mask)[:n], old_call=dt is None, want_out=want_out)
    sp.synchronize()
    return got


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _errors(got, ref, plain=None):
    """Relative errors of torque, cyl_out (M_ax against the torque scale) and, given the same pass with rolling off, of the
    couple alone against max|M|."""
    scale = np.abs(ref["f"]).max()
    tscale = max(scale, np.abs(ref["torque"]).max())
    ro = ref["cyl_out"]
    e = dict(f=np.abs(got[0] - ref["f"]).max() / scale, torque=np.abs(got[1] - ref["torque"]).max() / tscale,
             wall=np.abs(got[2][:, :4] - ro[:, :4]).max() / np.abs(ro[:, :4]).max(),
             M_ax=np.abs(got[2][:, 4] - ro[:, 4]).max() / max(tscale, np.abs(ro[:, 4]).max()))
    if plain is not None:
        e["couple"] = np.abs((got[1] - plain[1]) - ref["couple"]).max() / tscale
    return e


# ---- 1. the inputs (no GPU) ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lmax,nq", K.CONFIGS)
def test_the_bed_takes_every_branch(oracle, lmax, nq):
    """A condition on the inputs, read from the reference alone: at least five (particle, cylinder) viscous and capped of
    both kinds, within reach with V <= 0, clamped, and particles in reach of two cylinders; bit 7 of the mask is used,
    particles are outside the group and at rest.  It also prints max |N - p_tot|S_n|| / N with friction off and on (SPEC
    §2.21 records both)."""
    import cyl_roll_ref as CR
    s = K.sums(lmax, nq)
    x, _, tw, mask = K.bed()
    assert K.rmax(lmax) < 1.35
    el, di = K.reference(lmax, nq, "elastic"), K.reference(lmax, nq, "dissipative")
    reach = {}
    for (i, c) in s:
        reach.setdefault(i, []).append(c)
    dry = sum(1 for v in s.values() if not v[0] > 0)
    clamped = sum(1 for k in s if s[k][0] > 0 and di["NS"][k] == 0.0)
    two = sum(len(v) >= 2 for v in reach.values())
    print(f"L={lmax} nq={nq}: {len(s)} (particle, cylinder) rows, {dry} within reach with V <= 0, {clamped} clamped, {two} particles in "
          f"reach of two cylinders or more; branches elastic {CR.branch_counts(el['branch'])}, dissipative {CR.branch_counts(di['branch'])}; "
          f"max |N - p_tot|S_n|| / N = {CR.load_gap(el):.3e} with friction off, {CR.load_gap(di):.3e} with friction on")
    for r in (el, di):
        assert all(v >= 5 for v in CR.branch_counts(r["branch"]).values())
    assert dry >= 5 and clamped >= 5 and two >= 5
    assert {c for v in reach.values() for c in v} == {0, 1, 7}
    assert all(di["N"][k] == 0.0 and not di["couple"][k[0]].any() for k in s if len(reach[k[0]]) == 1 and di["NS"][k] == 0.0)
    assert (mask == 2).sum() >= 20 and not any(mask[i] == 2 for i in reach)
    assert sum(1 for i in reach if not tw[i, 3:].any()) >= 5
    assert np.ptp(np.log10([np.linalg.norm(tw[i, 3:]) for i in reach if tw[i, 3:].any()])) >= 3.0
    assert CR.load_gap(el) <= 0.05 and CR.load_gap(di) <= 0.2    # a record, loosely bounded: SPEC §2.21 says what the gap is made of


# ---- 2. parity behind every instance, off is off, deterministic -----------------------------------------------------------

@gpu
@pytest.mark.parametrize("lmax,nq", K.CONFIGS)
@pytest.mark.parametrize("name", ["elastic", "dissipative", "spring", "spring-look"])
def test_the_bed_matches_the_reference_and_the_force_keeps_its_bits(oracle, lmax, nq, name):
    """torque, M_ax and the other totals against the reference behind one instance of the contact kernel; f and entries 0..3
    of the rows (through their ordered totals) bit for bit those of the same pass with rolling off; the rows are kept whether
    or not cyl_out is asked for; set and zeroed again gives the bits of a context that never saw a coefficient; the same
    bits with "deterministic"."""
    ref = K.reference(lmax, nq, name)
    sp = _ctx(lmax, nq, name, roll=False)
    assert sp.rmax(0) == K.rmax(lmax) and not sp.has_cyl_rolling
    plain = _pass(sp, name)                                     # rolling never set: the parent's pass
    sp.cylinder_rolling(K.MUR, K.GR)
    sp.cylinder_twisting(K.MUTW, K.GTW)
    assert sp.has_cyl_rolling and sp.cylinder_reads_twists
    if name.startswith("spring"):
        sp.reset_cyl_history()                                  # every pass here starts from nothing live, as the reference
    got = _pass(sp, name)
    nc = sp.cylinder_stats()
    if name.startswith("spring"):
        sp.reset_cyl_history()
    noout = _pass(sp, name, want_out=False)
    sp.cylinder_rolling(0.0, 0.0)
    sp.cylinder_twisting(0.0, 0.0)
    assert not sp.has_cyl_rolling
    if name.startswith("spring"):
        sp.reset_cyl_history()
    back = _pass(sp, name)
    sp.close()
    sp = _ctx(lmax, nq, name, det=1)
    det = _pass(sp, name)
    sp.close()
    e = _errors(got, ref, plain)
    print(f"L={lmax} nq={nq} {name}: {nc} contacts, max|tau| {np.abs(ref['torque']).max():.4g} max|M| {np.abs(ref['couple']).max():.4g} "
          f"M_ax {ref['cyl_out'][:, 4].tolist()} (without the couples {ref['max0'].tolist()}); rel err {e}")
    assert nc == ref["ncontacts"] > 0
    assert max(e.values()) <= TOL
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[2][:, :4], plain[2][:, :4])     # f, E_c and F_w: bit for bit
    moved = (got[1] != plain[1]).any(axis=1)
    assert moved.sum() >= 20 and np.array_equal(moved, ref["couple"].any(axis=1))                   # exactly the rows the reference moves
    assert (got[2][:, 4] != plain[2][:, 4]).sum() >= 2 and np.array_equal(got[2][2:7], plain[2][2:7])
    assert np.array_equal(noout[0], got[0]) and np.array_equal(noout[1], got[1]) and not noout[2].any()
    assert _same(back, plain)
    assert _same(det, got)


@gpu
def test_off_is_off_against_a_fresh_context(oracle):
    """The coefficients set and zeroed: bit for bit the pass of a context that never had them, and nothing reads twists."""
    lmax, nq = 4, 10
    fresh = _ctx(lmax, nq, roll=False)
    want = _pass(fresh)
    fresh.close()
    sp = _ctx(lmax, nq)
    sp.cylinder_rolling(0.0, 0.0)
    sp.cylinder_twisting(np.zeros(K.NCYL), np.zeros(K.NCYL))
    assert not sp.cylinder_reads_twists and not sp.has_dissipation
    assert _same(_pass(sp), want)
    sp.close()


# ---- 3. one cylinder, two crossing ones, the rows of single particles ------------------------------------------------------

@gpu
@pytest.mark.parametrize("ids", [(0,), (0, 1), (7, 1, 0)])
def test_one_cylinder_two_crossing_ones_and_another_order(oracle, ids):
    lmax, nq = 6, 16
    ref = K.reference(lmax, nq, "dissipative", cyl_ids=ids)
    sp = _ctx(lmax, nq, "dissipative", cyl_ids=ids)
    got = _pass(sp, "dissipative")
    e = _errors(got, ref)
    print(f"cylinders {ids}: M_ax {ref['cyl_out'][:, 4].tolist()}, rel err {e}")
    assert max(e.values()) <= TOL and sp.cylinder_stats() == ref["ncontacts"]
    # the rows of single particles, those in reach of the most cylinders first, by a one-particle group
    x, _, _, m0 = K.bed()
    reach = (np.array([[ref["N"].get((i, c), -1.0) >= 0 for c in range(len(ids))] for i in range(NBED)])).sum(axis=1)
    reach = reach * ref["couple"].any(axis=1)                   # ... among those the couples move
    for i in np.argsort(-reach, kind="stable")[:3]:
        assert reach[i] >= min(2, len(ids))
        m = np.full(NBED, 2, np.int32)
        m[i] = 1
        one = K.reference(lmax, nq, "dissipative", cyl_ids=ids, mask=m)
        g1 = _pass(sp, "dissipative", mask=m)
        e1 = _errors(g1, one)
        print(f"  particle {i} in reach of {reach[i]}: rows' M_ax {one['cyl_out'][:, 4].tolist()}, rel err {e1}")
        assert max(e1.values()) <= TOL and not np.delete(g1[1], i, axis=0).any()
    sp.close()


# ---- 4. stale rows ---------------------------------------------------------------------------------------------------------

@gpu
def test_rows_of_an_earlier_call_and_of_another_nlocal_are_never_read(oracle):
    """A pass over fewer particles behind one over all of them, and a pass behind one whose masks were wider (a narrower
    group; then the same group with the wide cylinders only, whose mask is empty): bit for bit a fresh context's."""
    lmax, nq, name = 4, 10, "dissipative"
    _, _, _, m0 = K.bed()
    narrow = m0.copy()
    narrow[1::2] = 2
    fresh = _ctx(lmax, nq, name)
    want_small, want_narrow = _pass(fresh, name, n=120), None
    fresh.close()
    fresh = _ctx(lmax, nq, name)
    want_narrow = _pass(fresh, name, mask=narrow)
    fresh.close()
    sp = _ctx(lmax, nq, name)
    full = _pass(sp, name)
    assert _same(_pass(sp, name, n=120), want_small)
    assert _same(_pass(sp, name), full)
    assert _same(_pass(sp, name, mask=narrow), want_narrow)
    ref = K.reference(lmax, nq, name, mask=narrow)
    assert max(_errors(want_narrow, ref).values()) <= TOL
    none = _pass(sp, name, mask=np.full(NBED, 2, np.int32))     # nobody in the group: every mask is 0, nothing is touched
    assert not none[0].any() and not none[1].any() and not none[2].any()
    sp.close()


# ---- 5. the axis of a narrow cylinder, a particle carried round -------------------------------------------------------------

@gpu
def test_a_centre_on_the_axis_takes_the_frame_rule_and_a_carried_particle_feels_nothing(oracle):
    """tests/cyl_history_cases.py's narrow cylinder (Rc < R_i, a state the cylinder tests accept): particle 0 sits exactly on
    the axis, d = 0 as computed, and c^ is the e1 of the frame rule.  Then omega_i = Omega_c a^ formed by the same product:
    the torque keeps the bits of the pass with rolling off."""
    import cyl_history_cases as H
    import cyl_ref as Cy
    import cyl_roll_ref as CR
    from dissipation_common import _wall_ctx
    from test_gpu_cyl_history import Pass
    from oracle import oracle as O
    lmax, nq = 4, 10
    from shpair import bed, shapes
    anm = shapes.random_shape(lmax, 40 + lmax, amp=0.1)
    rm = O.shape_rmax(lmax, anm)
    cyls, _, _, _, _, place = H.geometry("axis", rm)
    rng = np.random.default_rng(77)
    x = place(rng)
    n = len(x)
    assert Cy.foot(x[0], cyls[0])[1] == 0.0
    quat = bed.random_quaternions(n, rng)
    tw = rng.normal(size=(n, 6))
    om = 0.6
    s = CR.reach_sums([(lmax, anm, rm)], nq, x, quat, np.zeros(n, int), cyls)
    ref = CR.cyl_roll(s, n, x, tw, cyls, KN, EXPO, 0.05, 4.0, 0.03, 2.5, gamma=3.0, mu=0.5, gt=2.0, omega=om)
    assert ref["N"][(0, 0)] > 0 and ref["couple"][0].any()
    sp = _wall_ctx([(lmax, anm)], nq, kn=KN, expo=EXPO)
    sp.set_cylinders(cyls, KN, EXPO)
    sp.cylinder_damping(3.0)
    sp.cylinder_friction(0.5, 2.0)
    sp.cylinder_rotation(om)
    P = Pass(sp, n)
    plain = P.go(x, quat, tw, 0.0, old_call=True)
    sp.cylinder_rolling(0.05, 4.0)
    sp.cylinder_twisting(0.03, 2.5)
    got = P.go(x, quat, tw, 0.0, old_call=True)
    e = _errors(got, ref, plain)
    print(f"axis: N of the particle on the axis {ref['N'][(0, 0)]:.4g}, its couple {ref['couple'][0].tolist()}; rel err {e}")
    assert max(e.values()) <= TOL
    carried = tw.copy()
    carried[:, 3:] = om * cyls[0][3:6]                          # the product the kernel forms
    sp.cylinder_rolling(0.0, 0.0)
    sp.cylinder_twisting(0.0, 0.0)
    plain_c = P.go(x, quat, carried, 0.0, old_call=True)
    sp.cylinder_rolling(0.05, 4.0)
    sp.cylinder_twisting(0.03, 2.5)
    got_c = P.go(x, quat, carried, 0.0, old_call=True)
    assert _same(got_c, plain_c)
    sp.close()


# ---- 6. the shell ledger -----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("lmax,nq", K.CONFIGS)
@pytest.mark.parametrize("name", ["ledger-elastic", "ledger-dissipative", "ledger-spring"])
def test_the_couples_powers_go_into_the_shell_ledger(oracle, lmax, nq, name):
    """Both ledgers on: behind the elastic instance the roll kernel is the writer of the power rows, behind a LEDGER twin it
    adds to them.  Per-cylinder entries and totals at the bar; the pass keeps the bits it has with both ledgers off; the
    same ledger bits with "deterministic" and with the energy ledger switched on first; a fold folds once."""
    import shell_ledger_ref as SL
    ref = K.reference(lmax, nq, name)
    per, tot = SL.shell_fold(ref["P"], K.DT)
    per0, _ = SL.shell_fold(ref["P0"], K.DT)
    off = _ctx(lmax, nq, name.replace("ledger-", ""))
    want = _pass(off, name)
    off.close()
    res = []
    for det, first in ((0, False), (1, True)):
        sp = _ctx(lmax, nq, name, det=det, ledger_first=first)
        got = _pass(sp, name)
        sp.ledger_fold_device(K.DT)
        t, p = sp.shell_ledger()
        sp.ledger_fold_device(K.DT)                             # nothing fresh
        t2, p2 = sp.shell_ledger()
        assert np.array_equal(t, t2) and np.array_equal(p, p2)
        assert _same(got, want)
        res.append((t, p))
        sp.close()
    (t, p), (t1, p1) = res
    scale = np.abs(per).max()
    e_per, e_tot = np.abs(p - per).max() / scale, np.abs(t - tot).max() / scale
    print(f"L={lmax} nq={nq} {name}: per cylinder {per[[0, 1, 7]].tolist()} (without the couples {per0[[0, 1, 7]].tolist()}), "
          f"rel err {e_per:.1e} totals {e_tot:.1e}")
    assert max(e_per, e_tot) <= TOL
    assert (per[[0, 1, 7], 1] > per0[[0, 1, 7], 1]).all() and per[0, 2] != per0[0, 2] and per[1, 2] == per0[1, 2]   # cylinder 1 stands still
    assert not p[2:7].any()
    assert np.array_equal(t, t1) and np.array_equal(p, p1)


# ---- 7. refusals and the look ------------------------------------------------------------------------------------------------

@gpu
def test_refusals_and_both_forms_carry_the_couples(oracle):
    from shpair.capi import ShPairError
    from test_gpu_cyl_history import Pass
    import torch
    lmax, nq = 4, 10
    sp = _ctx(lmax, nq)
    x, quat, tw, m0 = K.bed()
    n = 40
    P = Pass(sp, n)
    xd, qd, m = (torch.from_numpy(np.ascontiguousarray(a[:n])).cuda() for a in (x, quat, m0))
    f, tq = (torch.zeros(n, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
    args = (n, xd.data_ptr(), qd.data_ptr(), P.sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr())
    with pytest.raises(ShPairError, match="cylinder rolling or twisting resistance: null twist pointer") as e:
        sp.cylinder_force_device(*args, twist=None)
    assert e.value.code == -1
    with pytest.raises(ShPairError, match="cylinder rolling or twisting resistance: null twist pointer"):
        sp.cyl_contact_device(*args, None, 1e-3)
    assert not f.any() and not tq.any()
    a = P.go(x[:n], quat[:n], tw[:n], 0.0, mask=m0[:n], old_call=True)
    b = P.go(x[:n], quat[:n], tw[:n], 0.0, mask=m0[:n])          # a look: the couples have no state
    c = P.go(x[:n], quat[:n], tw[:n], 1e-3, mask=m0[:n])
    assert _same(a, b) and _same(a, c)
    ref = K.reference(lmax, nq, n=n)
    assert ref["couple"].any() and max(_errors(a, ref).values()) <= TOL
    sp.close()


# ---- 8. the run loops ----------------------------------------------------------------------------------------------------------

def _spinner(mode, nsteps=8, roll=True, det=1):
    """A near-sphere (L = 4, amplitude 0.02) resting on the shell of a horizontal drum that turns at Omega = 0.8, spinning
    about an oblique axis, under gravity, with damping, friction and both couples; both ledgers on."""
    import torch
    from dissipation_common import _wall_ctx, dev
    from oracle import oracle as O
    from shpair import shapes
    from shpair.run import DeviceRun
    anm = shapes.random_shape(4, 5, amp=0.02)
    rm = O.shape_rmax(4, anm)
    Rc = 3.0
    cyl = np.array([4.0, 4.0, 4.0, 0.0, 1.0, 0.0, Rc])
    x = np.array([[4.0 + 0.3, 4.0, 4.0 - np.sqrt((Rc - 0.97) ** 2 - 0.09)]])
    sp = _wall_ctx([(4, anm)], 10, kn=2000.0, deterministic=det)
    extra = dict(cylinder_rolling=(0.05, 3.0), cylinder_twisting=(0.03, 2.0)) if roll else {}
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.5, dt=5e-4,
                  gravity=(0.0, 0.0, -9.81), ledger=True, shell_ledger=True, cylinders=([cyl], 2000.0, 1.25), cylinder_damping=20.0,
                  cylinder_friction=(0.4, 30.0), cylinder_rotation=0.8, **extra)
    _, _, inertia = sp.body(0)
    r.L[:] = dev(np.array([[2.0, 5.0, -3.0]]) * inertia[0])
    r.force()
    if mode == "python":
        r.run(nsteps)
    else:
        r.run_native(nsteps, use_graph=(mode == "graph"))
    torch.cuda.synchronize()
    state = [t.cpu().numpy().copy() for t in (r.x[:1], r.v, r.q[:1], r.L, r.f[:1], r.tq[:1])]
    led = r.shell_ledger()
    n = sp.cylinder_stats()
    sp.close()
    return state, led, n


@gpu
def test_the_three_loops_agree_bitwise_over_eight_steps(oracle):
    ref, led, n = _spinner("python")
    off, led0, _ = _spinner("python", roll=False)
    print(f"spinner: contacts {n}, L {ref[3].tolist()} (without the couples {off[3].tolist()}), shell ledger {led}")
    assert n == 1 and led["friction"] > 0 and led["friction"] != led0["friction"] and not np.array_equal(ref[3], off[3])
    for mode in ("plain", "graph"):
        got, l2, _ = _spinner(mode)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), mode
        assert all(l2[k] == led[k] for k in ("damping", "friction", "work")) and np.array_equal(l2["per_cylinder"], led["per_cylinder"])


def _throw(k, resist=True):
    """tests/shell_ledger_ref.py's THROW (a unit sphere thrown obliquely at the shell of a turning drum, with damping and
    friction) with both couples on, through shstep_run_device with graph replay at dt / k."""
    import torch
    import cyl_roll_ref as CR
    from dissipation_common import _wall_ctx, dev
    from shell_ledger_ref import THROW as c
    from shpair import shapes
    from shpair.run import DeviceRun
    sp = _wall_ctx([(0, shapes.sphere(1.0))], c["nq"], kn=c["kn"], expo=c["m"], rmax=[1.01], deterministic=1)
    extra = dict(cylinder_damping=c["gamma"], cylinder_friction=(c["mu"], c["gt"]), cylinder_rolling=CR.THROW_ROLL,
                 cylinder_twisting=CR.THROW_TWIST) if resist else {}
    r = DeviceRun(sp, np.array([c["x0"]]), np.array([[1.0, 0, 0, 0]]), np.zeros(1, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.5,
                  dt=c["dt"] / k, ledger=True, shell_ledger=True, cylinders=([np.array(c["cyl"])], c["kn"], c["m"]),
                  cylinder_rotation=c["omega"], check=False, **extra)
    _, _, inertia = sp.body(0)
    r.v[:] = dev(np.array([c["v0"]]))
    r.L[:] = dev(np.array([c["w0"]]) * inertia[0])
    r.force()
    e0 = r.energies()
    r.run_native(c["nsteps"] * k, use_graph=True)
    torch.cuda.synchronize()
    e1, led = r.energies(), r.shell_ledger()
    d = float(np.hypot(r.x[0, 0].item() - 4.0, r.x[0, 2].item() - 4.0))
    sp.close()
    return e0[1] + e0[2], e1[1] + e1[2], led, c["Rc"] - d


@gpu
def test_the_balance_of_a_thrown_sphere_closes_to_first_order_in_dt_with_the_couples_on(oracle):
    """|Delta E_mech - W_shell + D_shell| at dt and dt / 2 against the bar of tests/test_gpu_shell_ledger.py's closure test:
    the elastic run's residual is at most a tenth of it, and halving dt brings it below 0.75 of itself.  The reference's own
    trajectory (tests/test_cyl_roll_ref.py) predicts R = 7.023e-2 / 3.450e-2, ratio 0.491.
    Measured on an MI355X: R = 7.023e-2 at dt and 3.450e-2 at dt / 2 (ratio 0.491), the elastic runs' 2.113e-3 and 5.569e-5;
    D_d 0.2528, D_f 21.507, W 22.846 at dt."""
    R, R0 = [], []
    for k in (1, 2):
        E0, E1, led, h = _throw(k)
        e0, e1, led0, h0 = _throw(k, resist=False)
        R.append(abs(E1 - E0 - (led["work"] - led["damping"] - led["friction"])))
        R0.append(abs(e1 - e0))
        print(f"dt/{k}: E0 {E0:.6f} E1 {E1:.6f} D_d {led['damping']:.6f} D_f {led['friction']:.6f} W {led['work']:.6f} R {R[-1]:.3e} "
              f"elastic R0 {R0[-1]:.3e}, final h {h:.3f}")
        assert h > 1.01 and h0 > 1.01 and abs(E1 - E0) > 0.5
        assert led["damping"] > 0 and led["friction"] > 0
        assert not any(led0[t] for t in ("damping", "friction", "work"))
    print(f"R(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert R0[0] <= 0.1 * R[0] and R0[1] <= 0.1 * R[1]
    assert R[1] <= 0.75 * R[0]
