"""The run loops against the whole-step reference with cylinders on (docs/SPEC.md §6, "Order of a step with every model
on", the cylinder halves of items 11 and 13): the recorded scene tests/golden/traj_drum.npz — a periodic drum that
rotates, with damping, friction, springs, rolling and twisting at its shell, a plain-friction cylinder and an elastic one
across it, a rising chord plane, every pair model, both ledgers, frozen rows, rebuilds with wraps — through
DeviceRun.step, run_native plain and replayed from graphs, with the ledgers off, and across a restart.  The bars are the
fixture's: 10 x the reference's own deviation under a 1e-12 relative perturbation of every integral and sum
(tests/golden/make_traj_drum.py); every test prints measured error against bar.  Reads the fixture and test modules only:
no oracle call."""
import functools
import os

import numpy as np
import pytest

import traj_ref as TR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_drum.npz")
STATE = ("x", "v", "quat", "angmom")
QUANTITIES = TR.QUANTITIES + TR.CYL_QUANTITIES


@functools.lru_cache(maxsize=None)
def fixture():
    fix = np.load(GOLDEN)
    sc = {k[3:]: fix[k] for k in fix.files if k.startswith("in_")}
    return fix, sc


def snap(label):
    fix, _ = fixture()
    return {k[len(label) + 1:]: fix[k] for k in fix.files if k.startswith(label + "_")}


def bars():
    fix, _ = fixture()
    assert tuple(str(q) for q in fix["quantities"]) == QUANTITIES
    return dict(zip(QUANTITIES, fix["bar"]))


def pair_options(sc):
    nt = sc["K"].shape[0] - 1
    tp = [(a, b) for a in range(1, nt + 1) for b in range(a, nt + 1)]
    return dict(pair_damping={p: sc["G"][p] for p in tp if sc["G"][p]},
                pair_friction={p: (sc["MU"][p], sc["GT"][p]) for p in tp if sc["MU"][p] or sc["GT"][p]},
                pair_spring={p: sc["KT"][p] for p in tp if sc["KT"][p]},
                pair_rolling={p: (sc["MUR"][p], sc["GR"][p]) for p in tp if sc["MUR"][p] or sc["GR"][p]},
                pair_twisting={p: (sc["MUTW"][p], sc["GTW"][p]) for p in tp if sc["MUTW"][p] or sc["GTW"][p]})


def make_run(det, ledger=True, shell=True, state=None):
    """A DeviceRun of the scene with every option; ledger, shell: the two switches (shell None: never touched); state:
    start from these x, v, quat, angmom, f, torque, planes, cylinders and histories instead of the scene's (a restart)."""
    import torch
    from shpair import ShPair
    from shpair.run import DeviceRun
    _, sc = fixture()
    nt = sc["K"].shape[0] - 1
    sp = ShPair(0)
    sp.settings(int(sc["nq"]))
    sp.set_ntypes(nt, len(sc["a_nm"]))
    for s, a in enumerate(sc["a_nm"]):
        sp.set_shape(s, int(sc["lmax"]), a)
        sp.set_density(s, float(sc["density"][s]))
    for a in range(1, nt + 1):
        for b in range(1, nt + 1):
            sp.coeff(a, b, sc["K"][a, b], sc["E"][a, b])
    if det:
        sp.set_option("deterministic", 1)
    st = state or dict(x=sc["x"], v=sc["v"], quat=sc["quat"], angmom=sc["angmom"], planes=sc["planes"], cyls=sc["cyl"])
    r = DeviceRun(sp, st["x"], st["quat"], sc["shtype"], sc["lo"], sc["hi"], tuple(int(p) for p in sc["periodic"]), float(sc["skin"]),
                  type_=sc["type"], dt=float(sc["dt"]), gravity=tuple(sc["gravity"]), gamma_t=float(sc["gamma_t"]),
                  gamma_r=float(sc["gamma_r"]), mask=sc["mask"], groupbit=int(sc["groupbit"]), ledger=ledger, shell_ledger=shell,
                  walls=(st["planes"], sc["wall_kn"], sc["wall_expo"]), wall_damping=sc["wall_damping"],
                  wall_friction=(sc["wall_mu"], sc["wall_gt"]), wall_spring=sc["wall_kt"], wall_velocity=sc["wall_velocity"],
                  cylinders=(st["cyls"], sc["cyl_kn"], sc["cyl_expo"]), cylinder_damping=sc["cyl_damping"],
                  cylinder_friction=(sc["cyl_mu"], sc["cyl_gt"]), cylinder_rotation=sc["cyl_omega"], cylinder_spring=sc["cyl_kt"],
                  cylinder_rolling=(sc["cyl_mur"], sc["cyl_gr"]), cylinder_twisting=(sc["cyl_mutw"], sc["cyl_gtw"]),
                  **pair_options(sc))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(r.dev)
    r.v[:] = dev(st["v"])
    r.L[:] = dev(st["angmom"])
    if state is None:
        r.force()           # the set-up forces of the scene's velocities (the constructor's saw v = 0): a look, dt = 0
    else:
        # a step's forces are formed from the half-step twists, which no restart can form again: f and torque are state
        keys = owner_keys(r)
        xi = np.zeros((len(keys[0]), 3))
        for s, k in enumerate(zip(*keys)):
            xi[s] = state["xi_by_key"].get((int(k[0]), int(k[1])), 0.0)
        sp.set_contact_history(r.n, xi)
        sp.set_wall_history(r.n, state["wall_xi"])
        sp.set_cyl_history(r.n, state["cyl_xi"])
        r.f[:r.n], r.tq[:r.n] = dev(state["f"]), dev(state["torque"])
    torch.cuda.synchronize()
    sp.synchronize()
    return sp, r


def owner_keys(r):
    """(i, owner tag of j) of every list slot, from copy_neighbors and the rows: the tags are the row indices, and a ghost
    row is its owner's position plus whole box lengths along the periodic directions."""
    _, sc = fixture()
    n, ng = r.n, r.nghost
    xi = r.contact_history()
    offs, jl = r.sp.copy_neighbors(n, len(xi))
    x = r.x[:n + ng].cpu().numpy()
    box, per = sc["hi"] - sc["lo"], sc["periodic"].astype(bool)
    own = np.zeros(ng, np.int64)
    for g in range(ng):
        d = (x[n + g] - x[:n]) / box
        k = np.rint(d)
        ok = (np.abs(d - k) < 1e-9).all(axis=1) & (np.abs(k) <= 1).all(axis=1) & (k[:, ~per] == 0).all(axis=1) & (k != 0).any(axis=1)
        assert ok.sum() == 1, (g, int(ok.sum()))
        own[g] = np.flatnonzero(ok)[0]
    owner = np.concatenate([np.arange(n), own])
    return np.repeat(np.arange(n), np.diff(offs)).astype(np.int32), owner[jl].astype(np.int32), xi


def read(r):
    """The device state in the layout of traj_ref.snapshot.  Blocks."""
    import torch
    torch.cuda.synchronize()
    r.sp.synchronize()
    n = r.n
    out = dict(x=r.x[:n].cpu().numpy(), v=r.v[:n].cpu().numpy(), quat=r.q[:n].cpu().numpy(), angmom=r.L[:n].cpu().numpy(),
               f=r.f[:n].cpu().numpy(), torque=r.tq[:n].cpu().numpy(), planes=r.sp.get_walls(), cyls=r.sp.get_cylinders(),
               wall_xi=r.wall_history(), cyl_xi=r.cylinder_history(), builds=r.builds)
    out["xi_i"], out["xi_key"], out["xi"] = owner_keys(r)
    if r.sp.ledger_on:
        tot, per = r.sp.energy_ledger()
        out["ledger"], out["per_wall"] = np.array(tot), np.array(per)
    if r.sp.shell_ledger_on:
        tot, per = r.sp.shell_ledger()
        out["shell"], out["per_cylinder"] = np.array(tot), np.array(per)
    return out


def same_bits(a, b, ledger=True):
    """Every quantity of two device states bit for bit; pair xi by key (the lists may differ in slots that hold nothing)."""
    bad = [k for k in STATE + ("f", "torque", "planes", "cyls", "wall_xi", "cyl_xi") if not np.array_equal(a[k], b[k])]
    ka, kb = TR.xi_by_key(a["xi_i"], a["xi_key"], a["xi"]), TR.xi_by_key(b["xi_i"], b["xi_key"], b["xi"])
    if set(ka) != set(kb) or any(not np.array_equal(ka[k], kb[k]) for k in ka):
        bad.append("xi")
    if ledger:
        bad += [k for k in ("ledger", "per_wall", "shell", "per_cylinder") if not np.array_equal(a[k], b[k])]
    return bad


def within_bars(got, label, what, ledger=True):
    """Prints measured error against bar per quantity and returns the quantities over their bar."""
    ref = snap(label)
    if not ledger:
        got = dict(got, **{k: ref[k] for k in ("ledger", "per_wall", "shell", "per_cylinder")})
    err, bar = TR.deviation(got, ref), bars()
    print(f"{what} at {label}: " + "  ".join(f"{q} {err[q]:.1e} / {bar[q]:.1e}" for q in QUANTITIES))
    bad = [q for q in QUANTITIES if not err[q] <= bar[q]]
    if not np.array_equal((got["wall_xi"] == 0).all(axis=-1), (ref["wall_xi"] == 0).all(axis=-1)):
        bad.append("live wall springs")
    if not np.array_equal((got["cyl_xi"] != 0).any(axis=-1), ref["cyl_live"]):
        bad.append("live cylinder springs")
    if not np.abs(got["planes"] - ref["planes"]).max() <= 1e-14 * np.abs(ref["planes"]).max():
        bad.append("planes")
    return bad


@functools.lru_cache(maxsize=None)
def step_run(det, ledger=True, shell=True):
    """DeviceRun.step through the whole fixture: the state at every stored label (the restart point is one)."""
    fix, _ = fixture()
    sp, r = make_run(det, ledger, shell)
    labels = [str(s) for s in fix["labels"]]
    out = {"setup": read(r)}
    for k in range(1, int(fix["nsteps"]) + 1):
        r.step()
        if f"step{k}" in labels:
            out[f"step{k}"] = read(r)
    sp.close()
    return out


# ---- the tests ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("det", [0, 1])
def test_setup_forces_match_the_reference(det):
    got, ref = step_run(det)["setup"], snap("setup")
    scale = np.abs(ref["f"]).max()
    ef = np.abs(got["f"] - ref["f"]).max() / scale
    et = np.abs(got["torque"] - ref["torque"]).max() / max(scale, np.abs(ref["torque"]).max())
    print(f"set-up forces: |dF| {ef:.1e}, |dtau| {et:.1e} of max|F| = {scale:.4g} (bar 1e-9)")
    assert scale > 100 and ef < 1e-9 and et < 1e-9
    assert got["builds"] == int(ref["builds"]) == 1 and not got["xi"].any() and not got["wall_xi"].any()
    assert not got["cyl_xi"].any() and not ref["cyl_live"].any()                            # a look: nothing live
    assert not got["shell"].any() and not got["per_cylinder"].any() and not got["ledger"].any()      # and nothing folded
    assert np.array_equal(np.sort(got["xi_i"].astype(np.int64) * 1000 + got["xi_key"]),
                          np.sort(ref["xi_i"].astype(np.int64) * 1000 + ref["xi_key"]))      # the same list, key for key


@pytest.mark.parametrize("det", [0, 1])
def test_step_follows_the_reference_through_every_snapshot(det):
    fix, _ = fixture()
    run = step_run(det)
    bad = {}
    for lab in (str(s) for s in fix["labels"]):
        b = within_bars(run[lab], lab, f"step (deterministic {det})")
        if run[lab]["builds"] != int(snap(lab)["builds"]):
            b.append(f"builds {run[lab]['builds']} != {int(snap(lab)['builds'])}")
        if b:
            bad[lab] = b
    assert not bad, bad


@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
def test_run_native_is_the_step_run_bit_for_bit(graph):
    fix, _ = fixture()
    last = f"step{int(fix['nsteps'])}"
    sp, r = make_run(1)
    r.run_native(int(fix["nsteps"]), use_graph=graph)
    got = read(r)
    sp.close()
    want = step_run(1)[last]
    assert same_bits(got, want) == [] and got["builds"] == want["builds"]
    assert within_bars(got, last, f"run_native ({'graph' if graph else 'plain'})") == []


@pytest.mark.parametrize("shell", [None, True], ids=["both_off", "shell_on_alone"])
def test_ledgers_off_change_nothing_but_the_ledgers(shell):
    """The shell ledger off beside the energy ledger on is a refused state (§2.20), so: both off; and the shell ledger
    switched on ahead of the options while the energy ledger stays off, whose accumulator must stay zero."""
    fix, _ = fixture()
    on, off = step_run(1), step_run(1, False, shell)
    for lab in on:
        assert same_bits(off[lab], on[lab], ledger=False) == [], lab
        assert off[lab]["builds"] == on[lab]["builds"] and "ledger" not in off[lab]
        if shell:
            assert not off[lab]["shell"].any() and not off[lab]["per_cylinder"].any(), lab
        else:
            assert "shell" not in off[lab]
    last = f"step{int(fix['nsteps'])}"
    assert within_bars(off[last], last, f"ledgers off ({'shell on alone' if shell else 'both'})", ledger=False) == []


def test_restart_in_the_middle_continues_bit_for_bit():
    """From x, v, quat, angmom, f, torque, the planes, the cylinders and the three histories of the fixture's restart step
    (pair xi through its keys: the restarted list is another one; cylinder xi by the row).  No row is outside the box
    there, so the new build wraps nothing; both ledgers start again and are added to the ones read at the restart."""
    fix, sc = fixture()
    nst, restart = int(fix["nsteps"]), int(fix["restart"])
    reb = np.flatnonzero(fix["rebuilt"]) + 1
    assert not fix["rebuilt"][restart - 1] and reb.min() < restart < reb.max()
    run = step_run(1)
    mid, want = run[f"step{restart}"], run[f"step{nst}"]
    per = sc["periodic"].astype(bool)
    assert ((mid["x"][:, per] >= sc["lo"][per]) & (mid["x"][:, per] < sc["hi"][per])).all()
    state = dict(mid, xi_by_key=TR.xi_by_key(mid["xi_i"], mid["xi_key"], mid["xi"]))
    assert len(state["xi_by_key"]) > 10 and mid["wall_xi"].any() and (mid["cyl_xi"] != 0).any(axis=-1).sum() >= 3
    sp, r = make_run(1, state=state)
    for _ in range(nst - restart):
        r.step()
    got = read(r)
    sp.close()
    assert same_bits(got, want, ledger=False) == []
    for k in ("ledger", "per_wall", "shell", "per_cylinder"):
        got[k] = got[k] + mid[k]
    assert within_bars(got, f"step{nst}", "restart") == []
