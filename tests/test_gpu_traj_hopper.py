"""The run loops against the whole-step reference with cones on (docs/SPEC.md §6, "Order of a step with every model on",
the cone half of item 11): the recorded scene tests/golden/traj_hopper.npz — a turning hopper with damping, friction and
springs at its wall, a plain-friction cone and an elastic one about the bed, a rising plane under it, a bin cylinder with
springs, every pair model, frozen rows, rebuilds — through DeviceRun.step, run_native plain and replayed from graphs, and
across a restart; and its el_ run, the same scene with every cone elastic and both ledgers on.  The bars are the
fixture's: 10 x the reference's own deviation under a 1e-12 relative perturbation of every integral and sum
(tests/golden/make_traj_hopper.py); every test prints measured error against bar.  Reads the fixture and test modules
only: no oracle call."""
import functools
import os

import numpy as np
import pytest

import traj_ref as TR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_hopper.npz")
STATE = ("x", "v", "quat", "angmom")
QUANTITIES = tuple(q for q in TR.QUANTITIES if q != "ledger") + ("cyl_xi",) + TR.CONE_QUANTITIES
EL_QUANTITIES = TR.QUANTITIES + TR.CYL_QUANTITIES
LEDGERS = ("ledger", "per_wall", "shell", "per_cylinder")
CONE_COEFF = ("cone_damping", "cone_mu", "cone_gt", "cone_omega", "cone_kt")


@functools.lru_cache(maxsize=None)
def fixture():
    """(the file, the main scene, the el_ scene: the main one with the el_in_* entries in place of its own)."""
    fix = np.load(GOLDEN)
    sc = {k[3:]: fix[k] for k in fix.files if k.startswith("in_")}
    el = dict(sc, **{k[6:]: fix[k] for k in fix.files if k.startswith("el_in_")})
    assert el["ledger"] == 1 and el["shell_ledger"] == 1 and not any(el[k].any() for k in CONE_COEFF)
    assert sc["ledger"] == 0 and sc["shell_ledger"] == 0 and all(sc[k][0] != 0 for k in CONE_COEFF)
    return fix, sc, el


def snap(label):
    fix = fixture()[0]
    return {k[len(label) + 1:]: fix[k] for k in fix.files if k.startswith(label + "_")}


def bars(el=False):
    fix = fixture()[0]
    names = EL_QUANTITIES if el else QUANTITIES
    assert tuple(str(q) for q in fix["el_quantities" if el else "quantities"]) == names
    return dict(zip(names, fix["el_bar" if el else "bar"]))


def pair_options(sc):
    nt = sc["K"].shape[0] - 1
    tp = [(a, b) for a in range(1, nt + 1) for b in range(a, nt + 1)]
    return dict(pair_damping={p: sc["G"][p] for p in tp if sc["G"][p]},
                pair_friction={p: (sc["MU"][p], sc["GT"][p]) for p in tp if sc["MU"][p] or sc["GT"][p]},
                pair_spring={p: sc["KT"][p] for p in tp if sc["KT"][p]},
                pair_rolling={p: (sc["MUR"][p], sc["GR"][p]) for p in tp if sc["MUR"][p] or sc["GR"][p]},
                pair_twisting={p: (sc["MUTW"][p], sc["GTW"][p]) for p in tp if sc["MUTW"][p] or sc["GTW"][p]})


def make_run(det, el=False, cones="scene", state=None):
    """A DeviceRun of the main scene, or of the el_ scene (both ledgers on).  cones: "scene", None (a control without
    cones) or "far" (the scene's cones moved out of every row's reach).  state: start from these x, v, quat, angmom, f,
    torque, planes, cylinders, cones and histories instead of the scene's (a restart)."""
    import torch
    from shpair import ShPair
    from shpair.run import DeviceRun
    sc = fixture()[2 if el else 1]
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
    st = state or dict(x=sc["x"], v=sc["v"], quat=sc["quat"], angmom=sc["angmom"], planes=sc["planes"], cyls=sc["cyl"],
                       cones=sc["cone"])
    cone = {}
    if cones is not None:
        rec = np.array(st["cones"], float)
        if cones == "far":
            rec[:, :3] -= 1.0e3 * rec[:, 3:6]
        # a coefficient that is zero everywhere is not set at all: set_cones leaves every one at 0 (the el_ scene)
        some = lambda k: sc[k] if sc[k].any() else None
        cone = dict(cones=(rec, sc["cone_kn"], sc["cone_expo"]), cone_damping=some("cone_damping"),
                    cone_friction=(sc["cone_mu"], sc["cone_gt"]) if sc["cone_mu"].any() or sc["cone_gt"].any() else None,
                    cone_rotation=some("cone_omega"), conic_spring=some("cone_kt"))
    r = DeviceRun(sp, st["x"], st["quat"], sc["shtype"], sc["lo"], sc["hi"], tuple(int(p) for p in sc["periodic"]), float(sc["skin"]),
                  type_=sc["type"], dt=float(sc["dt"]), gravity=tuple(sc["gravity"]), gamma_t=float(sc["gamma_t"]),
                  gamma_r=float(sc["gamma_r"]), mask=sc["mask"], groupbit=int(sc["groupbit"]), ledger=bool(sc["ledger"]),
                  shell_ledger=bool(sc["shell_ledger"]),
                  walls=(st["planes"], sc["wall_kn"], sc["wall_expo"]), wall_damping=sc["wall_damping"],
                  wall_friction=(sc["wall_mu"], sc["wall_gt"]), wall_spring=sc["wall_kt"], wall_velocity=sc["wall_velocity"],
                  cylinders=(st["cyls"], sc["cyl_kn"], sc["cyl_expo"]), cylinder_damping=sc["cyl_damping"],
                  cylinder_friction=(sc["cyl_mu"], sc["cyl_gt"]), cylinder_rotation=sc["cyl_omega"], cylinder_spring=sc["cyl_kt"],
                  cylinder_rolling=(sc["cyl_mur"], sc["cyl_gr"]), cylinder_twisting=(sc["cyl_mutw"], sc["cyl_gtw"]),
                  **cone, **pair_options(sc))
    assert sp.ncones == (0 if cones is None else len(sc["cone"])) and sp.has_conic_history == (not el and cones is not None)
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
        sp.set_conic_history(r.n, state["cone_xi"])
        r.f[:r.n], r.tq[:r.n] = dev(state["f"]), dev(state["torque"])
    torch.cuda.synchronize()
    sp.synchronize()
    return sp, r


def owner_keys(r):
    """(i, owner tag of j) of every list slot: the box is not periodic, so there is no ghost row and, the tags being the
    row indices, j is its own owner."""
    assert r.nghost == 0
    xi = r.contact_history()
    offs, jl = r.sp.copy_neighbors(r.n, len(xi))
    return np.repeat(np.arange(r.n), np.diff(offs)).astype(np.int32), np.asarray(jl, np.int32), xi


def read(r):
    """The device state in the layout of traj_ref.snapshot.  Blocks."""
    import torch
    torch.cuda.synchronize()
    r.sp.synchronize()
    n = r.n
    out = dict(x=r.x[:n].cpu().numpy(), v=r.v[:n].cpu().numpy(), quat=r.q[:n].cpu().numpy(), angmom=r.L[:n].cpu().numpy(),
               f=r.f[:n].cpu().numpy(), torque=r.tq[:n].cpu().numpy(), planes=r.sp.get_walls(), cyls=r.sp.get_cylinders(),
               wall_xi=r.wall_history(), cyl_xi=r.cylinder_history(), builds=r.builds)
    if r.sp.ncones:
        out["cones"] = r.sp.get_cones()
        out["cone_xi"] = r.cone_history() if r.sp.has_conic_history else np.zeros((n, r.sp.ncones, 3))
        out["cone_live"] = (out["cone_xi"] != 0).any(axis=-1)
    out["xi_i"], out["xi_key"], out["xi"] = owner_keys(r)
    if r.sp.ledger_on:
        tot, per = r.sp.energy_ledger()
        out["ledger"], out["per_wall"] = np.array(tot), np.array(per)
    if r.sp.shell_ledger_on:
        tot, per = r.sp.shell_ledger()
        out["shell"], out["per_cylinder"] = np.array(tot), np.array(per)
    return out


def same_bits(a, b):
    """Every quantity of two device states bit for bit; pair xi by key (the lists may differ in slots that hold nothing)."""
    bad = [k for k in STATE + ("f", "torque", "planes", "cyls", "cones", "wall_xi", "cyl_xi", "cone_xi")
           if (k in a) != (k in b) or (k in a and not np.array_equal(a[k], b[k]))]
    ka, kb = TR.xi_by_key(a["xi_i"], a["xi_key"], a["xi"]), TR.xi_by_key(b["xi_i"], b["xi_key"], b["xi"])
    if set(ka) != set(kb) or any(not np.array_equal(ka[k], kb[k]) for k in ka):
        bad.append("xi")
    bad += [k for k in LEDGERS if (k in a) != (k in b) or (k in a and not np.array_equal(a[k], b[k]))]
    return bad


def within_bars(got, label, what, el=False):
    """Prints measured error against bar per quantity and returns the quantities over their bar, the live masks of the
    wall, cylinder and conic springs that differ from the reference's, and the planes if they are off by 1e-14."""
    ref = snap(label)
    if not el:                     # neither ledger is on: the reference's rows are zero and are not compared
        assert not any(k in got for k in LEDGERS) and not any(ref[k].any() for k in LEDGERS)
        got = dict(got, **{k: ref[k] for k in LEDGERS})
    err, bar = TR.deviation(got, ref), bars(el)
    print(f"{what} at {label}: " + "  ".join(f"{q} {err[q]:.1e} / {bar[q]:.1e}" for q in bar))
    bad = [q for q in bar if not err[q] <= bar[q]]
    if not np.array_equal((got["wall_xi"] == 0).all(axis=-1), (ref["wall_xi"] == 0).all(axis=-1)):
        bad.append("live wall springs")
    if not np.array_equal((got["cyl_xi"] != 0).any(axis=-1), ref["cyl_live"]):
        bad.append("live cylinder springs")
    if not np.array_equal(got["cone_live"], ref["cone_live"]):
        bad.append("live conic springs")
    if not np.abs(got["planes"] - ref["planes"]).max() <= 1e-14 * np.abs(ref["planes"]).max():
        bad.append("planes")
    return bad


@functools.lru_cache(maxsize=None)
def step_run(det):
    """DeviceRun.step through the whole fixture: the state at every stored label (the restart point is one)."""
    fix = fixture()[0]
    sp, r = make_run(det)
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
    assert not got["cone_xi"].any() and not ref["cone_xi"].any() and not ref["cone_live"].any()     # the conic state all zero
    assert np.array_equal(got["cones"], fixture()[1]["cone"])
    assert np.array_equal(np.sort(got["xi_i"].astype(np.int64) * 1000 + got["xi_key"]),
                          np.sort(ref["xi_i"].astype(np.int64) * 1000 + ref["xi_key"]))      # the same list, key for key


@pytest.mark.parametrize("det", [0, 1])
def test_step_follows_the_reference_through_every_snapshot(det):
    fix = fixture()[0]
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
    fix = fixture()[0]
    last = f"step{int(fix['nsteps'])}"
    sp, r = make_run(1)
    r.run_native(int(fix["nsteps"]), use_graph=graph)
    got = read(r)
    sp.close()
    want = step_run(1)[last]
    assert same_bits(got, want) == [] and got["builds"] == want["builds"]
    assert within_bars(got, last, f"run_native ({'graph' if graph else 'plain'})") == []


def test_restart_in_the_middle_continues_bit_for_bit():
    """From x, v, quat, angmom, f, torque, the planes, the cylinders and the cones as read back and the four histories of
    the fixture's restart step (pair xi through its keys: the restarted list is another one; wall, cylinder and conic
    state by the row).  The conic state handed over is a transported one: live entries whose phi_c has moved since step 1."""
    fix = fixture()[0]
    nst, restart = int(fix["nsteps"]), int(fix["restart"])
    reb = np.flatnonzero(fix["rebuilt"]) + 1
    assert not fix["rebuilt"][restart - 1] and reb.min() < restart < reb.max()
    run = step_run(1)
    first, mid, want = run["step1"], run[f"step{restart}"], run[f"step{nst}"]
    state = dict(mid, xi_by_key=TR.xi_by_key(mid["xi_i"], mid["xi_key"], mid["xi"]))
    both = first["cone_live"] & mid["cone_live"]
    moved = np.abs(mid["cone_xi"][..., 2] - first["cone_xi"][..., 2])[both]
    assert len(state["xi_by_key"]) > 10 and mid["wall_xi"].any() and (mid["cyl_xi"] != 0).any(axis=-1).sum() >= 3
    assert mid["cone_live"].sum() >= 3 and moved.size and 1e-3 < moved.max() < 1.0
    sp, r = make_run(1, state=state)
    for _ in range(nst - restart):
        r.step()
    got = read(r)
    sp.close()
    assert same_bits(got, want) == []
    assert within_bars(got, f"step{nst}", "restart") == []


@functools.lru_cache(maxsize=None)
def el_run(graph, cones="scene"):
    fix = fixture()[0]
    sp, r = make_run(1, el=True, cones=cones)
    first = read(r)
    r.run_native(int(fix["el_nsteps"]), use_graph=graph)
    got = read(r)
    sp.close()
    return first, got


@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
def test_elastic_cones_beside_both_ledgers_follow_the_reference(graph):
    """The el_ run: every cone elastic and at rest, the one state in which cones and ledgers coexist (§2.22).  The loops
    run cone_force_device behind the cylinder pass (the trajectory is the reference's, which has the cones' wrench) and
    the cone pass adds nothing to either ledger (the reference's fold has no cone term): ledger and shell within their
    bars."""
    fix = fixture()[0]
    last = f"el_step{int(fix['el_nsteps'])}"
    first, got = el_run(graph)
    ref = snap("el_setup")
    scale = np.abs(ref["f"]).max()
    ef = np.abs(first["f"] - ref["f"]).max() / scale
    print(f"el_ set-up forces: |dF| {ef:.1e} of max|F| = {scale:.4g} (bar 1e-9)")
    assert ef < 1e-9 and not first["ledger"].any() and not first["shell"].any()
    assert got["ledger"][:4].sum() > 0 and got["shell"].any() and not got["cone_xi"].any()
    assert within_bars(got, last, f"el_ run_native ({'graph' if graph else 'plain'})", el=True) == []
    assert got["builds"] == int(snap(last)["builds"])
    assert same_bits(got, el_run(False)[1]) == []


def test_elastic_cones_leave_no_row_in_the_ledgers():
    """Controls of the el_ run.  Without cones the ledgers have the shapes they always had, and the run with cones has the
    same: no cone row.  With the scene's cones moved out of every row's reach the cone pass runs and the state and both
    ledgers are those of the run without cones bit for bit; so what differs between the run with the scene's cones and
    the control is what the cones' elastic wrench did to the trajectories."""
    _, sc, _ = fixture()
    nw, nc = len(sc["planes"]), len(sc["cyl"])
    _, with_cones = el_run(False)
    _, control = el_run(False, None)
    _, far = el_run(False, "far")
    for got in (with_cones, control, far):
        assert got["ledger"].shape == (5,) and got["per_wall"].shape == (nw, 3)
        assert got["shell"].shape == (3,) and got["per_cylinder"].shape == (nc, 3)
    assert "cones" not in control and far["cones"].shape == (3, 8)
    far = {k: v for k, v in far.items() if k not in ("cones", "cone_xi", "cone_live")}
    assert same_bits(far, control) == [] and far["builds"] == control["builds"]
    d = np.abs(with_cones["x"] - control["x"]).max()
    print(f"the cones moved the rows by up to {d:.2e}; ledger totals {with_cones['ledger']} against {control['ledger']}")
    assert d > 1e-6
