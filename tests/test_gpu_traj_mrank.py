"""The loop over several ranks (shhalo_run_device, driven by shpair.mrank.RankRun) against the whole-step reference
(docs/SPEC.md §6, "The same step over several ranks"): the recorded scene tests/golden/traj_mrank.npz — everything that
loop accepts switched on at once: two types, two shapes, frozen rows, pair damping, history-free friction, rolling,
twisting, a piston, a belt, gravity, drag and the ledger, with rows that change rank through every cut and through the
periodic faces — on the grids 1x1x1 (the self-periodic rank), 2x1x1, 1x1x2 and 2x2x2.  The ranks are host threads on one
mrank.Hub.  The bars are the fixture's: 10 x the reference's own deviation under a 1e-12 relative perturbation of every
integral (tests/golden/make_traj_mrank.py); every test prints measured error against bar.  Reads the fixture and test
modules only: no oracle call."""
import functools
import os

import numpy as np
import pytest

import traj_ref as TR
from mrank_common import _distribute, _gather, _run_ranks
from test_gpu_traj import pair_options

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_mrank.npz")
STATE = ("x", "v", "quat", "angmom")
QUANTITIES = STATE + ("ledger",)                 # the spring quantities are left out: this loop refuses the springs
GRIDS = [(1, 1, 1), (2, 1, 1), (1, 1, 2), (2, 2, 2)]
gid = lambda g: "x".join(str(k) for k in g)


@functools.lru_cache(maxsize=None)
def fixture():
    fix = np.load(GOLDEN)
    sc = {k[3:]: fix[k] for k in fix.files if k.startswith("in_")}
    return fix, sc


@functools.lru_cache(maxsize=None)
def snap(label):
    fix, _ = fixture()
    return {k[len(label) + 1:]: fix[k] for k in fix.files if k.startswith(label + "_")}


def labels():
    return [str(s) for s in fixture()[0]["labels"]]


def bars():
    fix, _ = fixture()
    return dict(zip((str(q) for q in fix["quantities"]), fix["bar"]))


def make_ranks(grid, det, overlap=0, ledger=True):
    """(world, hub, owner, make): make(rank) -> (sp, halo, RankRun) of the scene with every option, the same on every
    rank; to be called by the rank's own thread (the constructor is collective)."""
    from shpair import ShPair, mrank
    _, sc = fixture()
    nt = sc["K"].shape[0] - 1
    world = int(np.prod(grid))
    per = tuple(int(p) for p in sc["periodic"])
    xw, owner = _distribute(grid, sc["lo"], sc["hi"], per, 2.0 * sc["rmax"].max() + float(sc["skin"]), sc["x"])
    hub = mrank.Hub(world) if world > 1 else None

    def make(rank):
        sp = ShPair(0)
        sp.settings(int(sc["nq"]))
        sp.set_ntypes(nt, len(sc["a_nm"]))
        for s, a in enumerate(sc["a_nm"]):
            sp.set_shape(s, int(sc["lmax"]), a)
            sp.set_density(s, float(sc["density"][s]))
        for a in range(1, nt + 1):
            for b in range(1, nt + 1):
                sp.coeff(a, b, sc["K"][a, b], sc["E"][a, b])
        sp.set_option("deterministic", det)
        sp.set_option("halo_overlap", overlap)
        sp.set_option("halo_twists", 1)
        if ledger:
            sp.set_energy_ledger(True)
        halo = mrank.Halo(sp, rank, world, grid, sc["lo"], sc["hi"], per, float(sc["skin"]), hub=hub)
        m = owner == rank
        opts = pair_options(sc)
        assert not opts.pop("pair_spring") and not sc["wall_kt"].any()
        run = mrank.RankRun(sp, halo, xw[m], sc["quat"][m], sc["shtype"][m], sc["tag"][m], type_=sc["type"][m], v=sc["v"][m],
                            angmom=sc["angmom"][m], mask=sc["mask"][m], groupbit=int(sc["groupbit"]), dt=float(sc["dt"]),
                            gravity=tuple(sc["gravity"]), gamma_t=float(sc["gamma_t"]), gamma_r=float(sc["gamma_r"]), check_every=1,
                            walls=(sc["planes"], sc["wall_kn"], sc["wall_expo"]), wall_damping=sc["wall_damping"],
                            wall_friction=(sc["wall_mu"], sc["wall_gt"]), wall_velocity=sc["wall_velocity"], **opts)
        return sp, halo, run
    return world, hub, owner, make


def read(sp, run):
    """One rank's share of a state: its owned rows with their tags, its planes, its ledger, its build count.  Blocks."""
    import torch
    run.sync()
    torch.cuda.synchronize()
    n = run.n
    out = dict(tag=run.tag[:n].cpu().numpy(), x=run.x[:n].cpu().numpy(), v=run.v[:n].cpu().numpy(), quat=run.q[:n].cpu().numpy(),
               angmom=run.L[:n].cpu().numpy(), f=run.f[:n].cpu().numpy(), torque=run.tq[:n].cpu().numpy(), planes=sp.get_walls(),
               builds=run.builds, n=n)
    if sp.ledger_on:
        out["ledger"], out["per_wall"] = sp.energy_ledger()
    return out


def gather(parts):
    """The ranks' shares as one state in the reference's rows: every tag once, the ledger summed over the ranks."""
    _, sc = fixture()
    n = len(sc["x"])
    keys = STATE + ("f", "torque")
    out = {k: a[sc["tag"]] for k, a in zip(keys, _gather(parts, n, keys))}
    out["parts"] = parts
    if "ledger" in parts[0]:
        out["ledger"], out["per_wall"] = sum(p["ledger"] for p in parts), sum(p["per_wall"] for p in parts)
    return out


@functools.lru_cache(maxsize=None)
def follow(grid, det, overlap=0, ledger=True, segmented=True):
    """RankRun.run on every rank of a grid, from label to label (or in one call): {label: gathered state}."""
    fix, _ = fixture()
    world, hub, _, make = make_ranks(grid, det, overlap, ledger)
    at = [int(l[4:]) for l in labels() if l != "setup"] if segmented else [int(fix["nsteps"])]

    def body(rank):
        sp, halo, run = make(rank)
        out, done = {"setup": read(sp, run)}, 0
        for k in at:
            run.run(k - done)
            done = k
            out[f"step{k}"] = read(sp, run)
        halo.close()
        sp.close()
        return out
    parts = _run_ranks(world, body)
    if hub is not None:
        hub.close()
    return {lab: gather([p[lab] for p in parts]) for lab in parts[0]}


def errors(got, label, what, ledger=True):
    """Prints measured error against bar per quantity; returns what is wrong: the quantities over their bar, a rank whose
    build count or planes are not the reference's, ranks whose planes differ in a bit."""
    ref = snap(label)
    full = dict(got, **{k: ref[k] for k in ("xi", "xi_i", "xi_key", "wall_xi")})
    if not ledger:
        full.update(ledger=ref["ledger"], per_wall=ref["per_wall"])
    err, bar = TR.deviation(full, ref), bars()
    qs = [q for q in QUANTITIES if ledger or q != "ledger"]
    print(f"{what} at {label}: " + "  ".join(f"{q} {err[q]:.1e} / {bar[q]:.1e}" for q in qs))
    bad = [q for q in qs if not err[q] <= bar[q]]
    parts = got["parts"]
    if any(p["builds"] != int(ref["builds"]) for p in parts):
        bad.append(f"builds {[p['builds'] for p in parts]} != {int(ref['builds'])}")
    if any(not np.array_equal(p["planes"], parts[0]["planes"]) for p in parts):
        bad.append("the ranks' planes differ")
    if not np.abs(parts[0]["planes"] - ref["planes"]).max() <= 1e-14 * np.abs(ref["planes"]).max():
        bad.append("planes")
    return bad


def same_bits(a, b):
    return [k for k in STATE if not np.array_equal(a[k], b[k])]


# ---- the tests ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", GRIDS, ids=gid)
def test_setup_forces_match_the_reference(grid):
    got, ref = follow(grid, 1)["setup"], snap("setup")
    scale = np.abs(ref["f"]).max()
    ef = np.abs(got["f"] - ref["f"]).max() / scale
    et = np.abs(got["torque"] - ref["torque"]).max() / max(scale, np.abs(ref["torque"]).max())
    print(f"set-up forces on {gid(grid)}: |dF| {ef:.1e}, |dtau| {et:.1e} of max|F| = {scale:.4g} (bar 1e-9)")
    assert scale > 100 and ef < 1e-9 and et < 1e-9
    assert all(p["builds"] == 1 for p in got["parts"]) and all(p["n"] > 0 for p in got["parts"])
    assert not got["ledger"].any() and not got["per_wall"].any()           # the set-up pass is a look: nothing is folded


@pytest.mark.parametrize("grid,det", [(g, 1) for g in GRIDS] + [((2, 2, 2), 0)], ids=lambda v: gid(v) if isinstance(v, tuple) else f"det{v}")
def test_the_loop_follows_the_reference_through_every_snapshot(grid, det):
    run = follow(grid, det)
    bad = {}
    for lab in labels():
        b = errors(run[lab], lab, f"{gid(grid)} (deterministic {det})")
        if b:
            bad[lab] = b
    assert not bad, bad


@pytest.mark.parametrize("overlap", [1, 2])
def test_overlapped_exchanges_stay_within_the_bars(overlap):
    last = labels()[-1]
    got = follow((2, 2, 2), 1, overlap, True, False)[last]
    assert errors(got, last, f"2x2x2, halo_overlap {overlap}") == []


def test_one_unsegmented_run_is_the_segmented_one_bit_for_bit():
    last = labels()[-1]
    got, want = follow((2, 2, 2), 1, 0, True, False)[last], follow((2, 2, 2), 1)[last]
    assert errors(got, last, "2x2x2, one call") == []
    assert same_bits(got, want) == []
    assert np.array_equal(got["ledger"], want["ledger"]) and np.array_equal(got["per_wall"], want["per_wall"])


def test_ledger_off_changes_nothing_but_the_ledger():
    on, off = follow((2, 2, 2), 1), follow((2, 2, 2), 1, 0, False)
    for lab in labels():
        assert same_bits(off[lab], on[lab]) == [], lab
        assert "ledger" not in off[lab]
    last = labels()[-1]
    assert errors(off[last], last, "2x2x2, ledger off", ledger=False) == []


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 1, 2)], ids=gid)
def test_a_rank_tallies_only_the_walls_its_rows_reach(grid):
    """The reference decides which rank could have touched which wall: a rank owns a row from one build to the next
    (traj_ref.brick_owner on the build's rows), and a row reaches a wall in a step if its bounding sphere crosses the plane
    (the fixture's wall_reach).  A rank that never owned a row within reach of a wall holds exact zeros for that wall.  On
    2x1x1 both ranks reach every wall in this scene (rows carry the belt's contact through the periodic face), so there
    only the signs are checked; on 1x1x2 the upper rank never reaches the floor or the belt."""
    fix, sc = fixture()
    axis = int(np.argmax(grid))
    owner = lambda x: TR.brick_owner(x, sc["lo"], sc["hi"], sc["periodic"], grid)[:, axis]
    run = follow(grid, 1)
    last = labels()[-1]
    parts = run[last]["parts"]
    # the brick of each library rank, from the rows it was given
    first = run["setup"]["parts"]
    tag_row = np.argsort(sc["tag"])
    ix0 = owner(snap("setup")["x"])
    brick = []
    for p in first:
        b = set(ix0[tag_row[p["tag"]]].tolist())
        assert len(b) == 1
        brick.append(b.pop())
    assert sorted(brick) == [0, 1]
    # the owner of every row at every step
    ix, reached = ix0, np.zeros((2, len(sc["planes"])), bool)
    for k in range(int(fix["nsteps"])):
        if fix["rebuilt"][k]:
            ix = owner(snap(f"step{k + 1}")["x"])
        for b in (0, 1):
            reached[b] |= fix["wall_reach"][k][ix == b].any(axis=0)
    print("bricks of the ranks", brick, "reach", reached.tolist(), "per wall", [p["per_wall"].tolist() for p in parts])
    for r, p in enumerate(parts):
        assert p["ledger"][0] >= 0 and p["ledger"][1] >= 0
        for w in range(len(sc["planes"])):
            if not reached[brick[r], w]:
                assert not p["per_wall"][w].any(), (r, w)
    assert reached.any() and sum(p["per_wall"][0, 2] for p in parts) > 0
    if grid == (1, 1, 2):
        assert not reached[1, 0] and not reached[1, 1] and reached[0, 0] and reached[0, 1]
