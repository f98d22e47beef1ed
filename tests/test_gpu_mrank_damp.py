"""Volume-rate contact damping (docs/SPEC.md §2.10) in the loop over several ranks: option "halo_twists" of the pair
context, shhalo_forward_twist_device (the forward exchange that carries the owners' twists, 13 doubles per ghost row)
and the damped step order of shhalo_run_device.  The ranks are host threads on the one GPU that share an in-process hub,
as in tests/test_gpu_mrank.py; helpers and bed are those of tests/mrank_common.py: L = 4, n_q = 8, two random shapes (amp 0.2),
periodic_hcp(3000, 1.9) with jitter 0.15, skin 0.2, kn = 400, m = 1.25, random v (|v| ~ 0.3) and angmom drawn per tag.

gamma_11: SPEC §2.10's pressure is p_tot = max(0, p + gamma Vdot); a test of the damping pass has to see both branches.
On this bed with |v| ~ 0.3 the numpy reference (tests/damp_ref.py on the CPU oracle's integrals, 10824 touching slots of
the 2912-particle bed without its periodic images) clamps 0 % of the touching slots at gamma = 40 and at 300, 6.1 % at
1000, 19.2 % at 2000, 31.7 % at 4000.  So the static tests (1, 2) use gamma = 2000 and assert >= 5 % of the reference's
touching slots in each class; there the largest damping force is 0.8 of the largest force of the bed.  The explicit
integrator cannot take that coefficient at dt = 2e-3: the damping part of 6540 force units over relative speeds of ~0.4 is
a drag rate c/m of ~4000 per time unit, c dt / m ~ 8, far beyond the leapfrog's limit of 2, and two runs that differ in the
last bit part (decomposed against single rank, measured): 4e-15 in x after 5 steps, 8e-12 in v after 20, 1.3e-4 in x
after 60, 2e-3 after 120.  The loops (3, 5) therefore run at gamma = 40 (c dt / m ~ 0.16),
where the bed's own elastic energy drives relative speeds high enough for both branches as it expands.

Every test sets "halo_twists" to 1 — an unknown option, SHPAIR_EINVAL, before the option existed.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mrank_common import (LMAX, NQ, SKIN, GAMMA, GAMMA_LOOP, NBED, DT, _bed, _ctx, _run_ranks, _shapes, _motion, _masses, _wrap,   # noqa: E402
                          _setup, _rank_run, _gather)



def _damped_ctx(shp, gamma=GAMMA, overlap=0, det=0, twists=1, nq=NQ, kn=400.0):
    sp = _ctx(LMAX, shp, nq, kn=kn)
    sp.set_option("halo_overlap", overlap)
    if det:
        sp.set_option("deterministic", 1)
    sp.set_option("halo_twists", twists)
    if gamma:
        sp.pair_damping(1, 1, gamma)
    return sp


def _clamp_shares(sp, r, gamma):
    """Shares (clamped, unclamped) of the touching slots of DeviceRun r's last force(): tests/damp_ref.py's pass over the
    integrals that compute left in `r.pair_out`, the library's list and the rows (ghosts included) of x and twist."""
    import damp_ref as D
    n, nall = r.n, r.n + r.nghost
    offs, jl = sp.copy_neighbors(n, r.npairs)
    pi, pj = D.expand(np.arange(n), offs, jl)
    K, E, G = np.full((2, 2), 400.0), np.full((2, 2), 1.25), np.full((2, 2), gamma)
    _, _, det = D.pair_damping(r.pair_out.cpu().numpy()[:r.npairs], pi, pj, r.x[:nall].cpu().numpy(), r.twist[:nall].cpu().numpy(),
                               np.ones(nall, np.int32), K, E, G, n, details=True)
    ok = ~np.isnan(det[:, 0])
    clamped = det[ok, 0] == -det[ok, 2]
    return float(clamped.mean()), float((~clamped).mean()), int(ok.sum())


@functools.lru_cache(maxsize=None)
def _static_reference(periodic):
    """The whole box on one rank (shstep's own periodic images): elastic and damped forces of the bed, computed once."""
    import torch
    from shpair.run import DeviceRun
    shp = _shapes()
    x, quat, sht, tag, lo, hi, _ = _bed(NBED, periodic)
    n = x.shape[0]
    v, L = _motion(n)
    out = {}
    for name, gamma in (("elastic", 0.0), ("damped", GAMMA)):
        sp = _ctx(LMAX, shp, NQ)
        r = DeviceRun(sp, x, quat, sht, lo, hi, periodic, SKIN, dt=0.0, pair_damping={(1, 1): gamma} if gamma else None)
        r.v[:] = torch.from_numpy(v).to(r.v.device)
        r.L[:] = torch.from_numpy(L).to(r.L.device)
        if gamma:
            r.pair_out = torch.zeros(max(r.npairs, 1), 7, dtype=torch.float64, device=r.dev)
            sp.set_pair_output(r.pair_out.data_ptr())
        r.force()
        torch.cuda.synchronize()
        sp.synchronize()
        out[name] = (r.f[:n].cpu().numpy(), r.tq[:n].cpu().numpy())
        out["npairs"] = r.npairs
        if gamma:
            out["shares"] = _clamp_shares(sp, r, gamma)
        sp.close()
    return out


def _assert_both_branches(shares):
    clamped, unclamped, touching = shares
    print(f"reference: {touching} touching slots, clamped {clamped:.3f}, unclamped {unclamped:.3f}")
    assert touching > 1000 and clamped >= 0.05 and unclamped >= 0.05


# ---- 1. ghost twists are their owners', bit for bit ---------------------------------------------------------------------

@pytest.mark.parametrize("grid,periodic", [((2, 1, 1), (1, 1, 1)), ((2, 2, 2), (1, 1, 0))])
def test_ghost_twists_are_their_owners_bit_for_bit(grid, periodic):
    import torch
    S = _setup(grid, periodic)

    def body(rank):
        sp = _damped_ctx(S["shp"])
        halo, run = _rank_run(S, sp, rank, dt=0.0)        # its force(): twists of the owned rows, then forward_twist
        n, ng, a = run.n, run.nghost, run.a
        geo = halo.geometry()
        peers = [geo.peer[c] for c in range(27) if c != 13]
        gx, gq = run.x[n:n + ng].clone(), run.q[n:n + ng].clone()
        res = dict(tag=run.tag[:n].cpu().numpy(), tw=run.twist[:n].cpu().numpy(), gtag=run.tag[n:n + ng].cpu().numpy(),
                   gtw=run.twist[n:n + ng].cpu().numpy(), self_dirs=sum(p == rank for p in peers),
                   open_dirs=sum(p < 0 for p in peers), npeers=halo.stats()["npeers"])
        # the narrow exchange into cleared ghost rows: the same x and quat
        run.x[n:n + ng] = 0.0
        run.q[n:n + ng] = 0.0
        torch.cuda.synchronize()
        halo.forward(a.x, a.quat, run.stream)
        run.sync()
        res["xq_equal"] = bool(torch.equal(run.x[n:n + ng], gx) and torch.equal(run.q[n:n + ng], gq))
        res["gx"] = gx.cpu().numpy()
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(S["world"], body)
    n = S["x"].shape[0]
    owner_tw = np.full((n, 6), np.nan)
    for p in parts:
        owner_tw[p["tag"]] = p["tw"]
    assert not np.isnan(owner_tw).any() and np.abs(owner_tw).min(axis=1).max() > 0
    for p in parts:
        assert p["gtag"].size > 0 and p["npeers"] >= 1 and np.abs(p["gx"]).max() > 0
        assert np.array_equal(p["gtw"], owner_tw[p["gtag"]])
        assert p["xq_equal"]
    if periodic == (1, 1, 1):
        assert all(p["self_dirs"] > 0 for p in parts)         # directions that lead back to the rank itself
    else:
        assert all(p["open_dirs"] > 0 for p in parts)         # open boundaries
        assert all(p["npeers"] >= 3 for p in parts)           # faces, edges, corners
    if S["hub"]:
        S["hub"].close()


# ---- 2. static damped forces match the single domain --------------------------------------------------------------------

@pytest.mark.parametrize("grid,periodic", [((2, 1, 1), (1, 1, 1)), ((2, 2, 2), (1, 1, 0)), ((1, 1, 1), (1, 1, 1))])
def test_static_damped_forces_match_single_domain(grid, periodic):
    S = _setup(grid, periodic)

    def body(rank):
        sp = _damped_ctx(S["shp"])
        halo, run = _rank_run(S, sp, rank, dt=0.0)
        t, _, _, _, f, tq = run.owned()
        res = dict(tag=t, f=f, tq=tq, npairs=run.npairs)
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(S["world"], body)
    ref = _static_reference(periodic)
    _assert_both_branches(ref["shares"])
    n = S["x"].shape[0]
    f, tq = _gather(parts, n, ("f", "tq"))
    fr, tr = ref["damped"]
    fs = np.abs(fr).max()
    ddamp = np.abs(fr - ref["elastic"][0]).max()
    ef, et = np.abs(f - fr).max(), np.abs(tq - tr).max()
    print(f"grid {grid}: max|f| {fs:.4g}, damping part {ddamp:.4g}, |df| {ef:.2e} |dtau| {et:.2e} (bar {1e-12 * fs:.2e})")
    assert ddamp > 1e-3 * fs                                  # the damping contribution is not negligible
    assert sum(p["npairs"] for p in parts) == ref["npairs"]
    assert fs > 0 and ef <= 1e-12 * fs and et <= 1e-12 * fs
    if S["hub"]:
        S["hub"].close()


# ---- 3. the loop matches the single-rank loop -----------------------------------------------------------------------------

NSTEPS = 120


def _kinetic(run):
    """Translational + rotational kinetic energy of the owned rows (shstep_energies_device)."""
    a = run.a
    run.sync()
    run.en.zero_()
    run.torch.cuda.synchronize()
    run.sp.energies_device(a.nlocal, np.zeros(3), a.x, a.v, a.quat, a.angmom, a.shtype, a.mask, run.en.data_ptr(), stream=run.stream)
    run.sync()
    e = run.en.cpu().numpy()
    return float(e[0] + e[1])


def _decomposed_run(grid, periodic, overlap, gamma, nsteps=NSTEPS, det=0):
    """nsteps of shhalo_run_device on every rank of the grid, from the bed and motion of _setup()."""
    S = _setup(grid, periodic)

    def body(rank):
        sp = _damped_ctx(S["shp"], gamma=gamma, overlap=overlap, det=det)
        halo, run = _rank_run(S, sp, rank, dt=DT)
        b0 = run.builds
        run.run(nsteps)
        t, X, V, Q, _, _ = run.owned()
        res = dict(tag=t, x=X, v=V, q=Q, rebuilds=run.builds - b0, ke=_kinetic(run) if run.n else 0.0, stats=halo.stats())
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(S["world"], body)
    if S["hub"]:
        S["hub"].close()
    return S, parts


@functools.lru_cache(maxsize=None)
def _undamped_kinetic(grid, periodic):
    _, parts = _decomposed_run(grid, periodic, 0, 0.0)
    return sum(p["ke"] for p in parts)


@functools.lru_cache(maxsize=None)
def _dynamic_reference(periodic, gamma=GAMMA_LOOP, nsteps=NSTEPS):
    import torch
    from shpair.run import DeviceRun
    shp = _shapes()
    x, quat, sht, tag, lo, hi, _ = _bed(NBED, periodic)
    n = x.shape[0]
    v, L = _motion(n)
    sp = _ctx(LMAX, shp, NQ)
    ref = DeviceRun(sp, x, quat, sht, lo, hi, periodic, SKIN, dt=DT, pair_damping={(1, 1): gamma})
    ref.v[:] = torch.from_numpy(v).to(ref.v.device)
    ref.L[:] = torch.from_numpy(L).to(ref.L.device)
    ref.force()
    ref.run(nsteps)
    torch.cuda.synchronize()
    sp.synchronize()
    out = ref.x[:n].cpu().numpy(), ref.v.cpu().numpy(), ref.q[:n].cpu().numpy()
    sp.close()
    return out


@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("grid,periodic", [((2, 1, 1), (1, 1, 1)), ((2, 2, 2), (1, 1, 0))])
def test_damped_loop_matches_single_rank_loop(grid, periodic, overlap):
    S, parts = _decomposed_run(grid, periodic, overlap, GAMMA_LOOP)
    n = S["x"].shape[0]
    X, V, Q = _gather(parts, n, ("x", "v", "q"))
    rebuilds = [p["rebuilds"] for p in parts]
    migrated = sum(p["stats"]["migrated_out"] for p in parts)
    xr, vr, qr = _dynamic_reference(periodic)
    dx = _wrap(X - xr, S["lo"], S["hi"], periodic)
    mass = _masses(S["shp"])[S["sht"]][:, None]
    p0, p1 = (mass * S["v"]).sum(axis=0), (mass * V).sum(axis=0)
    ke, ke0 = sum(p["ke"] for p in parts), _undamped_kinetic(grid, periodic)
    print(f"grid {grid} overlap {overlap}: rebuilds {rebuilds}, migrated {migrated}, |dx| {np.abs(dx).max():.2e}, "
          f"|dv|/max|v| {np.abs(V - vr).max() / np.abs(vr).max():.2e}, quat {np.abs(np.abs((Q * qr).sum(1)) - 1).max():.2e}, "
          f"KE damped {ke:.6g} undamped {ke0:.6g}, |dP| {np.abs(p1 - p0).max():.2e} of {np.abs(mass * S['v']).sum():.4g}")
    assert min(rebuilds) >= 1 and len(set(rebuilds)) == 1 and migrated > 0       # a rebuild with migration, together
    assert np.abs(dx).max() < 1e-7 and np.abs(V - vr).max() < 1e-6 * np.abs(vr).max()
    assert np.abs(np.abs((Q * qr).sum(1)) - 1).max() < 1e-9
    assert ke < ke0                                                              # the damping acted
    assert np.abs(p1 - p0).max() <= 1e-10 * np.abs(mass * S["v"]).sum()          # nothing external acts


# ---- 4. two spheres across a rank boundary ----------------------------------------------------------------------------------

def test_two_spheres_collide_across_a_rank_boundary():
    """The set-up of tests/test_gpu_damp.py's _two_spheres (L = 0, kn = 1e4, m = 1.25, dt = 2e-4, gamma = 1000, open box) at
    n_q = 16, one sphere on each rank of a 2 x 1 x 1 grid: the contact exists only through ghost rows."""
    import torch
    from shpair import ShPair, shapes, mrank
    from shpair.run import DeviceRun
    x = np.array([[2.99, 4.0, 4.0], [5.01, 4.0, 4.0]])
    v = np.array([[1.0, 0, 0], [-1.0, 0, 0]])
    quat = np.array([[1.0, 0, 0, 0]] * 2)
    lo, hi, per, skin, dt, nsteps, gamma = np.zeros(3), np.full(3, 8.0), (0, 0, 0), 0.3, 2e-4, 700, 1000.0
    grid, world = (2, 1, 1), 2

    def ctx():
        sp = ShPair(0)
        sp.settings(16)
        sp.set_ntypes(1, 1)
        sp.set_shape(0, 0, shapes.sphere(1.0), 1.01)
        sp.coeff(1, 1, 1e4, 1.25)
        sp.set_option("deterministic", 1)
        return sp
    hub = mrank.Hub(world)

    def body(rank):
        sp = ctx()
        sp.set_option("halo_twists", 1)
        sp.pair_damping(1, 1, gamma)
        halo = mrank.Halo(sp, rank, world, grid, lo, hi, per, skin, hub=hub)
        mine = np.array([rank == 0, rank == 1])                 # the brick face is x = 4
        run = mrank.RankRun(sp, halo, x[mine], quat[mine], np.zeros(1, np.int32), np.arange(2, dtype=np.int32)[mine], v=v[mine], dt=dt,
                            capacity=64)
        n0 = run.n
        run.run(nsteps)
        t, X, V, _, _, _ = run.owned()
        res = dict(tag=t, x=X, v=V, n0=n0, mass=sp.body(0)[0])
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(world, body)
    hub.close()
    assert [p["n0"] for p in parts] == [1, 1]
    X, V = _gather(parts, 2, ("x", "v"))
    sp = ctx()
    r = DeviceRun(sp, x, quat, np.zeros(2, np.int32), lo, hi, per, skin, dt=dt, pair_damping={(1, 1): gamma})
    r.v[:] = torch.from_numpy(v).to(r.v.device)
    r.force()
    r.run_native(nsteps)
    torch.cuda.synchronize()
    xr, vr = r.x[:2].cpu().numpy(), r.v.cpu().numpy()
    sp.close()
    sep, mass = V[1, 0] - V[0, 0], parts[0]["mass"]
    print(f"separation speed {sep:.6f} (approach 2), gap {X[1, 0] - X[0, 0]:.4f}, net momentum {np.abs(mass * V.sum(axis=0)).max():.2e}, "
          f"|dx| {np.abs(X - xr).max():.2e} |dv| {np.abs(V - vr).max():.2e}")
    assert X[1, 0] - X[0, 0] > 2.02 and 0 < sep < 2.0                        # they met, parted, and slower than they came
    assert np.abs(mass * V.sum(axis=0)).max() <= 1e-10 * mass * 2.0          # the total was zero: relative to sum |m v|
    assert np.abs(X - xr).max() <= 1e-9 and np.abs(V - vr).max() <= 1e-9


# ---- 5. deterministic mode is bitwise reproducible ----------------------------------------------------------------------------

def test_deterministic_damped_run_is_bitwise_reproducible():
    S = _setup((2, 2, 1), (1, 1, 0))

    def body(rank):
        sp = _damped_ctx(S["shp"], gamma=GAMMA_LOOP, det=1)
        halo, run = _rank_run(S, sp, rank, dt=DT)
        state = run.save_state()
        out = []
        for _ in range(2):
            run.run(40)
            run.sync()
            n = run.n
            out.append([t[:n].cpu().numpy().copy() for t in (run.tag, run.x, run.v, run.q, run.L)])
            run.restore_state(state)
        halo.close()
        sp.close()
        return out
    parts = _run_ranks(S["world"], body)
    for first, second in parts:
        assert first[0].size > 0 and np.abs(first[2]).max() > 0
        assert all(np.array_equal(a, b) for a, b in zip(first, second))
    S["hub"].close()


# ---- 6. wall damping only --------------------------------------------------------------------------------------------------------

def test_wall_damping_only_keeps_the_narrow_exchange():
    """gamma_w > 0 and every gamma_ij = 0 over a floor, with gravity: the twists of the owned rows are all the damped wall
    pass needs, so the exchange stays 7 wide; periodic in x only, so every send row goes to the other rank."""
    import torch
    from shpair.run import DeviceRun
    grid, periodic, nsteps, gw = (2, 1, 1), (1, 0, 0), 40, 500.0
    S = _setup(grid, periodic)
    planes = [[0.0, 0.0, 1.0, float(S["x"][:, 2].min() - 0.8)]]   # the lowest layer's particles overlap the floor
    walls, grav = (planes, 400.0, 1.25), (0.0, 0.0, -0.5)

    def body(rank):
        sp = _damped_ctx(S["shp"], gamma=0.0)
        halo, run = _rank_run(S, sp, rank, dt=DT, gravity=grav, walls=walls, wall_damping=gw)
        run.run(nsteps)
        t, X, V, Q, _, _ = run.owned()
        st7 = halo.stats()
        sp.pair_damping(1, 1, GAMMA)
        st13 = halo.stats()
        res = dict(tag=t, x=X, v=V, q=Q, st7=st7, st13=st13, wall_contacts=sp.wall_stats())
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(S["world"], body)
    S["hub"].close()
    for p in parts:
        rows = p["st7"]["nsend_rows"]
        assert rows > 0 and p["st7"]["forward_bytes_per_step"] == 7 * 8 * rows
        assert p["st13"]["nsend_rows"] == rows and p["st13"]["forward_bytes_per_step"] == 13 * 8 * rows
    assert sum(p["wall_contacts"] for p in parts) > 10
    n = S["x"].shape[0]
    X, V, Q = _gather(parts, n, ("x", "v", "q"))
    sp0 = _ctx(LMAX, S["shp"], NQ)
    ref = DeviceRun(sp0, S["x"], S["quat"], S["sht"], S["lo"], S["hi"], periodic, SKIN, dt=DT, gravity=grav, walls=walls,
                    wall_damping=gw)
    ref.v[:] = torch.from_numpy(S["v"]).to(ref.v.device)
    ref.L[:] = torch.from_numpy(S["L"]).to(ref.L.device)
    ref.force()
    ref.run(nsteps)
    torch.cuda.synchronize()
    xr, vr, qr = ref.x[:n].cpu().numpy(), ref.v.cpu().numpy(), ref.q[:n].cpu().numpy()
    sp0.close()
    dx = _wrap(X - xr, S["lo"], S["hi"], periodic)
    print(f"wall damping only: |dx| {np.abs(dx).max():.2e}, |dv|/max|v| {np.abs(V - vr).max() / np.abs(vr).max():.2e}")
    assert np.abs(dx).max() < 1e-7 and np.abs(V - vr).max() < 1e-6 * np.abs(vr).max()
    assert np.abs(np.abs((Q * qr).sum(1)) - 1).max() < 1e-9


# ---- 7. gamma = 0 is the loop without the option ----------------------------------------------------------------------------------

def test_option_without_coefficients_changes_no_bit():
    from shpair import mrank
    S = _setup((2, 1, 1), (1, 1, 1))
    S["hub"].close()
    runs = []
    for twists in (0, 1):
        S["hub"] = mrank.Hub(S["world"])

        def body(rank):
            sp = _damped_ctx(S["shp"], gamma=0.0, det=1, twists=twists)
            halo, run = _rank_run(S, sp, rank, dt=DT)
            run.run(40)
            run.sync()
            n = run.n
            res = [t[:n].cpu().numpy().copy() for t in (run.tag, run.x, run.v, run.q, run.L, run.f, run.tq)]
            res.append(halo.stats()["forward_bytes_per_step"])
            halo.close()
            sp.close()
            return res
        runs.append(_run_ranks(S["world"], body))
        S["hub"].close()
    for off, on in zip(*runs):
        assert off[0].size > 0 and np.abs(off[2]).max() > 0
        assert all(np.array_equal(a, b) for a, b in zip(off[:-1], on[:-1])) and off[-1] == on[-1]


# ---- 8. argument checks ---------------------------------------------------------------------------------------------------------------

def test_argument_checks():
    import torch
    from shpair import mrank, ShPairError
    from shpair.capi import HaloArrays, HaloRunParams
    shp = _shapes()
    periodic = (1, 1, 1)
    x, quat, sht, tag, lo, hi, _ = _bed(300, periodic)
    sp = _damped_ctx(shp, gamma=0.0)
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), lo, hi, periodic, SKIN)
    buf = torch.zeros(16, 6, dtype=torch.float64, device="cuda:0")
    with pytest.raises(ShPairError, match="no plan") as e:          # before shhalo_borders_device
        halo.forward_twist(buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
    assert e.value.code == -4
    run = mrank.RankRun(sp, halo, x, quat, sht, tag, dt=1e-3)
    assert run.nghost > 0
    with pytest.raises(ShPairError, match="null array pointer") as e:
        halo.forward_twist(run.a.x, run.a.quat, None, run.stream)
    assert e.value.code == -1
    # without the option the loop still refuses while a coefficient is set
    sp.set_option("halo_twists", 0)
    sp.pair_damping(1, 1, 10.0)
    with pytest.raises(ShPairError, match="contact damping is not supported") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -1
    halo.close()
    sp.close()
