"""Coulomb-capped friction (docs/SPEC.md §2.11) in the loop over several ranks: with option "halo_twists" a pair friction
coefficient widens the forward exchange to 13 doubles per row exactly as a gamma_ij does, a wall friction coefficient
does not.  The ranks are host threads on the one GPU that share an in-process hub; bed, shapes, motion and helpers are
those of tests/mrank_common.py (L = 4, n_q = 8, periodic_hcp(3000, 1.9), kn = 400, m = 1.25, |v| ~ 0.3).

Coefficients.  Static tests: mu = 0.5 with gamma_t = 60 and the damping tests' gamma = 2000; whether both branches of
kappa occur is read from tests/friction_ref.py on the integrals the single-domain compute leaves (asserted >= 5 % each).
Loops at dt = 2e-3: the explicit integrator needs gamma_t dt (1/m + R^2/I) well below 2; with m ~ 4, I ~ 1.7 that is
gamma_t << 1000, so gamma_t = 20 (0.03) beside the damping loops' gamma = 40.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mrank_common import (LMAX, NQ, SKIN, NBED, DT, GAMMA, GAMMA_LOOP, _bed, _ctx, _run_ranks, _shapes, _motion, _setup, _rank_run,   # noqa: E402
                          _gather, _wrap, _masses)

MU, GT, GT_LOOP = 0.5, 60.0, 20.0
NSTEPS = 20


def _friction_ctx(shp, gamma, gt, overlap=0, det=0, twists=1):
    sp = _ctx(LMAX, shp, NQ)
    sp.set_option("halo_overlap", overlap)
    if det:
        sp.set_option("deterministic", 1)
    sp.set_option("halo_twists", twists)
    if gamma:
        sp.pair_damping(1, 1, gamma)
    if gt:
        sp.pair_friction(1, 1, MU, gt)
    return sp


def _branch_shares(sp, r, gamma, gt):
    """Shares (capped, viscous) of the slots with friction of DeviceRun r's last force(), from tests/friction_ref.py."""
    import damp_ref as D
    import friction_ref as F
    n, nall = r.n, r.n + r.nghost
    offs, jl = sp.copy_neighbors(n, r.npairs)
    pi, pj = D.expand(np.arange(n), offs, jl)
    one = lambda v: np.full((2, 2), v)
    _, _, det = F.pair_friction(r.pair_out.cpu().numpy()[:r.npairs], pi, pj, r.x[:nall].cpu().numpy(), r.twist[:nall].cpu().numpy(),
                                np.ones(nall, np.int32), r.sh[:nall].cpu().numpy(), [sp.rmax(0), sp.rmax(1)], one(400.0), one(1.25),
                                one(gamma), one(MU), one(gt), n)
    live = det["fric"] & (det["N"] > 0)
    return float(det["capped"][live].mean()), float((~det["capped"][live]).mean()), int(live.sum())


@functools.lru_cache(maxsize=None)
def _static_reference(periodic):
    """The whole box on one rank (shstep's own periodic images): forces without and with friction, computed once."""
    import torch
    from shpair.run import DeviceRun
    shp = _shapes()
    x, quat, sht, tag, lo, hi, _ = _bed(NBED, periodic)
    n = x.shape[0]
    v, L = _motion(n)
    out = {}
    for name, gt in (("damped", 0.0), ("friction", GT)):
        sp = _ctx(LMAX, shp, NQ)
        r = DeviceRun(sp, x, quat, sht, lo, hi, periodic, SKIN, dt=0.0, pair_damping={(1, 1): GAMMA},
                      pair_friction={(1, 1): (MU, gt)} if gt else None)
        r.v[:] = torch.from_numpy(v).to(r.v.device)
        r.L[:] = torch.from_numpy(L).to(r.L.device)
        r.pair_out = torch.zeros(max(r.npairs, 1), 7, dtype=torch.float64, device=r.dev)
        sp.set_pair_output(r.pair_out.data_ptr())
        r.force()
        torch.cuda.synchronize()
        sp.synchronize()
        out[name] = (r.f[:n].cpu().numpy(), r.tq[:n].cpu().numpy())
        out["npairs"] = r.npairs
        if gt:
            out["shares"] = _branch_shares(sp, r, GAMMA, gt)
        sp.close()
    return out


# ---- 1. static forces with friction (+ damping) match the single domain ----------------------------------------------------

@pytest.mark.parametrize("grid,periodic", [((2, 1, 1), (1, 1, 1)), ((2, 2, 2), (1, 1, 0))])
def test_static_forces_with_friction_match_single_domain(grid, periodic):
    S = _setup(grid, periodic)

    def body(rank):
        sp = _friction_ctx(S["shp"], GAMMA, GT)
        halo, run = _rank_run(S, sp, rank, dt=0.0)
        t, _, _, _, f, tq = run.owned()
        res = dict(tag=t, f=f, tq=tq, npairs=run.npairs)
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(S["world"], body)
    ref = _static_reference(periodic)
    capped, viscous, live = ref["shares"]
    print(f"reference: {live} slots with friction, capped {capped:.3f}, viscous {viscous:.3f}")
    assert live > 1000 and capped >= 0.05 and viscous >= 0.05
    n = S["x"].shape[0]
    f, tq = _gather(parts, n, ("f", "tq"))
    fr, tr = ref["friction"]
    fs = np.abs(fr).max()
    dfric = np.abs(fr - ref["damped"][0]).max()
    ef, et = np.abs(f - fr).max(), np.abs(tq - tr).max()
    print(f"grid {grid}: max|f| {fs:.4g}, friction part {dfric:.4g}, |df| {ef:.2e} |dtau| {et:.2e} (bar {1e-9 * fs:.2e})")
    assert dfric > 1e-2 * fs                                  # the friction contribution is not negligible
    assert sum(p["npairs"] for p in parts) == ref["npairs"]
    assert fs > 0 and ef <= 1e-9 * fs and et <= 1e-9 * fs
    if S["hub"]:
        S["hub"].close()


# ---- 2. the loop matches the single-rank loop ---------------------------------------------------------------------------------

def _decomposed_run(grid, periodic, overlap, gamma, gt, nsteps=NSTEPS, det=0, walls=None, wall_friction=None):
    S = _setup(grid, periodic)

    def body(rank):
        sp = _friction_ctx(S["shp"], gamma, gt, overlap=overlap, det=det)
        halo, run = _rank_run(S, sp, rank, dt=DT, walls=walls, wall_friction=wall_friction)
        run.run(nsteps)
        t, X, V, Q, F, _ = run.owned()
        res = dict(tag=t, x=X, v=V, q=Q, f=F, L=run.L[:run.n].cpu().numpy()[np.argsort(run.tag[:run.n].cpu().numpy())],
                   fwd=halo.stats()["forward_bytes_per_step"], nghost=run.nghost)
        sp.pair_damping(1, 1, 0.0)           # with no pair coefficient left the exchange is the narrow one: its size
        sp.pair_friction(1, 1, 0.0, 0.0)
        res["fwd_narrow"] = halo.stats()["forward_bytes_per_step"]
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(S["world"], body)
    if S["hub"]:
        S["hub"].close()
    return S, parts


@functools.lru_cache(maxsize=None)
def _dynamic_reference(periodic, gt):
    import torch
    from shpair.run import DeviceRun
    shp = _shapes()
    x, quat, sht, tag, lo, hi, _ = _bed(NBED, periodic)
    n = x.shape[0]
    v, L = _motion(n)
    sp = _ctx(LMAX, shp, NQ)
    ref = DeviceRun(sp, x, quat, sht, lo, hi, periodic, SKIN, dt=DT, pair_damping={(1, 1): GAMMA_LOOP},
                    pair_friction={(1, 1): (MU, gt)} if gt else None)
    ref.v[:] = torch.from_numpy(v).to(ref.v.device)
    ref.L[:] = torch.from_numpy(L).to(ref.L.device)
    ref.force()
    ref.run_native(NSTEPS)
    torch.cuda.synchronize()
    sp.synchronize()
    out = ref.x[:n].cpu().numpy(), ref.v.cpu().numpy(), ref.q[:n].cpu().numpy()
    sp.close()
    return out


@pytest.mark.parametrize("overlap", [0, 2])
def test_friction_loop_over_two_ranks_matches_single_rank_loop(overlap):
    grid, periodic = (2, 1, 1), (1, 1, 1)
    S, parts = _decomposed_run(grid, periodic, overlap, GAMMA_LOOP, GT_LOOP)
    n = S["x"].shape[0]
    X, V, Q = _gather(parts, n, ("x", "v", "q"))
    xr, vr, qr = _dynamic_reference(periodic, GT_LOOP)
    x0, v0, _ = _dynamic_reference(periodic, 0.0)
    dx = _wrap(X - xr, S["lo"], S["hi"], periodic)
    mass = _masses(S["shp"])[S["sht"]][:, None]
    p0, p1 = (mass * S["v"]).sum(axis=0), (mass * V).sum(axis=0)
    acted = np.abs(vr - v0).max() / np.abs(vr).max()
    print(f"overlap {overlap}: |dx| {np.abs(dx).max():.2e}, |dv|/max|v| {np.abs(V - vr).max() / np.abs(vr).max():.2e}, "
          f"quat {np.abs(np.abs((Q * qr).sum(1)) - 1).max():.2e}, friction moved v by {acted:.2e}, |dP| {np.abs(p1 - p0).max():.2e}")
    assert acted > 1e-3                                                          # the friction acted
    # 20 steps from the same state; the two loops differ in the order of their atomic sums only (1e-16 relative per step)
    assert np.abs(dx).max() <= 1e-9 and np.abs(V - vr).max() <= 1e-9 * np.abs(vr).max()
    assert np.abs(np.abs((Q * qr).sum(1)) - 1).max() <= 1e-9
    assert np.abs(p1 - p0).max() <= 1e-10 * np.abs(mass * S["v"]).sum()          # nothing external acts
    assert all(p["fwd_narrow"] > 0 and 7 * p["fwd"] == 13 * p["fwd_narrow"] for p in parts)   # the wide exchange


# ---- 3. wall friction alone keeps the 7-wide exchange -----------------------------------------------------------------------

def test_wall_friction_alone_keeps_the_narrow_forward_exchange():
    grid, periodic = (2, 1, 1), (1, 1, 0)
    x, _, _, _, lo, hi, _ = _bed(NBED, periodic)
    floor = ([[0.0, 0.0, 1.0, float(x[:, 2].min() - 0.6)]], 400.0, 1.25)     # within reach of the lowest layer
    # (deterministic sums: two runs agree bit for bit wherever the wall friction did not reach)
    S, parts = _decomposed_run(grid, periodic, 0, 0.0, 0.0, nsteps=1, det=1, walls=floor, wall_friction=(0.5, 20.0))
    S0, parts0 = _decomposed_run(grid, periodic, 0, 0.0, 0.0, nsteps=1, det=1, walls=floor)
    n = S["x"].shape[0]
    assert all(p["nghost"] > 0 and p["fwd"] > 0 and p["fwd"] == p["fwd_narrow"] == q["fwd"] for p, q in zip(parts, parts0))
    (V,), (V0,) = _gather(parts, n, ("v",)), _gather(parts0, n, ("v",))
    low = S["x"][:, 2] < x[:, 2].min() + 0.3
    print(f"wall friction changed v of {int((np.abs(V - V0).max(axis=1) > 0).sum())} particles, {int(low.sum())} in the lowest layer")
    # one step: the wall's particles, and through their drifted positions the neighbours they touch
    assert np.abs(V - V0)[low].max() > 0 and not np.abs(V - V0)[S["x"][:, 2] > x[:, 2].min() + 4.0].any()


# ---- 4. a deterministic run is bitwise reproducible ---------------------------------------------------------------------------

def test_deterministic_friction_run_is_bitwise_reproducible():
    grid, periodic = (2, 1, 1), (1, 1, 1)
    runs = []
    for _ in range(2):
        S, parts = _decomposed_run(grid, periodic, 0, GAMMA_LOOP, GT_LOOP, nsteps=10, det=1)
        runs.append(_gather(parts, S["x"].shape[0], ("x", "v", "q", "L", "f")))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
