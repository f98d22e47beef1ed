"""Rolling and twisting resistance at planar walls (docs/SPEC.md §2.17) in the loop over several ranks, in the manner of
tests/test_gpu_mrank_damp.py's wall-damping test: a small bed over a floor, on the 1x1x1 and the 2x1x1 grid under option
"halo_twists", against the single-rank driver at that file's bars; and the refusal without the option.  A wall has no ghost
rows and nothing new travels: the exchange stays 7 wide.  Helpers and bed are those of tests/mrank_common.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mrank_common import LMAX, NQ, SKIN, DT, _ctx, _run_ranks, _setup, _rank_run, _gather, _wrap   # noqa: E402

NBED, NSTEPS = 600, 20
ROLL, TWIST = (0.05, 4.0), (0.03, 2.5)
GRAV = (0.0, 0.0, -0.5)
PERIODIC = (1, 0, 0)
_ref = {}


def _walls(S):
    return ([[0.0, 0.0, 1.0, float(S["x"][:, 2].min() - 0.8)]], 400.0, 1.25)   # the lowest layer's particles overlap the floor


def _reference(S, resist=True):
    """The whole box on one rank through DeviceRun: x, v, q, f, torque after NSTEPS, computed once."""
    import torch
    from shpair.run import DeviceRun
    if resist not in _ref:
        n = S["x"].shape[0]
        sp = _ctx(LMAX, S["shp"], NQ)
        kw = dict(wall_rolling=ROLL, wall_twisting=TWIST) if resist else {}
        r = DeviceRun(sp, S["x"], S["quat"], S["sht"], S["lo"], S["hi"], PERIODIC, SKIN, dt=DT, gravity=GRAV, walls=_walls(S), **kw)
        r.v[:] = torch.from_numpy(S["v"]).to(r.v.device)
        r.L[:] = torch.from_numpy(S["L"]).to(r.L.device)
        r.force()
        r.run(NSTEPS)
        torch.cuda.synchronize()
        _ref[resist] = [t[:n].cpu().numpy().copy() for t in (r.x, r.v, r.q, r.f, r.tq)] + [sp.wall_stats()]
        sp.close()
    return _ref[resist]


@pytest.mark.parametrize("grid", [(1, 1, 1), (2, 1, 1)])
def test_the_decomposed_run_agrees_with_the_single_rank_run(grid):
    S = _setup(grid, PERIODIC, nbed=NBED)

    def body(rank):
        sp = _ctx(LMAX, S["shp"], NQ)
        sp.set_option("halo_twists", 1)
        halo, run = _rank_run(S, sp, rank, dt=DT, gravity=GRAV, walls=_walls(S), wall_rolling=ROLL, wall_twisting=TWIST)
        assert sp.has_wall_rolling and not sp.keeps_integrals
        run.run(NSTEPS)
        run.sync()
        t, X, V, Q, Fo, To = run.owned()
        res = dict(tag=t, x=X, v=V, q=Q, f=Fo, tq=To, st=halo.stats(), wall_contacts=sp.wall_stats())
        halo.close()
        sp.close()
        return res
    parts = _run_ranks(S["world"], body)
    if S["hub"] is not None:
        S["hub"].close()
    for p in parts:
        rows = p["st"]["nsend_rows"]
        assert p["st"]["forward_bytes_per_step"] == (7 * 8 * rows if S["world"] > 1 else 0)    # nothing new travels
    n = S["x"].shape[0]
    X, V, Q, Fg, Tg = _gather(parts, n, ("x", "v", "q", "f", "tq"))
    xr, vr, qr, fr, tr, ncr = _reference(S)
    off = _reference(S, resist=False)
    dx = _wrap(X - xr, S["lo"], S["hi"], PERIODIC)
    ef, et = np.abs(Fg - fr).max() / np.abs(fr).max(), np.abs(Tg - tr).max() / max(np.abs(fr).max(), np.abs(tr).max())
    print(f"grid {grid}: {sum(p['wall_contacts'] for p in parts)} wall contacts (single rank {ncr}); |dx| {np.abs(dx).max():.2e}, "
          f"|dv|/max|v| {np.abs(V - vr).max() / np.abs(vr).max():.2e}, rel |df| {ef:.2e} |dtau| {et:.2e}; "
          f"the resistance moved the torques by {np.abs(tr - off[4]).max():.3e} of {np.abs(tr).max():.3e}")
    assert sum(p["wall_contacts"] for p in parts) == ncr and ncr > 10
    assert np.abs(tr - off[4]).max() > 1e-3 * np.abs(tr).max()                    # it acts on this bed
    assert np.abs(dx).max() < 1e-7 and np.abs(V - vr).max() < 1e-6 * np.abs(vr).max()
    assert np.abs(np.abs((Q * qr).sum(1)) - 1).max() < 1e-9
    assert ef < 1e-6 and et < 1e-6


def test_the_loop_refuses_without_the_option():
    from shpair import mrank, ShPairError
    from shpair.capi import HaloArrays, HaloRunParams
    S = _setup((1, 1, 1), PERIODIC, nbed=NBED)
    sp = _ctx(LMAX, S["shp"], NQ)
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), S["lo"], S["hi"], PERIODIC, SKIN)
    sp.set_walls(*_walls(S))
    sp.wall_twisting(*TWIST)
    with pytest.raises(ShPairError, match="halo_twists") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -1
    sp.wall_twisting(0.0, 0.0)
    sp.wall_rolling(*ROLL)
    with pytest.raises(ShPairError, match="halo_twists") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -1
    halo.close()
    sp.close()
