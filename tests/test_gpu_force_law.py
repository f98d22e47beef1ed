"""Every branch of the force law (docs/SPEC.md §2.7) against references.

The epilogues of both contact-kernel families form V^(m-1) with pow_quarter (wave_ops.hpp): seven hand-written branches
for m - 1 = 0.25, 0.5, 0.75, 1, 1.25, 1.5, 2 built on sqrt_nr, and pow() for every other exponent.  The exponent set M
below puts every branch and the fall-back on touching pairs:

  1. isolated pairs, where every atom's force, torque and per-atom tallies are ONE contribution: the epilogue's outputs
     against the force law evaluated with 40 digits (mpmath) from the per-slot rows (V, S_n, T_n) of the same compute,
     at 1e-12 of the pair's largest |F| (|tau|, E).  The hand-written branches are a few sqrt_nr at 1-2 ulp and under
     ten multiplies, ~1e-15; a wrong branch is an O(1) error.  Once per epilogue and instance, newton on and off (with
     ghost rows), deterministic mode off and on.
  2. beds of three types whose exponent table is drawn from M, against the oracle at the suite's 1e-9.

The rows themselves are held to references elsewhere (test_gpu_parity.py, test_gpu_pair_ref.py, ...); this file holds
what is built on them.  The isolated-pair scene has 288 pairs, not the 240 of the other soups: about 73 % of a soup's
pairs touch, and ten exponents on 20 touching pairs each need 200.
"""
import numpy as np
import pytest

from common import make_case, make_soup, coeff_tables, oracle_compute, rel_err
from test_gpu_parity import make_ctx

pytestmark = pytest.mark.gpu
TOL = 1e-9            # the suite's gate against the oracle
GATE = 1e-12          # the epilogue against the extended-precision force law
M = (1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 3.0, 1.3, 4.0 / 3.0)
NTYPES = 4
TYPE_PAIRS = [(a, b) for a in range(1, NTYPES + 1) for b in range(a, NTYPES + 1)]   # ten unordered pairs: one per exponent
NPAIR = 288
VIR = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))     # xx yy zz xy xz yz

assert len(TYPE_PAIRS) == len(M)


def soup_tables():
    """kn and exponent of the four types: type pair k of TYPE_PAIRS has the exponent M[k], both ways round."""
    K = np.zeros((NTYPES + 1, NTYPES + 1))
    E = np.ones((NTYPES + 1, NTYPES + 1))
    for k, (a, b) in enumerate(TYPE_PAIRS):
        K[a, b] = K[b, a] = 600.0 + 70.0 * k
        E[a, b] = E[b, a] = M[k]
    return K, E


_SCENES = {}


def soup_scene(oracle, lmax, nq, rule):
    """make_soup with the types assigned from the oracle's rows: the touching pairs go round the ten type pairs in turn
    (and so do the others), every second one with the types of i and j swapped.  Returns the scene and the number of
    touching pairs per exponent, counted from the oracle."""
    key = (lmax, nq, rule)
    if key in _SCENES:
        return _SCENES[key]
    s = make_soup(lmax, oracle.shape_rmax, NPAIR)
    n = 2 * NPAIR
    K1, E1 = coeff_tables(1, 1000.0, 1.25)
    oracle.set_rule("weighted" if rule else "sharp")
    try:
        o = oracle.compute([(lmax, a, r) for a, r in zip(s["shapes"], s["rmax"])], K1, E1, nq, n, s["x"], s["quat"], s["type"],
                           s["shtype"], s["ilist"], s["offsets"], s["jlist"], want_pairs=True, force_volume=True)
    finally:
        oracle.set_rule("sharp")
    touching = o["pairs"][:, 0] > 0
    ty = np.ones(n, np.int32)
    kind = np.zeros(NPAIR, int)
    for mask in (touching, ~touching):
        for c, p in enumerate(np.nonzero(mask)[0]):
            k = c % len(M)
            a, b = TYPE_PAIRS[k] if (c // len(M)) % 2 == 0 else TYPE_PAIRS[k][::-1]
            ty[2 * p], ty[2 * p + 1] = a, b
            kind[p] = k
    s = dict(s, type=ty)
    counts = {M[k]: int((touching & (kind == k)).sum()) for k in range(len(M))}
    _SCENES[key] = (s, counts)
    return _SCENES[key]


def arrange(s, ghosts):
    """The soup as (x, quat, type, shtype, nlocal, ilist, offsets, jlist, pi, pj): pi, pj are the atoms of slot p.  With
    `ghosts` the second atom of every third pair is moved behind the owned rows, where a newton-off compute leaves it
    alone."""
    n = 2 * NPAIR
    if not ghosts:
        return dict(x=s["x"], quat=s["quat"], type=s["type"], shtype=s["shtype"], nlocal=n, ilist=s["ilist"],
                    offsets=s["offsets"], jlist=s["jlist"], pi=np.arange(0, n, 2), pj=np.arange(1, n, 2))
    gh = np.array([2 * p + 1 for p in range(NPAIR) if p % 3 == 2])
    order = np.concatenate([np.setdiff1d(np.arange(n), gh), gh])
    new = np.empty(n, int)
    new[order] = np.arange(n)
    nlocal = n - gh.size
    has_row = order[:nlocal] % 2 == 0                       # the first atom of each pair lists the second
    of = np.zeros(nlocal + 1, np.int32)
    of[1:] = np.cumsum(has_row)
    pi, pj = new[np.arange(0, n, 2)], new[np.arange(1, n, 2)]
    assert np.all(np.diff(pi) > 0)                          # slot p is still pair p
    return dict(x=s["x"][order], quat=s["quat"][order], type=s["type"][order], shtype=s["shtype"][order], nlocal=nlocal,
                ilist=np.arange(nlocal, dtype=np.int32), offsets=of, jlist=pj.astype(np.int32), pi=pi, pj=pj)


def force_law_deviations(rows, a, K, E, newton, got):
    """The force law of SPEC §2.7 from the rows (V, S_n, T_n) with 40 digits:

      F_i = -kn m V^(m-1) S_n,  tau_i = -kn m V^(m-1) T_n,  F_j = -F_i,  tau_j = -tau_i - d x F_j,  E = sum kn V^m,
      virial = -d (x) F_i, and half of a pair's energy and virial per atom; with newton off a ghost j gets nothing and
      the pair counts half in the global sums.

    `got` = (f, torque, eng, vir, eatom, vatom) of the compute.  Returns ({m: worst deviation of f, torque, eatom, vatom
    over the pairs with that exponent, each relative to the pair's largest |F|, |tau|, E, |virial|}, deviation of the
    energy, of the virial, number of touching pairs); atoms of pairs that do not touch must hold exact zeros."""
    import mpmath as mp
    mp.mp.dps = 40
    f, tq, eng, vir, ea, va = got
    x, ty, nlocal = a["x"], a["type"], a["nlocal"]
    worst = {m: 0.0 for m in M}
    etot, vtot = mp.mpf(0), [mp.mpf(0)] * 6
    ntouch = 0

    def dev(values, want, scale):
        return float(max(abs(mp.mpf(float(g)) - w) for g, w in zip(values, want)) / scale)

    for p in range(rows.shape[0]):
        i, j = int(a["pi"][p]), int(a["pj"][p])
        jown = newton or j < nlocal
        V = mp.mpf(float(rows[p, 0]))
        if not V > 0:
            assert not f[i].any() and not f[j].any() and not tq[i].any() and not tq[j].any()
            assert ea[i] == 0.0 and ea[j] == 0.0 and not va[i].any() and not va[j].any()
            continue
        ntouch += 1
        kn, m = mp.mpf(float(K[ty[i], ty[j]])), mp.mpf(float(E[ty[i], ty[j]]))
        pn = kn * m * V ** (m - 1)
        Fi = [-pn * mp.mpf(float(v)) for v in rows[p, 1:4]]
        Ti = [-pn * mp.mpf(float(v)) for v in rows[p, 4:7]]
        d = [mp.mpf(float(x[j, c])) - mp.mpf(float(x[i, c])) for c in range(3)]
        Fj = [-v for v in Fi]
        dxF = [d[1] * Fj[2] - d[2] * Fj[1], d[2] * Fj[0] - d[0] * Fj[2], d[0] * Fj[1] - d[1] * Fj[0]]
        Tj = [-Ti[c] - dxF[c] for c in range(3)]
        epair = kn * V ** m
        vpair = [-d[c] * Fi[b] for c, b in VIR]
        share = mp.mpf(1) if jown else mp.mpf("0.5")
        etot += share * epair
        vtot = [t + share * v for t, v in zip(vtot, vpair)]
        fs, ts, vs = max(abs(v) for v in Fi), max(abs(v) for v in Ti + Tj), max(abs(v) for v in vpair)
        zero3, zero6 = [mp.mpf(0)] * 3, [mp.mpf(0)] * 6
        w = max(dev(f[i], Fi, fs), dev(tq[i], Ti, ts),
                dev(f[j], Fj if jown else zero3, fs), dev(tq[j], Tj if jown else zero3, ts),
                dev([ea[i]], [epair / 2], epair), dev([ea[j]], [epair / 2 if jown else 0], epair),
                dev(va[i], [v / 2 for v in vpair], vs), dev(va[j], [v / 2 for v in vpair] if jown else zero6, vs))
        mm = float(E[ty[i], ty[j]])
        worst[mm] = max(worst[mm], w)
    de = float(abs(mp.mpf(float(eng)) - etot) / etot)
    dv = dev(vir, vtot, max(abs(v) for v in vtot))
    return worst, de, dv, ntouch


INSTANCES = [
    # id, L, n_q, options, weighted rule, what kernel_info() must report
    ("tail-4-10", 4, 10, {}, 0, dict(family=1, waves_per_pair=1, compiled_order=1, specialised=1)),
    ("tail-5-9", 5, 9, {"jpoly": 1}, 0, dict(family=1, waves_per_pair=1, compiled_order=1, specialised=0)),
    ("phase1-6-16-spec", 6, 16, {"spec": 1}, 0, dict(family=1, waves_per_pair=1, compiled_order=1, specialised=1)),
    ("phase1-6-16-general", 6, 16, {"spec": 0}, 0, dict(family=1, waves_per_pair=1, compiled_order=1, specialised=0)),
    ("two-waves-8-16", 8, 16, {"jpoly": 1, "split": 1}, 0, dict(family=1, waves_per_pair=2, compiled_order=1)),
    ("body-6-16", 6, 16, {"jpoly": 0}, 0, dict(family=0, waves_per_pair=1, compiled_order=1)),
    ("loop-14-8", 14, 8, {}, 0, dict(compiled_order=0, waves_per_pair=1)),
    ("weighted-5-9", 5, 9, {"rule": 1}, 1, dict(weighted=1, waves_per_pair=1, compiled_order=1)),
]


@pytest.mark.parametrize("name,lmax,nq,opts,rule,info", INSTANCES, ids=[c[0] for c in INSTANCES])
def test_epilogue_matches_the_extended_precision_force_law_on_isolated_pairs(oracle, name, lmax, nq, opts, rule, info):
    import torch
    s, counts = soup_scene(oracle, lmax, nq, rule)
    print(f"{name}: touching pairs per exponent (oracle) {counts}")
    assert min(counts.values()) >= 20, counts
    K, E = soup_tables()
    n = 2 * NPAIR
    for newton in (True, False):
        a = arrange(s, ghosts=not newton)
        for det in (0, 1):
            case = dict(lmax=lmax, shapes=s["shapes"], ilist=a["ilist"], offsets=a["offsets"], jlist=a["jlist"])
            sp = make_ctx(case, nq, K, E)
            for k, v in opts.items():
                sp.set_option(k, v)
            sp.set_option("deterministic", det)
            rows = torch.zeros(NPAIR, 7, dtype=torch.float64, device="cuda:0")
            sp.set_pair_output(rows.data_ptr())
            ea, va = np.zeros(n), np.zeros((n, 6))
            sp.set_peratom_host(ea, va)
            f, tq, eng, vir = sp.compute(a["nlocal"], a["x"], a["quat"], a["type"], a["shtype"], newton_pair=newton,
                                         eflag=True, vflag=True)
            ki = sp.kernel_info()
            sp.set_pair_output(None)
            sp.set_peratom_host(None, None)
            sp.close()
            assert ki["lmax"] == lmax and ki["needv"] == 1 and ki["weighted"] == rule and ki["scratch_bytes"] == 0, ki
            assert {k: ki[k] for k in info} == info, ki
            worst, de, dv, ntouch = force_law_deviations(rows.cpu().numpy(), a, K, E, newton, (f, tq, eng, vir, ea, va))
            print(f"{name} newton {int(newton)} deterministic {det}: {ntouch} touching, worst deviation per exponent "
                  + " ".join(f"{m:.4g}:{w:.1e}" for m, w in worst.items()) + f" energy {de:.1e} virial {dv:.1e}")
            assert ntouch == sum(counts.values())          # the GPU rows touch where the oracle's do: its count
            assert max(worst.values()) < GATE, worst
            assert de < GATE and dv < GATE, (de, dv)
            if not newton:
                assert not f[a["nlocal"]:].any() and not tq[a["nlocal"]:].any() and not ea[a["nlocal"]:].any()


BEDS = [
    # L, n_q, the six exponents of the three types' pairs (11, 12, 13, 22, 23, 33): every member of M is on two beds or more
    (4, 10, (1.0, 1.25, 1.75, 2.25, 1.3, 3.0)),
    (6, 16, (1.5, 1.75, 2.0, 2.5, 4.0 / 3.0, 1.3)),
    (14, 8, (1.75, 2.0, 2.25, 1.5, 3.0, 4.0 / 3.0)),
]

assert all(set(b[2]) <= set(M) for b in BEDS) and set().union(*(b[2] for b in BEDS)) == set(M)


@pytest.mark.parametrize("lmax,nq,expos", BEDS, ids=[f"{b[0]}-{b[1]}" for b in BEDS])
def test_mixed_exponent_bed_matches_oracle(oracle, lmax, nq, expos):
    """A bed of three types, every type pair with its own exponent and stiffness: forces, torques, energy, virial, the
    per-atom tallies and the per-slot rows against the oracle."""
    import torch
    case = make_case(150, lmax, 2, seed=1200 + lmax, ntypes=3, rmax_fn=oracle.shape_rmax)
    pairs3 = [(a, b) for a in (1, 2, 3) for b in range(a, 4)]
    table = {p: m for p, m in zip(pairs3, expos)}
    K, E = coeff_tables(3, kn=lambda i, j: 400.0 + 90.0 * (i + j), expo=lambda i, j: table[(min(i, j), max(i, j))])
    b = case["bed"]
    n = case["n"]
    o = oracle_compute(oracle, case, nq, K, E, eflag=True, vflag=True, want_pairs=True, want_peratom=True, nthreads=8)
    # touching slots per exponent, from the oracle's rows
    ii = np.repeat(case["ilist"], np.diff(case["offsets"]))
    m_slot = E[b["type"][ii], b["type"][case["jlist"]]]
    counts = {m: int(((m_slot == m) & (o["pairs"][:, 0] > 0)).sum()) for m in expos}
    print(f"L {lmax} n_q {nq}: touching slots per exponent (oracle) {counts}")
    assert min(counts.values()) >= 30, counts
    sp = make_ctx(case, nq, K, E)
    sp.set_option("count", 1)
    rows = torch.zeros(case["jlist"].size, 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(rows.data_ptr())
    ea, va = np.zeros(n), np.zeros((n, 6))
    sp.set_peratom_host(ea, va)
    f, tq, eng, vir = sp.compute(n, b["x"], b["quat"], b["type"], b["shtype"], eflag=True, vflag=True)
    ki, st = sp.kernel_info(), sp.stats()
    sp.set_pair_output(None)
    sp.set_peratom_host(None, None)
    sp.close()
    assert ki["lmax"] == lmax and ki["needv"] == 1 and ki["compiled_order"] == (0 if lmax > 12 else 1), ki
    fs = np.abs(o["f"]).max()
    ts = max(fs, np.abs(o["torque"]).max())
    pscale = np.abs(o["pairs"]).max(axis=0)
    dev = dict(f=rel_err(f, o["f"], fs), torque=rel_err(tq, o["torque"], ts),
               energy=abs(eng - o["eng_virial"][0]) / abs(o["eng_virial"][0]),
               virial=rel_err(vir, o["eng_virial"][1:]), eatom=rel_err(ea, o["eatom"]), vatom=rel_err(va, o["vatom"]),
               rows=(np.abs(rows.cpu().numpy() - o["pairs"]) / pscale).max())
    print(f"L {lmax} n_q {nq}: " + " ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    assert fs > 0 and max(dev.values()) < TOL, dev
    assert (st["n_candidates"], st["n_contact"], st["n_touching"]) == tuple(o["counts"])
