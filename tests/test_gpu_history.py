"""GPU tests of the tangential contact springs with history of docs/SPEC.md §2.14 (csrc/history_kernels.hpp through the
C ABI of include/shstep.h) against tests/history_ref.py fed by the ORACLE's per-pair integrals: the pass, the look with
dt = 0, stick / slip / hold in closed form, the carry across a rebuild, the three loops, the ledger, and off is off.
L = 4, n_q = 8 unless stated.

The coefficients, seeds and beds below were chosen on the CPU, with the oracle, tests/history_ref.py and
tests/step_ref.py alone, so that the conditions the tests assert on their INPUTS hold."""
import numpy as np
import pytest

from common import coeff_tables, oracle_compute
from dissipation_common import NQ, dev, bed_case, motion, _total_energy

pytestmark = pytest.mark.gpu

TOL = 1e-9            # tests/test_gpu_friction.py's: of the largest force, SPEC §4
GAMMA = {(1, 1): 300.0, (1, 2): 900.0, (2, 2): 1800.0}
FRIC = {(1, 1): (2.0, 300.0), (1, 2): (1.5, 400.0), (2, 2): (2.5, 250.0)}      # (mu, gamma_t)
SPRING = {(1, 1): 4.0e4, (1, 2): 3.0e4}                                        # k_t; type pair (2, 2) keeps §2.11
DT = 1e-3
XI_SCALE = 0.01
N_BED, BED_SEED, NLOCAL, MOTION_SEED, XI_SEED = 150, 4, 110, 11, 3


def table(coef, k=None):
    G = np.zeros((3, 3))
    for (a, b), g in coef.items():
        G[a, b] = G[b, a] = g if k is None else g[k]
    return G


# ---- the bed of tests 1, 2 and 7: tests/test_gpu_friction.py's largest, its list built on the device -----------------

def _bed_ctx(case, K, E, det=0, gamma=GAMMA, fric=FRIC, spring=SPRING):
    """A context with the case's shapes and coefficients and a box around the bed; no list yet."""
    from shpair import ShPair
    sp = ShPair(0)
    sp.settings(NQ)
    sp.set_ntypes(2, len(case["shapes"]))
    for s, a in enumerate(case["shapes"]):
        sp.set_shape(s, case["lmax"], a)
    for i in (1, 2):
        for j in (1, 2):
            sp.coeff(i, j, K[i, j], E[i, j])
    if det:
        sp.set_option("deterministic", 1)
    for (a, b), g in (gamma or {}).items():
        sp.pair_damping(a, b, g)
    for (a, b), (mu, gt) in (fric or {}).items():
        sp.pair_friction(a, b, mu, gt)
    for (a, b), kt in (spring or {}).items():
        sp.set_pair_tangential_spring(a, b, kt)
    x = case["bed"]["x"]
    sp.set_box(x.min(axis=0) - 1.0, x.max(axis=0) + 1.0, (0, 0, 0), 0.1)
    return sp


class _Bed:
    """The case's rows on the device, the device-built half list of its first nlocal rows (the rows behind are a host's
    own ghosts with tags of their own), one compute and the twists of all rows."""

    def __init__(self, sp, case, v, L, nlocal, newton):
        import torch
        b, n = case["bed"], case["n"]
        self.sp, self.n, self.nlocal, self.newton = sp, n, nlocal, newton
        self.x, self.q = dev(b["x"]), dev(b["quat"])
        self.ty, self.sh = dev(b["type"].astype(np.int32)), dev(b["shtype"].astype(np.int32))
        self.tag = dev(np.arange(n, dtype=np.int32))
        self.np = sp.neighbor_build_device(nlocal, n - nlocal, self.x.data_ptr(), self.sh.data_ptr(), tag=self.tag.data_ptr())
        self.offs, self.jl = sp.copy_neighbors(nlocal, self.np)
        self.f, self.tq = (torch.zeros(n, 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
        self.tw = torch.zeros(n, 6, dtype=torch.float64, device="cuda:0")
        self.compute()
        vd, Ld = dev(v), dev(L)                 # (kept until the kernel has run)
        sp.twist_device(n, 0, vd.data_ptr(), self.q.data_ptr(), Ld.data_ptr(), self.sh.data_ptr(), self.tw.data_ptr())
        torch.cuda.synchronize()
        sp.synchronize()

    def build(self):
        return self.sp.neighbor_build_device(self.nlocal, self.n - self.nlocal, self.x.data_ptr(), self.sh.data_ptr(),
                                             tag=self.tag.data_ptr())

    def compute(self):
        """The elastic forces of the installed list into f, torque (from zero)."""
        import torch
        self.f.zero_()
        self.tq.zero_()
        torch.cuda.synchronize()
        self.sp.compute_device(self.nlocal, self.n - self.nlocal, self.x.data_ptr(), self.q.data_ptr(), self.ty.data_ptr(),
                               self.sh.data_ptr(), self.f.data_ptr(), self.tq.data_ptr(), newton_pair=self.newton)
        torch.cuda.synchronize()
        self.sp.synchronize()

    def pass_(self, dt=None, call="contact"):
        """The wrench one pass adds to the elastic forces (f, torque of the compute stay as they are)."""
        import torch
        f, tq = self.f.clone(), self.tq.clone()
        a = (self.nlocal, self.n - self.nlocal, self.x.data_ptr(), self.ty.data_ptr(), self.sh.data_ptr(), self.tw.data_ptr(),
             f.data_ptr(), tq.data_ptr())
        if call == "contact":
            self.sp.pair_contact_device(*a, dt, newton_pair=self.newton)
        else:
            self.sp.pair_dissipation_device(*a, newton_pair=self.newton)
        torch.cuda.synchronize()
        self.sp.synchronize()
        return (f - self.f).cpu().numpy(), (tq - self.tq).cpu().numpy(), f.cpu().numpy(), tq.cpu().numpy()


_refs = {}


def history_inputs(oracle, newton, expo=1.25):
    """The bed, its motion, a random xi and the reference's answers for dt = DT and dt = 0: computed once per newton_pair
    and exponent, shared, never changed.  The list is the §7 half list of the first NLOCAL rows (tests/step_ref.py), which the tests
    check the device's against."""
    import damp_ref as D
    import history_ref as H
    import step_ref as SR
    key = (newton, expo)
    if key not in _refs:
        case = dict(bed_case(oracle, N_BED, BED_SEED))
        b, n = case["bed"], case["n"]
        offs, jl = SR.half_list(NLOCAL, b["x"], b["shtype"], np.arange(n), np.asarray(case["rmax"]), 0.1)
        case["ilist"], case["offsets"], case["jlist"] = np.arange(NLOCAL, dtype=np.int32), offs, jl
        K, E = coeff_tables(2, lambda i, j: 1000.0 + 100.0 * (i + j), expo)
        v, L = motion(case, MOTION_SEED)
        o = oracle_compute(oracle, case, NQ, K, E, nlocal=NLOCAL, newton_pair=newton, force_volume=True, want_pairs=True)
        pi, pj = D.expand(case["ilist"], offs, jl)
        tw = D.twists(case["massprops"], [1.0, 1.0], v, b["quat"], L, b["shtype"])
        xi = XI_SCALE * np.random.default_rng(XI_SEED).normal(size=(jl.size, 3))
        a = (o["pairs"], pi, pj, b["x"], tw, b["type"], b["shtype"], case["rmax"], K, E, table(GAMMA), table(FRIC, 0), table(FRIC, 1),
             table(SPRING), xi)
        step = H.pair_history(*a, DT, NLOCAL, newton_pair=newton)
        look = H.pair_history(*a, 0.0, NLOCAL, newton_pair=newton)
        _refs[key] = dict(case=case, K=K, E=E, v=v, L=L, o=o, xi=xi, step=step, look=look, offs=offs, jl=jl)
    return _refs[key]


def input_conditions(r):
    import history_ref as H
    det = r["step"][3]
    kind = det["kind"]
    live = np.isin(kind, (H.STICK, H.SLIDE))
    near = np.abs(det["trial"][live] - det["cap"][live]) / det["cap"][live]
    return dict(slots=int(kind.size), stick=int((kind == H.STICK).sum()), slide=int((kind == H.SLIDE).sum()),
                untouched=int((kind == H.RESET_UNTOUCHED).sum()), guard=int((kind == H.RESET_GUARD).sum()),
                no_history=int((kind == H.NONE).sum()), nearest=float(near.min()))


def assert_input_conditions(c):
    assert c["slots"] > 256 and c["slots"] % 256 != 0, c
    assert c["stick"] >= 10 and c["slide"] >= 10 and c["untouched"] >= 10, c
    assert c["nearest"] > 1e-6, c                 # no slot within 1e-6 relative of the branch |F*| = mu N


# ---- 1. the pass against the reference ----------------------------------------------------------------------------------

@pytest.mark.parametrize("newton", [True, False])
@pytest.mark.parametrize("det", [0, 1])
def test_contact_pass_matches_the_reference_on_oracle_integrals(oracle, newton, det):
    _contact_pass_against_the_reference(oracle, newton, det, 1.25)


@pytest.mark.parametrize("expo,newton,det", [(1.75, True, 0), (1.75, False, 1), (2.5, True, 0), (2.5, False, 1), (1.3, True, 0),
                                             (1.3, False, 1)])
def test_contact_pass_matches_the_reference_at_exponents_that_take_pow(oracle, expo, newton, det):
    """V^(m-1) of the pass is pow() (m - 1 = 0.75, 1.5, 0.3): it feeds the damping clamp and the cap mu N."""
    _contact_pass_against_the_reference(oracle, newton, det, expo)


def _contact_pass_against_the_reference(oracle, newton, det, expo):
    r = history_inputs(oracle, newton, expo)
    cond = input_conditions(r)
    print(f"m={expo} newton={newton} det={det}: inputs {cond}")
    assert_input_conditions(cond)
    sp = _bed_ctx(r["case"], r["K"], r["E"], det=det)
    bed = _Bed(sp, r["case"], r["v"], r["L"], NLOCAL, newton)
    assert np.array_equal(bed.offs, r["offs"]) and np.array_equal(bed.jl, r["jl"])
    sp.set_contact_history(NLOCAL, r["xi"])
    assert np.array_equal(sp.contact_history(NLOCAL), r["xi"])
    df, dt_, f1, _ = bed.pass_(DT)
    xi1 = sp.contact_history(NLOCAL)
    sp.close()
    rf, rt, rxi, rdet = r["step"]
    o = r["o"]
    scale = np.abs(o["f"] + rf).max()
    tscale = max(scale, np.abs(o["torque"] + rt).max())
    vt = np.where(np.isnan(rdet["vt"]), 0.0, rdet["vt"])
    xscale = (np.linalg.norm(r["xi"], axis=1) + DT * np.linalg.norm(vt, axis=1)).max()
    ef, et = np.abs(df - rf).max() / scale, np.abs(dt_ - rt).max() / tscale
    ex = np.abs(xi1 - rxi).max() / xscale
    e0 = np.abs((f1 - df) - o["f"]).max() / scale
    print(f"  max|F| {scale:.4g}, max|dF| {np.abs(rf).max():.4g}, rel err dF {ef:.1e} dtau {et:.1e} xi {ex:.1e} elastic {e0:.1e}")
    assert np.abs(rf).max() > 0.05 * scale
    assert e0 <= TOL and ef <= TOL and et <= TOL
    assert ex <= TOL
    import history_ref as H
    dead = ~np.isin(rdet["kind"], (H.STICK, H.SLIDE))
    assert not xi1[dead].any() and np.abs(r["xi"][dead]).min() > 0      # resets are exact zeros
    if not newton:
        assert not df[NLOCAL:].any() and not dt_[NLOCAL:].any()
    else:
        assert np.abs(df[NLOCAL:]).max() > 0                            # ghost j rows got their share


# ---- 2. dt = 0 is a look -------------------------------------------------------------------------------------------------

def test_a_pass_with_dt_zero_writes_nothing_and_gives_the_reference_forces(oracle):
    r = history_inputs(oracle, True)
    sp = _bed_ctx(r["case"], r["K"], r["E"], det=1)
    bed = _Bed(sp, r["case"], r["v"], r["L"], NLOCAL, True)
    sp.set_contact_history(NLOCAL, r["xi"])
    df, dt_, _, _ = bed.pass_(0.0)
    xi1 = sp.contact_history(NLOCAL)
    sp.close()
    rf, rt, rxi, _ = r["look"]
    assert np.array_equal(xi1, r["xi"]) and np.array_equal(rxi, r["xi"])
    scale = np.abs(r["o"]["f"] + rf).max()
    tscale = max(scale, np.abs(r["o"]["torque"] + rt).max())
    print(f"dt = 0: rel err dF {np.abs(df - rf).max() / scale:.1e} dtau {np.abs(dt_ - rt).max() / tscale:.1e}; "
          f"against the dt > 0 forces {np.abs(rf - r['step'][0]).max() / scale:.1e}")
    assert np.abs(df - rf).max() <= TOL * scale and np.abs(dt_ - rt).max() <= TOL * tscale
    assert np.abs(rf - r["step"][0]).max() > 1e-3 * scale            # the two references differ: the test can tell them apart


# ---- 3. stick, slip, hold in closed form ---------------------------------------------------------------------------------

def test_two_spheres_stick_then_slide_then_hold_a_load_at_rest(oracle):
    """tests/test_history_ref.py's sequence through the real pass: two unit spheres (L = 0) 1.9 apart along x, a constant
    tangential velocity of sphere 0.  N = p |S_n| is the elastic force of the pair itself."""
    import torch
    from shpair import ShPair, shapes
    from test_history_ref import MU, KT, GT, VT
    sp = ShPair(0)
    sp.settings(NQ)
    sp.set_ntypes(1, 1)
    sp.set_shape(0, 0, shapes.sphere(1.0), 1.01)
    sp.coeff(1, 1, 1e4, 1.25)
    sp.pair_friction(1, 1, MU, GT)
    sp.set_pair_tangential_spring(1, 1, KT)
    sp.set_box((-3, -3, -3), (5, 3, 3), (0, 0, 0), 0.1)
    x, q = dev(np.array([[0.0, 0, 0], [1.9, 0, 0]])), dev(np.array([[1.0, 0, 0, 0]] * 2))
    ty, sh = dev(np.ones(2, np.int32)), dev(np.zeros(2, np.int32))
    assert sp.neighbor_build_device(2, 0, x.data_ptr(), sh.data_ptr()) == 1
    f0, t0 = torch.zeros(2, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(2, 3, dtype=torch.float64, device="cuda:0")
    sp.compute_device(2, 0, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f0.data_ptr(), t0.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    N = abs(float(f0[0, 0].item()))
    tn = max(float(t0.abs().max().item()) / N, 1e-16)       # the sphere's own T_n is rounding of the quadrature

    def one(tw):
        f, tq = f0.clone(), t0.clone()
        sp.pair_contact_device(2, 0, x.data_ptr(), ty.data_ptr(), sh.data_ptr(), tw.data_ptr(), f.data_ptr(), tq.data_ptr(), DT)
        torch.cuda.synchronize()
        sp.synchronize()
        return (f - f0).cpu().numpy(), sp.contact_history(2)[0]

    moving, rest = dev(np.array([[*VT, 0, 0, 0], [0.0] * 6])), dev(np.zeros((2, 6)))
    tol = TOL * N + 10 * tn * (MU * N + GT * np.linalg.norm(VT))
    kslip, held = None, None
    for k in range(1, 160):
        df, xi = one(moving)
        trial = -KT * (k * DT * VT) - GT * VT
        if kslip is None and np.linalg.norm(trial) <= MU * N * (1 - 1e-6):
            assert np.abs(df[0] - trial).max() <= tol and np.abs(xi - k * DT * VT).max() <= TOL * k * DT
        elif kslip is None and np.linalg.norm(trial) < MU * N * (1 + 1e-6):
            pytest.fail("a step within 1e-6 of the branch: choose other inputs")
        else:
            kslip = kslip or k
            assert abs(np.linalg.norm(df[0]) - MU * N) <= tol
            hold = (MU * N - GT * np.linalg.norm(VT)) / KT
            assert abs(np.linalg.norm(xi) - hold) <= TOL * hold + tol / KT          # xi no longer grows
        assert np.abs(df[0] + df[1]).max() <= 1e-12 * MU * N
        held = xi
    assert kslip is not None and 10 < kslip < 150
    df, xi = one(rest)                                        # at rest the spring holds its load: history-free friction gives 0
    sp.close()
    print(f"N {N:.6g}, mu N {MU * N:.6g}, first sliding pass {kslip}, held |F_t| {np.linalg.norm(df[0]):.6g}")
    assert np.abs(df[0] + KT * held).max() <= tol and np.linalg.norm(df[0]) > 0.5 * MU * N
    assert np.abs(xi - held).max() <= TOL * np.abs(held).max()


# ---- 4. carry across a rebuild ---------------------------------------------------------------------------------------------

CARRY_N, CARRY_SHIFT, CARRY_JITTER, CARRY_SEED, CARRY_SKIN = 300, np.array([0.9, -0.7, 0.5]), 0.06, 6, 0.15


def carry_bed():
    """A periodic hcp bed, explicit tags (a permutation), and the positions of the second build: shifted and perturbed."""
    from shpair import shapes, bed
    shp = [shapes.random_shape(4, 4000 + 17 * s + 4, amp=0.2) for s in range(2)]
    pts, lo, hi = bed.periodic_hcp(CARRY_N, 1.9, (1, 1, 1))
    rng = np.random.default_rng(CARRY_SEED)
    n = pts.shape[0]
    x0 = pts + rng.uniform(-0.05, 0.05, pts.shape)
    x1 = x0 + CARRY_SHIFT + rng.uniform(-CARRY_JITTER, CARRY_JITTER, pts.shape)
    tag = (rng.permutation(n) + 1).astype(np.int32)
    return dict(shapes=shp, lo=np.asarray(lo, float), hi=np.asarray(hi, float), n=n, x0=x0, x1=x1, tag=tag,
                quat=bed.random_quaternions(n, rng), shtype=(np.arange(n) % 2).astype(np.int32))


def carry_reference(c, rmax):
    """From tests/step_ref.py alone, with the oracle's bounding radii of the shapes (rmax, computed on the host): for both
    position sets the dict (i, owner tag of j) -> j is a ghost row."""
    import step_ref as SR
    cmax = 2 * max(rmax) + CARRY_SKIN
    out = []
    for x in (c["x0"], c["x1"]):
        ln = c["hi"] - c["lo"]
        xw = x - np.floor((x - c["lo"]) / ln) * ln
        own, code = SR.images(xw, c["lo"], c["hi"], (1, 1, 1), cmax)
        xa = np.concatenate([xw, xw[own] + SR.shift_of(code) * ln])
        sh, tg = np.concatenate([c["shtype"], c["shtype"][own]]), np.concatenate([c["tag"], c["tag"][own]])
        offs, jl = SR.half_list(c["n"], xa, sh, tg, np.asarray(rmax), CARRY_SKIN)
        pi = np.repeat(np.arange(c["n"]), np.diff(offs))
        out.append({(int(i), int(tg[j])): bool(j >= c["n"]) for i, j in zip(pi, jl)})
    old, new = out
    both = set(old) & set(new)
    return dict(to_ghost=sum(1 for k in both if not old[k] and new[k]), to_owned=sum(1 for k in both if old[k] and not new[k]),
                vanished=len(set(old) - set(new)), new=len(set(new) - set(old)), kept=len(both))


def test_xi_follows_its_pair_across_a_rebuild_and_a_changed_nlocal_zeroes_it(oracle):
    import torch
    from shpair import ShPair
    c = carry_bed()
    n = c["n"]
    sp = ShPair(0)
    sp.settings(NQ)
    sp.set_ntypes(1, 2)
    for s, a in enumerate(c["shapes"]):
        sp.set_shape(s, 4, a)
    sp.coeff(1, 1, 1000.0, 1.25)
    sp.pair_friction(1, 1, 0.5, 100.0)
    sp.set_pair_tangential_spring(1, 1, 1e4)
    rmax = [oracle.shape_rmax(4, a) for a in c["shapes"]]
    kinds = carry_reference(c, rmax)
    print(f"{n} particles, pairs by kind (tests/step_ref.py): {kinds}")
    assert min(kinds["to_ghost"], kinds["to_owned"], kinds["vanished"], kinds["new"]) >= 10, kinds
    sp.set_box(c["lo"], c["hi"], (1, 1, 1), CARRY_SKIN)
    nmax = 8 * n
    x, q = torch.zeros(nmax, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(nmax, 4, dtype=torch.float64, device="cuda:0")
    ty, sh, tag = (torch.ones(nmax, dtype=torch.int32, device="cuda:0") for _ in range(3))
    q[:n], sh[:n], tag[:n] = dev(c["quat"]), dev(c["shtype"]), dev(c["tag"])

    def build(xh, nl):
        x[:nl] = dev(xh[:nl])
        torch.cuda.synchronize()
        ng = sp.borders_device(nl, nmax, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), tag=tag.data_ptr())
        npairs = sp.neighbor_build_device(nl, ng, x.data_ptr(), sh.data_ptr(), tag=tag.data_ptr())
        offs, jl = sp.copy_neighbors(nl, npairs)
        tg = tag[:nl + ng].cpu().numpy()
        pi = np.repeat(np.arange(nl), np.diff(offs))
        return npairs, pi, tg[jl], jl >= nl

    np0, pi0, key0, _ = build(c["x0"], n)
    assert not sp.contact_history(n).any()                            # a first build starts from zero
    g = lambda i, k: np.stack([i + 0.25, -(k + 0.5), (i + 1.0) * (k + 2.0) * 1e-3], axis=1)   # xi = g(i, owner tag): never zero
    xi0 = g(pi0.astype(float), key0.astype(float))
    sp.set_contact_history(n, xi0)
    np1, pi1, key1, ghost1 = build(c["x1"], n)
    xi1 = sp.contact_history(n)
    old = {(int(i), int(k)) for i, k in zip(pi0, key0)}
    assert len(old) == np0                                              # a row holds an owner's tag once
    kept = np.array([(int(i), int(k)) in old for i, k in zip(pi1, key1)])
    assert kept.sum() == kinds["kept"] and (~kept).sum() == kinds["new"] and np0 - kept.sum() == kinds["vanished"]
    assert np.array_equal(xi1[kept], g(pi1[kept].astype(float), key1[kept].astype(float)))     # the old xi, bitwise
    assert not xi1[~kept].any()                                         # new pairs start from zero
    assert ghost1[kept].any() and (~ghost1[kept]).any()
    np2, _, _, _ = build(c["x1"], n - 1)                                # another nlocal: nothing is carried
    assert np2 > 0 and not sp.contact_history(n - 1).any()
    sp.close()


# ---- 5. the loops ------------------------------------------------------------------------------------------------------------

LOOP_STEPS, LOOP_DT = 120, 1e-3


def _loop_run(mode, reset_before=None):
    """mode "step" also returns (k, xi after step k) for the first step k whose neighbour check rebuilt the list.  With
    reset_before = k every xi is zeroed just ahead of step k and the run ends behind it: the rebuild inside that step
    then carries zeros, which is bit for bit what a build that dropped the history would leave."""
    import torch
    from shpair import ShPair, shapes, bed
    from shpair.run import DeviceRun
    shp = [shapes.random_shape(4, 4000 + 17 * s + 4, amp=0.2) for s in range(2)]
    pts, lo, hi = bed.periodic_hcp(60, 1.9, (1, 1, 1))
    rng = np.random.default_rng(4)
    n = pts.shape[0]
    sp = ShPair(0)
    sp.settings(NQ)
    sp.set_ntypes(2, 2)
    for s, a in enumerate(shp):
        sp.set_shape(s, 4, a)
    sp.coeff("*", "*", 1000.0, 1.25)
    sp.set_option("deterministic", 1)
    shtype = (np.arange(n) % 2).astype(np.int32)
    r = DeviceRun(sp, pts + rng.uniform(-0.1, 0.1, pts.shape), bed.random_quaternions(n, rng), shtype, lo, hi, (1, 1, 1), 0.2,
                  type_=1 + (np.arange(n) // 2) % 2, dt=LOOP_DT, pair_friction={("*", "*"): (0.5, 20.0)},
                  pair_spring={("*", "*"): 2.0e3})
    r.v[:] = dev(1.5 * rng.normal(size=(n, 3)))
    r.L[:] = dev(0.3 * rng.normal(size=(n, 3)))
    r.force()
    torch.cuda.synchronize()
    sp.synchronize()
    mass = np.array([sp.body(int(s))[0] for s in shtype])
    p0 = (mass[:, None] * r.v.cpu().numpy()).sum(axis=0)
    b0 = r.builds
    first = None
    if mode == "step":
        for k in range(LOOP_STEPS):
            if k == reset_before:
                sp.reset_contact_history()
            r.step()
            if first is None and r.builds > b0:
                first = (k, r.contact_history().copy(), r.x[:n].cpu().numpy().copy())
            if k == reset_before:
                break
    else:
        r.run_native(LOOP_STEPS, use_graph=(mode == "graph"))
    torch.cuda.synchronize()
    sp.synchronize()
    xi = r.contact_history()
    out = [t.cpu().numpy().copy() for t in (r.x[:n], r.v, r.q[:n], r.L)] + [xi]
    p1 = (mass[:, None] * out[1]).sum(axis=0)
    pscale = np.abs(mass[:, None] * out[1]).sum()
    rebuilds = r.builds - b0
    sp.close()
    return out, rebuilds, np.abs(p1 - p0).max() / pscale, first


def test_the_three_loops_carry_the_same_history_bits_across_a_rebuild(oracle):
    res = {}
    for mode in ("step", "plain", "graph"):
        res[mode] = _loop_run(mode)
        out, reb, dp, _ = res[mode]
        print(f"{mode}: rebuilds {reb}, slots {len(out[4])}, slots with xi != 0 {int(out[4].any(axis=1).sum())}, momentum drift {dp:.2e}")
        assert reb >= 1 and out[4].any()
        assert dp <= 1e-12
    for mode in ("plain", "graph"):
        for a, b in zip(res["step"][0], res[mode][0]):
            assert np.array_equal(a, b), mode
    # Some xi != 0 survives the rebuild.  The final xi cannot show it: the steps behind the last rebuild load the springs
    # again whatever the rebuild left.  So the run is repeated up to its first rebuilding step k with every xi zeroed just
    # ahead of that step.  Up to the rebuild inside step k both runs have the same bits in x, so they build the same list;
    # the repeat's xi behind step k is what a rebuild that zeroed (or mis-keyed) every slot would give, one step's worth
    # from zero: had the run's own rebuild done that, the two would agree in every bit.  A carry that works leaves what the k
    # steps before had loaded.  (That every surviving slot gets exactly its own xi is test 4's.)
    k, xi_kept, x_kept = res["step"][3]
    _, _, _, (k0, xi_zeroed, x_zeroed) = _loop_run("step", reset_before=k)
    assert k0 == k and k >= 5 and xi_kept.shape == xi_zeroed.shape and len(xi_kept) > 0
    differ = (xi_kept != xi_zeroed).any(axis=1)
    big, small = np.linalg.norm(xi_kept, axis=1).max(), np.linalg.norm(xi_zeroed, axis=1).max()
    print(f"first rebuild in step {k}: {int(differ.sum())} of {len(differ)} slots differ from a zeroed rebuild's; max|xi| {big:.3e} "
          f"against {small:.3e}")
    assert np.array_equal(x_kept, x_zeroed)             # the same positions went into the two builds
    assert differ.any()


def _oblique(k, gamma, fric, spring, offset=0.5):
    """tests/test_gpu_ledger.py's two-sphere collision (test_ledger_ref.COLLISION) made oblique: centres offset along y."""
    from shpair import ShPair, shapes
    from shpair.run import DeviceRun
    from test_ledger_ref import COLLISION as c
    sp = ShPair(0)
    sp.settings(c["nq"])
    sp.set_ntypes(1, 1)
    sp.set_shape(0, 0, shapes.sphere(1.0), 1.01)
    sp.coeff(1, 1, c["kn"], c["m"])
    sp.set_option("deterministic", 1)
    x = np.array([[2.99, 4.0 - 0.5 * offset, 4.0], [5.01, 4.0 + 0.5 * offset, 4.0]])
    r = DeviceRun(sp, x, np.array([[1.0, 0, 0, 0]] * 2), np.zeros(2, np.int32), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.3, dt=c["dt"] / k,
                  ledger=True, pair_damping={(1, 1): gamma} if gamma else None, pair_friction=fric, pair_spring=spring)
    r.v[:] = dev(np.array([[0.5 * c["vrel"], 0, 0], [-0.5 * c["vrel"], 0, 0]]))
    r.force()
    return sp, r, c


def test_an_oblique_impact_with_a_spring_conserves_momentum_and_angular_momentum(oracle):
    """As tests/test_gpu_friction.py asserts for its oblique impact.  (In the periodic bed above the total angular momentum
    about a point is no conserved quantity: a pair across a face acts on an image, not on its owner's position.)"""
    sp, r, c = _oblique(1, 2e3, {(1, 1): (0.5, 50.0)}, {(1, 1): 2e4})
    mass = sp.body(0)[0]
    J, p, seen = [], [], 0.0
    for _ in range(28):
        r.run_native(50, use_graph=True)
        x, v, L = r.x[:2].cpu().numpy(), r.v.cpu().numpy(), r.L.cpu().numpy()
        p.append(mass * v.sum(axis=0))
        J.append((np.cross(x, mass * v) + L).sum(axis=0))
        seen = max(seen, float(np.abs(r.contact_history()).max(initial=0.0)))   # (no slot while they are apart)
    sp.close()
    J, p = np.array(J), np.array(p)
    Jscale = np.abs(J[0]).max()                 # the angular momentum itself, as tests/test_gpu_friction.py takes it
    print(f"largest |xi| seen {seen:.3e}, momentum {np.abs(p).max():.2e}, angular momentum change {np.abs(J - J[0]).max():.2e} of {Jscale:.3g}, "
          f"L_z {L[:, 2]}")
    assert seen > 0 and (np.abs(L[:, 2]) > 0).all()                    # the spring was loaded; both spheres spin
    assert Jscale > 0.9 * mass * (0.5 * c["vrel"]) * 0.5               # m (vrel / 2) times the offset 0.5: the orbital moment is not small
    assert np.abs(p).max() <= 1e-12 * mass * c["vrel"]
    assert np.abs(J - J[0]).max() <= 1e-12 * Jscale


# ---- 6. the ledger -------------------------------------------------------------------------------------------------------------

def _oblique_balance(k, gamma, fric, spring):
    sp, r, c = _oblique(k, gamma, fric, spring)
    E0 = _total_energy(sp, r)
    r.run_native(c["nsteps"] * k, use_graph=True)
    D = r.ledger()["dissipated"]
    E1 = _total_energy(sp, r)
    gap = float(np.linalg.norm((r.x[1] - r.x[0]).cpu().numpy()))
    xi = r.contact_history() if spring else np.zeros((1, 3))
    sp.close()
    return E0, E1, D, gap, xi


def test_the_balance_of_an_oblique_collision_with_a_spring_closes_to_first_order_in_dt(oracle):
    """The bounds are those of tests/test_gpu_ledger.py's first-order test: the elastic residual is at most a tenth of the
    dissipative one, and the dissipative one falls to at most 0.75 of itself at dt / 2.
    Measured on an MI355X: see DESIGN.md §4.10."""
    from test_ledger_ref import COLLISION
    R, R0 = [], []
    for k in (1, 2):
        E0, E1, D, gap, xi = _oblique_balance(k, COLLISION["gamma"], {(1, 1): (0.5, 50.0)}, {(1, 1): 2e4})
        e0, e1, d0, gap0, _ = _oblique_balance(k, 0.0, None, None)
        R.append(abs(E1 - E0 + D))
        R0.append(abs(e1 - e0))
        print(f"dt/{k}: E0 {E0:.6f} E1 {E1:.6f} D {D:.6f} R {R[-1]:.3e} R/D {R[-1] / D:.2e} elastic R0 {R0[-1]:.3e} gap {gap:.3f}")
        assert gap > 2.02 and gap0 > 2.02 and d0 == 0.0                 # they met and parted
        # after separation xi is zero, and it is the pass' reset of an untouched slot that zeroed it: the spheres have
        # parted but are still inside the skin, so the list holds their slot (an emptied list would say nothing)
        assert xi.shape == (1, 3) and not xi.any()
        assert 0.3 * E0 < D < E0
    print(f"R(dt/2) / R(dt) = {R[1] / R[0]:.3f}")
    assert R0[0] <= 0.1 * R[0] and R0[1] <= 0.1 * R[1]
    assert R[1] <= 0.75 * R[0]


# ---- 7. off is off ---------------------------------------------------------------------------------------------------------------

def test_without_a_spring_the_contact_pass_is_the_dissipation_pass_bit_for_bit(oracle):
    r = history_inputs(oracle, True)
    sp = _bed_ctx(r["case"], r["K"], r["E"], det=1, spring=None)
    bed = _Bed(sp, r["case"], r["v"], r["L"], NLOCAL, True)
    a = bed.pass_(call="dissipation")
    b = bed.pass_(DT)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.abs(a[0]).max() > 0
    sp.close()
    # set and set back to zero: the parent's bits again (a context that never saw a spring is the parent's)
    sp = _bed_ctx(r["case"], r["K"], r["E"], det=1, spring=SPRING)
    for (i, j) in SPRING:
        sp.set_pair_tangential_spring(i, j, 0.0)
    assert not sp.has_history
    bed = _Bed(sp, r["case"], r["v"], r["L"], NLOCAL, True)
    c = bed.pass_(call="dissipation")
    d = bed.pass_(DT)
    sp.close()
    for k in (2, 3):
        assert np.array_equal(a[k], c[k]) and np.array_equal(a[k], d[k])


def test_a_list_built_while_no_spring_was_set_holds_no_history(oracle):
    """Spring on, build, xi installed; spring off, the same rows built again (the same slot count); spring on again.  What
    the first build left in xi and the keys is not the installed list's history: the pass and the copy refuse until the
    next build, and that build starts from zero instead of carrying it."""
    from shpair.capi import ShPairError
    r = history_inputs(oracle, True)
    sp = _bed_ctx(r["case"], r["K"], r["E"], det=1)
    bed = _Bed(sp, r["case"], r["v"], r["L"], NLOCAL, True)
    sp.set_contact_history(NLOCAL, r["xi"])
    assert sp.contact_history(NLOCAL).any()
    for (i, j) in SPRING:
        sp.set_pair_tangential_spring(i, j, 0.0)
    assert not sp.has_history
    assert bed.build() == bed.np                                        # a build without a spring: no keys, no xi
    for (i, j), kt in SPRING.items():
        sp.set_pair_tangential_spring(i, j, kt)
    bed.compute()
    for call in (lambda: bed.pass_(DT), lambda: sp.contact_history(NLOCAL), lambda: sp.set_contact_history(NLOCAL, r["xi"])):
        with pytest.raises(ShPairError, match="build it again") as e:
            call()
        assert e.value.code == -4
    assert bed.build() == bed.np
    assert not sp.contact_history(NLOCAL).any()                         # nothing was carried from the first build
    bed.compute()
    df, _, _, _ = bed.pass_(DT)                                         # and the pass runs on it
    assert np.abs(df).max() > 0
    # switched off and on with no build between: the installed list's xi is dropped just the same
    sp.set_contact_history(NLOCAL, r["xi"])
    for (i, j) in SPRING:
        sp.set_pair_tangential_spring(i, j, 0.0)
    for (i, j), kt in SPRING.items():
        sp.set_pair_tangential_spring(i, j, kt)
    with pytest.raises(ShPairError, match="build it again") as e:
        bed.pass_(DT)
    assert e.value.code == -4
    assert bed.build() == bed.np and not sp.contact_history(NLOCAL).any()
    sp.close()


def test_refusals(oracle):
    import torch
    from shpair import mrank
    from shpair.capi import ShPairError, HaloArrays, HaloRunParams
    r = history_inputs(oracle, True)
    case = r["case"]
    sp = _bed_ctx(case, r["K"], r["E"])
    bed = _Bed(sp, case, r["v"], r["L"], NLOCAL, True)
    with pytest.raises(ShPairError, match="shstep_pair_contact_device") as e:       # the dissipation call while a k_t is set
        bed.pass_(call="dissipation")
    assert e.value.code == -1
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ShPairError, match="dt") as e:
            bed.pass_(bad)
        assert e.value.code == -1
    for a, b, kt in ((1, 1, -1.0), (1, 2, np.nan), (1, 1, np.inf), (0, 1, 1.0), (1, 3, 1.0)):
        with pytest.raises(ShPairError) as e:
            sp.set_pair_tangential_spring(a, b, kt)
        assert e.value.code == -1
    # a fresh build: no compute has run on it yet
    sp.neighbor_build_device(NLOCAL, bed.n - NLOCAL, bed.x.data_ptr(), bed.sh.data_ptr(), tag=bed.tag.data_ptr())
    with pytest.raises(ShPairError, match="no compute has run") as e:
        bed.pass_(DT)
    assert e.value.code == -4
    # a caller's list drops the history and is refused
    sp.set_neighbors_csr(case["ilist"], case["offsets"], case["jlist"])
    for call in (lambda: bed.pass_(DT), lambda: sp.contact_history(NLOCAL), lambda: sp.set_contact_history(NLOCAL, r["xi"])):
        with pytest.raises(ShPairError, match="shstep_neighbor_build_device|no device-built neighbour list") as e:
            call()
        assert e.value.code == -4
    # no spring: no history to copy
    for (i, j) in SPRING:
        sp.set_pair_tangential_spring(i, j, 0.0)
    sp.neighbor_build_device(NLOCAL, bed.n - NLOCAL, bed.x.data_ptr(), bed.sh.data_ptr(), tag=bed.tag.data_ptr())
    with pytest.raises(ShPairError, match="no tangential spring") as e:
        sp.contact_history(NLOCAL)
    assert e.value.code == -4
    sp.close()
    # a list partitioned by halo_overlap, and the loop over several ranks
    c = carry_bed()
    n = c["n"]
    sp = ShPair_for(c)
    sp.set_option("halo_overlap", 1)
    nmax = 8 * n
    x, q = torch.zeros(nmax, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(nmax, 4, dtype=torch.float64, device="cuda:0")
    ty, sh = torch.ones(nmax, dtype=torch.int32, device="cuda:0"), torch.zeros(nmax, dtype=torch.int32, device="cuda:0")
    x[:n], q[:n], sh[:n] = dev(c["x0"]), dev(c["quat"]), dev(c["shtype"])
    torch.cuda.synchronize()
    ng = sp.borders_device(n, nmax, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr())
    assert ng > 0 and sp.neighbor_build_device(n, ng, x.data_ptr(), sh.data_ptr()) > 0
    f, tq = torch.zeros(nmax, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(nmax, 3, dtype=torch.float64, device="cuda:0")
    tw = torch.zeros(nmax, 6, dtype=torch.float64, device="cuda:0")
    sp.compute_device(n, ng, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f.data_ptr(), tq.data_ptr())
    with pytest.raises(ShPairError, match="partitioned") as e:
        sp.pair_contact_device(n, ng, x.data_ptr(), ty.data_ptr(), sh.data_ptr(), tw.data_ptr(), f.data_ptr(), tq.data_ptr(), DT)
    assert e.value.code == -4
    sp.synchronize()
    sp.set_option("halo_overlap", 0)
    halo = mrank.Halo(sp, 0, 1, (1, 1, 1), c["lo"], c["hi"], (1, 1, 1), CARRY_SKIN)
    with pytest.raises(ShPairError, match="tangential history is single-rank") as e:
        halo.run(HaloArrays(), HaloRunParams(), 1, 0)
    assert e.value.code == -4
    halo.close()
    sp.close()


def ShPair_for(c):
    """A one-type context with carry_bed()'s shapes, friction, a spring and its periodic box."""
    from shpair import ShPair
    sp = ShPair(0)
    sp.settings(NQ)
    sp.set_ntypes(1, 2)
    for s, a in enumerate(c["shapes"]):
        sp.set_shape(s, 4, a)
    sp.coeff(1, 1, 1000.0, 1.25)
    sp.pair_friction(1, 1, 0.5, 100.0)
    sp.set_pair_tangential_spring(1, 1, 1e4)
    sp.set_box(c["lo"], c["hi"], (1, 1, 1), CARRY_SKIN)
    return sp
