"""The unit of length (docs/SPEC.md §4): the model is homogeneous in length, with time and density unchanged.

Multiplying every length of a scene by s and every coefficient by its power of s below multiplies every output by a
power of s and changes nothing else.  tests/test_units_refs.py proves these tables on the references alone;
tests/test_gpu_units.py holds the library to the references at the scales S.

  inputs                                                          x s^p
  x, a_nm, rmax, box, skin, wall offsets c, v, wall velocities    1
  gravity                                                         1
  kn (per type pair, per wall)                                    5 - 3 m
  gamma (volume-rate damping: a pressure per volume rate)         -1
  gamma_t (force per velocity), k_t (force per length)            3
  mu                                                              0
  mu_r, mu_tw (lengths)                                           1
  gamma_r, gamma_tw (torque per angular velocity)                 5
  angmom                                                          5

  outputs: V 3, S_n 2, T_n 3, f 4, torque / energy / virial / ledger 5, mass 3, inertia 5, xi 1.

Proven by test_units_refs.py, row by row (the walls' k_t and velocities on the corner scene through wall_history_ref).
scale(scene, s) takes a whole-step scene (traj_ref.scene); the helpers above it take the beds and tables of the single-pass tests.
"""
import numpy as np

S = (2.0 ** -10, 1e-3, 2.0 ** 12)
OFFSET = np.array([-1024.0, 2048.0, 4096.0])          # x s x R where a test also translates
ROW_POW = np.array([3, 2, 2, 2, 3, 3, 3])             # (V, S_n, T_n)
POW = dict(f=4, torque=5, energy=5, virial=5, eatom=5, vatom=5, mass=3, inertia=5, xi=1, twist_v=1, twist_w=0)


def is_pow2(s):
    return float(np.frexp(s)[0]) == 0.5


def scale_kn(K, E, s):
    """kn s^(5 - 3 m), element by element (type-pair tables or per-wall vectors)."""
    return np.asarray(K, dtype=np.float64) * s ** (5.0 - 3.0 * np.asarray(E, dtype=np.float64))


def scale_coef(coef, s, *powers):
    """A {type pair: value or tuple} table of the dissipation tests with component k times s^powers[k]."""
    out = {}
    for key, val in (coef or {}).items():
        if isinstance(val, tuple):
            out[key] = tuple(v * s ** p for v, p in zip(val, powers))
        else:
            out[key] = val * s ** powers[0]
    return out


def scale_case(case, s, rmax_fn, offset=None, mass_fn=None):
    """A bed of common.make_case (or dissipation_common.bed_case with mass_fn) with every length times s; the list is
    kept.  rmax is the reference's own bounding radius of the scaled shape.  offset: the bed is also translated by
    offset x s x (the largest bounding radius)."""
    c = dict(case)
    c["shapes"] = [np.asarray(a) * s for a in case["shapes"]]
    c["rmax"] = [rmax_fn(case["lmax"], a) for a in c["shapes"]]
    b = dict(case["bed"])
    b["x"] = case["bed"]["x"] * s
    if offset is not None:
        b["x"] = b["x"] + np.asarray(offset) * (s * max(case["rmax"]))
    c["bed"] = b
    if mass_fn is not None:
        c["massprops"] = [mass_fn(case["lmax"], a) for a in c["shapes"]]
    return c


def unscale_rows(rows, s):
    return np.asarray(rows) / s ** ROW_POW


def unscale(name, value, s):
    return np.asarray(value) / s ** POW[name]


def scale_planes(planes, s, offset=None, radius=1.0):
    """Planes n.p = c with c times s; translated by offset x s x radius: c += n.t."""
    pl = np.array(planes, dtype=np.float64)
    pl[:, 3] *= s
    if offset is not None:
        pl[:, 3] += pl[:, :3] @ (np.asarray(offset) * (s * radius))
    return pl


# ---- the scenes of tests/test_units_refs.py and tests/test_gpu_units.py ---------------------------------------------------

def _plan(id_, lmax, nq, n=120, m=1.25, **opts):
    return dict(id=id_, lmax=lmax, nq=nq, n=n, m=m, opts=opts)


# one bed per launch plan; info: what kernel_info() must report
PLANS = [
    dict(_plan("4-10", 4, 10), info=dict(family=1, waves_per_pair=1, compiled_order=1, specialised=1)),
    dict(_plan("6-16-spec", 6, 16, spec=1), info=dict(family=1, waves_per_pair=1, compiled_order=1, specialised=1)),
    dict(_plan("6-16-general", 6, 16, spec=0), info=dict(family=1, waves_per_pair=1, compiled_order=1, specialised=0)),
    dict(_plan("6-16-m2", 6, 16, m=2.0), info=dict(family=1, waves_per_pair=1, compiled_order=1, specialised=1)),
    dict(_plan("8-16-split", 8, 16, jpoly=1, split=1), info=dict(family=1, waves_per_pair=2, compiled_order=1)),
    dict(_plan("12-32", 12, 32, n=24), info=dict(family=1, waves_per_pair=2, compiled_order=1)),
    dict(_plan("14-8-loop", 14, 8), info=dict(compiled_order=0, waves_per_pair=1)),
    dict(_plan("6-16-body", 6, 16, jpoly=0), info=dict(family=0, waves_per_pair=1, compiled_order=1)),
    dict(_plan("5-9-weighted", 5, 9, rule=1), info=dict(weighted=1, waves_per_pair=1, compiled_order=1)),
]


def plan_bed(plan, oracle):
    from common import make_case
    return make_case(plan["n"], plan["lmax"], 2, seed=1500 + plan["lmax"], rmax_fn=oracle.shape_rmax)


def plan_scaled(base, plan, s, rmax_fn, offset=None):
    """(case, K, E) of a plan's bed at scale s."""
    from common import coeff_tables
    K, E = coeff_tables(1, 1000.0, plan["m"])
    case = base if s == 1.0 and offset is None else scale_case(base, s, rmax_fn, offset)
    return case, scale_kn(K, E, s), E


def wall_scene(rmax_fn, s, lmax=4, nq=10, n=60):
    """Particles in the corner of the walls x = 0, y = 0, z = 0 and an oblique one, at scale s; exponents 1.25, 2, 1, 1.25."""
    from shpair import shapes, bed
    rng = np.random.default_rng(41)
    shp = [shapes.random_shape(lmax, 660 + 7 * k, amp=0.1) * s for k in range(2)]
    planes = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [3 ** -0.5, 3 ** -0.5, 3 ** -0.5, 1.2]], dtype=np.float64)
    x = np.zeros((0, 3))
    while x.shape[0] < n:
        p = rng.uniform(0, 3.0, size=(4 * n, 3))
        x = np.concatenate([x, p[(p @ planes[:, :3].T - planes[:, 3] >= 0.35).all(axis=1)]])
    x = x[:n]
    kn, expo = np.array([1000.0, 800.0, 1200.0, 900.0]), np.array([1.25, 2.0, 1.0, 1.25])
    return dict(lmax=lmax, nq=nq, n=n, anm=shp, shapes=[(lmax, a, rmax_fn(lmax, a)) for a in shp], x=x * s,
                quat=bed.random_quaternions(n, rng), shtype=rng.integers(0, 2, n).astype(np.int32), planes=scale_planes(planes, s),
                kn=scale_kn(kn, expo, s), expo=expo)


def list_scene(rmax_fn, n=512, lmax=4):
    """A periodic box of 512 particles of two shapes at about the density of the beds."""
    from shpair import shapes
    rng = np.random.default_rng(53)
    shp = [shapes.random_shape(lmax, 680 + 7 * k, amp=0.1) for k in range(2)]
    edge = 1.9 * 8
    return dict(n=n, lmax=lmax, anm=shp, rmax=np.array([rmax_fn(lmax, a) for a in shp]), lo=np.zeros(3), hi=np.full(3, edge),
                periodic=(1, 1, 1), skin=0.25, x=rng.uniform(0, edge, (n, 3)), shtype=rng.integers(0, 2, n).astype(np.int32))


def dissipation_scene(oracle, s):
    """The L = 4 / n_q = 8 bed of dissipation_common at scale s with the coefficients of the four pair laws as
    tests/test_gpu_friction.py, test_gpu_rolling.py and test_gpu_history.py set them."""
    from common import coeff_tables
    from dissipation_common import bed_case, motion
    from test_gpu_friction import GAMMA, FRIC
    from test_gpu_rolling import ROLL, TWIST
    from test_gpu_history import SPRING
    case = bed_case(oracle, 60, 1)
    K, E = coeff_tables(2, lambda i, j: 1000.0 + 100.0 * (i + j), 1.25)
    v, L = motion(case, 8)
    cs = scale_case(case, s, oracle.shape_rmax, mass_fn=oracle.mass_props) if s != 1.0 else case
    xi = 0.01 * np.random.default_rng(3).normal(size=(case["jlist"].size, 3))
    return dict(case=cs, K=scale_kn(K, E, s), E=E, v=v * s, L=L * s ** 5, xi=xi * s, gamma=scale_coef(GAMMA, s, -1),
                fric=scale_coef(FRIC, s, 0, 3), spring=scale_coef(SPRING, s, 3), roll=scale_coef(ROLL, s, 1, 5),
                twist=scale_coef(TWIST, s, 1, 5))


def corner_wall_scene(s, offset=None):
    """One L = 6 particle in the corner of three walls with damping and friction on each (the corner case of
    tests/test_gpu_friction.py), at scale s; offset: translated by offset x s (the radius is about 1)."""
    from shpair import shapes
    planes = np.array([[1.0, 0, 0, 0.0], [0, 1.0, 0, 0.0], [0, 0, 1.0, 0.0]])
    x0, tw0 = np.array([0.8, 0.9, 0.7]), np.array([0.35, -0.6, -0.25, 0.5, 0.8, -0.7])
    kn, expo = np.array([1000.0, 800.0, 1200.0]), np.array([1.25, 1.0, 2.0])
    x = (x0 * s)[None, :]
    if offset is not None:
        x = x + np.asarray(offset) * s
    return dict(lmax=6, nq=16, anm=shapes.random_shape(6, 3, amp=0.1) * s, x=x, quat=np.array([[0.5, 0.5, -0.5, 0.5]]),
                twist=(tw0 * np.array([s, s, s, 1, 1, 1]))[None, :], planes=scale_planes(planes, s, offset), kn=scale_kn(kn, expo, s),
                expo=expo, gamma=np.array([400.0, 250.0, 600.0]) / s, mu=np.array([0.5, 0.1, 0.6]),
                gt=np.array([200.0, 400.0, 100.0]) * s ** 3,
                # the spring and moving instance of tests/test_gpu_wall_history.py: springs on two walls, plain friction on
                # the third, every wall translating, a live xi on each
                kt=np.array([2000.0, 2000.0, 0.0]) * s ** 3, dt=1e-3,
                vel=np.array([[0.9, -0.7, 0.4], [0.6, -1.1, 0.8], [-0.5, 0.9, -1.2]]) * s,
                xi0=np.array([[0.0, 0.004, -0.003], [0.3, 0.0, -0.2], [0.1, 0.1, 0.0]]) * s)


def scale_fixture(g, s):
    """An exact-root fixture of tests/pair_ref.py (load_fixture) with inputs and expected rows scaled analytically; exact
    for a power of two."""
    out = dict(g)
    out["a_nm"], out["rmax"], out["x"] = g["a_nm"] * s, g["rmax"] * s, g["x"] * s
    out["V"], out["S"], out["T"] = g["V"] * s ** 3, g["S"] * s ** 2, g["T"] * s ** 3
    out["shape_table"] = [(g["lmax"], a, r) for a, r in zip(out["a_nm"], out["rmax"])]
    return out


# powers of s of the entries of a whole-step scene (tests/traj_ref.py: scene); what is not listed is dimensionless
SCENE_POW = dict(a_nm=1, rmax=1, x=1, v=1, angmom=5, lo=1, hi=1, skin=1, gravity=1, gamma_t=3, gamma_r=5, G=-1, GT=3, KT=3,
                 MUR=1, GR=5, MUTW=1, GTW=5, wall_damping=-1, wall_gt=3, wall_kt=3, wall_velocity=1)
STATE_POW = dict(x=1, v=1, quat=0, angmom=5, f=4, torque=5, xi=1, wall_xi=1, ledger=5, per_wall=5)


def scale(scene, s, offset=None):
    """A whole-step scene (the dict of traj_ref.scene) with every dimensional input times its power of s, time and density
    unchanged: the table of the module docstring; the drag of SPEC §6 is a force per velocity (gamma_t, s^3) and a torque
    per angular velocity (gamma_r, s^5); kn and the walls' kn go with s^(5 - 3 m).  The mass properties are the
    reference's own of the scaled shapes.  offset: the scene is also translated by offset x s x (the largest radius)."""
    from oracle import oracle as O
    sc = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    for k, p in SCENE_POW.items():
        sc[k] = scene[k] * s ** p
    sc["K"] = scale_kn(scene["K"], scene["E"], s)
    sc["wall_kn"] = scale_kn(scene["wall_kn"], scene["wall_expo"], s)
    sc["massprops"] = np.array([O.mass_props(int(scene["lmax"]), a) for a in sc["a_nm"]])
    t = None if offset is None else np.asarray(offset) * (s * scene["rmax"].max())
    sc["planes"] = scale_planes(scene["planes"], s) if len(scene["planes"]) else scene["planes"].copy()
    if t is not None:
        sc["x"], sc["lo"], sc["hi"] = sc["x"] + t, sc["lo"] + t, sc["hi"] + t
        if len(sc["planes"]):
            sc["planes"][:, 3] += sc["planes"][:, :3] @ t
    return sc


def step_reference(sc, nsteps, noise_seed=20261020):
    """The reference run of a whole-step scene and its own D_q, as mixed_common.step_reference computes them: the
    deviation of the reference from itself at the last step with every integral scaled by 1 + 1e-12 eta; bars 10 D_q."""
    import traj_ref as TR
    st = TR.setup(sc)
    setup, recs = TR.snapshot(st), []
    for _ in range(nsteps):
        recs.append(TR.step(sc, st))
    last = TR.snapshot(st)
    noisy, nrecs = TR.run(sc, nsteps, noise=np.random.default_rng(noise_seed))
    assert [r["rebuilt"] for r in nrecs] == [r["rebuilt"] for r in recs]
    D = TR.deviation(noisy[f"step{nsteps}"], last)
    return dict(sc=sc, setup=setup, last=last, recs=recs, rebuilt=[r["rebuilt"] for r in recs], margin=[r["margin"] for r in recs],
                touching=[r["counts"]["touching"] for r in recs], D=D, bar={q: 10.0 * D[q] for q in D})


def pair_powers(oracle, sc):
    """[nslots][2] = P_d, P_f of the pair pass on a dissipation scene, from the oracle's rows and ledger_ref."""
    import damp_ref as D
    import ledger_ref as LR
    import test_gpu_friction as TF
    case, K, E = sc["case"], sc["K"], sc["E"]
    b, n = case["bed"], case["n"]
    from common import oracle_compute
    from dissipation_common import NQ
    o = oracle_compute(oracle, case, NQ, K, E, force_volume=True, want_pairs=True)
    pi, pj = D.expand(case["ilist"], case["offsets"], case["jlist"])
    tw = D.twists(case["massprops"], [1.0, 1.0], sc["v"], b["quat"], sc["L"], b["shtype"])
    return LR.pair_powers(o["pairs"], pi, pj, b["x"], tw, b["type"], b["shtype"], case["rmax"], K, E, TF.table(2, sc["gamma"]),
                          TF.table(2, sc["fric"], 0), TF.table(2, sc["fric"], 1), n)
