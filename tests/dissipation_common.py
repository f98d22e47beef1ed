"""Helpers of the single-domain GPU tests of contact dissipation (tests/test_gpu_damp.py: docs/SPEC.md §2.10,
tests/test_gpu_friction.py: §2.11): the bed and its motion, a context on a CSR list, one compute + twists + pair pass,
a periodic bed in a DeviceRun, the energy of a run, and the wall pass on a handful of particles.  L = 4, n_q = 8."""
import numpy as np

from common import make_case

NQ = 8


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def bed_case(oracle, n, seed, nlocal=None, spacing=1.9):
    """A bed of n particles, 2 shapes, 2 types; nlocal < n: the rows behind it are ghosts and own no list row."""
    case = make_case(n, 4, 2, seed=seed, amp=0.2, ntypes=2, rmax_fn=oracle.shape_rmax, spacing=spacing)
    if nlocal is not None:
        case["ilist"] = case["ilist"][:nlocal]
        case["jlist"] = case["jlist"][:case["offsets"][nlocal]]
        case["offsets"] = case["offsets"][:nlocal + 1]
    case["massprops"] = [oracle.mass_props(4, a) for a in case["shapes"]]
    return case


def motion(case, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(case["n"], 3)), 0.3 * rng.normal(size=(case["n"], 3))


def ctx(case, K, E, det=0, nq=NQ, gamma=None, fric=None):
    from shpair import ShPair
    sp = ShPair(0)
    sp.settings(nq)
    sp.set_ntypes(K.shape[0] - 1, len(case["shapes"]))
    for s, a in enumerate(case["shapes"]):
        sp.set_shape(s, case["lmax"], a)
    for i in range(1, K.shape[0]):
        for j in range(1, K.shape[0]):
            sp.coeff(i, j, K[i, j], E[i, j])
    sp.set_neighbors_csr(case["ilist"], case["offsets"], case["jlist"])
    if det:
        sp.set_option("deterministic", 1)
    for (a, b), g in (gamma or {}).items():
        sp.pair_damping(a, b, g)
    for (a, b), (mu, gt) in (fric or {}).items():
        sp.pair_friction(a, b, mu, gt)
    return sp


def gpu_forces(sp, case, v, L, nlocal=None, newton=True, old_call=False):
    """compute + twists + dissipation pass on fresh arrays: f, torque [n][3], twist [n][6]."""
    import torch
    b, n = case["bed"], case["n"]
    nlocal = n if nlocal is None else nlocal
    x, q, ty, sh = dev(b["x"]), dev(b["quat"]), dev(b["type"].astype(np.int32)), dev(b["shtype"].astype(np.int32))
    vd, Ld = dev(v), dev(L)
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    tw = torch.zeros(n, 6, dtype=torch.float64, device="cuda:0")
    sp.compute_device(nlocal, n - nlocal, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f.data_ptr(), tq.data_ptr(),
                      newton_pair=newton)
    # the rows behind nlocal are a host's own ghosts: it fills their twists itself — here by asking for all n rows
    sp.twist_device(n, 0, vd.data_ptr(), q.data_ptr(), Ld.data_ptr(), sh.data_ptr(), tw.data_ptr())
    if old_call:
        sp.pair_damping_device(nlocal, n - nlocal, x.data_ptr(), ty.data_ptr(), tw.data_ptr(), f.data_ptr(), tq.data_ptr(),
                               newton_pair=newton)
    else:
        sp.pair_dissipation_device(nlocal, n - nlocal, x.data_ptr(), ty.data_ptr(), sh.data_ptr(), tw.data_ptr(), f.data_ptr(),
                                   tq.data_ptr(), newton_pair=newton)
    torch.cuda.synchronize()
    sp.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), tw.cpu().numpy()


def _rigid_motion(case, v0, Om):
    """v (of the centres of mass) and angmom of a common rigid motion: w = v0 + Om x x, omega = Om."""
    import wall_ref as W
    b, n = case["bed"], case["n"]
    v, L = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        mp = case["massprops"][int(b["shtype"][i])]
        xx, yy, zz, xy, xz, yz = mp[4:10]
        R = W.quat_to_mat(b["quat"][i])
        L[i] = R @ np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]) @ R.T @ Om
        v[i] = v0 + np.cross(Om, b["x"][i] + R @ mp[1:4])
    return v, L


def periodic_run(v, L=None, det=1, pair_damping=None, pair_friction=None):
    """A periodic hcp bed in a DeviceRun: ghosts, list and twists of the ghost rows are the library's."""
    from shpair import ShPair, shapes, bed
    from shpair.run import DeviceRun
    shp = [shapes.random_shape(4, 4000 + 17 * s + 4, amp=0.2) for s in range(2)]
    pts, lo, hi = bed.periodic_hcp(60, 1.9, (1, 1, 1))
    rng = np.random.default_rng(4)
    n = pts.shape[0]
    x = pts + rng.uniform(-0.1, 0.1, pts.shape)
    sp = ShPair(0)
    sp.settings(NQ)
    sp.set_ntypes(2, 2)
    for s, a in enumerate(shp):
        sp.set_shape(s, 4, a)
    sp.coeff("*", "*", 1000.0, 1.25)
    if det:
        sp.set_option("deterministic", 1)
    r = DeviceRun(sp, x, bed.random_quaternions(n, rng), (np.arange(n) % 2).astype(np.int32), lo, hi, (1, 1, 1), 0.2,
                  type_=1 + (np.arange(n) // 2) % 2, pair_damping=pair_damping, pair_friction=pair_friction)
    r.v[:] = dev(np.broadcast_to(v, (n, 3)) if np.ndim(v) == 1 else v)
    if L is not None:
        r.L[:] = dev(L)
    r.force()
    import torch
    torch.cuda.synchronize()
    sp.synchronize()
    return sp, r


def _total_energy(sp, r):
    """KE (shstep_energies_device) + pair energy of the current positions (a compute into scratch rows: f stays)."""
    import torch
    f2, t2 = torch.zeros_like(r.f), torch.zeros_like(r.tq)
    r.ev.zero_()
    sp.compute_device(r.n, r.nghost, r.x.data_ptr(), r.q.data_ptr(), r.ty.data_ptr(), r.sh.data_ptr(), f2.data_ptr(), t2.data_ptr(),
                      eflag=True, ev=r.ev.data_ptr())
    e = r.energies()
    return e[0] + e[1] + e[2]


def _wall_ctx(shp, nq, kn=1000.0, expo=1.25, rmax=None, deterministic=0):
    """shp: [(lmax, anm)], all of one lmax or mixed."""
    from shpair import ShPair
    sp = ShPair(0)
    sp.settings(nq)
    sp.set_ntypes(1, len(shp))
    for s, (lmax, a) in enumerate(shp):
        sp.set_shape(s, lmax, a, 0.0 if rmax is None else rmax[s])
    sp.coeff(1, 1, kn, expo)
    if deterministic:
        sp.set_option("deterministic", 1)
    return sp


def _wall_pass(sp, x, quat, tw, nwalls, damped=True):
    import torch
    n = len(x)
    xd, qd, sh, m, twd = dev(x), dev(quat), dev(np.zeros(n, np.int32)), dev(np.ones(n, np.int32)), dev(tw)
    f, tq = torch.zeros(n, 3, dtype=torch.float64, device="cuda:0"), torch.zeros(n, 3, dtype=torch.float64, device="cuda:0")
    out = torch.zeros(nwalls, 4, dtype=torch.float64, device="cuda:0")
    if damped:
        sp.wall_force_damped_device(n, xd.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                    twd.data_ptr(), wall_out=out.data_ptr())
    else:
        sp.wall_force_device(n, xd.data_ptr(), qd.data_ptr(), sh.data_ptr(), m.data_ptr(), f.data_ptr(), tq.data_ptr(),
                             wall_out=out.data_ptr())
    torch.cuda.synchronize()
    sp.synchronize()
    return f.cpu().numpy(), tq.cpu().numpy(), out.cpu().numpy()
