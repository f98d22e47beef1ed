"""Cost of the planar walls (docs/SPEC.md §2.9, csrc/wall_kernels.hpp) beside the pair path, in one process:
bench.py's headline bed shape (100k particles, L = 6, n_q = 16) inside a 6-wall box drawn just inside its outermost
centres, so that the outer layer of particles touches the walls.
  python tools/wall_bench.py [--lmax 6 --nq 16 --n 100000 --rounds 10 --inset 0.8 --gamma-w 0 --mu-w 0 --gt-w 0 --spring 0 --wall-vel UX UY UZ --roll MU_R GAMMA_R MU_TW GAMMA_TW]
--gamma-w G > 0 times the damped instance of the contact kernel (docs/SPEC.md §2.10) with its twist pass instead;
--mu-w MU --gt-w GT (both > 0) the friction instance (§2.11); --wall-vel gives every wall that velocity, which selects the
moving instance of either (§2.12), and times the advance kernel of the planes on its own.  --spring KT (> 0, with
--mu-w) gives every wall a tangential spring (§2.15): the history instance through wall_contact_device with a small dt,
the live sweep included.  --roll gives every wall rolling and twisting resistance (§2.17) and adds a leg that times the
wall pass as configured with and without wall_roll_kernel in the same process (the particles then spin).
--cylinder adds a leg for the cylindrical walls of §2.18 (csrc/cylinder_kernels.hpp): the core of the same bed inside a
cylinder along z drawn --inset behind its outermost centres, the cylinder pass timed like the planar one and printed
beside it; with --gamma-w or --mu-w/--gt-w (and --omega) the dissipative instance with its twist pass; with --spring KT
and --mu-w a further leg times the pass with the cylinder's tangential spring (§2.19: cyl_contact_device with a small dt,
the live sweep included) in rounds that alternate with the dissipative pass.  --ledger (with --cylinder and a coefficient)
adds a leg for the shell ledger of §2.20: the pass as configured with both ledgers off and on in alternating rounds (the
ordinary instance against its cyl_power_* twin), and the fold of the power rows timed on its own.  --rolling MU_R GAMMA_R
MU_TW GAMMA_TW (with --cylinder) adds a leg for the couples of §2.21: the cylinder pass as configured, twists included,
without and with cyl_roll_kernel in alternating rounds (the particles then spin), and the traffic the kernel is bound by.
--cone adds a leg for the conical walls of §2.22 and §2.23 (csrc/cone_kernels.hpp): the part of the same bed inside a
30-degree hopper along z whose apex lies below the bed, every centre at least --inset from its wall; the elastic pass, the
dissipative pass (gamma 3, mu 0.5, gamma_t 2, --omega) with its twist pass and the advancing pass with a tangential spring
(k_t 4000, conic_contact_device with a small dt, the live sweep included), in rounds that alternate, taken in the same run.
Prints the wall contacts, the wall pass's time per call (device events around its launches, both kernels and the
memset), that time per wall contact, and the pair path's kernel time per contact pair from the same run (the library's
"timing" option); then whole steps of shstep_run_device with and without walls on a periodic bed."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-spherharm_amd"))
import torch  # noqa: E402
from shpair import ShPair, shapes, bed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lmax", type=int, default=6)
ap.add_argument("--nq", type=int, default=16)
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inset", type=float, default=0.8, help="distance of the walls behind the outermost centres")
ap.add_argument("--gamma-w", type=float, default=0.0, help="wall damping coefficient: > 0 times the damped wall pass (twists + DAMP instance)")
ap.add_argument("--mu-w", type=float, default=0.0, help="wall friction coefficient mu_w (with --gt-w: the friction instance)")
ap.add_argument("--gt-w", type=float, default=0.0, help="wall friction coefficient gamma_t,w")
ap.add_argument("--spring", type=float, default=0.0, help="wall tangential spring k_t,w (with --mu-w: the history instance, advancing)")
ap.add_argument("--wall-vel", type=float, nargs=3, default=None, help="velocity of every wall: the moving instances and the advance kernel")
ap.add_argument("--roll", type=float, nargs=4, default=None, metavar=("MU_R", "GAMMA_R", "MU_TW", "GAMMA_TW"),
                help="wall rolling and twisting resistance: a leg that times the wall pass with and without wall_roll_kernel")
ap.add_argument("--cylinder", action="store_true", help="a leg that times the cylinder pass (SPEC 2.18) on the core of the bed")
ap.add_argument("--cone", action="store_true", help="a leg that times the cone pass (SPEC 2.22, 2.23): elastic, dissipative, advancing spring")
ap.add_argument("--ledger", action="store_true",
                help="with --cylinder and a coefficient: a leg that times the pass with both ledgers on (SPEC 2.20) beside the plain pass, and the fold")
ap.add_argument("--rolling", type=float, nargs=4, default=None, metavar=("MU_R", "GAMMA_R", "MU_TW", "GAMMA_TW"),
                help="with --cylinder: rolling and twisting resistance at the cylinder (SPEC 2.21), a leg with and without cyl_roll_kernel")
ap.add_argument("--omega", type=float, default=0.0, help="angular velocity of the cylinder about its axis (with --mu-w/--gt-w)")
a = ap.parse_args()
sprung = a.mu_w > 0 and a.spring > 0
twisted = a.gamma_w > 0 or (a.mu_w > 0 and a.gt_w > 0) or sprung

sp = ShPair(0)
sp.settings(a.nq)
sp.set_ntypes(1, 1)
sp.set_shape(0, a.lmax, shapes.random_shape(a.lmax, bed.SEED0 + 2))
sp.coeff("*", "*", 1000.0, 1.25)
rmax = [sp.rmax(0)]
b = bed.make_bed(a.n, rmax, seed=bed.SEED0 + 2)
il, of, jl = bed.half_neighbor_list(b["x"], b["shtype"], rmax)
sp.set_neighbors_csr(il, of, jl)
sp.set_option("timing", 1)
sp.set_option("count", 1)
lo, hi = b["x"].min(axis=0) - a.inset, b["x"].max(axis=0) + a.inset
planes = np.array([[1, 0, 0, lo[0]], [-1, 0, 0, -hi[0]], [0, 1, 0, lo[1]], [0, -1, 0, -hi[1]], [0, 0, 1, lo[2]], [0, 0, -1, -hi[2]]])
sp.set_walls(planes, 1000.0, 1.25)
if a.gamma_w > 0:
    sp.wall_damping(a.gamma_w)
if a.mu_w > 0 and (a.gt_w > 0 or sprung):
    sp.wall_friction(a.mu_w, a.gt_w)
if sprung:
    sp.set_wall_tangential_spring(a.spring)
if a.wall_vel is not None:
    sp.wall_velocity(a.wall_vel)
dev = torch.device("cuda:0")
x, q = torch.from_numpy(b["x"]).to(dev), torch.from_numpy(b["quat"]).to(dev)
ty, sh = torch.from_numpy(b["type"]).to(dev), torch.from_numpy(b["shtype"]).to(dev)
mask = torch.ones(a.n, dtype=torch.int32, device=dev)
f = torch.zeros(a.n, 3, dtype=torch.float64, device=dev)
tq = torch.zeros_like(f)
out = torch.zeros(6, 4, dtype=torch.float64, device=dev)
vel = torch.from_numpy(np.random.default_rng(1).normal(size=(a.n, 3))).to(dev)   # damped pass: thermal velocities, no spin
angm = torch.zeros_like(vel)
if a.roll is not None or a.rolling is not None:
    angm = torch.from_numpy(np.random.default_rng(2).normal(size=(a.n, 3))).to(dev)   # the couples act on a spin
tw = torch.zeros(a.n, 6, dtype=torch.float64, device=dev)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
st = torch.cuda.current_stream()
pair_ms, wall_ms, wall_out_ms = [], [], []
for r in range(a.rounds + 2):
    ps, ws, wo = [], [], []
    for _ in range(a.reps):
        f.zero_()
        tq.zero_()
        sp.compute_device(a.n, 0, x.data_ptr(), q.data_ptr(), ty.data_ptr(), sh.data_ptr(), f.data_ptr(), tq.data_ptr(),
                          stream=st.cuda_stream)
        torch.cuda.synchronize()
        stats = sp.stats()
        ps.append(stats["kernel_ms"])
        for want, acc in ((False, ws), (True, wo)):
            e0.record(st)
            if twisted:
                sp.twist_device(a.n, 0, vel.data_ptr(), q.data_ptr(), angm.data_ptr(), sh.data_ptr(), tw.data_ptr(), stream=st.cuda_stream)
            if sprung:
                sp.wall_contact_device(a.n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), mask.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                       tw.data_ptr(), 1e-6, wall_out=out.data_ptr() if want else None, stream=st.cuda_stream)
            elif twisted:
                sp.wall_force_damped_device(a.n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), mask.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                            tw.data_ptr(), wall_out=out.data_ptr() if want else None, stream=st.cuda_stream)
            else:
                sp.wall_force_device(a.n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), mask.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                     wall_out=out.data_ptr() if want else None, stream=st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1))
    if r >= 2:
        pair_ms.append(float(np.mean(ps)))
        wall_ms.append(float(np.mean(ws)))
        wall_out_ms.append(float(np.mean(wo)))
nc = sp.wall_stats()
p, w, wo = np.median(pair_ms), np.median(wall_ms), np.median(wall_out_ms)
print(f"L={a.lmax} nq={a.nq} n={a.n}: {jl.size} list slots, {stats['n_contact']} contact pairs, {nc} wall contacts")
print(f"pair kernels {p:.4f} ms = {1e6 * p / max(1, stats['n_contact']):.2f} ns per contact pair")
print(f"wall pass    {w:.4f} ms = {1e6 * w / max(1, nc):.2f} ns per wall contact (candidates over {a.n} particles + contact kernel + memset)")
print(f"wall pass with per-wall totals {wo:.4f} ms")
if sprung:
    xi = sp.wall_history(a.n)
    print(f"wall history: {int(xi.any(axis=2).sum())} live (particle, wall) rows, max|xi| {np.abs(xi).max():.3e}")
if a.wall_vel is not None:
    # the advance kernel alone: 200 launches back to back between two events, dt so small that the planes stay put
    adv = []
    for r in range(a.rounds + 2):
        e0.record(st)
        for _ in range(200):
            sp.advance_walls_device(1e-12, stream=st.cuda_stream)
        e1.record(st)
        torch.cuda.synchronize()
        if r >= 2:
            adv.append(1e3 * e0.elapsed_time(e1) / 200)
    print(f"wall advance kernel {np.median(adv):.2f} us per call (200 launches back to back, 6 walls)")
if a.roll is not None:
    # the wall pass as configured above (twists included), without and with the two couples of §2.17, interleaved
    def timed_pass():
        e0.record(st)
        sp.twist_device(a.n, 0, vel.data_ptr(), q.data_ptr(), angm.data_ptr(), sh.data_ptr(), tw.data_ptr(), stream=st.cuda_stream)
        if sprung:
            sp.wall_contact_device(a.n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), mask.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                   tw.data_ptr(), 1e-6, stream=st.cuda_stream)
        else:
            sp.wall_force_damped_device(a.n, x.data_ptr(), q.data_ptr(), sh.data_ptr(), mask.data_ptr(), f.data_ptr(), tq.data_ptr(),
                                        tw.data_ptr(), stream=st.cuda_stream)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    legs = {"off": [], "on": []}
    for r in range(a.rounds + 2):
        for leg in ("off", "on") if r % 2 == 0 else ("on", "off"):
            on = leg == "on"
            sp.wall_rolling(a.roll[0] if on else 0.0, a.roll[1] if on else 0.0)
            sp.wall_twisting(a.roll[2] if on else 0.0, a.roll[3] if on else 0.0)
            ts = [timed_pass() for _ in range(a.reps)]
            if r >= 2:
                legs[leg].append(float(np.mean(ts)))
    off_ms, on_ms = np.median(legs["off"]), np.median(legs["on"])
    print(f"wall pass + twists without / with rolling and twisting resistance: {off_ms:.4f} / {on_ms:.4f} ms "
          f"(wall_roll_kernel and the rows it makes the pass keep: {1e3 * (on_ms - off_ms):.1f} us over {a.n} rows, {nc} wall contacts)")
if a.cylinder:
    # the particles within the largest circle about the bed's vertical mid-axis, in a cylinder --inset behind the outermost
    c0, ext = 0.5 * (b["x"].min(axis=0) + b["x"].max(axis=0)), b["x"].max(axis=0) - b["x"].min(axis=0)
    rad = np.hypot(b["x"][:, 0] - c0[0], b["x"][:, 1] - c0[1])
    keep = rad <= 0.5 * min(ext[0], ext[1])
    ncy = int(keep.sum())
    sp.set_cylinders([[c0[0], c0[1], 0.0, 0.0, 0.0, 1.0, rad[keep].max() + a.inset]], 1000.0, 1.25)
    cdiss = a.gamma_w > 0 or (a.mu_w > 0 and a.gt_w > 0)
    if a.gamma_w > 0:
        sp.cylinder_damping(a.gamma_w)
    if a.mu_w > 0 and a.gt_w > 0:
        sp.cylinder_friction(a.mu_w, a.gt_w)
        sp.cylinder_rotation(a.omega)
    kd = torch.from_numpy(keep).to(dev)   # every per-particle array by the same rows
    xc, qc, shc = x[kd].contiguous(), q[kd].contiguous(), sh[kd].contiguous()
    velc, angc, maskc = vel[kd].contiguous(), angm[kd].contiguous(), mask[kd].contiguous()
    fc, tc, twc = torch.zeros(ncy, 3, dtype=torch.float64, device=dev), torch.zeros(ncy, 3, dtype=torch.float64, device=dev), tw[kd].contiguous()
    outc = torch.zeros(1, 5, dtype=torch.float64, device=dev)
    cyl_ms = {False: [], True: []}
    for r in range(a.rounds + 2):
        for want in (False, True):
            ts = []
            for _ in range(a.reps):
                e0.record(st)
                if cdiss:
                    sp.twist_device(ncy, 0, velc.data_ptr(), qc.data_ptr(), angc.data_ptr(), shc.data_ptr(), twc.data_ptr(), stream=st.cuda_stream)
                sp.cylinder_force_device(ncy, xc.data_ptr(), qc.data_ptr(), shc.data_ptr(), maskc.data_ptr(), fc.data_ptr(), tc.data_ptr(),
                                         twist=twc.data_ptr() if cdiss else None, cyl_out=outc.data_ptr() if want else None,
                                         stream=st.cuda_stream)
                e1.record(st)
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            if r >= 2:
                cyl_ms[want].append(float(np.mean(ts)))
    ncc = sp.cylinder_stats()
    cm, cmo = np.median(cyl_ms[False]), np.median(cyl_ms[True])
    print(f"cylinder pass{' (dissipative)' if cdiss else ''} {cm:.4f} ms = {1e6 * cm / max(1, ncc):.2f} ns per cylinder contact "
          f"({ncc} contacts, candidates over {ncy} particles + contact kernel + memset); min / max over rounds {min(cyl_ms[False]):.4f} / {max(cyl_ms[False]):.4f}")
    print(f"cylinder pass with per-cylinder totals {cmo:.4f} ms; planar pass in the same run {w:.4f} ms = {1e6 * w / max(1, nc):.2f} ns per wall contact")
    if a.spring > 0 and a.mu_w > 0:
        # SPEC 2.19: the same pass with a tangential spring on the cylinder, advancing (sweep + HIST instance), timed in
        # rounds that alternate with the dissipative pass above (k_t back to 0), so that the two share the clock state
        legs = {"dissipative": [], "spring": []}
        for r in range(a.rounds + 2):
            for leg in ("dissipative", "spring"):
                sp.set_cyl_tangential_spring(a.spring if leg == "spring" else 0.0)
                ts = []
                for _ in range(a.reps):
                    e0.record(st)
                    sp.twist_device(ncy, 0, velc.data_ptr(), qc.data_ptr(), angc.data_ptr(), shc.data_ptr(), twc.data_ptr(), stream=st.cuda_stream)
                    sp.cyl_contact_device(ncy, xc.data_ptr(), qc.data_ptr(), shc.data_ptr(), maskc.data_ptr(), fc.data_ptr(), tc.data_ptr(),
                                          twc.data_ptr(), 1e-3, stream=st.cuda_stream)
                    e1.record(st)
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                if r >= 2:
                    legs[leg].append(float(np.mean(ts)))
        dm, sm = np.median(legs["dissipative"]), np.median(legs["spring"])
        print(f"cylinder pass + twists, dissipative / with the tangential spring (advancing): {dm:.4f} / {sm:.4f} ms "
              f"(sweep and HIST instance: {1e3 * (sm - dm):+.1f} us over {ncy} rows, {ncc} contacts; min / max of the spring leg "
              f"{min(legs['spring']):.4f} / {max(legs['spring']):.4f})")
    if a.rolling is not None:
        # SPEC 2.21: the pass as configured above (the spring leg's k_t back to 0), twists included, without and with the two
        # couples, in rounds that alternate; the bound: 1 + 48 B per particle and 88 B per (particle, cylinder) in reach
        sp.set_cyl_tangential_spring(0.0)
        sp.cylinder_rotation(a.omega)
        legs = {"off": [], "on": []}
        for r in range(a.rounds + 2):
            for leg in ("off", "on") if r % 2 == 0 else ("on", "off"):
                on = leg == "on"
                sp.cylinder_rolling(a.rolling[0] if on else 0.0, a.rolling[1] if on else 0.0)
                sp.cylinder_twisting(a.rolling[2] if on else 0.0, a.rolling[3] if on else 0.0)
                ts = []
                for _ in range(a.reps):
                    e0.record(st)
                    sp.twist_device(ncy, 0, velc.data_ptr(), qc.data_ptr(), angc.data_ptr(), shc.data_ptr(), twc.data_ptr(), stream=st.cuda_stream)
                    sp.cylinder_force_device(ncy, xc.data_ptr(), qc.data_ptr(), shc.data_ptr(), maskc.data_ptr(), fc.data_ptr(), tc.data_ptr(),
                                             twist=twc.data_ptr(), stream=st.cuda_stream)
                    e1.record(st)
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                if r >= 2:
                    legs[leg].append(float(np.mean(ts)))
        off_ms, on_ms = np.median(legs["off"]), np.median(legs["on"])
        # rows in reach: the centres within Rmax of the shell
        reach = int((rad[keep].max() + a.inset - rad[keep] < rmax[0]).sum())
        nbytes = 49 * ncy + 88 * reach
        print(f"cylinder pass + twists without / with rolling and twisting resistance: {off_ms:.4f} / {on_ms:.4f} ms "
              f"(cyl_roll_kernel and the rows it makes the pass keep: {1e3 * (on_ms - off_ms):+.1f} us over {ncy} rows, {reach} in reach, "
              f"{ncc} contacts; min / max of the on leg {min(legs['on']):.4f} / {max(legs['on']):.4f}; its bound of {nbytes} B is "
              f"{nbytes / 8.0e6:.2f} us at 8 TB/s)")
        sp.cylinder_rolling(0.0, 0.0)
        sp.cylinder_twisting(0.0, 0.0)
    if a.ledger and cdiss:
        # SPEC 2.20: the pass as configured above (with the spring if one is given) without and with both ledgers on, i.e.
        # the ordinary instance against its cyl_power_* twin, in rounds that alternate; then the fold of the rows on its own
        hist = a.spring > 0 and a.mu_w > 0
        sp.set_cyl_tangential_spring(a.spring if hist else 0.0)
        legs, fold = {"plain": [], "ledger": []}, []
        for r in range(a.rounds + 2):
            for leg in ("plain", "ledger") if r % 2 == 0 else ("ledger", "plain"):
                if leg == "ledger":
                    sp.set_shell_ledger(True)
                    sp.set_energy_ledger(True)
                else:
                    sp.set_energy_ledger(False)
                    sp.set_shell_ledger(False)
                ts, tf = [], []
                for _ in range(a.reps):
                    e0.record(st)
                    sp.twist_device(ncy, 0, velc.data_ptr(), qc.data_ptr(), angc.data_ptr(), shc.data_ptr(), twc.data_ptr(), stream=st.cuda_stream)
                    sp.cyl_contact_device(ncy, xc.data_ptr(), qc.data_ptr(), shc.data_ptr(), maskc.data_ptr(), fc.data_ptr(), tc.data_ptr(),
                                          twc.data_ptr(), 1e-3, stream=st.cuda_stream)
                    e1.record(st)
                    torch.cuda.synchronize()
                    ts.append(e0.elapsed_time(e1))
                    if leg == "ledger":
                        e0.record(st)
                        sp.ledger_fold_device(1e-3, stream=st.cuda_stream)
                        e1.record(st)
                        torch.cuda.synchronize()
                        tf.append(e0.elapsed_time(e1))
                if r >= 2:
                    legs[leg].append(float(np.mean(ts)))
                    if tf:
                        fold.append(float(np.mean(tf)))
        pm, lm, fm = np.median(legs["plain"]), np.median(legs["ledger"]), np.median(fold)
        tot, _ = sp.shell_ledger()
        print(f"cylinder pass + twists{' with the tangential spring' if hist else ', dissipative'}, ledgers off / on "
              f"(cyl_power_{'spring' if hist else 'dissipative'}_kernel): {pm:.4f} / {lm:.4f} ms ({1e3 * (lm - pm):+.1f} us over {ncy} rows, "
              f"{ncc} contacts; min / max of the ledger leg {min(legs['ledger']):.4f} / {max(legs['ledger']):.4f}); "
              f"fold of the shell rows {1e3 * fm:.1f} us; shell ledger {tot.tolist()}")
        sp.set_energy_ledger(False)
        sp.set_shell_ledger(False)
if a.cone:
    # the particles inside a 30-degree cone along z through the bed's vertical mid-axis, apex 2 below the bed, every centre
    # at least --inset from the wall; the ones nearer than Rmax are the contacts
    c0 = 0.5 * (b["x"].min(axis=0) + b["x"].max(axis=0))
    apex = np.array([c0[0], c0[1], b["x"][:, 2].min() - 2.0])
    cth, sth = np.cos(np.pi / 6), np.sin(np.pi / 6)
    hk = sth * (b["x"][:, 2] - apex[2]) - cth * np.hypot(b["x"][:, 0] - apex[0], b["x"][:, 1] - apex[1])
    keep = hk >= a.inset
    nco = int(keep.sum())
    sp.set_cones([[*apex, 0.0, 0.0, 1.0, cth, sth]], 1000.0, 1.25)
    kd = torch.from_numpy(keep).to(dev)   # every per-particle array by the same rows
    xk, qk, shk = x[kd].contiguous(), q[kd].contiguous(), sh[kd].contiguous()
    velk, angk, maskk = vel[kd].contiguous(), angm[kd].contiguous(), mask[kd].contiguous()
    fk, tk, twk = torch.zeros(nco, 3, dtype=torch.float64, device=dev), torch.zeros(nco, 3, dtype=torch.float64, device=dev), tw[kd].contiguous()
    args = (nco, xk.data_ptr(), qk.data_ptr(), shk.data_ptr(), maskk.data_ptr(), fk.data_ptr(), tk.data_ptr())
    legs = {"elastic": [], "dissipative": [], "spring": []}
    for r in range(a.rounds + 2):
        for leg in legs if r % 2 == 0 else list(legs)[::-1]:
            sp.cone_damping(0.0 if leg == "elastic" else 3.0)
            sp.cone_friction(0.0 if leg == "elastic" else 0.5, 0.0 if leg == "elastic" else 2.0)
            sp.cone_rotation(a.omega)
            sp.conic_spring(4000.0 if leg == "spring" else 0.0)
            ts = []
            for _ in range(a.reps):
                e0.record(st)
                if leg != "elastic":
                    sp.twist_device(nco, 0, velk.data_ptr(), qk.data_ptr(), angk.data_ptr(), shk.data_ptr(), twk.data_ptr(), stream=st.cuda_stream)
                if leg == "spring":
                    sp.conic_contact_device(*args, twk.data_ptr(), 1e-3, stream=st.cuda_stream)
                else:
                    sp.cone_force_device(*args, twist=None if leg == "elastic" else twk.data_ptr(), stream=st.cuda_stream)
                e1.record(st)
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            if r >= 2:
                legs[leg].append(float(np.mean(ts)))
            if leg == "spring":
                xi = sp.conic_history(nco)
    nkc = sp.cone_stats()
    em, dm, sm = (np.median(legs[k]) for k in ("elastic", "dissipative", "spring"))
    print(f"cone pass, elastic / dissipative + twists / advancing spring + twists: {em:.4f} / {dm:.4f} / {sm:.4f} ms "
          f"= {1e6 * em / max(1, nkc):.2f} / {1e6 * dm / max(1, nkc):.2f} / {1e6 * sm / max(1, nkc):.2f} ns per cone contact "
          f"({nkc} contacts, candidates over {nco} particles + contact kernel + memset; the spring leg with the live sweep: "
          f"{1e3 * (sm - dm):+.1f} us; min / max of the spring leg {min(legs['spring']):.4f} / {max(legs['spring']):.4f}; "
          f"{int((xi != 0).any(axis=2).sum())} live rows)")
    sp.set_cones(None)
sp.close()
if twisted or a.wall_vel is not None or a.roll is not None or a.cylinder or a.cone:
    sys.exit(0)   # the whole-step comparison below is the elastic one

# whole steps, walls off / on: a periodic bed with a floor and a lid just outside it in z
from shpair.run import DeviceRun  # noqa: E402
pts, plo, phi = bed.periodic_hcp(a.n, 1.9, (1, 1, 0))
rng = np.random.default_rng(bed.SEED0 + 7)
n = pts.shape[0]
xx = pts + rng.uniform(-0.04, 0.04, pts.shape)
qq = bed.random_quaternions(n, rng)
walls = (np.array([[0, 0, 1, xx[:, 2].min() - a.inset], [0, 0, -1, -(xx[:, 2].max() + a.inset)]]), 1000.0, 1.25)
runs = {}
for label, wl in (("no walls", None), ("floor + lid", walls)):
    s2 = ShPair(0)
    s2.settings(a.nq)
    s2.set_ntypes(1, 1)
    s2.set_shape(0, a.lmax, shapes.random_shape(a.lmax, bed.SEED0 + 2))
    s2.coeff("*", "*", 1000.0, 1.25)
    runs[label] = (s2, DeviceRun(s2, xx, qq, np.zeros(n, np.int32), plo, phi, (1, 1, 0), 0.1, dt=1e-5, walls=wl))
times = {k: [] for k in runs}
for r in range(a.rounds + 2):
    for label, (s2, run) in (list(runs.items()) if r % 2 == 0 else list(runs.items())[::-1]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run.run_native(20)          # blocks until the last step has finished
        if r >= 2:
            times[label].append(1e3 * (time.perf_counter() - t0) / 20)
for label, (s2, run) in runs.items():
    print(f"shstep_run_device, {n} particles, {label}: {np.median(times[label]):.4f} ms per step"
          + (f" ({s2.wall_stats()} wall contacts)" if s2.nwalls else ""))
    s2.close()
