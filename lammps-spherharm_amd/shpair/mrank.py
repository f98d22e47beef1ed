"""Host-side mirror of include/shhalo.h: the N > 1 path of `pair_style sh` (BASELINE configs[3]).

Everything that moves or decides anything is in libshpair.so (csrc/shhalo_api.hip, shhalo_run.cpp, halo_transport.cpp,
halo_kernels.hpp, halo_plan.cpp):
brick geometry, atom migration, ghost selection, the forward / reverse exchange on RCCL point-to-point (or, for
rehearsals of N ranks on one GPU, an in-process hub between host threads) and the timestep loop over all ranks.
This module is the ctypes binding plus `RankRun`, which owns one rank's arrays (torch tensors: memory only) —
what tests and bench.py drive; its call-by-call force pass is the one it shares with run.DeviceRun
(step_pass.force_pass).  The plan functions (`plan_*`) are the library's pure host planner and need no GPU.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import HaloArrays, HaloGeometry, HaloLayout, HaloRunParams, HaloStats, ShPairError
from .step_pass import StepView, apply_contact_options, force_pass, rank_arrays

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _chk(rc, what=""):
    if rc:
        raise ShPairError(rc, what)


def _i3(v):
    return (C.c_int * 3)(*[int(a) for a in v])


def _d3(v):
    return (C.c_double * 3)(*[float(a) for a in v])


# ---- the pure host planner (no GPU) ------------------------------------------------------------------------------
def proc_grid(nranks):
    g = (C.c_int * 3)()
    _chk(capi.load_library().shhalo_proc_grid(int(nranks), g), "shhalo_proc_grid")
    return tuple(g)


def plan_geometry(grid, lo, hi, periodic, cut, rank):
    g = HaloGeometry()
    _chk(capi.load_library().shhalo_plan_geometry(_i3(grid), _d3(lo), _d3(hi), _i3(periodic), float(cut), int(rank), C.byref(g)),
         f"shhalo_plan_geometry(grid={tuple(grid)}, cut={cut})")
    return g


def plan_owner(geo, x):
    """Wrapped copy of x and the owning rank of every row."""
    xw = np.ascontiguousarray(x, dtype=np.float64).copy()
    owner = np.zeros(xw.shape[0], dtype=np.int32)
    _chk(capi.load_library().shhalo_plan_owner(C.byref(geo), xw.shape[0], xw.ctypes.data_as(_dp), owner.ctypes.data_as(_ip)))
    return xw, owner


def plan_ghost_mask(geo, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    mask = np.zeros(x.shape[0], dtype=np.uint32)
    _chk(capi.load_library().shhalo_plan_ghost_mask(C.byref(geo), x.shape[0], x.ctypes.data_as(_dp),
                                                    mask.ctypes.data_as(C.POINTER(C.c_uint))))
    return mask


def plan_layout(geo, send_cnt, recv_cnt):
    lay = HaloLayout()
    s = (C.c_int * 27)(*[int(v) for v in send_cnt])
    r = (C.c_int * 27)(*[int(v) for v in recv_cnt])
    _chk(capi.load_library().shhalo_plan_layout(C.byref(geo), s, r, C.byref(lay)))
    return lay


def unique_id():
    """ncclGetUniqueId as 128 bytes (rank 0; broadcast it to the other ranks)."""
    buf = C.create_string_buffer(128)
    _chk(capi.load_library().shhalo_get_unique_id(buf), "shhalo_get_unique_id (is librccl loadable?)")
    return buf.raw


_szp = C.POINTER(C.c_size_t)
_vpp = C.POINTER(C.c_void_p)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, _ip, _vpp, _szp, C.c_int, _ip, _vpp, _szp)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int)


class GlooStaged:
    """The caller's side of the host-staged transport (shhalo_create_staged) on torch.distributed's CPU backend: the
    library hands over page-locked host buffers, this class moves them with isend / irecv and combines the all-reduce
    values — what MPI_Isend / MPI_Irecv / MPI_Allreduce would do in a LAMMPS host without GPU-aware MPI.  One instance
    per rank; keep it alive as long as the halo context."""

    def __init__(self, dist, group=None):
        import torch
        self.dist, self.group, self.torch = dist, group, torch
        self.calls = 0
        self.last_error = ""

        def _view(ptr, nbytes, dtype):
            buf = (C.c_char * int(nbytes)).from_address(int(ptr))
            return torch.frombuffer(buf, dtype=dtype)

        def _exchange(user, ns, speer, sptr, sbytes, nr, rpeer, rptr, rbytes):
            try:
                reqs = [dist.irecv(_view(rptr[k], rbytes[k], torch.uint8), src=int(rpeer[k]), group=group) for k in range(nr)]
                reqs += [dist.isend(_view(sptr[k], sbytes[k], torch.uint8), dst=int(speer[k]), group=group) for k in range(ns)]
                for r in reqs:
                    r.wait()
                self.calls += 1
                return 0
            except BaseException as e:  # noqa: BLE001 — never let an exception cross the C frame
                self.last_error = repr(e)
                return 1

        def _allreduce(user, data, n, kind):
            try:
                if kind == 0:
                    t = _view(data, 4 * n, torch.int32)
                    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
                else:
                    t = _view(data, 8 * n, torch.float64)
                    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
                return 0
            except BaseException as e:  # noqa: BLE001
                self.last_error = repr(e)
                return 1
        self.exchange_fn = EXCHANGE_FN(_exchange)
        self.allreduce_fn = ALLREDUCE_FN(_allreduce)


class Hub:
    """In-process transport between the rank THREADS of one process (rehearsal of N ranks on one GPU)."""

    def __init__(self, nranks):
        self._lib = capi.load_library()
        h = C.c_void_p()
        _chk(self._lib.shhalo_hub_create(C.byref(h), int(nranks)))
        self._h, self.nranks = h, nranks

    def close(self):
        if getattr(self, "_h", None):
            self._lib.shhalo_hub_destroy(self._h)
            self._h = None


class Halo:
    """One rank's shhalo context."""

    def __init__(self, sp, rank, nranks, grid, lo, hi, periodic, skin, hub=None, unique_id_bytes=None, staged=None):
        self._lib = capi.load_library()
        self.sp = sp
        h = C.c_void_p()
        self._staged = staged    # keeps the callbacks alive
        if staged is not None:
            rc = self._lib.shhalo_create_staged(C.byref(h), sp._h, C.cast(staged.exchange_fn, C.c_void_p), C.cast(staged.allreduce_fn, C.c_void_p),
                                                None, int(rank), int(nranks), _i3(grid), _d3(lo), _d3(hi), _i3(periodic), float(skin))
        elif unique_id_bytes is not None:
            idb = C.create_string_buffer(bytes(unique_id_bytes), 128)
            rc = self._lib.shhalo_create_rccl(C.byref(h), sp._h, idb, int(rank), int(nranks), _i3(grid), _d3(lo), _d3(hi),
                                              _i3(periodic), float(skin))
        else:
            rc = self._lib.shhalo_create_local(C.byref(h), sp._h, hub._h if hub is not None else None, int(rank), int(nranks),
                                               _i3(grid), _d3(lo), _d3(hi), _i3(periodic), float(skin))
        if rc:
            raise ShPairError(rc, self._lib.shpair_last_error(sp._h).decode())
        self._h = h
        self.rank, self.nranks = rank, nranks

    def close(self):
        if getattr(self, "_h", None):
            self._lib.shhalo_destroy(self._h)
            self._h = None

    def _chk(self, rc):
        if rc:
            raise ShPairError(rc, self._lib.shhalo_last_error(self._h).decode())

    def geometry(self):
        g = HaloGeometry()
        self._chk(self._lib.shhalo_get_geometry(self._h, C.byref(g)))
        return g

    def exchange(self, arrays, stream=None):
        self._chk(self._lib.shhalo_exchange_device(self._h, C.byref(arrays), stream))

    def borders(self, arrays, stream=None):
        ng = C.c_int(0)
        self._chk(self._lib.shhalo_borders_device(self._h, C.byref(arrays), C.byref(ng), stream))
        return ng.value

    def neighbor_build(self, arrays, nghost, stream=None):
        """shhalo_neighbor_build_device: the half list over the brick + ghosts; collective (failures are agreed on)."""
        np_ = C.c_int(0)
        self._chk(self._lib.shhalo_neighbor_build_device(self._h, C.byref(arrays), int(nghost), C.byref(np_), stream))
        return np_.value

    def forward(self, x, quat, stream=None):
        self._chk(self._lib.shhalo_forward_device(self._h, x, quat, stream))

    def forward_twist(self, x, quat, twist, stream=None):
        """shhalo_forward_twist_device: the forward exchange with the owners' twists (13 doubles per row); the ghost rows of
        x, quat and twist [nmax][6] are written."""
        self._chk(self._lib.shhalo_forward_twist_device(self._h, x, quat, twist, stream))

    def reverse(self, f, torque, stream=None):
        self._chk(self._lib.shhalo_reverse_device(self._h, f, torque, stream))

    def check_rebuild(self, nlocal, x, stream=None):
        r = C.c_int(0)
        self._chk(self._lib.shhalo_check_rebuild_device(self._h, int(nlocal), x, C.byref(r), stream))
        return bool(r.value)

    def allreduce_sum(self, data_ptr, n, stream=None):
        self._chk(self._lib.shhalo_allreduce_sum_device(self._h, data_ptr, int(n), stream))

    def transport_selftest(self, nbytes=1 << 20, stream=None):
        """shhalo_transport_selftest: this rank sends nbytes to itself through the transport's exchange (RCCL: ncclSend /
        ncclRecv with the caller as peer) and all-reduces three doubles and two ints; raises on a mismatch."""
        self._chk(self._lib.shhalo_transport_selftest(self._h, int(nbytes), stream))

    def stats(self):
        s = HaloStats()
        self._chk(self._lib.shhalo_get_stats(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in HaloStats._fields_}

    def run(self, arrays, params, nsteps, nghost, stream=None, timed=False):
        """shhalo_run_device. Returns (nghost, rebuilds, kernel_ms_sum)."""
        ng, nr, ms = C.c_int(int(nghost)), C.c_int(0), C.c_double(0.0)
        self._chk(self._lib.shhalo_run_device(self._h, C.byref(arrays), C.byref(params), int(nsteps), C.byref(ng), C.byref(nr),
                                              C.byref(ms) if timed else None, stream))
        return ng.value, nr.value, ms.value


class RankRun:
    """One rank of a device-resident multi-rank run: its arrays (torch owns the memory) and the calls into the C ABI.

    Every rank (process with RCCL, or thread with a Hub) constructs one with ITS atoms and then calls the same
    methods in the same order (they are collective where LAMMPS' Comm calls are)."""

    def __init__(self, sp, halo, x, quat, shtype, tag, type_=None, v=None, angmom=None, mask=None, groupbit=1, dt=1e-3,
                 gravity=(0.0, 0.0, 0.0), gamma_t=0.0, gamma_r=0.0, device="cuda:0", capacity=None, check_every=1, **contact):
        """contact: walls, pair_damping, wall_damping, pair_friction, wall_friction, wall_velocity, pair_rolling,
        pair_twisting, wall_rolling, wall_twisting, as step_pass.apply_contact_options takes them (None leaves the context's as they are).  Every rank passes the same:
        each applies the walls to the particles it owns and advances its own copy of the planes with the same arithmetic.
        The cylinder options (cylinders ... cylinder_rolling, cylinder_twisting, docs/SPEC.md §2.18-§2.21) are single-rank:
        this loop refuses to run while a cylinder is set.  So are the cone options (cones ... cone_rotation, §2.22; conic_spring, §2.23; conic_rolling, conic_twisting, §2.24)."""
        import torch
        self.torch = torch
        self.sp, self.halo = sp, halo
        self.dt, self.groupbit, self.check_every = float(dt), int(groupbit), max(1, int(check_every))
        self.g = tuple(float(c) for c in gravity)
        self.gamma_t, self.gamma_r = float(gamma_t), float(gamma_r)
        n = int(np.asarray(x).shape[0])
        self.nmax = int(capacity) if capacity is not None else int(3.0 * max(n, 64)) + 256
        rank_arrays(self, device, n, self.nmax, self.nmax, x, quat, shtype, type_=type_, v=v, angmom=angmom, mask=mask, tag=tag)
        self.q[n:, 0] = 1.0
        # (w, omega) of owned and ghost rows, docs/SPEC.md §2.10: always, the coefficients may be set later
        self.twist = torch.zeros(self.nmax, 6, dtype=torch.float64, device=self.dev)
        self.stream = sp.own_stream()
        apply_contact_options(sp, **contact)
        a = HaloArrays()
        a.nlocal, a.nmax = n, self.nmax
        a.x, a.v, a.quat, a.angmom = self.x.data_ptr(), self.v.data_ptr(), self.q.data_ptr(), self.L.data_ptr()
        a.f, a.torque = self.f.data_ptr(), self.tq.data_ptr()
        a.type, a.shtype, a.mask, a.tag = self.ty.data_ptr(), self.sh.data_ptr(), self.mask.data_ptr(), self.tag.data_ptr()
        self.a = a
        self.nghost = 0
        self.npairs = 0
        self.builds = 0
        self.kernel_ms = 0.0
        torch.cuda.synchronize()   # the tensors were filled on torch's stream; everything below runs on the context's
        self.rebuild()
        self.force()

    @property
    def n(self):
        return self.a.nlocal

    def sync(self):
        self.sp.synchronize()

    def rebuild(self):
        """Comm::exchange + Comm::borders + Neighbor::build."""
        self.halo.exchange(self.a, self.stream)
        self.nghost = self.halo.borders(self.a, self.stream)
        self.npairs = self.halo.neighbor_build(self.a, self.nghost, self.stream)
        self.builds += 1

    def force(self, eflag=False, advance=False):
        """advance: the force pass of a step — the planes of translating walls move by dt ahead of the wall pass, as in
        step_after_reverse."""
        a, st, halo = self.a, self.stream, self.halo
        if self.sp.has_history:   # as shhalo_run_device: xi does not migrate with its atoms yet (docs/SPEC.md §2.14)
            raise ShPairError(-4, "tangential history is single-rank (set every tangential spring to 0 or use run.DeviceRun)")
        if self.sp.has_wall_history:   # ... nor does xi_iw of the walls (§2.15)
            raise ShPairError(-4, "wall tangential history is single-rank (set every wall tangential spring to 0 or use run.DeviceRun)")
        if self.sp.ncylinders:   # ... and cylindrical walls are not modelled over several ranks (§2.18)
            raise ShPairError(-4, "cylindrical walls are single-rank (remove them with set_cylinders(None) or use run.DeviceRun)")
        if self.sp.ncones:   # ... nor are conical walls (§2.22)
            raise ShPairError(-4, "conical walls are single-rank (remove them with set_cones(None) or use run.DeviceRun)")
        self.sync()
        self.f.zero_()
        self.tq.zero_()
        if eflag:
            self.ev.zero_()
        self.torch.cuda.synchronize()
        v = StepView(a.nlocal, self.nghost, a.x, a.quat, a.v, a.angmom, a.type, a.shtype, a.mask, a.f, a.torque,
                     self.twist.data_ptr(), self.groupbit, self.dt, self.g, self.gamma_t, self.gamma_r, st)

        # contact dissipation (docs/SPEC.md §2.10, §2.11): the twist kernel fills the owned rows only; with a pair
        # coefficient set the twists travel to the ghost rows with the positions (one message of 13 doubles per row)
        def forward(twist):
            if twist is None:
                halo.forward(a.x, a.quat, st)
            else:
                halo.forward_twist(a.x, a.quat, twist, st)
        force_pass(self.sp, v, forward, lambda: halo.reverse(a.f, a.torque, st), 0, eflag=eflag, ev=self.ev.data_ptr(),
                   advance=advance)
        self.sync()

    def run(self, nsteps, eflag_last=False, timed=False):
        """Verlet::run over all ranks inside the library (shhalo_run_device)."""
        p = HaloRunParams()
        p.dt, p.groupbit = self.dt, self.groupbit
        p.gravity = (self.g[0], self.g[1], self.g[2])
        p.gamma_t, p.gamma_r, p.check_every = self.gamma_t, self.gamma_r, self.check_every
        p.eflag_last = 1 if eflag_last else 0
        p.ev_dev = self.ev.data_ptr() if eflag_last else None
        if eflag_last:
            self.ev.zero_()
            self.torch.cuda.synchronize()
        self.nghost, nreb, ms = self.halo.run(self.a, p, nsteps, self.nghost, stream=self.stream, timed=timed)
        self.builds += nreb
        self.kernel_ms += ms
        return nreb

    def save_state(self):
        """Everything a rank needs to come back to this instant: the owned rows of every per-atom array (clones on the
        device) and their count.  Ghosts, plan and list are NOT saved: restore_state() rebuilds them."""
        self.sync()
        n = self.a.nlocal
        keep = {k: getattr(self, k)[:n].clone() for k in ("x", "q", "v", "L", "tag", "sh", "ty", "mask")}
        self.torch.cuda.synchronize()
        return dict(n=n, arrays=keep)

    def restore_state(self, state):
        """Back to save_state()'s instant: owned rows, then (collectively, every rank calls it) migration + ghost plan +
        list + forces, as after the constructor.  The list is built under the context's CURRENT options (a changed
        "halo_overlap" takes effect here)."""
        self.sync()
        n = state["n"]
        for k, t in state["arrays"].items():
            getattr(self, k)[:n] = t
        self.a.nlocal = n
        self.torch.cuda.synchronize()
        self.rebuild()
        self.force()

    def owned(self):
        """(tag, x, v, quat, f, torque) of the owned atoms on the host, sorted by tag."""
        self.sync()
        n = self.a.nlocal
        t = self.tag[:n].cpu().numpy()
        o = np.argsort(t)
        return (t[o], self.x[:n].cpu().numpy()[o], self.v[:n].cpu().numpy()[o], self.q[:n].cpu().numpy()[o],
                self.f[:n].cpu().numpy()[o], self.tq[:n].cpu().numpy()[o])
