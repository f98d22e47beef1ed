"""ctypes binding of include/shpair.h (the C ABI of the HIP contact path).

Mirrors the LAMMPS call order of the reference's PairSH (sources ABSENT FROM
MOUNT): settings() -> coeff() -> init_style()/init_one() ->
[neighbour build] -> compute(eflag, vflag).
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class ShPairError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = load_library().shpair_strerror(code).decode()
        super().__init__(f"shpair error {code}: {msg}" + (f" — {detail}" if detail else ""))


class Stats(C.Structure):
    _fields_ = [("n_candidates", C.c_longlong), ("n_contact", C.c_longlong), ("n_touching", C.c_longlong),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double)]


class KernelInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("lmax", "compiled_order", "vgprs", "scratch_bytes", "lds_bytes_per_wave", "ring_rows",
                                       "waves_per_simd_vgpr", "waves_per_cu_lds", "waves_per_cu", "family", "waves_per_pair",
                                       "needv", "weighted", "queue_entries", "specialised")]


class StepArrays(C.Structure):
    """shstep_arrays of include/shstep.h."""
    _fields_ = [("nlocal", C.c_int), ("nmax", C.c_int),
                ("x", C.c_void_p), ("v", C.c_void_p), ("quat", C.c_void_p), ("angmom", C.c_void_p), ("f", C.c_void_p),
                ("torque", C.c_void_p), ("type", C.c_void_p), ("shtype", C.c_void_p), ("mask", C.c_void_p),
                ("groupbit", C.c_int), ("dt", C.c_double), ("gravity", C.c_double * 3), ("gamma_t", C.c_double),
                ("gamma_r", C.c_double), ("check_every", C.c_int)]


class HaloGeometry(C.Structure):
    """shhalo_geometry of include/shhalo.h."""
    _fields_ = [("grid", C.c_int * 3), ("coord", C.c_int * 3), ("rank", C.c_int), ("nranks", C.c_int),
                ("periodic", C.c_int * 3), ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("blo", C.c_double * 3),
                ("bhi", C.c_double * 3), ("cut", C.c_double), ("peer", C.c_int * 27), ("shift", (C.c_double * 3) * 27)]


class HaloLayout(C.Structure):
    """shhalo_layout of include/shhalo.h."""
    _fields_ = [("send_off", C.c_int * 27), ("send_cnt", C.c_int * 27), ("recv_off", C.c_int * 27), ("recv_cnt", C.c_int * 27),
                ("nsend", C.c_int), ("nghost", C.c_int), ("npeers", C.c_int), ("peer_rank", C.c_int * 26),
                ("peer_send_off", C.c_int * 26), ("peer_send_cnt", C.c_int * 26), ("peer_recv_off", C.c_int * 26),
                ("peer_recv_cnt", C.c_int * 26)]


class HaloArrays(C.Structure):
    """shhalo_arrays of include/shhalo.h."""
    _fields_ = [("nlocal", C.c_int), ("nmax", C.c_int), ("x", C.c_void_p), ("v", C.c_void_p), ("quat", C.c_void_p),
                ("angmom", C.c_void_p), ("f", C.c_void_p), ("torque", C.c_void_p), ("type", C.c_void_p), ("shtype", C.c_void_p),
                ("mask", C.c_void_p), ("tag", C.c_void_p)]


class HaloStats(C.Structure):
    _fields_ = [("nranks_transport", C.c_int), ("npeers", C.c_int), ("nsend_rows", C.c_int), ("nghost_rows", C.c_int),
                ("rebuilds", C.c_longlong), ("migrated_out", C.c_longlong), ("migrated_in", C.c_longlong),
                ("forward_bytes_per_step", C.c_longlong), ("reverse_bytes_per_step", C.c_longlong), ("transport", C.c_int),
                ("rccl_version", C.c_int)]


class HaloRunParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("groupbit", C.c_int), ("gravity", C.c_double * 3), ("gamma_t", C.c_double),
                ("gamma_r", C.c_double), ("check_every", C.c_int), ("eflag_last", C.c_int), ("ev_dev", C.c_void_p)]


_up = C.POINTER(C.c_uint)
_idp = C.c_char_p  # SHHALO_UNIQUE_ID_BYTES raw bytes

# every symbol include/shpair.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "shpair_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "shpair_destroy": (None, [C.c_void_p]),
    "shpair_strerror": (C.c_char_p, [C.c_int]),
    "shpair_last_error": (C.c_char_p, [C.c_void_p]),
    "shpair_version": (C.c_char_p, []),
    "shpair_settings": (C.c_int, [C.c_void_p, C.c_int]),
    "shpair_set_ntypes": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "shpair_set_shape": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_double]),
    "shpair_set_coeff": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]),
    "shpair_get_rmax": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shpair_shape_radius": (C.c_int, [C.c_int, _dp, _dp, _dp]),
    "shpair_shape_default_rmax": (C.c_int, [C.c_int, _dp, _dp]),
    "shpair_set_neighbors": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, C.POINTER(_ip)]),
    "shpair_set_neighbors_csr": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip, _ip]),
    "shpair_set_neighbors_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int, C.c_void_p]),
    "shpair_compute": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _ip, _ip, C.c_int, C.c_int, C.c_int,
                                 _dp, _dp, _dp, _dp]),
    "shpair_compute_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "shpair_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "shpair_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "shpair_get_kernel_info": (C.c_int, [C.c_void_p, C.POINTER(KernelInfo)]),
    "shpair_set_pair_output": (C.c_int, [C.c_void_p, C.c_void_p]),
    "shpair_set_peratom_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "shpair_set_peratom_host": (C.c_int, [C.c_void_p, _dp, _dp]),
    "shpair_pin_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "shpair_unpin_host": (C.c_int, [C.c_void_p, C.c_void_p]),
    "shpair_fp64_peak": (C.c_int, [C.c_void_p, C.c_int, C.c_double, _dp, _dp]),
    "shpair_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "shpair_synchronize": (C.c_int, [C.c_void_p]),
    # include/shstep.h
    "shstep_shape_mass_props": (C.c_int, [C.c_int, _dp, _dp]),
    "shstep_set_density": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "shstep_get_body": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "shstep_nve_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p]),
    "shstep_nve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int]),
    "shstep_force_clear_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "shstep_post_force_device": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_double, C.c_double] + [C.c_void_p] * 5 +
                                 [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "shstep_energies_device": (C.c_int, [C.c_void_p, C.c_int, _dp] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p]),
    "shstep_set_box": (C.c_int, [C.c_void_p, _dp, _dp, _ip, C.c_double]),
    "shstep_borders_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [_ip, C.c_void_p]),
    "shstep_forward_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "shstep_reverse_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "shstep_neighbor_build_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _ip,
                                               C.c_void_p]),
    "shstep_neighbor_check_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, _ip, C.c_void_p]),
    "shstep_copy_neighbors": (C.c_int, [C.c_void_p, _ip, _ip]),
    "shstep_set_walls": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "shstep_wall_force_device": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4),
    "shstep_wall_force": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _ip, _ip, C.c_int, _dp, _dp, _dp]),
    "shstep_get_wall_stats": (C.c_int, [C.c_void_p, _ip]),
    "shstep_set_wall_velocity": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_advance_walls_device": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "shstep_get_walls": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_pair_damping": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double]),
    "shstep_set_wall_damping": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_twist_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "shstep_pair_damping_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3),
    "shstep_wall_force_damped_device": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5),
    "shstep_set_pair_friction": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]),
    "shstep_set_wall_friction": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_pair_dissipation_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3),
    "shstep_set_pair_tangential_spring": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double]),
    "shstep_pair_contact_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_double] +
                                   [C.c_void_p] * 3),
    "shstep_copy_contact_history": (C.c_int, [C.c_void_p, _dp]),
    "shstep_set_contact_history": (C.c_int, [C.c_void_p, _dp]),
    "shstep_reset_contact_history": (C.c_int, [C.c_void_p]),
    "shstep_set_wall_tangential_spring": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_wall_contact_device": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 +
                                   [C.c_double, C.c_void_p]),
    "shstep_copy_wall_history": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_wall_history": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_reset_wall_history": (C.c_int, [C.c_void_p]),
    "shstep_set_pair_rolling": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]),
    "shstep_set_pair_twisting": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]),
    "shstep_pair_rolling_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 2),
    "shstep_set_wall_rolling": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_set_wall_twisting": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_set_energy_ledger": (C.c_int, [C.c_void_p, C.c_int]),
    "shstep_ledger_fold_device": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "shstep_get_energy_ledger": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp]),
    "shstep_reset_energy_ledger": (C.c_int, [C.c_void_p]),
    "shstep_set_cylinders": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "shstep_set_cylinder_damping": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_cylinder_friction": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_set_cylinder_rotation": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_cylinder_force_device": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5),
    "shstep_get_cylinder_stats": (C.c_int, [C.c_void_p, _ip]),
    "shstep_get_cylinders": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_cones": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "shstep_set_cone_damping": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_cone_friction": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_set_cone_rotation": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_cone_force_device": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5),
    "shstep_get_cone_stats": (C.c_int, [C.c_void_p, _ip]),
    "shstep_get_cones": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_conic_tangential_spring": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_rolling_con": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_set_twisting_con": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_conic_contact_device": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 +
                                    [C.c_double, C.c_void_p]),
    "shstep_copy_conic_history": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_conic_history": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_reset_conic_history": (C.c_int, [C.c_void_p]),
    "shstep_set_cyl_tangential_spring": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_rolling_cyl": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_set_twisting_cyl": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "shstep_cyl_contact_device": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 +
                                  [C.c_double, C.c_void_p]),
    "shstep_copy_cyl_history": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_set_cyl_history": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "shstep_reset_cyl_history": (C.c_int, [C.c_void_p]),
    "shstep_set_shell_ledger": (C.c_int, [C.c_void_p, C.c_int]),
    "shstep_get_shell_ledger": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp]),
    "shstep_run_device": (C.c_int, [C.c_void_p, C.POINTER(StepArrays), C.c_int, C.c_int, _ip, _ip, C.c_void_p]),
    # include/shhalo.h
    "shhalo_proc_grid": (C.c_int, [C.c_int, _ip]),
    "shhalo_plan_geometry": (C.c_int, [_ip, _dp, _dp, _ip, C.c_double, C.c_int, C.POINTER(HaloGeometry)]),
    "shhalo_plan_owner": (C.c_int, [C.POINTER(HaloGeometry), C.c_int, _dp, _ip]),
    "shhalo_plan_ghost_mask": (C.c_int, [C.POINTER(HaloGeometry), C.c_int, _dp, _up]),
    "shhalo_plan_layout": (C.c_int, [C.POINTER(HaloGeometry), _ip, _ip, C.POINTER(HaloLayout)]),
    "shhalo_get_unique_id": (C.c_int, [C.c_void_p]),
    "shhalo_create_rccl": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, _dp, _dp, _ip,
                                     C.c_double]),
    "shhalo_hub_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "shhalo_hub_destroy": (None, [C.c_void_p]),
    "shhalo_create_staged": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, _dp,
                                       _dp, _ip, C.c_double]),
    "shhalo_create_local": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, _dp, _dp, _ip,
                                      C.c_double]),
    "shhalo_destroy": (None, [C.c_void_p]),
    "shhalo_last_error": (C.c_char_p, [C.c_void_p]),
    "shhalo_get_geometry": (C.c_int, [C.c_void_p, C.POINTER(HaloGeometry)]),
    "shhalo_exchange_device": (C.c_int, [C.c_void_p, C.POINTER(HaloArrays), C.c_void_p]),
    "shhalo_borders_device": (C.c_int, [C.c_void_p, C.POINTER(HaloArrays), _ip, C.c_void_p]),
    "shhalo_neighbor_build_device": (C.c_int, [C.c_void_p, C.POINTER(HaloArrays), C.c_int, _ip, C.c_void_p]),
    "shhalo_forward_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "shhalo_forward_twist_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "shhalo_reverse_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "shhalo_check_rebuild_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, _ip, C.c_void_p]),
    "shhalo_allreduce_sum_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "shhalo_transport_selftest": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "shhalo_get_stats": (C.c_int, [C.c_void_p, C.POINTER(HaloStats)]),
    "shhalo_run_device": (C.c_int, [C.c_void_p, C.POINTER(HaloArrays), C.POINTER(HaloRunParams), C.c_int, _ip, _ip, _dp,
                                    C.c_void_p]),
}


def library_path():
    """libshpair.so beside this file.  SHPAIR_LIB=<file name in this directory> selects a diagnostic build (ablation /
    statistics libraries made by `make abl` / `make stats`: some give WRONG results by construction) — honoured only
    together with SHPAIR_DIAGNOSTIC=1, refused loudly otherwise; there is no other fallback."""
    name = os.environ.get("SHPAIR_LIB")
    if name and name != "libshpair.so":
        if os.environ.get("SHPAIR_DIAGNOSTIC") != "1":
            raise ImportError(f"SHPAIR_LIB={name} selects a diagnostic build of libshpair; set SHPAIR_DIAGNOSTIC=1 as well "
                              "if that is what you mean (profiling tools do), or unset SHPAIR_LIB")
        return os.path.join(_HERE, name)
    return os.path.join(_HERE, "libshpair.so")


def library_name():
    """Base name of the library this process loaded (bench.py prints it in its JSON line)."""
    return os.path.basename(library_path())


def load_library():
    """Loads libshpair.so. Raises (never falls back) if it is not built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise ImportError(f"{path} is not built: run `make -C lammps-spherharm_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
        # PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).
        # Whichever is loaded first serves the whole process, and torch cannot see the
        # GPU behind the system runtime ("No HIP GPUs are available"). So when torch is
        # installed it is imported first and libshpair.so binds to torch's runtime; a
        # LAMMPS process (no torch) binds to /opt/rocm's through the library's RUNPATH.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            if os.environ.get("SHPAIR_AB_OLD_LIB") and not hasattr(lib, name):
                continue  # tools/ab_libs.py timing an older build that predates an entry point
            fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def shape_radius(lmax, anm, u):
    anm, pa = _d(anm)
    u, pu = _d(u)
    r = C.c_double()
    rc = load_library().shpair_shape_radius(lmax, pa, pu, C.byref(r))
    if rc:
        raise ShPairError(rc)
    return r.value


def shape_default_rmax(lmax, anm):
    anm, pa = _d(anm)
    r = C.c_double()
    rc = load_library().shpair_shape_default_rmax(lmax, pa, C.byref(r))
    if rc:
        raise ShPairError(rc)
    return r.value


def shape_mass_props(lmax, anm):
    """(V, c[3], J_c xx,yy,zz,xy,xz,yz) at unit density (docs/SPEC.md §5)."""
    anm, pa = _d(anm)
    out = np.zeros(10)
    rc = load_library().shstep_shape_mass_props(lmax, pa, out.ctypes.data_as(_dp))
    if rc:
        raise ShPairError(rc)
    return out


def _per_wall(value, nwalls, width=None):
    """A coefficient of the walls as the setters take it: one value for all of them (a scalar; with `width`, one vector) or
    one per wall, which goes through as it is."""
    value = np.asarray(value, dtype=np.float64)
    if value.ndim == (0 if width is None else 1):
        return np.broadcast_to(value, (nwalls,) if width is None else (nwalls, width))
    return value


def cone_record(apex, axis, theta):
    """The 8 doubles of a cone as ShPair.set_cones takes them: the apex, the unit axis from the apex into the opening (as
    given: it is not normalised here) and the cosine and sine of the half-angle theta, 0 < theta < pi/2."""
    return np.array([*np.asarray(apex, dtype=np.float64), *np.asarray(axis, dtype=np.float64), np.cos(theta), np.sin(theta)])


# One row per surface family: what the copies of a family's methods differ in, and nothing else.  rows: the name of the
# geometry argument in messages; width / xi: the doubles of a geometry record and of a history entry per (particle, surface);
# the rest: the C symbol of each role, copied from SYMBOLS (the names are irregular; here is where that is written down).
# A new family, or a new law on these three, starts from a row or a column here.
_SurfaceFamily = namedtuple("_SurfaceFamily", "noun rows width xi set damping friction rotation spring rolling twisting force "
                                              "contact copy_history set_history reset_history stats get")
_WALL = _SurfaceFamily(
    "wall", "planes", 4, 3, "shstep_set_walls", "shstep_set_wall_damping", "shstep_set_wall_friction", None,
    "shstep_set_wall_tangential_spring", "shstep_set_wall_rolling", "shstep_set_wall_twisting", "shstep_wall_force_damped_device",
    "shstep_wall_contact_device", "shstep_copy_wall_history", "shstep_set_wall_history", "shstep_reset_wall_history",
    "shstep_get_wall_stats", "shstep_get_walls")
_CYLINDER = _SurfaceFamily(
    "cylinder", "cylinders", 7, 2, "shstep_set_cylinders", "shstep_set_cylinder_damping", "shstep_set_cylinder_friction",
    "shstep_set_cylinder_rotation", "shstep_set_cyl_tangential_spring", "shstep_set_rolling_cyl", "shstep_set_twisting_cyl",
    "shstep_cylinder_force_device", "shstep_cyl_contact_device", "shstep_copy_cyl_history", "shstep_set_cyl_history",
    "shstep_reset_cyl_history", "shstep_get_cylinder_stats", "shstep_get_cylinders")
_CONE = _SurfaceFamily(
    "cone", "cones", 8, 3, "shstep_set_cones", "shstep_set_cone_damping", "shstep_set_cone_friction", "shstep_set_cone_rotation",
    "shstep_set_conic_tangential_spring", "shstep_set_rolling_con", "shstep_set_twisting_con", "shstep_cone_force_device",
    "shstep_conic_contact_device", "shstep_copy_conic_history", "shstep_set_conic_history", "shstep_reset_conic_history",
    "shstep_get_cone_stats", "shstep_get_cones")
_FAMILIES = (_WALL, _CYLINDER, _CONE)


def _any_both(a, b):
    """Some surface has both of two coefficients non-zero."""
    return bool(np.any((np.asarray(a) != 0.0) & (np.asarray(b) != 0.0)))


class _SurfaceFlags:
    """The coefficients of one surface family as its setters took them, and the library's predicates of them
    (csrc/shstep_state.hpp).  Friction and history are derived from the arrays together, as the library does (docs/SPEC.md
    §2.11, §2.15), so the setters may come in any order; a surface has rolling or twisting resistance iff both coefficients
    of the kind are non-zero (§2.17)."""

    def __init__(self):
        self.reset(0)

    def reset(self, n):
        """The family's geometry setter: n surfaces, every coefficient back to zero."""
        self.n = int(n)
        self.gamma = self.mu = self.gamma_t = self.k_t = np.zeros(self.n)
        self.roll = self.twist = False

    def damping(self, gamma):
        self.gamma = np.array(gamma, dtype=np.float64)

    def friction(self, mu, gamma_t):
        self.mu, self.gamma_t = np.array(mu, dtype=np.float64), np.array(gamma_t, dtype=np.float64)

    def rotation(self, omega):
        """Omega enters the friction only: alone it is no coefficient, and nothing is kept."""

    def spring(self, kt):
        self.k_t = np.array(kt, dtype=np.float64)

    def rolling(self, mu_r, gamma_r):
        self.roll = _any_both(mu_r, gamma_r)

    def twisting(self, mu_tw, gamma_tw):
        self.twist = _any_both(mu_tw, gamma_tw)

    damp = property(lambda self: bool(np.any(self.gamma != 0.0)), doc="Some gamma != 0.")
    fric = property(lambda self: _any_both(self.mu, self.gamma_t), doc="Some surface has mu != 0 and gamma_t != 0.")
    hist = property(lambda self: _any_both(self.mu, self.k_t), doc="Some surface has mu != 0 and k_t != 0.")
    diss = property(lambda self: self.damp or self.fric, doc="Damping or friction (the rotation alone is no coefficient).")
    rolls = property(lambda self: self.roll or self.twist, doc="Some surface has rolling or twisting resistance.")
    reads_twists = property(lambda self: self.diss or self.hist or self.rolls, doc="A coefficient is set: the pass reads twists.")


class _Of:
    """A name of _StepFlags that is a name of one family's _SurfaceFlags, method or property alike; on the class itself, the
    _SurfaceFlags attribute."""

    def __init__(self, noun, name):
        self.noun, self.name = noun, name

    def __get__(self, flags, owner=None):
        return getattr(_SurfaceFlags if flags is None else flags.surface[self.noun], self.name)


class _StepFlags:
    """What the setters of one ShPair have switched on: the binding's copy of the flags behind the library's step
    predicates (csrc/shpair_ctx.hpp, csrc/shstep_state.hpp).  The library has no query for them, so every setter calls
    the matching method here once its library call has succeeded; nothing else writes them."""

    def __init__(self):
        self.damp_pairs, self.fric_pairs = set(), set()   # the type pairs (i <= j) with gamma_ij != 0 / with friction
        self.spring_pairs = set()                         # ... with k_t,ij != 0 (docs/SPEC.md §2.14)
        self.roll_pairs, self.twist_pairs = set(), set()  # ... with rolling / with twisting resistance (§2.16)
        self.surface = {fam.noun: _SurfaceFlags() for fam in _FAMILIES}
        self.set_walls(np.zeros((0, 3)))

    def of(self, fam):
        """The shadow of a family of _FAMILIES."""
        return self.surface[fam.noun]

    # The names the three families had while each kept a copy of its own: every one is a name of _SurfaceFlags.
    # shstep_set_cylinders resets every gamma_c, mu_c, gamma_t,c, Omega and k_t,c (docs/SPEC.md §2.18, §2.19) and the four
    # coefficients of §2.21; shstep_set_cones the same of the cones (§2.22, §2.23, §2.24).
    set_cylinders, ncyl = _Of("cylinder", "reset"), _Of("cylinder", "n")
    cylinder_damping, cylinder_friction = _Of("cylinder", "damping"), _Of("cylinder", "friction")
    cylinder_spring = _Of("cylinder", "spring")
    cylinder_rolling, cylinder_twisting = _Of("cylinder", "rolling"), _Of("cylinder", "twisting")
    roll_cylinders, twist_cylinders = _Of("cylinder", "roll"), _Of("cylinder", "twist")
    hist_cylinders, diss_cylinders = _Of("cylinder", "hist"), _Of("cylinder", "diss")
    set_cones, ncone = _Of("cone", "reset"), _Of("cone", "n")
    cone_damping, cone_friction = _Of("cone", "damping"), _Of("cone", "friction")
    conic_spring = _Of("cone", "spring")
    conic_rolling, conic_twisting = _Of("cone", "rolling"), _Of("cone", "twisting")
    roll_cones, twist_cones = _Of("cone", "roll"), _Of("cone", "twist")
    hist_cones, diss_cones = _Of("cone", "hist"), _Of("cone", "diss")
    wall_damping, wall_friction = _Of("wall", "damping"), _Of("wall", "friction")
    wall_spring = _Of("wall", "spring")
    wall_rolling, wall_twisting = _Of("wall", "rolling"), _Of("wall", "twisting")
    roll_walls, twist_walls = _Of("wall", "roll"), _Of("wall", "twist")
    damp_walls, fric_walls, hist_walls = _Of("wall", "damp"), _Of("wall", "fric"), _Of("wall", "hist")

    def set_ntypes(self):
        """The pair coefficients go with the type table."""
        self.damp_pairs.clear()
        self.fric_pairs.clear()
        self.spring_pairs.clear()
        self.roll_pairs.clear()
        self.twist_pairs.clear()

    def set_walls(self, normals):
        """shstep_set_walls resets every gamma_w, mu_w, gamma_t,w, k_t,w and u_w and the four coefficients of §2.17, and
        keeps the normals for n_w.u_w."""
        self.normals = np.array(normals, dtype=np.float64).reshape(-1, 3)
        self.move_walls = self.advance_walls = False
        self.surface["wall"].reset(len(self.normals))

    def pair_damping(self, a, b, gamma):
        (self.damp_pairs.add if gamma != 0.0 else self.damp_pairs.discard)((min(a, b), max(a, b)))

    def pair_friction(self, a, b, mu, gamma_t):
        """A pair has friction iff both coefficients are non-zero."""
        (self.fric_pairs.add if mu != 0.0 and gamma_t != 0.0 else self.fric_pairs.discard)((min(a, b), max(a, b)))

    def pair_spring(self, a, b, kt):
        (self.spring_pairs.add if kt != 0.0 else self.spring_pairs.discard)((min(a, b), max(a, b)))

    def pair_rolling(self, a, b, mu_r, gamma_r):
        """A pair has rolling resistance iff both coefficients are non-zero."""
        (self.roll_pairs.add if mu_r != 0.0 and gamma_r != 0.0 else self.roll_pairs.discard)((min(a, b), max(a, b)))

    def pair_twisting(self, a, b, mu_tw, gamma_tw):
        (self.twist_pairs.add if mu_tw != 0.0 and gamma_tw != 0.0 else self.twist_pairs.discard)((min(a, b), max(a, b)))

    def wall_velocity(self, u):
        """As shstep_set_wall_velocity forms them: some u_w != 0, and some n_w.u_w != 0 with the sum in its order."""
        u, n = np.asarray(u, dtype=np.float64).reshape(-1, 3), self.normals
        self.move_walls = bool(np.any(u != 0.0))
        self.advance_walls = bool(np.any(n[:, 0] * u[:, 0] + n[:, 1] * u[:, 1] + n[:, 2] * u[:, 2] != 0.0))


class ShPair:
    """One context = one rank's `pair_style sh` instance on one GPU."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.shpair_create(C.byref(h), device)
        if rc:
            raise ShPairError(rc, "shpair_create")
        self._h = h
        self._reset_shadow()

    def _reset_shadow(self):
        """What this object remembers of a fresh context (needs no library: the CPU tests of the flags start here)."""
        self.nshapes = 0
        self.ntypes = 0
        self._flags = _StepFlags()
        self.ledger_on = False   # shstep_set_energy_ledger: the drivers fold once per step (docs/SPEC.md §2.13)
        self._shell_ledger_on = False   # shstep_set_shell_ledger (docs/SPEC.md §2.20)

    # --- the step's decisions: the library's predicates of the same names, from the flags the setters keep -----------
    @property
    def keeps_integrals(self):
        """shp_keeps_integrals: while damp_on, fric_on or hist_on, or a rolling or twisting pair is set, every compute
        leaves the per-slot integrals for the passes behind it."""
        return self.has_pair_pass or self.has_rolling

    @property
    def has_pair_pass(self):
        """shp_has_pair_pass: damp_on, fric_on or hist_on: the pair pass (pair_dissipation_device / pair_contact_device)
        has a kernel to launch."""
        return bool(self._flags.damp_pairs or self._flags.fric_pairs or self._flags.spring_pairs)

    @property
    def has_rolling(self):
        """shp_has_rolling: some type pair has rolling or twisting resistance: pair_rolling_device follows the pair pass
        (docs/SPEC.md §2.16)."""
        return bool(self._flags.roll_pairs or self._flags.twist_pairs)

    @property
    def has_history(self):
        """hist_on: some k_t,ij != 0: the pair pass is pair_contact_device, and device builds carry xi (docs/SPEC.md §2.14)."""
        return bool(self._flags.spring_pairs)

    @property
    def wall_reads_twists(self):
        """step_wall_reads_twists: a wall coefficient is set: the wall pass reads the twists."""
        return self._flags.of(_WALL).reads_twists

    @property
    def has_wall_rolling(self):
        """step_wall_rolling: some wall has rolling or twisting resistance: the wall pass keeps its rows and launches
        wall_roll_kernel behind the contact kernel (docs/SPEC.md §2.17)."""
        return self._flags.of(_WALL).rolls

    @property
    def has_wall_history(self):
        """step_wall_history: some wall has a tangential spring: the wall pass is wall_contact_device with the step's dt
        (docs/SPEC.md §2.15)."""
        return self._flags.of(_WALL).hist

    @property
    def walls_advance(self):
        """step_walls_advance: a wall has a normal velocity: the loops advance the planes ahead of the wall pass."""
        return self.nwalls > 0 and self._flags.advance_walls

    @property
    def has_dissipation(self):
        """step_has_dissipation: a dissipation coefficient is set, pair, wall, cylinder or cone: the loops compute twists."""
        return self.keeps_integrals or self.wall_reads_twists or self.cylinder_reads_twists or self.cone_reads_twists

    @property
    def cone_reads_twists(self):
        """step_cone_reads_twists: a cone has damping, friction, a tangential spring or rolling or twisting resistance: the
        cone pass is the dissipative instance, or the one with springs, or launches conic_roll_kernel, and reads the twists
        (docs/SPEC.md §2.22, §2.23, §2.24)."""
        return self._flags.of(_CONE).reads_twists

    @property
    def has_conic_rolling(self):
        """step_cone_rolling: some cone has rolling or twisting resistance: the cone pass keeps its rows and launches
        conic_roll_kernel behind the contact kernel (docs/SPEC.md §2.24)."""
        return self._flags.of(_CONE).rolls

    @property
    def has_conic_history(self):
        """step_cone_history: some cone has a tangential spring: the cone pass is conic_contact_device with the step's dt
        (docs/SPEC.md §2.23)."""
        return self._flags.of(_CONE).hist

    ncones = property(lambda self: self._flags.of(_CONE).n, doc="step_has_cones: the cones set (docs/SPEC.md §2.22).")

    @property
    def cylinder_reads_twists(self):
        """step_cyl_reads_twists: a cylinder has damping, friction, a tangential spring or rolling or twisting resistance:
        the cylinder pass is the dissipative instance, or the one with springs, or launches cyl_roll_kernel, and reads the
        twists (docs/SPEC.md §2.18, §2.19, §2.21)."""
        return self._flags.of(_CYLINDER).reads_twists

    @property
    def has_cyl_rolling(self):
        """step_cyl_rolling: some cylinder has rolling or twisting resistance: the cylinder pass keeps its rows and launches
        cyl_roll_kernel behind the contact kernel (docs/SPEC.md §2.21)."""
        return self._flags.of(_CYLINDER).rolls

    @property
    def has_cyl_history(self):
        """step_cyl_history: some cylinder has a tangential spring: the cylinder pass is cyl_contact_device with the step's
        dt (docs/SPEC.md §2.19)."""
        return self._flags.of(_CYLINDER).hist

    ncylinders = property(lambda self: self._flags.of(_CYLINDER).n, doc="step_has_cylinders: the cylinders set (docs/SPEC.md §2.18).")

    # the names the flags had before the predicates
    pair_dissipation = keeps_integrals
    nwalls = property(lambda self: self._flags.of(_WALL).n)
    damp_pairs = property(lambda self: bool(self._flags.damp_pairs), doc="Some gamma_ij != 0 (docs/SPEC.md §2.10).")
    fric_pairs = property(lambda self: bool(self._flags.fric_pairs), doc="Some type pair has friction (docs/SPEC.md §2.11).")
    damp_walls = property(lambda self: self._flags.of(_WALL).damp, doc="Some gamma_w != 0.")
    fric_walls = property(lambda self: self._flags.of(_WALL).fric, doc="Some wall has friction.")
    move_walls = property(lambda self: self._flags.move_walls, doc="Some wall has a velocity, normal or not (§2.12).")

    def _type_pairs(self, itype, jtype):
        """The type pairs (a, b) of `pair_coeff I J`: '*' stands for every type."""
        its = range(1, self.ntypes + 1) if itype == "*" else [int(itype)]
        jts = range(1, self.ntypes + 1) if jtype == "*" else [int(jtype)]
        return [(a, b) for a in its for b in jts]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.shpair_destroy(self._h)
            self._h = None

    __del__ = close

    def _chk(self, rc):
        if rc:
            raise ShPairError(rc, self._lib.shpair_last_error(self._h).decode())

    # --- PairSH::settings / coeff ------------------------------------------------
    def settings(self, nq):
        self._chk(self._lib.shpair_settings(self._h, int(nq)))

    def set_ntypes(self, ntypes, nshapes):
        self._chk(self._lib.shpair_set_ntypes(self._h, int(ntypes), int(nshapes)))
        self.ntypes, self.nshapes = ntypes, nshapes
        self._flags.set_ntypes()

    def set_shape(self, ishape, lmax, anm, rmax=0.0):
        anm, pa = _d(anm)
        if anm.size != (lmax + 1) * (lmax + 2):
            raise ValueError(f"anm has {anm.size} doubles, expected {(lmax + 1) * (lmax + 2)}")
        self._chk(self._lib.shpair_set_shape(self._h, int(ishape), int(lmax), pa, float(rmax)))

    def coeff(self, itype, jtype, kn, exponent):
        """`pair_coeff I J kn exponent`; itype/jtype may be '*' or int; mirrored i<->j."""
        for a, b in self._type_pairs(itype, jtype):
            self._chk(self._lib.shpair_set_coeff(self._h, a, b, float(kn), float(exponent)))
            self._chk(self._lib.shpair_set_coeff(self._h, b, a, float(kn), float(exponent)))

    def rmax(self, ishape):
        r = C.c_double()
        self._chk(self._lib.shpair_get_rmax(self._h, int(ishape), C.byref(r)))
        return r.value

    def init_one(self, ishape, jshape):
        """Cutoff of a shape pair, as PairSH::init_one returns it."""
        return self.rmax(ishape) + self.rmax(jshape)

    # --- neighbour list -----------------------------------------------------------
    def set_neighbors_csr(self, ilist, offsets, jlist):
        ilist, pi = _i(ilist)
        offsets, po = _i(offsets)
        jlist, pj = _i(jlist)
        if offsets.size != ilist.size + 1:
            raise ValueError("offsets must have inum+1 entries")
        self._chk(self._lib.shpair_set_neighbors_csr(self._h, ilist.size, pi, po, pj))

    def set_neighbors(self, ilist, numneigh, firstneigh):
        """LAMMPS layout: numneigh/firstneigh indexed by atom id; firstneigh = list of int32 arrays."""
        ilist, pi = _i(ilist)
        numneigh, pn = _i(numneigh)
        keep = [np.ascontiguousarray(a, dtype=np.int32) for a in firstneigh]
        arr = (_ip * len(keep))(*[a.ctypes.data_as(_ip) for a in keep])
        self._chk(self._lib.shpair_set_neighbors(self._h, ilist.size, pi, pn, arr))

    def set_neighbors_device(self, inum, ilist_ptr, offsets_ptr, jlist_ptr, npairs, max_atom_index, stream=None):
        """CSR half list already on the device (raw device addresses). Asynchronous on `stream`."""
        self._chk(self._lib.shpair_set_neighbors_device(self._h, int(inum), ilist_ptr, offsets_ptr, jlist_ptr,
                                                        int(npairs), int(max_atom_index), stream))

    # --- PairSH::compute ------------------------------------------------------------
    def compute(self, nlocal, x, quat, type_, shtype, newton_pair=True, eflag=False, vflag=False,
                f=None, torque=None):
        """Host-pointer entry point. Returns (f, torque, eng_vdwl, virial[6]); adds into f/torque if given."""
        x, px = _d(x)
        quat, pq = _d(quat)
        type_, pt = _i(type_)
        shtype, ps = _i(shtype)
        nall = x.shape[0]
        if quat.shape != (nall, 4) or type_.size != nall or shtype.size != nall:
            raise ValueError("atom arrays disagree on nall")
        if f is None:
            f = np.zeros((nall, 3))
        if torque is None:
            torque = np.zeros((nall, 3))
        assert f.flags.c_contiguous and torque.flags.c_contiguous and f.dtype == np.float64
        eng = C.c_double(0.0)
        vir = np.zeros(6)
        self._chk(self._lib.shpair_compute(self._h, int(nlocal), int(nall - nlocal), px, pq, pt, ps,
                                           int(newton_pair), int(eflag), int(vflag),
                                           f.ctypes.data_as(_dp), torque.ctypes.data_as(_dp),
                                           C.byref(eng), vir.ctypes.data_as(_dp)))
        return f, torque, eng.value, vir

    def pin_host(self, array):
        """shpair_pin_host: page-locks a numpy array that will be handed to compute() repeatedly (it must outlive the
        pin; unpin_host(array) or close() releases it)."""
        self._chk(self._lib.shpair_pin_host(self._h, C.c_void_p(array.ctypes.data), C.c_size_t(array.nbytes)))

    def unpin_host(self, array):
        self._chk(self._lib.shpair_unpin_host(self._h, C.c_void_p(array.ctypes.data)))

    def compute_device(self, nlocal, nghost, x, quat, type_, shtype, f, torque, newton_pair=True,
                       eflag=False, vflag=False, ev=None, stream=None):
        """Device-pointer entry point: arguments are raw device addresses (ints). Asynchronous.
        stream: a hipStream_t as int; None/0 = HIP null stream."""
        self._chk(self._lib.shpair_compute_device(self._h, int(nlocal), int(nghost), x, quat, type_, shtype,
                                                  int(newton_pair), int(eflag), int(vflag), f, torque,
                                                  ev, stream))

    def set_option(self, key, value):
        self._chk(self._lib.shpair_set_option(self._h, key.encode(), int(value)))

    def set_peratom_output(self, eatom_ptr, vatom_ptr):
        """Device arrays eatom[nall], vatom[nall,6] that following compute_device calls add into (None = off)."""
        self._chk(self._lib.shpair_set_peratom_output(self._h, eatom_ptr, vatom_ptr))

    def set_peratom_host(self, eatom, vatom):
        """Host arrays (float64, C-contiguous; None = off) that following compute() calls add into."""
        for a in (eatom, vatom):
            assert a is None or (a.dtype == np.float64 and a.flags.c_contiguous)
        self._keep_peratom = (eatom, vatom)
        self._chk(self._lib.shpair_set_peratom_host(self._h, None if eatom is None else eatom.ctypes.data_as(_dp),
                                                    None if vatom is None else vatom.ctypes.data_as(_dp)))

    def set_pair_output(self, dev_ptr):
        self._chk(self._lib.shpair_set_pair_output(self._h, dev_ptr))

    def stats(self):
        s = Stats()
        self._chk(self._lib.shpair_get_stats(self._h, C.byref(s)))
        return dict(n_candidates=s.n_candidates, n_contact=s.n_contact, n_touching=s.n_touching,
                    kernel_ms=s.kernel_ms, total_ms=s.total_ms)

    def kernel_info(self):
        """Registers, LDS and resident waves of the pair kernel the last compute launched."""
        k = KernelInfo()
        self._chk(self._lib.shpair_get_kernel_info(self._h, C.byref(k)))
        return {n: getattr(k, n) for n, _ in KernelInfo._fields_}

    def fp64_peak(self, mode=0, target_ms=20.0):
        """Measured FP64 ceilings of this GPU in TFLOP/s: (valu, mfma) of the waves running each loop
        (mode 0 v_fma_f64 chains, 1 v_mfma_f64_16x16x4_f64, 2 both side by side)."""
        a, b = C.c_double(), C.c_double()
        self._chk(self._lib.shpair_fp64_peak(self._h, int(mode), float(target_ms), C.byref(a), C.byref(b)))
        return a.value, b.value

    def own_stream(self):
        """The context's own hipStream_t as an int (None-safe for compute_device(stream=...))."""
        st = C.c_void_p()
        self._chk(self._lib.shpair_get_stream(self._h, C.byref(st)))
        return st.value

    def synchronize(self):
        self._chk(self._lib.shpair_synchronize(self._h))

    # --- include/shstep.h: integrator, body forces, ghosts, neighbour build (device pointers as ints) ----
    def set_density(self, ishape, rho):
        self._chk(self._lib.shstep_set_density(self._h, int(ishape), float(rho)))

    def body(self, ishape):
        """(mass, com[3], inertia[6]) of a shape."""
        m = C.c_double()
        com, inertia = np.zeros(3), np.zeros(6)
        self._chk(self._lib.shstep_get_body(self._h, int(ishape), C.byref(m), com.ctypes.data_as(_dp),
                                            inertia.ctypes.data_as(_dp)))
        return m.value, com, inertia

    def nve_device(self, phase, nlocal, dt, x, v, quat, angmom, f, torque, shtype, mask, groupbit=1, stream=None):
        self._chk(self._lib.shstep_nve_device(self._h, int(phase), int(nlocal), float(dt), x, v, quat, angmom, f, torque,
                                              shtype, mask, int(groupbit), stream))

    def nve(self, phase, dt, x, v, quat, angmom, f, torque, shtype, mask, groupbit=1):
        """Host-pointer form; x, v, quat, angmom are updated in place (float64 C-contiguous)."""
        for a in (x, v, quat, angmom):
            assert a.dtype == np.float64 and a.flags.c_contiguous
        f, pf = _d(f)
        torque, pt = _d(torque)
        shtype, ps = _i(shtype)
        mask, pm = _i(mask)
        self._chk(self._lib.shstep_nve(self._h, int(phase), x.shape[0], float(dt), x.ctypes.data_as(_dp),
                                       v.ctypes.data_as(_dp), quat.ctypes.data_as(_dp), angmom.ctypes.data_as(_dp),
                                       pf, pt, ps, pm, int(groupbit)))

    def force_clear_device(self, nall, f, torque, stream=None):
        """Verlet::force_clear: f and torque of nall atoms zeroed in one launch (raw device addresses)."""
        self._chk(self._lib.shstep_force_clear_device(self._h, int(nall), f, torque, stream))

    def post_force_device(self, nlocal, gravity, gamma_t, gamma_r, v, quat, angmom, shtype, mask, f, torque,
                          groupbit=1, stream=None):
        g, pg = _d(gravity)
        self._chk(self._lib.shstep_post_force_device(self._h, int(nlocal), pg, float(gamma_t), float(gamma_r), v, quat,
                                                     angmom, shtype, mask, int(groupbit), f, torque, stream))

    def energies_device(self, nlocal, gravity, x, v, quat, angmom, shtype, mask, out3, groupbit=1, stream=None):
        g, pg = _d(gravity)
        self._chk(self._lib.shstep_energies_device(self._h, int(nlocal), pg, x, v, quat, angmom, shtype, mask,
                                                   int(groupbit), out3, stream))

    def set_box(self, lo, hi, periodic, skin):
        lo, plo = _d(lo)
        hi, phi = _d(hi)
        per, pp = _i(periodic)
        self._chk(self._lib.shstep_set_box(self._h, plo, phi, pp, float(skin)))

    def borders_device(self, nlocal, nmax, x, quat, type_, shtype, tag=None, stream=None):
        """Returns nghost (blocks)."""
        ng = C.c_int(0)
        self._chk(self._lib.shstep_borders_device(self._h, int(nlocal), int(nmax), x, quat, type_, shtype, tag,
                                                  C.byref(ng), stream))
        return ng.value

    def forward_device(self, x, quat, stream=None):
        self._chk(self._lib.shstep_forward_device(self._h, x, quat, stream))

    def reverse_device(self, f, torque, stream=None):
        self._chk(self._lib.shstep_reverse_device(self._h, f, torque, stream))

    def neighbor_build_device(self, nlocal, nghost, x, shtype, tag=None, stream=None):
        """Builds and installs the half list; returns npairs (blocks)."""
        n = C.c_int(0)
        self._chk(self._lib.shstep_neighbor_build_device(self._h, int(nlocal), int(nghost), x, shtype, tag,
                                                         C.byref(n), stream))
        return n.value

    def neighbor_check_device(self, nlocal, x, stream=None):
        r = C.c_int(0)
        self._chk(self._lib.shstep_neighbor_check_device(self._h, int(nlocal), x, C.byref(r), stream))
        return bool(r.value)

    def copy_neighbors(self, nlocal, npairs):
        offs = np.zeros(nlocal + 1, dtype=np.int32)
        jl = np.zeros(max(npairs, 1), dtype=np.int32)
        self._chk(self._lib.shstep_copy_neighbors(self._h, offs.ctypes.data_as(_ip), jl.ctypes.data_as(_ip)))
        return offs, jl[:npairs]

    # --- the surface families (_FAMILIES): one body per role; the named methods below are the interface -------------------
    def _set_surfaces(self, fam, rows, kn, exponent):
        """The geometry setter of a family: rows [n][fam.width], kn and exponent scalars (broadcast to n) or one entry per
        surface, checked here for all three families; None / empty removes the family.  Returns the rows as the library took
        them, [n][fam.width]; the caller resets the family's shadow with them."""
        if rows is None or len(rows) == 0:
            self._chk(getattr(self._lib, fam.set)(self._h, 0, None, None, None))
            return np.zeros((0, fam.width))
        r, pr = _d(rows)
        if r.size == 0 or r.size % fam.width:
            raise ValueError(f"{fam.rows} must hold {fam.width} doubles per {fam.noun}")
        n = r.size // fam.width
        k, pk = _d(_per_wall(kn, n))
        e, pe = _d(_per_wall(exponent, n))
        if k.size != n or e.size != n:
            raise ValueError(f"kn and exponent must have one entry per {fam.noun}")
        self._chk(getattr(self._lib, fam.set)(self._h, n, pr, pk, pe))
        return r.reshape(n, fam.width)

    def _set_coefficient(self, fam, role, **values):
        """The setter of a family's `role` (a field of its row that is a method of _SurfaceFlags too), of one array or of
        two, named as the message names them.  One rule for every family: a scalar is broadcast, the first to the family's
        current count and the second to the first one's length; an array goes through as it is given; two arrays of
        different lengths are a ValueError ahead of any library call; a single array of the wrong length is the library's
        to refuse.  The shadow follows once the library has accepted."""
        first, *rest = values.values()
        first = np.ascontiguousarray(_per_wall(first, self._flags.of(fam).n))
        arrays = [first] + [np.ascontiguousarray(_per_wall(v, first.size)) for v in rest]
        if any(a.size != first.size for a in arrays):
            raise ValueError(f"{' and '.join(values)} must have one entry per {fam.noun}")
        self._chk(getattr(self._lib, getattr(fam, role))(self._h, int(first.size), *(a.ctypes.data_as(_dp) for a in arrays)))
        getattr(self._flags.of(fam), role)(*arrays)

    def _force_pass(self, fam, nlocal, x, quat, shtype, mask, f, torque, twist, groupbit, out, stream):
        self._chk(getattr(self._lib, fam.force)(self._h, int(nlocal), x, quat, shtype, mask, int(groupbit), f, torque, out, twist,
                                                stream))

    def _contact_pass(self, fam, nlocal, x, quat, shtype, mask, f, torque, twist, dt, groupbit, out, stream):
        self._chk(getattr(self._lib, fam.contact)(self._h, int(nlocal), x, quat, shtype, mask, int(groupbit), f, torque, out,
                                                  twist, float(dt), stream))

    def _history(self, fam, nlocal):
        xi = np.zeros((int(nlocal), self._flags.of(fam).n, fam.xi))
        self._chk(getattr(self._lib, fam.copy_history)(self._h, int(nlocal), xi.ctypes.data_as(_dp)))
        return xi

    def _set_history(self, fam, nlocal, xi):
        xi, px = _d(xi)
        if xi.shape != (int(nlocal), self._flags.of(fam).n, fam.xi):
            raise ValueError(f"xi has shape {xi.shape}, expected {(int(nlocal), self._flags.of(fam).n, fam.xi)}")
        self._chk(getattr(self._lib, fam.set_history)(self._h, int(nlocal), px))

    def _reset_history(self, fam):
        self._chk(getattr(self._lib, fam.reset_history)(self._h))

    def _surface_stats(self, fam):
        n = C.c_int(0)
        self._chk(getattr(self._lib, fam.stats)(self._h, C.byref(n)))
        return n.value

    def _get_surfaces(self, fam):
        rows = np.zeros((self._flags.of(fam).n, fam.width))
        self._chk(getattr(self._lib, fam.get)(self._h, len(rows), rows.ctypes.data_as(_dp)))
        return rows

    # --- planar walls (docs/SPEC.md §2.9; their damping §2.10 and friction §2.11) ------------------
    def set_walls(self, planes=None, kn=None, exponent=None):
        """planes [nw][4] = nx, ny, nz, c (unit normal into the domain, the wall occupies n.p < c); kn, exponent scalars or
        [nw].  None / empty removes all walls."""
        self._flags.set_walls(self._set_surfaces(_WALL, planes, kn, exponent)[:, :3])

    def wall_damping(self, gamma):
        """gamma_w >= 0, a scalar or one per wall; after set_walls(), which resets it to zero."""
        self._set_coefficient(_WALL, "damping", gamma=gamma)

    def wall_friction(self, mu, gamma_t):
        """mu_w, gamma_t,w >= 0, scalars or one per wall; after set_walls(), which resets them to zero."""
        self._set_coefficient(_WALL, "friction", mu=mu, gamma_t=gamma_t)

    def set_wall_tangential_spring(self, kt):
        """k_t,w >= 0, a scalar or one per wall; after set_walls(), which resets it to zero and drops the history.  A wall
        has history iff mu_w and k_t,w are non-zero (docs/SPEC.md §2.15); wall_friction() may come before or after."""
        self._set_coefficient(_WALL, "spring", kt=kt)

    def wall_rolling(self, mu_r, gamma_r):
        """mu_r,w (a length) and gamma_r,w (torque per angular velocity) >= 0, scalars or one per wall; after set_walls(),
        which resets them to zero.  A wall has rolling resistance iff both are non-zero (docs/SPEC.md §2.17)."""
        self._set_coefficient(_WALL, "rolling", mu_r=mu_r, gamma_r=gamma_r)

    def wall_twisting(self, mu_tw, gamma_tw):
        """mu_tw,w (a length) and gamma_tw,w >= 0: twisting resistance at the walls, as wall_rolling()."""
        self._set_coefficient(_WALL, "twisting", mu_tw=mu_tw, gamma_tw=gamma_tw)

    def wall_velocity(self, u):
        """u_w, the translation velocity of the walls (docs/SPEC.md §2.12): one vector for all of them or [nw][3]; after
        set_walls(), which resets it to zero."""
        u, pu = _d(_per_wall(u, self.nwalls, 3))
        if u.ndim != 2 or u.shape[1] != 3:
            raise ValueError("wall velocities must hold 3 doubles per wall")
        self._chk(self._lib.shstep_set_wall_velocity(self._h, int(u.shape[0]), pu))
        self._flags.wall_velocity(u)

    def advance_walls_device(self, dt, stream=None):
        """c_w += dt (n_w.u_w) in the device wall table; nothing is enqueued while no wall has a normal velocity.
        Asynchronous."""
        self._chk(self._lib.shstep_advance_walls_device(self._h, float(dt), stream))

    def get_walls(self):
        """The current planes [nw][4] = nx, ny, nz, c (blocks)."""
        return self._get_surfaces(_WALL)

    def wall_force_device(self, nlocal, x, quat, shtype, mask, f, torque, groupbit=1, wall_out=None, stream=None):
        """ADDS the wall forces / torques to the owned rows (raw device addresses); wall_out: 4 doubles per wall or None.
        Asynchronous."""
        self._chk(self._lib.shstep_wall_force_device(self._h, int(nlocal), x, quat, shtype, mask, int(groupbit), f, torque,
                                                     wall_out, stream))

    def wall_force_damped_device(self, nlocal, x, quat, shtype, mask, f, torque, twist, groupbit=1, wall_out=None, stream=None):
        """wall_force_device with wall damping: twist[nlocal][6] as twist_device() writes it."""
        self._force_pass(_WALL, nlocal, x, quat, shtype, mask, f, torque, twist, groupbit, wall_out, stream)

    def wall_contact_device(self, nlocal, x, quat, shtype, mask, f, torque, twist, dt, groupbit=1, wall_out=None, stream=None):
        """wall_force_damped_device with the tangential springs of the walls: dt > 0 advances xi, dt = 0 only forms the
        forces.  Asynchronous."""
        self._contact_pass(_WALL, nlocal, x, quat, shtype, mask, f, torque, twist, dt, groupbit, wall_out, stream)

    def wall_history(self, nlocal):
        """xi [nlocal][nw][3] of the walls' tangential springs, 0 where nothing is live (docs/SPEC.md §2.15).  Blocks."""
        return self._history(_WALL, nlocal)

    def set_wall_history(self, nlocal, xi):
        """xi [nlocal][nw][3]; a (particle, wall) is live where any component is non-zero.  Blocks."""
        self._set_history(_WALL, nlocal, xi)

    def reset_wall_history(self):
        self._reset_history(_WALL)

    # --- cylindrical container walls (docs/SPEC.md §2.18) ------------------------------------------
    def set_cylinders(self, cylinders=None, kn=None, exponent=None):
        """cylinders [nc][7] = a[3] (a point on the axis), axis[3] (unit), Rc: the particles live INSIDE; kn, exponent
        scalars or [nc].  None / empty removes all cylinders.  Resets the damping, friction, rotation, springs and rolling
        and twisting resistance below."""
        self._flags.set_cylinders(len(self._set_surfaces(_CYLINDER, cylinders, kn, exponent)))

    def cylinder_damping(self, gamma):
        """gamma_c >= 0, a scalar or one per cylinder; after set_cylinders(), which resets it to zero."""
        self._set_coefficient(_CYLINDER, "damping", gamma=gamma)

    def cylinder_friction(self, mu, gamma_t):
        """mu_c, gamma_t,c >= 0, scalars or one per cylinder; a cylinder has friction iff both are non-zero."""
        self._set_coefficient(_CYLINDER, "friction", mu=mu, gamma_t=gamma_t)

    def cylinder_rotation(self, omega):
        """Omega, the angular velocity of each cylinder about its own axis: a scalar or one per cylinder.  It enters the
        friction only; the geometry never moves."""
        self._set_coefficient(_CYLINDER, "rotation", omega=omega)

    def get_cylinders(self):
        """The cylinders as set, [nc][7] (restarts)."""
        return self._get_surfaces(_CYLINDER)

    def cylinder_force_device(self, nlocal, x, quat, shtype, mask, f, torque, twist=None, groupbit=1, cyl_out=None, stream=None):
        """ADDS the cylinder forces / torques to the owned rows (raw device addresses); cyl_out: 5 doubles per cylinder
        (E_c, the force ON the wall, M_ax) or None; twist [nlocal][6], needed while a cylinder has damping, friction or
        rolling or twisting resistance.
        Only enqueues."""
        self._force_pass(_CYLINDER, nlocal, x, quat, shtype, mask, f, torque, twist, groupbit, cyl_out, stream)

    # --- conical container walls (docs/SPEC.md §2.22) ----------------------------------------------
    def set_cones(self, cones=None, kn=None, exponent=None):
        """cones [nk][8] = a[3] (the apex), axis[3] (unit, from the apex into the opening), cos theta, sin theta of the
        half-angle (cone_record() forms a row): the particles live INSIDE; kn, exponent scalars or [nk].  None / empty
        removes all cones.  Resets the damping, friction, rotation, springs and rolling and twisting resistance below."""
        self._flags.set_cones(len(self._set_surfaces(_CONE, cones, kn, exponent)))

    def cone_damping(self, gamma):
        """gamma_k >= 0, a scalar or one per cone; after set_cones(), which resets it to zero."""
        self._set_coefficient(_CONE, "damping", gamma=gamma)

    def cone_friction(self, mu, gamma_t):
        """mu_k, gamma_t,k >= 0, scalars or one per cone; a cone has friction iff both are non-zero."""
        self._set_coefficient(_CONE, "friction", mu=mu, gamma_t=gamma_t)

    def cone_rotation(self, omega):
        """Omega, the angular velocity of each cone about its own axis: a scalar or one per cone.  It enters the friction
        only; the geometry never moves."""
        self._set_coefficient(_CONE, "rotation", omega=omega)

    def get_cones(self):
        """The cones as set, [nk][8] (restarts)."""
        return self._get_surfaces(_CONE)

    def cone_force_device(self, nlocal, x, quat, shtype, mask, f, torque, twist=None, groupbit=1, cone_out=None, stream=None):
        """ADDS the cone forces / torques to the owned rows (raw device addresses); cone_out: 5 doubles per cone (E_k, the
        force ON the wall, M_ax) or None; twist [nlocal][6], needed while a cone has damping, friction or rolling or twisting
        resistance.  Only enqueues."""
        self._force_pass(_CONE, nlocal, x, quat, shtype, mask, f, torque, twist, groupbit, cone_out, stream)

    def cone_stats(self):
        """Particle/cone contacts with V > 0 of the last cone pass (blocks)."""
        return self._surface_stats(_CONE)

    # --- tangential springs with history at the cones (docs/SPEC.md §2.23) -------------------------
    def conic_spring(self, kt):
        """k_t,k >= 0, a scalar or one per cone; after set_cones(), which resets it to zero and drops the history.  A cone has
        history iff mu_k and k_t,k are non-zero; cone_friction() may come before or after."""
        self._set_coefficient(_CONE, "spring", kt=kt)

    # --- rolling and twisting resistance at the cones (docs/SPEC.md §2.24) --------------------------
    def conic_rolling(self, mu_r, gamma_r):
        """mu_r,k (a length) and gamma_r,k >= 0, scalars or one per cone: rolling resistance at the conical walls, on the
        angular velocity in the cone's frame; after set_cones(), which resets them to zero.  A cone has rolling resistance
        iff both are non-zero (docs/SPEC.md §2.24)."""
        self._set_coefficient(_CONE, "rolling", mu_r=mu_r, gamma_r=gamma_r)

    def conic_twisting(self, mu_tw, gamma_tw):
        """mu_tw,k (a length) and gamma_tw,k >= 0: twisting resistance at the conical walls, as conic_rolling()."""
        self._set_coefficient(_CONE, "twisting", mu_tw=mu_tw, gamma_tw=gamma_tw)

    def conic_contact_device(self, nlocal, x, quat, shtype, mask, f, torque, twist, dt, groupbit=1, cone_out=None, stream=None):
        """cone_force_device with the tangential springs of the cones: dt > 0 advances (xi_g, xi_theta, phi_c), dt = 0 only
        forms the forces.  Only enqueues."""
        self._contact_pass(_CONE, nlocal, x, quat, shtype, mask, f, torque, twist, dt, groupbit, cone_out, stream)

    def conic_history(self, nlocal):
        """(xi_g, xi_theta, phi_c) [nlocal][nk][3] of the cones' tangential springs, 0 where nothing is live.  Blocks."""
        return self._history(_CONE, nlocal)

    def set_conic_history(self, nlocal, xi):
        """xi [nlocal][nk][3]; a (particle, cone) is live where one of the three is non-zero.  Blocks."""
        self._set_history(_CONE, nlocal, xi)

    def reset_conic_history(self):
        self._reset_history(_CONE)

    # --- tangential springs with history at the cylinders (docs/SPEC.md §2.19) ---------------------
    def set_cyl_tangential_spring(self, kt):
        """k_t,c >= 0, a scalar or one per cylinder; after set_cylinders(), which resets it to zero and drops the history.
        A cylinder has history iff mu_c and k_t,c are non-zero; cylinder_friction() may come before or after."""
        self._set_coefficient(_CYLINDER, "spring", kt=kt)

    # --- rolling and twisting resistance at the cylinders (docs/SPEC.md §2.21) ----------------------
    def cylinder_rolling(self, mu_r, gamma_r):
        """mu_r,c (a length) and gamma_r,c >= 0, scalars or one per cylinder: rolling resistance at the shells, on the
        angular velocity in the drum's frame; after set_cylinders(), which resets them to zero.  A cylinder has rolling
        resistance iff both are non-zero (docs/SPEC.md §2.21)."""
        self._set_coefficient(_CYLINDER, "rolling", mu_r=mu_r, gamma_r=gamma_r)

    def cylinder_twisting(self, mu_tw, gamma_tw):
        """mu_tw,c (a length) and gamma_tw,c >= 0: twisting resistance at the shells, as cylinder_rolling()."""
        self._set_coefficient(_CYLINDER, "twisting", mu_tw=mu_tw, gamma_tw=gamma_tw)

    def cyl_contact_device(self, nlocal, x, quat, shtype, mask, f, torque, twist, dt, groupbit=1, cyl_out=None, stream=None):
        """cylinder_force_device with the tangential springs of the cylinders: dt > 0 advances (xi_a, xi_theta), dt = 0 only
        forms the forces.  Only enqueues."""
        self._contact_pass(_CYLINDER, nlocal, x, quat, shtype, mask, f, torque, twist, dt, groupbit, cyl_out, stream)

    def cyl_history(self, nlocal):
        """(xi_a, xi_theta) [nlocal][nc][2] of the cylinders' tangential springs, 0 where nothing is live.  Blocks."""
        return self._history(_CYLINDER, nlocal)

    def set_cyl_history(self, nlocal, xi):
        """xi [nlocal][nc][2]; a (particle, cylinder) is live where a component is non-zero.  Blocks."""
        self._set_history(_CYLINDER, nlocal, xi)

    def reset_cyl_history(self):
        self._reset_history(_CYLINDER)

    def cylinder_stats(self):
        """Particle/cylinder contacts with V > 0 of the last cylinder pass (blocks)."""
        return self._surface_stats(_CYLINDER)

    def wall_force(self, x, quat, shtype, mask=None, groupbit=1, f=None, torque=None, wall_out=None):
        """Host-pointer form.  Returns (f, torque, wall_out[nw][4]); adds into the arrays that are given."""
        x, px = _d(x)
        quat, pq = _d(quat)
        shtype, ps = _i(shtype)
        n = x.shape[0]
        mask, pm = _i(np.ones(n, dtype=np.int32) if mask is None else mask)
        f = np.zeros((n, 3)) if f is None else f
        torque = np.zeros((n, 3)) if torque is None else torque
        wall_out = np.zeros((self.nwalls, 4)) if wall_out is None else wall_out
        for a in (f, torque, wall_out):
            assert a.dtype == np.float64 and a.flags.c_contiguous
        self._chk(self._lib.shstep_wall_force(self._h, n, px, pq, ps, pm, int(groupbit), f.ctypes.data_as(_dp),
                                              torque.ctypes.data_as(_dp), wall_out.ctypes.data_as(_dp)))
        return f, torque, wall_out

    def wall_stats(self):
        """Particle/wall contacts with V > 0 of the last wall pass (blocks)."""
        return self._surface_stats(_WALL)

    # --- volume-rate contact damping of pairs (docs/SPEC.md §2.10) ---------------------------------
    def pair_damping(self, itype, jtype, gamma):
        """gamma_ij >= 0 of a type pair (symmetric); itype / jtype may be '*' or int, like coeff()."""
        for a, b in self._type_pairs(itype, jtype):
            self._chk(self._lib.shstep_set_pair_damping(self._h, a, b, float(gamma)))
            self._flags.pair_damping(a, b, float(gamma))

    def twist_device(self, nlocal, nghost, v, quat, angmom, shtype, twist, stream=None):
        """twist[nlocal + nghost][6] = velocity of the SH origin, angular velocity (raw device addresses). Asynchronous."""
        self._chk(self._lib.shstep_twist_device(self._h, int(nlocal), int(nghost), v, quat, angmom, shtype, twist, stream))

    def pair_damping_device(self, nlocal, nghost, x, type_, twist, f, torque, newton_pair=True, stream=None):
        """ADDS the damping wrench of the last compute_device's integrals to f / torque. Asynchronous."""
        self._chk(self._lib.shstep_pair_damping_device(self._h, int(nlocal), int(nghost), x, type_, twist, int(newton_pair),
                                                       f, torque, stream))

    # --- Coulomb-capped friction of pairs (docs/SPEC.md §2.11) -------------------------------------
    def pair_friction(self, itype, jtype, mu, gamma_t):
        """mu_ij, gamma_t,ij >= 0 of a type pair (symmetric); itype / jtype may be '*' or int, like coeff().  The pair has
        friction iff both are non-zero."""
        for a, b in self._type_pairs(itype, jtype):
            self._chk(self._lib.shstep_set_pair_friction(self._h, a, b, float(mu), float(gamma_t)))
            self._flags.pair_friction(a, b, float(mu), float(gamma_t))

    def pair_dissipation_device(self, nlocal, nghost, x, type_, shtype, twist, f, torque, newton_pair=True, stream=None):
        """ADDS the damping and friction wrench of the last compute_device's integrals to f / torque. Asynchronous."""
        self._chk(self._lib.shstep_pair_dissipation_device(self._h, int(nlocal), int(nghost), x, type_, shtype, twist,
                                                           int(newton_pair), f, torque, stream))

    # --- tangential springs with history of pairs (docs/SPEC.md §2.14) --------------------------------
    def set_pair_tangential_spring(self, itype, jtype, kt):
        """k_t,ij >= 0 of a type pair (symmetric); itype / jtype may be '*' or int, like coeff().  The pair has history iff
        mu_ij and k_t,ij are non-zero.  Ahead of the device build of the list it is to act on."""
        for a, b in self._type_pairs(itype, jtype):
            self._chk(self._lib.shstep_set_pair_tangential_spring(self._h, a, b, float(kt)))
            self._flags.pair_spring(a, b, float(kt))

    def pair_contact_device(self, nlocal, nghost, x, type_, shtype, twist, f, torque, dt, newton_pair=True, stream=None):
        """pair_dissipation_device with the tangential springs: dt > 0 advances xi, dt = 0 only forms the forces.
        Asynchronous."""
        self._chk(self._lib.shstep_pair_contact_device(self._h, int(nlocal), int(nghost), x, type_, shtype, twist,
                                                       int(newton_pair), float(dt), f, torque, stream))

    # --- rolling and twisting resistance of pairs (docs/SPEC.md §2.16) --------------------------------
    def pair_rolling(self, itype, jtype, mu_r, gamma_r):
        """mu_r,ij (a length) and gamma_r,ij (torque per angular velocity) >= 0 of a type pair (symmetric); itype / jtype
        may be '*' or int, like coeff().  The pair has rolling resistance iff both are non-zero."""
        for a, b in self._type_pairs(itype, jtype):
            self._chk(self._lib.shstep_set_pair_rolling(self._h, a, b, float(mu_r), float(gamma_r)))
            self._flags.pair_rolling(a, b, float(mu_r), float(gamma_r))

    def pair_twisting(self, itype, jtype, mu_tw, gamma_tw):
        """mu_tw,ij (a length) and gamma_tw,ij >= 0: twisting resistance, as pair_rolling()."""
        for a, b in self._type_pairs(itype, jtype):
            self._chk(self._lib.shstep_set_pair_twisting(self._h, a, b, float(mu_tw), float(gamma_tw)))
            self._flags.pair_twisting(a, b, float(mu_tw), float(gamma_tw))

    def pair_rolling_device(self, nlocal, nghost, x, type_, twist, torque, newton_pair=True, stream=None):
        """ADDS the rolling and twisting couples of the last compute_device's integrals to torque; f is not touched.
        Behind the pair pass, where one runs.  Asynchronous."""
        self._chk(self._lib.shstep_pair_rolling_device(self._h, int(nlocal), int(nghost), x, type_, twist, int(newton_pair),
                                                       torque, stream))

    def _history_slots(self, nlocal):
        """The slot count of the device-built list (the library has no query of its own: the last row offset)."""
        offs = np.zeros(int(nlocal) + 1, dtype=np.int32)
        self._chk(self._lib.shstep_copy_neighbors(self._h, offs.ctypes.data_as(_ip), None))
        return int(offs[-1])

    def contact_history(self, nlocal):
        """xi [npairs][3] of the device-built list of nlocal rows, in the slot order of copy_neighbors().  Blocks."""
        xi = np.zeros((max(self._history_slots(nlocal), 1), 3))
        self._chk(self._lib.shstep_copy_contact_history(self._h, xi.ctypes.data_as(_dp)))
        return xi[:self._history_slots(nlocal)]

    def set_contact_history(self, nlocal, xi):
        """xi [npairs][3], one triple per slot of the device-built list of nlocal rows.  Blocks."""
        xi, px = _d(xi)
        if xi.shape != (self._history_slots(nlocal), 3):
            raise ValueError(f"xi has shape {xi.shape}, the list has {self._history_slots(nlocal)} slots")
        self._chk(self._lib.shstep_set_contact_history(self._h, px))

    def reset_contact_history(self):
        self._chk(self._lib.shstep_reset_contact_history(self._h))

    # --- energy ledger (docs/SPEC.md §2.13) ----------------------------------------------------------
    LEDGER_TERMS = ("pair_damping", "pair_friction", "wall_damping", "wall_friction", "wall_work")

    def set_energy_ledger(self, on=True):
        """Switches the device tally of dissipated energy and wall work on (zeroed if it was off) or off.  Blocks."""
        self._chk(self._lib.shstep_set_energy_ledger(self._h, int(bool(on))))
        self.ledger_on = bool(on)

    def ledger_fold_device(self, dt, stream=None):
        """Adds dt times the powers of the last pair dissipation pass and the last wall pass, each at most once.
        Asynchronous."""
        self._chk(self._lib.shstep_ledger_fold_device(self._h, float(dt), stream))

    def energy_ledger(self):
        """(totals[5] in the order of LEDGER_TERMS, per_wall[nw][3] = damping, friction, work).  Blocks."""
        tot, per = np.zeros(5), np.zeros((self.nwalls, 3))
        self._chk(self._lib.shstep_get_energy_ledger(self._h, tot.ctypes.data_as(_dp), int(self.nwalls),
                                                     per.ctypes.data_as(_dp) if self.nwalls else None))
        return tot, per

    def reset_energy_ledger(self):
        self._chk(self._lib.shstep_reset_energy_ledger(self._h))

    # --- shell ledger: the cylinder entries of the energy ledger (docs/SPEC.md §2.20) ----------------
    SHELL_TERMS = ("damping", "friction", "work")

    def set_shell_ledger(self, on=True):
        """Switches the cylinder entries of the energy ledger on (zeroed if they were off) or off.  While they are on, a
        cylinder coefficient or spring and the energy ledger may be set together.  Blocks."""
        self._chk(self._lib.shstep_set_shell_ledger(self._h, int(bool(on))))
        self._shell_ledger_on = bool(on)

    shell_ledger_on = property(lambda self: self._shell_ledger_on,
                               doc="shstep_set_shell_ledger: the cylinder pass leaves power rows while the energy ledger is on too.")

    def shell_ledger(self):
        """(totals[3] in the order of SHELL_TERMS, per_cylinder[nc][3] = damping, friction, work).  Blocks."""
        tot, per = np.zeros(3), np.zeros((self.ncylinders, 3))
        self._chk(self._lib.shstep_get_shell_ledger(self._h, tot.ctypes.data_as(_dp), int(self.ncylinders),
                                                    per.ctypes.data_as(_dp) if self.ncylinders else None))
        return tot, per

    def run_device(self, arrays, nsteps, nghost, use_graph=False, stream=None):
        """shstep_run_device: the whole loop in the library. Returns (nghost, rebuilds). Blocks."""
        ng = C.c_int(int(nghost))
        nr = C.c_int(0)
        self._chk(self._lib.shstep_run_device(self._h, C.byref(arrays), int(nsteps), int(bool(use_graph)), C.byref(ng),
                                              C.byref(nr), stream))
        return ng.value, nr.value
