"""climate-sim-mpi-cpp_amd — thin ctypes front end of the C ABI in include/csim.h.

The product is the C-ABI shared library (csrc/ -> lib/libcsim.so: hand-written gfx950 HIP
kernels + RCCL halo exchange) and the C++17 headers in include/climate/ that mirror the
reference's own interface.  This module only exists so that tests/, bench.py and
__graft_entry__.py can reach that ABI from Python; names follow the reference
(`Field`, `Decomp2D`, `BCConfig`, `apply_boundary`, `diffusion_step`, `advection_step`,
`exchange_halos`, `safe_dt` — reference include/*.hpp).

There is no CPU fallback: if lib/libcsim.so is missing or no gfx950 device is usable the
calls raise.  (The directory name contains '-', so import it through
``__graft_entry__.load_package()``, which registers it as ``climate_sim_mpi_cpp_amd``.)
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# CSIM_LIB: another build of the engine (A/B measurements of two kernel versions in tools/)
LIB_PATH = os.environ.get("CSIM_LIB") or os.path.join(HERE, "lib", "libcsim.so")
HEADER = os.path.join(ROOT, "include", "csim.h")

DIRICHLET, NEUMANN, PERIODIC = 0, 1, 2
LEFT, RIGHT, BOTTOM, TOP = 0, 1, 2, 3
NO_NEIGHBOR = -1
UNIQUE_ID_BYTES = 128
VARIANTS = {"auto": 0, "dpp": 1, "lds": 2, "naive": 3}

_BC_NAMES = {  # reference src/io.cpp:35-44 bc_from_string aliases
    "dirichlet": DIRICHLET, "fixed": DIRICHLET,
    "neumann": NEUMANN, "noflux": NEUMANN, "zero-flux": NEUMANN,
    "periodic": PERIODIC, "period": PERIODIC,
}


class CsimError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"csim error {code}: {msg}")
        self.code = code


class Decomp(C.Structure):
    """struct csim_decomp == reference Decomp2D without the communicator."""
    _fields_ = [("size", C.c_int), ("rank", C.c_int), ("dims", C.c_int * 2),
                ("coords", C.c_int * 2), ("nbr", C.c_int * 4),
                ("nx_global", C.c_int), ("ny_global", C.c_int),
                ("nx_local", C.c_int), ("ny_local", C.c_int),
                ("x_offset", C.c_int), ("y_offset", C.c_int)]

    def as_dict(self):
        return dict(dims0=self.dims[0], dims1=self.dims[1], cx=self.coords[0], cy=self.coords[1],
                    left=self.nbr[0], right=self.nbr[1], down=self.nbr[2], up=self.nbr[3],
                    nx_local=self.nx_local, ny_local=self.ny_local, x_offset=self.x_offset,
                    y_offset=self.y_offset)


class Msg(C.Structure):
    """struct csim_msg: one message of a halo exchange (peer rank, direction 0..7, doubles)."""
    _fields_ = [("peer", C.c_int), ("dir", C.c_int), ("count", C.c_long)]


VERIFY_MAX_THRESHOLDS = 16


class CsimObsCycle(C.Structure):
    """csim_obs_cycle of include/csim.h: one recorded analysis of an observation network"""
    _fields_ = [(k, C.c_double) for k in ("n", "has_truth", "sum_ob", "sum_ob2", "sum_oa", "sum_oa2", "sum_oa_ob",
                                          "sum_ab_ob", "sum_vb", "sum_va", "sum_r", "sum_eb2", "sum_ea2")]


class CsimObsScreenCycle(C.Structure):
    """csim_obs_screen_cycle of include/csim.h: the used / inactive / rejected counts of one recorded analysis"""
    _fields_ = [(k, C.c_double) for k in ("n_used", "n_inactive", "n_rejected")]


class CsimObsImpactSummary(C.Structure):
    """csim_obs_impact_summary of include/csim.h"""
    _fields_ = [("used", C.c_longlong), ("beneficial", C.c_longlong), ("total", C.c_double)]


class CsimVerifyScores(C.Structure):
    """csim_verify_scores of include/csim.h"""
    _fields_ = [("cells", C.c_longlong), ("nan_cells", C.c_longlong), ("crps", C.c_double), ("rmse", C.c_double),
                ("spread", C.c_double), ("brier", C.c_double * VERIFY_MAX_THRESHOLDS)]


SPATIAL_MAX_HALF, SPATIAL_MAX_SCALES, SPATIAL_MAX_MEMBERS = 32, 8, 4096


class CsimSpatialScores(C.Structure):
    """csim_spatial_scores of include/csim.h"""
    _fields_ = [("cells", C.c_longlong), ("nan_cells", C.c_longlong)] + [
        (k, C.c_double * VERIFY_MAX_THRESHOLDS) for k in ("brier", "reliability", "resolution", "uncertainty",
                                                          "roc_area")] + [
        ("fss", (C.c_double * SPATIAL_MAX_SCALES) * VERIFY_MAX_THRESHOLDS)]


def build(force: bool = False) -> str:
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        args = ["make", "-s", "-C", os.path.join(HERE, "csrc")]
        if force:
            args.append("-B")
        subprocess.run(args, check=True)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """Load lib/libcsim.so and declare every prototype of include/csim.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: run __graft_entry__.build() (there is no CPU fallback)")
    if os.environ.get("CSIM_PRELOAD_TORCH", "1") != "0":
        # torch bundles its own ROCm runtime (libamdhip64.so.7 / librccl.so.1); importing it first
        # makes libcsim.so resolve to that same copy, so a process never holds two HIP runtimes.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    d, i = C.c_double, C.c_int
    u8p = C.POINTER(C.c_ulonglong)
    sig = {
        "csim_last_error": (C.c_char_p, []),
        "csim_abi_version": (i, []),
        "csim_device_count": (i, [ip]),
        "csim_set_device": (i, [i]),
        "csim_device_name": (i, [C.c_char_p, C.c_size_t]),
        "csim_safe_dt": (d, [d] * 5),
        "csim_pow2_velocity_screen": (i, [d] * 6 + [C.POINTER(d)]),
        "csim_screen_lease_bounds": (i, [d] * 6 + [C.c_long, C.POINTER(d)]),
        "csim_decomp_init": (i, [i, i, i, i, C.POINTER(Decomp)]),
        "csim_exchange_plan": (i, [C.POINTER(Decomp), i, C.POINTER(Msg), ip, C.POINTER(Msg), ip]),
        "csim_field_create": (i, [i, i, i, d, d, C.POINTER(vp)]),
        "csim_field_destroy": (i, [vp]),
        "csim_field_upload": (i, [vp, dp]),
        "csim_field_download": (i, [vp, dp]),
        "csim_field_download_interior": (i, [vp, dp]),
        "csim_field_fill": (i, [vp, d]),
        "csim_field_copy": (i, [vp, vp]),
        "csim_field_swap": (i, [vp, vp]),
        "csim_field_minmax": (i, [vp, dp]),
        "csim_field_sum": (i, [vp, dp]),
        "csim_field_linf_diff": (i, [vp, vp, dp]),
        "csim_apply_boundary": (i, [vp, ip, ip, d]),
        "csim_diffusion_step": (i, [vp, vp, d, d]),
        "csim_advection_step": (i, [vp, vp, d, d, d]),
        "csim_fused_step": (i, [vp, vp, d, d, d, d]),
        "csim_stepper_create": (i, [C.POINTER(Decomp), d, d, ip, d, C.POINTER(vp)]),
        "csim_stepper_destroy": (i, [vp]),
        "csim_comm_unique_id": (i, [vp, C.c_size_t]),
        "csim_stepper_comm_init": (i, [vp, vp, C.c_size_t]),
        "csim_stepper_upload": (i, [vp, dp]),
        "csim_stepper_download": (i, [vp, dp]),
        "csim_stepper_download_interior": (i, [vp, dp]),
        "csim_stepper_snapshot_begin": (i, [vp]),
        "csim_stepper_snapshot_wait": (i, [vp, C.POINTER(dp)]),
        "csim_stepper_init_gaussian": (i, [vp, d, d, d, d]),
        "csim_stepper_exchange_halos": (i, [vp]),
        "csim_stepper_halo_pack": (i, [vp, C.POINTER(dp)]),
        "csim_stepper_halo_unpack": (i, [vp, C.POINTER(dp)]),
        "csim_stepper_fuse_limit": (i, [vp, ip]),
        "csim_stepper_faces_neighbors": (i, [vp, i, ip, ip]),
        "csim_stepper_faces_pack": (i, [vp, i, C.POINTER(dp)]),
        "csim_stepper_faces_unpack": (i, [vp, i, C.POINTER(dp)]),
        "csim_stepper_run": (i, [vp, d, d, d, d, i]),
        "csim_stepper_tune": (i, [vp, d, d, d, d]),
        "csim_stepper_keep_warm": (i, [vp, d, d, d, d, d]),
        "csim_pass_schedule": (i, [i, i, C.c_long, i, ip, i, C.POINTER(C.c_long)]),
        "csim_pass_schedule_for": (i, [i, i, C.c_long, i, i, ip, i, C.POINTER(C.c_long)]),
        "csim_stepper_sync": (i, [vp]),
        "csim_stepper_checksum": (i, [vp, C.POINTER(C.c_ulonglong)]),
        "csim_stepper_comm_share": (i, [vp, vp]),
        "csim_stepper_minmax": (i, [vp, dp]),
        "csim_stepper_sum": (i, [vp, dp]),
        "csim_stepper_set_option": (i, [vp, C.c_char_p, C.c_long]),
        "csim_stepper_get_option": (i, [vp, C.c_char_p, C.POINTER(C.c_long)]),
        "csim_stepper_kernel_time": (i, [vp, i, dp, C.POINTER(C.c_long)]),
        "csim_stepper_comm_time": (i, [vp, dp, C.POINTER(C.c_long)]),
        "csim_stepper_reset_timers": (i, [vp]),
        "csim_ensemble_create": (i, [i, i, i, i, d, d, ip, d, C.POINTER(vp)]),
        "csim_ensemble_destroy": (i, [vp]),
        "csim_ensemble_upload": (i, [vp, i, dp]),
        "csim_ensemble_download": (i, [vp, i, dp]),
        "csim_ensemble_upload_all": (i, [vp, dp]),
        "csim_ensemble_download_all": (i, [vp, dp]),
        "csim_ensemble_init_gaussian": (i, [vp, i, d, d, d, d]),
        "csim_ensemble_set_physics": (i, [vp, dp, dp, dp, dp]),
        "csim_ensemble_run": (i, [vp, i]),
        "csim_ensemble_sync": (i, [vp]),
        "csim_ensemble_checksum": (i, [vp, C.POINTER(C.c_ulonglong)]),
        "csim_ensemble_minmax": (i, [vp, dp]),
        "csim_ensemble_sum": (i, [vp, dp]),
        "csim_ensemble_stats": (i, [vp, i, dp, dp, dp, dp]),
        "csim_ensemble_stats_begin": (i, [vp, i]),
        "csim_ensemble_stats_wait": (i, [vp, C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.POINTER(dp)]),
        "csim_ensemble_quantiles": (i, [vp, i, dp, i, dp, dp, dp]),
        "csim_ensemble_quantiles_begin": (i, [vp, i, dp, i, dp]),
        "csim_ensemble_quantiles_wait": (i, [vp, C.POINTER(dp), C.POINTER(dp)]),
        "csim_ensemble_quantile_plan": (i, [i, i, dp, ip, ip, dp]),
        "csim_ensemble_verify": (i, [vp, dp, i, i, i, dp, dp, dp, C.POINTER(C.c_ulonglong),
                                     C.POINTER(CsimVerifyScores)]),
        "csim_ensemble_verify_begin": (i, [vp, dp, i, i, i, dp]),
        "csim_ensemble_verify_wait": (i, [vp, C.POINTER(dp), C.POINTER(dp), C.POINTER(C.POINTER(C.c_ulonglong)),
                                          C.POINTER(CsimVerifyScores)]),
        "csim_ensemble_rank_slot": (i, [C.c_longlong, i, ip]),
        "csim_ensemble_verify_spatial": (i, [vp, dp, i, i, dp, i, ip, u8p, u8p, C.POINTER(C.c_ushort),
                                             C.POINTER(C.c_uint), u8p, u8p]),
        "csim_ensemble_verify_spatial_begin": (i, [vp, dp, i, i, dp, i, ip, i]),
        "csim_ensemble_verify_spatial_wait": (i, [vp, C.POINTER(u8p), C.POINTER(u8p),
                                                  C.POINTER(C.POINTER(C.c_ushort)), C.POINTER(C.POINTER(C.c_uint)),
                                                  u8p, u8p]),
        "csim_verify_spatial_limit": (i, [i, i, i, i]),
        "csim_verify_spatial_finish": (i, [i, i, i, u8p, u8p, C.c_ulonglong, C.c_ulonglong,
                                           C.POINTER(CsimSpatialScores), dp, dp]),
        "csim_ensemble_assimilate": (i, [vp, i, ip, ip, dp, dp, d, d, i, i, dp, dp, dp, dp, ip]),
        "csim_ensemble_gc_table": (i, [d, d, d, i, i, ip, ip, dp]),
        "csim_ensemble_assim_plan": (i, [i, ip, ip, i, i, i, ip, ip]),
        "csim_ensemble_perturb": (i, [vp, C.c_ulonglong, C.c_uint, d, d, i, i]),
        "csim_philox4x32": (i, [C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
        "csim_normal_from_bits": (i, [C.c_ulonglong, dp]),
        "csim_ensemble_perturb_taps": (i, [d, d, i, i, ip, dp]),
        "csim_ensemble_prior_capture": (i, [vp, i, i]),
        "csim_ensemble_relax": (i, [vp, i, d, i, dp]),
        "csim_obs_network_create": (i, [vp, i, ip, ip, dp, d, i, i, C.POINTER(vp)]),
        "csim_obs_network_destroy": (i, [vp]),
        "csim_obs_network_info": (i, [vp, ip, ip, ip, ip]),
        "csim_obs_network_set_values": (i, [vp, dp]),
        "csim_obs_network_observe": (i, [vp, i, C.c_ulonglong, C.c_uint, i]),
        "csim_obs_noise": (i, [C.c_ulonglong, C.c_uint, C.c_uint, dp]),
        "csim_ensemble_assimilate_network": (i, [vp, vp, d, i, i]),
        "csim_obs_network_fetch": (i, [vp, dp, dp, dp, dp, dp, dp]),
        "csim_obs_network_log": (i, [vp, i, C.POINTER(CsimObsCycle), ip]),
        "csim_obs_network_log_reset": (i, [vp]),
        "csim_obs_network_create_linear": (i, [vp, i, ip, ip, ip, ip, ip, dp, dp, d, i, i, C.POINTER(vp)]),
        "csim_obs_network_taps": (i, [vp, ip]),
        "csim_obs_linear_check": (i, [i, i, i, i, i, ip, ip, ip, ip, ip, dp]),
        "csim_obs_taps_bilinear": (i, [i, i, d, d, ip, ip, ip, ip, dp]),
        "csim_obs_taps_box": (i, [i, i, i, i, i, i, ip, ip, ip, dp]),
        "csim_obs_network_set_active": (i, [vp, C.POINTER(C.c_ubyte)]),
        "csim_ensemble_assimilate_screened": (i, [vp, vp, d, i, i, d]),
        "csim_obs_network_screen_log": (i, [vp, i, C.POINTER(CsimObsScreenCycle), ip]),
        "csim_obs_network_status": (i, [vp, C.POINTER(C.c_ubyte)]),
        "csim_obs_screen_decide": (i, [d, d, d, d, d, i, ip]),
        "csim_obs_network_impact_capture": (i, [vp, i]),
        "csim_ensemble_obs_impact": (i, [vp, vp, dp, dp, C.POINTER(CsimObsImpactSummary)]),
        "csim_obs_impact_fold": (i, [dp, C.c_long, dp]),
        "csim_ensemble_obs_impact_global": (i, [vp, vp, dp, dp, C.POINTER(CsimObsImpactSummary)]),
        "csim_obs_impact_global_value": (i, [i, dp, dp, d, dp]),
        "csim_ensemble_assimilate_local": (i, [vp, vp, d, i, i, d]),
        "csim_obs_network_local_info": (i, [vp, ip]),
        "csim_obs_local_count": (i, [i, i, i, ip, ip, i, i, ip, ip]),
        "csim_ensemble_gram": (i, [vp, i, i, dp]),
        "csim_ensemble_gram_plan": (i, [i, i, i, C.POINTER(C.c_long), ip]),
        "csim_ensemble_project": (i, [vp, i, i, i, dp, dp]),
        "csim_ensemble_transform": (i, [vp, i, i, dp, dp]),
        "csim_ensemble_dot": (i, [vp, i, i, i, dp, dp]),
        "csim_sym_eigen": (i, [i, dp, dp, dp, ip]),
        "csim_ensemble_eofs": (i, [vp, i, i, dp, dp, dp, ip]),
        "csim_ensemble_space_check": (i, [i] * 6),
        "csim_ensemble_obs_gram": (i, [vp, vp, i, dp, dp, C.POINTER(C.c_longlong)]),
        "csim_obs_gram_plan": (i, [i, i, C.POINTER(C.c_long), ip]),
        "csim_etkf_weights": (i, [i, dp, d, dp, dp, dp, dp, ip]),
        "csim_ensemble_assimilate_etkf": (i, [vp, vp, d, i, i, d]),
        "csim_ensemble_etkf_info": (i, [vp, C.POINTER(C.c_longlong), dp, dp, dp, ip]),
        "csim_sym_eigen_ordered": (i, [i, dp, i, dp, dp, ip]),
        "csim_sym_eigen_batch_gpu": (i, [i, i, dp, dp, dp, ip, ip, i]),
        "csim_sym_eigen_device_form": (i, [i, i, ip, ip]),
        "csim_etkf_weights_ordered": (i, [i, dp, d, i, dp, dp, dp, dp, ip]),
        "csim_ensemble_assimilate_etkf_device": (i, [vp, vp, d, i, i, d]),
        "csim_ensemble_etkf_info2": (i, [vp, C.POINTER(C.c_longlong), dp, dp, dp, ip, ip, ip]),
        "csim_obs_slots_present": (i, [i, ip, C.POINTER(C.c_ulonglong)]),
        "csim_obs_network_set_slots": (i, [vp, ip]),
        "csim_obs_network_hold": (i, [vp, i, i]),
        "csim_obs_network_observe_slot": (i, [vp, i, i, C.c_ulonglong, C.c_uint, i]),
        "csim_obs_network_held": (i, [vp, dp, ip, ip]),
        "csim_ensemble_obs_gram_held": (i, [vp, vp, dp, dp, C.POINTER(C.c_longlong)]),
        "csim_ensemble_assimilate_etkf_held": (i, [vp, vp, d, i, i, d, i]),
        "csim_ensemble_assimilate_letkf": (i, [vp, vp, d, i, i, d, i]),
        "csim_ensemble_letkf_info": (i, [vp, ip, ip, dp, ip, ip, ip]),
        "csim_letkf_nodes": (i, [i, i, i, ip, ip, ip, ip]),
        "csim_letkf_blend": (i, [i, i, i, i, i, ip, dp]),
        "csim_letkf_plan": (i, [i, i, i, i, C.POINTER(C.c_long), C.POINTER(C.c_longlong)]),
        "csim_ensemble_set_option": (i, [vp, C.c_char_p, C.c_long]),
        "csim_ensemble_get_option": (i, [vp, C.c_char_p, C.POINTER(C.c_long)]),
        "csim_ensemble_plan": (i, [i, i, i, i, ip]),
        "csim_ensemble_sign_class": (i, [d, d, d, d, d, d, i, ip]),
        "csim_ensemble_classes": (i, [i, ip, ip]),
    }
    for name, (res, args) in sig.items():
        if name in ("csim_pow2_velocity_screen", "csim_screen_lease_bounds") and os.environ.get("CSIM_LIB") and not hasattr(L, name):
            continue  # CSIM_LIB: the build of an earlier revision in an A/B measurement (tools/gpu_lib_ab.sh)
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def declared_symbols():
    """Every function name declared in include/csim.h (parsed from the header text)."""
    import re
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(csim_[a-z0-9_]+)\s*\(", txt)))


def _ck(rc):
    if rc != 0:
        raise CsimError(rc, lib().csim_last_error().decode())


def _dp(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i4(v):
    return (C.c_int * 4)(*[int(x) for x in v])


def bc_from_string(s: str) -> int:
    try:
        return _BC_NAMES[s.lower()]
    except KeyError:
        raise RuntimeError("Unknown BC type: " + s)


def bc_codes(code: str):
    """'dnpd' -> [left, right, bottom, top]."""
    m = {"d": DIRICHLET, "n": NEUMANN, "p": PERIODIC}
    return [m[c] for c in code.lower()]


def device_count() -> int:
    n = C.c_int(0)
    _ck(lib().csim_device_count(C.byref(n)))
    return n.value


def set_device(dev: int) -> None:
    _ck(lib().csim_set_device(dev))


def device_name() -> str:
    buf = C.create_string_buffer(256)
    _ck(lib().csim_device_name(buf, 256))
    return buf.value.decode()


def safe_dt(dx, dy, vx, vy, D) -> float:
    return lib().csim_safe_dt(dx, dy, vx, vy, D)


def pow2_velocity_screen(D, dt, vx, vy, dx=1.0, dy=1.0):
    """(L, upper, q, K) of the stepper option "pow2_v" for these parameters, L == 0.0: the form is off (csim.h)"""
    out = (C.c_double * 4)()
    _ck(lib().csim_pow2_velocity_screen(dx, dy, D, dt, vx, vy, out))
    return tuple(out)


def screen_lease_bounds(D, dt, vx, vy, dx=1.0, dy=1.0, R=1024):
    """(M_req, m_req, eta, a0) of the stepper option "screen_lease" for these parameters and a lease of R steps;
    M_req == 0.0: no lease, m_req == 0.0: the 12-operation body is not leased (csim.h)"""
    out = (C.c_double * 4)()
    _ck(lib().csim_screen_lease_bounds(dx, dy, D, dt, vx, vy, int(R), out))
    return tuple(out)


def decomp_init(size, rank, nx_global, ny_global) -> Decomp:
    d = Decomp()
    _ck(lib().csim_decomp_init(size, rank, nx_global, ny_global, C.byref(d)))
    return d


def exchange_plan(dec: Decomp, depth: int):
    """(sends, recvs) of one halo exchange of this rank, each an ordered list of (peer, dir, count)."""
    sends, recvs = (Msg * 8)(), (Msg * 8)()
    ns, nr = C.c_int(0), C.c_int(0)
    _ck(lib().csim_exchange_plan(C.byref(dec), depth, sends, C.byref(ns), recvs, C.byref(nr)))
    return ([(m.peer, m.dir, m.count) for m in sends[:ns.value]],
            [(m.peer, m.dir, m.count) for m in recvs[:nr.value]])


def pass_schedule(nsteps: int, smallest_tile: int = 1 << 30, fuse: int = -1, tile_cells: int = 0, diffusion_only: bool = False):
    """time steps per HBM pass of a run of nsteps (csim_pass_schedule_for), as a list"""
    n = C.c_long(0)
    args = (nsteps, min(smallest_tile, 1 << 30), tile_cells, fuse, int(diffusion_only))
    _ck(lib().csim_pass_schedule_for(*args, None, 0, C.byref(n)))
    buf = (C.c_int * max(1, n.value))()
    _ck(lib().csim_pass_schedule_for(*args, buf, n.value, C.byref(n)))
    return list(buf[:n.value])


class Field:
    """Device mirror of the reference `struct Field` (include/field.hpp:5-21)."""

    def __init__(self, nx, ny, halo=1, dx=1.0, dy=1.0):
        self.nx_local, self.ny_local, self.halo, self.dx, self.dy = nx, ny, halo, dx, dy
        h = C.c_void_p()
        _ck(lib().csim_field_create(nx, ny, halo, dx, dy, C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            lib().csim_field_destroy(self._h)
            self._h = None

    def nx_total(self):
        return self.nx_local + 2 * self.halo

    def ny_total(self):
        return self.ny_local + 2 * self.halo

    def upload(self, host: np.ndarray):
        assert host.shape == (self.ny_total(), self.nx_total())
        _ck(lib().csim_field_upload(self._h, _dp(np.ascontiguousarray(host, dtype=np.float64))))
        return self

    def download(self) -> np.ndarray:
        out = np.empty((self.ny_total(), self.nx_total()))
        _ck(lib().csim_field_download(self._h, _dp(out)))
        return out

    def download_interior(self) -> np.ndarray:
        out = np.empty((self.ny_local, self.nx_local))
        _ck(lib().csim_field_download_interior(self._h, _dp(out)))
        return out

    def fill(self, v):
        _ck(lib().csim_field_fill(self._h, v))

    def copy_from(self, other: "Field"):
        _ck(lib().csim_field_copy(self._h, other._h))

    def swap(self, other: "Field"):
        _ck(lib().csim_field_swap(self._h, other._h))

    def minmax(self):
        o = (C.c_double * 2)()
        _ck(lib().csim_field_minmax(self._h, o))
        return o[0], o[1]

    def sum(self):
        o = C.c_double()
        _ck(lib().csim_field_sum(self._h, C.byref(o)))
        return o.value

    def linf_diff(self, other: "Field"):
        o = C.c_double()
        _ck(lib().csim_field_linf_diff(self._h, other._h, C.byref(o)))
        return o.value


def checksum_host(interior: np.ndarray, x_offset=0, y_offset=0, nx_global=None) -> int:
    """numpy restatement of csim_stepper_checksum for an (ny, nx) interior block (the checker's side)"""
    a = np.ascontiguousarray(interior, dtype=np.float64)
    ny, nx = a.shape
    nxg = nx if nx_global is None else nx_global
    g = (np.arange(ny, dtype=np.uint64)[:, None] + np.uint64(y_offset)) * np.uint64(nxg) + \
        (np.arange(nx, dtype=np.uint64)[None, :] + np.uint64(x_offset))
    with np.errstate(over="ignore"):
        w = np.uint64(0x9E3779B97F4A7C15) + np.uint64(2) * g
        return int((a.view(np.uint64) * w).sum(dtype=np.uint64))


def apply_boundary(f: Field, bc, is_physical=(1, 1, 1, 1), value=0.0):
    _ck(lib().csim_apply_boundary(f._h, _i4(bc), _i4(is_physical), value))


def diffusion_step(u: Field, out: Field, D, dt):
    _ck(lib().csim_diffusion_step(u._h, out._h, D, dt))


def advection_step(u: Field, out: Field, vx, vy, dt):
    _ck(lib().csim_advection_step(u._h, out._h, vx, vy, dt))


def fused_step(u: Field, out: Field, D, dt, vx, vy):
    _ck(lib().csim_fused_step(u._h, out._h, D, dt, vx, vy))


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    _ck(lib().csim_comm_unique_id(buf, UNIQUE_ID_BYTES))
    return buf.raw


class Stepper:
    """The time loop of reference src/main.cpp:93-118 (minus I/O) on one GPU / one rank."""

    def __init__(self, dec: Decomp, dx=1.0, dy=1.0, bc=(0, 0, 0, 0), bc_value=0.0):
        self.dec = dec
        self.nx, self.ny = dec.nx_local, dec.ny_local
        h = C.c_void_p()
        _ck(lib().csim_stepper_create(C.byref(dec), dx, dy, _i4(bc), bc_value, C.byref(h)))
        self._h = h

    @classmethod
    def single(cls, nx, ny, dx=1.0, dy=1.0, bc=(0, 0, 0, 0), bc_value=0.0):
        return cls(decomp_init(1, 0, nx, ny), dx, dy, bc, bc_value)

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_h", None):
            lib().csim_stepper_destroy(self._h)
            self._h = None

    def comm_init(self, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        _ck(lib().csim_stepper_comm_init(self._h, buf, UNIQUE_ID_BYTES))

    def comm_share(self, owner: "Stepper"):
        """borrow another stepper's RCCL communicator (same rank; the owner must outlive this one)"""
        _ck(lib().csim_stepper_comm_share(self._h, owner._h))

    def checksum(self) -> int:
        """position-weighted 64-bit checksum of the local interior (csim_stepper_checksum)"""
        v = C.c_ulonglong(0)
        _ck(lib().csim_stepper_checksum(self._h, C.byref(v)))
        return v.value

    def upload(self, host: np.ndarray):
        assert host.shape == (self.ny + 2, self.nx + 2)
        _ck(lib().csim_stepper_upload(self._h, _dp(np.ascontiguousarray(host, dtype=np.float64))))

    def download(self) -> np.ndarray:
        out = np.empty((self.ny + 2, self.nx + 2))
        _ck(lib().csim_stepper_download(self._h, _dp(out)))
        return out

    def download_interior(self) -> np.ndarray:
        out = np.empty((self.ny, self.nx))
        _ck(lib().csim_stepper_download_interior(self._h, _dp(out)))
        return out

    def fuse_limit(self) -> int:
        d = C.c_int(0)
        _ck(lib().csim_stepper_fuse_limit(self._h, C.byref(d)))
        return d.value

    def faces_neighbors(self, depth):
        peers, lens = (C.c_int * 8)(), (C.c_int * 8)()
        _ck(lib().csim_stepper_faces_neighbors(self._h, depth, peers, lens))
        return list(peers), list(lens)

    def faces_pack(self, depth):
        """faces of the current field of the given depth per direction (None where no peer)."""
        peers, lens = self.faces_neighbors(depth)
        bufs = [np.empty(lens[d]) if peers[d] >= 0 else None for d in range(8)]
        arr = (C.POINTER(C.c_double) * 8)(*[_dp(b) if b is not None else None for b in bufs])
        _ck(lib().csim_stepper_faces_pack(self._h, depth, arr))
        return bufs

    def faces_unpack(self, depth, faces):
        keep = [np.ascontiguousarray(b, dtype=np.float64) if b is not None else None for b in faces]
        arr = (C.POINTER(C.c_double) * 8)(*[_dp(b) if b is not None else None for b in keep])
        _ck(lib().csim_stepper_faces_unpack(self._h, depth, arr))

    def snapshot_begin(self):
        _ck(lib().csim_stepper_snapshot_begin(self._h))

    def snapshot_wait(self) -> np.ndarray:
        """copy of the interior captured by the last snapshot_begin()"""
        ptr = C.POINTER(C.c_double)()
        _ck(lib().csim_stepper_snapshot_wait(self._h, C.byref(ptr)))
        return np.ctypeslib.as_array(ptr, shape=(self.ny, self.nx)).copy()

    def init_gaussian(self, A=1.0, sigma_frac=0.05, xc_frac=0.5, yc_frac=0.5):
        _ck(lib().csim_stepper_init_gaussian(self._h, A, sigma_frac, xc_frac, yc_frac))

    def exchange_halos(self):
        _ck(lib().csim_stepper_exchange_halos(self._h))

    def _side_len(self, k):
        return self.ny if k < 2 else self.nx

    def halo_pack(self):
        """edge lines of the current field per side (None on physical sides)."""
        bufs = [np.empty(self._side_len(k)) if self.dec.nbr[k] >= 0 else None for k in range(4)]
        arr = (C.POINTER(C.c_double) * 4)(*[_dp(b) if b is not None else None for b in bufs])
        _ck(lib().csim_stepper_halo_pack(self._h, arr))
        return bufs

    def halo_unpack(self, lines):
        """stage the neighbours' edge lines (list of 4, None on physical sides)."""
        keep = [np.ascontiguousarray(b, dtype=np.float64) if b is not None else None for b in lines]
        for k, b in enumerate(keep):
            assert b is None or b.shape == (self._side_len(k),)
        arr = (C.POINTER(C.c_double) * 4)(*[_dp(b) if b is not None else None for b in keep])
        _ck(lib().csim_stepper_halo_unpack(self._h, arr))

    def run(self, D, dt, vx, vy, nsteps):
        _ck(lib().csim_stepper_run(self._h, D, dt, vx, vy, nsteps))

    def sync(self):
        _ck(lib().csim_stepper_sync(self._h))

    def minmax(self):
        o = (C.c_double * 2)()
        _ck(lib().csim_stepper_minmax(self._h, o))
        return o[0], o[1]

    def sum(self):
        o = C.c_double()
        _ck(lib().csim_stepper_sum(self._h, C.byref(o)))
        return o.value

    def set_option(self, key: str, value: int):
        """the options of include/csim.h, e.g. "fuse", "pow2_v", "screen_lease", "wide_strips" (0 off, 1 wherever a wide
        strip fits, 2 = default: on tiles where it was measured to pay)"""
        _ck(lib().csim_stepper_set_option(self._h, key.encode(), int(value)))

    def tune(self, D, dt, vx, vy):
        _ck(lib().csim_stepper_tune(self._h, D, dt, vx, vy))

    def keep_warm(self, D, dt, vx, vy, seconds):
        """load without effect on the field for about `seconds` (see csim_stepper_keep_warm)"""
        _ck(lib().csim_stepper_keep_warm(self._h, D, dt, vx, vy, float(seconds)))

    def get_option(self, key: str) -> int:
        v = C.c_long()
        _ck(lib().csim_stepper_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def kernel_time(self, steps_per_launch=None):
        """(total ms, launches) of the timed sweep launches of one kind (1 or 2 steps per launch);
        with None: (total ms, launches, time steps covered) over both kinds."""
        def one(t):
            ms, n = C.c_double(), C.c_long()
            _ck(lib().csim_stepper_kernel_time(self._h, t, C.byref(ms), C.byref(n)))
            return ms.value, n.value
        if steps_per_launch is not None:
            return one(steps_per_launch)
        parts = [(t,) + one(t) for t in (1, 2, 3, 4, 5, 6, 7)]
        return (sum(p[1] for p in parts), sum(p[2] for p in parts), sum(p[0] * p[2] for p in parts))

    def comm_time(self):
        """(total ms, passes) of the sampled comm-stream chains (pack + RCCL exchange + unpack + ghost fill)"""
        ms, n = C.c_double(), C.c_long()
        _ck(lib().csim_stepper_comm_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def reset_timers(self):
        _ck(lib().csim_stepper_reset_timers(self._h))


def ensemble_plan(nsteps: int, nx: int, ny: int, fuse: int = -1):
    """(steps per fused pass, fused passes, single steps) of Ensemble.run(nsteps) — host arithmetic, no GPU"""
    o = (C.c_int * 3)()
    _ck(lib().csim_ensemble_plan(nsteps, nx, ny, fuse, o))
    return o[0], o[1], o[2]


def ensemble_sign_class(D, dt, vx, vy, dx=1.0, dy=1.0, fused_2c=1) -> int:
    """the per-pass launch (upwind-sign class 0..8) a member with these parameters runs in — host only"""
    c = C.c_int()
    _ck(lib().csim_ensemble_sign_class(dx, dy, D, dt, vx, vy, fused_2c, C.byref(c)))
    return c.value


def ensemble_launches(classes) -> int:
    """launches per pass of a batch whose members have these sign classes — host only"""
    a = (C.c_int * len(classes))(*[int(c) for c in classes])
    n = C.c_int()
    _ck(lib().csim_ensemble_classes(len(classes), a, C.byref(n)))
    return n.value


def ensemble_quantile_plan(members: int, q):
    """numpy's "linear" (lo, hi, gamma) of each level q for this many members, as lists — host only"""
    qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
    n = len(qs)
    lo, hi, g = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))(), np.empty(max(n, 1))
    _ck(lib().csim_ensemble_quantile_plan(int(members), n, _dp(qs), lo, hi, _dp(g)))
    return list(lo[:n]), list(hi[:n]), [float(v) for v in g[:n]]


EnsembleStats = collections.namedtuple("EnsembleStats", "mean var min max")
EnsembleStats.__doc__ = """per-cell statistics over an ensemble's members, (ny+2, nx+2) each, ghost ring included"""


EnsembleQuantiles = collections.namedtuple("EnsembleQuantiles", "q exceed")
EnsembleQuantiles.__doc__ = """per-cell quantiles (nq, ny+2, nx+2) and exceedance probabilities (nt, ny+2, nx+2) over an
ensemble's members, ghost ring included"""


EnsembleVerification = collections.namedtuple("EnsembleVerification", "crps brier rank_hist scores")
EnsembleVerification.__doc__ = """verification of an ensemble against a truth: per-cell CRPS (ny+2, nx+2) and Brier scores
(nt, ny+2, nx+2), ghost ring included, the interior's rank histogram (M+1,) uint64, and VerifyScores"""

VerifyScores = collections.namedtuple("VerifyScores", "cells nan_cells crps rmse spread brier")
VerifyScores.__doc__ = """domain scores over the non-NaN interior cells: their count, the NaN interior cells, mean CRPS,
RMSE of the ensemble mean, spread (root mean variance) and the mean Brier score per threshold (nt,)"""


def ensemble_rank_slot(g: int, ties: int) -> int:
    """the rank histogram's tie-break: splitmix64(g) mod (ties + 1) — host only"""
    v = C.c_int()
    _ck(lib().csim_ensemble_rank_slot(int(g), int(ties), C.byref(v)))
    return v.value


SpatialScores = collections.namedtuple(
    "SpatialScores", "cells nan_cells brier reliability resolution uncertainty roc_area fss hit_rate false_alarm")
SpatialScores.__doc__ = """scores finished from the integer tables of a spatial verification (csim_verify_spatial_finish):
per threshold (nt,) the Brier score and its reliability, resolution and uncertainty, the ROC area, fss (nt, ns), and
the ROC points hit_rate / false_alarm (nt, M+1) of the decisions "at least k members exceed", k = 0 .. M"""

SpatialVerification = collections.namedtuple("SpatialVerification", "table nbh cells nan_cells scores counts flags")
SpatialVerification.__doc__ = """Ensemble.verify_spatial: table (nt, M+1, 2) and nbh (nt, ns, 3) uint64, the non-NaN and NaN
interior cells, SpatialScores, and with counts=True the count planes (nt, ny, nx) uint16 and flags (ny, nx) uint32"""


def _u8p(a):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_ulonglong))


def verify_spatial_limit(M: int, nx: int, ny: int, half_max: int) -> bool:
    """whether M forecast members on nx x ny cells with half-widths up to half_max stay inside the overflow bound
    M^2 w^4 nx ny <= 2^62, M <= 4096 (csim_verify_spatial_limit) — host only"""
    rc = lib().csim_verify_spatial_limit(int(M), int(nx), int(ny), int(half_max))
    if rc not in (0, 5):  # CSIM_ERR_UNSUPPORTED: outside the bound
        _ck(rc)
    return rc == 0


def verify_spatial_finish(M: int, table, nbh, cells: int, nan_cells: int = 0) -> SpatialScores:
    """the scores of the integer tables: table (nt, M+1, 2), nbh (nt, ns, 3) (csim_verify_spatial_finish) — host only"""
    table = np.ascontiguousarray(table, dtype=np.uint64)
    nt = table.shape[0]
    if table.shape != (nt, int(M) + 1, 2):
        raise ValueError("table must have shape (nt, M + 1, 2)")
    nbh = np.ascontiguousarray(nbh, dtype=np.uint64).reshape(nt, -1, 3)
    ns = nbh.shape[1]
    sc = CsimSpatialScores()
    hit, fa = np.empty((nt, int(M) + 1)), np.empty((nt, int(M) + 1))
    _ck(lib().csim_verify_spatial_finish(int(M), nt, ns, _u8p(table), _u8p(nbh) if ns else None, int(cells),
                                         int(nan_cells), C.byref(sc), _dp(hit), _dp(fa)))
    per = [np.array(getattr(sc, k)[:nt], dtype=np.float64)
           for k in ("brier", "reliability", "resolution", "uncertainty", "roc_area")]
    fss = np.array([[sc.fss[q][s] for s in range(ns)] for q in range(nt)], dtype=np.float64).reshape(nt, ns)
    return SpatialScores(sc.cells, sc.nan_cells, *per, fss, hit, fa)


EnsembleAnalysis = collections.namedtuple("EnsembleAnalysis", "nlevels prior_mean prior_var post_mean post_var")
EnsembleAnalysis.__doc__ = """an analysis (Ensemble.assimilate): the plan's level count and, per observation in input
order, the forecast mean and variance at its cell when its turn came and the analysis mean and variance there after
all observations"""


def _ints(v, n=None):
    """int32 copy of integral values (integer dtype, or floats with no fraction) within the int32 range"""
    v = np.atleast_1d(np.asarray(v))
    if v.ndim != 1:
        raise ValueError("expected a one-dimensional sequence of indices")
    if v.size and not np.issubdtype(v.dtype, np.integer):
        if not np.issubdtype(v.dtype, np.floating) or not np.all(np.isfinite(v)) or np.any(v != np.trunc(v)):
            raise ValueError("indices must be integral")
    if v.size and (v.min() < np.iinfo(np.int32).min or v.max() > np.iinfo(np.int32).max):
        raise ValueError("indices out of the int32 range")
    a = np.ascontiguousarray(v, dtype=np.int32)
    if n is not None and a.shape != (n,):
        raise ValueError(f"expected {n} values")
    return a


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def ensemble_gc_table(dx, dy, loc, nx, ny) -> np.ndarray:
    """the Gaspari-Cohn localisation table of csim_ensemble_gc_table, shape (2 ly + 1, 2 lx + 1) — host only"""
    lx, ly = C.c_int(), C.c_int()
    _ck(lib().csim_ensemble_gc_table(float(dx), float(dy), float(loc), int(nx), int(ny), C.byref(lx), C.byref(ly),
                                     None))
    t = np.empty((2 * ly.value + 1, 2 * lx.value + 1))
    _ck(lib().csim_ensemble_gc_table(float(dx), float(dy), float(loc), int(nx), int(ny), C.byref(lx), C.byref(ly),
                                     _dp(t)))
    return t


def ensemble_assim_plan(i, j, lx, ly, ordered=False) -> np.ndarray:
    """the level of each observation (int32) in csim_ensemble_assimilate's plan — host only"""
    ii = _ints(i)
    jj = _ints(j, len(ii))
    lev, nl = np.zeros(len(ii), dtype=np.int32), C.c_int()
    _ck(lib().csim_ensemble_assim_plan(len(ii), _ip(ii), _ip(jj), int(lx), int(ly), int(bool(ordered)), _ip(lev),
                                       C.byref(nl)))
    return lev


PERTURB_MAX_RADIUS = 32


def philox4x32(ctr, key):
    """Philox4x32-10 of a counter (4 x uint32) under a key (2 x uint32): 4 x uint32 (csim_philox4x32) — host only"""
    c, k, o = (C.c_uint * 4)(*[int(v) for v in ctr]), (C.c_uint * 2)(*[int(v) for v in key]), (C.c_uint * 4)()
    _ck(lib().csim_philox4x32(c, k, o))
    return np.array(o[:], dtype=np.uint32)


def _per_element(values, call):
    """call(v, z) for every element v of an array, z a double the library writes: the doubles as an array of the same
    shape, a float for a scalar"""
    out = np.empty(values.shape)
    z = C.c_double()
    flat = out.reshape(-1)
    for n, v in enumerate(values.reshape(-1).tolist()):
        _ck(call(v, C.byref(z)))
        flat[n] = z.value
    return out if out.ndim else float(out)


def normal_from_bits(bits):
    """the normal deviate csim_ensemble_perturb makes of 64 random bits (csim_normal_from_bits); a scalar or an array
    of uint64 — host only"""
    return _per_element(np.asarray(bits, dtype=np.uint64), lib().csim_normal_from_bits)


def ensemble_perturb_taps(d, corr_len, n, periodic=False) -> np.ndarray:
    """the 2 R + 1 smoothing taps of csim_ensemble_perturb along an axis of n cells of spacing d — host only"""
    R = C.c_int()
    _ck(lib().csim_ensemble_perturb_taps(float(d), float(corr_len), int(n), int(bool(periodic)), C.byref(R), None))
    t = np.empty(2 * R.value + 1)
    _ck(lib().csim_ensemble_perturb_taps(float(d), float(corr_len), int(n), int(bool(periodic)), C.byref(R), _dp(t)))
    return t


RELAX_SPREAD, RELAX_PERT = 1, 2  # CSIM_RELAX_SPREAD (RTPS), CSIM_RELAX_PERT (RTPP)
_RELAX_MODES = {"spread": RELAX_SPREAD, "rtps": RELAX_SPREAD, "pert": RELAX_PERT, "rtpp": RELAX_PERT}


def _relax_mode(mode) -> int:
    """"spread" / "rtps", "pert" / "rtpp", or the integer code as it is (the library checks it)"""
    if isinstance(mode, str):
        if mode.lower() not in _RELAX_MODES:
            raise ValueError(f"unknown relaxation mode {mode!r}")
        return _RELAX_MODES[mode.lower()]
    return int(mode)


def obs_noise(seed, draw, o):
    """the deviate z_o that ObsNetwork.observe adds (times sqrt(r_o)) to observation o under (seed, draw); o a scalar or
    an array of input indices (csim_obs_noise) — host only"""
    seed, draw = int(seed), int(draw)
    if not (0 <= seed < 1 << 64 and 0 <= draw < 1 << 32):
        raise ValueError("seed must fit 64 bits and draw 32 bits, unsigned")
    fn = lib().csim_obs_noise
    return _per_element(np.asarray(o, dtype=np.uint32), lambda v, z: fn(seed, draw, v, z))


OBS_MAX_TAPS = 64  # CSIM_OBS_MAX_TAPS
OBS_MAX_SLOTS = 64  # CSIM_OBS_MAX_SLOTS
ObsTaps = collections.namedtuple("ObsTaps", "start di dj w")
ObsTaps.__doc__ = """the taps of linear observations (csim_obs_network_create_linear): observation o observes
sum_s w[s] x(i[o] + di[s], j[o] + dj[s]) over s = start[o] .. start[o + 1] - 1"""


def _taps(taps, n):
    """(start, di, dj, w) as contiguous arrays of the C types; start has n + 1 values, the others start[n] each"""
    start, di, dj, w = taps
    start = _ints(start, n + 1)
    di, dj = _ints(di), _ints(dj)
    w = np.ascontiguousarray(np.atleast_1d(np.asarray(w, dtype=np.float64)))
    # the library checks start itself, before it reads a tap; where start is in order the arrays must be as long as
    # it says
    in_order = start[0] == 0 and np.all(np.diff(start) >= 0)
    if not (len(di) == len(dj) == len(w)) or (in_order and len(w) != start[-1]):
        raise ValueError("taps: di, dj and w need start[-1] values each")
    return ObsTaps(start, di, dj, w)


def obs_linear_check(nx, ny, lx, ly, i, j, taps):
    """raises CsimError unless (i, j, taps) are valid linear observations on an nx x ny grid with localisation
    half-widths lx, ly (csim_obs_linear_check) — host only"""
    ii = _ints(i)
    jj = _ints(j, len(ii))
    t = _taps(taps, len(ii))
    _ck(lib().csim_obs_linear_check(int(nx), int(ny), int(lx), int(ly), len(ii), _ip(ii), _ip(jj), _ip(t.start),
                                    _ip(t.di), _ip(t.dj), _dp(t.w)))


def bilinear_taps(nx, ny, x, y):
    """(i, j, ObsTaps) of bilinear interpolation to the positions (x, y), arrays in cell-index units, 1 <= x <= nx,
    1 <= y <= ny: four taps per observation (csim_obs_taps_bilinear) — host only"""
    xx = np.atleast_1d(np.asarray(x, dtype=np.float64))
    yy = np.atleast_1d(np.asarray(y, dtype=np.float64))
    if xx.shape != yy.shape or xx.ndim != 1:
        raise ValueError("x and y must be arrays of one length")
    n = len(xx)
    i, j = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    di, dj, w = np.empty(4 * n, dtype=np.int32), np.empty(4 * n, dtype=np.int32), np.empty(4 * n)
    ci, cj, cdi, cdj, cw = C.c_int(), C.c_int(), (C.c_int * 4)(), (C.c_int * 4)(), (C.c_double * 4)()
    fn = lib().csim_obs_taps_bilinear
    for o in range(n):
        _ck(fn(int(nx), int(ny), float(xx[o]), float(yy[o]), C.byref(ci), C.byref(cj), cdi, cdj, cw))
        i[o], j[o] = ci.value, cj.value
        di[4 * o:4 * o + 4], dj[4 * o:4 * o + 4], w[4 * o:4 * o + 4] = cdi[:], cdj[:], cw[:]
    return i, j, ObsTaps(np.arange(0, 4 * n + 1, 4, dtype=np.int32), di, dj, w)


def box_taps(nx, ny, i, j, a, b):
    """(i, j, ObsTaps) of the means over the (2a+1) x (2b+1) boxes around the interior cells (i, j), clipped to the
    interior, at most 64 taps each (csim_obs_taps_box) — host only"""
    ii = _ints(i)
    jj = _ints(j, len(ii))
    start, di, dj, w = [0], [], [], []
    cn = C.c_int()
    cdi, cdj, cw = (C.c_int * OBS_MAX_TAPS)(), (C.c_int * OBS_MAX_TAPS)(), (C.c_double * OBS_MAX_TAPS)()
    fn = lib().csim_obs_taps_box
    for o in range(len(ii)):
        _ck(fn(int(nx), int(ny), int(ii[o]), int(jj[o]), int(a), int(b), C.byref(cn), cdi, cdj, cw))
        k = cn.value
        di += cdi[:k]
        dj += cdj[:k]
        w += cw[:k]
        start.append(len(w))
    return ii, jj, ObsTaps(np.array(start, dtype=np.int32), np.array(di, dtype=np.int32), np.array(dj, dtype=np.int32),
                           np.array(w, dtype=np.float64))


ObsNetworkInfo = collections.namedtuple("ObsNetworkInfo", "nobs nlevels lx ly")
ObsValues = collections.namedtuple("ObsValues", "y truth bg_mean bg_var post_mean post_var")
ObsValues.__doc__ = """what ObsNetwork.fetch() returns, each per observation in input order or None where the network
does not hold it: the values, the source member's own values (after observe), and the forecast members' mean and
variance at the cell before and after the last recorded analysis"""
OBS_CYCLE_FIELDS = tuple(k for k, _ in CsimObsCycle._fields_)
OBS_SCREEN_FIELDS = tuple(k for k, _ in CsimObsScreenCycle._fields_)
OBS_USED, OBS_INACTIVE, OBS_REJECTED = 0, 1, 2


def obs_slots_present(slot, nobs=None) -> int:
    """the mask of the time slots that occur among the observations' slots (None: every observation in slot 0): bit s
    for slot s; what a network holds against the slots held or observed (csim_obs_slots_present) — host only"""
    m = C.c_ulonglong()
    if slot is None:
        _ck(lib().csim_obs_slots_present(1 if nobs is None else int(nobs), None, C.byref(m)))
    else:
        ss = _ints(slot, nobs)
        _ck(lib().csim_obs_slots_present(len(ss), _ip(ss), C.byref(m)))
    return m.value


def obs_screen_decide(y, hb, vb, r, tol, active=True) -> int:
    """the status (OBS_USED / OBS_INACTIVE / OBS_REJECTED) that a screened analysis gives one observation with value y,
    background mean hb and variance vb, error variance r, under tolerance tol and its mask byte
    (csim_obs_screen_decide) — host only"""
    st = C.c_int()
    _ck(lib().csim_obs_screen_decide(float(y), float(hb), float(vb), float(r), float(tol),
                                     active if isinstance(active, int) else int(bool(active)), C.byref(st)))
    return st.value


IMPACT_MAX_DOUBLES = 1 << 27  # CSIM_IMPACT_MAX_DOUBLES
ObsImpactSummary = collections.namedtuple("ObsImpactSummary", "used beneficial total")
ObsImpactSummary.__doc__ = """of Ensemble.obs_impact(): the observations the captured analysis used, how many of them
have a negative impact (they reduced the forecast error), and the sum of the impacts"""
ObsImpact = collections.namedtuple("ObsImpact", "impact summary")
ObsImpact.__doc__ = """what Ensemble.obs_impact() returns: J_o per observation in input order, and an ObsImpactSummary"""


def obs_impact_fold(u) -> float:
    """the lane-and-butterfly sum that Ensemble.obs_impact() makes of a window's terms (csim_obs_impact_fold) — host
    only"""
    uu = np.ascontiguousarray(np.atleast_1d(np.asarray(u, dtype=np.float64)))
    if uu.ndim != 1:
        raise ValueError("expected a one-dimensional sequence of terms")
    out = C.c_double()
    _ck(lib().csim_obs_impact_fold(_dp(uu), len(uu), C.byref(out)))
    return out.value


def obs_impact_global_value(a, g, dn) -> float:
    """J_o of Ensemble.obs_impact_global() for one observation from its captured perturbations a, the M values g and
    dn: c = sum a_k g_k from +0 in member order, J = dn (c / (M-1)) (csim_obs_impact_global_value) — host only, no
    device needed"""
    aa, gg = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(g, dtype=np.float64).ravel()
    if aa.shape != gg.shape:
        raise ValueError("a and g must have the same length")
    out = C.c_double()
    _ck(lib().csim_obs_impact_global_value(len(aa), _dp(aa), _dp(gg), float(dn), C.byref(out)))
    return out.value


def impact_weight(mean_a, mean_b, truth) -> np.ndarray:
    """the weight C (e_a + e_b) of Ensemble.obs_impact() for the mean squared error of the interior: from the mean
    forecasts from the analysis and from the background and the truth at verification time, (ny+2, nx+2) each,
    ((mean_a - truth) + (mean_b - truth)) / (nx ny) on the interior and 0 on the ghost ring — numpy only"""
    a, b, t = (np.asarray(v, dtype=np.float64) for v in (mean_a, mean_b, truth))
    if a.ndim != 2 or a.shape != b.shape or a.shape != t.shape or min(a.shape) < 3:
        raise ValueError("mean_a, mean_b and truth must be fields of one shape (ny+2, nx+2)")
    w = np.zeros(a.shape)
    n = float((a.shape[0] - 2) * (a.shape[1] - 2))
    w[1:-1, 1:-1] = ((a[1:-1, 1:-1] - t[1:-1, 1:-1]) + (b[1:-1, 1:-1] - t[1:-1, 1:-1])) / n
    return w


LOCAL_MAX_OBS, LOCAL_MAX_DOUBLES, LOCAL_MAX_PRIOR_DOUBLES = 64, 4096, 1 << 26  # CSIM_LOCAL_MAX_*


def obs_local_count(nx, ny, i, j, lx, ly):
    """(count, max_local): per interior cell, (ny, nx), the observations at the cells (i, j) whose window rectangle of
    half-widths lx, ly, clipped to the interior, contains it, and the largest of them: the bound that
    Ensemble.assimilate_local() holds against LOCAL_MAX_OBS (csim_obs_local_count) — host only"""
    ii = _ints(i)
    jj = _ints(j, len(ii))
    count = np.zeros((int(ny), int(nx)), dtype=np.int32)
    most = C.c_int()
    _ck(lib().csim_obs_local_count(int(nx), int(ny), len(ii), _ip(ii), _ip(jj), int(lx), int(ly),
                                   count.ctypes.data_as(C.POINTER(C.c_int)), C.byref(most)))
    return count, most.value


ESPACE_MAX_MEMBERS, SYM_EIGEN_MAX_N, SYM_EIGEN_MAX_SWEEPS = 256, 256, 64  # CSIM_ESPACE_MAX_MEMBERS, CSIM_SYM_EIGEN_*
DOT_MAX_FIELDS = 16  # CSIM_DOT_MAX_FIELDS

SymEigen = collections.namedtuple("SymEigen", "lambda_ V sweeps")
SymEigen.__doc__ = """eigenvalues (descending), eigenvectors (column r belongs to lambda_[r]) and the sweeps made"""
EnsembleEOFs = collections.namedtuple("EnsembleEOFs", "lambda_ variance pcs patterns n_valid")
EnsembleEOFs.__doc__ = """leading modes of an ensemble's spread: eigenvalues of the Gram matrix, variance = lambda_ /
(M - 1), principal components (M, n_modes), patterns (n_modes, ny+2, nx+2) or None, and the number of modes that are
not null"""


EIGEN_ORDERS = {"rows": 0, "round_robin": 1}  # CSIM_EIGEN_ROWS, CSIM_EIGEN_ROUND_ROBIN
EIGEN_OK, EIGEN_NONFINITE, EIGEN_NOT_CONVERGED = 0, 1, 2  # CSIM_EIGEN_*
SYM_EIGEN_MAX_BATCH = 65535  # CSIM_SYM_EIGEN_MAX_BATCH
SymEigenBatch = collections.namedtuple("SymEigenBatch", "lambda_ V sweeps status")
SymEigenBatch.__doc__ = """what sym_eigen_batch() returns: per matrix the eigenvalues (batch, n), the eigenvectors
(batch, n, n), the sweeps made and the status EIGEN_OK, EIGEN_NONFINITE (NaN results) or EIGEN_NOT_CONVERGED"""


def _eigen_order(order) -> int:
    return EIGEN_ORDERS[order] if isinstance(order, str) and order in EIGEN_ORDERS else int(order)


def sym_eigen(A, order="rows") -> SymEigen:
    """eigenvalues and eigenvectors of a symmetric matrix by the cyclic Jacobi method, bit for bit the same for every
    caller; order "rows" takes the pairs of a sweep by rows, "round_robin" in steps of disjoint pairs, the order of
    sym_eigen_batch() (csim_sym_eigen_ordered) — host only"""
    a = np.ascontiguousarray(A, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("A must be a square matrix")
    n = a.shape[0]
    lam, V, sweeps = np.empty(n), np.empty((n, n)), C.c_int()
    _ck(lib().csim_sym_eigen_ordered(n, _dp(a), _eigen_order(order), _dp(lam), _dp(V), C.byref(sweeps)))
    return SymEigen(lam, V, sweeps.value)


def sym_eigen_batch(A, form=0) -> SymEigenBatch:
    """the symmetric matrices A[b] (batch, n, n) on the GPU, one workgroup per matrix, bit for bit
    sym_eigen(A[b], order="round_robin"); form forces a storage form of sym_eigen_device_form()
    (csim_sym_eigen_batch_gpu)"""
    a = np.ascontiguousarray(A, dtype=np.float64)
    if a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise ValueError("A must have shape (batch, n, n)")
    batch, n = a.shape[0], a.shape[1]
    lam, V = np.empty((batch, n)), np.empty((batch, n, n))
    sweeps, status = np.zeros(batch, dtype=np.int32), np.zeros(batch, dtype=np.int32)
    _ck(lib().csim_sym_eigen_batch_gpu(n, batch, _dp(a), _dp(lam), _dp(V), sweeps.ctypes.data_as(C.POINTER(C.c_int)),
                                       status.ctypes.data_as(C.POINTER(C.c_int)), int(form)))
    return SymEigenBatch(lam, V, sweeps, status)


def sym_eigen_device_form(n: int, form: int = 0):
    """(chosen, max_n): the storage form sym_eigen_batch() takes for n (1: both working matrices in LDS, 2: the matrix
    in LDS and the vectors in global memory, 3: both in global memory) and the largest n that `form` admits
    (csim_sym_eigen_device_form) — host only"""
    chosen, most = C.c_int(), C.c_int()
    _ck(lib().csim_sym_eigen_device_form(int(n), int(form), C.byref(chosen), C.byref(most)))
    return chosen.value, most.value


def ensemble_gram_plan(M: int, nx: int, ny: int):
    """(nseg, Gc): the 64-cell segments of the interior and the classes whose partial sums Ensemble.gram() adds in
    order (csim_ensemble_gram_plan) — host only"""
    nseg, gc = C.c_long(), C.c_int()
    _ck(lib().csim_ensemble_gram_plan(int(M), int(nx), int(ny), C.byref(nseg), C.byref(gc)))
    return nseg.value, gc.value


ObsGram = collections.namedtuple("ObsGram", "A loglik n_used")
ObsGram.__doc__ = """what Ensemble.obs_gram() returns: A (M+1, M+1) = Z^T Z of the normalised observation-space
perturbations with the normalised innovation as column M (A[:M, :M] = Y^T R^-1 Y, A[:M, M] = Y^T R^-1 (y - hb), A[M, M]
the innovation chi^2), loglik (M,) or None, and the number of observations used"""
EtkfWeights = collections.namedtuple("EtkfWeights", "W wbar gamma dfs sweeps")
EtkfWeights.__doc__ = """what etkf_weights() returns: Ensemble.transform(W, wbar) is the ETKF analysis; gamma are the
eigenvalues of Y^T R^-1 Y clamped at 0, dfs the degrees of freedom for signal, sweeps those of sym_eigen"""
EtkfAnalysis = collections.namedtuple("EtkfAnalysis", "n_used chi2 gamma dfs")
EtkfAnalysis.__doc__ = """what Ensemble.assimilate_etkf() returns: the observations used, the innovation chi^2, and gamma
and dfs of its weights"""
EtkfInfo = collections.namedtuple("EtkfInfo", "n_used chi2 gamma dfs sweeps status")
EtkfInfo.__doc__ = """what Ensemble.etkf_info() returns: EtkfAnalysis' fields, and after assimilate_etkf(device=True) the
device eigensolver's sweeps and status (EIGEN_OK or EIGEN_NOT_CONVERGED)"""


def obs_gram_plan(M: int, nobs: int):
    """(nseg, Gc): the 64-observation segments of a network's plan order and the classes whose partial sums
    Ensemble.obs_gram() adds in order (csim_obs_gram_plan) — host only"""
    nseg, gc = C.c_long(), C.c_int()
    _ck(lib().csim_obs_gram_plan(int(M), int(nobs), C.byref(nseg), C.byref(gc)))
    return nseg.value, gc.value


def etkf_weights(A, inflation=1.0, order="rows") -> EtkfWeights:
    """the symmetric square-root ETKF in ensemble space from the (M+1, M+1) matrix of Ensemble.obs_gram(), inflation
    taken in ensemble space, on sym_eigen(order=order) (csim_etkf_weights_ordered) — host only"""
    a = np.ascontiguousarray(A, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError("A must be a square matrix, (M+1, M+1)")
    M = a.shape[0] - 1
    W, wbar, gamma = np.empty((M, M)), np.empty(M), np.empty(M)
    dfs, sweeps = C.c_double(), C.c_int()
    _ck(lib().csim_etkf_weights_ordered(M, _dp(a), float(inflation), _eigen_order(order), _dp(W), _dp(wbar),
                                        _dp(gamma), C.byref(dfs), C.byref(sweeps)))
    return EtkfWeights(W, wbar, gamma, dfs.value, sweeps.value)


LETKF_MAX_NODES, LETKF_MAX_BYTES = 65535, 1 << 30  # CSIM_LETKF_MAX_NODES, CSIM_LETKF_MAX_BYTES
LETKF_OK, LETKF_IDLE, LETKF_NONFINITE, LETKF_NOT_CONVERGED = 0, 1, 2, 3  # CSIM_LETKF_*
LetkfNodes = collections.namedtuple("LetkfNodes", "nax nay xi yj")
LetkfNodes.__doc__ = """the lattice of analysis nodes of Ensemble.assimilate_letkf(): nay x nax nodes, node (a, b) at the
interior cell (xi[a], yj[b]) with index b * nax + a"""
LetkfBlend = collections.namedtuple("LetkfBlend", "node beta")
LetkfBlend.__doc__ = """the four nodes of a cell, (a, b), (a+1, b), (a, b+1), (a+1, b+1) by index, and their weights"""
LetkfPlan = collections.namedtuple("LetkfPlan", "nodes bytes")
LetkfInfo = collections.namedtuple("LetkfInfo", "dfs count sweeps status")
LetkfInfo.__doc__ = """what Ensemble.letkf_info() returns, each (nay, nax): per node the degrees of freedom for signal, the
local observations used, the eigensolver's sweeps and the status LETKF_OK, LETKF_IDLE (no local observation),
LETKF_NONFINITE or LETKF_NOT_CONVERGED"""


def letkf_nodes(nx: int, ny: int, spacing: int) -> LetkfNodes:
    """the analysis nodes of an nx x ny grid with this spacing: the first cell of an axis, every spacing-th after it
    and the last (csim_letkf_nodes) — host only"""
    nax, nay = C.c_int(), C.c_int()
    _ck(lib().csim_letkf_nodes(int(nx), int(ny), int(spacing), C.byref(nax), C.byref(nay), None, None))
    xi, yj = np.zeros(nax.value, dtype=np.int32), np.zeros(nay.value, dtype=np.int32)
    _ck(lib().csim_letkf_nodes(int(nx), int(ny), int(spacing), None, None, _ip(xi), _ip(yj)))
    return LetkfNodes(nax.value, nay.value, xi, yj)


def letkf_blend(nx: int, ny: int, spacing: int, i: int, j: int) -> LetkfBlend:
    """the four nodes between which the interior cell (i, j) lies and the bilinear weights with which
    Ensemble.assimilate_letkf() blends their analyses there (csim_letkf_blend) — host only"""
    node, beta = np.zeros(4, dtype=np.int32), np.zeros(4)
    _ck(lib().csim_letkf_blend(int(nx), int(ny), int(spacing), int(i), int(j), _ip(node), _dp(beta)))
    return LetkfBlend(node, beta)


def letkf_plan(M: int, nx: int, ny: int, spacing: int) -> LetkfPlan:
    """(nodes, bytes): the analysis nodes of a call of Ensemble.assimilate_letkf() with M forecast members and the
    device storage they take, held against LETKF_MAX_NODES and LETKF_MAX_BYTES (csim_letkf_plan) — host only"""
    nodes, nbytes = C.c_long(), C.c_longlong()
    _ck(lib().csim_letkf_plan(int(M), int(nx), int(ny), int(spacing), C.byref(nodes), C.byref(nbytes)))
    return LetkfPlan(nodes.value, nbytes.value)


class ObsNetwork:
    """observations that live on the device (csim_obs_network_*): planned once, their values drawn on the GPU
    from a member or set from the host, read by Ensemble.assimilate_network without staging.  Point observations of
    the cells (i, j), or with taps = (start, di, dj, w) linear observations anchored there
    (csim_obs_network_create_linear).  Made by Ensemble.obs_network(); closing the ensemble closes its networks."""

    def __init__(self, ens, i, j, r, loc, ordered=False, log_cycles=0, taps=None):
        ii = _ints(i)
        n = len(ii)
        jj = _ints(j, n)
        rr = np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.float64), (n,)))
        h = C.c_void_p()
        if taps is None:
            _ck(lib().csim_obs_network_create(ens._h, n, _ip(ii), _ip(jj), _dp(rr), float(loc), int(bool(ordered)),
                                              int(log_cycles), C.byref(h)))
        else:
            t = _taps(taps, n)
            _ck(lib().csim_obs_network_create_linear(ens._h, n, _ip(ii), _ip(jj), _ip(t.start), _ip(t.di), _ip(t.dj),
                                                     _dp(t.w), _dp(rr), float(loc), int(bool(ordered)),
                                                     int(log_cycles), C.byref(h)))
        self._h, self._ens, self.nobs = h, ens, n
        ens._nets.add(self)

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_h", None):
            # A closed ensemble has destroyed its networks.  It clears their handles, but only of those its weak set
            # still holds: when the collector frees a network together with its ensemble (both kept by a failed
            # test's traceback, say) it clears the weak references before it runs either __del__
            if getattr(self._ens, "_h", None):
                lib().csim_obs_network_destroy(self._h)
            self._h = None
            self._ens._nets.discard(self)

    @property
    def info(self) -> ObsNetworkInfo:
        v = [C.c_int() for _ in range(4)]
        _ck(lib().csim_obs_network_info(self._h, *[C.byref(x) for x in v]))
        return ObsNetworkInfo(*[x.value for x in v])

    @property
    def ntaps(self) -> int:
        """taps of all observations of a linear network, 0 for point observations (csim_obs_network_taps)"""
        v = C.c_int()
        _ck(lib().csim_obs_network_taps(self._h, C.byref(v)))
        return v.value

    def local_info(self) -> int:
        """max_local: the most window rectangles of the network over one cell, which Ensemble.assimilate_local() holds
        against LOCAL_MAX_OBS and, times the forecast members, LOCAL_MAX_DOUBLES (csim_obs_network_local_info)"""
        v = C.c_int()
        _ck(lib().csim_obs_network_local_info(self._h, C.byref(v)))
        return v.value

    def set_values(self, y):
        """the values, one per observation in input order; copied before the call returns, enqueued without waiting"""
        yy = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if yy.shape != (self.nobs,):
            raise ValueError(f"expected {self.nobs} values")
        _ck(lib().csim_obs_network_set_values(self._h, _dp(yy)))

    def set_active(self, mask=None):
        """which observations the analyses use from now on: one 0 / 1 per observation in input order, None: all;
        copied before the call returns, enqueued without waiting, kept until replaced (csim_obs_network_set_active)"""
        if mask is None:
            _ck(lib().csim_obs_network_set_active(self._h, None))
            return
        m = np.asarray(mask)
        if m.shape != (self.nobs,):
            raise ValueError(f"expected {self.nobs} mask bytes")
        m = np.ascontiguousarray(m.astype(np.uint8) if m.dtype == np.bool_ else m, dtype=np.uint8)
        _ck(lib().csim_obs_network_set_active(self._h, m.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def set_reports(self, y):
        """this cycle's reports, NaN (or any non-finite value) where a station did not report: the mask becomes
        isfinite(y) and the values y with 0.0 in place of the missing ones (set_active, then set_values)"""
        yy = np.asarray(y, dtype=np.float64)
        if yy.shape != (self.nobs,):
            raise ValueError(f"expected {self.nobs} values")
        ok = np.isfinite(yy)
        self.set_active(ok)
        self.set_values(np.where(ok, yy, 0.0))

    def status(self) -> np.ndarray:
        """waits for the ensemble's stream; OBS_USED / OBS_INACTIVE / OBS_REJECTED per observation in input order for
        the last analysis of this network (csim_obs_network_status)"""
        out = np.empty(self.nobs, dtype=np.uint8)
        _ck(lib().csim_obs_network_status(self._h, out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out

    def _log(self, fn, record, fields) -> np.ndarray:
        """the records of one of the two logs as a structured array: their number first, then that many"""
        k = C.c_int()
        _ck(fn(self._h, 0, None, C.byref(k)))
        rec = (record * max(k.value, 1))()
        _ck(fn(self._h, k.value, rec, C.byref(k)))
        out = np.zeros(k.value, dtype=[(f, np.float64) for f in fields])
        for c in range(k.value):
            out[c] = tuple(getattr(rec[c], f) for f in fields)
        return out

    def screen_log(self) -> np.ndarray:
        """waits for the ensemble's stream; n_used, n_inactive and n_rejected of the recorded analyses, oldest first,
        as a structured array parallel to log() (csim_obs_network_screen_log)"""
        return self._log(lib().csim_obs_network_screen_log, CsimObsScreenCycle, OBS_SCREEN_FIELDS)

    def set_slots(self, slot=None):
        """the time slot of every observation, 0 .. OBS_MAX_SLOTS - 1 in input order (None: all 0, as at first); forgets
        which slots are held and observed; enqueued without waiting (csim_obs_network_set_slots)"""
        if slot is None:
            _ck(lib().csim_obs_network_set_slots(self._h, None))
            return
        ss = _ints(slot, self.nobs)
        _ck(lib().csim_obs_network_set_slots(self._h, _ip(ss)))

    def hold(self, slot=None, truth_member=None):
        """keeps h_k of every forecast member for the observations of the slot (None: all), from the members as they
        are now, in rows of the network's own that stay across run(): what Ensemble.assimilate_etkf(held=True) reads at
        the end of the window; enqueued without waiting (csim_obs_network_hold)"""
        _ck(lib().csim_obs_network_hold(self._h, -1 if slot is None else int(slot),
                                        -1 if truth_member is None else int(truth_member)))

    def held(self) -> np.ndarray:
        """waits for the ensemble's stream; the held rows, (nobs, M) in input order: the forecast in observation space
        at the observations' own times, after a held analysis the analysis there (csim_obs_network_held)"""
        M = C.c_int()
        _ck(lib().csim_obs_network_held(self._h, None, C.byref(M), None))
        H = np.empty((self.nobs, M.value))
        _ck(lib().csim_obs_network_held(self._h, _dp(H), None, None))
        return H

    def observe(self, source_member, seed, draw=0, noise=True, slot=None):
        """the values from member source_member at the observed cells, with noise plus sqrt(r) times the seeded
        deviates obs_noise(seed, draw, o); enqueued without waiting (csim_obs_network_observe).  slot: only the
        observations of that time slot, the others keep their values (csim_obs_network_observe_slot)"""
        seed, draw = int(seed), int(draw)
        if not (0 <= seed < 1 << 64 and 0 <= draw < 1 << 32):
            raise ValueError("seed must fit 64 bits and draw 32 bits, unsigned")
        if slot is not None:
            _ck(lib().csim_obs_network_observe_slot(self._h, int(slot), int(source_member), seed, draw,
                                                    noise if isinstance(noise, int) else int(bool(noise))))
            return
        _ck(lib().csim_obs_network_observe(self._h, int(source_member), seed, draw,
                                           noise if isinstance(noise, int) else int(bool(noise))))

    def fetch(self) -> ObsValues:
        """waits for the ensemble's stream; whatever the network holds of ObsValues (csim_obs_network_fetch)"""
        fn, n = lib().csim_obs_network_fetch, self.nobs
        got = []
        for group in ((0,), (1,), (2, 3, 4, 5)):
            outs = [np.empty(n) for _ in group]
            args = [None] * 6
            for k, a in zip(group, outs):
                args[k] = _dp(a)
            rc = fn(self._h, *args)
            if rc == 4:  # CSIM_ERR_STATE: not held
                outs = [None for _ in group]
            else:
                _ck(rc)
            got += outs
        return ObsValues(*got)

    def log(self) -> np.ndarray:
        """waits for the ensemble's stream; the recorded analyses, oldest first, as a structured array with the fields
        of csim_obs_cycle (csim_obs_network_log)"""
        return self._log(lib().csim_obs_network_log, CsimObsCycle, OBS_CYCLE_FIELDS)

    def log_reset(self):
        _ck(lib().csim_obs_network_log_reset(self._h))

    def impact_capture(self, truth_member=None):
        """keeps what Ensemble.obs_impact() needs of the last analysis, which must be a recorded one: the analysis
        perturbations of the current members in observation space, the normalised innovations and which observations
        were used.  Call it on the ensemble the forecast starts from (after relax / perturb if they are part of the
        cycle); it stays valid across run() until the next capture; enqueued without waiting
        (csim_obs_network_impact_capture)"""
        _ck(lib().csim_obs_network_impact_capture(self._h, -1 if truth_member is None else int(truth_member)))


def _scores(sc: CsimVerifyScores, nt: int) -> VerifyScores:
    return VerifyScores(sc.cells, sc.nan_cells, sc.crps, sc.rmse, sc.spread, np.array(sc.brier[:nt], dtype=np.float64))


def _levels(v):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.float64)))


class Ensemble:
    """B members of one grid shape (own field, own D, dt, vx, vy each) stepped together on one GPU; every member
    ends bit-identical to a single-rank Stepper run with its own parameters (csim_ensemble_*)."""

    def __init__(self, members, nx, ny, dx=1.0, dy=1.0, bc=(0, 0, 0, 0), bc_value=0.0):
        self.members, self.nx, self.ny = members, nx, ny
        self._q_counts = (0, 0)  # levels and thresholds of the last quantiles_begin()
        self._v_counts = (0, 0)  # forecast members and thresholds of the last verify_begin()
        self._s_counts = (0, 0, 0, False)  # members, thresholds, scales, fields of the last verify_spatial_begin()
        # observation networks that are alive (the library destroys them with the ensemble); weak, so that a network,
        # which keeps its ensemble alive, makes no reference cycle with it
        self._nets = weakref.WeakSet()
        h = C.c_void_p()
        _ck(lib().csim_ensemble_create(members, nx, ny, 1, dx, dy, _i4(bc), bc_value, C.byref(h)))
        self._h = h

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_h", None):
            for net in list(self._nets):
                net._h = None
            self._nets.clear()
            lib().csim_ensemble_destroy(self._h)
            self._h = None

    def upload(self, k: int, host: np.ndarray):
        assert host.shape == (self.ny + 2, self.nx + 2)
        _ck(lib().csim_ensemble_upload(self._h, k, _dp(np.ascontiguousarray(host, dtype=np.float64))))

    def upload_all(self, host: np.ndarray):
        assert host.shape == (self.members, self.ny + 2, self.nx + 2)
        _ck(lib().csim_ensemble_upload_all(self._h, _dp(np.ascontiguousarray(host, dtype=np.float64))))

    def download(self, k: int) -> np.ndarray:
        out = np.empty((self.ny + 2, self.nx + 2))
        _ck(lib().csim_ensemble_download(self._h, k, _dp(out)))
        return out

    def download_all(self) -> np.ndarray:
        out = np.empty((self.members, self.ny + 2, self.nx + 2))
        _ck(lib().csim_ensemble_download_all(self._h, _dp(out)))
        return out

    def init_gaussian(self, k, A=1.0, sigma_frac=0.05, xc_frac=0.5, yc_frac=0.5):
        _ck(lib().csim_ensemble_init_gaussian(self._h, k, A, sigma_frac, xc_frac, yc_frac))

    def set_physics(self, D, dt, vx, vy):
        """scalars apply to every member, sequences give one value per member"""
        arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.members,)))
                for v in (D, dt, vx, vy)]
        _ck(lib().csim_ensemble_set_physics(self._h, *[_dp(a) for a in arrs]))

    def run(self, nsteps: int):
        _ck(lib().csim_ensemble_run(self._h, nsteps))

    def sync(self):
        _ck(lib().csim_ensemble_sync(self._h))

    def checksums(self):
        o = (C.c_ulonglong * self.members)()
        _ck(lib().csim_ensemble_checksum(self._h, o))
        return [int(v) for v in o]

    def minmax(self) -> np.ndarray:
        """(members, 2) array: min, max of each member, ghosts included"""
        o = np.empty((self.members, 2))
        _ck(lib().csim_ensemble_minmax(self._h, _dp(o)))
        return o

    def sums(self) -> np.ndarray:
        o = np.empty(self.members)
        _ck(lib().csim_ensemble_sum(self._h, _dp(o)))
        return o

    def stats(self, ddof=1) -> EnsembleStats:
        """per-cell mean, variance (divided by members - ddof), min and max over the members: numpy's mean, var,
        fmin.reduce and fmax.reduce over the member axis, bit for bit (csim_ensemble_stats)"""
        out = EnsembleStats(*[np.empty((self.ny + 2, self.nx + 2)) for _ in range(4)])
        _ck(lib().csim_ensemble_stats(self._h, int(ddof), *[_dp(a) for a in out]))
        return out

    def stats_begin(self, ddof=1):
        """start stats() of the current state without waiting; run() may follow before stats_wait()"""
        _ck(lib().csim_ensemble_stats_begin(self._h, int(ddof)))

    def stats_wait(self) -> EnsembleStats:
        """the statistics stats_begin() captured (copies)"""
        ptrs = [C.POINTER(C.c_double)() for _ in range(4)]
        _ck(lib().csim_ensemble_stats_wait(self._h, *[C.byref(p) for p in ptrs]))
        shape = (self.ny + 2, self.nx + 2)
        return EnsembleStats(*[np.ctypeslib.as_array(p, shape=shape).copy() for p in ptrs])

    def quantiles(self, q, thresholds=()) -> EnsembleQuantiles:
        """per-cell np.quantile(members, q, axis=0) (method "linear"; NaN where a member is NaN) and
        np.mean(members > t, axis=0) for each threshold t (csim_ensemble_quantiles)"""
        qs, ts = _levels(q), _levels(thresholds)
        shape = (self.ny + 2, self.nx + 2)
        out = EnsembleQuantiles(np.empty((len(qs),) + shape), np.empty((len(ts),) + shape))
        _ck(lib().csim_ensemble_quantiles(self._h, len(qs), _dp(qs), len(ts), _dp(ts), _dp(out.q), _dp(out.exceed)))
        return out

    def quantiles_begin(self, q, thresholds=()):
        """start quantiles() of the current state without waiting; run() may follow before quantiles_wait()"""
        qs, ts = _levels(q), _levels(thresholds)
        _ck(lib().csim_ensemble_quantiles_begin(self._h, len(qs), _dp(qs), len(ts), _dp(ts)))
        self._q_counts = (len(qs), len(ts))

    def quantiles_wait(self) -> EnsembleQuantiles:
        """the quantiles quantiles_begin() captured (copies)"""
        pq, pp = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        _ck(lib().csim_ensemble_quantiles_wait(self._h, C.byref(pq), C.byref(pp)))
        shape = (self.ny + 2, self.nx + 2)
        return EnsembleQuantiles(*[np.ctypeslib.as_array(p, shape=(n,) + shape).copy() if n else np.empty((0,) + shape)
                                   for p, n in zip((pq, pp), self._q_counts)])

    def _truth_args(self, truth, truth_member):
        if truth is not None:
            truth = np.ascontiguousarray(truth, dtype=np.float64)
            if truth.shape != (self.ny + 2, self.nx + 2):
                raise ValueError(f"truth must have shape {(self.ny + 2, self.nx + 2)}")
        forecast = self.members - (truth_member is not None)
        return truth, (None if truth is None else _dp(truth)), -1 if truth_member is None else int(truth_member), forecast

    def verify(self, truth=None, *, truth_member=None, thresholds=(), fair=False) -> EnsembleVerification:
        """CRPS, Brier scores, rank histogram and domain scores of the members against a truth: a host field
        (ny+2, nx+2), or member truth_member against the other members (csim_ensemble_verify)"""
        truth, tp, tm, M = self._truth_args(truth, truth_member)
        ts = _levels(thresholds)
        shape = (self.ny + 2, self.nx + 2)
        crps, brier = np.empty(shape), np.empty((len(ts),) + shape)
        hist, sc = np.zeros(max(M, 0) + 1, dtype=np.uint64), CsimVerifyScores()
        _ck(lib().csim_ensemble_verify(self._h, tp, tm, int(bool(fair)), len(ts), _dp(ts), _dp(crps), _dp(brier),
                                       hist.ctypes.data_as(C.POINTER(C.c_ulonglong)), C.byref(sc)))
        return EnsembleVerification(crps, brier, hist, _scores(sc, len(ts)))

    def verify_begin(self, truth=None, *, truth_member=None, thresholds=(), fair=False):
        """start verify() of the current state without waiting; run() may follow before verify_wait()"""
        truth, tp, tm, M = self._truth_args(truth, truth_member)
        ts = _levels(thresholds)
        _ck(lib().csim_ensemble_verify_begin(self._h, tp, tm, int(bool(fair)), len(ts), _dp(ts)))
        self._v_counts = (M, len(ts))

    def verify_wait(self) -> EnsembleVerification:
        """the verification verify_begin() captured (copies)"""
        pc, pb = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
        ph, sc = C.POINTER(C.c_ulonglong)(), CsimVerifyScores()
        _ck(lib().csim_ensemble_verify_wait(self._h, C.byref(pc), C.byref(pb), C.byref(ph), C.byref(sc)))
        M, nt = self._v_counts
        shape = (self.ny + 2, self.nx + 2)
        crps = np.ctypeslib.as_array(pc, shape=shape).copy()
        brier = np.ctypeslib.as_array(pb, shape=(nt,) + shape).copy() if nt else np.empty((0,) + shape)
        hist = np.ctypeslib.as_array(ph, shape=(M + 1,)).copy()
        return EnsembleVerification(crps, brier, hist, _scores(sc, nt))

    def _spatial_args(self, truth, truth_member, thresholds, half_widths):
        truth, tp, tm, M = self._truth_args(truth, truth_member)
        ts = _levels(thresholds)
        hs = _ints(half_widths) if len(half_widths) else np.zeros(0, dtype=np.int32)
        return truth, tp, tm, M, ts, hs

    def _spatial_result(self, M, nt, ns, table, nbh, cells, nan_cells, counts, flags) -> SpatialVerification:
        scores = verify_spatial_finish(M, table, nbh, cells, nan_cells)
        return SpatialVerification(table, nbh.reshape(nt, ns, 3), cells, nan_cells, scores, counts, flags)

    def verify_spatial(self, truth=None, *, truth_member=None, thresholds, half_widths=(),
                       counts=False) -> SpatialVerification:
        """neighbourhood and probability verification against a truth (as verify()): per threshold the contingency
        table of (members exceeding, truth exceeding) over the interior and, per half-width, the window sums behind the
        Fractions Skill Score, all exact integers from the device, and the scores finished from them: Brier score with
        reliability / resolution / uncertainty, ROC and FSS (csim_ensemble_verify_spatial).  counts=True also returns
        the per-cell member counts and the flags word"""
        truth, tp, tm, M, ts, hs = self._spatial_args(truth, truth_member, thresholds, half_widths)
        nt, ns = len(ts), len(hs)
        table = np.zeros((nt, max(M, 0) + 1, 2), dtype=np.uint64)
        nbh = np.zeros((nt, ns, 3), dtype=np.uint64)
        cnt = np.zeros((nt, self.ny, self.nx), dtype=np.uint16) if counts else None
        fl = np.zeros((self.ny, self.nx), dtype=np.uint32) if counts else None
        n, nan = C.c_ulonglong(), C.c_ulonglong()
        _ck(lib().csim_ensemble_verify_spatial(
            self._h, tp, tm, nt, _dp(ts), ns, _ip(hs), _u8p(table), _u8p(nbh),
            cnt.ctypes.data_as(C.POINTER(C.c_ushort)) if counts else None,
            fl.ctypes.data_as(C.POINTER(C.c_uint)) if counts else None, C.byref(n), C.byref(nan)))
        return self._spatial_result(M, nt, ns, table, nbh, n.value, nan.value, cnt, fl)

    def verify_spatial_begin(self, truth=None, *, truth_member=None, thresholds, half_widths=(), counts=False):
        """start verify_spatial() of the current state without waiting; run() may follow before verify_spatial_wait()"""
        truth, tp, tm, M, ts, hs = self._spatial_args(truth, truth_member, thresholds, half_widths)
        _ck(lib().csim_ensemble_verify_spatial_begin(self._h, tp, tm, len(ts), _dp(ts), len(hs), _ip(hs),
                                                     int(bool(counts))))
        self._s_counts = (M, len(ts), len(hs), bool(counts))

    def verify_spatial_wait(self) -> SpatialVerification:
        """the verification verify_spatial_begin() captured (copies)"""
        u8p = C.POINTER(C.c_ulonglong)
        pt, pn, pc, pf = u8p(), u8p(), C.POINTER(C.c_ushort)(), C.POINTER(C.c_uint)()
        n, nan = C.c_ulonglong(), C.c_ulonglong()
        _ck(lib().csim_ensemble_verify_spatial_wait(self._h, C.byref(pt), C.byref(pn), C.byref(pc), C.byref(pf),
                                                    C.byref(n), C.byref(nan)))
        M, nt, ns, fields = self._s_counts
        table = np.ctypeslib.as_array(pt, shape=(nt, M + 1, 2)).copy()
        nbh = np.ctypeslib.as_array(pn, shape=(nt, ns, 3)).copy() if ns else np.zeros((nt, 0, 3), dtype=np.uint64)
        cnt = np.ctypeslib.as_array(pc, shape=(nt, self.ny, self.nx)).copy() if fields else None
        fl = np.ctypeslib.as_array(pf, shape=(self.ny, self.nx)).copy() if fields else None
        return self._spatial_result(M, nt, ns, table, nbh, n.value, nan.value, cnt, fl)

    def assimilate(self, i, j, y, r, loc, inflation=1.0, truth_member=None, ordered=False, diagnostics=True):
        """serial EnSRF analysis of the forecast members with point observations at interior cells (i, j), values y
        and error variances r (a scalar broadcasts), Gaspari-Cohn length loc (csim_ensemble_assimilate).  With
        diagnostics: an EnsembleAnalysis (synchronous); without: the level count, and the work is only enqueued.
        inflation= is one factor for the whole field, applied before the analysis; prior_capture() before and relax()
        after the analysis is the spatially selective alternative"""
        ii = _ints(i)
        n = len(ii)
        jj = _ints(j, n)
        yy = np.ascontiguousarray(np.broadcast_to(np.asarray(y, dtype=np.float64), (n,)))
        rr = np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.float64), (n,)))
        tm = -1 if truth_member is None else int(truth_member)
        nl = C.c_int()
        outs = [np.empty(n) for _ in range(4)] if diagnostics else [None] * 4
        ptr = [_dp(o) if o is not None else None for o in outs]
        _ck(lib().csim_ensemble_assimilate(self._h, n, _ip(ii), _ip(jj), _dp(yy), _dp(rr), float(loc),
                                           float(inflation), tm, int(bool(ordered)), *ptr, C.byref(nl)))
        if not diagnostics:
            return nl.value
        return EnsembleAnalysis(nl.value, *outs)

    def obs_network(self, i, j, r, loc, ordered=False, log_cycles=0, taps=None) -> ObsNetwork:
        """an observation network on the device: cells (i, j), error variances r (a scalar broadcasts), Gaspari-Cohn
        length loc and the plan of assimilate(), made once; log_cycles: room for that many recorded analyses
        (csim_obs_network_create).  taps=(start, di, dj, w), as bilinear_taps() and box_taps() return them: linear
        observations sum_s w_s x(i + di_s, j + dj_s) anchored at (i, j) (csim_obs_network_create_linear)"""
        return ObsNetwork(self, i, j, r, loc, ordered, log_cycles, taps)

    def assimilate_network(self, net: ObsNetwork, inflation=1.0, truth_member=None, record=False, screen=None):
        """the analysis of assimilate() with the network's observations, always enqueued without waiting; record=True
        also appends the cycle's innovation statistics to the network's log on the device
        (csim_ensemble_assimilate_network).  Observations that net.set_active() masks out take no part.  screen=tol > 0
        adds the background check on the device: an observation with (y - hb)^2 > tol^2 (vb + r) is rejected
        (csim_ensemble_assimilate_screened); net.status() tells which were used"""
        tm = -1 if truth_member is None else int(truth_member)
        rec = record if isinstance(record, int) else int(bool(record))
        if screen is None or screen == 0:
            _ck(lib().csim_ensemble_assimilate_network(self._h, net._h, float(inflation), tm, rec))
        else:
            _ck(lib().csim_ensemble_assimilate_screened(self._h, net._h, float(inflation), tm, rec, float(screen)))

    def assimilate_local(self, net: ObsNetwork, inflation=1.0, truth_member=None, record=False, screen=None):
        """the local analysis with the network's observations, always enqueued: every cell from all used observations
        near it, R-localised, in input order, in one pass whatever the network (csim_ensemble_assimilate_local).
        inflation, truth_member, record and screen as in assimilate_network; CsimError (unsupported) beyond
        LOCAL_MAX_OBS windows over one cell, see net.local_info()"""
        tm = -1 if truth_member is None else int(truth_member)
        rec = record if isinstance(record, int) else int(bool(record))
        _ck(lib().csim_ensemble_assimilate_local(self._h, net._h, float(inflation), tm, rec,
                                                 0.0 if screen is None else float(screen)))

    def assimilate_letkf(self, net: ObsNetwork, inflation=1.0, truth_member=None, record=False, screen=None, spacing=8):
        """the LETKF with the network's observations, always enqueued: ensemble-space weights from the used observations
        near each analysis node, R-localised with the network's loc, on the lattice letkf_nodes(nx, ny, spacing), blended
        to the cells between the nodes; spacing=1 is the full LETKF.  inflation (on the field), truth_member, record and
        screen as in assimilate_local, whose limits on the windows over one cell do not apply; CsimError (unsupported)
        beyond LETKF_MAX_NODES nodes or LETKF_MAX_BYTES of node storage, see letkf_plan()
        (csim_ensemble_assimilate_letkf)"""
        tm = -1 if truth_member is None else int(truth_member)
        rec = record if isinstance(record, int) else int(bool(record))
        _ck(lib().csim_ensemble_assimilate_letkf(self._h, net._h, float(inflation), tm, rec,
                                                 0.0 if screen is None else float(screen), int(spacing)))

    def letkf_info(self) -> LetkfInfo:
        """what the nodes of the ensemble's last assimilate_letkf() found; waits for the stream, and raises CsimError
        when a node's Gram matrix was not finite (csim_ensemble_letkf_info)"""
        nax, nay = C.c_int(), C.c_int()
        rc = lib().csim_ensemble_letkf_info(self._h, C.byref(nax), C.byref(nay), None, None, None, None)
        if nax.value == 0:  # there was no LETKF
            _ck(rc)
        shape = (nay.value, nax.value)
        dfs = np.empty(shape)
        count, sweeps, status = (np.zeros(shape, dtype=np.int32) for _ in range(3))
        rc = lib().csim_ensemble_letkf_info(self._h, None, None, _dp(dfs), _ip(count), _ip(sweeps), _ip(status))
        self.letkf_last = LetkfInfo(dfs, count, sweeps, status)  # filled even where the call fails
        _ck(rc)
        return self.letkf_last

    def obs_gram(self, net: ObsNetwork, truth_member=None, loglik=False, held=False) -> ObsGram:
        """the observation-space Gram matrix of the forecast members over the network's active observations, and with
        loglik=True each member's sum of squared normalised departures (a particle weight is exp(-loglik / 2));
        synchronous, writes nothing of the network (csim_ensemble_obs_gram).  held=True: from the rows that the network
        holds (ObsNetwork.hold) instead of the current members; the members and the truth member are the hold's
        (csim_ensemble_obs_gram_held)"""
        if held:
            Mh = C.c_int()
            _ck(lib().csim_obs_network_held(net._h, None, C.byref(Mh), None))
            M = Mh.value
            A = np.empty((M + 1, M + 1))
            ll = np.empty(M) if loglik else None
            used = C.c_longlong()
            _ck(lib().csim_ensemble_obs_gram_held(self._h, net._h, _dp(A), None if ll is None else _dp(ll),
                                                  C.byref(used)))
            return ObsGram(A, ll, used.value)
        tm, M = self._forecast(truth_member)
        A = np.empty((max(M, 0) + 1, max(M, 0) + 1))
        ll = np.empty(max(M, 0)) if loglik else None
        used = C.c_longlong()
        _ck(lib().csim_ensemble_obs_gram(self._h, net._h, tm, _dp(A), None if ll is None else _dp(ll),
                                         C.byref(used)))
        return ObsGram(A, ll, used.value)

    def assimilate_etkf(self, net: ObsNetwork, inflation=1.0, truth_member=None, record=False,
                        screen=None, device=False, held=False):
        """the global ETKF analysis with the network's observations: obs_gram() over the used ones, etkf_weights() and
        transform() composed in the library; waits for the Gram matrix, the transform is enqueued.  inflation (taken in
        ensemble space), truth_member, record and screen as in assimilate_network; the network's loc plays no part
        (csim_ensemble_assimilate_etkf).  device=True: the eigensolver and the weights run on the GPU in the
        round-robin order, the call only enqueues and returns None; etkf_info() waits and tells what it found
        (csim_ensemble_assimilate_etkf_device).  held=True: the 4D form, with the weights from the rows that the network
        holds from its observations' own times (ObsNetwork.hold) and the rows transformed with the members
        (csim_ensemble_assimilate_etkf_held)"""
        tm, M = self._forecast(truth_member)
        rec = record if isinstance(record, int) else int(bool(record))
        if held:
            _ck(lib().csim_ensemble_assimilate_etkf_held(self._h, net._h, float(inflation), tm, rec,
                                                         0.0 if screen is None else float(screen), int(bool(device))))
            if device:
                return None
        elif device:
            _ck(lib().csim_ensemble_assimilate_etkf_device(self._h, net._h, float(inflation), tm, rec,
                                                           0.0 if screen is None else float(screen)))
            return None
        else:
            _ck(lib().csim_ensemble_assimilate_etkf(self._h, net._h, float(inflation), tm, rec,
                                                    0.0 if screen is None else float(screen)))
        used, chi2, dfs, ng = C.c_longlong(), C.c_double(), C.c_double(), C.c_int()
        gamma = np.empty(M)
        _ck(lib().csim_ensemble_etkf_info(self._h, C.byref(used), C.byref(chi2), C.byref(dfs), _dp(gamma),
                                          C.byref(ng)))
        return EtkfAnalysis(used.value, chi2.value, gamma, dfs.value)

    def etkf_info(self) -> EtkfInfo:
        """what the ensemble's last assimilate_etkf() found; after device=True it waits for the stream first, and a
        non-finite Gram matrix, which left the members unchanged, raises CsimError (csim_ensemble_etkf_info2)"""
        used, chi2, dfs, ng = C.c_longlong(), C.c_double(), C.c_double(), C.c_int()
        sweeps, status = C.c_int(), C.c_int()
        gamma = np.empty(ESPACE_MAX_MEMBERS)
        _ck(lib().csim_ensemble_etkf_info2(self._h, C.byref(used), C.byref(chi2), C.byref(dfs), _dp(gamma),
                                           C.byref(ng), C.byref(sweeps), C.byref(status)))
        return EtkfInfo(used.value, chi2.value, gamma[:ng.value].copy(), dfs.value, sweeps.value, status.value)

    def _obs_impact(self, call, net, weight) -> ObsImpact:
        w = np.ascontiguousarray(weight, dtype=np.float64)
        if w.shape != (self.ny + 2, self.nx + 2):
            raise ValueError(f"weight must have shape {(self.ny + 2, self.nx + 2)}")
        out, sm = np.empty(net.nobs), CsimObsImpactSummary()
        _ck(call(self._h, net._h, _dp(w), _dp(out), C.byref(sm)))
        return ObsImpact(out, ObsImpactSummary(sm.used, sm.beneficial, sm.total))

    def obs_impact(self, net: ObsNetwork, weight) -> ObsImpact:
        """the forecast impact J_o of every observation of net's captured analysis on the error of the current
        (verification-time) state, EFSOI: weight is C (e_a + e_b) as a (ny+2, nx+2) field, impact_weight() for the mean
        squared error; J_o < 0: the observation reduced the forecast error.  Synchronous (csim_ensemble_obs_impact)"""
        return self._obs_impact(lib().csim_ensemble_obs_impact, net, weight)

    def obs_impact_global(self, net: ObsNetwork, weight) -> ObsImpact:
        """obs_impact() without localisation, for a capture made after a global analysis (assimilate_etkf, either
        path), whose gain satisfies the estimate's premise exactly: one read of the members whatever the network,
        g = dot(weight), then J_o = dn_o sum_k a_{o,k} g_k / (M-1).  Synchronous (csim_ensemble_obs_impact_global)"""
        return self._obs_impact(lib().csim_ensemble_obs_impact_global, net, weight)

    def perturb(self, sigma, corr_len, seed, draw=0, centered=False, truth_member=None):
        """adds sigma times a seeded Gaussian random field of correlation length corr_len to the interior of every
        forecast member; a pure function of (seed, draw, member, cell), enqueued without waiting
        (csim_ensemble_perturb)"""
        seed, draw = int(seed), int(draw)
        if not (0 <= seed < 1 << 64 and 0 <= draw < 1 << 32):
            raise ValueError("seed must fit 64 bits and draw 32 bits, unsigned")
        tm = -1 if truth_member is None else int(truth_member)
        _ck(lib().csim_ensemble_perturb(self._h, seed, draw, float(sigma), float(corr_len),
                                        centered if isinstance(centered, int) else int(bool(centered)), tm))

    def prior_capture(self, mode="spread", truth_member=None):
        """keeps what relax() of the same mode and truth member needs of the current (forecast) state: the per-cell
        spread ("spread", RTPS) or the members themselves ("pert", RTPP); valid until the next run of at least one
        step or the next capture, enqueued without waiting (csim_ensemble_prior_capture)"""
        mode, tm = _relax_mode(mode), -1 if truth_member is None else int(truth_member)
        _ck(lib().csim_ensemble_prior_capture(self._h, mode, tm))

    def relax(self, alpha, mode="spread", truth_member=None, factor=False):
        """relaxation inflation after an analysis, cell by cell: towards the captured spread (x_k += f (x_k - mean),
        f = alpha (sb - sa) / sa; cells with f == 0 are not written) or the captured perturbations.  Enqueued without
        waiting; with factor=True ("spread" only) synchronous, returning f as a (ny+2, nx+2) array
        (csim_ensemble_relax)"""
        mode, tm = _relax_mode(mode), -1 if truth_member is None else int(truth_member)
        out = np.empty((self.ny + 2, self.nx + 2)) if factor else None
        _ck(lib().csim_ensemble_relax(self._h, mode, float(alpha), tm, None if out is None else _dp(out)))
        return out

    def _forecast(self, truth_member):
        return -1 if truth_member is None else int(truth_member), self.members - (truth_member is not None)

    def gram(self, truth_member=None, centered=True) -> np.ndarray:
        """(M, M) Gram matrix of the forecast members over the interior, G[a, b] = sum over cells of p_a p_b, p the
        perturbations from the per-cell mean (centered) or the members themselves; the same bits whatever the launch
        geometry, symmetric bit for bit (csim_ensemble_gram)"""
        tm, M = self._forecast(truth_member)
        G = np.empty((max(M, 0), max(M, 0)))
        _ck(lib().csim_ensemble_gram(self._h, tm, int(bool(centered)), _dp(G)))
        return G

    def project(self, W, truth_member=None, centered=True) -> np.ndarray:
        """(K, ny+2, nx+2): out[r] = sum_k p_k W[k, r] on every cell, ghost ring included; W is (M, K) or (M,)
        (csim_ensemble_project)"""
        tm, M = self._forecast(truth_member)
        w = np.ascontiguousarray(W, dtype=np.float64)
        if w.ndim == 1:
            w = np.ascontiguousarray(w[:, None])
        if w.ndim != 2 or w.shape[0] != M:
            raise ValueError(f"W must have {M} rows")
        out = np.empty((w.shape[1], self.ny + 2, self.nx + 2))
        _ck(lib().csim_ensemble_project(self._h, tm, int(bool(centered)), w.shape[1], _dp(w), _dp(out)))
        return out

    def dot(self, fields, truth_member=None, centered=True) -> np.ndarray:
        """(M, K): out[k, r] = sum over the interior of p_k fields[r], the adjoint of project(); fields is
        (K, ny+2, nx+2) or one (ny+2, nx+2) field (K = 1), of which only the interior is read; summed in the order of
        gram() (csim_ensemble_dot)"""
        tm, M = self._forecast(truth_member)
        f = np.ascontiguousarray(fields, dtype=np.float64)
        if f.ndim == 2:
            f = np.ascontiguousarray(f[None])
        if f.ndim != 3 or f.shape[1:] != (self.ny + 2, self.nx + 2):
            raise ValueError(f"fields must have shape (K, {self.ny + 2}, {self.nx + 2})")
        out = np.empty((max(M, 0), f.shape[0]))
        _ck(lib().csim_ensemble_dot(self._h, tm, int(bool(centered)), f.shape[0], _dp(f), _dp(out)))
        return out

    def transform(self, W, wbar=None, truth_member=None, centered=True):
        """replaces the forecast members on the interior by x'_r = m' + sum_k p_k W[k, r], m' = m + sum_k p_k wbar[k]
        (centered; without wbar m' = m), or by x'_r = sum_k x_k W[k, r] (not centered: a 0/1 selection matrix copies
        or resamples members exactly); W is (M, M).  Enqueued without waiting, W and wbar may be reused at once
        (csim_ensemble_transform)"""
        tm, M = self._forecast(truth_member)
        w = np.ascontiguousarray(W, dtype=np.float64)
        if w.shape != (M, M):
            raise ValueError(f"W must have shape {(M, M)}")
        wb = None if wbar is None else np.ascontiguousarray(wbar, dtype=np.float64)
        if wb is not None and wb.shape != (M,):
            raise ValueError(f"wbar must have shape {(M,)}")
        _ck(lib().csim_ensemble_transform(self._h, tm, int(bool(centered)), _dp(w), None if wb is None else _dp(wb)))

    def eofs(self, n_modes, truth_member=None, patterns=True) -> EnsembleEOFs:
        """the n_modes leading EOFs of the forecast members' spread: centered gram(), sym_eigen() and project()
        composed in the library (csim_ensemble_eofs)"""
        tm, M = self._forecast(truth_member)
        K = int(n_modes)
        lam, pcs = np.empty(max(K, 0)), np.empty((max(M, 0), max(K, 0)))
        pat = np.empty((max(K, 0), self.ny + 2, self.nx + 2)) if patterns else None
        nv = C.c_int()
        _ck(lib().csim_ensemble_eofs(self._h, tm, K, _dp(lam), _dp(pcs), None if pat is None else _dp(pat),
                                     C.byref(nv)))
        return EnsembleEOFs(lam, lam / (M - 1), pcs, pat, nv.value)

    def set_option(self, key: str, value: int):
        _ck(lib().csim_ensemble_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key: str) -> int:
        v = C.c_long()
        _ck(lib().csim_ensemble_get_option(self._h, key.encode(), C.byref(v)))
        return v.value
