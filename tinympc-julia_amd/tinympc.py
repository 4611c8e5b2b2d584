"""Python mirror of the reference's Julia module over the C-ABI (ctypes in place of ccall).

Same names, argument meaning and error behaviour as reference src/TinyMPC.jl:
  TinyMPCSolver (:34-48), setup (:55-112), set_x0 / set_x_ref / set_u_ref (:115-141),
  solve (:143-148, returns the status without throwing), get_solution (:150-177),
  update_settings (:181-211), set_bound_constraints (:214-227), set_cache_terms (:278-292)
with a batch dimension added:
  setup(..., batch=B); set_x0 takes (nx,) or (nx, B); set_x_ref (nx, N) or (nx, N, B);
  get_solution returns states (nx, N, B) / controls (nu, N-1, B) (squeezed to 2-D for B == 1,
  i.e. exactly the reference's shapes).

Like the reference (one process-global `g_solver`, bindings.cpp:15) the module-level functions
drive ONE global solver inside libtinympc_hip.so; `BatchSolver` wraps the handle API for callers
that need several solvers or device-resident I/O.

The library is the HIP build only.  If it is missing, or no GPU is usable, calls raise — there is
no CPU fallback.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "lib", "libtinympc_hip.so")

c_dp = ctypes.POINTER(ctypes.c_double)
c_fp = ctypes.POINTER(ctypes.c_float)
c_ip = ctypes.POINTER(ctypes.c_int)
c_int = ctypes.c_int
c_dbl = ctypes.c_double
c_vp = ctypes.c_void_p
c_ull = ctypes.c_ulonglong
c_up = ctypes.POINTER(ctypes.c_uint)


class TinyMPCError(RuntimeError):
    pass


_lib = None

# name -> (restype, argtypes); every symbol include/tinympc_hip.h declares
SIGNATURES = {
    "setup_solver": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int,
                             c_int, c_dp, c_int, c_int, c_dbl, c_int, c_int, c_int, c_int]),
    "set_x0": (c_int, [c_dp, c_int, c_int, c_int]),
    "set_x_ref": (c_int, [c_dp, c_int, c_int, c_int]),
    "set_u_ref": (c_int, [c_dp, c_int, c_int, c_int]),
    "solve_mpc": (c_int, [c_int]),
    "get_states": (c_int, [c_dp, c_ip, c_ip]),
    "get_controls": (c_int, [c_dp, c_ip, c_ip]),
    "cleanup_solver": (None, []),
    "update_settings": (c_int, [c_dbl, c_dbl, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_int, c_dbl, c_dbl, c_int, c_int]),
    "set_bound_constraints": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int,
                                      c_dp, c_int, c_int, c_int]),
    "set_cache_terms": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp,
                                c_int, c_int, c_int]),
    "set_sensitivity": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int, c_int]),
    "get_adaptive_rho": (c_int, [c_dp, c_ip]),
    "set_warm_start": (c_int, [c_int]),
    "get_kernel_name": (ctypes.c_char_p, []),
    "get_cone_mode": (c_int, []),
    "print_problem_data": (c_int, [c_int]),
    "set_linear_constraints": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_dp, c_int, c_int, c_dp,
                                       c_int, c_int]),
    "set_cone_constraints": (c_int, [c_ip, c_int, c_ip, c_int, c_dp, c_int, c_ip, c_int, c_ip, c_int,
                                     c_dp, c_int, c_int]),
    "set_batch_size": (c_int, [c_int]),
    "get_batch_size": (c_int, []),
    "get_status": (c_int, [c_ip, c_ip, c_dp]),
    "reset_workspace": (c_int, []),
    "tinympc_create": (c_int, [ctypes.POINTER(c_vp), c_dp, c_dp, c_dp, c_dp, c_dbl, c_int, c_int,
                               c_int, c_int, c_int, c_int]),
    "tinympc_create_families": (c_int, [ctypes.POINTER(c_vp), c_dp, c_dp, c_dp, c_dp, c_dp, c_int, c_int, c_int,
                                        c_int, c_int, c_int]),
    "tinympc_create_families_device": (c_int, [ctypes.POINTER(c_vp), c_dp, c_dp, c_dp, c_dp, c_dp, c_int, c_int, c_int,
                                               c_int, c_int, c_int]),
    "tinympc_set_families": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_get_family_cache": (c_int, [c_vp, c_int, c_int, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "tinympc_families_setup_mode": (c_int, [c_vp]),
    "tinympc_families_setup_ms": (c_int, [c_vp, c_dp]),
    "tinympc_host_precompute_sweeps": (c_int, [c_dp, c_dp, c_dp, c_dp, c_dbl, c_int, c_int]),
    "tinympc_host_family_cache": (c_int, [c_dp, c_dp, c_dp, c_dp, c_dbl, c_int, c_int, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "setup_families": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int, c_int,
                               c_int, c_int, c_int, c_int]),
    "set_families": (c_int, [c_dp, c_dp, c_dp, c_dp, c_dp]),
    "get_family_cache": (c_int, [c_int, c_int, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "families_setup_mode": (c_int, []),
    "tinympc_destroy": (None, [c_vp]),
    "tinympc_update_settings": (c_int, [c_vp, c_dbl, c_dbl, c_int, c_int, c_int, c_int]),
    "tinympc_set_bound_constraints": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_set_instance_bounds": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp, c_int]),
    "tinympc_bounds_mode": (c_int, [c_vp]),
    "tinympc_set_cache_terms": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_get_cache_terms": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_set_fdyn": (c_int, [c_vp, c_dp]),
    "tinympc_set_cone_constraints": (c_int, [c_vp, c_ip, c_ip, c_dp, c_int, c_ip, c_ip, c_dp, c_int]),
    "tinympc_enable_cones": (c_int, [c_vp, c_int, c_int]),
    "tinympc_set_linear_constraints": (c_int, [c_vp, c_dp, c_int, c_dp, c_dp, c_int, c_dp]),
    "tinympc_enable_linear": (c_int, [c_vp, c_int, c_int]),
    "tinympc_set_instance_linear": (c_int, [c_vp, c_dp, c_int, c_dp, c_dp, c_int, c_dp]),
    "tinympc_lin_mode": (c_int, [c_vp]),
    "tinympc_set_instance_cones": (c_int, [c_vp, c_ip, c_ip, c_dp, c_int, c_ip, c_ip, c_dp, c_int]),
    "tinympc_cone_mode": (c_int, [c_vp]),
    "tinympc_set_x0": (c_int, [c_vp, c_dp, c_int]),
    "tinympc_set_x_ref": (c_int, [c_vp, c_dp, c_int]),
    "tinympc_set_u_ref": (c_int, [c_vp, c_dp, c_int]),
    "tinympc_reset": (c_int, [c_vp]),
    "tinympc_set_warm_start": (c_int, [c_vp, c_int]),
    "tinympc_solve": (c_int, [c_vp]),
    "tinympc_get_states": (c_int, [c_vp, c_dp]),
    "tinympc_get_controls": (c_int, [c_vp, c_dp]),
    "tinympc_get_status": (c_int, [c_vp, c_ip, c_ip, c_dp]),
    "tinympc_get_workspace": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_set_workspace": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_device_buffers": (c_int, [c_vp] + [ctypes.POINTER(c_vp)] * 9),
    "tinympc_set_ref_mode": (c_int, [c_vp, c_int]),
    "tinympc_solve_async": (c_int, [c_vp, c_vp]),
    "tinympc_solve_status": (c_int, [c_vp]),
    "tinympc_mpc_rollout": (c_int, [c_vp, c_int, c_vp]),
    "tinympc_get_mpc_log": (c_int, [c_vp, c_dp, c_dp, c_ip]),
    "tinympc_set_x0_f32": (c_int, [c_vp, c_fp, c_int]),
    "tinympc_get_states_f32": (c_int, [c_vp, c_fp]),
    "tinympc_get_controls_f32": (c_int, [c_vp, c_fp]),
    "tinympc_pin_host": (c_int, [c_vp, c_vp, ctypes.c_size_t]),
    "tinympc_unpin_host": (c_int, [c_vp, c_vp]),
    "set_ref_sequence": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_int]),
    "mpc_rollout": (c_int, [c_int, c_dp, c_dp, c_ip]),
    "set_x0_f32": (c_int, [c_fp, c_int, c_int, c_int]),
    "get_states_f32": (c_int, [c_fp, c_ip, c_ip]),
    "get_controls_f32": (c_int, [c_fp, c_ip, c_ip]),
    "pin_host_buffer": (c_int, [c_vp, ctypes.c_size_t]),
    "set_precision": (c_int, [c_int]),
    "unpin_host_buffer": (c_int, [c_vp]),
    "tinympc_set_ref_sequence": (c_int, [c_vp, c_dp, c_int, c_int, c_dp, c_int, c_int, c_int]),
    "tinympc_set_plant": (c_int, [c_vp, c_dp, c_dp, c_dp, c_int]),
    "tinympc_set_disturbance": (c_int, [c_vp, c_dp, c_int, c_int]),
    "tinympc_plant_mode": (c_int, [c_vp]),
    "set_plant": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_dp, c_int, c_int]),
    "set_disturbance": (c_int, [c_dp, c_int, c_int, c_int]),
    "plant_mode": (c_int, []),
    "tinympc_set_ref_trajectory": (c_int, [c_vp, c_dp, c_int, c_dp, c_int, c_int]),
    "tinympc_set_ref_cursor": (c_int, [c_vp, c_int]),
    "tinympc_ref_cursor": (c_int, [c_vp]),
    "tinympc_ref_trajectory_mode": (c_int, [c_vp]),
    "set_ref_trajectory": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_int, c_int]),
    "set_ref_cursor": (c_int, [c_int]),
    "ref_cursor": (c_int, []),
    "tinympc_set_process_noise": (c_int, [c_vp, c_dp, c_int, c_ull]),
    "tinympc_set_measurement_noise": (c_int, [c_vp, c_dp, c_int, c_ull]),
    "tinympc_set_noise_cursor": (c_int, [c_vp, c_int]),
    "tinympc_noise_cursor": (c_int, [c_vp]),
    "tinympc_noise_mode": (c_int, [c_vp]),
    "tinympc_get_noise": (c_int, [c_vp, c_int, c_int, c_int, c_dp]),
    "tinympc_get_mpc_measured": (c_int, [c_vp, c_dp]),
    "tinympc_host_noise": (c_int, [c_ull, c_int, ctypes.c_longlong, c_int, c_int, c_dp, c_dp]),
    "tmpc_philox4x32_10": (c_int, [c_up, c_up, c_up]),
    "set_process_noise": (c_int, [c_dp, c_int, c_int, c_int, c_ull]),
    "set_measurement_noise": (c_int, [c_dp, c_int, c_int, c_int, c_ull]),
    "set_noise_cursor": (c_int, [c_int]),
    "noise_cursor": (c_int, []),
    "noise_mode": (c_int, []),
    "get_noise": (c_int, [c_int, c_int, c_int, c_dp]),
    "get_mpc_measured": (c_int, [c_dp]),
    "tinympc_set_estimator": (c_int, [c_vp, c_dp, c_int, c_dp, c_int]),
    "tinympc_set_estimator_state": (c_int, [c_vp, c_dp, c_int]),
    "tinympc_estimator_mode": (c_int, [c_vp]),
    "tinympc_estimator_outputs": (c_int, [c_vp]),
    "tinympc_get_estimator_state": (c_int, [c_vp, c_dp]),
    "tinympc_get_mpc_estimate": (c_int, [c_vp, c_dp]),
    "tinympc_get_mpc_outputs": (c_int, [c_vp, c_dp]),
    "tinympc_host_estimator_step": (c_int, [c_int, c_int, c_int, c_int, c_int] + [c_dp] * 10),
    "tinympc_host_kalman_gain": (c_int, [c_dp, c_dp, c_dp, c_dp, c_int, c_int, c_dp, c_dp]),
    "set_estimator": (c_int, [c_dp, c_int, c_int, c_dp, c_int, c_int, c_int]),
    "set_estimator_state": (c_int, [c_dp, c_int, c_int]),
    "estimator_mode": (c_int, []),
    "estimator_outputs": (c_int, []),
    "get_estimator_state": (c_int, [c_dp]),
    "get_mpc_estimate": (c_int, [c_dp]),
    "get_mpc_outputs": (c_int, [c_dp]),
    "tinympc_set_rollout_metrics": (c_int, [c_vp, c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_reset_rollout_metrics": (c_int, [c_vp]),
    "tinympc_rollout_metrics_mode": (c_int, [c_vp]),
    "tinympc_get_rollout_metrics": (c_int, [c_vp, c_dp]),
    "tinympc_get_rollout_summary": (c_int, [c_vp, c_dp]),
    "tinympc_host_rollout_metrics": (c_int, [c_int, c_int, c_int, c_fp, c_fp, c_ip, c_fp, c_fp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "set_rollout_metrics": (c_int, [c_int, c_dp, c_int, c_dp, c_int, c_dp, c_dp, c_dp, c_dp]),
    "reset_rollout_metrics": (c_int, []),
    "get_rollout_metrics": (c_int, [c_dp]),
    "get_rollout_summary": (c_int, [c_dp]),
    "tinympc_set_profiling": (c_int, [c_vp, c_int]),
    "tinympc_set_compaction": (c_int, [c_vp, c_int]),
    "tinympc_set_adaptive_rho": (c_int, [c_vp, c_int, c_dbl, c_dbl, c_int]),
    "tinympc_set_sensitivity": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_compute_sensitivity": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_get_adaptive_state": (c_int, [c_vp, c_dp, c_dp, c_dp]),
    "tinympc_kernel_elapsed_ms": (c_dbl, [c_vp]),
    "tinympc_kernel_elapsed_mean_ms": (c_dbl, [c_vp, c_int]),
    "tinympc_set_precision": (c_int, [c_vp, c_int]),
    "tinympc_kernel_name": (ctypes.c_char_p, [c_vp]),
    "tinympc_last_launch_name": (ctypes.c_char_p, [c_vp]),
    "tinympc_set_strict_precision": (c_int, [c_vp, c_int]),
    "tinympc_effective_precision": (c_int, [c_vp]),
    "tinympc_reload_switches": (c_int, [c_vp]),
    "tinympc_specialise": (c_int, [c_int, c_int, c_int, c_int]),
    "tinympc_algorithmic_bytes": (c_dbl, [c_vp]),
    "tinympc_algorithmic_flops": (c_dbl, [c_vp, c_int]),
    "tinympc_last_error": (ctypes.c_char_p, []),
    "tinympc_host_precompute": (c_int, [c_dp, c_dp, c_dp, c_dp, c_dbl, c_int, c_int, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_host_sensitivity": (c_int, [c_dp, c_dp, c_dp, c_dp, c_dbl, c_int, c_int, c_dp, c_dp, c_dp, c_dp]),
    # multi-GPU: one handle, n_gpus devices (include/tinympc_hip.h section 3)
    "tinympc_create_sharded": (c_int, [ctypes.POINTER(c_vp), c_dp, c_dp, c_dp, c_dp, c_dbl, c_int, c_int, c_int, c_int,
                                       c_int, c_ip, c_int]),
    "tinympc_sharded_destroy": (None, [c_vp]),
    "tinympc_sharded_n_shards": (c_int, [c_vp]),
    "tinympc_sharded_fold_backend": (ctypes.c_char_p, [c_vp]),
    "tinympc_sharded_shard": (c_int, [c_vp, c_int, c_ip, c_ip, c_ip, ctypes.POINTER(c_vp)]),
    "tinympc_shard_range": (None, [c_int, c_int, c_int, c_ip, c_ip]),
    "tinympc_sharded_update_settings": (c_int, [c_vp, c_dbl, c_dbl, c_int, c_int, c_int, c_int]),
    "tinympc_sharded_set_bound_constraints": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp]),
    "tinympc_sharded_set_instance_bounds": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp, c_int]),
    "tinympc_sharded_set_instance_linear": (c_int, [c_vp, c_dp, c_int, c_dp, c_dp, c_int, c_dp]),
    "tinympc_sharded_set_instance_cones": (c_int, [c_vp, c_ip, c_ip, c_dp, c_int, c_ip, c_ip, c_dp, c_int]),
    "tinympc_sharded_set_warm_start": (c_int, [c_vp, c_int]),
    "tinympc_sharded_reset": (c_int, [c_vp]),
    "tinympc_sharded_set_precision": (c_int, [c_vp, c_int]),
    "tinympc_sharded_set_compaction": (c_int, [c_vp, c_int]),
    "tinympc_sharded_set_x0": (c_int, [c_vp, c_dp, c_int]),
    "tinympc_sharded_set_x_ref": (c_int, [c_vp, c_dp, c_int]),
    "tinympc_sharded_set_u_ref": (c_int, [c_vp, c_dp, c_int]),
    "tinympc_sharded_solve": (c_int, [c_vp]),
    "tinympc_sharded_solve_async": (c_int, [c_vp]),
    "tinympc_sharded_wait": (c_int, [c_vp]),
    "tinympc_sharded_global_status": (c_int, [c_vp, c_dp, c_ip]),
    "tinympc_sharded_get_states": (c_int, [c_vp, c_dp]),
    "tinympc_sharded_get_controls": (c_int, [c_vp, c_dp]),
    "tinympc_sharded_get_status": (c_int, [c_vp, c_ip, c_ip, c_dp]),
    "tinympc_sharded_get_workspace": (c_int, [c_vp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "set_gpus": (c_int, [c_int]),
    "get_gpus": (c_int, []),
}


def load_library(path=None):
    """dlopen libtinympc_hip.so and bind every declared symbol (the `_ensure_loaded` of TinyMPC.jl:14)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or _LIB_PATH
    if not os.path.isfile(path):
        raise TinyMPCError(f"TinyMPC library not found: {path} (build it with __graft_entry__.build())")
    # A process that also uses PyTorch must load torch FIRST: the torch wheel brings its own copy of the HIP / HSA runtime
    # libraries, and if this library has pulled in the system's (/opt/rocm) before, torch's later initialisation finds
    # "No HIP GPUs" (two runtimes in one process; measured on this image).  A host without
    # torch (Julia, C) is not concerned.
    import sys
    if "torch" not in sys.modules and os.environ.get("TINYMPC_HIP_NO_TORCH_PRELOAD") is None:
        import importlib.util
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _err():
    try:
        return (load_library().tinympc_last_error() or b"").decode()
    except Exception:
        return ""


def _mat(a, name=None):
    m = np.asfortranarray(np.asarray(a, dtype=np.float64))
    if m.ndim == 1:
        m = np.asfortranarray(m.reshape(-1, 1))
    return m


def _dp(a):
    return a.ctypes.data_as(c_dp)


class TinyMPCSolver:
    """Mirror of the Julia struct (TinyMPC.jl:34-48): dims, rho, is_setup and copies of A, B, Q, R."""

    def __init__(self):
        self.nx = 0
        self.nu = 0
        self.N = 0
        self.batch = 1
        self.rho = 0.0
        self.is_setup = False
        self.A = np.zeros((0, 0))
        self.B = np.zeros((0, 0))
        self.Q = np.zeros((0, 0))
        self.R = np.zeros((0, 0))


def setup(solver, A, B, f, Q, R, rho, nx, nu, N, *, batch=1, n_gpus=1, verbose=False, abs_pri_tol=1e-3,
          abs_dua_tol=1e-3, max_iter=100, check_termination=True, adaptive_rho=False,
          adaptive_rho_min=0.1, adaptive_rho_max=10.0, adaptive_rho_clipping=True):
    """TinyMPC.jl:55-112.  Raises on failure like the Julia `error(...)`; returns the status."""
    lib = load_library()
    A, B, Q, R = _mat(A), _mat(B), _mat(Q), _mat(R)
    f = _mat(np.zeros(nx) if f is None else f)
    solver.nx, solver.nu, solver.N, solver.rho, solver.batch = nx, nu, N, float(rho), int(batch)
    solver.A, solver.B, solver.Q, solver.R = A.copy(), B.copy(), Q.copy(), R.copy()
    status = lib.setup_solver(_dp(A), A.shape[0], A.shape[1], _dp(B), B.shape[0], B.shape[1],
                              _dp(f), f.shape[0], f.shape[1], _dp(Q), Q.shape[0], Q.shape[1],
                              _dp(R), R.shape[0], R.shape[1], float(rho), nx, nu, N, 1 if verbose else 0)
    if status != 0:
        solver.is_setup = False
        raise TinyMPCError(f"Setup failed with status: {status} ({_err()})")
    if batch != 1 and lib.set_batch_size(int(batch)) != 0:
        raise TinyMPCError(f"Failed to set batch size ({_err()})")
    solver.is_setup = True
    if n_gpus != 1:
        set_gpus(solver, n_gpus)
    # TinyMPC.jl:89-104 — settings pushed with every en_* false
    update_settings(solver, abs_pri_tol=abs_pri_tol, abs_dua_tol=abs_dua_tol, max_iter=max_iter,
                    check_termination=check_termination, en_state_bound=False, en_input_bound=False,
                    en_state_soc=False, en_input_soc=False, en_state_linear=False,
                    en_input_linear=False, adaptive_rho=adaptive_rho,
                    adaptive_rho_min=adaptive_rho_min, adaptive_rho_max=adaptive_rho_max,
                    adaptive_rho_enable_clipping=adaptive_rho_clipping, verbose=verbose)
    return status


def _need_setup(solver):
    if not solver.is_setup:
        raise TinyMPCError("Solver not setup")


def set_gpus(solver, n_gpus):
    """Spread the global solver's batch over devices 0 .. n_gpus-1 of this node (contiguous shards, status all-reduced
    over RCCL): every other call then acts on the whole sharded batch.  Inputs / workspace are reset."""
    _need_setup(solver)
    if load_library().set_gpus(int(n_gpus)) != 0:
        raise TinyMPCError(f"Failed to set the number of GPUs ({_err()})")
    solver.n_gpus = int(n_gpus)
    return 0


def set_warm_start(solver, on):
    """on=False: every solve() starts from the zero workspace and keeps none (one-shot solves; the on-chip kernels
    apply); True (default): the reference's semantics, the workspace persists between solves"""
    _need_setup(solver)
    if load_library().set_warm_start(1 if on else 0) != 0:
        raise TinyMPCError(f"Failed to set warm start ({_err()})")


def kernel_name():
    """the kernel the global solver's last solve ran on"""
    return load_library().get_kernel_name().decode()


def cone_mode():
    """0 no cones or cones shared by the batch, 1 a coefficient per instance (the global solver; -1 without one)"""
    return int(load_library().get_cone_mode())


def set_batch_size(solver, batch):
    _need_setup(solver)
    if load_library().set_batch_size(int(batch)) != 0:
        raise TinyMPCError(f"Failed to set batch size ({_err()})")
    solver.batch = int(batch)
    return 0


def set_x0(solver, x0, *, verbose=False):
    """TinyMPC.jl:115-123.  x0: (nx,) broadcast to the batch, or (nx, batch)."""
    _need_setup(solver)
    m = _mat(x0)
    status = load_library().set_x0(_dp(m), m.shape[0], m.shape[1], 1 if verbose else 0)
    if status != 0:
        raise TinyMPCError(f"Failed to set initial state ({_err()})")
    return status


def _ref3(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 3:  # (rows, knots, batch) -> rows x (knots*batch), column-major
        a = np.asfortranarray(a).reshape(a.shape[0], -1, order="F")
    return _mat(a)


def set_x_ref(solver, x_ref, *, verbose=False):
    """TinyMPC.jl:125-132.  (nx, N) shared or (nx, N, batch)."""
    _need_setup(solver)
    m = _ref3(x_ref)
    status = load_library().set_x_ref(_dp(m), m.shape[0], m.shape[1], 1 if verbose else 0)
    if status != 0:
        raise TinyMPCError(f"Failed to set state reference ({_err()})")
    return status


def set_u_ref(solver, u_ref, *, verbose=False):
    """TinyMPC.jl:134-141.  (nu, N-1) shared or (nu, N-1, batch)."""
    _need_setup(solver)
    m = _ref3(u_ref)
    status = load_library().set_u_ref(_dp(m), m.shape[0], m.shape[1], 1 if verbose else 0)
    if status != 0:
        raise TinyMPCError(f"Failed to set input reference ({_err()})")
    return status


def solve(solver, *, verbose=False):
    """TinyMPC.jl:143-148 — returns the status (0 converged / 1 max_iter / -1 error), never raises on it."""
    _need_setup(solver)
    return int(load_library().solve_mpc(1 if verbose else 0))


def get_solution(solver):
    """TinyMPC.jl:150-177.  Returns dict(states=(nx,N[,B]), controls=(nu,N-1[,B]))."""
    _need_setup(solver)
    lib = load_library()
    nx, nu, N, B = solver.nx, solver.nu, solver.N, solver.batch
    sb = np.zeros(nx * N * B)
    cb = np.zeros(nu * (N - 1) * B)
    sr, sc, cr, cc = c_int(), c_int(), c_int(), c_int()
    s1 = lib.get_states(_dp(sb), ctypes.byref(sr), ctypes.byref(sc))
    s2 = lib.get_controls(_dp(cb), ctypes.byref(cr), ctypes.byref(cc))
    if s1 != 0 or s2 != 0:
        raise TinyMPCError(f"Failed to get solution ({_err()})")
    states = sb[: sr.value * sc.value].reshape((sr.value, sc.value), order="F")
    controls = cb[: cr.value * cc.value].reshape((cr.value, cc.value), order="F")
    if B > 1:
        states = states.reshape((nx, N, B), order="F")
        controls = controls.reshape((nu, N - 1, B), order="F")
    return dict(states=states, controls=controls)


def get_status(solver):
    """Batched solution->iter / solved / residuals (extension; types.hpp:32-37,128-131)."""
    _need_setup(solver)
    B = solver.batch
    it = np.zeros(B, dtype=np.int32)
    so = np.zeros(B, dtype=np.int32)
    res = np.zeros((B, 4))
    if load_library().get_status(it.ctypes.data_as(c_ip), so.ctypes.data_as(c_ip), _dp(res)) != 0:
        raise TinyMPCError(f"Failed to get status ({_err()})")
    return dict(iter=it, solved=so, residuals=res)


def set_ref_sequence(solver, x_ref_seq, u_ref_seq):
    """shared references of every step of the next closed loops, (nx, N, steps) / (nu, N-1, steps).  Supported wherever
    mpc_rollout is (see BatchSolver.set_ref_sequence); replaces a reference trajectory (set_ref_trajectory, which serves windows of
    ONE trajectory, per instance too, without the N-fold blow-up); not on a sharded solver"""
    _need_setup(solver)
    xs = np.asfortranarray(np.asarray(x_ref_seq, dtype=np.float64))
    us = np.asfortranarray(np.asarray(u_ref_seq, dtype=np.float64))
    steps = xs.shape[2]
    xs, us = xs.reshape(-1, order="F"), us.reshape(-1, order="F")
    if load_library().set_ref_sequence(_dp(xs), solver.nx, solver.N * steps, _dp(us), solver.nu, (solver.N - 1) * steps, steps) != 0:
        raise TinyMPCError(f"Failed to set the reference sequence ({_err()})")


def _flat_f(a):
    return np.ascontiguousarray(np.asfortranarray(np.asarray(a, dtype=np.float64)).reshape(-1, order="F"))


def set_plant(solver, A, B, f=None):
    """the plant the global solver's mpc_rollout steps when it is not the model (see BatchSolver.set_plant): (nx, nx) / (nx, nu) /
    (nx,) shared, or (nx, nx, B) / (nx, nu, B) / (nx, B) per instance; None, None drops it.  The library checks the shapes;
    not on a set_gpus solver"""
    _need_setup(solver)
    lib = load_library()
    if A is None and B is None:
        rc = lib.set_plant(None, 0, 0, None, 0, 0, None, 0, 0)
    else:
        A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        per = 1 if A.ndim == 3 else 0
        Af, Bf = _flat_f(A), _flat_f(B)
        ff = None if f is None else _flat_f(f)
        rc = lib.set_plant(_dp(Af), A.shape[0], Af.size // max(1, A.shape[0]), _dp(Bf), B.shape[0], Bf.size // max(1, B.shape[0]),
                           None if ff is None else _dp(ff), 0 if ff is None else ff.size, per)
    if rc != 0:
        raise TinyMPCError(f"Failed to set the plant ({_err()})")


def set_disturbance(solver, w):
    """additive disturbance of every step of the global solver's next closed loops: (nx, steps) shared or (nx, steps, B); None
    drops it (see BatchSolver.set_disturbance).  Not on a set_gpus solver"""
    _need_setup(solver)
    lib = load_library()
    if w is None:
        rc = lib.set_disturbance(None, 0, 0, 0)
    else:
        w = np.asarray(w, dtype=np.float64)
        wf = _flat_f(w)
        rc = lib.set_disturbance(_dp(wf), w.shape[0], wf.size // max(1, w.shape[0]), 1 if w.ndim == 3 else 0)
    if rc != 0:
        raise TinyMPCError(f"Failed to set the disturbance ({_err()})")


def plant_mode(solver):
    """0 model, 1 shared plant, 2 per-instance plant; | 4 shared disturbance, | 8 per-instance disturbance"""
    _need_setup(solver)
    m = int(load_library().plant_mode())
    if m < 0:
        raise TinyMPCError(f"plant_mode failed ({_err()})")
    return m


NOISE_PROCESS, NOISE_MEASUREMENT = 0, 1


def _noise_factor(G, what):
    """(flat column-major G, rows, columns, per_instance) of a noise factor: (nx, nx), (nx, nx, B), or (nx,) = diag(sigma)"""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim == 1:
        G = np.diag(G)
    if G.ndim not in (2, 3) or G.shape[0] < 1 or G.shape[0] != G.shape[1]:
        raise TinyMPCError(f"{what}: expected G (nx, nx), (nx, nx, batch) or sigma (nx,) for diag(sigma); got {G.shape}")
    Gf = _flat_f(G)
    return Gf, G.shape[0], Gf.size // G.shape[0], 1 if G.ndim == 3 else 0


def _set_noise_global(solver, which, G, seed):
    _need_setup(solver)
    lib = load_library()
    name = "set_process_noise" if which == NOISE_PROCESS else "set_measurement_noise"
    fn = getattr(lib, name)
    if G is None:
        rc = fn(None, 0, 0, 0, 0)
    else:
        Gf, rows, cols, per = _noise_factor(G, name)
        rc = fn(_dp(Gf), rows, cols, per, int(seed) & 0xFFFFFFFFFFFFFFFF)
    if rc != 0:
        raise TinyMPCError(f"{name} failed ({_err()})")


def set_process_noise(solver, G, seed=0):
    """seeded process noise of the global solver's closed loops, drawn on the device (see BatchSolver.set_process_noise): G (nx, nx)
    shared, (nx, nx, B) per instance, (nx,) = diag(sigma); None drops it.  Not on a set_gpus solver"""
    _set_noise_global(solver, NOISE_PROCESS, G, seed)


def set_measurement_noise(solver, G, seed=0):
    """seeded measurement noise of the global solver's closed loops (see BatchSolver.set_measurement_noise); None drops it"""
    _set_noise_global(solver, NOISE_MEASUREMENT, G, seed)


def set_noise_cursor(solver, t):
    """move the global solver's noise cursor (>= 0): the step index the next mpc_rollout's first draw carries"""
    _need_setup(solver)
    if load_library().set_noise_cursor(int(t)) != 0:
        raise TinyMPCError(f"Failed to set the noise cursor ({_err()})")


def noise_cursor(solver):
    """the global solver's noise cursor: 0 for a new solver, `steps` further on after every mpc_rollout of a solver with noise"""
    _need_setup(solver)
    c = int(load_library().noise_cursor())
    if c < 0:
        raise TinyMPCError(f"noise_cursor failed ({_err()})")
    return c


def noise_mode(solver):
    """1 shared / 2 per-instance process factor; | 4 shared / | 8 per-instance measurement factor"""
    _need_setup(solver)
    m = int(load_library().noise_mode())
    if m < 0:
        raise TinyMPCError(f"noise_mode failed ({_err()})")
    return m


def get_noise(solver, which, t0, steps):
    """the realised noise vectors G xi of the global solver's steps t0 .. t0 + steps - 1, computed on the device: (nx, steps, B)"""
    _need_setup(solver)
    buf = np.zeros(solver.nx * int(steps) * solver.batch)
    if load_library().get_noise(int(which), int(t0), int(steps), _dp(buf)) != 0:
        raise TinyMPCError(f"get_noise failed ({_err()})")
    return buf.reshape((solver.nx, int(steps), solver.batch), order="F")


def host_noise(seed, which, b, t, nx, G=None):
    """THE DRAW RULE on the host (csrc/noise.h, the text the device kernels compile; no device needed): the noise vector G xi of
    kind `which` (0 process, 1 measurement), instance b, step t — xi the nx standard normals Philox4x32-10 and Box-Muller give for
    (seed, which, b, t); G (nx, nx), or (nx,) = diag(sigma), or None = identity.  Returns (nx,) fp64."""
    out = np.zeros(int(nx))
    Gf = None
    if G is not None:
        Gf, rows, cols, per = _noise_factor(G, "host_noise")
        if rows != nx or cols != nx or per:
            raise TinyMPCError(f"host_noise: expected G ({nx}, {nx}) or sigma ({nx},); got {np.shape(G)}")
    rc = load_library().tinympc_host_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(which), int(b), int(t), int(nx), None if Gf is None else _dp(Gf), _dp(out))
    if rc != 0:
        raise TinyMPCError(f"host_noise failed ({_err()})")
    return out


def _estimator_matrices(C, L, what):
    """(flat C, flat L, ny, nx, per_instance) of an estimator: C (ny, nx) and L (nx, ny), or (ny, nx, B) and (nx, ny, B)"""
    C, L = np.asarray(C, dtype=np.float64), np.asarray(L, dtype=np.float64)
    if C.ndim not in (2, 3) or L.ndim != C.ndim or L.shape[:2] != C.shape[:2][::-1] or (C.ndim == 3 and C.shape[2] != L.shape[2]):
        raise TinyMPCError(f"{what}: expected C (ny, nx) and L (nx, ny), or (ny, nx, batch) and (nx, ny, batch); got {C.shape} and {L.shape}")
    return _flat_f(C), _flat_f(L), C.shape[0], C.shape[1], 1 if C.ndim == 3 else 0


def set_estimator(solver, C, L=None):
    """a fixed-gain state estimator for the global solver's closed loops, stepped on the device (see BatchSolver.set_estimator): C
    (ny, nx) and L (nx, ny) shared, or (ny, nx, B) and (nx, ny, B) per instance; C None drops it.  Not on a set_gpus solver"""
    _need_setup(solver)
    lib = load_library()
    if C is None and L is None:
        rc = lib.set_estimator(None, 0, 0, None, 0, 0, 0)
    elif C is None or L is None:
        raise TinyMPCError("set_estimator: expected both C (ny, nx) and L (nx, ny), or neither to drop the estimator")
    else:
        Cf, Lf, ny, nx, per = _estimator_matrices(C, L, "set_estimator")
        rc = lib.set_estimator(_dp(Cf), ny, Cf.size // ny, _dp(Lf), nx, Lf.size // nx, per)
    if rc != 0:
        raise TinyMPCError(f"set_estimator failed ({_err()})")


def set_estimator_state(solver, xhat):
    """install the global solver's estimate xhat- of the next step: (nx,) shared or (nx, B); None re-arms it at x0"""
    _need_setup(solver)
    lib = load_library()
    if xhat is None:
        rc = lib.set_estimator_state(None, 0, 0)
    else:
        xh = np.asarray(xhat, dtype=np.float64)
        xf = _flat_f(xh)
        rc = lib.set_estimator_state(_dp(xf), xh.shape[0], xf.size // max(1, xh.shape[0]))
    if rc != 0:
        raise TinyMPCError(f"set_estimator_state failed ({_err()})")


def estimator_mode(solver):
    """0: no estimator, 1: shared C and L, 2: per instance"""
    _need_setup(solver)
    m = int(load_library().estimator_mode())
    if m < 0:
        raise TinyMPCError(f"estimator_mode failed ({_err()})")
    return m


def get_estimator_state(solver):
    """the global solver's current estimate xhat- of the next step, (nx, B) fp64"""
    _need_setup(solver)
    buf = np.zeros(solver.nx * solver.batch)
    if load_library().get_estimator_state(_dp(buf)) != 0:
        raise TinyMPCError(f"get_estimator_state failed ({_err()})")
    return buf.reshape((solver.nx, solver.batch), order="F")


def host_estimator_step(xhat, A=None, B=None, f=None, u=None, C=None, L=None, x=None, v=None, predict=True, correct=True):
    """THE ESTIMATOR'S RULE on the host (csrc/estimator.h, the text the device kernel compiles; no device needed), one step for one
    instance or a batch of them: predict xhat- = f + A xhat + B u with the model (A (nx, nx), B (nx, nu), f (nx,) or None, u (nu,)) and /
    or correct xhat = xhat- + L (y - C xhat-), y = C x + v (C (ny, nx), L (nx, ny), the true state x, v (ny,) or None); with both the
    predict first, as the fused kernel.  xhat (nx,), or (nx, n) with u (nu, n), x (nx, n), v (ny, n) and matrices shared or with a
    trailing axis n.  Returns (xhat, y): shaped as the input, y (ny,) / (ny, n), None without the correct."""
    lib = load_library()
    xh = np.array(xhat, dtype=np.float64)
    single = xh.ndim == 1
    xh2 = xh.reshape(xh.shape[0], -1)
    nx, n = xh2.shape
    if predict and (A is None or B is None or u is None):
        raise TinyMPCError("host_estimator_step: the predict needs A, B and u")
    if correct and (C is None or L is None or x is None):
        raise TinyMPCError("host_estimator_step: the correct needs C, L and the true state x")

    def inst(M, b, nd):
        """instance b's slice of an array that is shared (nd axes) or carries a trailing axis, flat column-major"""
        if M is None:
            return None
        M = np.asarray(M, dtype=np.float64)
        return _flat_f(M[..., b] if M.ndim == nd + 1 else M)

    nu = np.asarray(B).shape[1] if B is not None else 1
    ny = np.asarray(C).shape[0] if C is not None else 1
    out, ys = np.zeros((nx, n)), np.zeros((ny, n))
    for b in range(n):
        xb, yb = np.ascontiguousarray(xh2[:, b]), np.zeros(ny)
        args = [inst(A, b, 2), inst(B, b, 2), inst(f, b, 1), inst(C, b, 2), inst(L, b, 2), inst(u, b, 1), inst(x, b, 1), inst(v, b, 1)]
        rc = lib.tinympc_host_estimator_step(nx, nu, ny, int(bool(predict)), int(bool(correct)),
                                             *[None if a is None else _dp(a) for a in args], _dp(xb), _dp(yb))
        if rc != 0:
            raise TinyMPCError(f"host_estimator_step failed ({_err()})")
        out[:, b], ys[:, b] = xb, yb
    if single:
        return out[:, 0], (ys[:, 0] if correct else None)
    return out, (ys if correct else None)


def host_kalman_gain(A, C, W, V):
    """the steady-state gain of the filter Riccati recursion P <- A (P - P C' (C P C' + V)^-1 C P) A' + W from P = W (host only,
    csrc/estimator.h): (L (nx, ny) = P C' (C P C' + V)^-1, P (nx, nx)).  TinyMPCError: an undetectable pair, a V that is not positive
    definite"""
    A, C, W, V = (np.asarray(M, dtype=np.float64) for M in (A, C, W, V))
    nx, ny = A.shape[0], C.shape[0]
    if A.shape != (nx, nx) or C.shape != (ny, nx) or W.shape != (nx, nx) or V.shape != (ny, ny):
        raise TinyMPCError(f"host_kalman_gain: expected A (nx, nx), C (ny, nx), W (nx, nx), V (ny, ny); got {A.shape}, {C.shape}, {W.shape}, {V.shape}")
    L, P = np.zeros(nx * ny), np.zeros(nx * nx)
    if load_library().tinympc_host_kalman_gain(_dp(_flat_f(A)), _dp(_flat_f(C)), _dp(_flat_f(W)), _dp(_flat_f(V)), nx, ny, _dp(L), _dp(P)) != 0:
        raise TinyMPCError(f"host_kalman_gain failed ({_err()})")
    return L.reshape((nx, ny), order="F"), P.reshape((nx, nx), order="F")


def kalman_gain(A, C, Gw, Gv):
    """the steady-state Kalman gain L (nx, ny) of the model (A, C) under the noise factors of set_process_noise / set_measurement_noise:
    W = Gw Gw', V = Gv[:ny] Gv[:ny]' — the covariance of the first ny rows of G_v xi_v, the estimator's output noise; Gw, Gv (nx, nx) or
    (nx,) = diag(sigma)"""
    C = np.asarray(C, dtype=np.float64)
    Gw, Gv = (np.diag(G) if np.ndim(G) == 1 else np.asarray(G, dtype=np.float64) for G in (Gw, Gv))
    ny = C.shape[0]
    return host_kalman_gain(A, C, Gw @ Gw.T, Gv[:ny] @ Gv[:ny].T)[0]


METRIC_NAMES = ("steps", "cost_x", "cost_u", "peak_err", "final_err", "x_viol_max", "x_viol_steps", "first_viol", "u_sat_steps",
                "iters", "maxiter_steps")
METRIC_COUNT = len(METRIC_NAMES)
SUMMARY_NAMES = ("sum", "min", "max", "count")


def _metric_vec(v, n, what):
    """a weight / limit array of n doubles, or None"""
    if v is None:
        return None
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if a.size != n:
        raise TinyMPCError(f"{what}: expected {n} values, got {a.size}")
    return a


def _metric_config(nx, nu, qw, rw, x_lo, x_hi, u_lo, u_hi, what):
    vecs = [_metric_vec(v, n, f"{what}: {name}") for v, n, name in ((qw, nx, "qw"), (rw, nu, "rw"), (x_lo, nx, "x_lo"), (x_hi, nx, "x_hi"),
                                                                   (u_lo, nu, "u_lo"), (u_hi, nu, "u_hi"))]
    return vecs, [None if v is None else _dp(v) for v in vecs]


def summary_dict(summary):
    """the (11, 4) batch summary as {slot name: {"sum", "min", "max", "count"}}"""
    s = np.asarray(summary, dtype=np.float64).reshape(METRIC_COUNT, 4)
    return {name: dict(zip(SUMMARY_NAMES, (float(x) for x in s[k]))) for k, name in enumerate(METRIC_NAMES)}


def set_rollout_metrics(solver, enable=True, qw=None, rw=None, x_lo=None, x_hi=None, u_lo=None, u_hi=None):
    """per-instance metrics of the global solver's closed loops, folded on the device (see BatchSolver.set_rollout_metrics);
    enable=False drops them.  Not on a set_gpus solver"""
    _need_setup(solver)
    vecs, p = _metric_config(solver.nx, solver.nu, qw, rw, x_lo, x_hi, u_lo, u_hi, "set_rollout_metrics")
    rc = load_library().set_rollout_metrics(1 if enable else 0, p[0], 0 if vecs[0] is None else vecs[0].size, p[1],
                                            0 if vecs[1] is None else vecs[1].size, p[2], p[3], p[4], p[5])
    if rc != 0:
        raise TinyMPCError(f"set_rollout_metrics failed ({_err()})")


def reset_rollout_metrics(solver):
    """the global solver's metric accumulators to zero, the configuration kept"""
    _need_setup(solver)
    if load_library().reset_rollout_metrics() != 0:
        raise TinyMPCError(f"reset_rollout_metrics failed ({_err()})")


def get_rollout_metrics(solver):
    """the global solver's per-instance metrics, (B, 11) fp64, columns in METRIC_NAMES' order"""
    _need_setup(solver)
    buf = np.zeros((solver.batch, METRIC_COUNT))
    if load_library().get_rollout_metrics(_dp(buf)) != 0:
        raise TinyMPCError(f"get_rollout_metrics failed ({_err()})")
    return buf


def get_rollout_summary(solver, as_dict=False):
    """the global solver's batch summary, (11, 4) fp64: per slot the sum, minimum, maximum and number of instances > 0"""
    _need_setup(solver)
    buf = np.zeros((METRIC_COUNT, 4))
    if load_library().get_rollout_summary(_dp(buf)) != 0:
        raise TinyMPCError(f"get_rollout_summary failed ({_err()})")
    return summary_dict(buf) if as_dict else buf


def host_rollout_metrics(x_log, u_log, iter_log, qw, rw, xr=None, ur=None, x_lo=None, x_hi=None, u_lo=None, u_hi=None, acc=None):
    """THE METRIC RULE on the host (csrc/metrics.h, the text the device kernel compiles; no device needed): one instance's log —
    x_log (steps, nx), u_log (steps, nu), iter_log (steps,), the targets xr (steps, nx) / ur (steps, nu) or None = zero, all taken
    as float32 / int32 — folded step after step into the 11 slots.  acc: the slots an earlier call returned, to continue them.
    Returns (11,) fp64."""
    x = np.ascontiguousarray(x_log, dtype=np.float32)
    u = np.ascontiguousarray(u_log, dtype=np.float32)
    it = np.ascontiguousarray(iter_log, dtype=np.int32).reshape(-1)
    steps = it.size
    if x.ndim != 2 or u.ndim != 2 or x.shape[0] != steps or u.shape[0] != steps:
        raise TinyMPCError(f"host_rollout_metrics: expected x_log (steps, nx), u_log (steps, nu), iter_log (steps,); got {x.shape}, {u.shape}, {it.shape}")
    nx, nu = x.shape[1], u.shape[1]
    xr = None if xr is None else np.ascontiguousarray(xr, dtype=np.float32)
    ur = None if ur is None else np.ascontiguousarray(ur, dtype=np.float32)
    if (xr is not None and xr.shape != x.shape) or (ur is not None and ur.shape != u.shape):
        raise TinyMPCError("host_rollout_metrics: the targets have the logs' shapes")
    vecs, p = _metric_config(nx, nu, qw, rw, x_lo, x_hi, u_lo, u_hi, "host_rollout_metrics")
    out = np.zeros(METRIC_COUNT) if acc is None else np.array(acc, dtype=np.float64).reshape(METRIC_COUNT).copy()
    rc = load_library().tinympc_host_rollout_metrics(nx, nu, steps, x.ctypes.data_as(c_fp), u.ctypes.data_as(c_fp), it.ctypes.data_as(c_ip),
                                                     None if xr is None else xr.ctypes.data_as(c_fp), None if ur is None else ur.ctypes.data_as(c_fp),
                                                     p[0], p[1], p[2], p[3], p[4], p[5], _dp(out))
    if rc != 0:
        raise TinyMPCError(f"host_rollout_metrics failed ({_err()})")
    return out


def ref_window(traj, cursor, knots):
    """THE WINDOW RULE of a reference trajectory, in numpy: the references of a solve with the cursor at `cursor` are the `knots`
    rows  traj[min(cursor + k, L - 1)], k = 0 .. knots-1  — a sliding window, the last row held beyond the end, so any L >= 1
    serves any cursor.  traj is (rows, L) or (rows, L, B) (rows: nx with knots = N for x_ref, nu with knots = N - 1 for u_ref);
    returns (rows, knots) or (rows, knots, B), a copy, in traj's dtype: what set_x_ref / set_u_ref take, and what the library's
    window kernel writes on the device (there in the fp32 rounding set_ref_trajectory made)."""
    traj = np.asarray(traj)
    if traj.ndim not in (2, 3) or traj.shape[1] < 1 or cursor < 0 or knots < 0:
        raise ValueError(f"ref_window: expected traj (rows, L) or (rows, L, B) with L >= 1, cursor >= 0, knots >= 0; got {traj.shape}, {cursor}, {knots}")
    rows = np.minimum(int(cursor) + np.arange(int(knots)), traj.shape[1] - 1)
    return np.array(traj[:, rows], order="F")


def _traj_args(x_traj, u_traj):
    """(x flat, x rows, x cols, u flat | None, u rows, u cols, per_instance) of a trajectory pair, the batch on the columns"""
    x = np.asarray(x_traj, dtype=np.float64)
    u = None if u_traj is None else np.asarray(u_traj, dtype=np.float64)
    if x.ndim not in (2, 3) or (u is not None and u.ndim not in (2, 3)):
        raise TinyMPCError("set_ref_trajectory: expected x_traj (nx, Lx) or (nx, Lx, batch), u_traj (nu, Lu) or (nu, Lu, batch)")
    if u is not None and u.ndim != x.ndim:
        raise TinyMPCError(f"set_ref_trajectory: x_traj and u_traj are both shared or both per instance; got x_traj {x.shape}, u_traj {u.shape} "
                           "(a shared one beside a per-instance one: tile it over the batch)")
    xf, uf = _flat_f(x), None if u is None else _flat_f(u)
    return (xf, x.shape[0], xf.size // max(1, x.shape[0]), uf, 0 if u is None else u.shape[0],
            0 if u is None else uf.size // max(1, u.shape[0]), 1 if x.ndim == 3 else 0)


def set_ref_trajectory(solver, x_traj, u_traj=None, *, verbose=False):
    """a reference trajectory for the global solver, windowed on the device (see BatchSolver.set_ref_trajectory): x_traj (nx, Lx)
    and u_traj (nu, Lu) shared, or (nx, Lx, B) and (nu, Lu, B) per instance; u_traj None: zero input references; x_traj None drops
    it.  The library checks row counts and widths; not on a set_gpus solver"""
    _need_setup(solver)
    lib = load_library()
    if x_traj is None:
        rc = lib.set_ref_trajectory(None, 0, 0, None, 0, 0, 0, 1 if verbose else 0)
    else:
        xf, xr, xc, uf, ur, uc, per = _traj_args(x_traj, u_traj)
        rc = lib.set_ref_trajectory(_dp(xf), xr, xc, None if uf is None else _dp(uf), ur, uc, per, 1 if verbose else 0)
    if rc != 0:
        raise TinyMPCError(f"Failed to set the reference trajectory ({_err()})")


def set_ref_cursor(solver, cursor):
    """move the global solver's reference cursor (>= 0): the next solve reads the window there, the next mpc_rollout starts there"""
    _need_setup(solver)
    if load_library().set_ref_cursor(int(cursor)) != 0:
        raise TinyMPCError(f"Failed to set the reference cursor ({_err()})")


def ref_cursor(solver):
    """the global solver's reference cursor: 0 for a new trajectory, `steps` further on after every mpc_rollout"""
    _need_setup(solver)
    c = int(load_library().ref_cursor())
    if c < 0:
        raise TinyMPCError(f"ref_cursor failed ({_err()})")
    return c


def mpc_rollout(solver, steps):
    """`steps` closed-loop steps on the global solver — solve, then the plant step x+ = f + A x + B u0 of the model, or of the plant
    set_plant installed, plus the disturbance of set_disturbance; with set_ref_trajectory every step against its own window of the
    trajectory, the cursor left `steps` further on; with set_process_noise / set_measurement_noise under noise drawn on the device:
    dict(status, x (nx, steps, B), u (nu, steps, B), iter, solved), and y (nx, steps, B) — what every step's solve started from —
    only while measurement noise is installed"""
    _need_setup(solver)
    nx, nu, B = solver.nx, solver.nu, solver.batch
    x, u = np.zeros(nx * steps * B), np.zeros(nu * steps * B)
    it = np.zeros(steps * B, dtype=np.int32)
    lib = load_library()
    st = int(lib.mpc_rollout(int(steps), _dp(x), _dp(u), it.ctypes.data_as(c_ip)))
    if st < 0:
        raise TinyMPCError(f"mpc_rollout failed ({_err()})")
    it = it.reshape((steps, B), order="F")
    out = dict(status=st, x=x.reshape((nx, steps, B), order="F"), u=u.reshape((nu, steps, B), order="F"),
               iter=np.abs(it), solved=(it > 0).astype(np.int32))
    if int(lib.estimator_mode()) > 0:
        ny = int(lib.estimator_outputs())
        xh, yo = np.zeros(nx * steps * B), np.zeros(ny * steps * B)
        if lib.get_mpc_estimate(_dp(xh)) != 0 or lib.get_mpc_outputs(_dp(yo)) != 0:
            raise TinyMPCError(f"get_mpc_estimate / get_mpc_outputs failed ({_err()})")
        out["xhat"], out["yout"] = xh.reshape((nx, steps, B), order="F"), yo.reshape((ny, steps, B), order="F")
    elif max(0, int(lib.noise_mode())) & 12:
        y = np.zeros(nx * steps * B)
        if lib.get_mpc_measured(_dp(y)) != 0:
            raise TinyMPCError(f"get_mpc_measured failed ({_err()})")
        out["y"] = y.reshape((nx, steps, B), order="F")
    return out


def reset_workspace(solver):
    _need_setup(solver)
    if load_library().reset_workspace() != 0:
        raise TinyMPCError(f"Failed to reset workspace ({_err()})")
    return 0


def update_settings(solver, *, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100,
                    check_termination=True, en_state_bound=False, en_input_bound=False,
                    en_state_soc=False, en_input_soc=False, en_state_linear=False,
                    en_input_linear=False, adaptive_rho=False, adaptive_rho_min=0.1,
                    adaptive_rho_max=10.0, adaptive_rho_enable_clipping=True, verbose=False):
    """TinyMPC.jl:181-211 — every field is sent with its keyword default, like the reference
    (so calling it later resets en_*_bound to false and the tolerances to 1e-3).
    `check_termination` may also be an int interval (extension); True/False map to 1/0."""
    ct = int(check_termination) if not isinstance(check_termination, bool) else (1 if check_termination else 0)
    status = load_library().update_settings(
        float(abs_pri_tol), float(abs_dua_tol), int(max_iter), ct, int(bool(en_state_bound)),
        int(bool(en_input_bound)), int(bool(en_state_soc)), int(bool(en_input_soc)),
        int(bool(en_state_linear)), int(bool(en_input_linear)), int(bool(adaptive_rho)),
        float(adaptive_rho_min), float(adaptive_rho_max), int(bool(adaptive_rho_enable_clipping)),
        1 if verbose else 0)
    if status != 0:
        raise TinyMPCError(f"Failed to update settings ({_err()})")
    return status


def _instance_bounds(x_min, x_max, u_min, u_max):
    """the four arrays of set_instance_bounds in the library's instance-major layout, and whether they are per knot:
    (nx, B) / (nu, B) constant over the horizon, or (nx, N, B) / (nu, N-1, B)"""
    arrs = [np.asarray(a, dtype=np.float64) for a in (x_min, x_max, u_min, u_max)]
    nd = {a.ndim for a in arrs}
    if nd not in ({2}, {3}):
        raise TinyMPCError("set_instance_bounds: the four arrays must all be (rows, batch) or all (rows, knots, batch)")
    return [np.ascontiguousarray(np.asfortranarray(a).reshape(-1, order="F")) for a in arrs], nd == {3}


def set_bound_constraints(solver, x_min, x_max, u_min, u_max, *, verbose=False):
    """TinyMPC.jl:214-227; both bound flags are auto-enabled in the library (bindings.cpp:400-404).  (nx, N) / (nu, N-1)
    shared by the batch, or — batch > 1 — (nx, N, batch) / (nu, N-1, batch): every instance its own bounds at every knot."""
    ms = [_ref3(m) for m in (x_min, x_max, u_min, u_max)]
    args = []
    for m in ms:
        args += [_dp(m), m.shape[0], m.shape[1]]
    status = load_library().set_bound_constraints(*args, 1 if verbose else 0)
    if status != 0:
        raise TinyMPCError(f"Failed to set bound constraints ({_err()})")
    return status


def _lin_block(A, b, n):
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))
    A = np.asarray(A, dtype=np.float64)
    A = _mat(A.reshape(len(b), n) if len(b) else np.zeros((0, n)))
    return A, b


def _instance_linear(A, b, n, batch):
    """one side of set_instance_linear, (rows, n, B) with (rows, B), in the library's layout: [B] blocks of rows x n,
    column-major, and [B][rows]; an empty side (None, or zero rows) gives 0 rows"""
    if A is None or np.asarray(A).size == 0:
        return np.zeros(0), np.zeros(0), 0
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if A.ndim != 3 or b.ndim != 2 or A.shape[1:] != (n, batch) or b.shape != (A.shape[0], batch):
        raise TinyMPCError(f"set_instance_linear: expected (rows, {n}, {batch}) with (rows, {batch})")
    return (np.ascontiguousarray(np.asfortranarray(A).reshape(-1, order="F")),
            np.ascontiguousarray(np.asfortranarray(b).reshape(-1, order="F")), A.shape[0])


def set_linear_constraints(solver, Alin_x, blin_x, Alin_u, blin_u, *, verbose=False):
    """TinyMPC.jl:229-243: Alin_x x <= blin_x, Alin_u u <= blin_u at every knot; parity unpinned.  (rows, nx)
    with (rows,) shared by the batch, or — batch > 1 — (rows, nx, batch) with (rows, batch): every instance its own rows
    (an all-zero row is a row that instance does not have); the input side alike."""
    _need_setup(solver)
    def side(A, b, n):     # a 3-D side travels with the batch on its width; the library refuses mixed widths by name
        if A is not None and np.asarray(A).ndim == 3:
            A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
            return (_mat(np.asfortranarray(A).reshape(A.shape[0], -1, order="F")),
                    np.ascontiguousarray(np.asfortranarray(b).reshape(-1, order="F")))
        return _lin_block(np.zeros((0, n)) if A is None else A, [] if b is None else b, n)
    Ax, bx = side(Alin_x, blin_x, solver.nx)
    Au, bu = side(Alin_u, blin_u, solver.nu)
    status = load_library().set_linear_constraints(_dp(Ax), Ax.shape[0], Ax.shape[1], _dp(bx), len(bx),
                                                   _dp(Au), Au.shape[0], Au.shape[1], _dp(bu), len(bu),
                                                   1 if verbose else 0)
    if status != 0:
        raise TinyMPCError(f"Failed to set linear constraints ({_err()})")
    return status


def set_equality_constraints(solver, Aeq_x, beq_x, Aeq_u=None, beq_u=None):
    """TinyMPC.jl:261-270: equalities as two inequalities each"""
    _need_setup(solver)
    Ax, bx = _lin_block(Aeq_x, beq_x, solver.nx)
    Au, bu = _lin_block(np.zeros((0, solver.nu)) if Aeq_u is None else Aeq_u, [] if beq_u is None else beq_u,
                        solver.nu)
    return set_linear_constraints(solver, np.vstack([Ax, -Ax]), np.concatenate([bx, -bx]),
                                  np.vstack([Au, -Au]), np.concatenate([bu, -bu]))


def _instance_cones(Ac, qc, c, batch):
    """one side of set_instance_cones: the layout (n,) and the coefficients (n, B), in the library's layout [B][n]; an empty
    side (None, or no cone) gives 0 cones"""
    if Ac is None or np.asarray(Ac).size == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), 0
    Ac = np.ascontiguousarray(np.asarray(Ac, dtype=np.int32).ravel())
    qc = np.ascontiguousarray(np.asarray(qc, dtype=np.int32).ravel())
    c = np.asarray(c, dtype=np.float64)
    if len(qc) != len(Ac) or c.shape != (len(Ac), batch):
        raise TinyMPCError(f"set_instance_cones: expected Ac, qc of one length n and coefficients ({len(Ac)}, {batch})")
    return Ac, qc, np.ascontiguousarray(c.T).reshape(-1), len(Ac)


def set_cone_constraints(solver, Acu, qcu, cu, Acx, qcx, cx, *, verbose=False):
    """TinyMPC.jl:245-259.  Per-knot second-order cones, inputs first; parity unpinned.  cu (n,) and cx (n,)
    shared by the batch, or — batch > 1 — cu (n, batch) and cx (n, batch): every instance its own coefficients over the one
    layout (+inf: a cone that instance does not have)."""
    ia = [np.asarray(a, dtype=np.int32) for a in (Acu, qcu, Acx, qcx)]
    # a 2-D side travels with the batch on its width, [batch][cone]; the library refuses mixed widths by name
    da = [np.ascontiguousarray(a.T).reshape(-1) if a.ndim == 2 else a for a in (np.asarray(a, dtype=np.float64) for a in (cu, cx))]
    status = load_library().set_cone_constraints(
        ia[0].ctypes.data_as(c_ip), len(ia[0]), ia[1].ctypes.data_as(c_ip), len(ia[1]), _dp(da[0]),
        len(da[0]), ia[2].ctypes.data_as(c_ip), len(ia[2]), ia[3].ctypes.data_as(c_ip), len(ia[3]),
        _dp(da[1]), len(da[1]), 1 if verbose else 0)
    if status != 0:
        raise TinyMPCError(f"Failed to set cone constraints ({_err()})")
    return status


def _solve_lqr(A, B, Q, R, rho):
    """TinyMPC.jl:326-352: the rho-regularised LQR the sensitivities are differenced on (rho enters once, P0 = Q + rho I)"""
    nx, nu = A.shape[0], B.shape[1]
    Qr, Rr = Q + rho * np.eye(nx), R + rho * np.eye(nu)
    P, K = Qr.copy(), np.zeros((nu, nx))
    for it in range(1, 5001):
        Kp = K
        K = np.linalg.solve(Rr + B.T @ P @ B + 1e-8 * np.eye(nu), B.T @ P @ A)
        P = Qr + A.T @ P @ (A - B @ K)
        if it > 1 and np.linalg.norm(K - Kp) < 1e-10:
            break
    return K, P, np.linalg.inv(Rr + B.T @ P @ B), (A - B @ K).T


def compute_sensitivity_autograd(solver):
    """TinyMPC.jl:301-323: forward differences (h = 1e-6) of (Kinf, Pinf, Quu_inv, AmBKt) in rho -> (dK, dP, dC1, dC2)"""
    _need_setup(solver)
    h = 1e-6
    m0 = _solve_lqr(solver.A, solver.B, solver.Q, solver.R, solver.rho)
    m1 = _solve_lqr(solver.A, solver.B, solver.Q, solver.R, solver.rho + h)
    return tuple((b - a) / h for a, b in zip(m0, m1))


def set_sensitivity(solver, dK, dP, dC1=None, dC2=None, *, verbose=False):
    """hand the live solver the sensitivities codegen_with_sensitivity would bake in (TinyMPC.jl:374-394)"""
    _need_setup(solver)
    ms = [None if m is None else _mat(m) for m in (dK, dP, dC1, dC2)]
    args = []
    for m in ms:
        args += [None, 0, 0] if m is None else [_dp(m), m.shape[0], m.shape[1]]
    if load_library().set_sensitivity(*args, 1 if verbose else 0) != 0:
        raise TinyMPCError(f"Failed to set sensitivity matrices ({_err()})")
    return 0


def get_adaptive_rho(solver):
    """rho of each instance after adaptation, shape (batch,)"""
    _need_setup(solver)
    rho, n = np.zeros(solver.batch), ctypes.c_int()
    if load_library().get_adaptive_rho(_dp(rho), ctypes.byref(n)) != 0:
        raise TinyMPCError(f"Failed to get adaptive rho ({_err()})")
    return rho[: n.value]


def set_cache_terms(solver, Kinf, Pinf, Quu_inv, AmBKt, *, verbose=False):
    """TinyMPC.jl:278-292"""
    _need_setup(solver)
    ms = [_mat(m) for m in (Kinf, Pinf, Quu_inv, AmBKt)]
    args = []
    for m in ms:
        args += [_dp(m), m.shape[0], m.shape[1]]
    status = load_library().set_cache_terms(*args, 1 if verbose else 0)
    if status != 0:
        raise TinyMPCError(f"Failed to set cache terms ({_err()})")
    return status


def print_problem_data(solver, *, verbose=False):
    _need_setup(solver)
    return load_library().print_problem_data(1 if verbose else 0)


def cleanup():
    """TinyMPC.jl:428-429"""
    try:
        load_library().cleanup_solver()
    except Exception:
        pass


def host_sensitivity(A, B, Q, R, rho):
    """the library's host finite differences (dK, dP, dC1, dC2) without a GPU (TinyMPC.jl:301-352 semantics)"""
    A, B, Q, R = _mat(A), _mat(B), _mat(Q), _mat(R)
    nx, nu = A.shape[0], B.shape[1]
    dK, dP = np.zeros((nu, nx), order="F"), np.zeros((nx, nx), order="F")
    d1, d2 = np.zeros((nu, nu), order="F"), np.zeros((nx, nx), order="F")
    if load_library().tinympc_host_sensitivity(_dp(A), _dp(B), _dp(Q), _dp(R), float(rho), nx, nu, _dp(dK), _dp(dP),
                                               _dp(d1), _dp(d2)) != 0:
        raise TinyMPCError(f"host_sensitivity failed ({_err()})")
    return dK, dP, d1, d2


def host_precompute(A, B, Q, R, rho):
    """fp64 Riccati cache on the host (no GPU needed): dict(Kinf, Pinf, Quu_inv, AmBKt)."""
    A, B, Q, R = _mat(A), _mat(B), _mat(Q), _mat(R)
    nx, nu = A.shape[0], B.shape[1]
    K, P = np.zeros((nu, nx), order="F"), np.zeros((nx, nx), order="F")
    Qi, Am = np.zeros((nu, nu), order="F"), np.zeros((nx, nx), order="F")
    if load_library().tinympc_host_precompute(_dp(A), _dp(B), _dp(Q), _dp(R), float(rho), nx, nu, _dp(K),
                                              _dp(P), _dp(Qi), _dp(Am)) != 0:
        raise TinyMPCError(f"host_precompute failed ({_err()})")
    return dict(Kinf=K, Pinf=P, Quu_inv=Qi, AmBKt=Am)


def host_precompute_sweeps(A, B, Q, R, rho):
    """the Riccati sweeps host_precompute runs for the family (1000: the cap); raises where R + B'PB is singular"""
    A, B, Q, R = _mat(A), _mat(B), _mat(Q), _mat(R)
    n = load_library().tinympc_host_precompute_sweeps(_dp(A), _dp(B), _dp(Q), _dp(R), float(rho), A.shape[0], B.shape[1])
    if n < 0:
        raise TinyMPCError(f"host_precompute_sweeps failed ({_err()})")
    return int(n)


def host_family_cache(A, B, Q, R, rho):
    """the same cache by the rule the device setup of per-instance families runs (csrc/riccati.h), on the host, no GPU needed:
    dict(Kinf, Pinf, Quu_inv, AmBKt, sweeps).  Shapes of the stream kernel's grid (nx in {2,3,4,6,8,10,12}, nu <= 4); raises
    TinyMPCError where R + B'PB is singular."""
    A, B, Q, R = _mat(A), _mat(B), _mat(Q), _mat(R)
    nx, nu = A.shape[0], B.shape[1]
    K, P = np.zeros((nu, nx), order="F"), np.zeros((nx, nx), order="F")
    Qi, Am = np.zeros((nu, nu), order="F"), np.zeros((nx, nx), order="F")
    sweeps = ctypes.c_int(0)
    if load_library().tinympc_host_family_cache(_dp(A), _dp(B), _dp(Q), _dp(R), float(rho), nx, nu, _dp(K), _dp(P), _dp(Qi),
                                                _dp(Am), ctypes.byref(sweeps)) != 0:
        raise TinyMPCError(f"host_family_cache failed ({_err()})")
    return dict(Kinf=K, Pinf=P, Quu_inv=Qi, AmBKt=Am, sweeps=int(sweeps.value))


class BatchSolver:
    """Handle-API wrapper (tinympc_* in include/tinympc_hip.h): several solvers per process,
    device-resident I/O, stream-ordered solves.  Used by bench.py and the sharded driver."""

    def __init__(self, A, B, Q, R, rho, N, batch, device=-1, verbose=False):
        self.lib = load_library()
        A, B, Q, R = _mat(A), _mat(B), _mat(Q), _mat(R)
        self.nx, self.nu, self.N, self.batch = A.shape[0], B.shape[1], int(N), int(batch)
        h = c_vp()
        st = self.lib.tinympc_create(ctypes.byref(h), _dp(A), _dp(B), _dp(Q), _dp(R), float(rho), self.nx,
                                     self.nu, self.N, self.batch, int(device), 1 if verbose else 0)
        if st != 0:
            raise TinyMPCError(f"tinympc_create failed ({_err()})")
        self.h = h

    @classmethod
    def from_families(cls, A, B, Q, R, rho, N, device=-1, verbose=False, setup="host"):
        """One (A, B, Q, R, rho) family PER INSTANCE: A (nx, nx, batch), B (nx, nu, batch), Q (nx, nx, batch),
        R (nu, nu, batch), rho (batch,).  Each instance gets its own fp64 Riccati cache: computed on the host (setup="host",
        the default) or by a kernel on the device (setup="device": the same recursion, and the coefficient pack is written
        on the device too — the route for large batches)."""
        if setup not in ("host", "device"):
            raise TinyMPCError('from_families: setup is "host" or "device"')
        self = cls.__new__(cls)
        self.lib = load_library()
        A, B, Q, R = (np.asfortranarray(np.asarray(m, dtype=np.float64)) for m in (A, B, Q, R))
        rho = np.ascontiguousarray(np.asarray(rho, dtype=np.float64))
        self.nx, self.nu, self.N, self.batch = A.shape[0], B.shape[1], int(N), A.shape[2]
        h = c_vp()
        create = self.lib.tinympc_create_families_device if setup == "device" else self.lib.tinympc_create_families
        st = create(ctypes.byref(h), _dp(A), _dp(B), _dp(Q), _dp(R), _dp(rho), self.nx,
                    self.nu, self.N, self.batch, int(device), 1 if verbose else 0)
        if st != 0:
            raise TinyMPCError(f"tinympc_create_families{'_device' if setup == 'device' else ''} failed ({_err()})")
        self.h = h
        return self

    def set_families(self, A=None, B=None, Q=None, R=None, rho=None):
        """replaces EVERY instance's family on a family solver (either setup mode), arrays as from_families takes them; A and B
        come together, so do Q and R; what is None is kept.  The caches are recomputed on the device (the solver is in device
        mode afterwards); settings, bounds, rows, cones, the affine term, references, the closed loop's configuration and the
        warm-start workspace are kept.  Raises, the solver unchanged, if some instance's R + B'PB is singular."""
        if (A is None) != (B is None) or (Q is None) != (R is None):
            raise TinyMPCError("set_families: A and B come together, and so do Q and R")
        want = dict(A=(self.nx, self.nx), B=(self.nx, self.nu), Q=(self.nx, self.nx), R=(self.nu, self.nu))
        arrs = {}
        for name, m in (("A", A), ("B", B), ("Q", Q), ("R", R)):
            if m is None:
                arrs[name] = None
                continue
            m = np.asfortranarray(np.asarray(m, dtype=np.float64))
            if m.shape != want[name] + (self.batch,):
                raise TinyMPCError(f"set_families: {name} must be {want[name] + (self.batch,)}, got {m.shape}")
            arrs[name] = m
        if rho is not None:
            rho = np.ascontiguousarray(np.asarray(rho, dtype=np.float64).reshape(-1))
            if rho.size != self.batch:
                raise TinyMPCError("set_families: rho must have one entry per instance")
        self._chk(self.lib.tinympc_set_families(self.h, *[None if arrs[k] is None else _dp(arrs[k]) for k in "ABQR"],
                                                None if rho is None else _dp(rho)), "set_families")

    def family_cache(self, first=0, count=None, sweeps_only=False):
        """the Riccati caches of instances [first, first + count) of a family solver, in either setup mode: dict(Kinf (nu, nx, n),
        Pinf (nx, nx, n), Quu_inv (nu, nu, n), AmBKt (nx, nx, n), sweeps (n,) — 1000: the instance stopped at the cap);
        sweeps_only: the sweep counts alone (no matrix is copied)"""
        n = self.batch - int(first) if count is None else int(count)
        if sweeps_only:
            sw = np.zeros(n, dtype=np.int32)
            self._chk(self.lib.tinympc_get_family_cache(self.h, int(first), n, None, None, None, None, sw.ctypes.data_as(c_ip)), "family_cache")
            return dict(sweeps=sw)
        K, P = np.zeros((self.nu, self.nx, n), order="F"), np.zeros((self.nx, self.nx, n), order="F")
        Qi, Am = np.zeros((self.nu, self.nu, n), order="F"), np.zeros((self.nx, self.nx, n), order="F")
        sw = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.tinympc_get_family_cache(self.h, int(first), n, _dp(K), _dp(P), _dp(Qi), _dp(Am),
                                                    sw.ctypes.data_as(c_ip)), "family_cache")
        return dict(Kinf=K, Pinf=P, Quu_inv=Qi, AmBKt=Am, sweeps=sw)

    @property
    def families_setup_mode(self):
        """0 not a family solver, 1 families set up on the host, 2 on the device"""
        return int(self.lib.tinympc_families_setup_mode(self.h))

    def families_setup_ms(self):
        """kernel times in ms of the last device setup and the last device pack fill (-1.0: none has run)"""
        ms = np.zeros(2)
        self._chk(self.lib.tinympc_families_setup_ms(self.h, _dp(ms)), "families_setup_ms")
        return float(ms[0]), float(ms[1])

    def close(self):
        if getattr(self, "h", None):
            self.lib.tinympc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st, what):
        if st != 0:
            raise TinyMPCError(f"{what} failed ({_err()})")

    def update_settings(self, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1,
                        en_state_bound=0, en_input_bound=0):
        self._chk(self.lib.tinympc_update_settings(self.h, float(abs_pri_tol), float(abs_dua_tol),
                                                   int(max_iter), int(check_termination),
                                                   int(en_state_bound), int(en_input_bound)),
                  "update_settings")

    def set_bound_constraints(self, x_min, x_max, u_min, u_max):
        ms = [_mat(m) for m in (x_min, x_max, u_min, u_max)]
        self._chk(self.lib.tinympc_set_bound_constraints(self.h, *[_dp(m) for m in ms]), "set_bound_constraints")

    def set_instance_bounds(self, x_min, x_max, u_min, u_max):
        """box bounds PER INSTANCE: (nx, B) / (nu, B) constant over the horizon, or (nx, N, B) / (nu, N-1, B) per knot (the layout
        follows from the number of dimensions).  The solver then runs on the `ib` form of the stream or the generic kernel;
        set_bound_constraints returns it to shared bounds.  Not with adaptive rho; mpc_rollout only under TINYMPC_HIP_STREAM_MPC."""
        flat, per_knot = _instance_bounds(x_min, x_max, u_min, u_max)
        want = [self.nx * (self.N if per_knot else 1), self.nx * (self.N if per_knot else 1),
                self.nu * (self.N - 1 if per_knot else 1), self.nu * (self.N - 1 if per_knot else 1)]
        if [f.size for f in flat] != [w * self.batch for w in want]:
            raise TinyMPCError("set_instance_bounds: expected (nx, batch) / (nu, batch) or (nx, N, batch) / (nu, N-1, batch)")
        self._chk(self.lib.tinympc_set_instance_bounds(self.h, *[_dp(f) for f in flat], 1 if per_knot else 0), "set_instance_bounds")

    def bounds_mode(self):
        """0 shared bounds, 1 per instance and constant over the horizon, 2 per instance and per knot"""
        return int(self.lib.tinympc_bounds_mode(self.h))

    def set_cache_terms(self, Kinf, Pinf, Quu_inv, AmBKt):
        ms = [_mat(m) for m in (Kinf, Pinf, Quu_inv, AmBKt)]
        self._chk(self.lib.tinympc_set_cache_terms(self.h, *[_dp(m) for m in ms]), "set_cache_terms")

    def set_fdyn(self, fdyn):
        """affine dynamics term x+ = A x + B u + f (parity unpinned; stream / generic kernels)"""
        f = np.ascontiguousarray(np.asarray(fdyn, dtype=np.float64).reshape(-1))
        self._chk(self.lib.tinympc_set_fdyn(self.h, _dp(f)), "set_fdyn")

    def set_cone_constraints(self, Acu, qcu, cu, Acx, qcx, cx):
        """per-knot second-order cones, inputs first (TinyMPC.jl:245-259 argument order); parity unpinned"""
        ia = [np.ascontiguousarray(np.asarray(a, dtype=np.int32)) for a in (Acu, qcu, Acx, qcx)]
        da = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (cu, cx)]
        self._chk(self.lib.tinympc_set_cone_constraints(
            self.h, ia[0].ctypes.data_as(c_ip), ia[1].ctypes.data_as(c_ip), _dp(da[0]), len(da[0]),
            ia[2].ctypes.data_as(c_ip), ia[3].ctypes.data_as(c_ip), _dp(da[1]), len(da[1])), "set_cone_constraints")

    def set_linear_constraints(self, Alin_x, blin_x, Alin_u, blin_u):
        """Alin_x x <= blin_x, Alin_u u <= blin_u at every knot (TinyMPC.jl:229-243); parity unpinned"""
        Ax, bx = _lin_block(Alin_x, blin_x, self.nx)
        Au, bu = _lin_block(Alin_u, blin_u, self.nu)
        self._chk(self.lib.tinympc_set_linear_constraints(self.h, _dp(Ax), Ax.shape[0], _dp(bx), _dp(Au), Au.shape[0],
                                                          _dp(bu)), "set_linear_constraints")

    def set_instance_linear(self, Alin_x, blin_x, Alin_u, blin_u):
        """linear rows PER INSTANCE: Alin_x (rows, nx, B) with blin_x (rows, B), Alin_u (rows, nu, B) with blin_u (rows, B); an
        empty side is None or zero rows; an all-zero row of an instance is a row that instance does not have.  The solver
        then runs on the `il` form of the stream or the generic kernel; set_linear_constraints returns it to shared rows.
        Not with adaptive rho; mpc_rollout only as a chain (a plant of its own, or TINYMPC_HIP_STREAM_MPC)."""
        Ax, bx, mx = _instance_linear(Alin_x, blin_x, self.nx, self.batch)
        Au, bu, mu = _instance_linear(Alin_u, blin_u, self.nu, self.batch)
        self._chk(self.lib.tinympc_set_instance_linear(self.h, _dp(Ax) if mx else None, mx, _dp(bx) if mx else None,
                                                       _dp(Au) if mu else None, mu, _dp(bu) if mu else None), "set_instance_linear")

    def lin_mode(self):
        """0 no rows or rows shared by the batch, 1 per instance"""
        return int(self.lib.tinympc_lin_mode(self.h))

    def set_instance_cones(self, Acu, qcu, cu, Acx, qcx, cx):
        """cone coefficients PER INSTANCE over one layout: Acu, qcu (ncu,) with cu (ncu, B), Acx, qcx (ncx,) with cx (ncx, B); an
        empty side is None or no cone; +inf is a cone that instance does not have.  The solver then runs on the `ic` form of
        the stream or the generic kernel; set_cone_constraints returns it to shared cones.  Not with adaptive rho; mpc_rollout
        only as a chain (a plant of its own, or TINYMPC_HIP_STREAM_MPC)."""
        au, qu, cuv, n_u = _instance_cones(Acu, qcu, cu, self.batch)
        ax, qx, cxv, n_x = _instance_cones(Acx, qcx, cx, self.batch)
        self._chk(self.lib.tinympc_set_instance_cones(
            self.h, au.ctypes.data_as(c_ip) if n_u else None, qu.ctypes.data_as(c_ip) if n_u else None, _dp(cuv) if n_u else None, n_u,
            ax.ctypes.data_as(c_ip) if n_x else None, qx.ctypes.data_as(c_ip) if n_x else None, _dp(cxv) if n_x else None, n_x),
            "set_instance_cones")

    def enable_cones(self, en_state_soc, en_input_soc):
        """the two cone switches of update_settings (TinyMPC.jl:100-101) on their own: a side keeps its cones while it is off"""
        self._chk(self.lib.tinympc_enable_cones(self.h, int(bool(en_state_soc)), int(bool(en_input_soc))), "enable_cones")

    def cone_mode(self):
        """0 no cones or cones shared by the batch, 1 a coefficient per instance"""
        return int(self.lib.tinympc_cone_mode(self.h))

    def enable_linear(self, en_state_linear, en_input_linear):
        """the two linear-row switches of update_settings (TinyMPC.jl:98-99) on their own: a side keeps its rows while it is off"""
        self._chk(self.lib.tinympc_enable_linear(self.h, int(bool(en_state_linear)), int(bool(en_input_linear))), "enable_linear")

    def set_equality_constraints(self, Aeq_x, beq_x, Aeq_u=None, beq_u=None):
        """equalities as two inequalities each (TinyMPC.jl:261-270)"""
        Ax, bx = _lin_block(Aeq_x, beq_x, self.nx)
        Au, bu = _lin_block(np.zeros((0, self.nu)) if Aeq_u is None else Aeq_u, [] if beq_u is None else beq_u, self.nu)
        self.set_linear_constraints(np.vstack([Ax, -Ax]), np.concatenate([bx, -bx]), np.vstack([Au, -Au]),
                                    np.concatenate([bu, -bu]))

    def set_adaptive_rho(self, enable=True, rho_min=0.1, rho_max=10.0, enable_clipping=True):
        """per-instance rho adaptation every 5th iteration (admm.cpp:147-174); defaults TinyMPC.jl:59-61"""
        self._chk(self.lib.tinympc_set_adaptive_rho(self.h, int(bool(enable)), float(rho_min), float(rho_max),
                                                    int(bool(enable_clipping))), "set_adaptive_rho")

    def set_sensitivity(self, dK, dP, dC1=None, dC2=None):
        """dKinf/drho, dPinf/drho (dC1, dC2 accepted and unused, as in the reference's iteration)"""
        ms = [None if m is None else _mat(m) for m in (dK, dP, dC1, dC2)]
        self._chk(self.lib.tinympc_set_sensitivity(self.h, *[None if m is None else _dp(m) for m in ms]), "set_sensitivity")

    def compute_sensitivity(self):
        """(dK, dP, dC1, dC2) by the library's host finite differences (TinyMPC.jl:301-352)"""
        nx, nu = self.nx, self.nu
        dK, dP = np.zeros((nu, nx), order="F"), np.zeros((nx, nx), order="F")
        d1, d2 = np.zeros((nu, nu), order="F"), np.zeros((nx, nx), order="F")
        self._chk(self.lib.tinympc_compute_sensitivity(self.h, _dp(dK), _dp(dP), _dp(d1), _dp(d2)), "compute_sensitivity")
        return dK, dP, d1, d2

    def get_adaptive_state(self):
        """each instance's current rho (batch,), Kinf (nu, nx, batch), Pinf (nx, nx, batch)"""
        nx, nu, Bn = self.nx, self.nu, self.batch
        rho, K, P = np.zeros(Bn), np.zeros((nu, nx, Bn), order="F"), np.zeros((nx, nx, Bn), order="F")
        self._chk(self.lib.tinympc_get_adaptive_state(self.h, _dp(rho), _dp(K), _dp(P)), "get_adaptive_state")
        return dict(rho=rho, Kinf=K, Pinf=P)

    def get_cache_terms(self):
        nx, nu = self.nx, self.nu
        K, P = np.zeros((nu, nx), order="F"), np.zeros((nx, nx), order="F")
        Qi, Am = np.zeros((nu, nu), order="F"), np.zeros((nx, nx), order="F")
        self._chk(self.lib.tinympc_get_cache_terms(self.h, _dp(K), _dp(P), _dp(Qi), _dp(Am)), "get_cache_terms")
        return dict(Kinf=K, Pinf=P, Quu_inv=Qi, AmBKt=Am)

    def set_x0(self, x0):
        m = _mat(x0)
        self._chk(self.lib.tinympc_set_x0(self.h, _dp(m), m.shape[1]), "set_x0")

    def set_x_ref(self, x_ref):
        m = _ref3(x_ref)
        self._chk(self.lib.tinympc_set_x_ref(self.h, _dp(m), m.shape[1]), "set_x_ref")

    def set_u_ref(self, u_ref):
        m = _ref3(u_ref)
        self._chk(self.lib.tinympc_set_u_ref(self.h, _dp(m), m.shape[1]), "set_u_ref")

    def reset(self):
        self._chk(self.lib.tinympc_reset(self.h), "reset")

    def set_warm_start(self, on):
        self._chk(self.lib.tinympc_set_warm_start(self.h, 1 if on else 0), "set_warm_start")

    def solve(self):
        st = int(self.lib.tinympc_solve(self.h))
        if st < 0:
            raise TinyMPCError(f"solve failed ({_err()})")
        return st

    def solve_async(self, stream=None):
        self._chk(self.lib.tinympc_solve_async(self.h, c_vp(stream or 0)), "solve_async")

    def solve_status(self):
        return int(self.lib.tinympc_solve_status(self.h))

    def get_solution(self):
        nx, nu, N, B = self.nx, self.nu, self.N, self.batch
        sb, cb = np.zeros(nx * N * B), np.zeros(nu * (N - 1) * B)
        self._chk(self.lib.tinympc_get_states(self.h, _dp(sb)), "get_states")
        self._chk(self.lib.tinympc_get_controls(self.h, _dp(cb)), "get_controls")
        return dict(states=sb.reshape((nx, N, B), order="F"), controls=cb.reshape((nu, N - 1, B), order="F"))

    def get_status(self):
        B = self.batch
        it, so, res = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros((B, 4))
        self._chk(self.lib.tinympc_get_status(self.h, it.ctypes.data_as(c_ip), so.ctypes.data_as(c_ip), _dp(res)),
                  "get_status")
        return dict(iter=it, solved=so, residuals=res)

    def get_workspace(self):
        nx, nu, N, B = self.nx, self.nu, self.N, self.batch
        d, y, z = (np.zeros(nu * (N - 1) * B) for _ in range(3))
        g, v = (np.zeros(nx * N * B) for _ in range(2))
        self._chk(self.lib.tinympc_get_workspace(self.h, _dp(d), _dp(y), _dp(g), _dp(v), _dp(z)), "get_workspace")
        ru = lambda a: a.reshape((nu, N - 1, B), order="F")
        rx = lambda a: a.reshape((nx, N, B), order="F")
        return dict(d=ru(d), y=ru(y), z=ru(z), g=rx(g), v=rx(v))

    def set_workspace(self, ws):
        """installs a warm-start workspace: the dict get_workspace returns (d, y, z (nu, N-1, B); g, v (nx, N, B))"""
        flat = {k: np.ascontiguousarray(np.asarray(ws[k], dtype=np.float64).ravel(order="F")) for k in ("d", "y", "g", "v", "z")}
        self._chk(self.lib.tinympc_set_workspace(self.h, *[_dp(flat[k]) for k in ("d", "y", "g", "v", "z")]), "set_workspace")

    def device_buffers(self):
        ptrs = [c_vp() for _ in range(9)]
        self._chk(self.lib.tinympc_device_buffers(self.h, *[ctypes.byref(p) for p in ptrs]), "device_buffers")
        names = ("x0", "x_ref", "u_ref", "states", "controls", "iter", "solved", "residuals", "gstat")
        return {n: p.value for n, p in zip(names, ptrs)}

    def set_ref_mode(self, mode):
        self._chk(self.lib.tinympc_set_ref_mode(self.h, int(mode)), "set_ref_mode")

    def set_x0_f32(self, x0):
        """x0 as a float32 array (nx,) or (nx, B): a plain copy to the device, no fp64 pass on the host"""
        m = np.asfortranarray(np.asarray(x0, dtype=np.float32))
        m = m.reshape(self.nx, -1, order="F")
        self._chk(self.lib.tinympc_set_x0_f32(self.h, m.ctypes.data_as(c_fp), m.shape[1]), "set_x0_f32")

    def get_solution_f32(self, states=None, controls=None):
        """the solution into float32 arrays (nx, N, B) / (nu, N-1, B) (allocated, or the caller's own F-ordered ones)"""
        nx, nu, N, B = self.nx, self.nu, self.N, self.batch
        states = np.zeros((nx, N, B), dtype=np.float32, order="F") if states is None else states
        controls = np.zeros((nu, N - 1, B), dtype=np.float32, order="F") if controls is None else controls
        assert states.flags.f_contiguous and controls.flags.f_contiguous and states.dtype == controls.dtype == np.float32
        self._chk(self.lib.tinympc_get_states_f32(self.h, states.ctypes.data_as(c_fp)), "get_states_f32")
        self._chk(self.lib.tinympc_get_controls_f32(self.h, controls.ctypes.data_as(c_fp)), "get_controls_f32")
        return dict(states=states, controls=controls)

    def pin_host(self, arr):
        """page-lock a numpy array the caller keeps alive and reuses (the fp32 transfers then DMA straight into it);
        call unpin_host(arr) before dropping the array"""
        self._chk(self.lib.tinympc_pin_host(self.h, arr.ctypes.data_as(c_vp), arr.nbytes), "pin_host")

    def unpin_host(self, arr):
        self._chk(self.lib.tinympc_unpin_host(self.h, arr.ctypes.data_as(c_vp)), "unpin_host")

    def set_ref_sequence(self, x_ref_seq, u_ref_seq):
        """shared references of every step of the next closed loops: x_ref_seq (nx, N, steps), u_ref_seq (nu, N-1, steps)
        (rocket_landing_constraints.jl:107-115 shifts them step by step); None, None drops the sequence.
        Step 0's references become the solver's own shared references and stay installed after the loop.
        Supported wherever mpc_rollout is: inside the launch on the transposed-sets kernel (mfmat) and on the lanes-per-instance
        kernels at horizons up to 20 (quad), launch by launch on the chained loops (mfma; the lean kernel's with TINYMPC_HIP_LEAN_WS=1).  mpc_rollout
        raises TinyMPCError, naming the condition, with fewer sequence steps than loop steps, with per-instance references
        (set after the sequence — a later SHARED set_x_ref / set_u_ref drops the sequence instead), with adaptive rho, at
        precision 2, on a quad entry with a horizon above 20, and on shapes without a closed loop (stream / generic kernels) —
        the last two unless TINYMPC_HIP_STREAM_MPC=1 (see mpc_rollout) gives those solvers their chained loop, which takes the
        sequence launch by launch.  A sequence is shared by the batch and N-fold redundant where the steps' references are
        shifted windows of one trajectory: set_ref_trajectory takes that trajectory itself, per instance too.  A sequence
        (steps > 0) replaces an installed trajectory, and a trajectory drops the sequence: the later call wins"""
        if x_ref_seq is None:
            self._chk(self.lib.tinympc_set_ref_sequence(self.h, None, 0, 0, None, 0, 0, 0), "set_ref_sequence")
            return
        xs = np.asfortranarray(np.asarray(x_ref_seq, dtype=np.float64))
        us = np.asfortranarray(np.asarray(u_ref_seq, dtype=np.float64))
        steps = xs.shape[2]
        assert xs.shape == (self.nx, self.N, steps) and us.shape == (self.nu, self.N - 1, steps)
        xs, us = xs.reshape(-1, order="F"), us.reshape(-1, order="F")
        self._chk(self.lib.tinympc_set_ref_sequence(self.h, _dp(xs), self.nx, self.N * steps, _dp(us), self.nu,
                                                    (self.N - 1) * steps, steps), "set_ref_sequence")

    def set_plant(self, A, B, f=None):
        """the plant mpc_rollout steps when it is not the controller's model: x+ = f_p + A_p x + B_p u0 (+ w).  The dimensions
        decide: A (nx, nx), B (nx, nu), f (nx,) shared by the batch, or A (nx, nx, B), B (nx, nu, B), f (nx, B) one plant per
        instance; f None is zero.  set_plant(None, None) drops it: back to the model and to the routes that serve it.  fp64 on
        the host and the device; set_precision keeps it.  See mpc_rollout for the route such a solver takes."""
        if A is None and B is None:
            self._chk(self.lib.tinympc_set_plant(self.h, None, None, None, 0), "set_plant")
            return
        nx, nu, Bn = self.nx, self.nu, self.batch
        A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        f = None if f is None else np.asarray(f, dtype=np.float64)
        per = A.ndim == 3
        want = ((nx, nx, Bn), (nx, nu, Bn), (nx, Bn)) if per else ((nx, nx), (nx, nu), (nx,))
        if A.shape != want[0] or B.shape != want[1] or (f is not None and f.shape != want[2]):
            raise TinyMPCError(f"set_plant: expected A {(nx, nx)}, B {(nx, nu)}, f {(nx,)} or A {(nx, nx, Bn)}, B {(nx, nu, Bn)}, f {(nx, Bn)}; "
                               f"got A {A.shape}, B {B.shape}" + ("" if f is None else f", f {f.shape}"))
        Af, Bf, ff = _flat_f(A), _flat_f(B), None if f is None else _flat_f(f)
        self._chk(self.lib.tinympc_set_plant(self.h, _dp(Af), _dp(Bf), None if ff is None else _dp(ff), 1 if per else 0), "set_plant")

    def set_disturbance(self, w):
        """additive disturbance of every step of the next closed loops: w (nx, steps) shared, or (nx, steps, B) per instance
        (the layout of mpc_rollout's x).  Every mpc_rollout reads it from row 0; a loop longer than `steps` is refused.
        Without set_plant it disturbs the model plant.  None drops it."""
        if w is None:
            self._chk(self.lib.tinympc_set_disturbance(self.h, None, 0, 0), "set_disturbance")
            return
        w = np.asarray(w, dtype=np.float64)
        if w.ndim not in (2, 3) or w.shape[0] != self.nx or w.shape[1] < 1 or (w.ndim == 3 and w.shape[2] != self.batch):
            raise TinyMPCError(f"set_disturbance: expected w (nx, steps) = ({self.nx}, steps) or (nx, steps, batch) = "
                               f"({self.nx}, steps, {self.batch}); got {w.shape}")
        wf = _flat_f(w)
        self._chk(self.lib.tinympc_set_disturbance(self.h, _dp(wf), w.shape[1], 1 if w.ndim == 3 else 0), "set_disturbance")

    def plant_mode(self):
        """0 model, 1 shared plant, 2 per-instance plant; | 4 shared disturbance, | 8 per-instance disturbance"""
        return int(self.lib.tinympc_plant_mode(self.h))

    def set_ref_trajectory(self, x_traj, u_traj=None):
        """a reference trajectory, windowed on the device: every instance tracks a moving target of its own through a closed
        loop, and nothing is uploaded per step.  The dimensions decide: x_traj (nx, Lx) and u_traj (nu, Lu) shared by the batch,
        or (nx, Lx, B) and (nu, Lu, B) one trajectory per instance (the shapes of mpc_rollout's x and u: one run's log can be
        another run's trajectory); both shared or both per instance; u_traj None: zero input references.  With the cursor c the
        references of a solve are ref_window(x_traj, c, N) and ref_window(u_traj, c, N - 1): rows c, c+1, ... with the last
        row held beyond the end, so any Lx, Lu >= 1 serve any number of steps.  Values are rounded to fp32 once, here.
        A new trajectory starts at cursor 0; solve() reads the window at the cursor and leaves it; mpc_rollout(steps) reads the
        windows at c .. c+steps-1 and leaves c+steps (see there for its route); set_ref_cursor moves it.
        set_ref_trajectory(None) drops the trajectory: the window at the cursor stays installed as ordinary references, shared
        or per instance, and the solver returns to the routes that serve those.  set_x_ref / set_u_ref do the same and then
        replace their side; set_ref_sequence and set_ref_mode replace it outright; a trajectory drops a sequence.  set_precision
        keeps the trajectory; re-batching the global solver (set_batch_size, set_gpus) drops it."""
        if x_traj is None:
            self._chk(self.lib.tinympc_set_ref_trajectory(self.h, None, 0, None, 0, 0), "set_ref_trajectory")
            return
        xf, xr, xc, uf, ur, uc, per = _traj_args(x_traj, u_traj)
        n = self.batch if per else 1
        if xr != self.nx or xc < 1 or xc % n != 0 or (uf is not None and (ur != self.nu or uc < 1 or uc % n != 0)) or \
                (per and (np.shape(x_traj)[2] != n or (uf is not None and np.shape(u_traj)[2] != n))):
            raise TinyMPCError(f"set_ref_trajectory: expected x_traj (nx, Lx) = ({self.nx}, Lx) and u_traj (nu, Lu) = ({self.nu}, Lu), or "
                               f"(nx, Lx, batch) = ({self.nx}, Lx, {self.batch}) and (nu, Lu, batch) = ({self.nu}, Lu, {self.batch}), Lx, Lu >= 1; "
                               f"got x_traj {np.shape(x_traj)}" + ("" if u_traj is None else f", u_traj {np.shape(u_traj)}"))
        self._chk(self.lib.tinympc_set_ref_trajectory(self.h, _dp(xf), xc // n, None if uf is None else _dp(uf), uc // n, per),
                  "set_ref_trajectory")

    def set_ref_cursor(self, cursor):
        """move the reference cursor (>= 0): the next solve reads the window there, the next mpc_rollout starts there"""
        self._chk(self.lib.tinympc_set_ref_cursor(self.h, int(cursor)), "set_ref_cursor")

    def ref_cursor(self):
        """the reference cursor: 0 for a new trajectory, `steps` further on after every mpc_rollout"""
        return int(self.lib.tinympc_ref_cursor(self.h))

    def ref_trajectory_mode(self):
        """0 no reference trajectory, 1 shared, 2 per instance"""
        return int(self.lib.tinympc_ref_trajectory_mode(self.h))

    def mpc_rollout(self, steps, stream=None):
        """`steps` closed-loop MPC steps without the host in between: solve, apply u0 to the plant, solve again.  By default
        the plant is the family's own model, x+ = f + A x + B u0, and the loop is fused into one launch where the kernel has one.
        With set_plant / set_disturbance the plant is the caller's, x+ = f_p + A_p x + B_p u0 (+ w) in fp64: the loop then is a
        chain of `steps` ordinary kept-workspace launches, each from the fp32 rounding of the state, with the plant step between
        them — on whatever kernel such a solve takes, every kernel family, shape and precision, no switch, reference sequences
        included; two loops in a row continue the fp64 state unless x0 was set in between.  Refused there: fewer disturbance
        rows than steps, adaptive rho, set_warm_start(0), per-instance bounds without TINYMPC_HIP_STREAM_MPC.
        With set_ref_trajectory every step solves against its own window of the trajectory — step t of the loop against the
        window at cursor + t, cut out on the device by one small kernel before the step's launch — and the cursor is left
        `steps` further on, so two loops in a row continue the trajectory as they continue the state.  Such a solver takes the
        same chain, against the model where no plant is installed, under the environment switches below too (`steps`
        launches), with the same refusals.
        With set_process_noise / set_measurement_noise the same chain again, with noise drawn on the device: the solve of step t
        starts from float32(x_t + G_v xi_v[b][t]) and the plant step ends with + G_w xi_w[b][t], t = noise cursor + loop step;
        the cursor is left `steps` further on, and the dict gains y (nx, steps, B), what every solve started from, while
        measurement noise is installed.  Refused there too: a cursor that would pass the largest int.
        With the model plant, no trajectory and no noise:
        (TINYMPC_HIP_LEAN_WS=1 when the solver is created: cartpole-class shapes on the lean kernel, as a chain of `steps`
        launches; with TINYMPC_HIP_LEAN_LOOP=1 beside it as one launch of its in-kernel loop — the same results.)
        Solvers on the stream / generic kernels (a horizon without a built-in entry, linear rows, cones or the affine term
        outside mfmat, per-instance families, other (nx, nu), precision 2) raise TinyMPCError by default.  With
        TINYMPC_HIP_STREAM_MPC=1 when the solver is created they run the loop as a chain of `steps` warm launches with the
        plant x+ = f + A x + B u0 in fp64 between them (precision 0, 1, 2; reference sequences; each solve starts from the
        fp32 rounding of x+); TINYMPC_HIP_STREAM_LOOP=1 beside it: one launch of the stream kernel's in-kernel loop where it
        is built, bit-identical to the chain.  Adaptive rho, families at precision 2 and set_warm_start(0) stay refused.
        Returns dict(status, x=(nx, steps, B), u=(nu, steps, B), iter=(steps, B), solved=(steps, B))."""
        st = int(self.lib.tinympc_mpc_rollout(self.h, int(steps), c_vp(stream or 0)))
        if st < 0:
            raise TinyMPCError(f"mpc_rollout failed ({_err()})")
        nx, nu, B = self.nx, self.nu, self.batch
        x, u = np.zeros(nx * steps * B), np.zeros(nu * steps * B)
        it = np.zeros(steps * B, dtype=np.int32)
        self._chk(self.lib.tinympc_get_mpc_log(self.h, _dp(x), _dp(u), it.ctypes.data_as(c_ip)), "get_mpc_log")
        it = it.reshape((steps, B), order="F")
        out = dict(status=st, x=x.reshape((nx, steps, B), order="F"), u=u.reshape((nu, steps, B), order="F"),
                   iter=np.abs(it), solved=(it > 0).astype(np.int32))
        if self.estimator_mode():
            ny = int(self.lib.tinympc_estimator_outputs(self.h))
            xh, yo = np.zeros(nx * steps * B), np.zeros(ny * steps * B)
            self._chk(self.lib.tinympc_get_mpc_estimate(self.h, _dp(xh)), "get_mpc_estimate")
            self._chk(self.lib.tinympc_get_mpc_outputs(self.h, _dp(yo)), "get_mpc_outputs")
            out["xhat"], out["yout"] = xh.reshape((nx, steps, B), order="F"), yo.reshape((ny, steps, B), order="F")
        elif self.noise_mode() & 12:
            y = np.zeros(nx * steps * B)
            self._chk(self.lib.tinympc_get_mpc_measured(self.h, _dp(y)), "get_mpc_measured")
            out["y"] = y.reshape((nx, steps, B), order="F")
        return out

    def set_estimator(self, C, L=None):
        """output feedback: the loop measures y = C x + v (ny <= nx outputs; v the first ny rows of the measurement noise, where
        installed) and a fixed-gain estimator stepped in fp64 on the device feeds the solves — correct xhat_t = xhat-_t + L (y_t - C
        xhat-_t), the solve of step t from float32(xhat_t), predict xhat-_{t+1} = f + A xhat_t + B u_t with the MODEL (never an
        installed plant; a per-instance-family solver: each instance's A_b, B_b); host_estimator_step states the rule.  C (ny, nx)
        and L (nx, ny) shared, or (ny, nx, B) and (nx, ny, B); kalman_gain gives the steady-state L.  C None drops it.  Such a
        solver is an own-plant solver (see mpc_rollout): the chain of `steps` launches, every kernel family and precision; its
        log has xhat (nx, steps, B), what each solve started from, and yout (ny, steps, B), and no y.  Between rollouts the solver
        keeps xhat- of the next step (get_estimator_state): two loops in a row are one; the first loop after set_estimator takes
        xhat-_0 = x0 unless set_estimator_state installed another; set_x0 moves the plant, not the estimate.  set_precision
        keeps the estimator, re-batching drops it."""
        if C is None and L is None:
            self._chk(self.lib.tinympc_set_estimator(self.h, None, 0, None, 0), "set_estimator")
            return
        if C is None or L is None:
            raise TinyMPCError("set_estimator: expected both C (ny, nx) and L (nx, ny), or neither to drop the estimator")
        Cf, Lf, ny, nx, per = _estimator_matrices(C, L, "set_estimator")
        if nx != self.nx or (per and np.shape(C)[2] != self.batch):
            raise TinyMPCError(f"set_estimator: expected C (ny, {self.nx}) and L ({self.nx}, ny), or with a trailing axis of {self.batch}; got {np.shape(C)} and {np.shape(L)}")
        self._chk(self.lib.tinympc_set_estimator(self.h, _dp(Cf), ny, _dp(Lf), per), "set_estimator")

    def set_estimator_state(self, xhat):
        """install xhat- of the next step, (nx,) shared or (nx, B) fp64; None re-arms it: the next mpc_rollout takes xhat-_0 = x0"""
        if xhat is None:
            self._chk(self.lib.tinympc_set_estimator_state(self.h, None, 0), "set_estimator_state")
            return
        xh = np.asarray(xhat, dtype=np.float64)
        if xh.shape not in ((self.nx,), (self.nx, self.batch)):
            raise TinyMPCError(f"set_estimator_state: expected xhat ({self.nx},) or ({self.nx}, {self.batch}); got {xh.shape}")
        self._chk(self.lib.tinympc_set_estimator_state(self.h, _dp(_flat_f(xh)), 1 if xh.ndim == 2 else 0), "set_estimator_state")

    def estimator_mode(self):
        """0: no estimator, 1: shared C and L, 2: per instance"""
        return int(self.lib.tinympc_estimator_mode(self.h))

    def get_estimator_state(self):
        """the current xhat- of the next step, (nx, B) fp64"""
        buf = np.zeros(self.nx * self.batch)
        self._chk(self.lib.tinympc_get_estimator_state(self.h, _dp(buf)), "get_estimator_state")
        return buf.reshape((self.nx, self.batch), order="F")

    host_estimator_step = staticmethod(host_estimator_step)
    kalman_gain = staticmethod(kalman_gain)

    def _set_noise(self, which, G, seed):
        name = "set_process_noise" if which == NOISE_PROCESS else "set_measurement_noise"
        fn = getattr(self.lib, "tinympc_" + name)
        if G is None:
            self._chk(fn(self.h, None, 0, 0), name)
            return
        Gf, rows, cols, per = _noise_factor(G, name)
        if rows != self.nx or cols != self.nx * (self.batch if per else 1):
            raise TinyMPCError(f"{name}: expected G (nx, nx) = ({self.nx}, {self.nx}), (nx, nx, batch) = ({self.nx}, {self.nx}, {self.batch}) "
                               f"or sigma (nx,) = ({self.nx},); got {np.shape(G)}")
        self._chk(fn(self.h, _dp(Gf), per, int(seed) & 0xFFFFFFFFFFFFFFFF), name)

    def set_process_noise(self, G, seed=0):
        """seeded process noise, drawn on the device: every plant step of mpc_rollout ends with one fp64 add of G xi_w[b][t], after
        the uploaded disturbance if there is one, x+ = ((f_p + A_p x + B_p u0) + w) + G xi.  xi are standard normals that are a
        pure function of (seed, kind, instance b, step t) — Philox4x32-10 and Box-Muller, host_noise states the rule — so
        nothing is stored or uploaded, and t = noise cursor + loop step: two loops in a row continue the noise stream as they
        continue the state.  The dimensions decide: G (nx, nx) shared, (nx, nx, B) one factor per instance, a 1-D (nx,) array
        is diag(sigma); the covariance is G G'.  None drops it.  A solver with either noise is an own-plant solver (see
        mpc_rollout): the chain of `steps` launches, every kernel family and precision.  A newly installed noise leaves the
        cursor alone; set_precision keeps the noise, re-batching drops it."""
        self._set_noise(NOISE_PROCESS, G, seed)

    def set_measurement_noise(self, G, seed=0):
        """seeded measurement noise, drawn on the device: the solve of step t starts from float32(x_t + G xi_v[b][t]), x_t the fp64
        plant state, which the measurement never contaminates — the x log, x0d and x0 after the loop hold the true state.  What
        every solve started from comes back as mpc_rollout's `y`.  G, seed, None: as set_process_noise; one cursor serves both."""
        self._set_noise(NOISE_MEASUREMENT, G, seed)

    def set_noise_cursor(self, t):
        """move the noise cursor (>= 0): the step index the next mpc_rollout's first draw carries"""
        self._chk(self.lib.tinympc_set_noise_cursor(self.h, int(t)), "set_noise_cursor")

    def noise_cursor(self):
        """the noise cursor: 0 for a new solver, `steps` further on after every mpc_rollout of a solver with noise"""
        return int(self.lib.tinympc_noise_cursor(self.h))

    def noise_mode(self):
        """1 shared / 2 per-instance process factor; | 4 shared / | 8 per-instance measurement factor"""
        return int(self.lib.tinympc_noise_mode(self.h))

    def get_noise(self, which, t0, steps):
        """the realised noise vectors G xi of kind `which` (0 process, 1 measurement) at the steps t0 .. t0 + steps - 1, computed
        on the device by the loop's own device function: (nx, steps, B) fp64 — as a disturbance, set_disturbance(get_noise(0, c,
        steps)) reproduces the process noise of a loop from cursor c bit for bit"""
        buf = np.zeros(self.nx * int(steps) * self.batch)
        self._chk(self.lib.tinympc_get_noise(self.h, int(which), int(t0), int(steps), _dp(buf)), "get_noise")
        return buf.reshape((self.nx, int(steps), self.batch), order="F")

    host_noise = staticmethod(host_noise)

    def set_rollout_metrics(self, enable=True, qw=None, rw=None, x_lo=None, x_hi=None, u_lo=None, u_hi=None):
        """per-instance metrics of the closed loop, folded on the device: while enabled every mpc_rollout, whatever its route, is
        followed on its stream by one kernel that reads the log it wrote and updates 11 fp64 slots per instance (METRIC_NAMES:
        steps, cost_x = sum qw e^2, cost_u = sum rw v^2, peak_err, final_err, x_viol_max, x_viol_steps, first_viol, u_sat_steps,
        iters, maxiter_steps; e = x - the step's x target, v = u - its u target, the targets knot 1 / knot 0 of the references
        the step's solve used; host_rollout_metrics states the rule).  They accumulate over rollouts until reset_rollout_metrics,
        so a long run is a sequence of short rollouts on a fixed-size log and only the statistics leave the device.
        qw (nx,), rw (nu,): non-negative weights, None = the diagonal of Q / R (refused on a per-instance-family solver).
        x_lo, x_hi (nx,), u_lo, u_hi (nu,): the metric's own safe set, not the solver's bounds; None = that side never counts.
        enable=True installs or replaces the configuration and zeroes the accumulators; False drops both.  set_precision keeps
        them, re-batching drops them."""
        vecs, p = _metric_config(self.nx, self.nu, qw, rw, x_lo, x_hi, u_lo, u_hi, "set_rollout_metrics")
        self._chk(self.lib.tinympc_set_rollout_metrics(self.h, 1 if enable else 0, *p), "set_rollout_metrics")

    def reset_rollout_metrics(self):
        """the accumulators to zero, the configuration kept"""
        self._chk(self.lib.tinympc_reset_rollout_metrics(self.h), "reset_rollout_metrics")

    def rollout_metrics_mode(self):
        """0 off, 1 on"""
        return int(self.lib.tinympc_rollout_metrics_mode(self.h))

    def get_rollout_metrics(self):
        """the per-instance metrics, (B, 11) fp64, columns in METRIC_NAMES' order; zeros before any rollout"""
        buf = np.zeros((self.batch, METRIC_COUNT))
        self._chk(self.lib.tinympc_get_rollout_metrics(self.h, _dp(buf)), "get_rollout_metrics")
        return buf

    def get_rollout_summary(self, as_dict=False):
        """the batch summary folded on the device in a fixed order, (11, 4) fp64: per slot the sum, the minimum, the maximum and
        the number of instances whose value is > 0; as_dict: {slot name: {"sum", "min", "max", "count"}}"""
        buf = np.zeros((METRIC_COUNT, 4))
        self._chk(self.lib.tinympc_get_rollout_summary(self.h, _dp(buf)), "get_rollout_summary")
        return summary_dict(buf) if as_dict else buf

    host_rollout_metrics = staticmethod(host_rollout_metrics)

    def set_profiling(self, on):
        self._chk(self.lib.tinympc_set_profiling(self.h, 1 if on else 0), "set_profiling")

    def set_compaction(self, chunk_iters):
        """tolerance-terminated solves in chunks of `chunk_iters` iterations with the unconverged instances compacted
        in between (0: off)"""
        self._chk(self.lib.tinympc_set_compaction(self.h, int(chunk_iters)), "set_compaction")

    def kernel_elapsed_ms(self, last_n=1):
        """duration of the last launch, or the mean over the last `last_n` launches (profiling mode)"""
        if last_n == 1:
            return float(self.lib.tinympc_kernel_elapsed_ms(self.h))
        return float(self.lib.tinympc_kernel_elapsed_mean_ms(self.h, int(last_n)))

    def set_precision(self, precision):
        """0: fp64 recurrences, fp32 state (default); 1: all fp32; 2: all fp64 like the reference — on the generic kernel
        (slow), except cold one-shot solves of the lean kernel's shapes (its fp64-state form, specialised on request) and, with
        TINYMPC_HIP_STREAM_F64=1 set when the solver is created, every fixed-rho unchunked solve of (4,1), (6,3), (12,4) shapes
        on the stream kernel's fp64-state form ("stream4<NX,NU;f64>").  Precision 2 has no closed loop (mpc_rollout raises)
        unless TINYMPC_HIP_STREAM_MPC=1 is set when the solver is created: then the chain of launches, or with
        TINYMPC_HIP_STREAM_LOOP=1 the fp64-state form's in-kernel loop"""
        self._chk(self.lib.tinympc_set_precision(self.h, int(precision)), "set_precision")

    def reload_switches(self):
        """re-read the TINYMPC_HIP_* environment switches (they are read once, at creation)"""
        self._chk(self.lib.tinympc_reload_switches(self.h), "reload_switches")

    def set_strict_precision(self, strict):
        """True: precision = 1 means fp32 recurrences even where a (faster) fp64 matrix-core kernel exists for the shape"""
        self._chk(self.lib.tinympc_set_strict_precision(self.h, 1 if strict else 0), "set_strict_precision")

    @property
    def effective_precision(self):
        """recurrence precision the current options run with: 0 fp64, 1 fp32"""
        return int(self.lib.tinympc_effective_precision(self.h))

    @property
    def kernel_name(self):
        return self.lib.tinympc_kernel_name(self.h).decode()

    @property
    def last_launch_name(self):
        """the kernel the most recent launch actually ran (the family, or e.g. its lean<nx,nu,N> one-shot variant)"""
        return self.lib.tinympc_last_launch_name(self.h).decode()

    def algorithmic_bytes(self):
        return float(self.lib.tinympc_algorithmic_bytes(self.h))

    def algorithmic_flops(self, iters):
        return float(self.lib.tinympc_algorithmic_flops(self.h, int(iters)))


def specialise(nx, nu, N, verbose=False):
    """compile / load the on-chip kernel of a shape the library was not built with, ahead of time (what BatchSolver does by
    itself at creation): True if the shape has an on-chip kernel afterwards"""
    return bool(load_library().tinympc_specialise(int(nx), int(nu), int(N), 1 if verbose else 0))


def shard_range(batch, n_shards, shard):
    """the library's partition rule (no GPU needed): [lo, hi) of `shard`"""
    lo, hi = c_int(), c_int()
    load_library().tinympc_shard_range(int(batch), int(n_shards), int(shard), ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


class ShardedBatchSolver:
    """One handle, several GPUs of one node, ONE host process (tinympc_sharded_* in include/tinympc_hip.h): the batch in
    contiguous shards, one per device; inputs scattered, outputs gathered, the solve status all-reduced over RCCL."""

    def __init__(self, A, B, Q, R, rho, N, batch, n_gpus=1, devices=None, verbose=False):
        self.lib = load_library()
        A, B, Q, R = _mat(A), _mat(B), _mat(Q), _mat(R)
        self.nx, self.nu, self.N, self.batch = A.shape[0], B.shape[1], int(N), int(batch)
        dv = None
        if devices is not None:
            devices = np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
            n_gpus, dv = len(devices), devices.ctypes.data_as(c_ip)
        h = c_vp()
        st = self.lib.tinympc_create_sharded(ctypes.byref(h), _dp(A), _dp(B), _dp(Q), _dp(R), float(rho), self.nx, self.nu,
                                             self.N, self.batch, int(n_gpus), dv, 1 if verbose else 0)
        if st != 0:
            raise TinyMPCError(f"tinympc_create_sharded failed ({_err()})")
        self.h = h
        self.n_shards = int(self.lib.tinympc_sharded_n_shards(h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.tinympc_sharded_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st, what):
        if st != 0:
            raise TinyMPCError(f"{what} failed ({_err()})")

    @property
    def fold_backend(self):
        return self.lib.tinympc_sharded_fold_backend(self.h).decode()

    def shard(self, i):
        """(device, lo, hi, handle of the shard's single-device solver)"""
        d, lo, hi, loc = c_int(), c_int(), c_int(), c_vp()
        self._chk(self.lib.tinympc_sharded_shard(self.h, int(i), ctypes.byref(d), ctypes.byref(lo), ctypes.byref(hi),
                                                 ctypes.byref(loc)), "shard")
        return d.value, lo.value, hi.value, loc

    def kernel_names(self):
        return [self.lib.tinympc_kernel_name(self.shard(i)[3]).decode() for i in range(self.n_shards)]

    def update_settings(self, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1, en_state_bound=0,
                        en_input_bound=0):
        self._chk(self.lib.tinympc_sharded_update_settings(self.h, float(abs_pri_tol), float(abs_dua_tol), int(max_iter),
                                                           int(check_termination), int(en_state_bound),
                                                           int(en_input_bound)), "update_settings")

    def set_bound_constraints(self, x_min, x_max, u_min, u_max):
        ms = [_mat(m) for m in (x_min, x_max, u_min, u_max)]
        self._chk(self.lib.tinympc_sharded_set_bound_constraints(self.h, *[_dp(m) for m in ms]), "set_bound_constraints")

    def set_instance_bounds(self, x_min, x_max, u_min, u_max):
        """per-instance bounds over the whole batch (shapes as BatchSolver.set_instance_bounds), scattered to the shards"""
        flat, per_knot = _instance_bounds(x_min, x_max, u_min, u_max)
        want = [self.nx * (self.N if per_knot else 1), self.nx * (self.N if per_knot else 1),
                self.nu * (self.N - 1 if per_knot else 1), self.nu * (self.N - 1 if per_knot else 1)]
        if [f.size for f in flat] != [w * self.batch for w in want]:
            raise TinyMPCError("set_instance_bounds: expected (nx, batch) / (nu, batch) or (nx, N, batch) / (nu, N-1, batch)")
        self._chk(self.lib.tinympc_sharded_set_instance_bounds(self.h, *[_dp(f) for f in flat], 1 if per_knot else 0),
                  "set_instance_bounds")

    def set_instance_linear(self, Alin_x, blin_x, Alin_u, blin_u):
        """per-instance linear rows over the whole batch (shapes as BatchSolver.set_instance_linear), scattered to the shards"""
        Ax, bx, mx = _instance_linear(Alin_x, blin_x, self.nx, self.batch)
        Au, bu, mu = _instance_linear(Alin_u, blin_u, self.nu, self.batch)
        self._chk(self.lib.tinympc_sharded_set_instance_linear(self.h, _dp(Ax) if mx else None, mx, _dp(bx) if mx else None,
                                                               _dp(Au) if mu else None, mu, _dp(bu) if mu else None), "set_instance_linear")

    def set_instance_cones(self, Acu, qcu, cu, Acx, qcx, cx):
        """per-instance cone coefficients over the whole batch (shapes as BatchSolver.set_instance_cones), scattered to the shards"""
        au, qu, cuv, n_u = _instance_cones(Acu, qcu, cu, self.batch)
        ax, qx, cxv, n_x = _instance_cones(Acx, qcx, cx, self.batch)
        self._chk(self.lib.tinympc_sharded_set_instance_cones(
            self.h, au.ctypes.data_as(c_ip) if n_u else None, qu.ctypes.data_as(c_ip) if n_u else None, _dp(cuv) if n_u else None, n_u,
            ax.ctypes.data_as(c_ip) if n_x else None, qx.ctypes.data_as(c_ip) if n_x else None, _dp(cxv) if n_x else None, n_x),
            "set_instance_cones")

    def set_warm_start(self, on):
        self._chk(self.lib.tinympc_sharded_set_warm_start(self.h, 1 if on else 0), "set_warm_start")

    def reset(self):
        self._chk(self.lib.tinympc_sharded_reset(self.h), "reset")

    def set_precision(self, precision):
        self._chk(self.lib.tinympc_sharded_set_precision(self.h, int(precision)), "set_precision")

    def set_compaction(self, chunk_iters):
        self._chk(self.lib.tinympc_sharded_set_compaction(self.h, int(chunk_iters)), "set_compaction")

    def set_x0(self, x0):
        m = _mat(x0)
        self._chk(self.lib.tinympc_sharded_set_x0(self.h, _dp(m), m.shape[1]), "set_x0")

    def set_x_ref(self, x_ref):
        m = _ref3(x_ref)
        self._chk(self.lib.tinympc_sharded_set_x_ref(self.h, _dp(m), m.shape[1]), "set_x_ref")

    def set_u_ref(self, u_ref):
        m = _ref3(u_ref)
        self._chk(self.lib.tinympc_sharded_set_u_ref(self.h, _dp(m), m.shape[1]), "set_u_ref")

    def solve(self):
        st = int(self.lib.tinympc_sharded_solve(self.h))
        if st < 0:
            raise TinyMPCError(f"sharded solve failed ({_err()})")
        return st

    def solve_async(self):
        self._chk(self.lib.tinympc_sharded_solve_async(self.h), "solve_async")

    def wait(self):
        st = int(self.lib.tinympc_sharded_wait(self.h))
        if st < 0:
            raise TinyMPCError(f"sharded wait failed ({_err()})")
        return st

    def global_status(self):
        """(residual maxima over all instances (4,), largest per-device unsolved count) of the last solve"""
        res, n = np.zeros(4), c_int()
        self._chk(self.lib.tinympc_sharded_global_status(self.h, _dp(res), ctypes.byref(n)), "global_status")
        return res, n.value

    def get_solution(self):
        nx, nu, N, B = self.nx, self.nu, self.N, self.batch
        sb, cb = np.zeros(nx * N * B), np.zeros(nu * (N - 1) * B)
        self._chk(self.lib.tinympc_sharded_get_states(self.h, _dp(sb)), "get_states")
        self._chk(self.lib.tinympc_sharded_get_controls(self.h, _dp(cb)), "get_controls")
        return dict(states=sb.reshape((nx, N, B), order="F"), controls=cb.reshape((nu, N - 1, B), order="F"))

    def get_status(self):
        B = self.batch
        it, so, res = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros((B, 4))
        self._chk(self.lib.tinympc_sharded_get_status(self.h, it.ctypes.data_as(c_ip), so.ctypes.data_as(c_ip), _dp(res)),
                  "get_status")
        return dict(iter=it, solved=so, residuals=res)

    def get_workspace(self):
        nx, nu, N, B = self.nx, self.nu, self.N, self.batch
        d, y, z = (np.zeros(nu * (N - 1) * B) for _ in range(3))
        g, v = (np.zeros(nx * N * B) for _ in range(2))
        self._chk(self.lib.tinympc_sharded_get_workspace(self.h, _dp(d), _dp(y), _dp(g), _dp(v), _dp(z)), "get_workspace")
        ru = lambda a: a.reshape((nu, N - 1, B), order="F")
        rx = lambda a: a.reshape((nx, N, B), order="F")
        return dict(d=ru(d), y=ru(y), z=ru(z), g=rx(g), v=rx(v))
