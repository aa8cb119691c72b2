"""ctypes binding of libdpgo_hip.so (include/dpgo_hip.h).

This is the Python-side binding a maintainer would add next to the reference's C++ API; it is
used by the test-suite, ``bench.py`` and the multi-GPU RBCD driver.  It never falls back to a
CPU implementation: if the shared library or a gfx950 device is missing, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DPGO_HIP_LIB: another build of the library (tools/ A/B runs against a previous build only)
LIB_PATH = os.environ.get("DPGO_HIP_LIB") or os.path.join(_HERE, "libdpgo_hip.so")

PRECON_EXACT, PRECON_BLOCK_JACOBI, PRECON_NONE = 0, 1, 2
QFMT_BSR, QFMT_EDGES = 0, 1
ROBUST = {"L2": 0, "L1": 1, "TLS": 2, "Huber": 3, "GM": 4, "GNC_TLS": 5}
ALG_RTR, ALG_RGD = 0, 1
TCG_NAMES = {-1: "NONE", 0: "NEGCURVTURE", 1: "EXCREGION", 2: "LCON", 3: "SCON", 4: "MAXITER"}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class OptParams(C.Structure):
    _fields_ = [("algorithm", C.c_int), ("rgd_stepsize", C.c_double), ("tr_iterations", C.c_int),
                ("tr_tolerance", C.c_double), ("tr_initial_radius", C.c_double),
                ("tr_max_inner", C.c_int), ("verbose", C.c_int), ("precon", C.c_int)]


class OptResult(C.Structure):
    _fields_ = [("success", C.c_int), ("fInit", C.c_double), ("gradNormInit", C.c_double),
                ("fOpt", C.c_double), ("gradNormOpt", C.c_double), ("relativeChange", C.c_double),
                ("elapsedMs", C.c_double), ("tCGStatus", C.c_int), ("runs", C.c_int),
                ("outer_iters", C.c_int), ("inner_iters", C.c_int), ("gave_up", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class EscapeParams(C.Structure):
    """dpgo_escape_params (include/dpgo_hip.h)."""
    _fields_ = [("alpha0", C.c_double), ("decrease", C.c_double), ("min_gradnorm", C.c_double),
                ("max_halvings", C.c_int)]


class EscapeInfo(C.Structure):
    """dpgo_escape_info (include/dpgo_hip.h)."""
    _fields_ = [("accepted", C.c_int), ("trials", C.c_int), ("alpha", C.c_double), ("f_before", C.c_double),
                ("f_after", C.c_double), ("gradnorm_after", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RankInfo(C.Structure):
    """dpgo_rank_info (include/dpgo_rbcd.h)."""
    _fields_ = [("w", C.c_double * 8), ("dropped", C.c_double), ("f_before", C.c_double), ("f_after", C.c_double)]


class CholCertParams(C.Structure):
    """dpgo_chol_cert_params (include/dpgo_hip.h)."""
    _fields_ = [("ratio", C.c_double), ("max_factorisations", C.c_int), ("tol", C.c_double), ("max_iters", C.c_int)]


class BlockCertParams(C.Structure):
    """dpgo_block_cert_params (include/dpgo_hip.h)."""
    _fields_ = [("max_iters", C.c_int), ("tol", C.c_double), ("flags", C.c_int), ("precon", C.c_int),
                ("refresh", C.c_int)]


class CholCertInfo(C.Structure):
    """dpgo_chol_cert_info (include/dpgo_hip.h)."""
    _fields_ = [("certified", C.c_int), ("factorisations", C.c_int), ("sigma_lo", C.c_double),
                ("sigma_hi", C.c_double), ("invit_iters", C.c_int), ("residual", C.c_double),
                ("factor_ms", C.c_double), ("panel_doubles", C.c_longlong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Edges(C.Structure):
    """dpgo_edges (include/dpgo_hip.h): host or device pointers, as the entry point says."""
    _fields_ = [("m", C.c_longlong), ("p1", C.c_void_p), ("p2", C.c_void_p), ("R", C.c_void_p), ("t", C.c_void_p),
                ("kappa", C.c_void_p), ("tau", C.c_void_p), ("w", C.c_void_p)]


class AlignInfo(C.Structure):
    """dpgo_align_info (include/dpgo_hip.h)."""
    _fields_ = [("count", C.c_double), ("sigma", C.c_double * 3), ("rank", C.c_int)]


class EvalInfo(C.Structure):
    """dpgo_eval_info (include/dpgo_rbcd.h)."""
    _fields_ = [("count", C.c_double), ("Aa", C.c_double * 12), ("sigma", C.c_double * 3), ("rank", C.c_int),
                ("ate_rmse", C.c_double), ("ate_max", C.c_double), ("rot_rmse", C.c_double), ("rot_max", C.c_double),
                ("rpe_tra_rmse", C.c_double), ("rpe_rot_rmse", C.c_double), ("edges_used", C.c_double)]


class DPGOHipError(RuntimeError):
    code = 0  # the C ABI's return code where one raised it


_lib = None

# (name, argtypes, restype)
_SIGS = [
    ("dpgo_hip_version", [], C.c_char_p),
    ("dpgo_hip_last_error", [], C.c_char_p),
    ("dpgo_hip_device_count", [], C.c_int),
    ("dpgo_hip_default_params", [C.POINTER(OptParams)], None),
    ("dpgo_hip_problem_create", [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    ("dpgo_hip_problem_create_batch", [C.c_int, _ip, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    ("dpgo_hip_problem_destroy", [C.c_void_p], C.c_int),
    ("dpgo_hip_problem_set_stream", [C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_problem_info", [C.c_void_p, _ip, _ip, _ip, _ip], C.c_int),
    ("dpgo_hip_set_precon", [C.c_void_p, C.c_int], C.c_int),
    ("dpgo_hip_set_Q_csr", [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _dp], C.c_int),
    ("dpgo_hip_set_Q_bsr", [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _dp], C.c_int),
    ("dpgo_hip_set_Q_edges", [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_set_edge_weights_dev", [C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_set_G", [C.c_void_p, C.c_int, C.c_int, _ip, _dp], C.c_int),
    ("dpgo_hip_set_G_dense", [C.c_void_p, C.c_int, _dp], C.c_int),
    ("dpgo_hip_f", [C.c_void_p, _dp, _dp], C.c_int),
    ("dpgo_hip_egrad", [C.c_void_p, _dp, _dp], C.c_int),
    ("dpgo_hip_ehvp", [C.c_void_p, _dp, _dp], C.c_int),
    ("dpgo_hip_riegrad", [C.c_void_p, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_rhvp", [C.c_void_p, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_precondition", [C.c_void_p, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_tangent_project", [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_retract_qf", [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, _dp], C.c_int),
    ("dpgo_hip_project_polar", [C.c_int, C.c_int, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_hip_round_se", [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_round_se_dev", [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
     C.c_int),
    ("dpgo_hip_frame_lift", [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _ip, _dp], C.c_int),
    ("dpgo_hip_frame_lift_dev", [C.c_int, C.c_int, C.c_longlong, C.c_void_p, _dp, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_lift_escape", [C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, _dp], C.c_int),
    ("dpgo_hip_lift_escape_dev", [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                  C.c_void_p], C.c_int),
    ("dpgo_hip_escape_direction", [C.c_int, C.c_int, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_hip_default_escape_params", [C.POINTER(EscapeParams)], None),
    ("dpgo_hip_escape", [C.c_void_p, _dp, _dp, C.c_double, C.POINTER(EscapeParams), _dp, C.POINTER(EscapeInfo)],
     C.c_int),
    ("dpgo_hip_gram", [C.c_int, C.c_int, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_hip_gram_work_doubles", [C.c_int, C.c_int, C.c_longlong], C.c_longlong),
    ("dpgo_hip_gram_dev", [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_gram_eig", [C.c_int, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_rank_reduce", [C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_hip_rank_reduce_dev", [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, _dp, C.c_void_p, C.c_void_p],
     C.c_int),
    ("dpgo_hip_edge_errors", [C.c_int, C.c_int, C.c_int, C.POINTER(Edges), _dp, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_edge_errors_work_doubles", [C.c_longlong], C.c_longlong),
    ("dpgo_hip_edge_errors_dev", [C.c_int, C.c_int, C.c_longlong, C.POINTER(Edges), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_traj_moments", [C.c_int, C.c_int, _dp, _dp, _ip, _dp, _dp], C.c_int),
    ("dpgo_hip_traj_moments_work_doubles", [C.c_int, C.c_longlong], C.c_longlong),
    ("dpgo_hip_traj_moments_dev", [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_void_p,
                                   C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_align_moments", [C.c_int, _dp, _dp, C.c_double, _dp, C.POINTER(AlignInfo)], C.c_int),
    ("dpgo_hip_traj_align", [C.c_int, C.c_int, _dp, _dp, _ip, _dp, C.POINTER(AlignInfo)], C.c_int),
    ("dpgo_hip_traj_errors", [C.c_int, C.c_int, _dp, _dp, _ip, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_traj_errors_work_doubles", [C.c_int, C.c_longlong], C.c_longlong),
    ("dpgo_hip_traj_errors_dev", [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_relative_poses", [C.c_int, C.c_int, _dp, C.c_int, _ip, _ip, _dp, _dp], C.c_int),
    ("dpgo_hip_relative_poses_dev", [C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_optimize", [C.c_void_p, C.POINTER(OptParams), _dp, _dp, C.POINTER(OptResult)], C.c_int),
    ("dpgo_hip_f_dev", [C.c_void_p, C.c_void_p, _dp], C.c_int),
    ("dpgo_hip_egrad_dev", [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_ehvp_dev", [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_riegrad_dev", [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_rhvp_dev", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_project_polar_dev", [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_hip_polar_combine_dev", [C.c_void_p, C.c_void_p, C.c_void_p, _dp, _dp, C.c_void_p], C.c_int),
    ("dpgo_hip_optimize_dev", [C.c_void_p, C.POINTER(OptParams), C.c_void_p, C.c_void_p, _ip,
                               C.POINTER(OptResult)], C.c_int),
    ("dpgo_hip_synchronize", [C.c_void_p], C.c_int),
    ("dpgo_hip_set_tuning", [C.c_int, C.c_int], C.c_int),
    ("dpgo_hip_get_tuning", [C.c_int, C.POINTER(C.c_int)], C.c_int),
    ("dpgo_hip_exact_factor_info", [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_int)], C.c_int),
    ("dpgo_hip_exact_factor_flops", [C.c_void_p, _dp, _dp], C.c_int),
    ("dpgo_hip_exact_fallback_agents", [C.c_void_p, _ip, _ip], C.c_int),
    ("dpgo_hip_exact_sweep_bytes", [C.c_void_p, _dp, _dp], C.c_int),
    ("dpgo_hip_bench_precond", [C.c_void_p, C.c_void_p, C.c_int, _dp, _dp, _dp], C.c_int),
    ("dpgo_hip_problem_set_tuning", [C.c_void_p, C.c_int, C.c_int], C.c_int),
    ("dpgo_hip_spmm_bytes", [C.c_void_p], C.c_double),
    ("dpgo_hip_bench_spmm", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _dp], C.c_int),
    ("dpgo_hip_spmm_bytes_bsr", [C.c_void_p], C.c_double),
    ("dpgo_hip_certify", [C.c_void_p, _dp, C.c_int, C.c_double, _dp, _dp, _ip, _dp], C.c_int),
    ("dpgo_hip_certify_ex", [C.c_void_p, _dp, C.c_int, C.c_int, C.c_int, C.c_double, _dp, _dp, C.c_void_p],
     C.c_int),
    ("dpgo_default_chol_cert_params", [C.POINTER(CholCertParams)], None),
    ("dpgo_hip_certify_chol", [C.c_void_p, _dp, C.c_double, _ip], C.c_int),
    ("dpgo_hip_certify_chol_ex", [C.c_void_p, _dp, C.c_double, C.POINTER(CholCertParams), _dp, _dp,
                                  C.POINTER(CholCertInfo)], C.c_int),
    ("dpgo_default_block_cert_params", [C.POINTER(BlockCertParams)], None),
    ("dpgo_hip_certify_block", [C.c_void_p, _dp, C.POINTER(BlockCertParams), _dp, _dp, C.c_void_p], C.c_int),
    ("dpgo_hip_bench_hvp", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _dp], C.c_int),
    ("dpgo_hip_stats", [C.c_void_p, _ip], C.c_int),
    ("dpgo_hip_set_trace", [C.c_void_p, C.c_int], C.c_int),
    ("dpgo_hip_get_trace", [C.c_void_p, C.c_int, _dp, C.c_int, _ip], C.c_int),
    ("dpgo_hip_build_id", [], C.c_char_p),
    ("dpgo_hip_tile_of_block", [C.c_int, C.c_int, C.c_int], C.c_int),
    ("dpgo_hip_tile_map", [C.c_int, C.c_int, _ip], C.c_int),
]
STATS_INTS = 13
STATS_FIELDS = ["calls", "early", "runs", "tcg_iters", "NEGCURVTURE", "EXCREGION", "LCON", "SCON", "MAXITER",
                "gave_up", "cg_steps", "implicit", "first_full"]
TRACE_WIDTH = 16
TRACE_FIELDS = ["op", "j", "f1", "f2", "rho", "Delta", "alpha", "beta", "tau", "d_Hd", "norm_r", "z_r", "status",
                "accepted", "ngf", "run"]
SPMM_MODES = ["XQ", "XQ_G", "EVAL", "HESS", "F", "EVAL_TCG", "CERT", "QF", "HESS_QF", "HESS_M", "HESS_QF_M"]

EXPORTED_SYMBOLS = [s[0] for s in _SIGS]


def lib():
    """Load libdpgo_hip.so (built in-tree by __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DPGOHipError(f"{LIB_PATH} not built: run __graft_entry__.build() (no CPU fallback)")
        # torch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7, NEEDED as
        # "libamdhip64.so").  Load torch first so our NEEDED libamdhip64.so.7 binds to that same
        # runtime; loading ours first would put two HIP runtimes in one process.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, args, res in _SIGS:
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _lib = L
        # DPGO_TUNE="key=value,...": process defaults of tuning keys (A/B and profiling runs of tools/ and bench.py)
        for kv in filter(None, os.environ.get("DPGO_TUNE", "").split(",")):
            k, v = kv.split("=")
            _check(L.dpgo_hip_set_tuning(int(k), int(v)))
    return _lib


def _check(rc):
    if rc != 0:
        e = DPGOHipError(f"dpgo_hip error {rc}: {lib().dpgo_hip_last_error().decode()}")
        e.code = rc
        raise e


def chol_cert_params(**kw) -> CholCertParams:
    """dpgo_default_chol_cert_params with the given fields (ratio, max_factorisations, tol, max_iters) replaced."""
    p = CholCertParams()
    lib().dpgo_default_chol_cert_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(CholCertParams._fields_):
            raise TypeError(f"unknown certificate parameter {k!r}")
        setattr(p, k, v)
    return p


def block_cert_params(**kw) -> BlockCertParams:
    """dpgo_default_block_cert_params with the given fields (max_iters, tol, flags, precon, refresh) replaced."""
    p = BlockCertParams()
    lib().dpgo_default_block_cert_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(BlockCertParams._fields_):
            raise TypeError(f"unknown certificate parameter {k!r}")
        setattr(p, k, v)
    return p


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def device_count() -> int:
    return int(lib().dpgo_hip_device_count())


def build_id() -> str:
    """Source hash compiled into the loaded libdpgo_hip.so (__graft_entry__.source_hash())."""
    return lib().dpgo_hip_build_id().decode()


def tile_of_block(block: int, num_blocks: int, reverse: int) -> int:
    """The tile a block of a pose-tiled launch works on (dpgo_hip_tile_of_block)."""
    return int(lib().dpgo_hip_tile_of_block(int(block), int(num_blocks), int(reverse)))


def tile_map(num_blocks: int, reverse: int) -> np.ndarray:
    """tile_of_block of every block of a launch (dpgo_hip_tile_map)."""
    out = np.empty(int(num_blocks), np.int32)
    _check(lib().dpgo_hip_tile_map(int(num_blocks), int(reverse), out.ctypes.data_as(_ip)))
    return out


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the library's RCCL (128 opaque bytes)."""
    buf = C.create_string_buffer(128)
    _check(lib().dpgo_rccl_unique_id(buf))
    return buf.raw


def get_tuning(key: int) -> int:
    """Process default of a tuning key."""
    v = C.c_int()
    _check(lib().dpgo_hip_get_tuning(int(key), C.byref(v)))
    return v.value


def set_tuning(key: int, value: int):
    """Process default of a tuning key: handles created afterwards copy it (Problem / Rbcd.set_tuning change
    an existing one)."""
    _check(lib().dpgo_hip_set_tuning(int(key), int(value)))


def default_params(**kw) -> OptParams:
    p = OptParams()
    lib().dpgo_hip_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ----------------------------------------------------------------------------------------
# Layout helpers: the C ABI uses the reference's column-major r x (b n) layout.
# ----------------------------------------------------------------------------------------
def to_dev_layout(X: np.ndarray) -> np.ndarray:
    """r x (b n) matrix -> flat column-major buffer."""
    return np.ascontiguousarray(np.asarray(X, dtype=np.float64).T).ravel()


def from_dev_layout(a: np.ndarray, r: int) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a).reshape(-1, r).T)


class Problem:
    """Batched QuadraticProblem handle (one agent = the reference's QuadraticProblem)."""

    def __init__(self, n, d, r, poses_per_agent=None):
        self.d, self.r, self.b = d, r, d + 1
        h = C.c_void_p()
        if poses_per_agent is None:
            _check(lib().dpgo_hip_problem_create(int(n), d, r, C.byref(h)))
            self.poses = [int(n)]
        else:
            arr, ptr = _i32(poses_per_agent)
            _check(lib().dpgo_hip_problem_create_batch(len(arr), ptr, d, r, C.byref(h)))
            self.poses = [int(x) for x in arr]
        self.h = h
        self.K = len(self.poses)
        self.N = int(sum(self.poses))
        self.offsets = np.concatenate([[0], np.cumsum(self.poses)]).astype(np.int64)

    def close(self):
        if getattr(self, "h", None):
            lib().dpgo_hip_problem_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def vec_len(self):
        return self.N * self.r * self.b

    def set_stream(self, stream_ptr: int | None):
        _check(lib().dpgo_hip_problem_set_stream(self.h, C.c_void_p(stream_ptr or 0)))

    def set_precon(self, mode):
        _check(lib().dpgo_hip_set_precon(self.h, mode))

    def set_Q_bsr(self, agent, browptr, bcol, blocks_colmajor):
        rp, rpp = _i32(browptr)
        cc, ccp = _i32(bcol)
        bb, bbp = _f64(blocks_colmajor)
        self._keep = (rp, cc, bb)
        _check(lib().dpgo_hip_set_Q_bsr(self.h, agent, len(rp) - 1, rpp, ccp, bbp))

    def set_Q_csr(self, agent, indptr, indices, data):
        rp, rpp = _i32(indptr)
        cc, ccp = _i32(indices)
        dd, ddp = _f64(data)
        _check(lib().dpgo_hip_set_Q_csr(self.h, agent, len(rp) - 1, rpp, ccp, ddp))

    def set_Q_scipy(self, agent, Q):
        """Q: scipy sparse (b n_a x b n_a) symmetric; uploaded as BSR with column-major blocks."""
        import scipy.sparse as sp
        Qb = sp.bsr_matrix(Q, blocksize=(self.b, self.b))
        Qb.sort_indices()
        self.set_Q_bsr(agent, Qb.indptr, Qb.indices, np.ascontiguousarray(Qb.data.transpose(0, 2, 1)))

    def set_Q_edges(self, agent, p1, p2, R, t, kappa, tau, weight=None):
        """Q of one agent from its measurements (agent-local endpoints, -1 = other agent)."""
        a1, a1p = _i32(p1)
        a2, a2p = _i32(p2)
        Rr, Rp = _f64(np.asarray(R, dtype=np.float64).reshape(-1))
        tt, tp = _f64(np.asarray(t, dtype=np.float64).reshape(-1))
        kk, kp = _f64(kappa)
        ta, tap = _f64(tau)
        if weight is not None:
            ww, wp = _f64(weight)
        else:
            wp = None
        _check(lib().dpgo_hip_set_Q_edges(self.h, agent, len(a1), a1p, a2p, Rp, tp, kp, tap, wp))

    def set_edge_weights_dev(self, w_dev_ptr: int):
        _check(lib().dpgo_hip_set_edge_weights_dev(self.h, C.c_void_p(w_dev_ptr)))

    def set_G_dense(self, agent, G):
        """G: r x (b n_a) matrix."""
        g, gp = _f64(to_dev_layout(G))
        _check(lib().dpgo_hip_set_G_dense(self.h, agent, gp))

    def set_G_blocks(self, agent, pose_idx, blocks):
        """blocks: (count, r, b) pose blocks."""
        idx, ip = _i32(pose_idx)
        bl = np.ascontiguousarray(np.asarray(blocks, dtype=np.float64).transpose(0, 2, 1)).ravel()
        bl, bp = _f64(bl)
        _check(lib().dpgo_hip_set_G(self.h, agent, len(idx), ip, bp))

    # --- evaluations on host matrices (r x (b N)) ----------------------------------------
    def _in(self, X):
        return _f64(to_dev_layout(X))

    def _out(self):
        o = np.empty(self.vec_len)
        return o, o.ctypes.data_as(_dp)

    def f(self, X):
        x, xp = self._in(X)
        out = np.empty(self.K)
        _check(lib().dpgo_hip_f(self.h, xp, out.ctypes.data_as(_dp)))
        return out

    def egrad(self, X):
        x, xp = self._in(X)
        o, op = self._out()
        _check(lib().dpgo_hip_egrad(self.h, xp, op))
        return from_dev_layout(o, self.r)

    def ehvp(self, V):
        x, xp = self._in(V)
        o, op = self._out()
        _check(lib().dpgo_hip_ehvp(self.h, xp, op))
        return from_dev_layout(o, self.r)

    def riegrad(self, X):
        x, xp = self._in(X)
        o, op = self._out()
        norms = np.empty(self.K)
        fv = np.empty(self.K)
        _check(lib().dpgo_hip_riegrad(self.h, xp, op, norms.ctypes.data_as(_dp), fv.ctypes.data_as(_dp)))
        return from_dev_layout(o, self.r), norms, fv

    def rhvp(self, X, V):
        x, xp = self._in(X)
        v, vp = self._in(V)
        o, op = self._out()
        _check(lib().dpgo_hip_rhvp(self.h, xp, vp, op))
        return from_dev_layout(o, self.r)

    def precondition(self, X, V):
        x, xp = self._in(X)
        v, vp = self._in(V)
        o, op = self._out()
        _check(lib().dpgo_hip_precondition(self.h, xp, vp, op))
        return from_dev_layout(o, self.r)

    def optimize(self, X, params: OptParams | None = None):
        x, xp = self._in(X)
        o, op = self._out()
        res = (OptResult * self.K)()
        p = params or default_params()
        _check(lib().dpgo_hip_optimize(self.h, C.byref(p), xp, op, res))
        return from_dev_layout(o, self.r), [r.as_dict() for r in res]

    # --- device pointers ---------------------------------------------------------------------
    def optimize_dev(self, X_dev: int, X_out_dev: int, params: OptParams | None = None, enabled=None,
                     want_results=True):
        """want_results=False: no statistics (the RBCD engine's call: f(x2) only, direct X_out)."""
        res = (OptResult * self.K)() if want_results else None
        p = params or default_params()
        if enabled is not None:
            en, enp = _i32(enabled)
        else:
            enp = None
        _check(lib().dpgo_hip_optimize_dev(self.h, C.byref(p), C.c_void_p(X_dev), C.c_void_p(X_out_dev),
                                           enp, res))
        return [r.as_dict() for r in res] if want_results else None

    def project_polar_dev(self, in_dev, out_dev):
        """out = LiftedSEManifold::project(in) on device pointers, queued on the handle's stream."""
        _check(lib().dpgo_hip_project_polar_dev(self.h, C.c_void_p(in_dev), C.c_void_p(out_dev)))

    def polar_combine_dev(self, A_dev, B_dev, ca, cb, out_dev):
        """out = project(ca[k] A + cb[k] B) per agent k (B_dev None: project(ca[k] A)) on device pointers."""
        a, ap = _f64(ca)
        if B_dev is not None:
            b, bp = _f64(cb)
        else:
            bp = None
        _check(lib().dpgo_hip_polar_combine_dev(self.h, C.c_void_p(A_dev), C.c_void_p(B_dev or 0), ap, bp,
                                                C.c_void_p(out_dev)))

    def certify(self, X, max_iters=300, tol=1e-8, want_vector=False, basis=0, seed_x=False):
        """lambda_min of S(X) = Q - Lambda(X) (Lanczos on the device): (lambda_min, residual, iters, vec).
        basis > 0: thick restart at that basis size; seed_x: the rows of X in the start block
        (dpgo_hip_certify_ex)."""
        x, xp = self._in(X)
        lam, info = C.c_double(), CertInfo()
        v = np.empty(self.vec_len) if want_vector else None
        _check(lib().dpgo_hip_certify_ex(self.h, xp, int(max_iters), int(basis), 1 if seed_x else 0, float(tol),
                                         C.byref(lam), v.ctypes.data_as(_dp) if v is not None else None,
                                         C.byref(info)))
        self.last_certificate = info.as_dict()
        return lam.value, info.residual, info.iters, (from_dev_layout(v, self.r) if v is not None else None)

    def certify_chol(self, X, sigma):
        """True iff the device Cholesky factorisation of S(X) + sigma I met no non-positive pivot: lambda_min(S(X)) >
        -sigma up to its backward error (dpgo_hip_certify_chol; single agent, edge-stream Q)."""
        x, xp = self._in(X)
        pd = C.c_int(-1)
        _check(lib().dpgo_hip_certify_chol(self.h, xp, float(sigma), C.byref(pd)))
        return bool(pd.value)

    def certify_chol_ex(self, X, eta, want_vector=True, **params):
        """The certificate by factorisation (dpgo_hip_certify_chol_ex): dict(lambda_min, certified, factorisations,
        sigma_lo, sigma_hi, invit_iters, residual, factor_ms, panel_doubles[, eigvec r x (d+1) n: the unit vector on
        row 0]).  Certified (S(X) + eta I positive definite): lambda_min = -eta, no eigvec.  params: the fields of
        dpgo_chol_cert_params."""
        x, xp = self._in(X)
        lam, info = C.c_double(), CholCertInfo()
        v = np.empty(self.vec_len) if want_vector else None
        _check(lib().dpgo_hip_certify_chol_ex(self.h, xp, float(eta), C.byref(chol_cert_params(**params)),
                                              C.byref(lam), v.ctypes.data_as(_dp) if v is not None else None,
                                              C.byref(info)))
        out = dict(lambda_min=lam.value, **info.as_dict())
        if v is not None and not info.certified:
            out["eigvec"] = from_dev_layout(v, self.r)
        return out

    def certify_block(self, X, want_vector=True, **params):
        """The block certificate (dpgo_hip_certify_block: LOBPCG on the r lifted rows, any Q format and weights, any
        size): dict(lambda_min, lower_bound and the other dpgo_cert_info fields[, eigvec r x (d+1) n: the unit vector
        on row 0]).  params: the fields of dpgo_block_cert_params."""
        x, xp = self._in(X)
        lam, info = C.c_double(), CertInfo()
        v = np.empty(self.vec_len) if want_vector else None
        _check(lib().dpgo_hip_certify_block(self.h, xp, C.byref(block_cert_params(**params)), C.byref(lam),
                                            v.ctypes.data_as(_dp) if v is not None else None, C.byref(info)))
        out = dict(lambda_min=lam.value, **info.as_dict())
        if v is not None:
            out["eigvec"] = from_dev_layout(v, self.r)
        return out

    def escape(self, X, v, lambda_min, params: "EscapeParams | None" = None):
        """The rank staircase's escape with its line search on this handle (single agent, rank r + 1, Q set): X
        (r x (d+1) n) a critical point of rank r = self.r - 1, v the unit eigenvector of lambda_min(S(X)) < 0.
        Returns (X_out (r+1) x (d+1) n, info dict); not accepted: X_out = [X; 0] (dpgo_hip_escape)."""
        X = np.asarray(X, dtype=np.float64)
        if X.shape != (self.r - 1, self.b * self.N):
            raise DPGOHipError(f"escape: X must be {self.r - 1} x {self.b * self.N} for this rank-{self.r} handle")
        x, xp = _f64(to_dev_layout(X))
        vv, vp = _f64(np.asarray(v, dtype=np.float64).ravel())
        if vv.size != self.b * self.N:
            raise DPGOHipError("escape: v must have (d+1) n entries")
        o, op = self._out()
        info = EscapeInfo()
        _check(lib().dpgo_hip_escape(self.h, xp, vp, float(lambda_min), C.byref(params) if params else None, op,
                                     C.byref(info)))
        return from_dev_layout(o, self.r), info.as_dict()

    def spmm_bytes(self) -> float:
        return float(lib().dpgo_hip_spmm_bytes(self.h))

    def bench_spmm(self, X_dev: int, Y_dev: int, reps: int) -> float:
        ms = C.c_double()
        _check(lib().dpgo_hip_bench_spmm(self.h, C.c_void_p(X_dev), C.c_void_p(Y_dev), reps, C.byref(ms)))
        return ms.value

    def synchronize(self):
        _check(lib().dpgo_hip_synchronize(self.h))

    def stats(self):
        """Cumulative solver counters per agent: list of dicts (STATS_FIELDS)."""
        out = np.zeros(self.K * STATS_INTS, np.int32)
        _check(lib().dpgo_hip_stats(self.h, out.ctypes.data_as(_ip)))
        return [dict(zip(STATS_FIELDS, (int(v) for v in out[a * STATS_INTS:(a + 1) * STATS_INTS])))
                for a in range(self.K)]

    def set_trace(self, capacity):
        _check(lib().dpgo_hip_set_trace(self.h, int(capacity)))
        self._trace_cap = int(capacity)

    def exact_factor_info(self):
        """The exact preconditioner's factor: supernodes, levels, widest separator (64-row tiles), panel doubles,
        last device factorisation ms, device factorisations so far."""
        n, lv, mt, pd, ms, cnt = C.c_longlong(), C.c_int(), C.c_int(), C.c_longlong(), C.c_double(), C.c_int()
        _check(lib().dpgo_hip_exact_factor_info(self.h, C.byref(n), C.byref(lv), C.byref(mt), C.byref(pd), C.byref(ms),
                                                C.byref(cnt)))
        fl, ifl = C.c_double(), C.c_double()
        _check(lib().dpgo_hip_exact_factor_flops(self.h, C.byref(fl), C.byref(ifl)))
        return {"nodes": n.value, "levels": lv.value, "max_s_tiles": mt.value, "panel_doubles": pd.value,
                "factor_ms": ms.value, "factor_count": cnt.value, "cholesky_flops": fl.value,
                "inverse_flops": ifl.value}

    def exact_fallback_agents(self):
        """Per agent 1 where the last exact factorisation met a non-positive pivot (that agent's preconditioner is
        the identity, src/QuadraticProblem.cpp:81-86; the other agents keep their factors)."""
        flags = np.zeros(self.K, np.int32)
        cnt = C.c_int()
        _check(lib().dpgo_hip_exact_fallback_agents(self.h, flags.ctypes.data_as(_ip), C.byref(cnt)))
        assert int(flags.sum()) == cnt.value
        return flags

    def set_tuning(self, key, value):
        """A tuning key on this handle only (dpgo_hip_problem_set_tuning)."""
        _check(lib().dpgo_hip_problem_set_tuning(self.h, int(key), int(value)))

    def get_trace(self, agent=0):
        """Per-iteration records of one agent: list of dicts (TRACE_FIELDS)."""
        cap = getattr(self, "_trace_cap", 0)
        buf = np.zeros(max(cap, 1) * TRACE_WIDTH)
        n = C.c_int()
        _check(lib().dpgo_hip_get_trace(self.h, int(agent), buf.ctypes.data_as(_dp), cap, C.byref(n)))
        k = min(n.value, cap)
        return [dict(zip(TRACE_FIELDS, buf[i * TRACE_WIDTH:(i + 1) * TRACE_WIDTH].tolist())) for i in range(k)]


def tangent_project(X, V, d):
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    x, xp = _f64(to_dev_layout(X))
    v, vp = _f64(to_dev_layout(V))
    o = np.empty_like(x)
    _check(lib().dpgo_hip_tangent_project(r, d, n, xp, vp, o.ctypes.data_as(_dp)))
    return from_dev_layout(o, r)


def retract_qf(X, V, d, scale=1.0):
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    x, xp = _f64(to_dev_layout(X))
    v, vp = _f64(to_dev_layout(V))
    o = np.empty_like(x)
    _check(lib().dpgo_hip_retract_qf(r, d, n, xp, vp, scale, o.ctypes.data_as(_dp)))
    return from_dev_layout(o, r)


def project_polar(M, d):
    r = M.shape[0]
    n = M.shape[1] // (d + 1)
    x, xp = _f64(to_dev_layout(M))
    o = np.empty_like(x)
    _check(lib().dpgo_hip_project_polar(r, d, n, xp, o.ctypes.data_as(_dp)))
    return from_dev_layout(o, r)


def round_se(X, d, anchor=None):
    """SE(d) rounding of the lifted poses X (r x (d+1) n) in the frame of the lifted pose `anchor` (r x (d+1); None =
    pose 0 of X, PGOAgent::getTrajectoryInLocalFrame): d x (d+1) n, [R_j | t_j] per pose."""
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    x, xp = _f64(to_dev_layout(X))
    ap = None
    if anchor is not None:
        a, ap = _f64(to_dev_layout(anchor))
    o = np.empty(n * d * (d + 1))
    _check(lib().dpgo_hip_round_se(r, d, n, xp, ap, o.ctypes.data_as(_dp)))
    return from_dev_layout(o, d)


def round_se_dev(r, d, n, X_dev: int, anchor_dev: int | None, T_dev: int, stream_ptr: int | None = None):
    """round_se on device pointers, queued on `stream_ptr` (None = the null stream) without synchronisation."""
    _check(lib().dpgo_hip_round_se_dev(int(r), int(d), int(n), C.c_void_p(X_dev), C.c_void_p(anchor_dev or 0),
                                       C.c_void_p(T_dev), C.c_void_p(stream_ptr or 0)))


def _ylift_colmajor(YLift, r, d):
    Y = np.asarray(YLift, dtype=np.float64)
    if Y.shape != (r, d):
        raise DPGOHipError(f"YLift must be r x d = {r} x {d}")
    return _f64(Y.T.ravel())


def frame_lift(T, YLift, frames=None, frame_of=None):
    """The inverse of round_se: X (r x (d+1) n) = YLift [F_R R_j | F_R t_j + F_t] per pose of the SE(d) trajectory T
    (d x (d+1) n), F = frames[frame_of[j]] (frames: nf x d x (d+1), each [F_R | F_t]; frame_of: one int per pose).
    frames and frame_of both None: X = YLift T."""
    T = np.asarray(T, dtype=np.float64)
    d = T.shape[0]
    n = T.shape[1] // (d + 1)
    r = np.asarray(YLift).shape[0]
    t, tp = _f64(to_dev_layout(T))
    Y, Yp = _ylift_colmajor(YLift, r, d)
    fp, fop, nf = None, None, 0
    if frames is not None:
        F = np.asarray(frames, dtype=np.float64).reshape(-1, d, d + 1)
        nf = F.shape[0]
        f, fp = _f64(np.ascontiguousarray(F.transpose(0, 2, 1)).ravel())  # column-major per frame
    if frame_of is not None:
        fo, fop = _i32(frame_of)
        if fo.size != n:
            raise DPGOHipError("frame_lift: frame_of must have one entry per pose")
    o = np.empty(n * r * (d + 1))
    _check(lib().dpgo_hip_frame_lift(r, d, n, tp, Yp, fp, nf, fop, o.ctypes.data_as(_dp)))
    return from_dev_layout(o, r)


def frame_lift_dev(r, d, n, T_dev: int, YLift, frames_dev: int | None, nf, frame_of_dev: int | None, X_out_dev: int,
                   stream_ptr: int | None = None):
    """frame_lift on device pointers (YLift: the host r x d matrix), queued on `stream_ptr` (None = the null stream)
    without synchronisation."""
    Y, Yp = _ylift_colmajor(YLift, int(r), int(d))
    _check(lib().dpgo_hip_frame_lift_dev(int(r), int(d), int(n), C.c_void_p(T_dev), Yp, C.c_void_p(frames_dev or 0),
                                         int(nf), C.c_void_p(frame_of_dev or 0), C.c_void_p(X_out_dev),
                                         C.c_void_p(stream_ptr or 0)))


def escape_params(**kw) -> EscapeParams:
    p = EscapeParams()
    lib().dpgo_hip_default_escape_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def lift_escape(X, d, v=None, alpha=1.0):
    """Retr_[X; 0](alpha [0; v^T]) of the lifted poses X (r x (d+1) n) along the (d+1) n vector v, at rank r + 1:
    per pose [qf([Y_j; alpha v_Y^T]) | (p_j; alpha v_p)].  v None: the plain lift [X; 0].  (r+1) x (d+1) n."""
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    x, xp = _f64(to_dev_layout(X))
    vp = None
    if v is not None:
        vv, vp = _f64(np.asarray(v, dtype=np.float64).ravel())
        if vv.size != (d + 1) * n:
            raise DPGOHipError("lift_escape: v must have (d+1) n entries")
    o = np.empty(n * (r + 1) * (d + 1))
    _check(lib().dpgo_hip_lift_escape(r, d, n, xp, vp, float(alpha), o.ctypes.data_as(_dp)))
    return from_dev_layout(o, r + 1)


def lift_escape_dev(r, d, n, X_dev: int, v_dev: int | None, alpha, X_out_dev: int, stream_ptr: int | None = None):
    """lift_escape on device pointers, queued on `stream_ptr` (None = the null stream) without synchronisation."""
    _check(lib().dpgo_hip_lift_escape_dev(int(r), int(d), int(n), C.c_void_p(X_dev), C.c_void_p(v_dev or 0),
                                          float(alpha), C.c_void_p(X_out_dev), C.c_void_p(stream_ptr or 0)))


def escape_direction(vec, d):
    """The unit escape direction ((d+1) n) from the certificate's Ritz matrix (r x (d+1) n: its row of largest
    norm) or from a plain (d+1) n vector.  Host only."""
    V = np.asarray(vec, dtype=np.float64)
    V = V.reshape(1, -1) if V.ndim == 1 else V
    r, n = V.shape[0], V.shape[1] // (d + 1)
    x, xp = _f64(to_dev_layout(V))
    out = np.empty(V.shape[1])
    _check(lib().dpgo_hip_escape_direction(r, d, n, xp, out.ctypes.data_as(_dp)))
    return out


def gram(X, d):
    """C = sum_j Y_j Y_j^T (r x r) over the rotation columns of the lifted poses X (r x (d+1) n), on the device: a
    function of (X, n) alone, bitwise repeatable."""
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    x, xp = _f64(to_dev_layout(X))
    o = np.empty(r * r)
    _check(lib().dpgo_hip_gram(r, d, n, xp, o.ctypes.data_as(_dp)))
    return o.reshape(r, r).T.copy()


def gram_work_doubles(r, d, n) -> int:
    """doubles of the work buffer gram_dev needs."""
    return int(lib().dpgo_hip_gram_work_doubles(int(r), int(d), int(n)))


def gram_dev(r, d, n, X_dev: int, C_dev: int, work_dev: int, stream_ptr: int | None = None):
    """gram on device pointers (C_dev: r r doubles, column-major; work_dev: gram_work_doubles), queued on `stream_ptr`
    (None = the null stream) without synchronisation."""
    _check(lib().dpgo_hip_gram_dev(int(r), int(d), int(n), C.c_void_p(X_dev), C.c_void_p(C_dev), C.c_void_p(work_dev),
                                   C.c_void_p(stream_ptr or 0)))


def gram_eig(Cm):
    """(w, U) of the symmetric r x r matrix Cm (r <= 8) by cyclic Jacobi: w descending, U's columns the eigenvectors,
    each with its largest-magnitude entry positive.  Host only."""
    Cm = np.asarray(Cm, dtype=np.float64)
    if Cm.ndim != 2 or Cm.shape[0] != Cm.shape[1]:
        raise DPGOHipError("gram_eig: C must be square")
    r = Cm.shape[0]
    c, cp = _f64(Cm.T.ravel())
    w = np.empty(max(r, 1))
    U = np.empty(max(r * r, 1))
    _check(lib().dpgo_hip_gram_eig(r, cp, w.ctypes.data_as(_dp), U.ctypes.data_as(_dp)))
    return w[:r].copy(), U[:r * r].reshape(r, r).T.copy()


def numerical_rank(w, d, tol):
    """k = max(d, #{i : w_i > tol w_1}) of a descending spectrum w."""
    w = np.asarray(w)
    return max(int(d), int(np.count_nonzero(w > tol * w[0])))


def _w_colmajor(W, r):
    W = np.asarray(W, dtype=np.float64)
    if W.ndim != 2 or W.shape[0] != r:
        raise DPGOHipError(f"W must be r x k with r = {r}")
    return W.shape[1], _f64(W.T.ravel())


def rank_reduce(X, d, W):
    """X truncated to rank k along W (r x k, orthonormal columns): per pose [polar(W^T Y_j) | W^T p_j], k x (d+1) n."""
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    k, (w, wp) = _w_colmajor(W, r)
    x, xp = _f64(to_dev_layout(X))
    o = np.empty(max(n * k * (d + 1), 1))
    _check(lib().dpgo_hip_rank_reduce(r, d, n, xp, k, wp, o.ctypes.data_as(_dp)))
    return from_dev_layout(o, k)


def rank_reduce_dev(r, d, n, X_dev: int, W, X_out_dev: int, stream_ptr: int | None = None):
    """rank_reduce on device pointers (W: the host r x k matrix), queued on `stream_ptr` (None = the null stream)
    without synchronisation."""
    k, (w, wp) = _w_colmajor(W, int(r))
    _check(lib().dpgo_hip_rank_reduce_dev(int(r), int(d), int(n), C.c_void_p(X_dev), k, wp, C.c_void_p(X_out_dev),
                                          C.c_void_p(stream_ptr or 0)))


def _edge_outputs(m, want):
    """The output arrays of an edge_errors call: want = names among err, rot_sq, tra_sq, cost (None = all)."""
    names = ("err", "rot_sq", "tra_sq", "cost")
    want = names if want is None else tuple(want)
    bad = [k for k in want if k not in names]
    if bad:
        raise DPGOHipError(f"edge_errors: unknown output {bad[0]}")
    out = {k: np.empty(1 if k == "cost" else max(int(m), 1)) for k in want}
    return out, [out[k].ctypes.data_as(_dp) if k in out else None for k in names]


def _edge_result(out, m):
    return {k: (float(v[0]) if k == "cost" else v[:m]) for k, v in out.items()}


def edge_errors(X, d, p1, p2, R, t, kappa, tau, w=None, outputs=None):
    """Per-measurement residuals of the poses X (r x (d+1) n: a lifted X or, at r = d, an SE(d) trajectory) on the
    device: dict(err, rot_sq, tra_sq, cost) with rot_sq = |Y1 R - Y2|_F^2, tra_sq = |p2 - p1 - Y1 t|^2,
    err = kappa rot_sq + tau tra_sq per edge and cost = 1/2 sum w err (w None = ones).  R: m x d x d (row-major per
    edge), t: m x d.  outputs: the subset of those names to compute (None = all four)."""
    X = np.asarray(X, dtype=np.float64)
    r = X.shape[0]
    n = X.shape[1] // (d + 1)
    x, xp = _f64(to_dev_layout(X))
    a1, _ = _i32(p1)
    a2, _ = _i32(p2)
    m = a1.size
    Rr, _ = _f64(np.asarray(R).reshape(-1))
    tt, _ = _f64(np.asarray(t).reshape(-1))
    kk, _ = _f64(kappa)
    ta, _ = _f64(tau)
    if a2.size != m or Rr.size != m * d * d or tt.size != m * d or kk.size != m or ta.size != m:
        raise DPGOHipError("edge_errors: p1, p2, R, t, kappa, tau must describe the same m edges")
    ww = None
    if w is not None:
        ww, _ = _f64(w)
        if ww.size != m:
            raise DPGOHipError("edge_errors: w must have one entry per edge")
    E = Edges(m, a1.ctypes.data, a2.ctypes.data, Rr.ctypes.data, tt.ctypes.data, kk.ctypes.data, ta.ctypes.data,
              ww.ctypes.data if ww is not None else None)
    out, ptrs = _edge_outputs(m, outputs)
    _check(lib().dpgo_hip_edge_errors(r, d, n, C.byref(E), xp, *ptrs))
    return _edge_result(out, m)


def edge_errors_work_doubles(m) -> int:
    """doubles of the work buffer edge_errors_dev needs for the cost of m edges."""
    return int(lib().dpgo_hip_edge_errors_work_doubles(int(m)))


def edge_errors_dev(r, d, n, m, p1_dev: int, p2_dev: int, R_dev: int, t_dev: int, kappa_dev: int, tau_dev: int,
                    w_dev: int | None, X_dev: int, err_dev: int | None = None, rot_sq_dev: int | None = None,
                    tra_sq_dev: int | None = None, cost_dev: int | None = None, work_dev: int | None = None,
                    stream_ptr: int | None = None):
    """edge_errors on device pointers (int32 indices, trusted; work_dev: edge_errors_work_doubles, needed with
    cost_dev), queued on `stream_ptr` (None = the null stream) without synchronisation."""
    E = Edges(int(m), p1_dev, p2_dev, R_dev, t_dev, kappa_dev, tau_dev, w_dev or None)
    _check(lib().dpgo_hip_edge_errors_dev(int(r), int(d), int(n), C.byref(E), C.c_void_p(X_dev),
                                          C.c_void_p(err_dev or 0), C.c_void_p(rot_sq_dev or 0),
                                          C.c_void_p(tra_sq_dev or 0), C.c_void_p(cost_dev or 0),
                                          C.c_void_p(work_dev or 0), C.c_void_p(stream_ptr or 0)))


# ---- trajectory evaluation against a ground truth (dpgo_hip_traj_*, include/dpgo_hip.h) ----
TRAJ_SUMS = 5


def traj_moments_len(d) -> int:
    """DPGO_TRAJ_MOMENTS(d)."""
    return 3 + 2 * d + d * d


def _traj_flat(T, d, what="trajectory"):
    """A d x (d+1) n matrix, or the flat column-major buffer of one, as (flat float64 buffer, n)."""
    T = np.asarray(T, dtype=np.float64)
    flat = np.ascontiguousarray(T.T).ravel() if T.ndim == 2 else np.ascontiguousarray(T).ravel()
    if (T.ndim == 2 and T.shape[0] != d) or flat.size % (d * (d + 1)) != 0:
        raise DPGOHipError(f"{what}: need d x (d+1) n with d = {d}")
    return flat, flat.size // (d * (d + 1))


def _traj_pair(That, T, d, use):
    a, n = _traj_flat(That, d, "That")
    b, nb = _traj_flat(T, d, "T")
    if nb != n:
        raise DPGOHipError("That and T must have the same number of poses")
    u = None
    if use is not None:
        u, _ = _i32(use)
        if u.size != n:
            raise DPGOHipError("use must have one entry per pose")
    return a, b, u, n


def _opt_ptr(a, ptype=_dp):
    return a.ctypes.data_as(ptype) if a is not None else None


def _opt_vec(v, size, what):
    if v is None:
        return None
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel())
    if a.size != size:
        raise DPGOHipError(f"{what} must have {size} entries")
    return a


def traj_moments(That, T, d, use=None, shift=None):
    """mom = [count, sum |a|^2, sum |b|^2, sum a, sum b, M = sum b a^T (column-major)] of the translations of the
    estimate That and the truth T (d x (d+1) n each) about shift = (s^, s) (2 d, None = zeros), over the poses with
    use[j] != 0 (None = all), on the device: bitwise repeatable, additive over disjoint pose sets."""
    a, b, u, n = _traj_pair(That, T, d, use)
    s = _opt_vec(shift, 2 * d, "shift")
    mom = np.empty(traj_moments_len(d))
    _check(lib().dpgo_hip_traj_moments(int(d), n, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), _opt_ptr(u, _ip),
                                       _opt_ptr(s), mom.ctypes.data_as(_dp)))
    return mom


def traj_moments_work_doubles(d, n) -> int:
    return int(lib().dpgo_hip_traj_moments_work_doubles(int(d), int(n)))


def traj_moments_dev(d, n, That_dev: int, T_dev: int, use_dev: int | None, shift, mom_dev: int, work_dev: int,
                     stream_ptr: int | None = None):
    """traj_moments on device pointers (shift: host, None = zeros; work_dev: traj_moments_work_doubles), queued on
    `stream_ptr` (None = the null stream) without synchronisation."""
    s = _opt_vec(shift, 2 * int(d), "shift")
    _check(lib().dpgo_hip_traj_moments_dev(int(d), int(n), C.c_void_p(That_dev), C.c_void_p(T_dev),
                                           C.c_void_p(use_dev or 0), _opt_ptr(s), C.c_void_p(mom_dev),
                                           C.c_void_p(work_dev), C.c_void_p(stream_ptr or 0)))


def _align_result(d, Aa, info):
    return Aa.reshape(d + 1, d).T.copy(), dict(count=info.count, sigma=np.array(info.sigma[:d]), rank=info.rank)


def align_moments(d, mom, shift=None, rank_tol=1e-12):
    """(Aa, info) from traj_moments' vector (the sum of the ranks' vectors): Aa = [A | a] (d x (d+1)) minimises
    sum |A t^_j + a - t_j|^2 over SE(d); info = dict(count, sigma (descending, the last signed by det(U V^T)),
    rank = #{sigma_i > rank_tol sigma_1}).  Host only."""
    m = _opt_vec(mom, traj_moments_len(d), "mom")
    s = _opt_vec(shift, 2 * d, "shift")
    Aa, info = np.empty(d * (d + 1)), AlignInfo()
    _check(lib().dpgo_hip_align_moments(int(d), _opt_ptr(s), _opt_ptr(m), float(rank_tol), Aa.ctypes.data_as(_dp),
                                        C.byref(info)))
    return _align_result(d, Aa, info)


def traj_align(That, T, d, use=None):
    """(Aa, info) of align_moments from two moment launches on the device: the first gives the means, the second
    takes the moments about them."""
    a, b, u, n = _traj_pair(That, T, d, use)
    Aa, info = np.empty(d * (d + 1)), AlignInfo()
    _check(lib().dpgo_hip_traj_align(int(d), n, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), _opt_ptr(u, _ip),
                                     Aa.ctypes.data_as(_dp), C.byref(info)))
    return _align_result(d, Aa, info)


def _aa_colmajor(Aa, d):
    if Aa is None:
        return None
    A = np.asarray(Aa, dtype=np.float64)
    if A.shape != (d, d + 1):
        raise DPGOHipError(f"Aa must be d x (d+1) = {d} x {d + 1}")
    return np.ascontiguousarray(A.T).ravel()


def traj_errors(That, T, d, use=None, Aa=None, outputs=None):
    """Per-pose errors of That against T under Aa = [A | a] (d x (d+1), None = identity), on the device:
    dict(tra_sq [n] = |A t^_j + a - t_j|^2, rot_sq [n] = |A R^_j - R_j|_F^2, sums = [count, sum tra_sq, sum rot_sq,
    max tra_sq, max rot_sq]); an unused pose has NaN and takes no part in sums.  outputs: the subset of those names
    to compute (None = all three)."""
    a, b, u, n = _traj_pair(That, T, d, use)
    names = ("tra_sq", "rot_sq", "sums")
    want = names if outputs is None else tuple(outputs)
    bad = [k for k in want if k not in names]
    if bad:
        raise DPGOHipError(f"traj_errors: unknown output {bad[0]}")
    out = {k: np.empty(TRAJ_SUMS if k == "sums" else n) for k in want}
    A = _aa_colmajor(Aa, d)
    _check(lib().dpgo_hip_traj_errors(int(d), n, a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), _opt_ptr(u, _ip),
                                      _opt_ptr(A), *[_opt_ptr(out.get(k)) for k in names]))
    return out


def traj_errors_work_doubles(d, n) -> int:
    return int(lib().dpgo_hip_traj_errors_work_doubles(int(d), int(n)))


def traj_errors_dev(d, n, That_dev: int, T_dev: int, use_dev: int | None, Aa, tra_sq_dev: int | None = None,
                    rot_sq_dev: int | None = None, sums_dev: int | None = None, work_dev: int | None = None,
                    stream_ptr: int | None = None):
    """traj_errors on device pointers (Aa: host, None = identity; work_dev: traj_errors_work_doubles, needed with
    sums_dev), queued on `stream_ptr` (None = the null stream) without synchronisation."""
    A = _aa_colmajor(Aa, int(d))
    _check(lib().dpgo_hip_traj_errors_dev(int(d), int(n), C.c_void_p(That_dev), C.c_void_p(T_dev),
                                          C.c_void_p(use_dev or 0), _opt_ptr(A), C.c_void_p(tra_sq_dev or 0),
                                          C.c_void_p(rot_sq_dev or 0), C.c_void_p(sums_dev or 0),
                                          C.c_void_p(work_dev or 0), C.c_void_p(stream_ptr or 0)))


def relative_poses(T, d, p1, p2):
    """(R [m x d x d], t [m x d]) of the trajectory T (d x (d+1) n) over the edges (p1, p2), on the device:
    R[e] = R_p1^T R_p2, t[e] = R_p1^T (t_p2 - t_p1), the form edge_errors takes measurements in."""
    a, n = _traj_flat(T, d, "T")
    a1, a1p = _i32(p1)
    a2, a2p = _i32(p2)
    m = a1.size
    if a2.size != m:
        raise DPGOHipError("relative_poses: p1 and p2 must have the same length")
    R, t = np.empty(max(m, 1) * d * d), np.empty(max(m, 1) * d)
    _check(lib().dpgo_hip_relative_poses(int(d), n, a.ctypes.data_as(_dp), m, a1p, a2p, R.ctypes.data_as(_dp),
                                         t.ctypes.data_as(_dp)))
    return R[:m * d * d].reshape(m, d, d), t[:m * d].reshape(m, d)


def relative_poses_dev(d, n, T_dev: int, m, p1_dev: int, p2_dev: int, R_out_dev: int, t_out_dev: int,
                       stream_ptr: int | None = None):
    """relative_poses on device pointers (int32 indices, trusted), queued on `stream_ptr` without synchronisation."""
    _check(lib().dpgo_hip_relative_poses_dev(int(d), int(n), C.c_void_p(T_dev), int(m), C.c_void_p(p1_dev),
                                             C.c_void_p(p2_dev), C.c_void_p(R_out_dev), C.c_void_p(t_out_dev),
                                             C.c_void_p(stream_ptr or 0)))


def rot_angle(rot_sq):
    """The angle (rad) of a chordal rotation error |A R^ - R|_F^2 for d = 2 and 3: 2 asin(min(1, sqrt(rot_sq / 8)))."""
    return 2.0 * np.arcsin(np.minimum(1.0, np.sqrt(np.asarray(rot_sq, dtype=np.float64) / 8.0)))


def merge_traj_sums(parts):
    """traj_errors' sums of disjoint pose sets (one per rank) as one: entries 0-2 add, 3-4 take the maximum."""
    P = np.asarray(parts, dtype=np.float64).reshape(-1, TRAJ_SUMS)
    return np.concatenate([P[:, :3].sum(axis=0), P[:, 3:].max(axis=0)])


def g2o_read_vertices(path, d, n):
    """(T [d x (d+1) n], present [n]) from the VERTEX_SE2 / VERTEX_SE3:QUAT lines of a g2o file: the quaternion is
    normalised (a reference pose must be a rotation); an absent id has present = 0 and NaN poses.  Host only."""
    T = np.empty(d * (d + 1) * int(n))
    present = np.empty(int(n), np.int32)
    _check(lib().dpgo_g2o_read_vertices(str(path).encode(), int(d), int(n), T.ctypes.data_as(_dp),
                                        present.ctypes.data_as(_ip)))
    return from_dev_layout(T, d), present


def grid3d_truth(k, seed=0):
    """The 3 x 4 k^3 ground-truth trajectory Graph.grid3d(k, seed, ..) measured.  Host only."""
    T = np.empty(12 * int(k) ** 3 if 2 <= int(k) <= 200 else 1)
    _check(lib().dpgo_graph_grid3d_truth(int(k), int(seed), T.ctypes.data_as(_dp)))
    return from_dev_layout(T, 3)


# ----------------------------------------------------------------------------------------
# Pose graphs + multi-agent RBCD engine (include/dpgo_rbcd.h)
# ----------------------------------------------------------------------------------------
class CertInfo(C.Structure):
    """dpgo_cert_info (include/dpgo_hip.h)."""
    _fields_ = [("iters", C.c_int), ("restarts", C.c_int), ("seeds", C.c_int), ("residual", C.c_double),
                ("lambda_seed", C.c_double), ("lambda_complement", C.c_double), ("residual_complement", C.c_double),
                ("coupling", C.c_double), ("lower_bound", C.c_double), ("ritz", C.c_double * 8)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "ritz"}
        d["ritz"] = [float(x) for x in self.ritz]
        return d


class RbcdParams(C.Structure):
    _fields_ = [("r", C.c_int), ("acceleration", C.c_int), ("restart_interval", C.c_int),
                ("max_inner", C.c_int), ("initial_radius", C.c_double), ("tolerance", C.c_double),
                ("precon", C.c_int), ("algorithm", C.c_int), ("q_format", C.c_int),
                ("robust_cost", C.c_int), ("robust_opt_inner_iters", C.c_int), ("gnc_max_iters", C.c_int),
                ("gnc_barc", C.c_double), ("gnc_mu_step", C.c_double), ("gnc_init_mu", C.c_double),
                ("huber_threshold", C.c_double), ("tls_threshold", C.c_double),
                ("status", C.c_int), ("rel_change_tol", C.c_double), ("min_convergence_ratio", C.c_double)]


class InitParams(C.Structure):
    """dpgo_init_params (include/dpgo_rbcd.h)."""
    _fields_ = [("local_init", C.c_int), ("align", C.c_int), ("max_rotation_error", C.c_double),
                ("gnc_max_iters", C.c_int), ("gnc_mu_step", C.c_double), ("use_gpu", C.c_int), ("rtol", C.c_double),
                ("max_iters", C.c_int), ("max_translation_error", C.c_double), ("clique_node_budget", C.c_longlong)]


class PcmInfo(C.Structure):
    """dpgo_pcm_info (include/dpgo_rbcd.h)."""
    _fields_ = [("groups", C.c_int), ("candidates", C.c_longlong), ("pair_tests", C.c_longlong),
                ("inliers", C.c_longlong), ("min_clique_ratio", C.c_double), ("unproven", C.c_int)]


LOCAL_INIT = {"chordal": 0, "odometry": 1}
ALIGN = {"l2": 0, "robust": 1, "pcm": 2}
EVAL_ALIGN = {"none": 0, "pose": 1, "lsq": 2}  # DPGO_ALIGN_NONE / _POSE / _LSQ of dpgo_graph_evaluate
_ubp = C.POINTER(C.c_ubyte)

_lp = C.POINTER(C.c_longlong)
_ullp = C.POINTER(C.c_ulonglong)
_SIGS2 = [
    ("dpgo_graph_read_g2o", [C.c_char_p, C.POINTER(C.c_void_p)], C.c_int),
    ("dpgo_graph_grid3d", [C.c_int, C.c_ulonglong, C.c_double, C.c_double, C.POINTER(C.c_void_p)], C.c_int),
    ("dpgo_graph_from_arrays", [C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp,
                                C.POINTER(C.c_void_p)], C.c_int),
    ("dpgo_graph_info", [C.c_void_p, _ip, _ip, _ip, _ip], C.c_int),
    ("dpgo_graph_copy_out", [C.c_void_p, _ip, _ip, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_graph_destroy", [C.c_void_p], C.c_int),
    ("dpgo_graph_laplacian_bsr", [C.c_void_p, _lp, _ip, _ip, _dp], C.c_int),
    ("dpgo_graph_chain_init", [C.c_void_p, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_graph_chordal_init", [C.c_void_p, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_chordal_initialization", [C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_graph_grid_partition", [C.c_void_p, C.c_int, _ip], C.c_int),
    ("dpgo_graph_certify", [C.c_void_p, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, _ip, _dp, _dp, _dp, _dp],
     C.c_int),
    ("dpgo_graph_certify_ex", [C.c_void_p, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp,
                               _dp, C.c_void_p], C.c_int),
    ("dpgo_graph_certify_chol", [C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.POINTER(CholCertParams), _dp, _dp, _dp,
                                 C.POINTER(CholCertInfo)], C.c_int),
    ("dpgo_graph_certify_block", [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(BlockCertParams), _dp, _dp, _dp,
                                  C.POINTER(CertInfo)], C.c_int),
    ("dpgo_graph_escape", [C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.c_double, C.POINTER(EscapeParams), _dp,
                           C.POINTER(EscapeInfo)], C.c_int),
    ("dpgo_graph_rank_reduce", [C.c_void_p, C.c_int, _dp, C.c_double, _ip, _dp, C.POINTER(RankInfo)], C.c_int),
    ("dpgo_graph_edge_errors", [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_graph_grid3d_truth", [C.c_int, C.c_ulonglong, _dp], C.c_int),
    ("dpgo_g2o_read_vertices", [C.c_char_p, C.c_int, C.c_int, _dp, _ip], C.c_int),
    ("dpgo_graph_evaluate", [C.c_void_p, C.c_int, _dp, _dp, _ip, C.c_int, C.c_int, C.POINTER(EvalInfo), _dp, _dp, _dp,
                             _dp], C.c_int),
    ("dpgo_rbcd_set_truth", [C.c_void_p, _dp, _ip], C.c_int),
    ("dpgo_rbcd_truth_moments", [C.c_void_p, _dp, _dp, _dp], C.c_int),
    ("dpgo_rbcd_truth_errors", [C.c_void_p, _dp, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_rbcd_get_errors", [C.c_void_p, C.c_void_p, C.c_int, _dp, _dp, _dp, _dp], C.c_int),
    ("dpgo_rbcd_gram", [C.c_void_p, _dp], C.c_int),
    ("dpgo_rbcd_get_X_reduced", [C.c_void_p, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_chordal_initialization_gpu", [C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, C.c_double,
                                         C.c_int, _dp, _ip, _dp], C.c_int),
    ("dpgo_graph_chordal_init_gpu", [C.c_void_p, C.c_int, _dp, C.c_double, C.c_int, _dp, _ip, _dp], C.c_int),
    ("dpgo_graph_distributed_init", [C.c_void_p, C.c_int, _ip, C.c_int, _dp, C.c_int, C.c_double, C.c_int, _dp, _ip,
                                     _dp], C.c_int),
    ("dpgo_robust_rotation_average", [C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_double, _dp, _dp, _ip],
     C.c_int),
    ("dpgo_default_init_params", [C.POINTER(InitParams)], None),
    ("dpgo_graph_distributed_init_ex", [C.c_void_p, C.c_int, _ip, C.POINTER(InitParams), _dp, _dp, _ip, _ip, _ip, _ubp,
                                        _ip, _dp], C.c_int),
    ("dpgo_graph_pcm", [C.c_void_p, C.c_int, _ip, _dp, C.POINTER(InitParams), _ubp, C.POINTER(PcmInfo)], C.c_int),
    ("dpgo_hip_pair_consistency_words", [C.c_int, _ip, _lp, C.c_longlong], C.c_int),
    ("dpgo_hip_pair_consistency", [C.c_int, C.c_int, _dp, _dp, C.c_int, _ip, C.c_double, C.c_double, _ullp,
                                   C.c_longlong, _ip, _dp, _dp], C.c_int),
    ("dpgo_hip_pair_consistency_dev", [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, _ip, C.c_double, C.c_double,
                                       C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
     C.c_int),
    ("dpgo_hip_pair_consistency_bench", [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, _ip, C.c_double, C.c_double,
                                         C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, _dp], C.c_int),
    ("dpgo_pair_consistency_host", [C.c_int, C.c_int, _dp, _dp, C.c_int, _ip, C.c_double, C.c_double, _ullp,
                                    C.c_longlong, _ip, _dp, _dp], C.c_int),
    ("dpgo_max_clique", [C.c_int, C.c_int, _ullp, C.c_longlong, _ip, _ip, _ip], C.c_int),
    ("dpgo_rbcd_default_params", [C.POINTER(RbcdParams)], None),
    ("dpgo_rbcd_plan", [C.c_void_p, C.c_int, _ip, _ip, C.c_int, C.c_int, _lp, _lp, _ip, _ip], C.c_int),
    ("dpgo_rbcd_create", [C.c_void_p, C.c_int, _ip, _ip, C.c_int, C.c_int, C.POINTER(RbcdParams),
                          C.POINTER(C.c_void_p)], C.c_int),
    ("dpgo_rbcd_destroy", [C.c_void_p], C.c_int),
    ("dpgo_rbcd_set_stream", [C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_rbcd_info", [C.c_void_p, _ip, _ip, _ip, _ip], C.c_int),
    ("dpgo_rbcd_color_of_agent", [C.c_void_p, _ip], C.c_int),
    ("dpgo_rbcd_exchange_counts", [C.c_void_p, _lp, _lp], C.c_int),
    ("dpgo_rbcd_set_X", [C.c_void_p, _dp], C.c_int),
    ("dpgo_rbcd_get_X", [C.c_void_p, _dp], C.c_int),
    ("dpgo_rbcd_set_trajectory", [C.c_void_p, _dp, _dp, _dp], C.c_int),
    ("dpgo_rbcd_get_anchor", [C.c_void_p, C.c_int, _dp, _ip], C.c_int),
    ("dpgo_rbcd_get_trajectory", [C.c_void_p, _dp, _dp], C.c_int),
    ("dpgo_rbcd_get_weights", [C.c_void_p, _dp], C.c_int),
    ("dpgo_rbcd_weight_owner", [C.c_void_p, C.c_int, _ip, _ip], C.c_int),
    ("dpgo_rbcd_pre_exchange", [C.c_void_p, C.c_int], C.c_int),
    ("dpgo_rbcd_pack", [C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_rbcd_update", [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OptResult)], C.c_int),
    ("dpgo_rbcd_set_selected", [C.c_void_p, _ip], C.c_int),
    ("dpgo_rbcd_bench_spmm", [C.c_void_p, C.c_int, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_rbcd_counters", [C.c_void_p, _lp, _lp], C.c_int),
    ("dpgo_rbcd_next_y_counters", [C.c_void_p, _lp, _lp], C.c_int),
    ("dpgo_rbcd_tcg_blocks", [C.c_void_p, C.c_int, _ip, _ip], C.c_int),
    ("dpgo_rbcd_spmm_bytes", [C.c_void_p, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_rbcd_bench_hvp", [C.c_void_p, C.c_int, C.c_int, _dp], C.c_int),
    ("dpgo_rbcd_reset_stream", [C.c_void_p], C.c_int),
    ("dpgo_rbcd_central_eval", [C.c_void_p, C.c_void_p, _dp, _dp], C.c_int),
    ("dpgo_rbcd_central_eval_ex", [C.c_void_p, C.c_void_p, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_rbcd_set_weights", [C.c_void_p, _dp, C.c_void_p], C.c_int),
    ("dpgo_rbcd_set_weights_dev", [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_rbcd_bench_set_weights", [C.c_void_p, C.c_int, C.c_int, _dp], C.c_int),
    ("dpgo_rbcd_status", [C.c_void_p, _dp, _ip], C.c_int),
    ("dpgo_rbcd_stats", [C.c_void_p, _ip], C.c_int),
    ("dpgo_rbcd_bytes", [C.c_void_p, _dp, _dp], C.c_int),
    ("dpgo_rbcd_mode_bytes", [C.c_void_p, C.c_int, _dp], C.c_int),
    ("dpgo_rccl_unique_id", [C.c_void_p], C.c_int),
    ("dpgo_rbcd_comm_init", [C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_rbcd_comm_attach", [C.c_void_p, C.c_void_p], C.c_int),
    ("dpgo_rbcd_comm_info", [C.c_void_p, _ip, _ip], C.c_int),
    ("dpgo_rbcd_exact_factor_info", [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int)], C.c_int),
    ("dpgo_rbcd_exact_factor_flops", [C.c_void_p, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_rbcd_bench_precond", [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp], C.c_int),
    ("dpgo_rbcd_exact_sweep_bytes", [C.c_void_p, C.c_int, _dp, _dp], C.c_int),
    ("dpgo_rbcd_exchange", [C.c_void_p, C.POINTER(C.c_void_p)], C.c_int),
    ("dpgo_rbcd_set_kernel_timing", [C.c_void_p, C.c_int], C.c_int),
    ("dpgo_rbcd_set_tuning", [C.c_void_p, C.c_int, C.c_int], C.c_int),
    ("dpgo_rbcd_set_trace", [C.c_void_p, C.c_int], C.c_int),
    ("dpgo_rbcd_get_trace", [C.c_void_p, C.c_int, _dp, C.c_int, _ip], C.c_int),
    ("dpgo_rbcd_kernel_times", [C.c_void_p, _dp, _lp], C.c_int),
    ("dpgo_rbcd_kernel_times_ex", [C.c_void_p, _dp, _lp, _dp], C.c_int),
    ("dpgo_rbcd_plan_color", [C.c_void_p, C.c_int, _ip, _ip, C.c_int, C.c_int, C.c_int, _lp, _lp, _ip, _ip], C.c_int),
    ("dpgo_rbcd_exchange_counts_color", [C.c_void_p, C.c_int, _lp, _lp], C.c_int),
    ("dpgo_rbcd_pack_color", [C.c_void_p, C.c_int, C.c_void_p], C.c_int),
    ("dpgo_rbcd_update_color", [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OptResult)], C.c_int),
    ("dpgo_rbcd_exchange_color", [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
]
_SIGS.extend(_SIGS2)
EXPORTED_SYMBOLS.extend(s[0] for s in _SIGS2)


class Graph:
    """Pose graph held by the native library (g2o reader / synthetic grid / arrays)."""

    def __init__(self, handle):
        self.h = handle
        d, n, m, dup = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _check(lib().dpgo_graph_info(self.h, C.byref(d), C.byref(n), C.byref(m), C.byref(dup)))
        self.d, self.n, self.m, self.duplicates = d.value, n.value, m.value, dup.value

    @classmethod
    def read_g2o(cls, path):
        h = C.c_void_p()
        _check(lib().dpgo_graph_read_g2o(path.encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def grid3d(cls, k, seed=0, rot_sigma=0.2, trans_sigma=0.1):
        h = C.c_void_p()
        _check(lib().dpgo_graph_grid3d(int(k), int(seed), rot_sigma, trans_sigma, C.byref(h)))
        g = cls(h)
        g._grid = (int(k), int(seed))
        return g

    def truth(self):
        """The ground-truth trajectory (3 x 4 n) a grid graph measured (grid3d_truth of its side and seed)."""
        if getattr(self, "_grid", None) is None:
            raise DPGOHipError("truth: not a grid graph")
        return grid3d_truth(*self._grid)

    @classmethod
    def from_arrays(cls, d, n, p1, p2, R, t, kappa, tau):
        a1, a1p = _i32(p1)
        a2, a2p = _i32(p2)
        Rr, Rp = _f64(np.asarray(R).reshape(-1))
        tt, tp = _f64(np.asarray(t).reshape(-1))
        kk, kp = _f64(kappa)
        ta, tap = _f64(tau)
        h = C.c_void_p()
        _check(lib().dpgo_graph_from_arrays(d, int(n), len(a1), a1p, a2p, Rp, tp, kp, tap, C.byref(h)))
        return cls(h)

    def close(self):
        if getattr(self, "h", None):
            lib().dpgo_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def arrays(self):
        d, m = self.d, self.m
        p1 = np.empty(m, np.int32); p2 = np.empty(m, np.int32)
        R = np.empty(m * d * d); t = np.empty(m * d); k = np.empty(m); ta = np.empty(m)
        _check(lib().dpgo_graph_copy_out(self.h, p1.ctypes.data_as(_ip), p2.ctypes.data_as(_ip),
                                         R.ctypes.data_as(_dp), t.ctypes.data_as(_dp),
                                         k.ctypes.data_as(_dp), ta.ctypes.data_as(_dp)))
        return dict(p1=p1, p2=p2, R=R.reshape(m, d, d), t=t.reshape(m, d), kappa=k, tau=ta)

    def laplacian_bsr(self):
        """Whole-graph Q: (browptr, bcol, blocks[nnzb, b, b] column-major)."""
        nnz = C.c_longlong()
        _check(lib().dpgo_graph_laplacian_bsr(self.h, C.byref(nnz), None, None, None))
        b = self.d + 1
        rp = np.empty(self.n + 1, np.int32); col = np.empty(nnz.value, np.int32)
        blk = np.empty(nnz.value * b * b)
        _check(lib().dpgo_graph_laplacian_bsr(self.h, C.byref(nnz), rp.ctypes.data_as(_ip),
                                              col.ctypes.data_as(_ip), blk.ctypes.data_as(_dp)))
        return rp, col, blk

    def chain_init(self, r, YLift):
        """YLift (r x d) times the odometry-chain initialisation; returns r x (d+1) n."""
        Y, Yp = _f64(np.asarray(YLift, dtype=np.float64).T.ravel())  # column-major
        out = np.empty(self.n * (self.d + 1) * r)
        _check(lib().dpgo_graph_chain_init(self.h, r, Yp, out.ctypes.data_as(_dp)))
        return from_dev_layout(out, r)

    def chordal_init(self, r, YLift):
        """YLift (r x d) times chordalInitialization (host); returns r x (d+1) n."""
        Y, Yp = _f64(np.asarray(YLift, dtype=np.float64).T.ravel())
        out = np.empty(self.n * (self.d + 1) * r)
        _check(lib().dpgo_graph_chordal_init(self.h, r, Yp, out.ctypes.data_as(_dp)))
        return from_dev_layout(out, r)

    def chordal_init_gpu(self, r, YLift, rtol=1e-12, max_iters=20000, dev_layout=False):
        """chordalInitialization by Jacobi-PCG on the GPU; returns (X, PCG iterations, relative residual)."""
        Y, Yp = _f64(np.asarray(YLift, dtype=np.float64).T.ravel())
        out = np.empty(self.n * (self.d + 1) * r)
        it, rr = C.c_int(), C.c_double()
        _check(lib().dpgo_graph_chordal_init_gpu(self.h, r, Yp, float(rtol), int(max_iters), out.ctypes.data_as(_dp),
                                                 C.byref(it), C.byref(rr)))
        return (out if dev_layout else from_dev_layout(out, r)), it.value, rr.value

    def distributed_init(self, agent_of_pose, r, YLift, gpu=True, rtol=1e-12, max_iters=20000, dev_layout=False):
        """Per-agent chordal (localInitialization) + breadth-first frame alignment (initializeInGlobalFrame);
        returns (X, PCG iterations, relative residual)."""
        aop, ap = _i32(agent_of_pose)
        Y, Yp = _f64(np.asarray(YLift, dtype=np.float64).T.ravel())
        out = np.empty(self.n * (self.d + 1) * r)
        it, rr = C.c_int(), C.c_double()
        _check(lib().dpgo_graph_distributed_init(self.h, int(aop.max()) + 1, ap, r, Yp, int(bool(gpu)), float(rtol),
                                                 int(max_iters), out.ctypes.data_as(_dp), C.byref(it), C.byref(rr)))
        return (out if dev_layout else from_dev_layout(out, r)), it.value, rr.value

    def distributed_init_ex(self, agent_of_pose, local="chordal", align="l2", max_rotation_error=None,
                            gnc_max_iters=None, gnc_mu_step=None, gpu=False, rtol=1e-12, max_iters=20000,
                            max_translation_error=None, clique_node_budget=None):
        """The multi-robot initialisation as local trajectories plus frames (dpgo_graph_distributed_init_ex):
        local "chordal" | "odometry" (what the reference does under a robust cost), align "l2" | "robust" (GNC-TLS
        rotation averaging against the single breadth-first parent, translation mean over the inliers) | "pcm" (the
        same parent and candidates, inliers = their maximum pairwise consistent set under max_rotation_error and
        max_translation_error, which has no default; gpu then also selects the pair-test kernel).  Returns
        (T_local d x (d+1) n, frames K x d x (d+1), info dict(parent, candidates, inliers [K], edge_inlier [m]: 1 inlier
        candidate / 0 rejected / 255 unused, iters, relres)); Rbcd.set_trajectory and frame_lift take them as they
        are."""
        aop, ap = _i32(agent_of_pose)
        K, d = int(aop.max()) + 1, self.d
        P = InitParams()
        lib().dpgo_default_init_params(C.byref(P))
        P.local_init, P.align = LOCAL_INIT[local], ALIGN[align]
        if max_rotation_error is not None:
            P.max_rotation_error = float(max_rotation_error)
        if gnc_max_iters is not None:
            P.gnc_max_iters = int(gnc_max_iters)
        if gnc_mu_step is not None:
            P.gnc_mu_step = float(gnc_mu_step)
        P.use_gpu, P.rtol, P.max_iters = int(bool(gpu)), float(rtol), int(max_iters)
        if max_translation_error is not None:
            P.max_translation_error = float(max_translation_error)
        if clique_node_budget is not None:
            P.clique_node_budget = int(clique_node_budget)
        T = np.empty(self.n * d * (d + 1))
        F = np.empty(K * d * (d + 1))
        par = np.empty(K, np.int32); cand = np.empty(K, np.int32); inl = np.empty(K, np.int32)
        ei = np.empty(max(self.m, 1), np.uint8)
        it, rr = C.c_int(), C.c_double()
        _check(lib().dpgo_graph_distributed_init_ex(self.h, K, ap, C.byref(P), T.ctypes.data_as(_dp),
                                                    F.ctypes.data_as(_dp), par.ctypes.data_as(_ip),
                                                    cand.ctypes.data_as(_ip), inl.ctypes.data_as(_ip),
                                                    ei.ctypes.data_as(_ubp), C.byref(it), C.byref(rr)))
        frames = np.ascontiguousarray(F.reshape(K, d + 1, d).transpose(0, 2, 1))
        return from_dev_layout(T, d), frames, dict(parent=par, candidates=cand, inliers=inl,
                                                   edge_inlier=ei[:self.m], iters=it.value, relres=rr.value)

    def pcm(self, agent_of_pose, T_local, max_translation_error=None, max_rotation_error=None,
            clique_node_budget=None, gpu=False):
        """Pairwise consistent set of the inter-agent loop closures (dpgo_graph_pcm): every agent pair's shared
        closures are one group of pair_consistency (candidate = the pair's relative frame each closure implies under
        T_local, d x (d+1) n as distributed_init_ex returns it), the group's maximum clique its inliers.  Returns
        (edge_inlier [m] uint8: 1 inlier / 0 rejected / 255 an edge inside one agent, info dict(groups, candidates,
        pair_tests, inliers, min_clique_ratio, unproven)).  max_translation_error has no default."""
        aop, ap = _i32(agent_of_pose)
        P = InitParams()
        lib().dpgo_default_init_params(C.byref(P))
        if max_rotation_error is not None:
            P.max_rotation_error = float(max_rotation_error)
        if max_translation_error is not None:
            P.max_translation_error = float(max_translation_error)
        if clique_node_budget is not None:
            P.clique_node_budget = int(clique_node_budget)
        P.use_gpu = int(bool(gpu))
        T = np.asarray(T_local, dtype=np.float64)
        if T.shape != (self.d, (self.d + 1) * self.n):
            raise DPGOHipError("pcm: T_local must be d x (d+1) n")
        Tf, Tp = _f64(to_dev_layout(T))
        ei = np.empty(max(self.m, 1), np.uint8)
        info = PcmInfo()
        _check(lib().dpgo_graph_pcm(self.h, int(aop.max()) + 1, ap, Tp, C.byref(P), ei.ctypes.data_as(_ubp),
                                    C.byref(info)))
        return ei[:self.m], {k: getattr(info, k) for k, _ in PcmInfo._fields_}

    def chain_init_dev_layout(self, r, YLift):
        Y, Yp = _f64(np.asarray(YLift, dtype=np.float64).T.ravel())
        out = np.empty(self.n * (self.d + 1) * r)
        _check(lib().dpgo_graph_chain_init(self.h, r, Yp, out.ctypes.data_as(_dp)))
        return out

    def certify(self, X, r, max_iters=300, tol=1e-8, want_rounded=False, want_vector=False, basis=0, seed_x=False):
        """Certified optimality gap of X (flat r x (d+1) n column-major buffer, or the r x (d+1) n
        matrix) for the whole graph: dict(lambda_min, residual, iters, f_relax, f_rounded, gap, rel_gap
        [, T_rounded d x (d+1) n])."""
        X = np.asarray(X, dtype=np.float64)
        flat = np.ascontiguousarray(X.T).ravel() if X.ndim == 2 else np.ascontiguousarray(X).ravel()
        if flat.size != r * (self.d + 1) * self.n:
            raise DPGOHipError("X has the wrong size")
        lam, fx, fr, info = C.c_double(), C.c_double(), C.c_double(), CertInfo()
        T = np.empty(self.d * (self.d + 1) * self.n) if want_rounded else None
        V = np.empty(flat.size) if want_vector else None
        _check(lib().dpgo_graph_certify_ex(self.h, int(r), flat.ctypes.data_as(_dp), int(max_iters), int(basis),
                                           1 if seed_x else 0, float(tol), C.byref(lam), C.byref(fx), C.byref(fr),
                                           T.ctypes.data_as(_dp) if T is not None else None,
                                           V.ctypes.data_as(_dp) if V is not None else None, C.byref(info)))
        out = dict(lambda_min=lam.value, f_relax=fx.value, f_rounded=fr.value, gap=fr.value - fx.value,
                   rel_gap=(fr.value - fx.value) / fx.value if fx.value else float("nan"))
        out.update(info.as_dict())
        if T is not None:
            out["T_rounded"] = from_dev_layout(T, self.d)
        if V is not None:
            out["eigvec"] = V.reshape(-1, r).T if V.ndim == 1 else V  # r x (d+1) n
        return out

    def certify_chol(self, X, r, eta, w=None, want_vector=True, **params):
        """The certificate by factorisation for the whole graph (dpgo_graph_certify_chol): X as certify() takes it, w
        per-edge weights in the graph's order (None: ones; Rbcd.get_weights() certifies the problem a robust run
        solved).  dict(lambda_min, f_relax, pd, certified, factorisations, sigma_lo, sigma_hi, invit_iters, residual,
        factor_ms, panel_doubles[, eigvec r x (d+1) n]).  Certified (S(X) + eta I positive definite): lambda_min =
        -eta and no eigvec.  params: the fields of dpgo_chol_cert_params."""
        X = np.asarray(X, dtype=np.float64)
        flat = np.ascontiguousarray(X.T).ravel() if X.ndim == 2 else np.ascontiguousarray(X).ravel()
        if flat.size != r * (self.d + 1) * self.n:
            raise DPGOHipError("X has the wrong size")
        wp = None
        if w is not None:
            w, wp = _f64(w)
            if w.size != self.m:
                raise DPGOHipError("w must have one weight per edge")
        lam, fx, info = C.c_double(), C.c_double(), CholCertInfo()
        V = np.empty(flat.size) if want_vector else None
        _check(lib().dpgo_graph_certify_chol(self.h, int(r), flat.ctypes.data_as(_dp), wp, float(eta),
                                             C.byref(chol_cert_params(**params)), C.byref(lam),
                                             V.ctypes.data_as(_dp) if V is not None else None, C.byref(fx),
                                             C.byref(info)))
        out = dict(lambda_min=lam.value, f_relax=fx.value, pd=bool(info.certified), **info.as_dict())
        if V is not None and not info.certified:
            out["eigvec"] = V.reshape(-1, r).T  # r x (d+1) n
        return out

    def certify_block(self, X, r, w=None, want_vector=True, **params):
        """The block certificate for the whole graph (dpgo_graph_certify_block): X as certify() takes it, w per-edge
        weights in the graph's order (None: ones; Rbcd.get_weights() certifies the problem a robust run solved), any
        graph size.  dict(lambda_min, lower_bound, f_relax and the other dpgo_cert_info fields[, eigvec r x (d+1) n]).
        params: the fields of dpgo_block_cert_params."""
        X = np.asarray(X, dtype=np.float64)
        flat = np.ascontiguousarray(X.T).ravel() if X.ndim == 2 else np.ascontiguousarray(X).ravel()
        if flat.size != r * (self.d + 1) * self.n:
            raise DPGOHipError("X has the wrong size")
        wp = None
        if w is not None:
            w, wp = _f64(w)
            if w.size != self.m:
                raise DPGOHipError("w must have one weight per edge")
        lam, fx, info = C.c_double(), C.c_double(), CertInfo()
        V = np.empty(flat.size) if want_vector else None
        _check(lib().dpgo_graph_certify_block(self.h, int(r), flat.ctypes.data_as(_dp), wp,
                                              C.byref(block_cert_params(**params)), C.byref(lam),
                                              V.ctypes.data_as(_dp) if V is not None else None, C.byref(fx),
                                              C.byref(info)))
        out = dict(lambda_min=lam.value, f_relax=fx.value, **info.as_dict())
        if V is not None:
            out["eigvec"] = V.reshape(-1, r).T  # r x (d+1) n
        return out

    def escape(self, X, r, vec, lambda_min, params: "EscapeParams | None" = None):
        """The rank staircase's step after certify() returned lambda_min < 0 at the critical point X (flat r x (d+1) n
        column-major buffer, or the matrix): vec = certify's "eigvec" (r x (d+1) n) or a plain eigenvector
        ((d+1) n).  Returns (X_out, flat (r+1) x (d+1) n column-major, ready for Rbcd.set_X at rank r + 1; info
        dict(accepted, trials, alpha, f_before, f_after, gradnorm_after))."""
        X = np.asarray(X, dtype=np.float64)
        flat = np.ascontiguousarray(X.T).ravel() if X.ndim == 2 else np.ascontiguousarray(X).ravel()
        bn = (self.d + 1) * self.n
        if flat.size != r * bn:
            raise DPGOHipError("X has the wrong size")
        V = np.asarray(vec, dtype=np.float64)
        V = V.reshape(1, -1) if V.ndim == 1 else V
        if V.shape[1] != bn:
            raise DPGOHipError("the direction must have (d+1) n columns")
        vv, vp = _f64(to_dev_layout(V))
        out = np.empty((r + 1) * bn)
        info = EscapeInfo()
        _check(lib().dpgo_graph_escape(self.h, int(r), flat.ctypes.data_as(_dp), vp, int(V.shape[0]),
                                       float(lambda_min), C.byref(params) if params else None,
                                       out.ctypes.data_as(_dp), C.byref(info)))
        return out, info.as_dict()

    def rank_reduce(self, X, r, tol):
        """The staircase's way down: X (flat r x (d+1) n column-major buffer, or the matrix) truncated to its
        numerical rank k = max(d, #{i : w_i > tol w_1}) of the rotation Gram's spectrum w.  Returns (k, X_out flat
        k x (d+1) n column-major, ready for Rbcd.set_X at rank k; info dict(w [r], dropped, f_before, f_after)).
        k = r: X_out is a copy of X."""
        X = np.asarray(X, dtype=np.float64)
        flat = np.ascontiguousarray(X.T).ravel() if X.ndim == 2 else np.ascontiguousarray(X).ravel()
        bn = (self.d + 1) * self.n
        if flat.size != r * bn:
            raise DPGOHipError("X has the wrong size")
        out = np.empty(r * bn)
        k, info = C.c_int(), RankInfo()
        _check(lib().dpgo_graph_rank_reduce(self.h, int(r), flat.ctypes.data_as(_dp), float(tol), C.byref(k),
                                            out.ctypes.data_as(_dp), C.byref(info)))
        return k.value, out[:k.value * bn].copy(), dict(w=np.array(info.w[:r]), dropped=info.dropped,
                                                        f_before=info.f_before, f_after=info.f_after)

    def edge_errors(self, X, r, w=None, outputs=None):
        """hip.edge_errors over the graph's own measurements: X the flat r x (d+1) n column-major buffer (get_X_into,
        trajectory_into at r = d) or the matrix, w per edge (None = ones; weights_into's array gives the cost a robust
        run minimised).  dict(err [m], rot_sq [m], tra_sq [m], cost)."""
        X = np.asarray(X, dtype=np.float64)
        flat = np.ascontiguousarray(X.T).ravel() if X.ndim == 2 else np.ascontiguousarray(X).ravel()
        if flat.size != r * (self.d + 1) * self.n:
            raise DPGOHipError("X has the wrong size")
        wp = None
        if w is not None:
            ww, wp = _f64(w)
            if ww.size != self.m:
                raise DPGOHipError("w must have one entry per edge")
        out, ptrs = _edge_outputs(self.m, outputs)
        _check(lib().dpgo_graph_edge_errors(self.h, int(r), flat.ctypes.data_as(_dp), wp, *ptrs))
        return _edge_result(out, self.m)

    def evaluate(self, X, r, T_truth, use=None, align="lsq", pose=0, per_item=True):
        """A solution X (flat r x (d+1) n column-major buffer or the matrix) against the truth T_truth (d x (d+1) n),
        on the device: rounded in the frame of its pose `pose` when r > d, aligned ("none", "pose", "lsq"), then
        ATE and RPE over the graph's own edges.  dict(count, Aa [d x (d+1)], sigma, rank, ate_rmse, ate_max, rot_rmse,
        rot_max, rpe_tra_rmse, rpe_rot_rmse, edges_used) and, with per_item, tra_sq [n], rot_sq [n], rpe_rot_sq [m],
        rpe_tra_sq [m] (NaN for an unused pose or edge)."""
        d = self.d
        X = np.asarray(X, dtype=np.float64)
        flat = np.ascontiguousarray(X.T).ravel() if X.ndim == 2 else np.ascontiguousarray(X).ravel()
        if flat.size != r * (d + 1) * self.n:
            raise DPGOHipError("X has the wrong size")
        t, nt = _traj_flat(T_truth, d, "T_truth")
        if nt != self.n:
            raise DPGOHipError("T_truth must have one pose per pose of the graph")
        u = None
        if use is not None:
            u, _ = _i32(use)
            if u.size != self.n:
                raise DPGOHipError("use must have one entry per pose")
        if align not in EVAL_ALIGN:
            raise DPGOHipError(f"evaluate: unknown align {align!r}")
        info = EvalInfo()
        arr = {}
        if per_item:
            arr = dict(tra_sq=np.empty(self.n), rot_sq=np.empty(self.n), rpe_rot_sq=np.empty(max(self.m, 1)),
                       rpe_tra_sq=np.empty(max(self.m, 1)))
        _check(lib().dpgo_graph_evaluate(self.h, int(r), flat.ctypes.data_as(_dp), t.ctypes.data_as(_dp),
                                         _opt_ptr(u, _ip), EVAL_ALIGN[align], int(pose), C.byref(info),
                                         *[_opt_ptr(arr.get(k)) for k in ("tra_sq", "rot_sq", "rpe_rot_sq",
                                                                          "rpe_tra_sq")]))
        out = {k: getattr(info, k) for k, _ in EvalInfo._fields_ if k not in ("Aa", "sigma")}
        out["Aa"] = np.array(info.Aa[:d * (d + 1)]).reshape(d + 1, d).T.copy()
        out["sigma"] = np.array(info.sigma[:d])
        for k, v in arr.items():
            out[k] = v[:self.m] if k.startswith("rpe") else v
        return out

    def grid_partition(self, agents_per_axis):
        out = np.empty(self.n, np.int32)
        _check(lib().dpgo_graph_grid_partition(self.h, int(agents_per_axis), out.ctypes.data_as(_ip)))
        return out


def _pcm_inputs(F, x, d, group_off):
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, d * (d + 1))
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, d)
    if F.shape[0] != x.shape[0]:
        raise DPGOHipError("pair_consistency: F and x must hold the same number of candidates")
    go = np.ascontiguousarray(group_off, dtype=np.int32).reshape(-1)
    if go.size < 1:
        raise DPGOHipError("pair_consistency: group_off needs ngroups + 1 entries")
    return F, x, go


def pair_consistency_words(group_off, capacity=-1):
    """Offsets (int64 [ngroups + 1]) of every group's adjacency rows: m_g rows of ceil(m_g / 64) 64-bit words each."""
    go = np.ascontiguousarray(group_off, dtype=np.int32).reshape(-1)
    wo = np.zeros(go.size, np.int64)
    _check(lib().dpgo_hip_pair_consistency_words(go.size - 1, go.ctypes.data_as(_ip), wo.ctypes.data_as(_lp),
                                                 int(capacity)))
    return wo


def _pair_consistency(fn, F, x, d, group_off, c_R, c_t, dense, capacity):
    F, x, go = _pcm_inputs(F, x, d, group_off)
    m, ng = F.shape[0], go.size - 1
    wo = pair_consistency_words(go)
    cap = int(wo[-1]) if capacity is None else int(capacity)
    adj = np.zeros(max(cap, 1), np.uint64)
    deg = np.zeros(max(m, 1), np.int32)
    nd = int(np.sum(np.diff(go).astype(np.int64) ** 2)) if dense else 0
    er = np.empty(max(nd, 1)) if dense else None
    et = np.empty(max(nd, 1)) if dense else None
    _check(fn(int(d), m, F.ctypes.data_as(_dp), x.ctypes.data_as(_dp), ng, go.ctypes.data_as(_ip), float(c_R),
              float(c_t), adj.ctypes.data_as(_ullp), cap, deg.ctypes.data_as(_ip), _opt_ptr(er), _opt_ptr(et)))
    out = dict(adj=adj[:int(wo[-1])], word_off=wo, degree=deg[:m], group_off=go)
    if dense:
        out["e_rot"], out["e_tra"] = er[:nd], et[:nd]
    return out


def pair_consistency(F, x, d, group_off, c_R, c_t, dense=False, capacity=None):
    """The pair tests of frame candidates on the device (dpgo_hip_pair_consistency): F [m, d (d+1)] column-major
    frames, x [m, d] lever points, group_off [ngroups + 1].  Returns dict(adj uint64 words, word_off, degree [m],
    group_off[, e_rot, e_tra: dense m_g x m_g per group, back to back]); adjacency_matrix unpacks a group."""
    return _pair_consistency(lib().dpgo_hip_pair_consistency, F, x, d, group_off, c_R, c_t, dense, capacity)


def pair_consistency_host(F, x, d, group_off, c_R, c_t, dense=False, capacity=None):
    """pair_consistency by the host twin (dpgo_pair_consistency_host): no device, the same bits."""
    return _pair_consistency(lib().dpgo_pair_consistency_host, F, x, d, group_off, c_R, c_t, dense, capacity)


def pair_consistency_dev(d, m, F_dev: int, x_dev: int, group_off, c_R, c_t, adj_dev: int, adj_capacity, degree_dev: int,
                         e_rot_dev: int | None = None, e_tra_dev: int | None = None, stream_ptr: int | None = None):
    """pair_consistency on device pointers (group_off: host), queued on `stream_ptr`; returns once the stream has run
    it."""
    go = np.ascontiguousarray(group_off, dtype=np.int32).reshape(-1)
    _check(lib().dpgo_hip_pair_consistency_dev(int(d), int(m), C.c_void_p(F_dev), C.c_void_p(x_dev), go.size - 1,
                                               go.ctypes.data_as(_ip), float(c_R), float(c_t), C.c_void_p(adj_dev),
                                               int(adj_capacity), C.c_void_p(degree_dev), C.c_void_p(e_rot_dev or 0),
                                               C.c_void_p(e_tra_dev or 0), C.c_void_p(stream_ptr or 0)))


def pair_consistency_bench(d, m, F_dev: int, x_dev: int, group_off, c_R, c_t, adj_dev: int, adj_capacity,
                           degree_dev: int, warmup=5, reps=20):
    """Milliseconds of `reps` launches of the pair-test kernel (with its degree memset) after `warmup`, each between
    two HIP events, the tile table uploaded once beforehand (dpgo_hip_pair_consistency_bench)."""
    go = np.ascontiguousarray(group_off, dtype=np.int32).reshape(-1)
    ms = np.empty(int(reps))
    _check(lib().dpgo_hip_pair_consistency_bench(int(d), int(m), C.c_void_p(F_dev), C.c_void_p(x_dev), go.size - 1,
                                                 go.ctypes.data_as(_ip), float(c_R), float(c_t), C.c_void_p(adj_dev),
                                                 int(adj_capacity), C.c_void_p(degree_dev), int(warmup), int(reps),
                                                 ms.ctypes.data_as(_dp)))
    return ms


def adjacency_matrix(adj, word_off, group_off, g):
    """Group g of a pair_consistency result as a bool matrix [m_g, m_g] (entry (k, l) = bit l of row k)."""
    mg = int(group_off[g + 1] - group_off[g])
    W = (mg + 63) // 64
    rows = np.asarray(adj[int(word_off[g]):int(word_off[g]) + mg * W], dtype=np.uint64).reshape(mg, W)
    bits = np.unpackbits(rows.view(np.uint8).reshape(mg, W * 8), axis=1, bitorder="little")
    return bits[:, :mg].astype(bool)


def pack_adjacency(A):
    """A bool matrix [m, m] as max_clique's rows: uint64 [m, ceil(m / 64)], bit l of row k = A[k, l]."""
    A = np.asarray(A, dtype=bool)
    m = A.shape[0]
    W = max((m + 63) // 64, 1)
    bits = np.zeros((m, W * 64), np.uint8)
    bits[:, :m] = A
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(m, W)


def max_clique(rows, m=None, node_budget=-1):
    """Maximum clique of the graph whose row k is rows[k] (uint64 words, as pack_adjacency / a group's adj reshaped
    [m_g, words]): (members ascending, proven).  node_budget < 0: no limit; 0: the greedy clique (descending degree,
    ties to the lower index), proven False unless m = 0."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    m = rows.shape[0] if m is None else int(m)
    W = rows.shape[1] if rows.ndim == 2 else (m + 63) // 64
    cl = np.empty(max(m, 1), np.int32)
    size, proven = C.c_int(), C.c_int()
    _check(lib().dpgo_max_clique(m, int(W), rows.ctypes.data_as(_ullp), int(node_budget), cl.ctypes.data_as(_ip),
                                 C.byref(size), C.byref(proven)))
    return cl[:size.value].copy(), bool(proven.value)


def robust_rotation_average(R, kappa=None, threshold=None, max_iters=1000, mu_step=1.4):
    """robustSingleRotationAveraging (src/DPGO_utils.cpp:582-644), host: GNC-TLS over the chordal mean of the
    rotations R (n x d x d); threshold: chordal, default angular2ChordalSO3(0.5).  Returns (R_opt d x d -- the estimate
    before the final reweighting, as in the reference -- weights [n], GNC iterations)."""
    Rs = np.asarray(R, dtype=np.float64)
    n, d = Rs.shape[0], Rs.shape[-1]
    rr, rp = _f64(Rs.reshape(-1))
    kp = None
    if kappa is not None:
        kk, kp = _f64(kappa)
        if kk.size != n:
            raise DPGOHipError("kappa must have one entry per rotation")
    if threshold is None:
        threshold = 2.0 * np.sqrt(2.0) * np.sin(0.25)
    out = np.empty(d * d); w = np.empty(max(n, 1)); it = C.c_int()
    _check(lib().dpgo_robust_rotation_average(d, n, rp, kp, float(threshold), int(max_iters), float(mu_step),
                                              out.ctypes.data_as(_dp), w.ctypes.data_as(_dp), C.byref(it)))
    return out.reshape(d, d), w[:n], it.value


def chordal_initialization(d, n, p1, p2, R, t, kappa, tau):
    """chordalInitialization (src/DPGO_utils.cpp:377-424), host: T (d x (d+1) n)."""
    a1, a1p = _i32(p1)
    a2, a2p = _i32(p2)
    Rr, Rp = _f64(np.asarray(R).reshape(-1))
    tt, tp = _f64(np.asarray(t).reshape(-1))
    kk, kp = _f64(kappa)
    ta, tap = _f64(tau)
    out = np.empty(d * (d + 1) * n)
    _check(lib().dpgo_chordal_initialization(d, int(n), len(a1), a1p, a2p, Rp, tp, kp, tap, out.ctypes.data_as(_dp)))
    return from_dev_layout(out, d)


def chordal_initialization_gpu(d, n, p1, p2, R, t, kappa, tau, rtol=1e-12, max_iters=20000):
    """chordalInitialization with both solves by Jacobi-PCG on the GPU: (T, iterations, rel. residual)."""
    a1, a1p = _i32(p1)
    a2, a2p = _i32(p2)
    Rr, Rp = _f64(np.asarray(R).reshape(-1))
    tt, tp = _f64(np.asarray(t).reshape(-1))
    kk, kp = _f64(kappa)
    ta, tap = _f64(tau)
    out = np.empty(d * (d + 1) * n)
    it, rr = C.c_int(), C.c_double()
    _check(lib().dpgo_chordal_initialization_gpu(d, int(n), len(a1), a1p, a2p, Rp, tp, kp, tap, float(rtol),
                                                 int(max_iters), out.ctypes.data_as(_dp), C.byref(it), C.byref(rr)))
    return from_dev_layout(out, d), it.value, rr.value


def exchange_plan(graph: "Graph", agent_of_pose, agent_rank, rank, world):
    """Host-only exchange plan (no GPU): ([send pose ids per peer], [recv pose ids per peer])."""
    aop, ap = _i32(agent_of_pose)
    ar, arp = _i32(agent_rank)
    sc = np.empty(world, np.int64); rc = np.empty(world, np.int64)
    _check(lib().dpgo_rbcd_plan(graph.h, len(ar), ap, arp, rank, world, sc.ctypes.data_as(_lp),
                                rc.ctypes.data_as(_lp), None, None))
    sp_ = np.empty(max(int(sc.sum()), 1), np.int32); rp_ = np.empty(max(int(rc.sum()), 1), np.int32)
    _check(lib().dpgo_rbcd_plan(graph.h, len(ar), ap, arp, rank, world, None, None,
                                sp_.ctypes.data_as(_ip), rp_.ctypes.data_as(_ip)))
    so = np.concatenate([[0], np.cumsum(sc)]); ro = np.concatenate([[0], np.cumsum(rc)])
    return ([sp_[so[p]:so[p + 1]] for p in range(world)], [rp_[ro[p]:ro[p + 1]] for p in range(world)])


def exchange_plan_color(graph: "Graph", agent_of_pose, agent_rank, color, rank, world):
    """Host-only per-colour halo plan (the poses colour `color`'s agents read): ([send ids per peer],
    [recv ids per peer])."""
    aop, ap = _i32(agent_of_pose)
    ar, arp = _i32(agent_rank)
    sc = np.empty(world, np.int64); rc = np.empty(world, np.int64)
    _check(lib().dpgo_rbcd_plan_color(graph.h, len(ar), ap, arp, int(color), rank, world, sc.ctypes.data_as(_lp),
                                      rc.ctypes.data_as(_lp), None, None))
    sp_ = np.empty(max(int(sc.sum()), 1), np.int32); rp_ = np.empty(max(int(rc.sum()), 1), np.int32)
    _check(lib().dpgo_rbcd_plan_color(graph.h, len(ar), ap, arp, int(color), rank, world, None, None,
                                      sp_.ctypes.data_as(_ip), rp_.ctypes.data_as(_ip)))
    so = np.concatenate([[0], np.cumsum(sc)]); ro = np.concatenate([[0], np.cumsum(rc)])
    return ([sp_[so[p]:so[p + 1]] for p in range(world)], [rp_[ro[p]:ro[p + 1]] for p in range(world)])


def weight_owner(graph: "Graph", agent_of_pose, num_agents):
    """Host-only: per edge the agent whose weight Rbcd.weights_into reports (-1 = odometry, weight 1; a shared loop
    closure: the lower-ID agent)."""
    aop, ap = _i32(agent_of_pose)
    if len(aop) != graph.n:
        raise ValueError(f"agent_of_pose has {len(aop)} entries, the graph has {graph.n} poses")
    out = np.empty(graph.m, np.int32)
    _check(lib().dpgo_rbcd_weight_owner(graph.h, int(num_agents), ap, out.ctypes.data_as(_ip)))
    return out


def pcm_weights(edge_inlier):
    """Graph.pcm's edge_inlier as Rbcd.set_weights' (w, fixed): a rejected closure (0) is held at weight 0, an accepted
    one (1) and an edge PCM does not judge (255: odometry, private closures) start at 1 and stay free."""
    rejected = np.asarray(edge_inlier) == 0
    return np.where(rejected, 0.0, 1.0), rejected.astype(np.uint8)


def lifting_matrix(d, r, seed=2):
    """Repo-defined lifting matrix YLift in St(d, r) (replaces ROPTLIB's RNG)."""
    M = np.random.default_rng(seed).standard_normal((r, d))
    Qm, Rm = np.linalg.qr(M)
    s = np.sign(np.diag(Rm))
    s[s == 0] = 1
    return Qm * s


def rbcd_params(**kw) -> RbcdParams:
    p = RbcdParams()
    lib().dpgo_rbcd_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Rbcd:
    """Colour-class RBCD over N agents; this process owns the agents with agent_rank == rank."""

    def __init__(self, graph: Graph, agent_of_pose, agent_rank, rank=0, world=1, params=None):
        self.graph = graph
        aop, ap = _i32(agent_of_pose)
        ar, arp = _i32(agent_rank)
        self.num_agents = len(ar)
        self.params = params or rbcd_params()
        h = C.c_void_p()
        _check(lib().dpgo_rbcd_create(graph.h, self.num_agents, ap, arp, rank, world,
                                      C.byref(self.params), C.byref(h)))
        self.h = h
        self.rank, self.world = rank, world
        nc, na, npz = C.c_int(), C.c_int(), C.c_int()
        _check(lib().dpgo_rbcd_info(self.h, C.byref(nc), C.byref(na), C.byref(npz), None))
        self.num_colors, self.owned_agents, self.owned_poses = nc.value, na.value, npz.value
        per = np.empty(self.num_colors, np.int32)
        _check(lib().dpgo_rbcd_info(self.h, None, None, None, per.ctypes.data_as(_ip)))
        self.agents_per_color = per
        col = np.empty(self.num_agents, np.int32)
        _check(lib().dpgo_rbcd_color_of_agent(self.h, col.ctypes.data_as(_ip)))
        self.color_of_agent = col
        sc = np.empty(world, np.int64); rc = np.empty(world, np.int64)
        _check(lib().dpgo_rbcd_exchange_counts(self.h, sc.ctypes.data_as(_lp), rc.ctypes.data_as(_lp)))
        self.send_counts, self.recv_counts = sc, rc
        # per-colour halos (doubles per peer)
        self.send_counts_color, self.recv_counts_color = [], []
        for c in range(self.num_colors):
            sc = np.empty(world, np.int64); rc = np.empty(world, np.int64)
            _check(lib().dpgo_rbcd_exchange_counts_color(self.h, c, sc.ctypes.data_as(_lp), rc.ctypes.data_as(_lp)))
            self.send_counts_color.append(sc)
            self.recv_counts_color.append(rc)

    def close(self):
        if getattr(self, "h", None):
            lib().dpgo_rbcd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _check(lib().dpgo_rbcd_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_X(self, X):
        x, xp = _f64(to_dev_layout(X) if X.ndim == 2 else X)
        _check(lib().dpgo_rbcd_set_X(self.h, xp))

    def set_trajectory(self, T, YLift, frames=None):
        """Start from an SE(d) trajectory (dpgo_rbcd_set_trajectory): T d x (d+1) n (or its flat column-major
        buffer), every pose in the frame of its agent's entry of `frames` (K x d x (d+1); Graph.distributed_init_ex's
        outputs) or, with frames None, already in one frame (a warm start from trajectory_into).  Lifted on the
        device; the Nesterov state is (re)initialised as by set_X."""
        d, r = self.graph.d, self.params.r
        T = np.asarray(T, dtype=np.float64)
        t, tp = _f64(to_dev_layout(T) if T.ndim == 2 else T)
        if t.size != self.graph.n * d * (d + 1):
            raise ValueError("T must be d x (d+1) n")
        Y, Yp = _ylift_colmajor(YLift, r, d)
        fp = None
        if frames is not None:
            F = np.asarray(frames, dtype=np.float64)
            if F.shape != (self.num_agents, d, d + 1):
                raise ValueError("frames must be num_agents x d x (d+1)")
            f, fp = _f64(np.ascontiguousarray(F.transpose(0, 2, 1)).ravel())
        _check(lib().dpgo_rbcd_set_trajectory(self.h, tp, Yp, fp))

    def get_X_into(self, Xflat):
        """Write owned poses into a global flat (device-layout) host array."""
        assert Xflat.dtype == np.float64 and Xflat.flags.c_contiguous
        need = self.graph.n * (self.graph.d + 1) * self.params.r
        if Xflat.size < need:
            raise ValueError(f"X buffer holds {Xflat.size} doubles, the graph needs {need}")
        _check(lib().dpgo_rbcd_get_X(self.h, Xflat.ctypes.data_as(_dp)))

    def anchor(self, pose=0):
        """The lifted pose of global pose `pose` (r x (d+1)) if this rank owns it, else None."""
        r, b = self.params.r, self.graph.d + 1
        a = np.empty(r * b)
        owned = C.c_int()
        _check(lib().dpgo_rbcd_get_anchor(self.h, int(pose), a.ctypes.data_as(_dp), C.byref(owned)))
        return from_dev_layout(a, r) if owned.value else None

    def trajectory_into(self, T_flat, anchor=None):
        """getTrajectoryInGlobalFrame of every owned agent in the frame of `anchor` (r x (d+1); None = global pose 0,
        which this rank must own), rounded on the device: written at the owned poses of a global flat d x (d+1) n
        column-major host array (from_dev_layout(T_flat, d) is the d x (d+1) n matrix)."""
        assert T_flat.dtype == np.float64 and T_flat.flags.c_contiguous
        need = self.graph.n * (self.graph.d + 1) * self.graph.d
        if T_flat.size < need:
            raise ValueError(f"T buffer holds {T_flat.size} doubles, the graph needs {need}")
        ap = None
        if anchor is not None:
            a, ap = _f64(to_dev_layout(anchor))
            if a.size != self.params.r * (self.graph.d + 1):
                raise ValueError("anchor must be r x (d+1)")
        _check(lib().dpgo_rbcd_get_trajectory(self.h, ap, T_flat.ctypes.data_as(_dp)))

    def _anchor_ptr(self, anchor):
        if anchor is None:
            return None, None
        a, ap = _f64(to_dev_layout(anchor))
        if a.size != self.params.r * (self.graph.d + 1):
            raise ValueError("anchor must be r x (d+1)")
        return a, ap

    def set_truth(self, T_truth, use=None):
        """The ground truth (d x (d+1) n matrix or flat buffer, global pose order) and mask (one int per global pose,
        None = every pose) the truth_* calls compare against: the owned poses' part goes to the device once.
        T_truth None clears it."""
        if T_truth is None:
            _check(lib().dpgo_rbcd_set_truth(self.h, None, None))
            return
        d = self.graph.d
        t, n = _traj_flat(T_truth, d, "T_truth")
        if n != self.graph.n:
            raise ValueError("T_truth must have one pose per pose of the graph")
        u = None
        if use is not None:
            u, _ = _i32(use)
            if u.size != n:
                raise ValueError("use must have one entry per pose")
        _check(lib().dpgo_rbcd_set_truth(self.h, t.ctypes.data_as(_dp), _opt_ptr(u, _ip)))

    def truth_moments(self, anchor=None, shift=None):
        """This rank's traj_moments vector of its owned poses (rounded on the device in the frame of `anchor`, as
        trajectory_into) against their truth, about shift (2 d, None = zeros); with several ranks the caller sums."""
        d = self.graph.d
        a, ap = self._anchor_ptr(anchor)
        s = _opt_vec(shift, 2 * d, "shift")
        mom = np.empty(traj_moments_len(d))
        _check(lib().dpgo_rbcd_truth_moments(self.h, ap, _opt_ptr(s), mom.ctypes.data_as(_dp)))
        return mom

    def truth_errors(self, anchor=None, Aa=None, tra_sq=None, rot_sq=None, sums=True):
        """traj_errors of the owned poses under Aa (d x (d+1), None = identity): tra_sq / rot_sq (global arrays of n
        doubles, each optional) are written at the owned poses, other entries untouched; returns this rank's partial
        sums (merge_traj_sums joins the ranks') or None."""
        a, ap = self._anchor_ptr(anchor)
        A = _aa_colmajor(Aa, self.graph.d)
        for x in (tra_sq, rot_sq):
            if x is not None:
                assert x.dtype == np.float64 and x.flags.c_contiguous
                if x.size < self.graph.n:
                    raise ValueError(f"the array holds {x.size} doubles, the graph has {self.graph.n} poses")
        s = np.empty(TRAJ_SUMS) if sums else None
        _check(lib().dpgo_rbcd_truth_errors(self.h, ap, _opt_ptr(A), _opt_ptr(tra_sq), _opt_ptr(rot_sq), _opt_ptr(s)))
        return s

    def evaluate(self, anchor=None):
        """ATE of the engine's solution against set_truth's trajectory for world = 1: two truth_moments calls (the
        means, then about them), align_moments, truth_errors.  dict(count, Aa, sigma, rank, ate_rmse, ate_max,
        rot_rmse, rot_max, tra_sq [n], rot_sq [n]).  (The RPE is Graph.evaluate's, of trajectory_into's T.)"""
        d, n = self.graph.d, self.graph.n
        m0 = self.truth_moments(anchor)
        if not m0[0] >= 1:
            raise DPGOHipError("evaluate: no pose counted")
        shift = m0[3:3 + 2 * d] / m0[0]
        Aa, info = align_moments(d, self.truth_moments(anchor, shift), shift)
        tra, rot = np.full(n, np.nan), np.full(n, np.nan)
        s = self.truth_errors(anchor, Aa, tra, rot)
        return dict(count=s[0], Aa=Aa, sigma=info["sigma"], rank=info["rank"], ate_rmse=float(np.sqrt(s[1] / s[0])),
                    ate_max=float(np.sqrt(s[3])), rot_rmse=float(np.sqrt(s[2] / s[0])), rot_max=float(np.sqrt(s[4])),
                    tra_sq=tra, rot_sq=rot)

    def gram(self):
        """This rank's partial Gram sum_j Y_j Y_j^T (r x r) over its owned poses, from the engine's X on the device;
        with several ranks the caller sums the partials."""
        r = self.params.r
        o = np.empty(r * r)
        _check(lib().dpgo_rbcd_gram(self.h, o.ctypes.data_as(_dp)))
        return o.reshape(r, r).T.copy()

    def get_X_reduced_into(self, W, Xk_flat):
        """The engine's X truncated to rank k along W (r x k; hip.rank_reduce's pass on the device), written at the
        owned poses of a global flat k x (d+1) n column-major host array (from_dev_layout(Xk_flat, k) is the
        matrix; Rbcd.set_X of a rank-k engine takes it)."""
        assert Xk_flat.dtype == np.float64 and Xk_flat.flags.c_contiguous
        k, (w, wp) = _w_colmajor(W, self.params.r)
        need = self.graph.n * (self.graph.d + 1) * k
        if Xk_flat.size < need:
            raise ValueError(f"X buffer holds {Xk_flat.size} doubles, rank {k} needs {need}")
        _check(lib().dpgo_rbcd_get_X_reduced(self.h, k, wp, Xk_flat.ctypes.data_as(_dp)))

    def weights_into(self, w):
        """Current weight of every measurement this rank is responsible for (weight_owner's agent lives here), at
        its index in the graph's edge order; other entries untouched."""
        assert w.dtype == np.float64 and w.flags.c_contiguous
        if w.size < self.graph.m:
            raise ValueError(f"w holds {w.size} doubles, the graph has {self.graph.m} edges")
        _check(lib().dpgo_rbcd_get_weights(self.h, w.ctypes.data_as(_dp)))

    def errors_into(self, err, recv_ptr=None, rounded=False, anchor=None, rot_sq=None, tra_sq=None):
        """The residual err = kappa rot_sq + tau tra_sq of every measurement weights_into reports for this rank, at the
        engine's current X, at its index in the graph's edge order (other entries untouched); rot_sq / tra_sq
        likewise when given (err may be None then).  recv_ptr: the received public poses of a pack and exchange done
        after the last update (required when this rank receives poses).  rounded: the errors of the rounded
        trajectory in the frame of `anchor` (r x (d+1); None = global pose 0, which this rank must own), bitwise
        Graph.edge_errors(T, d) of trajectory_into's T."""
        ptrs = []
        for a in (err, rot_sq, tra_sq):
            if a is None:
                ptrs.append(None)
                continue
            assert a.dtype == np.float64 and a.flags.c_contiguous
            if a.size < self.graph.m:
                raise ValueError(f"the array holds {a.size} doubles, the graph has {self.graph.m} edges")
            ptrs.append(a.ctypes.data_as(_dp))
        ap = None
        if anchor is not None:
            a, ap = _f64(to_dev_layout(anchor))
            if a.size != self.params.r * (self.graph.d + 1):
                raise ValueError("anchor must be r x (d+1)")
        _check(lib().dpgo_rbcd_get_errors(self.h, C.c_void_p(recv_ptr or 0), 1 if rounded else 0, ap, *ptrs))

    def reset_stream(self):
        _check(lib().dpgo_rbcd_reset_stream(self.h))

    def central_eval(self, recv_ptr=None, weighted=False):
        """(this rank's central cost share, |RieGrad|^2 per agent [num_agents]) at the current X: at unit weights, or
        with weighted=True of the problem the engine is solving (the weights last set or left by the reweighting)."""
        f = C.c_double()
        g = np.zeros(self.num_agents)
        _check(lib().dpgo_rbcd_central_eval_ex(self.h, C.c_void_p(recv_ptr or 0), 1 if weighted else 0, C.byref(f),
                                               g.ctypes.data_as(_dp)))
        return f.value, g

    def set_weights(self, w, fixed=None):
        """Measurement weights from outside (dpgo_rbcd_set_weights): w one weight per edge in the graph's order,
        finite and >= 0; fixed (optional, one flag per edge) marks known inliers that GNC never rewrites and the
        converged ratio leaves out.  Replaces earlier weights and flags; an invalid weight or a BSR-format engine
        raises and changes nothing."""
        wv, wp = _f64(w)
        if wv.size != self.graph.m:
            raise ValueError(f"w has {wv.size} entries, the graph has {self.graph.m} edges")
        fv = None
        if fixed is not None:
            fv = np.ascontiguousarray(np.asarray(fixed) != 0, dtype=np.uint8)
            if fv.size != self.graph.m:
                raise ValueError(f"fixed has {fv.size} entries, the graph has {self.graph.m} edges")
        _check(lib().dpgo_rbcd_set_weights(self.h, wp, C.c_void_p(fv.ctypes.data if fv is not None else 0)))

    def set_weights_dev(self, w_ptr, fixed_ptr=0):
        """The same from device pointers (m doubles, m bytes or 0) valid until the engine's stream has passed the
        call; the caller guarantees finite weights >= 0."""
        _check(lib().dpgo_rbcd_set_weights_dev(self.h, C.c_void_p(w_ptr), C.c_void_p(fixed_ptr or 0)))

    def bench_set_weights(self, color, reps=1):
        """ms per k_set_weights launch of one colour, repeating the host-form set_weights call just made."""
        ms = C.c_double()
        _check(lib().dpgo_rbcd_bench_set_weights(self.h, int(color), int(reps), C.byref(ms)))
        return ms.value

    def status(self):
        """(relativeChange[num_agents], readyToTerminate[num_agents]); NaN / -1 for other ranks' agents."""
        rc = np.full(self.num_agents, np.nan)
        rd = np.full(self.num_agents, -1, np.int32)
        _check(lib().dpgo_rbcd_status(self.h, rc.ctypes.data_as(_dp), rd.ctypes.data_as(_ip)))
        return rc, rd

    def ready_votes(self):
        """This rank's share of PGOAgent::shouldTerminate (src/PGOAgent.cpp:1007-1031): (owned agents
        ready to terminate, owned agents).  Every agent of the team is ready iff the sums over ranks are
        equal (the caller all-reduces them); the maxNumIters cap is the caller's loop bound."""
        _, rd = self.status()
        mine = rd >= 0
        return int(np.sum(rd[mine] == 1)), int(np.sum(mine))

    def stats(self):
        """Cumulative solver counters per agent: int array [num_agents, STATS_INTS] (zeros elsewhere)."""
        out = np.zeros(self.num_agents * STATS_INTS, np.int32)
        _check(lib().dpgo_rbcd_stats(self.h, out.ctypes.data_as(_ip)))
        return out.reshape(self.num_agents, STATS_INTS)

    def bytes(self):
        """(cumulative algorithmic bytes of all launches, EVAL_TCG bytes per colour pass [num_colors])."""
        b = C.c_double()
        per = np.zeros(self.num_colors)
        _check(lib().dpgo_rbcd_bytes(self.h, C.byref(b), per.ctypes.data_as(_dp)))
        return b.value, per

    def comm_init(self, uid: bytes):
        """Create the engine's RCCL communicator (collective over the engine's ranks); uid from
        rccl_unique_id() on one rank, shared by the caller."""
        buf = C.create_string_buffer(bytes(uid), 128)
        _check(lib().dpgo_rbcd_comm_init(self.h, buf))

    def exact_factor_info(self, color):
        """Problem.exact_factor_info of the colour's batched problem."""
        n, lv, mt, pd, ms, cnt = C.c_longlong(), C.c_int(), C.c_int(), C.c_longlong(), C.c_double(), C.c_int()
        _check(lib().dpgo_rbcd_exact_factor_info(self.h, int(color), C.byref(n), C.byref(lv), C.byref(mt), C.byref(pd),
                                                 C.byref(ms), C.byref(cnt)))
        fl, ifl = C.c_double(), C.c_double()
        _check(lib().dpgo_rbcd_exact_factor_flops(self.h, int(color), C.byref(fl), C.byref(ifl)))
        out = {"nodes": n.value, "levels": lv.value, "max_s_tiles": mt.value, "panel_doubles": pd.value,
               "factor_ms": ms.value, "factor_count": cnt.value, "cholesky_flops": fl.value, "inverse_flops": ifl.value}
        if ms.value > 0:
            out["factor_tflops"] = fl.value / (ms.value * 1e-3) / 1e12
            out["factor_tflops_with_inverse"] = (fl.value + ifl.value) / (ms.value * 1e-3) / 1e12
        return out

    def bench_precond(self, color, reps):
        """The exact preconditioner's forward / backward sweeps over colour class c: (ms_fwd, ms_bwd, stored panel
        bytes)."""
        f, b, p = C.c_double(), C.c_double(), C.c_double()
        _check(lib().dpgo_rbcd_bench_precond(self.h, int(color), int(reps), C.byref(f), C.byref(b), C.byref(p)))
        return f.value, b.value, p.value

    def exact_sweep_bytes(self, color):
        """(forward, backward) panel bytes one application over colour class c reads (wide nodes' tiles, narrow nodes'
        compact copies)."""
        f, b = C.c_double(), C.c_double()
        _check(lib().dpgo_rbcd_exact_sweep_bytes(self.h, int(color), C.byref(f), C.byref(b)))
        return f.value, b.value

    def comm_info(self):
        """(ncclCommCount, ncclCommUserRank) of the engine's own RCCL communicator, (-1, -1) without one."""
        n, r = C.c_int(), C.c_int()
        _check(lib().dpgo_rbcd_comm_info(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def exchange_color(self, color):
        """Per-colour halo by the engine's RCCL group (after pre_exchange(color)); pass the result to
        update_color()."""
        p = C.c_void_p()
        _check(lib().dpgo_rbcd_exchange_color(self.h, int(color), C.byref(p)))
        return p.value

    def pack_color(self, color, send_ptr):
        _check(lib().dpgo_rbcd_pack_color(self.h, int(color), C.c_void_p(send_ptr or 0)))

    def update_color(self, color, recv_ptr, want_results=False):
        if want_results:
            n = int(self.agents_per_color[color])
            res = (OptResult * max(n, 1))()
            _check(lib().dpgo_rbcd_update_color(self.h, int(color), C.c_void_p(recv_ptr or 0), res))
            return [res[i].as_dict() for i in range(n)]
        _check(lib().dpgo_rbcd_update_color(self.h, int(color), C.c_void_p(recv_ptr or 0), None))
        return None

    def exchange(self):
        """Pack + RCCL send/recv of the public poses (after pre_exchange); returns the device pointer of
        the engine-owned receive buffer for update()."""
        p = C.c_void_p()
        _check(lib().dpgo_rbcd_exchange(self.h, C.byref(p)))
        return p.value

    def mode_bytes(self, color):
        """{SpMM mode: algorithmic bytes of one launch over every agent of the colour}."""
        out = np.zeros(len(SPMM_MODES))
        _check(lib().dpgo_rbcd_mode_bytes(self.h, int(color), out.ctypes.data_as(_dp)))
        return {SPMM_MODES[m]: float(out[m]) for m in range(len(SPMM_MODES)) if out[m] > 0}

    def set_trace(self, capacity):
        _check(lib().dpgo_rbcd_set_trace(self.h, int(capacity)))
        self._trace_cap = int(capacity)

    def get_trace(self, agent):
        """Per-iteration records of one owned agent's updates: list of dicts (TRACE_FIELDS)."""
        cap = getattr(self, "_trace_cap", 0)
        buf = np.zeros(max(cap, 1) * TRACE_WIDTH)
        n = C.c_int()
        _check(lib().dpgo_rbcd_get_trace(self.h, int(agent), buf.ctypes.data_as(_dp), cap, C.byref(n)))
        return [dict(zip(TRACE_FIELDS, buf[i * TRACE_WIDTH:(i + 1) * TRACE_WIDTH].tolist()))
                for i in range(min(n.value, cap))]

    def set_kernel_timing(self, on):
        _check(lib().dpgo_rbcd_set_kernel_timing(self.h, int(on)))  # 0 off, k: every k-th launch per mode

    def set_tuning(self, key, value):
        """A tuning key on this engine's colour problems (A/B timing without rebuilding the engine)."""
        _check(lib().dpgo_rbcd_set_tuning(self.h, int(key), int(value)))

    def kernel_times(self, batch_equiv=False):
        """{mode: (ms summed, launches)} of the timed in-step X.Q launches since the last call; with batch_equiv,
        (ms, launches, full-batch launch equivalents) -- the divisor of mode_bytes for a per-launch rate."""
        ms = np.zeros(len(SPMM_MODES))
        n = np.zeros(len(SPMM_MODES), np.int64)
        fr = np.zeros(len(SPMM_MODES))
        _check(lib().dpgo_rbcd_kernel_times_ex(self.h, ms.ctypes.data_as(_dp), n.ctypes.data_as(_lp),
                                               fr.ctypes.data_as(_dp)))
        if batch_equiv:
            return {SPMM_MODES[m]: (float(ms[m]), int(n[m]), float(fr[m])) for m in range(len(SPMM_MODES)) if n[m] > 0}
        return {SPMM_MODES[m]: (float(ms[m]), int(n[m])) for m in range(len(SPMM_MODES)) if n[m] > 0}

    def pre_exchange(self, color):
        _check(lib().dpgo_rbcd_pre_exchange(self.h, int(color)))

    def pack(self, send_ptr):
        _check(lib().dpgo_rbcd_pack(self.h, C.c_void_p(send_ptr or 0)))

    def set_selected(self, agent_mask=None):
        """Optimise only these agents of the updated colour (None: all; the greedy schedule selects one)."""
        if agent_mask is None:
            _check(lib().dpgo_rbcd_set_selected(self.h, None))
            return
        m, mp = _i32(np.asarray(agent_mask) != 0)
        if m.size != self.num_agents:
            raise ValueError("agent_mask needs one entry per agent")
        _check(lib().dpgo_rbcd_set_selected(self.h, mp))

    def update(self, color, recv_ptr, want_results=False):
        if want_results:
            n = int(self.agents_per_color[color])
            res = (OptResult * max(n, 1))()
            _check(lib().dpgo_rbcd_update(self.h, int(color), C.c_void_p(recv_ptr or 0), res))
            return [res[i].as_dict() for i in range(n)]
        _check(lib().dpgo_rbcd_update(self.h, int(color), C.c_void_p(recv_ptr or 0), None))
        return None

    def bench_spmm(self, color, reps):
        b, ms = C.c_double(), C.c_double()
        _check(lib().dpgo_rbcd_bench_spmm(self.h, int(color), int(reps), C.byref(b), C.byref(ms)))
        return b.value, ms.value

    def spmm_bytes(self, color):
        """(SURVEY 8d B_spmm for explicit blocks, bytes of the stored form) of one X.Q SpMM."""
        bb, fb = C.c_double(), C.c_double()
        _check(lib().dpgo_rbcd_spmm_bytes(self.h, int(color), C.byref(bb), C.byref(fb)))
        return bb.value, fb.value

    def bench_hvp(self, color, reps):
        ms = C.c_double()
        _check(lib().dpgo_rbcd_bench_hvp(self.h, int(color), int(reps), C.byref(ms)))
        return ms.value

    def counters(self):
        a, i = C.c_longlong(), C.c_longlong()
        _check(lib().dpgo_rbcd_counters(self.h, C.byref(a), C.byref(i)))
        return a.value, i.value

    def next_y_counters(self):
        """(skipped, mispredicted): selected-colour combination passes skipped because the previous iteration's
        non-selected pass wrote their outputs ahead (tuning key 15), and write-ahead records that were dropped."""
        s, m = C.c_longlong(), C.c_longlong()
        _check(lib().dpgo_rbcd_next_y_counters(self.h, C.byref(s), C.byref(m)))
        return s.value, m.value

    def tcg_blocks(self, color):
        """(blocks, agent_tiles): the agent blocks the colour's last update queued its merged tCG loop in (tuning key
        16; 0: the unblocked queueing ran) and the tile count of each of the colour's agents, in batch order."""
        n = C.c_int()
        tiles = np.zeros(max(int(self.agents_per_color[color]), 1), np.int32)
        _check(lib().dpgo_rbcd_tcg_blocks(self.h, int(color), C.byref(n), tiles.ctypes.data_as(_ip)))
        return n.value, tiles[:int(self.agents_per_color[color])]
