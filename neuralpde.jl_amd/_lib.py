"""ctypes binding of the C ABI in include/pinn_hip.h (libpinn_hip.so).

This is the Python mirror of the `ccall` layer the Julia glue uses.  There is no
CPU fallback: if the HIP library is missing this module raises, and if no gfx950 device is
present `pinn_create` fails with the library's own error message.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

# PyTorch ships its own copy of the HIP / HSA runtime (torch/lib/libamdhip64.so).  A process that maps libpinn_hip.so FIRST binds the
# engine to the system runtime (/opt/rocm) and then initialises a SECOND runtime when torch touches the device: the later one finds "no
# ROCm-capable device" (seen on hardware: build() followed by smoke() in one process).  With torch mapped first, the engine's HIP symbols
# resolve to the runtime torch already carries, and the two share one device context — which the zero-copy paths (device pointers and
# streams handed across the ABI) need anyway.  Hosts without torch (the Julia glue, the C client) use the system runtime alone.
try:
    import torch as _torch  # noqa: F401
except ImportError:          # pragma: no cover
    _torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_PATH = os.path.join(_HERE, "csrc", "libpinn_hip.so")

# every symbol declared in include/pinn_hip.h
SYMBOLS = [
    "pinn_backend", "pinn_abi_version", "pinn_last_error", "pinn_create", "pinn_destroy", "pinn_num_terms",
    "pinn_num_theta", "pinn_set_points", "pinn_set_points_device", "pinn_loss_grad", "pinn_loss_grad_f64",
    "pinn_term_grads", "pinn_loglik_grad", "pinn_loss_grad_device", "pinn_residual", "pinn_phi", "pinn_derivative", "pinn_last_timing", "pinn_set_timing", "pinn_describe", "pinn_num_groups", "pinn_group_timing",
    "pinn_create_on", "pinn_comm_unique_id", "pinn_comm_init_rank", "pinn_comm_init_all", "pinn_comm_size", "pinn_comm_rank", "pinn_comm_destroy",
    "pinn_loss_grad_sharded_device", "pinn_loss_grad_sharded",
    "pinn_set_sampler", "pinn_set_point_data", "pinn_set_point_weights", "pinn_get_points", "pinn_adam_init", "pinn_adam_steps", "pinn_adam_get", "pinn_lbfgs",
    "pinn_loss_device", "pinn_group_launched_by",
    "pinn_set_option", "pinn_get_option", "pinn_set_points_f64", "pinn_comm_init_custom", "pinn_adam_steps_sharded", "pinn_adam_apply",
    "pinn_adam_init_f64", "pinn_adam_get_f64", "pinn_set_point_data_f64", "pinn_loss_grad_device_f64",
    "pinn_residual_f64", "pinn_phi_f64", "pinn_derivative_f64", "pinn_term_grads_f64", "pinn_loglik_grad_f64",
    "pinn_loss_grad_sharded_device_f64", "pinn_loss_grad_sharded_f64",
    "pinn_hmc_init", "pinn_hmc_set_metric", "pinn_hmc_draws", "pinn_hmc_get", "pinn_hmc_find_stepsize", "pinn_hmc_warmup",
    "pinn_nuts_draws",
    "pinn_lbfgs_init", "pinn_lbfgs_steps", "pinn_lbfgs_get",
    "pinn_bfgs_init", "pinn_bfgs_steps", "pinn_bfgs_get",
    "pinn_phi_ensemble", "pinn_derivative_ensemble",
    "pinn_cubature_refine", "pinn_cubature_get",
]


class EngineError(RuntimeError):
    pass


class Library:
    """A loaded build of the engine ABI."""

    def __init__(self, path: str = DEFAULT_PATH):
        if not os.path.exists(path):
            raise EngineError(
                f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
                "The PINN engine has no CPU fallback.")
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        fp, dp, vp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p
        L.pinn_backend.restype = C.c_char_p
        L.pinn_abi_version.restype = C.c_int
        L.pinn_last_error.restype = C.c_char_p
        L.pinn_create.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.pinn_create_on.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
        L.pinn_comm_unique_id.argtypes = [vp, C.c_int64]
        L.pinn_comm_init_rank.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int64]
        L.pinn_comm_init_all.argtypes = [C.POINTER(vp), C.c_int]
        L.pinn_comm_size.argtypes = [vp]
        L.pinn_comm_rank.argtypes = [vp]
        L.pinn_comm_destroy.argtypes = [vp]
        L.pinn_loss_grad_sharded_device.argtypes = [vp, vp, fp, vp, vp]
        L.pinn_loss_grad_sharded.argtypes = [C.POINTER(vp), C.c_int, fp, C.c_int64, fp, dp, fp]
        L.pinn_destroy.argtypes = [vp]
        L.pinn_num_terms.argtypes = [vp]
        L.pinn_num_theta.argtypes = [vp]
        L.pinn_num_theta.restype = C.c_int64
        L.pinn_set_points.argtypes = [vp, C.c_int, fp, C.c_int64, C.c_int64]
        L.pinn_set_points_device.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int64]
        L.pinn_loss_grad.argtypes = [vp, fp, C.c_int64, fp, dp, fp]
        L.pinn_loss_grad_f64.argtypes = [vp, dp, C.c_int64, dp, dp, dp]
        L.pinn_term_grads.argtypes = [vp, fp, C.c_int64, dp, fp]
        L.pinn_loglik_grad.argtypes = [vp, fp, C.c_int64, dp, dp, fp, dp]
        L.pinn_loss_grad_device.argtypes = [vp, vp, fp, vp, vp]
        L.pinn_loss_device.argtypes = [vp, vp, vp, vp]
        L.pinn_group_launched_by.argtypes = [vp, C.c_int]
        L.pinn_residual.argtypes = [vp, C.c_int, fp, C.c_int64, fp]
        L.pinn_phi.argtypes = [vp, C.c_int, fp, C.c_int64, fp, C.c_int64, fp]
        L.pinn_derivative.argtypes = [vp, C.c_int, fp, C.c_int64, fp, C.c_int64, C.c_int, C.POINTER(C.c_int), fp]
        L.pinn_last_timing.argtypes = [vp, fp, fp]
        L.pinn_set_timing.argtypes = [vp, C.c_int, C.c_int]
        L.pinn_describe.argtypes = [vp, C.c_char_p, C.c_int64]
        L.pinn_num_groups.argtypes = [vp]
        L.pinn_set_sampler.argtypes = [vp, C.c_int, C.c_int, fp, fp, C.c_int64, C.c_uint64]
        L.pinn_get_points.argtypes = [vp, C.c_int, fp, C.c_int64]
        L.pinn_set_point_data.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int64]
        L.pinn_set_point_weights.argtypes = [vp, C.c_int, fp, C.c_int64]
        L.pinn_adam_init.argtypes = [vp, fp, C.c_int64]
        L.pinn_adam_steps.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, fp, dp]
        L.pinn_adam_get.argtypes = [vp, fp, C.c_int64]
        try:                                     # (r05 entry points: A/B variant libraries built before them still load for tools/ab_compare.py)
            L.pinn_adam_init_f64.argtypes = [vp, dp, C.c_int64]
            L.pinn_adam_get_f64.argtypes = [vp, dp, C.c_int64]
            L.pinn_set_point_data_f64.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int64]
            L.pinn_loss_grad_device_f64.argtypes = [vp, vp, fp, vp, vp]
            L.pinn_residual_f64.argtypes = [vp, C.c_int, dp, C.c_int64, dp]
            L.pinn_phi_f64.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_int64, dp]
            L.pinn_derivative_f64.argtypes = [vp, C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int, C.POINTER(C.c_int), dp]
            L.pinn_term_grads_f64.argtypes = [vp, dp, C.c_int64, dp, dp]
            L.pinn_loglik_grad_f64.argtypes = [vp, dp, C.c_int64, dp, dp, dp, dp]
            L.pinn_loss_grad_sharded_device_f64.argtypes = [vp, vp, fp, vp, vp]
            L.pinn_loss_grad_sharded_f64.argtypes = [C.POINTER(vp), C.c_int, dp, C.c_int64, dp, dp, dp]
        except AttributeError:
            pass
        try:                                     # (resident HMC: variant libraries built before it still load)
            L.pinn_hmc_init.argtypes = [vp, dp, C.c_int64, dp, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), dp, dp]
            L.pinn_hmc_set_metric.argtypes = [vp, dp, C.c_int64]
            L.pinn_hmc_draws.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint64, dp, dp, dp, C.c_int64, dp, dp]
            L.pinn_hmc_get.argtypes = [vp, dp, C.c_int64, dp, dp]
        except AttributeError:
            pass
        try:                                     # (resident HMC warm-up: variant libraries built before it still load)
            L.pinn_hmc_find_stepsize.argtypes = [vp, C.c_double, C.c_uint64, dp, C.c_int64, dp, C.POINTER(C.c_int)]
            L.pinn_hmc_warmup.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_uint64, dp, dp, dp, C.c_int64, dp, dp, dp, dp, dp]
        except AttributeError:
            pass
        try:                                     # (resident NUTS: variant libraries built before it still load)
            ip = C.POINTER(C.c_int)
            L.pinn_nuts_draws.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_uint64, dp, dp, dp, C.c_int64, dp, dp, ip, ip, ip]
        except AttributeError:
            pass
        try:                                     # (resident L-BFGS: variant libraries built before it still load)
            L.pinn_lbfgs_init.argtypes = [vp, dp, C.c_int64, C.c_int, fp]
            L.pinn_lbfgs_steps.argtypes = [vp, C.c_int, C.c_int, C.c_double, dp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.pinn_lbfgs_get.argtypes = [vp, dp, C.c_int64, dp, dp]
        except AttributeError:
            pass
        try:                                     # (resident BFGS: variant libraries built before it still load)
            L.pinn_bfgs_init.argtypes = [vp, dp, C.c_int64, fp]
            L.pinn_bfgs_steps.argtypes = [vp, C.c_int, C.c_int, C.c_double, dp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.pinn_bfgs_get.argtypes = [vp, dp, C.c_int64, dp, dp, dp]
        except AttributeError:
            pass
        try:                                     # (ensemble prediction: variant libraries built before it still load)
            L.pinn_phi_ensemble.argtypes = [vp, C.c_int, dp, C.c_int64, C.c_int64, dp, C.c_int64, C.c_int, dp, dp, dp]
        except AttributeError:
            pass
        try:                                     # (ensemble derivatives: variant libraries built before them still load)
            L.pinn_derivative_ensemble.argtypes = [vp, C.c_int, dp, C.c_int64, C.c_int64, dp, C.c_int64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, dp, dp, dp]
        except AttributeError:
            pass
        try:                                     # (adaptive cubature: variant libraries built before it still load)
            L.pinn_cubature_refine.argtypes = [vp, C.c_int, dp, C.c_int64, dp, dp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                               dp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.pinn_cubature_get.argtypes = [vp, C.c_int, dp, dp, C.c_int64]
        except AttributeError:
            pass
        L.pinn_lbfgs.argtypes = [vp, C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_int, C.c_double, fp, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        self.ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, vp, vp, C.c_int64, C.c_int, vp)
        L.pinn_comm_init_custom.argtypes = [vp, C.c_int, C.c_int, self.ALLREDUCE_FN, vp]
        L.pinn_adam_steps_sharded.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, fp, dp]
        L.pinn_adam_apply.argtypes = [vp, fp, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, fp, dp]
        L.pinn_set_points_f64.argtypes = [vp, C.c_int, dp, C.c_int64, C.c_int64]
        L.pinn_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
        L.pinn_get_option.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int64]
        L.pinn_group_timing.argtypes = [vp, C.c_int, fp, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]

    @property
    def backend(self) -> str:
        return self.lib.pinn_backend().decode()

    def last_error(self) -> str:
        return self.lib.pinn_last_error().decode()

    def check(self, rc: int, what: str):
        if rc != 0:
            raise EngineError(f"{what}: {self.last_error()}")


_default: Optional[Library] = None


def default_library() -> Library:
    global _default
    if _default is None:
        _default = Library(DEFAULT_PATH)
    return _default


def set_library(lib: Optional[Library]):
    """Replace the process-wide library object.  Used by the CPU test-suite to drive the host logic
    through tests/emu/libpinn_emu.so (same sources, wave emulation); never called by the package."""
    global _default
    _default = lib


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


COMM_ID_BYTES = 128


def comm_unique_id(lib: Optional[Library] = None) -> bytes:
    """rank 0 of a one-process-per-GPU job: the 128-byte id every rank passes to Engine.comm_init_rank"""
    L = lib or default_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    L.check(L.lib.pinn_comm_unique_id(buf, COMM_ID_BYTES), "pinn_comm_unique_id")
    return buf.raw


def comm_init_all(engines: Sequence["Engine"]):
    """single process, one engine per device (Engine(descriptor, device=g)): form their communicator (ncclCommInitAll)"""
    L = engines[0].L
    hs = (C.c_void_p * len(engines))(*[e.h for e in engines])
    L.check(L.lib.pinn_comm_init_all(hs, len(engines)), "pinn_comm_init_all")


def loss_grad_sharded(engines: Sequence["Engine"], theta, weights=None, want_grad: bool = True):
    """one evaluation over all devices of a comm_init_all communicator: every engine holds its shard of every term's point set
    (set_points(..., n_norm = global N)); returns the GLOBAL per-term losses and gradient (pinn_loss_grad_sharded)"""
    e0 = engines[0]
    L = e0.L
    hs = (C.c_void_p * len(engines))(*[e.h for e in engines])
    th = _f32(theta)
    losses = np.zeros(e0.K, dtype=np.float64)
    grad = np.zeros(e0.P, dtype=np.float32) if want_grad else None
    w = _f32(weights) if weights is not None else None
    L.check(L.lib.pinn_loss_grad_sharded(hs, len(engines), th.ctypes.data_as(C.POINTER(C.c_float)), th.size,
                                         w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
                                         losses.ctypes.data_as(C.POINTER(C.c_double)),
                                         grad.ctypes.data_as(C.POINTER(C.c_float)) if grad is not None else None), "pinn_loss_grad_sharded")
    return losses, grad


def loss_grad_sharded_f64(engines: Sequence["Engine"], theta, weights=None, want_grad: bool = True):
    """`pinn_loss_grad_sharded_f64`: the same over handles in float64 mode — theta, losses and gradient in double, one all-reduce of [P + K] doubles"""
    e0 = engines[0]
    L = e0.L
    hs = (C.c_void_p * len(engines))(*[e.h for e in engines])
    th = _f64(theta)
    losses = np.zeros(e0.K, dtype=np.float64)
    grad = np.zeros(e0.P, dtype=np.float64) if want_grad else None
    w = _f64(weights) if weights is not None else None
    L.check(L.lib.pinn_loss_grad_sharded_f64(hs, len(engines), th.ctypes.data_as(C.POINTER(C.c_double)), th.size,
                                             w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None,
                                             losses.ctypes.data_as(C.POINTER(C.c_double)),
                                             grad.ctypes.data_as(C.POINTER(C.c_double)) if grad is not None else None), "pinn_loss_grad_sharded_f64")
    return losses, grad


def adam_steps_sharded(engines: Sequence["Engine"], nsteps: int, lr: float, weights=None, beta1=0.9, beta2=0.999, eps=1e-8):
    """`pinn_adam_steps_sharded`: the resident Adam loop over the handles of one `comm_init_all` communicator (every handle
    `adam_init`-ed with the same theta): per iteration evaluate the local shards, ONE all-reduce, the same update on every device.
    Returns the loss history (rank 0's)."""
    L = engines[0].L
    hs = (C.c_void_p * len(engines))(*[e.h for e in engines])
    hist = np.zeros(nsteps, dtype=np.float64)
    w = _f32(weights) if weights is not None else None
    L.check(L.lib.pinn_adam_steps_sharded(hs, len(engines), nsteps, lr, beta1, beta2, eps,
                                          w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
                                          hist.ctypes.data_as(C.POINTER(C.c_double))), "pinn_adam_steps_sharded")
    return hist


class Engine:
    """One `pinn_handle`."""

    def __init__(self, descriptor: str, lib: Optional[Library] = None, device: int = -1):
        """device: HIP device index for single-process multi-GPU use (pinn_create_on); -1 = the caller's current device"""
        self.L = lib or default_library()
        self.h = C.c_void_p()
        self.descriptor = descriptor
        self.L.check(self.L.lib.pinn_create_on(descriptor.encode(), device, C.byref(self.h)), "pinn_create")
        self.K = self.L.lib.pinn_num_terms(self.h)
        self.P = int(self.L.lib.pinn_num_theta(self.h))
        # (no HIP events around the kernels of an evaluation unless a caller asks for timings with set_timing: the library's default since
        # r04 — the phase events behind pinn_last_timing cost 25 us per host-entry call, as much as a small problem's kernels)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.lib.pinn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_points(self, term: int, pts, n_norm: int = 0):
        """pts: (d x N) array as the reference holds it; stored point-major (Julia column-major)."""
        pts = np.asarray(pts)
        flat = _f32(pts.T).reshape(-1)     # (N x d) C-order == (d x N) Fortran order
        self.L.check(self.L.lib.pinn_set_points(self.h, term, flat.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[1], n_norm),
                     "pinn_set_points")

    def set_points_f64(self, term: int, pts, n_norm: int = 0):
        """`pinn_set_points_f64`: the set in double for the float64 evaluation mode (the fp32 kernels get its float conversion)"""
        pts = np.asarray(pts, dtype=np.float64)
        flat = np.ascontiguousarray(pts.T).reshape(-1)
        self.L.check(self.L.lib.pinn_set_points_f64(self.h, term, flat.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[1], n_norm), "pinn_set_points_f64")

    def set_points_device(self, term: int, dptr: int, n: int, n_norm: int = 0):
        self.L.check(self.L.lib.pinn_set_points_device(self.h, term, C.c_void_p(dptr), n, n_norm), "pinn_set_points_device")

    def loss_grad(self, theta, weights: Optional[Sequence[float]] = None, want_grad: bool = True):
        """K term losses (+ gradient).  want_grad=False is the LOSS-ONLY evaluation (grad = NULL at the ABI): forward pass + residuals +
        sums of squares, no reverse sweep — the same loss values at about a third of the cost."""
        th = _f32(theta)
        losses = np.zeros(self.K, dtype=np.float64)
        grad = np.zeros(self.P, dtype=np.float32) if want_grad else None
        w = _f32(weights) if weights is not None else None
        self.L.check(self.L.lib.pinn_loss_grad(
            self.h, th.ctypes.data_as(C.POINTER(C.c_float)), th.size,
            w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
            losses.ctypes.data_as(C.POINTER(C.c_double)),
            grad.ctypes.data_as(C.POINTER(C.c_float)) if grad is not None else None), "pinn_loss_grad")
        return losses, grad

    def loss_grad_f64(self, theta, weights=None, want_grad: bool = True):
        """theta, weights, losses and gradient in double at the ABI.  With the handle's precision option at "f64" the evaluation itself runs
        in double; otherwise the fp32 kernels run and the results are widened."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64))
        losses = np.zeros(self.K, dtype=np.float64)
        grad = np.zeros(self.P, dtype=np.float64) if want_grad else None
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64)) if weights is not None else None
        self.L.check(self.L.lib.pinn_loss_grad_f64(
            self.h, th.ctypes.data_as(C.POINTER(C.c_double)), th.size,
            w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None,
            losses.ctypes.data_as(C.POINTER(C.c_double)),
            grad.ctypes.data_as(C.POINTER(C.c_double)) if grad is not None else None), "pinn_loss_grad_f64")
        return losses, grad

    def term_grads(self, theta):
        th = _f32(theta)
        losses = np.zeros(self.K, dtype=np.float64)
        tg = np.zeros((self.K, self.P), dtype=np.float32)
        self.L.check(self.L.lib.pinn_term_grads(self.h, th.ctypes.data_as(C.POINTER(C.c_float)), th.size,
                                                losses.ctypes.data_as(C.POINTER(C.c_double)),
                                                tg.ctypes.data_as(C.POINTER(C.c_float))), "pinn_term_grads")
        return losses, tg

    def term_grads_f64(self, theta):
        """`pinn_term_grads_f64`: theta and the K x P per-term gradients in double (native in float64 mode)"""
        th = _f64(theta)
        losses = np.zeros(self.K, dtype=np.float64)
        tg = np.zeros((self.K, self.P), dtype=np.float64)
        self.L.check(self.L.lib.pinn_term_grads_f64(self.h, th.ctypes.data_as(C.POINTER(C.c_double)), th.size,
                                                    losses.ctypes.data_as(C.POINTER(C.c_double)),
                                                    tg.ctypes.data_as(C.POINTER(C.c_double))), "pinn_term_grads_f64")
        return losses, tg

    def loglik_grad_f64(self, theta, stds, want_grad: bool = True):
        """`pinn_loglik_grad_f64`: theta and d loglik / d theta in double (native in float64 mode)"""
        th = _f64(theta)
        sd = _f64(stds)
        if sd.shape != (self.K,):
            raise ValueError(f"need one std per loss term ({self.K})")
        ll = C.c_double()
        g = np.zeros(self.P, dtype=np.float64) if want_grad else None
        gs = np.zeros(self.K, dtype=np.float64)
        self.L.check(self.L.lib.pinn_loglik_grad_f64(self.h, th.ctypes.data_as(C.POINTER(C.c_double)), th.size, sd.ctypes.data_as(C.POINTER(C.c_double)),
                                                     C.byref(ll), g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
                                                     gs.ctypes.data_as(C.POINTER(C.c_double))), "pinn_loglik_grad_f64")
        return ll.value, g, gs

    def loglik_grad(self, theta, stds, want_grad: bool = True):
        """BPINN log-likelihood sum_k logpdf(MvNormal(r_k, std_k^2 I), 0), d/dtheta and d/dstd (pinn_loglik_grad)"""
        th = _f32(theta)
        sd = np.ascontiguousarray(np.asarray(stds, dtype=np.float64))
        if sd.shape != (self.K,):
            raise ValueError(f"need one std per loss term ({self.K})")
        ll = C.c_double()
        g = np.zeros(self.P, dtype=np.float32) if want_grad else None
        gs = np.zeros(self.K, dtype=np.float64)
        self.L.check(self.L.lib.pinn_loglik_grad(self.h, th.ctypes.data_as(C.POINTER(C.c_float)), th.size, sd.ctypes.data_as(C.POINTER(C.c_double)),
                                                 C.byref(ll), g.ctypes.data_as(C.POINTER(C.c_float)) if g is not None else None,
                                                 gs.ctypes.data_as(C.POINTER(C.c_double))), "pinn_loglik_grad")
        return ll.value, g, gs

    def loss_grad_device(self, d_theta: int, d_out: int, weights=None, stream: int = 0):
        w = _f32(weights) if weights is not None else None
        self.L.check(self.L.lib.pinn_loss_grad_device(
            self.h, C.c_void_p(d_theta), w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
            C.c_void_p(d_out), C.c_void_p(stream)), "pinn_loss_grad_device")

    def loss_grad_device_f64(self, d_theta: int, d_out: int, weights=None, stream: int = 0):
        """`pinn_loss_grad_device_f64`: a float64-mode handle on DOUBLE device buffers (d_theta: P doubles, d_out: P + K doubles)"""
        w = _f32(weights) if weights is not None else None
        self.L.check(self.L.lib.pinn_loss_grad_device_f64(
            self.h, C.c_void_p(d_theta), w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
            C.c_void_p(d_out), C.c_void_p(stream)), "pinn_loss_grad_device_f64")

    def loss_device(self, d_theta: int, d_sums: int, stream: int = 0):
        """loss-only evaluation on device pointers: d_sums = K floats (this shard's sums of squared residuals per term)"""
        self.L.check(self.L.lib.pinn_loss_device(self.h, C.c_void_p(d_theta), C.c_void_p(d_sums), C.c_void_p(stream)), "pinn_loss_device")

    # ---- engine-owned data parallelism (include/pinn_hip.h: pinn_comm_*) ----
    def comm_init_rank(self, nranks: int, rank: int, uid: bytes):
        """one process per GPU: join the communicator identified by `uid` (comm_unique_id() of rank 0, distributed by the host side)"""
        buf = C.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        self.L.check(self.L.lib.pinn_comm_init_rank(self.h, nranks, rank, buf, COMM_ID_BYTES), "pinn_comm_init_rank")

    def comm_size(self) -> int:
        return self.L.lib.pinn_comm_size(self.h)

    def comm_destroy(self):
        self.L.check(self.L.lib.pinn_comm_destroy(self.h), "pinn_comm_destroy")

    def loss_grad_sharded_device_f64(self, d_theta: int, d_out: int, weights=None, stream: int = 0):
        """`pinn_loss_grad_sharded_device_f64`: float64 mode, DOUBLE device buffers, the engine's all-reduce of [P + K] doubles on `stream`"""
        w = _f32(weights) if weights is not None else None
        self.L.check(self.L.lib.pinn_loss_grad_sharded_device_f64(
            self.h, C.c_void_p(d_theta), w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
            C.c_void_p(d_out), C.c_void_p(stream)), "pinn_loss_grad_sharded_device_f64")

    def loss_grad_sharded_device(self, d_theta: int, d_out: int, weights=None, stream: int = 0):
        """pinn_loss_grad_device on this rank's shards + the engine's all-reduce of d_out ([P + K] floats, device memory) on `stream`"""
        w = _f32(weights) if weights is not None else None
        self.L.check(self.L.lib.pinn_loss_grad_sharded_device(
            self.h, C.c_void_p(d_theta), w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
            C.c_void_p(d_out), C.c_void_p(stream)), "pinn_loss_grad_sharded_device")

    def residual(self, term: int, theta, n: int) -> np.ndarray:
        th = _f32(theta)
        r = np.zeros(n, dtype=np.float32)
        self.L.check(self.L.lib.pinn_residual(self.h, term, th.ctypes.data_as(C.POINTER(C.c_float)), th.size,
                                              r.ctypes.data_as(C.POINTER(C.c_float))), "pinn_residual")
        return r

    def residual_f64(self, term: int, theta, n: int) -> np.ndarray:
        """`pinn_residual_f64`: the term's residuals in double (native in float64 mode: equal to a Float64 evaluation to rounding)"""
        th = _f64(theta)
        r = np.zeros(n, dtype=np.float64)
        self.L.check(self.L.lib.pinn_residual_f64(self.h, term, th.ctypes.data_as(C.POINTER(C.c_double)), th.size,
                                                  r.ctypes.data_as(C.POINTER(C.c_double))), "pinn_residual_f64")
        return r

    def phi_f64(self, net: int, theta, pts) -> np.ndarray:
        """`pinn_phi_f64`: the trial function at the columns of pts (d x N), everything in double"""
        return self.derivative_f64(net, theta, pts, ())

    def derivative_f64(self, net: int, theta, pts, axes: Sequence[int]) -> np.ndarray:
        """`pinn_derivative_f64`: d^k phi_net / dx_axes in double (numeric_derivative at the reference's Float64 tolerances,
        test/Forward/forward__derivatives.jl:29-44)"""
        th = _f64(theta)
        pts = np.asarray(pts, dtype=np.float64)
        flat = np.ascontiguousarray(pts.T).reshape(-1)
        out = np.zeros(pts.shape[1], dtype=np.float64)
        ax = (C.c_int * max(len(axes), 1))(*[int(a) for a in axes])
        if len(axes) == 0:
            self.L.check(self.L.lib.pinn_phi_f64(self.h, net, th.ctypes.data_as(C.POINTER(C.c_double)), th.size,
                                                 flat.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[1],
                                                 out.ctypes.data_as(C.POINTER(C.c_double))), "pinn_phi_f64")
        else:
            self.L.check(self.L.lib.pinn_derivative_f64(self.h, net, th.ctypes.data_as(C.POINTER(C.c_double)), th.size,
                                                        flat.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[1], len(axes), ax,
                                                        out.ctypes.data_as(C.POINTER(C.c_double))), "pinn_derivative_f64")
        return out

    def phi_ensemble(self, net: int, thetas, pts, ddof: int = 0, return_preds: bool = False):
        """`pinn_phi_ensemble`: the trial function of network `net` at every row of thetas (S x P full parameter vectors) and the columns of
        pts (d x N; a single point may be given as (d,)), reduced over the rows on the device: -> (mean, std[, preds (S x N)]), `std` with
        numpy's `ddof`.  The compute type follows the handle (double in float64 mode, the float kernel otherwise); the statistics are in double."""
        th = np.atleast_2d(_f64(thetas))
        pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim == 1:
            pts = pts.reshape(-1, 1)
        flat = np.ascontiguousarray(pts.T).reshape(-1)
        n, dp = pts.shape[1], C.POINTER(C.c_double)
        mean, std = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        preds = np.zeros((th.shape[0], n), dtype=np.float64) if return_preds else None
        self.L.check(self.L.lib.pinn_phi_ensemble(self.h, int(net), th.ctypes.data_as(dp), th.shape[0], th.shape[1], flat.ctypes.data_as(dp), n, int(ddof),
                                                  mean.ctypes.data_as(dp), std.ctypes.data_as(dp), preds.ctypes.data_as(dp) if return_preds else None),
                     "pinn_phi_ensemble")
        return (mean, std, preds) if return_preds else (mean, std)

    def derivative_ensemble(self, net: int, thetas, pts, requests, ddof: int = 0, return_preds: bool = False):
        """`pinn_derivative_ensemble`: derivatives of the trial function of network `net` at every row of thetas (S x P full parameter vectors)
        and the columns of pts (d x N; a single point may be given as (d,)), reduced over the rows on the device.  `requests` = [(order, axes),
        ...]: request j is d^order phi / dx_axes (order 0, axes (): phi itself; order 2 may be mixed; orders 3 and 4 along one axis).
        -> (mean (R x N), std (R x N)[, preds (R x S x N)]), `std` with numpy's `ddof`.  The compute type follows the handle, as in `phi_ensemble`."""
        th = np.atleast_2d(_f64(thetas))
        pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim == 1:
            pts = pts.reshape(-1, 1)
        flat = np.ascontiguousarray(pts.T).reshape(-1)
        n, dp, R = pts.shape[1], C.POINTER(C.c_double), len(requests)
        orders = (C.c_int * max(R, 1))(*[int(o) for o, _ in requests])
        axes = (C.c_int * (4 * max(R, 1)))()
        for j, (o, ax) in enumerate(requests):
            ax = [int(a) for a in ax]
            if len(ax) != int(o) or len(ax) > 4:
                raise ValueError(f"request {j}: order {o} takes {o} axes (at most 4), not {ax}")
            axes[4 * j:4 * j + len(ax)] = ax
        mean, std = np.zeros((R, n), dtype=np.float64), np.zeros((R, n), dtype=np.float64)
        preds = np.zeros((R, th.shape[0], n), dtype=np.float64) if return_preds else None
        self.L.check(self.L.lib.pinn_derivative_ensemble(self.h, int(net), th.ctypes.data_as(dp), th.shape[0], th.shape[1], flat.ctypes.data_as(dp), n,
                                                         R, orders, axes, int(ddof), mean.ctypes.data_as(dp), std.ctypes.data_as(dp),
                                                         preds.ctypes.data_as(dp) if return_preds else None), "pinn_derivative_ensemble")
        return (mean, std, preds) if return_preds else (mean, std)

    def phi(self, net: int, theta, pts) -> np.ndarray:
        th = _f32(theta)
        pts = np.asarray(pts)
        flat = _f32(pts.T).reshape(-1)
        out = np.zeros(pts.shape[1], dtype=np.float32)
        self.L.check(self.L.lib.pinn_phi(self.h, net, th.ctypes.data_as(C.POINTER(C.c_float)), th.size,
                                         flat.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[1],
                                         out.ctypes.data_as(C.POINTER(C.c_float))), "pinn_phi")
        return out

    def derivative(self, net: int, theta, pts, axes: Sequence[int]) -> np.ndarray:
        """d^k phi_net / dx_axes at the columns of pts (d x N): the engine's counterpart of numeric_derivative (src/pinn_types.jl:445-482)"""
        th = _f32(theta)
        pts = np.asarray(pts)
        flat = _f32(pts.T).reshape(-1)
        out = np.zeros(pts.shape[1], dtype=np.float32)
        ax = (C.c_int * max(len(axes), 1))(*[int(a) for a in axes])
        self.L.check(self.L.lib.pinn_derivative(self.h, net, th.ctypes.data_as(C.POINTER(C.c_float)), th.size,
                                                flat.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[1], len(axes), ax,
                                                out.ctypes.data_as(C.POINTER(C.c_float))), "pinn_derivative")
        return out

    def set_timing(self, level: int, group: int = -1):
        self.L.check(self.L.lib.pinn_set_timing(self.h, level, group), "pinn_set_timing")

    def last_timing(self):
        k, t = C.c_float(), C.c_float()
        self.L.check(self.L.lib.pinn_last_timing(self.h, C.byref(k), C.byref(t)), "pinn_last_timing")
        return k.value, t.value

    def set_point_data(self, term: int, data):
        """data: (ndata x N) per-point channels of the term's current point set (descriptor op DATA j)"""
        data = _f32(np.atleast_2d(np.asarray(data)))
        self.L.check(self.L.lib.pinn_set_point_data(self.h, term, data.ctypes.data_as(C.POINTER(C.c_float)), data.shape[0], data.shape[1]),
                     "pinn_set_point_data")

    def set_point_data_f64(self, term: int, data):
        """`pinn_set_point_data_f64`: the observations in double for the float64 evaluation mode (the fp32 kernels get their float conversion)"""
        data = np.ascontiguousarray(np.atleast_2d(np.asarray(data, dtype=np.float64)))
        self.L.check(self.L.lib.pinn_set_point_data_f64(self.h, term, data.ctypes.data_as(C.POINTER(C.c_double)), data.shape[0], data.shape[1]),
                     "pinn_set_point_data_f64")

    def set_point_weights(self, term: int, w):
        """quadrature weights of the term's current point set: loss_k = sum_i w_i r_i^2 (None: back to mean(abs2, r))"""
        if w is None:
            self.L.check(self.L.lib.pinn_set_point_weights(self.h, term, None, 0), "pinn_set_point_weights")
            return
        w = _f32(np.asarray(w).reshape(-1))
        self.L.check(self.L.lib.pinn_set_point_weights(self.h, term, w.ctypes.data_as(C.POINTER(C.c_float)), w.size), "pinn_set_point_weights")

    def get_points(self, term: int, d: int, n: int) -> np.ndarray:
        """the term's current set as a (d x N) array (e.g. what the device sampler drew last)"""
        buf = np.zeros((n, d), dtype=np.float32)
        self.L.check(self.L.lib.pinn_get_points(self.h, term, buf.ctypes.data_as(C.POINTER(C.c_float)), n), "pinn_get_points")
        return buf.T.copy()

    def set_sampler(self, term: int, lb, ub, n: int, seed: int = 0, kind: int = 1):
        lb, ub = _f32(lb), _f32(ub)
        self.L.check(self.L.lib.pinn_set_sampler(self.h, term, kind, lb.ctypes.data_as(C.POINTER(C.c_float)),
                                                 ub.ctypes.data_as(C.POINTER(C.c_float)), n, seed), "pinn_set_sampler")

    def adam(self, theta, nsteps: int, lr: float, weights=None, beta1=0.9, beta2=0.999, eps=1e-8, init=True):
        """`nsteps` Adam iterations with theta resident on the device; returns (theta, loss history).  init=False continues from the
        optimiser state on the device (theta is not read)."""
        th = _f32(theta) if init else None
        if init:
            self.L.check(self.L.lib.pinn_adam_init(self.h, th.ctypes.data_as(C.POINTER(C.c_float)), th.size), "pinn_adam_init")
        hist = np.zeros(nsteps, dtype=np.float64)
        w = _f32(weights) if weights is not None else None
        self.L.check(self.L.lib.pinn_adam_steps(self.h, nsteps, lr, beta1, beta2, eps,
                                                w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
                                                hist.ctypes.data_as(C.POINTER(C.c_double))), "pinn_adam_steps")
        out = np.zeros(self.P, dtype=np.float32)
        self.L.check(self.L.lib.pinn_adam_get(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "pinn_adam_get")
        return out, hist

    def adam_f64(self, theta, nsteps: int, lr: float, weights=None, beta1=0.9, beta2=0.999, eps=1e-8, init=True):
        """the same through the double entry points (pinn_adam_init_f64 / pinn_adam_get_f64): on a handle in float64 mode every kernel of the
        loop — redraw, residual + gradient, Adam — runs in double on the device; returns (theta float64, loss history)"""
        if init:
            th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64))
            self.L.check(self.L.lib.pinn_adam_init_f64(self.h, th.ctypes.data_as(C.POINTER(C.c_double)), th.size), "pinn_adam_init_f64")
        hist = np.zeros(nsteps, dtype=np.float64)
        w = _f32(weights) if weights is not None else None
        self.L.check(self.L.lib.pinn_adam_steps(self.h, nsteps, lr, beta1, beta2, eps,
                                                w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
                                                hist.ctypes.data_as(C.POINTER(C.c_double))), "pinn_adam_steps")
        out = np.zeros(self.P, dtype=np.float64)
        self.L.check(self.L.lib.pinn_adam_get_f64(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), out.size), "pinn_adam_get_f64")
        return out, hist

    def lbfgs(self, theta, maxiters: int, weights=None, history: int = 10, gtol: float = 1e-8):
        """`pinn_lbfgs`: L-BFGS on the weighted objective over the installed (fixed) point sets; returns (theta float64, objective after
        every performed iteration)."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64)).copy()
        hist = np.zeros(int(maxiters), dtype=np.float64)
        done = C.c_int(0)
        w = _f32(weights) if weights is not None else None
        self.L.check(self.L.lib.pinn_lbfgs(self.h, th.ctypes.data_as(C.POINTER(C.c_double)), th.size, int(maxiters), int(history), float(gtol),
                                           w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
                                           hist.ctypes.data_as(C.POINTER(C.c_double)), C.byref(done)), "pinn_lbfgs")
        return th, hist[:done.value]

    # ---- resident L-BFGS (include/pinn_hip.h: pinn_lbfgs_init / _steps / _get) ----
    LBFGS_STATUS = ("RUN", "RETRY", "CONVERGED", "STALLED", "MAXITER")

    def _qn_init(self, symbol, theta, weights, *history):
        """the _init call of a resident quasi-Newton solver: theta in double, the term weights as floats (or none), L-BFGS's history between"""
        th = _f64(theta)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32)) if weights is not None else None
        self.L.check(getattr(self.L.lib, symbol)(self.h, th.ctypes.data_as(C.POINTER(C.c_double)), th.size, *history,
                                                 w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None), symbol)

    def _qn_steps(self, symbol, maxiters, max_evals, gtol):
        """the _steps call of a resident quasi-Newton solver -> (objective after every performed iteration, evaluations, status name)"""
        hist = np.zeros(max(int(maxiters), 1), dtype=np.float64)
        it, ev, st = C.c_int(0), C.c_int(0), C.c_int(0)
        me = 31 * max(int(maxiters), 1) if max_evals is None else int(max_evals)
        self.L.check(getattr(self.L.lib, symbol)(self.h, int(maxiters), me, float(gtol), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                                 C.byref(it), C.byref(ev), C.byref(st)), symbol)
        return hist[:it.value], ev.value, self.LBFGS_STATUS[st.value]

    def lbfgs_init(self, theta, weights=None, history: int = 10):
        """`pinn_lbfgs_init`: put the device-resident L-BFGS state at theta; the term weights are fixed here."""
        self._qn_init("pinn_lbfgs_init", theta, weights, int(history))

    def lbfgs_steps(self, maxiters: int, max_evals: int = None, gtol: float = 1e-8):
        """`pinn_lbfgs_steps`: at most `maxiters` further iterations / `max_evals` further trial evaluations (default: 31 per iteration, which
        never binds) from the stored state.  Returns (objective after every performed iteration, evaluations, status name)."""
        return self._qn_steps("pinn_lbfgs_steps", maxiters, max_evals, gtol)

    def lbfgs_get(self, want_grad: bool = True):
        """`pinn_lbfgs_get`: (theta, objective, gradient) of the current iterate"""
        th = np.zeros(self.P, dtype=np.float64)
        g = np.zeros(self.P, dtype=np.float64) if want_grad else None
        f, dp = C.c_double(), C.POINTER(C.c_double)
        self.L.check(self.L.lib.pinn_lbfgs_get(self.h, th.ctypes.data_as(dp), th.size, C.byref(f), g.ctypes.data_as(dp) if g is not None else None), "pinn_lbfgs_get")
        return th, f.value, g

    # ---- resident BFGS (include/pinn_hip.h: pinn_bfgs_init / _steps / _get) ----
    BFGS_STATUS = LBFGS_STATUS

    def bfgs_init(self, theta, weights=None):
        """`pinn_bfgs_init`: put the device-resident dense BFGS state at theta with H = I; the term weights are fixed here."""
        self._qn_init("pinn_bfgs_init", theta, weights)

    def bfgs_steps(self, maxiters: int, max_evals: int = None, gtol: float = 1e-8):
        """`pinn_bfgs_steps`: at most `maxiters` further iterations / `max_evals` further trial evaluations (default: 31 per iteration, which
        never binds) from the stored state.  Returns (objective after every performed iteration, evaluations, status name)."""
        return self._qn_steps("pinn_bfgs_steps", maxiters, max_evals, gtol)

    def bfgs_get(self, want_grad: bool = True, want_hinv: bool = False):
        """`pinn_bfgs_get`: (theta, objective, gradient, inverse-Hessian approximation [P, P]) of the current iterate; what was not asked
        for is None"""
        th = np.zeros(self.P, dtype=np.float64)
        g = np.zeros(self.P, dtype=np.float64) if want_grad else None
        hinv = np.zeros((self.P, self.P), dtype=np.float64) if want_hinv else None
        f, dp = C.c_double(), C.POINTER(C.c_double)
        self.L.check(self.L.lib.pinn_bfgs_get(self.h, th.ctypes.data_as(dp), th.size, C.byref(f), g.ctypes.data_as(dp) if g is not None else None,
                                              hinv.ctypes.data_as(dp) if hinv is not None else None), "pinn_bfgs_get")
        return th, f.value, g, hinv

    # ---- adaptive cubature (include/pinn_hip.h: pinn_cubature_refine / _get) ----
    CUBATURE_STATUS = ("CONVERGED", "MAX_REGIONS", "MAX_ROUNDS", "NONFINITE")

    def cubature_refine(self, term: int, theta, lb, ub, reltol: float = 1e-6, abstol: float = 1e-3, max_regions: int = 4096, max_rounds: int = 32,
                        nodes: int = 4):
        """`pinn_cubature_refine`: refine term `term`'s mesh over [lb, ub] at theta on the device and install the composite Gauss-Legendre rule
        (`nodes` per free axis per box) as its weighted point set.  Returns dict(integral, error, nregions, npoints, rounds, status)."""
        th, lo, hi = _f64(theta), _f64(lb).reshape(-1), _f64(ub).reshape(-1)
        if lo.size != hi.size:
            raise ValueError("lb and ub: one value per coordinate each")
        dp = C.POINTER(C.c_double)
        I, Er, nr, npts, rd, st = C.c_double(), C.c_double(), C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        self.L.check(self.L.lib.pinn_cubature_refine(self.h, int(term), th.ctypes.data_as(dp), th.size, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), lo.size,
                                                     float(reltol), float(abstol), int(max_regions), int(max_rounds), int(nodes), C.byref(I), C.byref(Er),
                                                     C.byref(nr), C.byref(npts), C.byref(rd), C.byref(st)), "pinn_cubature_refine")
        return dict(integral=I.value, error=Er.value, nregions=nr.value, npoints=npts.value, rounds=rd.value, status=st.value)

    def cubature_get(self, term: int, nregions: int, d: int):
        """`pinn_cubature_get`: (boxes [nregions, 2, d] — lo, hi —, est [nregions, 2] — I7, err) of the term's last refinement"""
        boxes, est = np.zeros((int(nregions), 2, int(d)), dtype=np.float64), np.zeros((int(nregions), 2), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        self.L.check(self.L.lib.pinn_cubature_get(self.h, int(term), boxes.ctypes.data_as(dp), est.ctypes.data_as(dp), int(nregions)), "pinn_cubature_get")
        return boxes, est

    # ---- resident HMC (include/pinn_hip.h: pinn_hmc_*) ----
    def hmc_init(self, theta, stds, nn_prior=(0.0, 2.0), param_priors=()):
        """`pinn_hmc_init`: put a chain at theta.  stds: one per loss term; nn_prior = (mu, sigma) of the Normal prior on the network weights;
        param_priors: one (kind, mu, sigma) per trailing PDE parameter, kind 0 / "normal" or 1 / "lognormal"."""
        th, sd = _f64(theta), _f64(stds).reshape(-1)
        kinds = {"normal": 0, "lognormal": 1}
        kd = np.ascontiguousarray([kinds.get(str(q[0]).lower(), q[0]) for q in param_priors], dtype=np.int32)
        mu, sg = _f64([q[1] for q in param_priors]), _f64([q[2] for q in param_priors])
        dp = C.POINTER(C.c_double)
        self.L.check(self.L.lib.pinn_hmc_init(self.h, th.ctypes.data_as(dp), th.size, sd.ctypes.data_as(dp), sd.size, float(nn_prior[0]), float(nn_prior[1]),
                                              kd.size, kd.ctypes.data_as(C.POINTER(C.c_int)) if kd.size else None,
                                              mu.ctypes.data_as(dp) if kd.size else None, sg.ctypes.data_as(dp) if kd.size else None), "pinn_hmc_init")

    def hmc_set_metric(self, inv_metric=None):
        """`pinn_hmc_set_metric`: the diagonal inverse mass matrix (None: ones)"""
        m = None if inv_metric is None else _f64(inv_metric).reshape(-1)
        self.L.check(self.L.lib.pinn_hmc_set_metric(self.h, m.ctypes.data_as(C.POINTER(C.c_double)) if m is not None else None,
                                                    m.size if m is not None else self.P), "pinn_hmc_set_metric")

    def hmc_draws(self, ndraws: int, n_leapfrog: int, eps: float, seed: int = 0, momenta=None, uniforms=None, want_samples: bool = True):
        """`pinn_hmc_draws`: `ndraws` transitions on the device, one download.  Returns (samples [ndraws x P] or None, accept_prob, logp).
        momenta ([ndraws x P]) / uniforms ([ndraws]) replace the device generator's draws when given."""
        nd, dp = max(int(ndraws), 0), C.POINTER(C.c_double)
        mom = None if momenta is None else _f64(momenta).reshape(-1)
        uni = None if uniforms is None else _f64(uniforms).reshape(-1)
        if (mom is not None and mom.size != nd * self.P) or (uni is not None and uni.size != nd):
            raise ValueError("momenta: ndraws x P values, uniforms: ndraws values")
        smp = np.zeros((nd, self.P), dtype=np.float64) if want_samples else None
        acc, lp = np.zeros(nd, dtype=np.float64), np.zeros(nd, dtype=np.float64)
        self.L.check(self.L.lib.pinn_hmc_draws(self.h, int(ndraws), int(n_leapfrog), float(eps), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               mom.ctypes.data_as(dp) if mom is not None else None, uni.ctypes.data_as(dp) if uni is not None else None,
                                               smp.ctypes.data_as(dp) if smp is not None else None, self.P, acc.ctypes.data_as(dp), lp.ctypes.data_as(dp)),
                     "pinn_hmc_draws")
        return smp, acc, lp

    def hmc_get(self, want_grad: bool = True):
        """`pinn_hmc_get`: (theta, logp, d logp / d theta) of the chain's current state"""
        th = np.zeros(self.P, dtype=np.float64)
        g = np.zeros(self.P, dtype=np.float64) if want_grad else None
        lp, dp = C.c_double(), C.POINTER(C.c_double)
        self.L.check(self.L.lib.pinn_hmc_get(self.h, th.ctypes.data_as(dp), th.size, C.byref(lp), g.ctypes.data_as(dp) if g is not None else None), "pinn_hmc_get")
        return th, lp.value, g

    def hmc_find_stepsize(self, eps0: float, seed: int = 0, normals=None):
        """`pinn_hmc_find_stepsize`: the initial step-size search from the chain's current state, which it leaves alone.  normals: P standard
        normals (None: the device generator at its reserved counter).  Returns (eps, ntrials)."""
        z = None if normals is None else _f64(normals).reshape(-1)
        if z is not None and z.size != self.P:
            raise ValueError("normals: P values")
        eps, nt, dp = C.c_double(), C.c_int(), C.POINTER(C.c_double)
        self.L.check(self.L.lib.pinn_hmc_find_stepsize(self.h, float(eps0), int(seed) & 0xFFFFFFFFFFFFFFFF, z.ctypes.data_as(dp) if z is not None else None,
                                                       self.P, C.byref(eps), C.byref(nt)), "pinn_hmc_find_stepsize")
        return eps.value, nt.value

    def hmc_warmup(self, n_adapts: int, n_leapfrog: int, eps0: float, target: float = 0.8, seed: int = 0, normals=None, uniforms=None):
        """`pinn_hmc_warmup`: `n_adapts` transitions with the step size (dual averaging) and the diagonal metric (windowed variance) adapted on
        the device, one download.  normals ([n_adapts x P] STANDARD normals: the device divides by sqrt(metric)) / uniforms ([n_adapts]) replace
        the device generator's draws when given.  Returns (samples, accept_prob, logp, step_sizes, eps_final, inv_metric); the handle holds
        inv_metric afterwards and `hmc_draws(..., eps_final, ...)` continues the run."""
        nd, dp = max(int(n_adapts), 0), C.POINTER(C.c_double)
        z = None if normals is None else _f64(normals).reshape(-1)
        uni = None if uniforms is None else _f64(uniforms).reshape(-1)
        if (z is not None and z.size != nd * self.P) or (uni is not None and uni.size != nd):
            raise ValueError("normals: n_adapts x P values, uniforms: n_adapts values")
        smp = np.zeros((nd, self.P), dtype=np.float64)
        acc, lp, steps, minv = np.zeros(nd, dtype=np.float64), np.zeros(nd, dtype=np.float64), np.zeros(nd, dtype=np.float64), np.zeros(self.P, dtype=np.float64)
        eps = C.c_double()
        self.L.check(self.L.lib.pinn_hmc_warmup(self.h, int(n_adapts), int(n_leapfrog), float(eps0), float(target), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                z.ctypes.data_as(dp) if z is not None else None, uni.ctypes.data_as(dp) if uni is not None else None,
                                                smp.ctypes.data_as(dp), self.P, acc.ctypes.data_as(dp), lp.ctypes.data_as(dp), steps.ctypes.data_as(dp),
                                                C.byref(eps), minv.ctypes.data_as(dp)), "pinn_hmc_warmup")
        return smp, acc, lp, steps, eps.value, minv

    def nuts_draws(self, ndraws: int, max_depth: int, eps: float, seed: int = 0, normals=None, uniforms=None, delta_max: float = 1000.0):
        """`pinn_nuts_draws`: `ndraws` No-U-Turn transitions of the chain of `hmc_init` on the device, one download.  normals ([ndraws x P]
        STANDARD normals) / uniforms ([ndraws x (2 D + 2^D - 1)], D = max_depth: u_dir | u_merge | u_leaf) replace the device generator's draws
        when given.  Returns (samples [ndraws x P], accept_stat, logp, tree_depth, n_leapfrog, divergent)."""
        nd, dp, ip = max(int(ndraws), 0), C.POINTER(C.c_double), C.POINTER(C.c_int)
        nu = 2 * int(max_depth) + (1 << min(max(int(max_depth), 0), 10)) - 1
        z = None if normals is None else _f64(normals).reshape(-1)
        uni = None if uniforms is None else _f64(uniforms).reshape(-1)
        if (z is not None and z.size != nd * self.P) or (uni is not None and uni.size != nd * nu):
            raise ValueError("normals: ndraws x P values, uniforms: ndraws x (2 max_depth + 2^max_depth - 1) values")
        smp = np.zeros((nd, self.P), dtype=np.float64)
        acc, lp = np.zeros(nd, dtype=np.float64), np.zeros(nd, dtype=np.float64)
        depth, nleap, div = np.zeros(nd, dtype=np.int32), np.zeros(nd, dtype=np.int32), np.zeros(nd, dtype=np.int32)
        self.L.check(self.L.lib.pinn_nuts_draws(self.h, int(ndraws), int(max_depth), float(eps), float(delta_max), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                z.ctypes.data_as(dp) if z is not None else None, uni.ctypes.data_as(dp) if uni is not None else None,
                                                smp.ctypes.data_as(dp), self.P, acc.ctypes.data_as(dp), lp.ctypes.data_as(dp),
                                                depth.ctypes.data_as(ip), nleap.ctypes.data_as(ip), div.ctypes.data_as(ip)), "pinn_nuts_draws")
        return smp, acc, lp, depth, nleap, div

    def adam_init_f64(self, theta):
        th = _f64(theta)
        self.L.check(self.L.lib.pinn_adam_init_f64(self.h, th.ctypes.data_as(C.POINTER(C.c_double)), th.size), "pinn_adam_init_f64")

    def adam_get_f64(self) -> np.ndarray:
        out = np.zeros(self.P, dtype=np.float64)
        self.L.check(self.L.lib.pinn_adam_get_f64(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), out.size), "pinn_adam_get_f64")
        return out

    def adam_init(self, theta):
        th = _f32(theta)
        self.L.check(self.L.lib.pinn_adam_init(self.h, th.ctypes.data_as(C.POINTER(C.c_float)), th.size), "pinn_adam_init")

    def adam_get(self) -> np.ndarray:
        out = np.zeros(self.P, dtype=np.float32)
        self.L.check(self.L.lib.pinn_adam_get(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "pinn_adam_get")
        return out

    def adam_apply(self, grad_and_sums, lr: float, weights=None, beta1=0.9, beta2=0.999, eps=1e-8) -> float:
        """`pinn_adam_apply`: one Adam update of the resident state from a host vector [gradient (P) | raw per-term sums (K)]"""
        v = _f32(grad_and_sums)
        w = _f32(weights) if weights is not None else None
        loss = C.c_double(0.0)
        self.L.check(self.L.lib.pinn_adam_apply(self.h, v.ctypes.data_as(C.POINTER(C.c_float)), v.size, lr, beta1, beta2, eps,
                                                w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None, C.byref(loss)), "pinn_adam_apply")
        return loss.value

    def comm_init_custom(self, nranks: int, rank: int, allreduce):
        """`pinn_comm_init_custom`: `allreduce(buf_ptr, count, dtype, stream_ptr) -> int` (dtype 0 float / 1 double) becomes the transport of
        this handle's communicator; the ctypes callback object is kept alive by the engine wrapper."""
        def _cb(ctx, buf, count, dtype, stream):
            try:
                return int(allreduce(buf, count, dtype, stream) or 0)
            except Exception:                                           # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._allreduce_cb = self.L.ALLREDUCE_FN(_cb)
        self.L.check(self.L.lib.pinn_comm_init_custom(self.h, nranks, rank, self._allreduce_cb, None), "pinn_comm_init_custom")

    def set_option(self, name: str, value: str):
        """run-time options of the handle (include/pinn_hip.h: pinn_set_option); "gemm" = "split" | "fp32" """
        self.L.check(self.L.lib.pinn_set_option(self.h, name.encode(), value.encode()), "pinn_set_option")

    def get_option(self, name: str) -> str:
        buf = C.create_string_buffer(64)
        self.L.check(self.L.lib.pinn_get_option(self.h, name.encode(), buf, 64), "pinn_get_option")
        return buf.value.decode()

    def group_timings(self):
        out = []
        for g in range(self.L.lib.pinn_num_groups(self.h)):
            ms, pts, ch, tiles = C.c_float(), C.c_int64(), C.c_int(), C.c_int()
            self.L.check(self.L.lib.pinn_group_timing(self.h, g, C.byref(ms), C.byref(pts), C.byref(ch), C.byref(tiles)),
                         "pinn_group_timing")
            out.append(dict(group=g, ms=ms.value, points=pts.value, channels=ch.value, tiles=tiles.value,
                            launched_by=self.L.lib.pinn_group_launched_by(self.h, g)))
        return out

    def describe(self) -> str:
        buf = C.create_string_buffer(4096)
        self.L.check(self.L.lib.pinn_describe(self.h, buf, 4096), "pinn_describe")
        return buf.value.decode()
