"""ctypes binding of the C ABI declared in include/ace_hip.h.

The shared library `libace_hip.so` is built in-tree (see build.py).  There is
no CPU fallback: if the library (or a GPU, for device entry points) is
missing, calls raise AceError.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACE_LIB_PATH") or os.path.join(_HERE, "libace_hip.so")

ACE_KERNEL_SE = 0
ACE_KERNEL_MATERN32 = 1
KIND = {"SE": ACE_KERNEL_SE, "Matern32": ACE_KERNEL_MATERN32}

# the header's types: int, double, int64_t, char*, void* (every handle) and
# the pointers double*, int*, int32_t*, uint32_t*, int64_t*, void**
_int = ctypes.c_int
_dbl = ctypes.c_double
_I64 = ctypes.c_int64
_str = ctypes.c_char_p
_vp = ctypes.c_void_p
_D = ctypes.POINTER(ctypes.c_double)
_IP = ctypes.POINTER(ctypes.c_int)
_I32 = ctypes.POINTER(ctypes.c_int32)
_U32 = ctypes.POINTER(ctypes.c_uint32)
_I64P = ctypes.POINTER(ctypes.c_int64)
_VPP = ctypes.POINTER(_vp)

# name -> (restype, argtypes); must match include/ace_hip.h exactly
SIGNATURES = {
    "ace_abi_version": (_int, []),
    "ace_create": (_int, [_int, _VPP]),
    "ace_destroy": (None, [_vp]),
    "ace_last_error": (_str, [_vp]),
    "ace_set_interrupt_poll": (_int, [_vp, _vp, _vp]),
    "ace_kernmat_cross": (_int, [_vp, _int, _I64, _I64, _int, _int, _D, _D, _D, _D, _D, _D, _D]),
    "ace_kernmat_sym": (_int, [_vp, _int, _I64, _int, _int, _D, _D, _D, _D, _D]),
    "ace_invkernel": (_int, [_vp, _I64, _D, _dbl, _D, _D]),
    "ace_grad": (_int, [_vp, _int, _I64, _int, _int, _D, _D, _D, _D, _D, _D, _D, _D, _D, _dbl,
                        _D]),
    "ace_stats": (_int, [_vp, _I64, _D, _D, _D, _D, _dbl, _dbl, _D]),
    "ace_mu_solution": (_int, [_vp, _I64, _D, _D, _D]),
    "ace_pred": (_int, [_vp, _I64, _I64, _D, _dbl, _dbl, _D, _D, _D, _dbl, _dbl, _D, _D, _D]),
    "ace_pred_marginal": (_int, [_vp, _I64, _I64, _int, _D, _D, _dbl, _dbl, _D, _D, _D, _dbl,
                                 _dbl, _dbl, _int, _D, _D, _D, _D]),
    "ace_dmat_upload": (_int, [_vp, _I64, _I64, _I64, _D, _VPP]),
    "ace_dmat_dims": (_int, [_vp, _I64P, _I64P, _I64P]),
    "ace_dmat_read": (_int, [_vp, _I64, _I64, _D]),
    "ace_dmat_materialized": (_int, [_vp]),
    "ace_dmat_free": (None, [_vp]),
    "ace_kernmat_sym_dev": (_int, [_vp, _int, _I64, _int, _int, _D, _D, _D, _VPP, _VPP]),
    "ace_kernmat_cross_dev": (_int, [_vp, _int, _I64, _I64, _int, _int, _D, _D, _D, _D, _D, _VPP,
                                     _VPP]),
    "ace_invkernel_dev": (_int, [_vp, _vp, _dbl, _D, _VPP]),
    "ace_mu_solution_dev": (_int, [_vp, _I64, _D, _vp, _D]),
    "ace_stats_dev": (_int, [_vp, _I64, _D, _vp, _vp, _D, _dbl, _dbl, _D]),
    "ace_grad_dev": (_int, [_vp, _int, _I64, _int, _int, _D, _D, _D, _vp, _vp, _vp, _D, _D, _D,
                            _dbl, _D]),
    "ace_pred_dev": (_int, [_vp, _I64, _I64, _D, _dbl, _dbl, _vp, _vp, _vp, _dbl, _dbl, _D, _D,
                            _D]),
    "ace_pred_marginal_dev": (_int, [_vp, _I64, _I64, _D, _D, _dbl, _dbl, _vp, _vp, _vp, _dbl,
                                     _dbl, _dbl, _int, _D, _D, _D, _D]),
    "ace_nesterov": (_int, [_I64, _dbl, _dbl, _D, _D, _D]),
    "ace_nadam": (_int, [_I64, _dbl, _dbl, _dbl, _dbl, _dbl, _D, _D, _D, _D]),
    "ace_adam": (_int, [_I64, _dbl, _dbl, _dbl, _dbl, _dbl, _D, _D, _D, _D]),
    "ace_norm_clip": (None, [_int, _I64, _D, _dbl]),
    "ace_ncs_basis": (_int, [_I64, _D, _I64, _D, _D, _I64P]),
    "ace_ncs_basis_deriv": (_int, [_I64, _D, _I64, _D, _D, _I64P]),
    "ace_normalize_train": (_int, [_I64, _int, _int, _D, _D, _D, _D]),
    "ace_normalize_test": (_int, [_I64, _int, _int, _D, _D, _D, _I64]),
    "ace_zero_pattern_order": (_int, [_I64, _int, _D, _I64P, _U32, _I32]),
    "ace_model_create": (_int, [_vp, _int, _I64, _int, _int, _VPP]),
    "ace_model_destroy": (None, [_vp]),
    "ace_model_set_data": (_int, [_vp, _D, _D, _D, _dbl]),
    "ace_model_para_update": (_int, [_vp, _int, _D, _D, _D, _D]),
    "ace_model_train_stats": (_int, [_vp, _D, _D]),
    "ace_model_get_inverse": (_int, [_vp, _D]),
    "ace_model_apply_inverse": (_int, [_vp, _I64, _D, _D]),
    "ace_model_predict": (_int, [_vp, _D, _I64, _D, _D, _dbl, _dbl, _D, _D, _D]),
    "ace_model_predict_marginal": (_int, [_vp, _D, _I64, _D, _D, _D, _dbl, _dbl, _int, _D, _D, _D,
                                          _D]),
    "ace_model_predict_marginal_groups": (_int, [_vp, _D, _I64, _D, _D, _dbl, _dbl, _int, _I32,
                                                 _D, _D, _D, _D, _I64P, _D]),
    "ace_robust_levels": (_int, [_I64, _D, _int, _D, _I32]),
    "ace_model_robust_treatment": (_int, [_vp, _D, _I64, _D, _D, _D, _dbl, _dbl, _int, _D, _D, _D,
                                          _D, _I32, _D, _I64P]),
    "ace_model_coef_posterior": (_int, [_vp, _D, _I64, _D, _D, _D]),
    "ace_model_coef_cross": (_int, [_vp, _D, _I64, _D, _D]),
    "ace_coef_contract": (_int, [_I64, _int, _I64, _D, _D, _D, _dbl, _dbl, _dbl, _dbl, _D, _D,
                                 _D]),
    "ace_model_predict_surface": (_int, [_vp, _D, _I64, _D, _I64, _D, _int, _dbl, _dbl, _dbl, _D,
                                         _D, _D]),
    "ace_model_coef_groups": (_int, [_vp, _D, _I64, _D, _int, _I32, _D, _D, _I64P]),
    "ace_coef_group_contract": (_int, [_int, _int, _I64, _D, _D, _I64P, _D, _dbl, _dbl, _dbl, _D,
                                       _D, _D, _D]),
    "ace_model_average_response": (_int, [_vp, _D, _I64, _D, _int, _I32, _I64, _D, _int, _dbl,
                                          _dbl, _dbl, _D, _D, _D, _D]),
    "ace_model_predict_joint": (_int, [_vp, _D, _I64, _D, _D, _int, _dbl, _dbl, _dbl, _int, _dbl,
                                       _I64, _D, _D, _D, _D, _D, _I64P]),
    "ace_potrf_lower": (_int, [_I64, _D, _I64, _dbl, _D, _I64, _I64P]),
    "ace_model_cv": (_int, [_vp, _D, _I64, _I64P, _I64P, _dbl, _dbl, _D, _D, _D, _D, _D, _I32]),
    "ace_cv_from_inverse": (_int, [_vp, _I64, _D, _I64, _D, _I64, _I64P, _I64P, _D, _D, _D, _D,
                                   _I32]),
    "ace_model_profile": (_int, [_vp, _int]),
    "ace_model_kernel_time": (_int, [_vp, _int, _D, _I64P, _D]),
    "ace_model_train": (_int, [_vp, _int, _dbl, _dbl, _dbl, _dbl, _int, _dbl, _int, _dbl, _D, _D,
                               _IP, _IP]),
    "ace_comm_unique_id": (_int, [_str]),
    "ace_model_create_sharded": (_int, [_vp, _int, _I64, _int, _int, _int, _int, _str, _VPP]),
    "ace_model_shard_info": (_int, [_vp, _IP, _IP]),
    "ace_model_comm_calls": (_int, [_vp, _I64P]),
    "ace_model_create_sharded_host": (_int, [_vp, _int, _I64, _int, _int, _int, _int, _vp, _VPP]),
    "ace_batch_create": (_int, [_vp, _int, _I64, _I64, _int, _int, _VPP]),
    "ace_batch_destroy": (None, [_vp]),
    "ace_batch_set_data": (_int, [_vp, _I64, _I64, _D, _D, _D, _dbl]),
    "ace_batch_para_update": (_int, [_vp, _int, _D, _D, _D, _D]),
    "ace_batch_train": (_int, [_vp, _int, _dbl, _dbl, _dbl, _dbl, _int, _dbl, _int, _dbl, _D, _D,
                               _I32, _I32, _I32]),
    "ace_batch_get_inverse": (_int, [_vp, _I64, _D]),
    "ace_predict_batch": (_int, [_vp, _D, _I64P, _D, _D, _D, _D, _D, _D, _D]),
    "ace_predict_marginal_batch": (_int, [_vp, _D, _I64P, _D, _D, _D, _D, _D, _int, _D, _D, _D,
                                          _D]),
    "ace_set_inverse_batch": (_int, [_vp, _I64, _D]),
}

# ace_comm_ops (include/ace_hip.h): host-callback collectives
BCAST_FN = ctypes.CFUNCTYPE(_int, _vp, _D, _I64, _int)
ALLGATHER_FN = ctypes.CFUNCTYPE(_int, _vp, _D, _D, _I64)
ALLREDUCE_FN = ctypes.CFUNCTYPE(_int, _vp, _D, _I64, _int)


class CommOps(ctypes.Structure):
    _fields_ = [("user", _vp), ("broadcast", BCAST_FN),
                ("allgather", ALLGATHER_FN), ("allreduce", ALLREDUCE_FN)]
UNIQUE_ID_BYTES = 128

STATUS = {0: "ACE_OK", 1: "ACE_ERR_ARG", 2: "ACE_ERR_HIP", 3: "ACE_ERR_OOM",
          4: "ACE_ERR_UNSUPPORTED", 5: "ACE_ERR_NONFINITE", 6: "ACE_ERR_INTERRUPTED", 7: "ACE_ERR_TIMEOUT"}
POLL_FN = ctypes.CFUNCTYPE(_int, _vp)
OPTIMIZER = {"GD": 0, "NAG": 0, "Adam": 1, "Nadam": 2}


class AceError(RuntimeError):
    """A non-zero ace_status (the Rcpp shim maps these to Rcpp::stop)."""


_lib = None
_lock = threading.Lock()


def lib():
    """Load libace_hip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise AceError(f"{LIB_PATH} is missing: run __graft_entry__.build() "
                               "(there is no CPU fallback)")
            L = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                # an older library built for an A/B run may lack newer entry
                # points: they stay unbound (calling one raises AttributeError);
                # tests/test_abi_cpu.py checks the in-tree library exports all
                f = getattr(L, name, None)
                if f is None:
                    continue
                f.restype = res
                f.argtypes = args
            _lib = L
    return _lib


def ptr(a):
    """double* of a contiguous float64 numpy array of any rank (or None)."""
    if a is None:
        return None
    assert a.dtype == np.float64 and (a.flags.f_contiguous or a.flags.c_contiguous)
    return a.ctypes.data_as(_D)


def check(status, ctx=None):
    if status != 0:
        msg = lib().ace_last_error(ctx)
        raise AceError(f"{STATUS.get(status, status)}: {msg.decode() if msg else ''}")


class Handle:
    """An owned library handle in `self.handle`, destroyed once by the entry
    point named `_destroy` (close(), or when the object is collected)."""

    _destroy = None

    def close(self):
        if getattr(self, "handle", None):
            getattr(lib(), self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(Handle):
    """One ace_ctx (one HIP device, one stream) -- one process per GPU."""

    _destroy = "ace_destroy"

    def __init__(self, device=None):
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = device
        h = _vp()
        check(lib().ace_create(device, ctypes.byref(h)), None)
        self.handle = h

    def set_interrupt_poll(self, fn):
        """fn() -> bool, polled between training iterations (ace_set_interrupt_poll);
        None removes it."""
        self._poll = None if fn is None else POLL_FN(lambda _u: 1 if fn() else 0)
        ptr_ = ctypes.cast(self._poll, _vp) if self._poll is not None else None
        check(lib().ace_set_interrupt_poll(self.handle, ptr_, None), self.handle)


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def fmat(a, shape=None):
    """Column-major float64 copy/view (R/Armadillo layout)."""
    a = np.asarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape, order="F") if a.ndim != len(shape) else a
    return np.asfortranarray(a)
