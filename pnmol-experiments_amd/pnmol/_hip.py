"""ctypes binding of `libpnmol_hip.so` (C ABI declared in include/pnmol_hip.h).

There is no CPU fallback: if the library or a GPU is missing, the solver classes raise.
"""

import ctypes
import os
import pathlib

import numpy as np


_c_double_p = ctypes.POINTER(ctypes.c_double)
_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = pathlib.Path(os.environ.get("PNMOL_HIP_LIB", _HERE.parent / "lib" / "libpnmol_hip.so"))


class PnmolHipError(RuntimeError):
    """A call into libpnmol_hip.so failed."""


class StepOut(ctypes.Structure):
    _fields_ = [
        ("t_new", ctypes.c_double),
        ("diffusion_squared_local", ctypes.c_double),
        ("sigma2_whitened", ctypes.c_double),
        ("error_sigma2", ctypes.c_double),
        ("info", ctypes.c_int),
    ]


class ObserveOut(ctypes.Structure):
    """`pnmol_observe_out`: log N(y; H m, S), |Ls^-1 (y - H m)|^2, log det S, info (-1 ok, else the failing pivot)."""

    _fields_ = [
        ("log_likelihood", ctypes.c_double),
        ("mahalanobis", ctypes.c_double),
        ("logdet", ctypes.c_double),
        ("info", ctypes.c_int),
    ]


class FilterDesc(ctypes.Structure):
    _fields_ = [
        ("d", ctypes.c_int),
        ("num_derivatives", ctypes.c_int),
        ("nB", ctypes.c_int),
        ("L", _c_double_p),
        ("B", _c_double_p),
        ("E_sqrtm", _c_double_p),
        ("R_sqrtm", _c_double_p),
        ("Gamma", _c_double_p),
        ("d_state", ctypes.c_int),
        ("dtype", ctypes.c_int),      # 0 fp64, 1 fp32 covariance (include/pnmol_hip.h)
        ("K", _c_double_p),           # optional Gram matrix Gamma Gamma^T (saves the library an O(d^3) host loop)
    ]


# name -> (restype, argtypes); every symbol include/pnmol_hip.h declares
_vp = ctypes.c_void_p
SYMBOLS = {
    "pnmol_abi_version": (ctypes.c_int, []),
    "pnmol_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "pnmol_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "pnmol_ctx_destroy": (ctypes.c_int, [_vp]),
    "pnmol_ctx_synchronize": (ctypes.c_int, [_vp]),
    "pnmol_fd_solve_batched": (ctypes.c_int, [_vp, _c_double_p, _c_double_p, _c_double_p, ctypes.c_int, ctypes.c_int,
                                              _c_double_p, _c_double_p]),
    "pnmol_cholesky_lower": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int, _c_double_p]),
    "pnmol_last_error": (ctypes.c_char_p, [_vp]),
    "pnmol_filter_create": (ctypes.c_int, [_vp, ctypes.POINTER(FilterDesc), ctypes.POINTER(_vp)]),
    "pnmol_filter_destroy": (ctypes.c_int, [_vp]),
    "pnmol_filter_set_error_model": (ctypes.c_int, [_vp, ctypes.c_double, _c_double_p, _c_double_p]),
    "pnmol_filter_predict_mean": (ctypes.c_int, [_vp, _vp, ctypes.c_double, _c_double_p]),
    "pnmol_filter_set_operator": (ctypes.c_int, [_vp, _c_double_p, _c_double_p]),
    "pnmol_filter_set_operator_diagonal": (ctypes.c_int, [_vp, _c_double_p, _c_double_p]),
    "pnmol_filter_set_reaction": (ctypes.c_int, [_vp, _vp]),           # (pnmol_reaction*: pde/reactions.py, ReactionDesc)
    "pnmol_filter_set_reaction_system": (ctypes.c_int, [_vp, _vp]),    # (pnmol_reaction_system*: SystemReactionDesc)
    "pnmol_filter_set_convection": (ctypes.c_int, [_vp, _vp, _c_double_p]),   # (pnmol_convection*: ConvectionDesc; G (d, d))
    "pnmol_filter_linearize": (ctypes.c_int, [_vp, _vp, ctypes.c_double]),
    "pnmol_filter_set_linearization_points": (ctypes.c_int, [_vp, ctypes.c_int, _c_double_p]),
    "pnmol_filter_linearization_pending": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "pnmol_filter_linearize_at": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_filter_set_forcing": (ctypes.c_int, [_vp, ctypes.c_int, _c_double_p]),
    "pnmol_filter_forcing_pending": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "pnmol_filter_force_at": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_filter_set_operator_family": (ctypes.c_int, [_vp, ctypes.c_int, _c_double_p, _c_double_p]),
    "pnmol_filter_set_operator_schedule": (ctypes.c_int, [_vp, ctypes.c_int, _c_double_p]),
    "pnmol_filter_operator_schedule_pending": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "pnmol_filter_operator_at": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_state_create": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "pnmol_state_destroy": (ctypes.c_int, [_vp]),
    "pnmol_state_clone": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "pnmol_state_set": (ctypes.c_int, [_vp, ctypes.c_double, _c_double_p, _c_double_p]),
    "pnmol_state_set_sqrtm": (ctypes.c_int, [_vp, ctypes.c_double, _c_double_p, _c_double_p]),
    "pnmol_state_get_time": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_state_get_mean": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_state_get_cov_sqrtm": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_state_get_cov": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_state_get_marginal_var": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_filter_step": (ctypes.c_int, [_vp, _vp, ctypes.c_double, _vp, ctypes.POINTER(StepOut), _c_double_p]),
    "pnmol_smoother_step": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _vp]),
    "pnmol_state_predict": (ctypes.c_int, [_vp, _vp, ctypes.c_double, _vp]),
    "pnmol_state_observe": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _c_double_p, _c_double_p, _c_double_p, _vp,
                                           ctypes.POINTER(ObserveOut)]),
    "pnmol_filter_set_observations": (ctypes.c_int, [_vp, ctypes.c_int, _c_double_p, ctypes.c_int, _c_double_p, _c_double_p,
                                                     _c_double_p]),
    "pnmol_filter_observations_pending": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "pnmol_filter_observation_results": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ObserveOut)]),
    "pnmol_state_observe_planned": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.POINTER(ObserveOut)]),
    "pnmol_state_predict_marginals": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _c_double_p, _c_double_p, _c_double_p]),
    "pnmol_smoother_step_bridge": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _vp, ctypes.c_int, ctypes.POINTER(_vp)]),
    "pnmol_bridge_destroy": (ctypes.c_int, [_vp]),
    "pnmol_bridge_get_interval": (ctypes.c_int, [_vp, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int)]),
    "pnmol_bridge_eval": (ctypes.c_int, [_vp, ctypes.c_int, _c_double_p, _c_double_p, _c_double_p]),
    "pnmol_bridge_state": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _vp]),
    "pnmol_samples_create": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(_vp)]),
    "pnmol_samples_destroy": (ctypes.c_int, [_vp]),
    "pnmol_samples_draw": (ctypes.c_int, [_vp, _vp, _c_double_p, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_double]),
    "pnmol_samples_step_back": (ctypes.c_int, [_vp, _vp, ctypes.c_double, _c_double_p, ctypes.c_ulonglong, ctypes.c_ulonglong,
                                               ctypes.c_double]),
    "pnmol_samples_interpolate": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_double, _c_double_p, ctypes.c_ulonglong,
                                                 ctypes.c_ulonglong, ctypes.c_double]),
    "pnmol_samples_clone": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "pnmol_samples_get": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_samples_get_time": (ctypes.c_int, [_vp, _c_double_p]),
    "pnmol_sample_noise": (ctypes.c_int, [_vp, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int,
                                          _c_double_p]),
    "pnmol_filter_steps": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_double, _c_double_p, _c_double_p,
                                          ctypes.POINTER(StepOut)]),
    "pnmol_filter_steps_begin": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_double]),
    "pnmol_filter_steps_end": (ctypes.c_int, [_vp, _vp, _c_double_p, _c_double_p, ctypes.POINTER(StepOut)]),
    "pnmol_filter_set_recorder": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(_vp)]),
    "pnmol_filter_recorder_pending": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "pnmol_filter_recorder_means": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "pnmol_smoother_steps": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(_vp), _c_double_p, ctypes.POINTER(_vp),
                                            _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int)]),
    "pnmol_functionals": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(_vp), _c_double_p, ctypes.c_int, _c_double_p,
                                         _c_double_p, _c_double_p]),
    "pnmol_filter_prepare_steps": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_double]),
    "pnmol_filter_last_steps_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    "pnmol_filter_prepare_error_model": (ctypes.c_int, [_vp, ctypes.c_double]),
    "pnmol_filter_debug_read": (ctypes.c_int, [_vp, ctypes.c_int, _c_double_p, ctypes.c_long]),
    "pnmol_filter_debug_poison": (ctypes.c_int, [_vp]),
    "pnmol_filter_dims": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_int)] * 5),
    "pnmol_filter_sweep_layout": (ctypes.c_int, [_vp] + [ctypes.POINTER(ctypes.c_int)] * 2),
    # include/pnmol_sqrt.h
    "pnmol_qr_r": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int, ctypes.c_int, _c_double_p]),
    "pnmol_qr_last_ms": (ctypes.c_int, [ctypes.POINTER(ctypes.c_float)]),
    "pnmol_sqrt_propagate_cholesky_factor": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int, ctypes.c_int, _c_double_p,
                                                             ctypes.c_int, _c_double_p]),
    "pnmol_sqrt_update": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int, ctypes.c_int, _c_double_p, _c_double_p,
                                         _c_double_p, _c_double_p, _c_double_p]),
    "pnmol_sqrt_filter_create": (ctypes.c_int, [_vp, ctypes.POINTER(FilterDesc), ctypes.POINTER(_vp)]),
    "pnmol_sqrt_filter_destroy": (ctypes.c_int, [_vp]),
    "pnmol_sqrt_filter_set_state": (ctypes.c_int, [_vp, ctypes.c_double, _c_double_p, _c_double_p]),
    "pnmol_sqrt_filter_get_state": (ctypes.c_int, [_vp, _c_double_p, _c_double_p, _c_double_p]),
    "pnmol_sqrt_filter_predict_mean": (ctypes.c_int, [_vp, ctypes.c_double, _c_double_p]),
    "pnmol_sqrt_filter_set_operator": (ctypes.c_int, [_vp, _c_double_p, _c_double_p]),
    "pnmol_sqrt_filter_prepare_error_model": (ctypes.c_int, [_vp, ctypes.c_double]),
    "pnmol_sqrt_filter_step": (ctypes.c_int, [_vp, ctypes.c_double, ctypes.POINTER(StepOut), _c_double_p]),
    "pnmol_sqrt_filter_steps": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, _c_double_p, _c_double_p,
                                               ctypes.POINTER(StepOut)]),
    "pnmol_sqrt_filter_last_steps_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    "pnmol_sqrt_update_no_meascov": (ctypes.c_int, [_vp, _c_double_p, ctypes.c_int, ctypes.c_int, _c_double_p,
                                                    _c_double_p, _c_double_p, _c_double_p]),
}

_lib = None


def load_library():
    """Load the shared library (no GPU needed for this) and declare all prototypes."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise PnmolHipError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
                "pnmol has no CPU fallback for the filter step."
            )
        lib = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _dp(a):
    return a.ctypes.data_as(_c_double_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


class Context:
    """One HIP device + stream (`pnmol_ctx`)."""

    _cache = {}

    def __init__(self, device=0):
        self.lib = load_library()
        n = ctypes.c_int(0)
        rc = self.lib.pnmol_device_count(ctypes.byref(n))
        if rc != 0 or n.value < 1:
            raise PnmolHipError("no HIP device visible: the PNMOL filter step needs an AMD GPU (MI355X / gfx950)")
        h = _vp()
        rc = self.lib.pnmol_ctx_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise PnmolHipError(f"pnmol_ctx_create(device={device}) failed with {rc}")
        self.handle, self.device = h, int(device)

    @classmethod
    def default(cls, device=None):
        if device is None:
            device = int(os.environ.get("PNMOL_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            n = ctypes.c_int(0)
            load_library().pnmol_device_count(ctypes.byref(n))
            if n.value > 0:
                device %= n.value
        if device not in cls._cache:
            cls._cache[device] = cls(device)
        return cls._cache[device]

    def cholesky(self, A):
        """Lower Cholesky factor of a symmetric positive definite matrix on the device (`pnmol_cholesky_lower`):
        `jnp.linalg.cholesky(spatial_kernel(X, X.T))`, white.py:84-85."""
        A = _f64(A)
        n = A.shape[0]
        if A.shape != (n, n):
            raise ValueError(f"expected a square matrix, got {A.shape}")
        L = np.empty((n, n))
        self.check(self.lib.pnmol_cholesky_lower(self.handle, _dp(A), n, _dp(L)), "pnmol_cholesky_lower")
        return L

    def fd_solve_batched(self, gram, lk, llk):
        """weights (N, s), uncertainty (N,) of N kernel-FD stencils (`pnmol_fd_solve_batched`; discretize.py:177-201)."""
        gram, lk, llk = _f64(gram), _f64(lk), _f64(llk)
        N, s = lk.shape
        if gram.shape != (N, s, s) or llk.shape != (N,):
            raise ValueError(f"shapes {gram.shape}, {lk.shape}, {llk.shape} do not describe N stencils of size s")
        w, u = np.empty((N, s)), np.empty(N)
        self.check(self.lib.pnmol_fd_solve_batched(self.handle, _dp(gram), _dp(lk), _dp(llk), N, s, _dp(w), _dp(u)),
                   "pnmol_fd_solve_batched")
        return w, u

    def qr_r(self, A):
        """R factor (upper, diag >= 0) of A on the device: `jnp.linalg.qr(A, mode="r")` (base/sqrt.py:21)."""
        A = _f64(A)
        rows, cols = A.shape
        R = np.empty((cols, cols))
        self.check(self.lib.pnmol_qr_r(self.handle, _dp(A), rows, cols, _dp(R)), "pnmol_qr_r")
        return R

    def sqrt_propagate(self, S1, S2=None):
        S1 = _f64(S1)
        n, k1 = S1.shape
        out = np.empty((n, n))
        if S2 is None:
            rc = self.lib.pnmol_sqrt_propagate_cholesky_factor(self.handle, _dp(S1), n, k1, None, 0, _dp(out))
        else:
            S2 = _f64(S2)
            if S2.shape[0] != n:
                raise ValueError(f"S1 {S1.shape} and S2 {S2.shape} must have the same number of rows")
            rc = self.lib.pnmol_sqrt_propagate_cholesky_factor(self.handle, _dp(S1), n, k1, _dp(S2), S2.shape[1], _dp(out))
        self.check(rc, "pnmol_sqrt_propagate_cholesky_factor")
        return out

    def sqrt_update(self, H, C, meascov_sqrtm=None):
        H, C = _f64(H), _f64(C)
        m, D = H.shape
        if C.shape != (D, D):
            raise ValueError(f"cov_cholesky must be {(D, D)}, got {C.shape}")
        if m > D:
            raise ValueError("update_sqrt needs output_dim <= input_dim (base/sqrt.py:56-58)")
        C_new, gain, Sl = np.empty((D, D)), np.empty((D, m)), np.empty((m, m))
        if meascov_sqrtm is None:
            rc = self.lib.pnmol_sqrt_update_no_meascov(self.handle, _dp(H), m, D, _dp(C), _dp(C_new), _dp(gain), _dp(Sl))
        else:
            E = _f64(meascov_sqrtm, (m, m))
            rc = self.lib.pnmol_sqrt_update(self.handle, _dp(H), m, D, _dp(C), _dp(E), _dp(C_new), _dp(gain), _dp(Sl))
        self.check(rc, "pnmol_sqrt_update")
        return C_new, gain, Sl

    def qr_last_ms(self):
        ms = ctypes.c_float(0)
        self.lib.pnmol_qr_last_ms(ctypes.byref(ms))
        return ms.value

    def sample_noise(self, seed, step_index, rows, cols):
        """(rows, cols) standard normals of the device generator (`pnmol_sample_noise`): what a draw of `rows` samples with
        `xi = NULL` uses for (seed, step_index)."""
        out = np.empty((int(rows), int(cols)))
        self.check(self.lib.pnmol_sample_noise(self.handle, int(seed), int(step_index), int(rows), int(cols), _dp(out)),
                   "pnmol_sample_noise")
        return out

    def check(self, rc, what):
        if rc != 0:
            msg = self.lib.pnmol_last_error(self.handle)
            raise PnmolHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def synchronize(self):
        self.check(self.lib.pnmol_ctx_synchronize(self.handle), "pnmol_ctx_synchronize")


class Filter:
    """`pnmol_filter`: the measurement/prior model of one discretised PDE on the device."""

    DTYPES = {"f64": 0, "f32": 1}

    def __init__(self, ctx, *, L, B, E_sqrtm, R_sqrtm, Gamma, num_derivatives, dtype="f64", K=None):
        """dtype "f32": the covariance and its bulk kernels (predict, H-apply, down-date) in fp32; the factorisation of
        the innovation matrix, the mean and all scalars stay fp64 (`pnmol_filter_desc.dtype`)."""
        self.ctx, self.lib = ctx, ctx.lib
        d, ds = L.shape          # ds = d (white-noise model) or 2d (latent-force model, state [u; eps])
        nB = B.shape[0]
        self._keep = [_f64(L, (d, ds)), _f64(B, (nB, ds)), _f64(E_sqrtm, (d, d)), _f64(R_sqrtm, (nB, nB)),
                      _f64(Gamma, (ds, ds))]
        gram = _f64(self._keep[4] @ self._keep[4].T if K is None else K, (ds, ds))   # (BLAS here; a scalar loop in the library)
        desc = FilterDesc(d, int(num_derivatives), nB, *[_dp(a) for a in self._keep], ds, self.DTYPES[dtype], _dp(gram))
        self.dtype = dtype
        self.ds = ds
        h = _vp()
        ctx.check(self.lib.pnmol_filter_create(ctx.handle, ctypes.byref(desc), ctypes.byref(h)), "pnmol_filter_create")
        self.handle = h
        self.d, self.n, self.nB, self.m = d, int(num_derivatives) + 1, nB, d + nB
        self.error_model_dt = None
        self.reaction = None        # the pde.reactions.Reaction the device evaluates (`set_reaction`)
        self.operator_family = 0    # number of operators of the family set (`set_operator_family`), 0: none
        self._operator_schedule = False
        # raw handles of the live pnmol_state objects of this filter, keyed by id(State): the C ABI refuses to destroy a
        # filter that still has states (include/pnmol_hip.h, "Lifetimes").  A plain dict, not weak references: the
        # cyclic collector clears weakrefs to unreachable objects BEFORE it runs finalisers, so a WeakSet would be empty
        # exactly when a filter and its states die together -- and the states' device buffers would leak.
        self._live = {}
        self._live_samples = {}     # the same for the pnmol_samples objects (Samples)
        self._live_bridges = {}     # ... and the pnmol_bridge objects (Bridge)
        self._recorder = None       # the States a set recorder fills (`set_recorder`), kept alive while it is set

    def __del__(self):
        if getattr(self, "_recorder", None) is not None and getattr(self, "handle", None):
            self.lib.pnmol_filter_set_recorder(self.handle, 0, None)   # (the library refuses to destroy a recorder's slot)
            self._recorder = None
        # The cyclic garbage collector (and interpreter shutdown) finalises a filter and its states in ANY order: the
        # states' handles go first here; a State finalised later finds its entry gone and does nothing (State._destroy).
        live = getattr(self, "_live", None)
        while live:
            _, sh = live.popitem()
            self.lib.pnmol_state_destroy(sh)
        live = getattr(self, "_live_samples", None)
        while live:
            _, sh = live.popitem()
            self.lib.pnmol_samples_destroy(sh)
        live = getattr(self, "_live_bridges", None)
        while live:
            _, sh = live.popitem()
            self.lib.pnmol_bridge_destroy(sh)
        h, self.handle = getattr(self, "handle", None), None
        if h:
            self.lib.pnmol_filter_destroy(h)

    def sweep_layout(self):
        """(kernel, xcd_home) of this filter's sweep launch: `pnmol_filter_sweep_layout`."""
        k, x = ctypes.c_int(0), ctypes.c_int(0)
        self.lib.pnmol_filter_sweep_layout(self.handle, ctypes.byref(k), ctypes.byref(x))
        return {"kernel": {1: "k_sweep", 2: "k_sweep_rl"}[k.value], "xcd_home": x.value}

    def dims(self):
        v = [ctypes.c_int(0) for _ in range(5)]
        self.lib.pnmol_filter_dims(self.handle, *[ctypes.byref(x) for x in v])
        return dict(zip(("d", "n", "m", "dp", "mp"), (x.value for x in v)))

    def prepare_error_model(self, dt):
        """Step-invariant part of `estimate_error` for step size dt, computed on the device from the current operator."""
        self.ctx.check(self.lib.pnmol_filter_prepare_error_model(self.handle, float(dt)), "pnmol_filter_prepare_error_model")
        self.error_model_dt = float(dt)

    def set_error_model(self, dt, Sq_inv, Sq_diag):
        a, b = _f64(Sq_inv, (self.m, self.m)), _f64(Sq_diag, (self.m,))
        self.ctx.check(self.lib.pnmol_filter_set_error_model(self.handle, float(dt), _dp(a), _dp(b)),
                       "pnmol_filter_set_error_model")
        self.error_model_dt = float(dt)

    def new_state(self):
        return State(self)

    def new_samples(self, num_samples):
        """A device-resident block of `num_samples` joint draws (`pnmol_samples_create`)."""
        return Samples(self, num_samples)

    def predict_mean(self, state_in, dt):
        out = np.empty(self.d)
        self.ctx.check(self.lib.pnmol_filter_predict_mean(self.handle, state_in.handle, float(dt), _dp(out)),
                       "pnmol_filter_predict_mean")
        return out

    def set_operator(self, M, shift=None):
        a = _f64(M, (self.d, self.ds))
        b = _f64(shift, (self.d,)) if shift is not None else None
        self.ctx.check(self.lib.pnmol_filter_set_operator(self.handle, _dp(a), _dp(b) if b is not None else None),
                       "pnmol_filter_set_operator")
        self.error_model_dt = None

    def set_operator_diagonal(self, jdiag, shift=None):
        """M = L + diag(jdiag) (pointwise nonlinearity): `pnmol_filter_set_operator_diagonal`."""
        a = _f64(jdiag, (self.d,))
        b = _f64(shift, (self.d,)) if shift is not None else None
        self.ctx.check(self.lib.pnmol_filter_set_operator_diagonal(self.handle, _dp(a), _dp(b) if b is not None else None),
                       "pnmol_filter_set_operator_diagonal")
        self.error_model_dt = None

    def set_reaction(self, reaction):
        """A pointwise reaction term (pde/reactions.py) that the device linearises itself -- a scalar `Reaction`
        (`pnmol_filter_set_reaction`), a coupled `SystemReaction` (`pnmol_filter_set_reaction_system`) or a `Convection` term
        with its operator G (`pnmol_filter_set_convection`) --, or None to clear any of them.  A filter holds one; while one is
        set, `steps` re-linearises in front of every step."""
        from .pde.reactions import Convection, SystemReaction

        desc = None if reaction is None else reaction.to_ctypes()
        if isinstance(reaction, Convection):
            if reaction.G is None:
                raise ValueError("the convection term has no operator G (Convection.set_operator; the problem recipes set it)")
            name = "pnmol_filter_set_convection"
            G = _f64(reaction.G, (self.d, self.d))
            rc = self.lib.pnmol_filter_set_convection(self.handle, ctypes.byref(desc), _dp(G))
        else:
            name = "pnmol_filter_set_reaction_system" if isinstance(reaction, SystemReaction) else "pnmol_filter_set_reaction"
            rc = getattr(self.lib, name)(self.handle, None if desc is None else ctypes.byref(desc))
        self.ctx.check(rc, name)
        self.reaction = reaction
        self.error_model_dt = None

    def linearize(self, state_in, dt):
        """Enqueue the EK1 linearisation of the reaction at the predicted mean of a step from `state_in` over dt
        (`pnmol_filter_linearize`; no synchronisation).  Then `prepare_error_model(dt)`, then `step(state_in, dt)`."""
        self.ctx.check(self.lib.pnmol_filter_linearize(self.handle, state_in.handle, float(dt)), "pnmol_filter_linearize")
        self.error_model_dt = None

    def _pending(self, name):
        """(next, count) of the loop option whose query is the library's `name`: its cursor and its length ((0, 0): none set)."""
        nxt, n = ctypes.c_int(0), ctypes.c_int(0)
        self.ctx.check(getattr(self.lib, name)(self.handle, ctypes.byref(nxt), ctypes.byref(n)), name)
        return nxt.value, n.value

    def _clear(self, name, *nulls):
        """The set call `name` of the library with the arguments that clear what it sets."""
        self.ctx.check(getattr(self.lib, name)(self.handle, *nulls), name)

    def set_linearization_points(self, points):
        """Linearisation points for the constant-step loop (`pnmol_filter_set_linearization_points`): `points` (count, d),
        derivative 0 in raw coordinates; the i-th step `steps` takes from now on linearises the term at row i in place of its own
        predicted mean.  The cursor starts at row 0."""
        u = _f64(points)
        if u.ndim != 2 or u.shape[0] < 1 or u.shape[1] != self.d:
            raise ValueError(f"points must be (count, {self.d}) with count >= 1, got {u.shape} "
                             "(clear_linearization_points() drops the table)")
        self.ctx.check(self.lib.pnmol_filter_set_linearization_points(self.handle, u.shape[0], _dp(u)),
                       "pnmol_filter_set_linearization_points")

    def clear_linearization_points(self):
        """Drop the table: the filter then takes the launches and gives the bits of one that never had a table."""
        self._clear("pnmol_filter_set_linearization_points", 0, None)

    def linearization_pending(self):
        """(next, count): the table's cursor -- the row the next step is linearised at -- and its number of rows ((0, 0): none)."""
        return self._pending("pnmol_filter_linearization_pending")

    def linearize_at(self, u):
        """Enqueue the EK1 linearisation of the term at the point `u` (d,) (`pnmol_filter_linearize_at`; no synchronisation).  Then
        `prepare_error_model(dt)` if the error estimate is wanted, then `step(state_in, dt)`."""
        u = _f64(u, (self.d,))
        self.ctx.check(self.lib.pnmol_filter_linearize_at(self.handle, _dp(u)), "pnmol_filter_linearize_at")
        self.error_model_dt = None

    def set_forcing(self, rhs):
        """Right-hand sides for the constant-step loop (`pnmol_filter_set_forcing`): `rhs` (count, m), a row [source (d); boundary
        values (nB)]; the k-th step `steps` takes from now on measures against row k.  The cursor starts at row 0."""
        r = _f64(rhs)
        if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] != self.m:
            raise ValueError(f"rhs must be (count, {self.m}) with count >= 1, got {r.shape} (clear_forcing() drops the table)")
        self.ctx.check(self.lib.pnmol_filter_set_forcing(self.handle, r.shape[0], _dp(r)), "pnmol_filter_set_forcing")

    def clear_forcing(self):
        """Drop the table: the filter then takes the launches and gives the bits of one that never had a table."""
        self._clear("pnmol_filter_set_forcing", 0, None)

    def forcing_pending(self):
        """(next, count): the table's cursor -- the row the next step measures against -- and its number of rows ((0, 0): none)."""
        return self._pending("pnmol_filter_forcing_pending")

    def force_at(self, rhs):
        """The right-hand side `rhs` (m,) every `step` measures against from now on (`pnmol_filter_force_at`; no
        synchronisation); None returns the filter to unforced."""
        r = None if rhs is None else _f64(rhs, (self.m,))
        self.ctx.check(self.lib.pnmol_filter_force_at(self.handle, None if r is None else _dp(r)), "pnmol_filter_force_at")

    def set_operator_family(self, operators, noise_diagonals):
        """A time-dependent operator M(t) = sum_r a_r(t) L_r (`pnmol_filter_set_operator_family`): `operators` (R, d, d) and the
        diagonals (R, d) of their FD uncertainties, R <= 4.  Until `operator_at` or a loop step with a schedule the filter
        measures with the operator given at creation."""
        L = _f64(operators)
        e = _f64(noise_diagonals)
        if L.ndim != 3 or L.shape[0] < 1 or L.shape[1:] != (self.d, self.d) or e.shape != (L.shape[0], self.d):
            raise ValueError(f"operators must be (R, {self.d}, {self.d}) and noise_diagonals (R, {self.d}) with R >= 1, got "
                             f"{L.shape} and {e.shape} (clear_operator_family() drops the family)")
        self.ctx.check(self.lib.pnmol_filter_set_operator_family(self.handle, L.shape[0], _dp(L), _dp(e)),
                       "pnmol_filter_set_operator_family")
        self.operator_family = L.shape[0]
        self._operator_schedule = False
        self.error_model_dt = None

    def clear_operator_family(self):
        """Drop the family and its schedule: the filter then gives the bits of one that never had a family."""
        self._clear("pnmol_filter_set_operator_family", 0, None, None)
        self.operator_family = 0
        self._operator_schedule = False
        self.error_model_dt = None

    def set_operator_schedule(self, coefficients):
        """Coefficients for the constant-step loop (`pnmol_filter_set_operator_schedule`): (count, R); the k-th step `steps` takes
        from now on runs with M = sum_r coefficients[k, r] L_r and its noise.  The cursor starts at row 0."""
        a = _f64(coefficients)
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != max(self.operator_family, 1):
            raise ValueError(f"coefficients must be (count, {max(self.operator_family, 1)}) with count >= 1, got {a.shape} "
                             "(clear_operator_schedule() drops the table)")
        self.ctx.check(self.lib.pnmol_filter_set_operator_schedule(self.handle, a.shape[0], _dp(a)),
                       "pnmol_filter_set_operator_schedule")
        self._operator_schedule = True

    def clear_operator_schedule(self):
        """Drop the table: the operator stays what the last step made it."""
        self._clear("pnmol_filter_set_operator_schedule", 0, None)
        self._operator_schedule = False

    def operator_schedule_pending(self):
        """(next, count): the table's cursor -- the row the next step runs with -- and its number of rows ((0, 0): none)."""
        return self._pending("pnmol_filter_operator_schedule_pending")

    def operator_at(self, coefficients):
        """The operator and its noise from the R coefficients (`pnmol_filter_operator_at`; enqueued at once, no synchronisation),
        until another call or a loop step with a schedule replaces them.  Then `linearize` (with a reaction), then
        `prepare_error_model(dt)` if the error estimate is wanted, then `step`."""
        a = _f64(coefficients, (max(self.operator_family, 1),))
        self.ctx.check(self.lib.pnmol_filter_operator_at(self.handle, _dp(a)), "pnmol_filter_operator_at")
        self.error_model_dt = None

    def step(self, state_in, dt, want_error=True):
        out = State(self)
        info = StepOut()
        err = np.empty(self.d) if want_error else None
        rc = self.lib.pnmol_filter_step(self.handle, state_in.handle, float(dt), out.handle, ctypes.byref(info),
                                        _dp(err) if want_error else None)
        self.ctx.check(rc, "pnmol_filter_step")
        return out, info, err

    def smoother_step(self, filt_k, smooth_next, dt, bridge=None):
        """One RTS backward step on the device (`pnmol_smoother_step`): a new State, the smoothed state at filt_k.t.
        bridge="marginal" / "full": `pnmol_smoother_step_bridge` instead, returning (State, Bridge): the same state bit for
        bit and what dense output inside [filt_k.t, filt_k.t + dt] needs ("full": with the cross-covariance C_k, Dp^2 doubles)."""
        out = State(self)
        if bridge is None:
            rc = self.lib.pnmol_smoother_step(self.handle, filt_k.handle, smooth_next.handle, float(dt), out.handle)
            self.ctx.check(rc, "pnmol_smoother_step")
            return out
        if bridge not in ("marginal", "full"):
            raise ValueError(f'bridge must be None, "marginal" or "full", got {bridge!r}')
        h = _vp()
        rc = self.lib.pnmol_smoother_step_bridge(self.handle, filt_k.handle, smooth_next.handle, float(dt), out.handle,
                                                 int(bridge == "full"), ctypes.byref(h))
        self.ctx.check(rc, "pnmol_smoother_step_bridge")
        t = ctypes.c_double(0.0)
        self.lib.pnmol_state_get_time(out.handle, ctypes.byref(t))
        return out, Bridge(self, h, (t.value, float(dt), bridge == "full"))

    def observe(self, state, C, y, R_sqrtm=None):
        """Condition `state` on y = C E0 x + e, e ~ N(0, R_sqrtm R_sqrtm^T) (`pnmol_state_observe`): (new State at the same
        time and in the same frame, ObserveOut).  C (q, d_state), y (q,), R_sqrtm (q, q) lower triangular or None (noise-free)."""
        C = _f64(C)
        if C.ndim != 2 or C.shape[1] != self.ds or not 1 <= C.shape[0] <= self.ds:
            raise ValueError(f"C must be (q, {self.ds}) with 1 <= q <= {self.ds}, got {C.shape}")
        q = C.shape[0]
        y = _f64(y, (q,))
        R = None if R_sqrtm is None else _f64(R_sqrtm, (q, q))
        out, res = State(self), ObserveOut()
        rc = self.lib.pnmol_state_observe(self.handle, state.handle, q, _dp(C), _dp(y), None if R is None else _dp(R),
                                          out.handle, ctypes.byref(res))
        self.ctx.check(rc, "pnmol_state_observe")
        return out, res

    def set_observations(self, times, C, ys, R_sqrtm=None):
        """The sensor plan of the constant-step loop (`pnmol_filter_set_observations`): a fixed sensor array C (q, d_state),
        R_sqrtm (q, q) lower triangular or None (noise-free), reporting ys[i] (nobs, q) at times[i].  `steps` then conditions the
        state behind the step that lands on each time, on the device; the cursor starts at entry 0."""
        t = _f64(np.atleast_1d(times))
        C = _f64(C)
        if t.ndim != 1 or t.size < 1:
            raise ValueError(f"times must be a non-empty 1-d array, got shape {t.shape}")
        if C.ndim != 2 or C.shape[1] != self.ds or not 1 <= C.shape[0] <= self.ds:
            raise ValueError(f"C must be (q, {self.ds}) with 1 <= q <= {self.ds}, got {C.shape}")
        q = C.shape[0]
        ys = _f64(ys, (t.size, q))
        R = None if R_sqrtm is None else _f64(R_sqrtm, (q, q))
        rc = self.lib.pnmol_filter_set_observations(self.handle, t.size, _dp(t), q, _dp(C), None if R is None else _dp(R), _dp(ys))
        self.ctx.check(rc, "pnmol_filter_set_observations")

    def clear_observations(self):
        """Drop the sensor plan: the filter then takes the launches and gives the bits of one that never had a plan."""
        self._clear("pnmol_filter_set_observations", 0, None, 0, None, None, None)

    def observations_pending(self):
        """(next, nobs): the plan's cursor -- the first entry that has not been applied -- and its length ((0, 0): no plan)."""
        return self._pending("pnmol_filter_observations_pending")

    def observation_results(self, first=0, count=None):
        """ObserveOut of the applied plan entries [first, first + count) (default: up to the cursor)."""
        if count is None:
            count = self.observations_pending()[0] - first
        res = (ObserveOut * max(count, 1))()
        self.ctx.check(self.lib.pnmol_filter_observation_results(self.handle, int(first), int(count), res),
                       "pnmol_filter_observation_results")
        return list(res)[:count]

    def observe_planned(self, state, index):
        """Entry `index` of the plan applied to `state` IN PLACE, by the path the loop takes (`pnmol_state_observe_planned`):
        ObserveOut."""
        res = ObserveOut()
        rc = self.lib.pnmol_state_observe_planned(self.handle, state.handle, int(index), ctypes.byref(res))
        self.ctx.check(rc, "pnmol_state_observe_planned")
        return res

    def set_recorder(self, states):
        """The recorder of the constant-step loop (`pnmol_filter_set_recorder`): `states[i]` (States of this filter) receives the
        state behind the i-th step `steps` takes from now on, on the device; the cursor starts at slot 0.  The filter keeps the
        states alive until `clear_recorder()` (the library refuses to destroy a slot)."""
        states = list(states)
        if not states:
            raise ValueError("set_recorder needs at least one state (clear_recorder() drops the recorder)")
        slots = (_vp * len(states))(*[None if s is None else s.handle for s in states])
        self.ctx.check(self.lib.pnmol_filter_set_recorder(self.handle, len(states), slots), "pnmol_filter_set_recorder")
        self._recorder = states

    def clear_recorder(self):
        """Drop the recorder: the filter then takes the launches and gives the bits of one that never had a recorder."""
        self._clear("pnmol_filter_set_recorder", 0, None)
        self._recorder = None

    def recorder_pending(self):
        """(next, count): the recorder's cursor -- the slot the next step fills -- and its number of slots ((0, 0): none)."""
        return self._pending("pnmol_filter_recorder_pending")

    def recorder_means(self, first=0, count=None):
        """Means (count, n, d_state) of the filled slots [first, first + count) (default: up to the cursor), raw coordinates, in
        one read-back (`pnmol_filter_recorder_means`)."""
        if count is None:
            count = self.recorder_pending()[0] - first
        out = np.empty((max(int(count), 0), self.n, self.ds))
        self.ctx.check(self.lib.pnmol_filter_recorder_means(self.handle, int(first), int(count), _dp(out)),
                       "pnmol_filter_recorder_means")
        return out

    def smoother_steps(self, states, dts, keep=False):
        """The whole RTS backward pass in one call (`pnmol_smoother_steps`): `states` the T+1 filtered States, `dts` the T steps
        between them.  Returns (means (T+1, d), stds (T+1, d)) -- the smoothed read-outs of derivative 0 -- and, with keep=True,
        a third element: the T+1 smoothed States (the last one a copy of the terminal filtered state)."""
        states = list(states)
        dts = _f64(np.atleast_1d(dts))
        T = len(states) - 1
        if T < 1 or dts.shape != (T,):
            raise ValueError(f"smoother_steps needs T + 1 >= 2 states and T step sizes, got {len(states)} and {dts.shape}")
        filt = (_vp * (T + 1))(*[None if s is None else s.handle for s in states])
        out = [State(self) for _ in range(T + 1)] if keep else None
        outs = None if out is None else (_vp * (T + 1))(*[s.handle for s in out])
        means, stds = np.empty((T + 1, self.d)), np.empty((T + 1, self.d))
        info = (ctypes.c_int * T)()
        rc = self.lib.pnmol_smoother_steps(self.handle, T, filt, _dp(dts), outs, _dp(means), _dp(stds), info)
        self.ctx.check(rc, "pnmol_smoother_steps")
        return (means, stds, out) if keep else (means, stds)

    def functionals(self, states, dts, weights):
        """(mean (Q,), cov (Q, Q)) of the Q linear functionals sum_k weights[:, k] . x_k of the trajectory under the smoothing
        posterior (`pnmol_functionals`): `states` the T+1 filtered States, `dts` the T steps between them, `weights`
        (Q, T+1, n, d) in raw coordinates.  One call, one synchronisation; the states are only read."""
        states = list(states)
        T = len(states) - 1
        dts = _f64(np.atleast_1d(dts)) if T > 0 else np.zeros(0)
        weights = _f64(weights)
        if T < 0 or dts.shape != (T,):
            raise ValueError(f"functionals needs T + 1 >= 1 states and T step sizes, got {len(states)} and {dts.shape}")
        if weights.ndim != 4 or weights.shape[1:] != (T + 1, self.n, self.d) or weights.shape[0] < 1:
            raise ValueError(f"functionals: weights must be (Q, {T + 1}, {self.n}, {self.d}), got {weights.shape}")
        Q = weights.shape[0]
        filt = (_vp * (T + 1))(*[None if s is None else s.handle for s in states])
        mean, cov = np.empty(Q), np.empty((Q, Q))
        rc = self.lib.pnmol_functionals(self.handle, T, filt, _dp(dts) if T > 0 else None, Q, _dp(weights), _dp(mean), _dp(cov))
        self.ctx.check(rc, "pnmol_functionals")
        return mean, cov

    def predict(self, state, dt):
        """The prior alone carried over dt > 0 from `state` (`pnmol_state_predict`): a new State at state.t + dt."""
        out = State(self)
        self.ctx.check(self.lib.pnmol_state_predict(self.handle, state.handle, float(dt), out.handle), "pnmol_state_predict")
        return out

    def predict_marginals(self, state, dts):
        """(means, stds), each (len(dts), n, d): the prediction from `state` over every dts[i] >= 0, all derivatives, raw
        coordinates (`pnmol_state_predict_marginals`)."""
        dts = _f64(np.atleast_1d(dts))
        if dts.ndim != 1 or dts.size < 1:
            raise ValueError(f"expected a non-empty 1-d array of step sizes, got shape {dts.shape}")
        means, stds = np.empty((dts.size, self.n, self.d)), np.empty((dts.size, self.n, self.d))
        rc = self.lib.pnmol_state_predict_marginals(self.handle, state.handle, dts.size, _dp(dts), _dp(means), _dp(stds))
        self.ctx.check(rc, "pnmol_state_predict_marginals")
        return means, stds

    def steps(self, state, k, dt, want_means=True, want_stds=True):
        means = np.empty((k, self.d)) if want_means else None
        stds = np.empty((k, self.d)) if want_stds else None
        infos = (StepOut * k)()
        rc = self.lib.pnmol_filter_steps(self.handle, state.handle, int(k), float(dt),
                                         _dp(means) if want_means else None, _dp(stds) if want_stds else None, infos)
        self.ctx.check(rc, "pnmol_filter_steps")
        if self.reaction is not None or self._operator_schedule:
            self.error_model_dt = None      # (the loop re-linearises: an error model prepared before is forgotten)
        return means, stds, infos

    def steps_begin(self, state, k, dt):
        self.ctx.check(self.lib.pnmol_filter_steps_begin(self.handle, state.handle, int(k), float(dt)),
                       "pnmol_filter_steps_begin")
        if self.reaction is not None or self._operator_schedule:
            self.error_model_dt = None      # (the loop re-linearises: an error model prepared before is forgotten)
        self._pending_k = int(k)

    def steps_end(self, state, want_means=True, want_stds=True):
        k = self._pending_k
        means = np.empty((k, self.d)) if want_means else None
        stds = np.empty((k, self.d)) if want_stds else None
        infos = (StepOut * k)()
        rc = self.lib.pnmol_filter_steps_end(self.handle, state.handle, _dp(means) if want_means else None,
                                             _dp(stds) if want_stds else None, infos)
        self.ctx.check(rc, "pnmol_filter_steps_end")
        return means, stds, infos

    def prepare_steps(self, state, k, dt):
        self.ctx.check(self.lib.pnmol_filter_prepare_steps(self.handle, state.handle, int(k), float(dt)),
                       "pnmol_filter_prepare_steps")

    def last_steps_ms(self):
        ms = ctypes.c_float(0.0)
        self.lib.pnmol_filter_last_steps_ms(self.handle, ctypes.byref(ms))
        return float(ms.value)

    def debug_poison(self):
        self.ctx.check(self.lib.pnmol_filter_debug_poison(self.handle), "pnmol_filter_debug_poison")

    def debug_read(self, which, count):
        out = np.empty(int(count))
        self.ctx.check(self.lib.pnmol_filter_debug_read(self.handle, int(which), _dp(out), int(count)),
                       "pnmol_filter_debug_read")
        return out


class State:
    """`pnmol_state`: device-resident (t, mean, covariance) of one filter state."""

    def __init__(self, flt, _handle=None):
        self.filter, self.lib, self.ctx = flt, flt.lib, flt.ctx
        if _handle is None:
            _handle = _vp()
            self.ctx.check(self.lib.pnmol_state_create(flt.handle, ctypes.byref(_handle)), "pnmol_state_create")
        self.handle = _handle
        flt._live[id(self)] = _handle

    def _destroy(self):
        h, self.handle = getattr(self, "handle", None), None
        flt = getattr(self, "filter", None)
        # (no entry: Filter.__del__ ran first and has destroyed this state's handle already)
        if h and flt is not None and flt._live.pop(id(self), None) is not None:
            self.lib.pnmol_state_destroy(h)

    def __del__(self):
        self._destroy()

    def clone(self):
        h = _vp()
        self.ctx.check(self.lib.pnmol_state_clone(self.handle, ctypes.byref(h)), "pnmol_state_clone")
        return State(self.filter, h)

    def set(self, t, mean_nd, cov_DD):
        f = self.filter
        D = f.n * f.ds
        a, b = _f64(mean_nd, (f.n, f.ds)), _f64(cov_DD, (D, D))
        self.ctx.check(self.lib.pnmol_state_set(self.handle, float(t), _dp(a), _dp(b)), "pnmol_state_set")

    def set_sqrtm(self, t, mean_nd, cov_sqrtm_DD):
        """As `set`, from any square root C of the covariance; C C^T is formed on the device."""
        f = self.filter
        D = f.n * f.ds
        a, b = _f64(mean_nd, (f.n, f.ds)), _f64(cov_sqrtm_DD, (D, D))
        self.ctx.check(self.lib.pnmol_state_set_sqrtm(self.handle, float(t), _dp(a), _dp(b)), "pnmol_state_set_sqrtm")

    @property
    def t(self):
        t = ctypes.c_double(0.0)
        self.lib.pnmol_state_get_time(self.handle, ctypes.byref(t))
        return t.value

    def mean(self):
        out = np.empty((self.filter.n, self.filter.ds))
        self.ctx.check(self.lib.pnmol_state_get_mean(self.handle, _dp(out)), "pnmol_state_get_mean")
        return out

    def marginal_var(self):
        out = np.empty((self.filter.n, self.filter.ds))
        self.ctx.check(self.lib.pnmol_state_get_marginal_var(self.handle, _dp(out)), "pnmol_state_get_marginal_var")
        return out

    def cov_sqrtm(self):
        """Lower-triangular Cholesky factor of the covariance (device Cholesky), reference state order."""
        D = self.filter.n * self.filter.ds
        out = np.empty((D, D))
        self.ctx.check(self.lib.pnmol_state_get_cov_sqrtm(self.handle, _dp(out)), "pnmol_state_get_cov_sqrtm")
        return out

    def cov(self):
        D = self.filter.n * self.filter.ds
        out = np.empty((D, D))
        self.ctx.check(self.lib.pnmol_state_get_cov(self.handle, _dp(out)), "pnmol_state_get_cov")
        return out


class Bridge:
    """`pnmol_bridge`: what dense output inside one step [t, t + dt] of a smoothed solution needs, device-resident."""

    def __init__(self, flt, handle, interval=None):
        self.filter, self.lib, self.ctx = flt, flt.lib, flt.ctx
        self.handle = handle
        flt._live_bridges[id(self)] = handle
        if interval is None:                            # (t, dt, full) as the maker of the bridge knows them, or from the library
            t, dt, full = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(0)
            self.lib.pnmol_bridge_get_interval(handle, ctypes.byref(t), ctypes.byref(dt), ctypes.byref(full))
            interval = (t.value, dt.value, bool(full.value))
        self.t, self.dt, self.full = interval

    def _destroy(self):
        h, self.handle = getattr(self, "handle", None), None
        flt = getattr(self, "filter", None)
        # (no entry: Filter.__del__ ran first and has destroyed this bridge's handle already)
        if h and flt is not None and flt._live_bridges.pop(id(self), None) is not None:
            self.lib.pnmol_bridge_destroy(h)

    def __del__(self):
        self._destroy()

    def eval(self, ts):
        """(means, stds), each (len(ts), n, d): posterior mean and marginal std of all derivatives at the times `ts` inside
        [t, t + dt], raw coordinates (`pnmol_bridge_eval`: one launch, the read-out copied into the result arrays)."""
        ts = _f64(np.atleast_1d(ts))
        if ts.ndim != 1 or ts.size < 1:
            raise ValueError(f"expected a non-empty 1-d array of times, got shape {ts.shape}")
        f = self.filter
        means, stds = np.empty((ts.size, f.n, f.d)), np.empty((ts.size, f.n, f.d))
        self.ctx.check(self.lib.pnmol_bridge_eval(self.handle, ts.size, _dp(ts), _dp(means), _dp(stds)), "pnmol_bridge_eval")
        return means, stds

    def state(self, smooth_k, smooth_next, t):
        """The full posterior at t strictly inside the interval as a new State (`pnmol_bridge_state`; needs a "full" bridge);
        smooth_k / smooth_next: the smoothed states at the two ends."""
        out = State(self.filter)
        rc = self.lib.pnmol_bridge_state(self.handle, smooth_k.handle, smooth_next.handle, float(t), out.handle)
        self.ctx.check(rc, "pnmol_bridge_state")
        return out


class Samples:
    """`pnmol_samples`: S joint draws of the state at one time point, device-resident; `draw` at the terminal state, then
    `step_back` through the filtered states in decreasing time."""

    def __init__(self, flt, num_samples, _handle=None):
        self.filter, self.lib, self.ctx = flt, flt.lib, flt.ctx
        self.num_samples = int(num_samples)
        h = _handle
        if h is None:
            h = _vp()
            self.ctx.check(self.lib.pnmol_samples_create(flt.handle, self.num_samples, ctypes.byref(h)), "pnmol_samples_create")
        self.handle = h
        flt._live_samples[id(self)] = h

    def _destroy(self):
        h, self.handle = getattr(self, "handle", None), None
        flt = getattr(self, "filter", None)
        # (no entry: Filter.__del__ ran first and has destroyed this block's handle already)
        if h and flt is not None and flt._live_samples.pop(id(self), None) is not None:
            self.lib.pnmol_samples_destroy(h)

    def __del__(self):
        self._destroy()

    def _noise(self, xi, cols):
        return None if xi is None else _f64(xi, (self.num_samples, cols))

    def draw(self, state, xi=None, *, seed=0, step_index=0, scale=1.0):
        """x <- mean + scale * C xi with C C^T = cov(state) (`pnmol_samples_draw`); xi (S, D) or None (device generator)."""
        a = self._noise(xi, self.filter.n * self.filter.d)
        rc = self.lib.pnmol_samples_draw(self.handle, state.handle, None if a is None else _dp(a), int(seed), int(step_index),
                                         float(scale))
        self.ctx.check(rc, "pnmol_samples_draw")

    def step_back(self, filt_k, dt, xi=None, *, seed=0, step_index=0, scale=1.0):
        """One backward step in place (`pnmol_samples_step_back`); xi (S, 2D) or None (device generator)."""
        a = self._noise(xi, 2 * self.filter.n * self.filter.d)
        rc = self.lib.pnmol_samples_step_back(self.handle, filt_k.handle, float(dt), None if a is None else _dp(a), int(seed),
                                              int(step_index), float(scale))
        self.ctx.check(rc, "pnmol_samples_step_back")

    def clone(self):
        """A copy of this block (`pnmol_samples_clone`)."""
        h = _vp()
        self.ctx.check(self.lib.pnmol_samples_clone(self.handle, ctypes.byref(h)), "pnmol_samples_clone")
        return Samples(self.filter, self.num_samples, h)

    def interpolate(self, left, right, t, xi=None, *, seed=0, step_index=0, scale=1.0):
        """This block <- draws at t, left.t < t < right.t, coupled to the draws in `left` and `right` (`pnmol_samples_interpolate`);
        right=None carries `left` forwards by the prior.  xi (S, D) or None (device generator)."""
        a = self._noise(xi, self.filter.n * self.filter.d)
        rc = self.lib.pnmol_samples_interpolate(self.handle, left.handle, None if right is None else right.handle, float(t),
                                                None if a is None else _dp(a), int(seed), int(step_index), float(scale))
        self.ctx.check(rc, "pnmol_samples_interpolate")

    def get(self):
        """The draws as (S, n, d), raw coordinates."""
        out = np.empty((self.num_samples, self.filter.n, self.filter.d))
        self.ctx.check(self.lib.pnmol_samples_get(self.handle, _dp(out)), "pnmol_samples_get")
        return out

    @property
    def t(self):
        t = ctypes.c_double(0.0)
        self.ctx.check(self.lib.pnmol_samples_get_time(self.handle, ctypes.byref(t)), "pnmol_samples_get_time")
        return t.value


class SqrtFilter:
    """`pnmol_sqrt_filter`: the white-noise EK1 step in square-root (QR) form, one device-resident state."""

    def __init__(self, ctx, *, L, B, E_sqrtm, R_sqrtm, Gamma, num_derivatives, dtype="f64"):
        """L (d, ds), B (nB, ds), Gamma (ds, ds) with ds = d (white-noise) or 2d (latent-force: [L, I], [B, 0],
        blockdiag(chol K, E_sqrtm), zero noise factors) -- the conventions of `Filter`.  dtype "f32": the QR (work
        matrices, reflectors, trailing updates) in fp32; the state, the mean path and all scalars stay fp64."""
        self.ctx = ctx
        self.dtype = dtype
        d, ds = L.shape
        nB = 0 if B is None else B.shape[0]
        self._keep = [_f64(L, (d, ds)), _f64(B if nB else np.zeros((0, ds))), _f64(E_sqrtm, (d, d)),
                      _f64(R_sqrtm if nB else np.zeros((0, 0))), _f64(Gamma, (ds, ds))]
        desc = FilterDesc(d=d, num_derivatives=int(num_derivatives), nB=nB, L=_dp(self._keep[0]),
                          B=_dp(self._keep[1]) if nB else None, E_sqrtm=_dp(self._keep[2]),
                          R_sqrtm=_dp(self._keep[3]) if nB else None, Gamma=_dp(self._keep[4]), d_state=ds,
                          dtype=Filter.DTYPES[dtype])
        h = _vp()
        ctx.check(ctx.lib.pnmol_sqrt_filter_create(ctx.handle, ctypes.byref(desc), ctypes.byref(h)),
                  "pnmol_sqrt_filter_create")
        self.handle, self.d, self.ds, self.n, self.m = h, d, ds, int(num_derivatives) + 1, d + nB

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.ctx.lib.pnmol_sqrt_filter_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def set_state(self, t, mean, cov_sqrtm):
        D = self.n * self.ds
        mean, C = _f64(mean, (self.n, self.ds)), _f64(cov_sqrtm, (D, D))
        self.ctx.check(self.ctx.lib.pnmol_sqrt_filter_set_state(self.handle, float(t), _dp(mean), _dp(C)),
                       "pnmol_sqrt_filter_set_state")

    def get_state(self, *, factor=True):
        D = self.n * self.ds
        t, mean = ctypes.c_double(0), np.empty((self.n, self.ds))
        C = np.empty((D, D)) if factor else None
        self.ctx.check(self.ctx.lib.pnmol_sqrt_filter_get_state(self.handle, ctypes.byref(t), _dp(mean),
                                                                 _dp(C) if factor else None), "pnmol_sqrt_filter_get_state")
        return t.value, mean, C

    def predict_mean(self, dt):
        out = np.empty(self.d)
        self.ctx.check(self.ctx.lib.pnmol_sqrt_filter_predict_mean(self.handle, float(dt), _dp(out)),
                       "pnmol_sqrt_filter_predict_mean")
        return out

    def set_operator(self, M, shift=None):
        M = _f64(M, (self.d, self.ds))
        sh = None if shift is None else _f64(shift, (self.d,))
        self.ctx.check(self.ctx.lib.pnmol_sqrt_filter_set_operator(self.handle, _dp(M), None if sh is None else _dp(sh)),
                       "pnmol_sqrt_filter_set_operator")

    def prepare_error_model(self, dt):
        self.ctx.check(self.ctx.lib.pnmol_sqrt_filter_prepare_error_model(self.handle, float(dt)),
                       "pnmol_sqrt_filter_prepare_error_model")

    def step(self, dt, want_error=False):
        info = StepOut()
        err = np.empty(self.d) if want_error else None
        self.ctx.check(self.ctx.lib.pnmol_sqrt_filter_step(self.handle, float(dt), ctypes.byref(info),
                                                           _dp(err) if want_error else None), "pnmol_sqrt_filter_step")
        return (info, err) if want_error else info

    def steps(self, k, dt):
        means, stds = np.empty((k, self.ds)), np.empty((k, self.ds))
        infos = (StepOut * k)()
        self.ctx.check(self.ctx.lib.pnmol_sqrt_filter_steps(self.handle, int(k), float(dt), _dp(means), _dp(stds), infos),
                       "pnmol_sqrt_filter_steps")
        return means, stds, list(infos)

    def last_steps_ms(self):
        ms = ctypes.c_float(0)
        self.ctx.lib.pnmol_sqrt_filter_last_steps_ms(self.handle, ctypes.byref(ms))
        return ms.value
