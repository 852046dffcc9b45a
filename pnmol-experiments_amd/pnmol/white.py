"""White-noise EK1 PDE filters (reference: src/pnmol/white.py).

`attempt_step` and the constant-step loop run on the GPU through libpnmol_hip.so in the
covariance (Cholesky) form that the reference's own tests prove equivalent to its QR form
(tests/test_base/test_sqrt.py:48-78).  There is no CPU implementation of the step in this package.

Documented deviations from the reference's numbers:
  * `cov_sqrtm` is the lower-triangular Cholesky factor of the same covariance (device Cholesky); the reference's QR
    factor differs by column signs, and arbitrarily where a pivot is exactly zero (noise-free Dirichlet nodes).
  * `diffusion_squared_local`: the reference evaluates |R1^-1 z|^2 / m with the QR factor R1 of the
    innovation (white.py:125), whose row signs LAPACK chooses from the data; here the same formula is
    evaluated with the Cholesky factor (positive diagonal).  `last_step_info.sigma2_whitened` holds
    z^T S^-1 z / m.
"""

import collections
import contextlib
import os

import numpy as np
import scipy.linalg
import scipy.sparse

from . import _hip, data, pdefilter
from .base import iwp, rv
from .odetools import step as _step


IteratedSolution = collections.namedtuple(
    "IteratedSolution", "filtered means stds smoothed increments num_iterations converged data_log_likelihood data_log_likelihoods")
IteratedSolution.__doc__ = """Result of `solve_iterated`: the last pass's filtering `PDESolution`, the smoothed means / stds (T+1, d),
the `smooth()` solution of the last pass (or None), the relative increment of every pass beyond pass 0, their number, whether the
last increment met the tolerance, and with observations the data log-likelihoods of the last pass (else None)."""

_LoopPlan = collections.namedtuple("_LoopPlan", "ts dts points forcing operator observations sensors at_t0")
_LoopPlan.__doc__ = """What one run of the device-resident constant-step loop needs, validated on the host (`_loop_plan`): the schedule
`ts` / `dts`; per option its table or None -- `points` (T, d) to linearise at, `forcing` (T, m) right-hand sides, `operator` (T, R)
coefficients of a time-dependent operator --; `observations` as
`data.prepare` returns them (None: the caller gave none); `sensors` = (times, C, R_sqrtm, ys) of the shared sensor array for the
observations behind t0 (None: there are none); `at_t0`: whether `observations[0]` sits at t0 and updates the initial state."""


def _padded_to_state(C, ds):
    """C with zero columns up to the state width `ds` of the bound filter (the eps half of a latent-force state)."""
    return C if C.shape[1] == ds else np.hstack((C, np.zeros((C.shape[0], ds - C.shape[1]))))


class _WhiteNoiseEK1Base(pdefilter.PDEFilter):
    _device_filter = None
    _device_pde = None
    _error_models = None
    last_step_info = None
    _covariance_form = True     # (pnmol.sqrtform: False)

    def _is_fp64_covariance_form(self):
        """This solver advances an fp64 covariance: `pnmol.white` / `pnmol.latent` with dtype "f64", not `pnmol.sqrtform`.  What the
        loop's options, the recorder, the device's own linearisation and the backward walks need."""
        return self._covariance_form and self.dtype == "f64"

    # ------------------------------------------------------------------ cold path
    def initialize_iwp(self, pde):
        """Gamma = chol(k(X, X^T)); IWP prior; E0, E1 (white.py:82-94)."""
        X = pde.mesh_spatial.points
        gram = self.spatial_kernel(X, X.T)
        self._last_gram = gram          # (handed to the device filter as it is: no Gamma Gamma^T product, `_bind`)
        diffusion_state_sqrtm = self._cholesky(gram)
        prior = iwp.IntegratedWienerTransition(num_derivatives=self.num_derivatives,
                                               wiener_process_dimension=pde.y0.shape[0],
                                               wp_diffusion_sqrtm=diffusion_state_sqrtm)
        return prior, prior.projection_matrix(0), prior.projection_matrix(1), diffusion_state_sqrtm

    # Gamma = chol(K) on the device (`pnmol_cholesky_lower`) from d >= CHOLESKY_ON_DEVICE_FROM mesh points on
    # (PNMOL_CHOL_ON_DEVICE=0/1 forces it off / on); LAPACK on the host below that (the factors agree to rounding:
    # tests/test_gpu_assembly.py)
    CHOLESKY_ON_DEVICE_FROM = 2048

    def _cholesky(self, gram):
        mode = os.environ.get("PNMOL_CHOL_ON_DEVICE", "")
        on_device = gram.shape[0] >= self.CHOLESKY_ON_DEVICE_FROM if mode not in ("0", "1") else mode == "1"
        if on_device:
            return (self._context or _hip.Context.default()).cholesky(gram)
        return np.linalg.cholesky(gram)

    _last_gram = None
    _context = None   # set to an `_hip.Context` to run this solver on its own device / stream
    # Build-side option (the reference is fp64 throughout, src/pnmol/__init__.py:9-11):
    # "f32" keeps the covariance and its bulk kernels in fp32 (include/pnmol_hip.h, pnmol_filter_desc.dtype;
    # BASELINE config 5).  Accuracy: DESIGN.md section 11.
    dtype = "f64"
    # The fp32 covariance diverges without an error flag for num_derivatives >= 2 (mean errors of 1e10
    # after 40 steps at N=256): refused unless a study asks for exactly that.
    allow_unstable_f32 = False

    def _bind(self, pde, gamma):
        if self.dtype == "f32" and self.num_derivatives > 1 and not self.allow_unstable_f32:
            raise ValueError('dtype="f32" keeps the covariance in single precision, which is only accurate for '
                             'num_derivatives = 1 (DESIGN.md section 11); use the fp64 path, or pnmol.sqrtform with dtype="f32"')
        ctx = self._context or _hip.Context.default()
        gram = self._last_gram if (self._last_gram is not None and self._last_gram.shape == gamma.shape) else gamma @ gamma.T
        self._device_filter = _hip.Filter(ctx, L=pde.L, B=pde.B, E_sqrtm=pde.E_sqrtm, R_sqrtm=pde.R_sqrtm, Gamma=gamma,
                                          num_derivatives=self.num_derivatives, dtype=self.dtype, K=gram)
        self._device_pde = pde
        self._gram = gram
        self._error_models = {}
        operator = getattr(pde, "time_dependent_operator", None)
        if operator is not None:                                # (checked by `_check_operator_supported` in front of `_bind`)
            self._device_filter.set_operator_family(operator.operators, operator.noise_diagonals)
        if self._reaction_for_device(pde) is not None:
            self._device_filter.set_reaction(pde.reaction)

    def _reaction_for_device(self, pde):
        """The reaction term the device evaluates itself for this solver and problem, or None (host callables)."""
        return None

    # ------------------------------------------------------------------ time-dependent operators
    def _check_operator_supported(self, pde):
        """A problem with `pde.time_dependent_operator` (pde/coefficients.py) is honoured or refused, never ignored: the refusal,
        before any device work.  Returns the operator, or None."""
        operator = getattr(pde, "time_dependent_operator", None)
        if operator is None:
            return None
        from . import latent
        from .pde.reactions import Reaction

        is_latent = isinstance(self, latent._LatentForceEK1Base)
        ok = (self._is_fp64_covariance_form() and not is_latent
              and (not self.semilinear or isinstance(self._reaction_for_device(pde), Reaction)))
        if not ok:
            raise TypeError(f"pde.time_dependent_operator is honoured by the fp64 covariance-form solvers LinearWhiteNoiseEK1 and "
                            f"SemiLinearWhiteNoiseEK1 with a scalar reaction the device linearises (`pde.reaction`, "
                            f"reaction_on_device=True); "
                            f"{type(self).__module__}.{type(self).__name__} with dtype={self.dtype!r} on this problem is not one")
        return operator

    # ------------------------------------------------------------------ driven problems
    def _check_forcing_supported(self, pde):
        """A problem with `pde.forcing` (pde/forcing.py) is honoured or refused, never ignored: the refusal, before any device
        work.  Returns the forcing, or None.  Every entry point of every solver class comes through here, so the refusal of a
        time-dependent operator (`_check_operator_supported`) is made here as well."""
        self._check_operator_supported(pde)
        forcing = getattr(pde, "forcing", None)
        if forcing is None:
            return None
        from . import latent

        is_latent = isinstance(self, latent._LatentForceEK1Base)
        ok = (self._is_fp64_covariance_form()
              and (not self.semilinear or (not is_latent and self._reaction_for_device(pde) is not None)))
        if not ok:
            raise TypeError(f"pde.forcing (source / boundary values) is honoured by the fp64 covariance-form solvers "
                            f"LinearWhiteNoiseEK1, LinearLatentForceEK1 and SemiLinearWhiteNoiseEK1 with a term the device "
                            f"linearises (`pde.reaction`, reaction_on_device=True); "
                            f"{type(self).__module__}.{type(self).__name__} with dtype={self.dtype!r} on this problem is not one")
        return forcing

    def _linearize_forced(self, pde, m_at, t):
        """(M, shift (d,), g (nB,)) of the measurement z = [x1 - M x0 + shift; B x0 - g] at time t: `_linearize`, with the source
        of `pde.forcing` taken off the shift (a semilinear `_linearize` has done so: `pde.f` includes the source) and its boundary
        values."""
        M, shift = self._linearize(pde, m_at, t)
        forcing = getattr(pde, "forcing", None)
        if forcing is None:
            return M, shift, np.zeros(pde.B.shape[0])
        if not self.semilinear:
            shift = shift - forcing.source_values(t, pde)
        return M, shift, forcing.boundary(t, pde)

    # True: the reference's own two `update_sqrt` calls, on the device (below); False: closed form on the host (O(d^3) LAPACK);
    # None (default; PNMOL_INIT_ON_DEVICE=0/1 overrides): on the device from n d >= 4096 on, where the host form takes
    # seconds (64x64 mesh: 18 s against 10 s), closed form below that (its rounding-level entries are what the
    # factor-level tests are tuned to; both match the oracle at the north-star tolerances)
    initialize_on_device = {"0": False, "1": True}.get(os.environ.get("PNMOL_INIT_ON_DEVICE", ""), None)
    INIT_ON_DEVICE_FROM = 4096

    def _initialize_on_device(self, pde, gamma):
        """white.py:12-80 as written: prior kron(Gamma, c I) -> update_sqrt on y0 (nugget 1e-10) -> update_sqrt on the
        PDE/BC residual at t0, both QRs on the device (include/pnmol_sqrt.h); the factor goes to the device state, which
        forms C C^T itself (`pnmol_state_set_sqrtm`).  No O(d^3) host work."""
        from .base import sqrt as dsqrt

        ctx = self._device_filter.ctx
        n, d, nB = self.num_derivatives + 1, pde.L.shape[0], pde.B.shape[0]
        C0_raw = np.zeros((n * d, n * d))               # = np.kron(gamma, c I_n) (white.py:21-24), without kron's temporaries
        for a in range(n):
            C0_raw[a::n, a::n] = self.diffuse_prior_scale * gamma
        C0_y0, k_y0, _ = dsqrt.update_sqrt(self.E0, C0_raw, 1e-10 * np.eye(d), ctx=ctx)
        m0_y0 = k_y0 @ pde.y0
        M, shift, g = self._linearize_forced(pde, m0_y0[0::n], pde.t0)
        H = np.zeros((d + nB, n * d))
        H[:d, 0::n] = -M
        H[np.arange(d), np.arange(d) * n + 1] += 1.0
        H[d:, 0::n] = pde.B
        z = H @ m0_y0 + np.concatenate([shift, -g])
        E = np.zeros((d + nB, d + nB))
        E[:d, :d], E[d:, d:] = pde.E_sqrtm, pde.R_sqrtm
        C0, k, _ = dsqrt.update_sqrt(H, C0_y0, E + 1e-10 * np.eye(d + nB), ctx=ctx)
        mean = (m0_y0 - k @ z).reshape((n, d), order="F")
        dev = self._device_filter.new_state()
        dev.set_sqrtm(pde.t0, mean, C0)
        return mean, dev

    def initialize(self, pde):
        """Initial state: prior conditioned on y0 and on the PDE/BC residual at t0 (white.py:12-80).

        The two updates of the reference have observation noise ~1e-20, which a plain covariance
        update cannot resolve; here they are evaluated block-wise in closed form (the prior
        Gamma Gamma^T (x) c^2 I is Kronecker, the derivative blocks decouple), every difference
        written so that it does not cancel.  O(d^3) on the host, once per solve.  A driven problem (`pde.forcing`): the update
        at t0 measures against rhs(t0).
        """
        self._check_forcing_supported(pde)
        self.iwp, self.E0, self.E1, gamma = self.initialize_iwp(pde)
        self._bind(pde, gamma)
        n, d = self.num_derivatives + 1, pde.L.shape[0]
        on_device = self.initialize_on_device
        if on_device is None:
            on_device = n * d >= self.INIT_ON_DEVICE_FROM
        if on_device:
            mean, dev = self._initialize_on_device(pde, gamma)
            return pdefilter.PDEFilterState(t=pde.t0, y=rv.DeviceMultivariateNormal(mean, dev), error_estimate=None,
                                            reference_state=None, diffusion_squared_local=[])
        mean, blocks = self._initial_moments(pde)
        cov = np.zeros((n * d, n * d))
        for (a, b), blk in blocks.items():
            cov[a::n, b::n] = blk
        dev = self._device_filter.new_state()
        dev.set(pde.t0, mean, cov)
        return pdefilter.PDEFilterState(t=pde.t0, y=rv.DeviceMultivariateNormal(mean, dev), error_estimate=None,
                                        reference_state=None, diffusion_squared_local=[])

    def _initial_moments(self, pde):
        n, d = self.num_derivatives + 1, pde.L.shape[0]
        eps2 = 1e-10 ** 2                                       # (1e-10 I)(1e-10 I)^T, white.py:33-39
        Kc = self.diffuse_prior_scale ** 2 * self._gram         # C0 C0^T = K (x) c^2 I, white.py:21-24
        # update 1: observe E0 x = y0.  V0 = Kc - Kc S1^-1 Kc = eps2 Kc S1^-1 (no cancellation)
        S1 = scipy.linalg.cho_factor(Kc + eps2 * np.eye(d), lower=True)
        G1 = scipy.linalg.cho_solve(S1, Kc).T                   # Kc S1^-1
        V0 = eps2 * 0.5 * (G1 + G1.T)
        m0 = G1 @ pde.y0
        # update 2 (white.py:42-58): rows [E1 - M E0 ; B E0], noise (E_bc + 1e-10 I)(...)^T, block diagonal
        M, shift, g = self._linearize_forced(pde, m0, pde.t0)
        nB = pde.B.shape[0]
        En = pde.E_sqrtm + 1e-10 * np.eye(d)
        Rn = pde.R_sqrtm + 1e-10 * np.eye(nB)
        Re, Rb = En @ En.T, Rn @ Rn.T
        # (a) boundary rows involve derivative 0 only
        if nB > 0:
            Sb = pde.B @ V0 @ pde.B.T + Rb
            Gb = np.linalg.solve(Sb, pde.B @ V0).T              # V0 B^T Sb^-1
            m0 = m0 - Gb @ (pde.B @ m0 - g)
            V0 = V0 - Gb @ (pde.B @ V0)
            V0 = 0.5 * (V0 + V0.T)
        # (b) PDE rows: z = x1 - M x0 + shift, prior blockdiag(V0, Kc);  Sp = Kc + T, T tiny
        T = M @ V0 @ M.T + Re
        Sp = scipy.linalg.cho_factor(Kc + T, lower=True)
        z = -M @ m0 + shift
        Spz = scipy.linalg.cho_solve(Sp, z)
        SpT = scipy.linalg.cho_solve(Sp, T)                     # Sp^-1 T
        V0Mt = V0 @ M.T
        mean = np.zeros((n, d))
        mean[0] = m0 + V0Mt @ Spz
        mean[1] = -(z - T @ Spz)                                # -Kc Sp^-1 z
        P00 = V0 - V0Mt @ scipy.linalg.cho_solve(Sp, V0Mt.T)
        P01 = V0Mt - V0Mt @ SpT                                 # V0 M^T Sp^-1 Kc
        P11 = T - T @ SpT                                       # Kc - Kc Sp^-1 Kc
        blocks = {(0, 0): 0.5 * (P00 + P00.T), (0, 1): P01, (1, 0): P01.T, (1, 1): 0.5 * (P11 + P11.T)}
        for q in range(2, n):
            blocks[(q, q)] = Kc
        return mean, blocks

    # ------------------------------------------------------------------ step-invariant error model
    def _error_model(self, pde, dt, M=None):
        """Sq^-1 and diag(Sq) of `estimate_error` (white.py:153-162) in the Nordsieck frame of dt.
        `M` is the operator of the linearisation (L for linear problems: cached per dt; J_x + L otherwise)."""
        key = float(dt)
        cache = M is None
        M = pde.L if M is None else M
        if not cache or self._error_models is None or key not in self._error_models:
            d, nB = pde.L.shape[0], pde.B.shape[0]
            s, _ = self.iwp.nordsieck_preconditioner_1d_raw(dt)
            n = self.num_derivatives + 1
            Q1 = np.flip(scipy.linalg.hilbert(n))
            Hv = scipy.sparse.csr_matrix(np.vstack((-M, pde.B)))
            F1K = np.vstack((self._gram, np.zeros((nB, d))))    # [I;0] K
            HvK = Hv @ self._gram
            cross = (Hv @ F1K.T).T                              # F1 K Hv^T
            Sq = Q1[1, 1] * s[1] ** 2 * np.hstack((F1K, np.zeros((d + nB, nB))))
            Sq = Sq + Q1[0, 1] * s[0] * s[1] * (cross + cross.T) + Q1[0, 0] * s[0] ** 2 * (Hv @ HvK.T).T
            Ebc = scipy.linalg.block_diag(pde.E_sqrtm, pde.R_sqrtm)
            Sq = Sq + Ebc @ Ebc.T
            Sq = 0.5 * (Sq + Sq.T)
            inv = scipy.linalg.cho_solve(scipy.linalg.cho_factor(Sq, lower=True), np.eye(d + nB))
            model = (0.5 * (inv + inv.T), np.diag(Sq).copy())
            if not cache:
                return model
            self._error_models = {key: model}
        return self._error_models[key]

    error_model_on_host = False   # True: Sq^-1 from the host (`_error_model`, an O(m^3) solve per new dt) instead of the GPU

    def _ensure_error_model(self, pde, dt):
        if self._device_filter.error_model_dt != float(dt):
            # (a time-dependent operator: the host form knows pde.L and pde.E_sqrtm, which are those of t0)
            if self.error_model_on_host and getattr(pde, "time_dependent_operator", None) is None:
                self._device_filter.set_error_model(dt, *self._error_model(pde, dt))
            else:
                self._device_filter.prepare_error_model(dt)   # Sq factorised by the step's own kernels

    # ------------------------------------------------------------------ hot path
    def _device_state_of(self, state, pde):
        if self._device_filter is None or self._device_pde is not pde:
            raise RuntimeError("call initialize(pde) before attempt_step (the device model is bound there)")
        y = state.y
        if isinstance(y, rv.DeviceMultivariateNormal) and y.device_state.filter is self._device_filter:
            return y.device_state
        dev = self._device_filter.new_state()                   # host-side state: upload mean and C C^T
        C = np.asarray(y.cov_sqrtm)
        dev.set(state.t, np.asarray(y.mean), C @ C.T)
        return dev

    semilinear = False

    @staticmethod
    def _jacobian_diagonal(pde, m_at, t):
        return None

    def attempt_step(self, state, dt, pde):
        """One predict + update + calibrate step on the GPU (white.py:96-146); `state` is not modified."""
        self._check_operator_supported(pde)
        dev_in = self._device_state_of(state, pde)
        operator = getattr(pde, "time_dependent_operator", None)
        if operator is not None:
            # in front of linearise / force: M(t + dt) and its noise from R numbers (`pnmol_filter_operator_at`); the error model
            # is forgotten, so the branches below prepare it for this operator
            self._device_filter.operator_at(operator.coefficients(state.t + dt))
        if self.semilinear and self._device_filter.reaction is not None:
            # pointwise reaction described to the device (pde/reactions.py): linearised there at the predicted mean, nothing
            # comes back and nothing goes up
            self._device_filter.linearize(dev_in, dt)
            self._device_filter.prepare_error_model(dt)
        elif self.semilinear:
            # EK1 linearisation at the predicted mean (white.py:192-208): f and df are host callables, so the
            # predicted point comes back once per step; the new stencil rows and shift go to the device
            flt = self._device_filter
            m_at = flt.predict_mean(dev_in, dt)
            jdiag = self._jacobian_diagonal(pde, m_at, state.t + dt)
            if jdiag is not None and not self.error_model_on_host:
                # pointwise nonlinearity (`df_diagonal`): 2 d numbers go to the device, which patches its stencil rows itself
                fx = np.asarray(pde.f(state.t + dt, m_at), dtype=np.float64)
                flt.set_operator_diagonal(jdiag, jdiag * m_at - fx)
                flt.prepare_error_model(dt)
            else:
                M, shift = self._linearize(pde, m_at, state.t + dt)
                flt.set_operator(M, shift)
                if self.error_model_on_host:
                    flt.set_error_model(dt, *self._error_model(pde, dt, M=M))
                else:
                    flt.prepare_error_model(dt)
        else:
            self._ensure_error_model(pde, dt)
        forcing = getattr(pde, "forcing", None)
        if forcing is not None:                                 # behind the linearisation: the step measures against rhs(t + dt)
            self._device_filter.force_at(forcing.rhs(state.t + dt, pde))
        dev_out, info, error = self._device_filter.step(dev_in, dt)
        self.last_step_info = info
        m_new = dev_out.mean()
        new_state = pdefilter.PDEFilterState(
            t=state.t + dt, error_estimate=error, reference_state=np.abs(m_new[0]),
            y=rv.DeviceMultivariateNormal(m_new, dev_out), diffusion_squared_local=info.diffusion_squared_local)
        return new_state, dict(num_f_evaluations=1, num_df_evaluations=1)

    # ------------------------------------------------------------------ sensor data
    def _check_observations_supported(self):
        if not self._is_fp64_covariance_form():
            raise TypeError(f"observations are supported by the fp64 covariance-form solvers of pnmol.white and pnmol.latent; "
                            f"{type(self).__module__}.{type(self).__name__} with dtype={self.dtype!r} is not one")

    def _observe(self, state, observation):
        """`state` conditioned on `observation` (`pnmol_state_observe`): (new state at the same time,
        log-likelihood of the data).  The observation reads derivative 0 of the solution components; the eps half of a
        latent-force state gets zero columns.  `diffusion_squared_local` keeps its meaning (PDE residuals only)."""
        flt = self._device_filter
        dev_in = self._device_state_of(state, self._device_pde)
        dev_out, res = flt.observe(dev_in, _padded_to_state(observation.C, flt.ds), observation.y, observation.R_sqrtm)
        m_new = dev_out.mean()
        ref = None if state.reference_state is None else np.abs(m_new[0][:observation.C.shape[1]])
        return state._replace(y=rv.DeviceMultivariateNormal(m_new, dev_out), reference_state=ref), res.log_likelihood

    def _checked_linearization_points(self, pde, linearize_at, num_steps_taken):
        """`linearize_at` as the (T, d) array the device takes, or None; refusals in front of any device work."""
        if linearize_at is None:
            return None
        if self._reaction_for_device(pde) is None:
            raise TypeError("linearize_at needs a term the device linearises (SemiLinearWhiteNoiseEK1, fp64 covariance form, "
                            "a problem with `pde.reaction`, reaction_on_device=True)")
        pts = np.ascontiguousarray(np.asarray(linearize_at, dtype=np.float64))
        want = (num_steps_taken, pde.L.shape[0])
        if pts.shape != want:
            raise ValueError(f"linearize_at must have shape {want} -- one row per step of the constant schedule, a runt last "
                             f"step included --, got {pts.shape}")
        if not np.all(np.isfinite(pts)):
            raise ValueError("linearize_at has entries that are not finite")
        return pts

    # ------------------------------------------------------------------ the device loop and its options
    def _loop_plan(self, pde, num_steps, observations, linearize_at):
        """The `_LoopPlan` of a constant-step solve: every argument validated on the host, in front of `initialize`, which binds the
        device."""
        obs = None
        if observations is not None:
            self._check_observations_supported()
            obs = data.prepare(observations, pde, self.steprule, pde.y0.shape[0])
        ts, dts = self._constant_schedule(pde, num_steps)
        points = self._checked_linearization_points(pde, linearize_at, len(dts))
        forcing = self._forcing_table(pde, ts)
        operator = self._operator_table(pde, ts)
        sensors, at_t0 = None, False
        if obs:
            dt0 = self.steprule.first_dt(pde)
            times, C, R, ys = data.shared_sensors(obs)
            if times[-1] > ts[-1] and not data.times_agree(times[-1], ts[-1], dt0):
                raise ValueError(f"observation at t={times[-1]} lies behind the last step taken (t={ts[-1]}, {len(dts)} steps)")
            at_t0 = bool(data.times_agree(obs[0].t, pde.t0, dt0))   # that one updates the initial state, as solve() does it
            if times.size > at_t0:
                sensors = (times[at_t0:], C, R, ys[at_t0:])
        return _LoopPlan(ts, dts, points, forcing, operator, obs, sensors, at_t0)

    def _observe_at_t0(self, state, plan):
        """(`state` conditioned on the observation at t0, [its log-likelihood]); (`state`, []) where the plan has none there."""
        if not plan.at_t0:
            return state, []
        state, ll = self._observe(state, plan.observations[0])
        return state, [ll]

    @contextlib.contextmanager
    def _loop_options(self, flt, plan, slots=None):
        """The options of `plan`, and the recorder into `slots`, installed on `flt` around the loop -- only where there is a step
        to take -- and cleared behind it; yields the names of those installed.  An option is cleared once its setter was attempted
        (one that failed half-way included), recorder first.  Behind a failure of the loop a `PnmolHipError` of a clear is dropped:
        the failure is the one to report.  Otherwise every clear is still attempted and the first such error raised."""
        options = {}                                            # name -> (setter, clear), in install order
        if plan.dts:
            if plan.sensors is not None:
                times, C, R, ys = plan.sensors
                options["observations"] = (lambda: flt.set_observations(times, _padded_to_state(C, flt.ds), ys, R),
                                           flt.clear_observations)
            if slots is not None:
                options["recorder"] = (lambda: flt.set_recorder(slots), flt.clear_recorder)
            if plan.points is not None:
                options["points"] = (lambda: flt.set_linearization_points(plan.points), flt.clear_linearization_points)
            if plan.forcing is not None:
                options["forcing"] = (lambda: flt.set_forcing(plan.forcing), flt.clear_forcing)
            if plan.operator is not None:
                options["operator"] = (lambda: flt.set_operator_schedule(plan.operator), flt.clear_operator_schedule)
        attempted, failed = [], True
        try:
            for name, (install, _) in options.items():
                attempted.append(name)
                install()
            yield tuple(options)
            failed = False
        finally:
            errors = []
            for name in ("recorder", "observations", "points", "forcing", "operator"):
                try:
                    if name in attempted:
                        options[name][1]()
                except _hip.PnmolHipError as error:
                    errors.append(error)
            if errors and not failed:
                raise errors[0]

    def _loop_consumed(self, flt, plan, installed, lls):
        """Behind the loop, inside `_loop_options`: every installed option was used up, or RuntimeError.  Returns the data
        log-likelihoods: `lls` (the update at t0) and those of the loop's updates."""
        T = len(plan.dts)
        if "recorder" in installed:
            filled, count = flt.recorder_pending()
            if filled != count:
                raise RuntimeError(f"{count - filled} step(s) of the loop were not recorded")
        if "observations" in installed:
            applied, nobs = flt.observations_pending()
            if applied != nobs:
                raise RuntimeError(f"{nobs - applied} observation(s) were not reached by the loop")
            lls = lls + [r.log_likelihood for r in flt.observation_results(0, nobs)]
        if "points" in installed and flt.linearization_pending() != (T, T):
            raise RuntimeError("the loop did not consume every linearisation point")
        if "forcing" in installed and flt.forcing_pending() != (T, T):
            raise RuntimeError("the loop did not consume every right-hand side of the forcing")
        if "operator" in installed and flt.operator_schedule_pending() != (T, T):
            raise RuntimeError("the loop did not consume every row of coefficients of the time-dependent operator")
        return lls

    def solve_marginals(self, pde, *, num_steps=None, observations=None, linearize_at=None):
        """Constant-step solve that keeps everything on the device: returns
        (t (T+1,), means (T+1,d), stds (T+1,d), diffusion_squared_local (T,), final PDEFilterState).

        `means`/`stds` are `sol.mean[:, 0]` and sqrt(diag(cov) E0^T) of the reference's read-out
        (experiments/figure1.py:76-80).  Steps follow the t-accumulation of the reference's loop
        (pdefilter.py:140-160, :220-223), including a runt final step when sum(dt) lands short of tmax.

        observations (beyond the reference): `pnmol.data.Observation`s of ONE sensor array (`pnmol.data.shared_sensors`) at grid
        times; the state is conditioned on each behind the step that lands on its time, inside the device loop
        (`pnmol_filter_set_observations`), and the rows of `means` / `stds` are those of the conditioned
        states.  The result then has a sixth element `info = dict(num_steps, data_log_likelihood, data_log_likelihoods)`, as
        `solve(pde, observations=...)` reports them.  Per-time sensor arrays stay with `solve()`.

        linearize_at (beyond the reference; problems whose term the device linearises): (T, d), row k the point at which the step
        that lands on `t[k+1]` linearises the term, in place of its own predicted mean (`pnmol_filter_set_linearization_points`,
        DESIGN.md section 22).  None: the EK1 of the reference.
        """
        if not isinstance(self.steprule, _step.Constant):
            raise TypeError("solve_marginals needs the Constant step rule")
        self._check_forcing_supported(pde)
        plan = self._loop_plan(pde, num_steps, observations, linearize_at)
        state, lls = self._observe_at_t0(self.initialize(pde), plan)
        flt = self._device_filter
        with self._loop_options(flt, plan) as installed:
            out = self._run_device_loop(pde, state, plan.ts, plan.dts)
            lls = self._loop_consumed(flt, plan, installed, lls)
        if observations is None:
            return out
        return out + (dict(num_steps=len(plan.dts), data_log_likelihood=float(sum(lls)), data_log_likelihoods=lls),)

    def _forcing_table(self, pde, ts):
        """The right-hand sides of the constant schedule `ts` (a runt last step included) as the (T, m) table the device takes, or
        None: no `pde.forcing`, or no step.  Validated on the host, in front of any device work."""
        forcing = self._check_forcing_supported(pde)
        if forcing is None or len(ts) < 2:
            return None
        return np.ascontiguousarray(forcing.table(ts, pde))

    def _operator_table(self, pde, ts):
        """The coefficients of `pde.time_dependent_operator` on the constant schedule `ts` (a runt last step included) as the (T, R)
        table the device takes, or None: no such operator, or no step.  Validated on the host, in front of any device work."""
        operator = self._check_operator_supported(pde)
        if operator is None or len(ts) < 2:
            return None
        return np.ascontiguousarray(operator.table(ts))

    def _constant_schedule(self, pde, num_steps):
        """(times, steps) of the constant-step loop: the t-accumulation of the reference, a runt final step included."""
        return data.constant_schedule(pde.t0, pde.tmax, self.steprule.first_dt(pde), num_steps)

    def _run_device_loop(self, pde, state, ts, dts):
        """The steps `dts` from `state` on the device, runs of equal dt in one call each: the 5-tuple of `solve_marginals`."""
        dev = state.y.device_state
        # re-linearised, or its operator rebuilt, inside the loop: no error model there
        on_device = self._device_filter.reaction is not None or getattr(pde, "time_dependent_operator", None) is not None
        d = pde.L.shape[0]                                      # (the latent-force state carries eps behind u)
        means = [state.y.mean[0][:d]]
        stds = [np.sqrt(np.maximum(state.y.marginal_var[0][:d], 0.0))]
        sig = []
        for count, dt in data.equal_step_runs(dts):             # runs of equal dt -> one device call each
            if not on_device:
                self._ensure_error_model(pde, dt)
            mk, sk, infos = self._device_filter.steps(dev, count, dt)
            means.extend(mk), stds.extend(sk)
            sig.extend(o.diffusion_squared_local for o in infos)
        m_final = dev.mean()
        final = pdefilter.PDEFilterState(t=ts[-1], y=rv.DeviceMultivariateNormal(m_final, dev), error_estimate=None,
                                         reference_state=np.abs(m_final[0][:d]),
                                         diffusion_squared_local=sig[-1] if sig else [])
        return np.array(ts), np.array(means), np.array(stds), np.array(sig), final

    # ------------------------------------------------------------------ the device loop with the trajectory kept
    def solve_on_device(self, pde, *, num_steps=None, observations=None, linearize_at=None):
        """`solve()` of the `Constant` rule through the device-resident loop: a `PDESolution` with the time grid of
        `solve_marginals` (a runt last step included), `mean` (T+1, n, d_state), device-resident states, the calibrated
        diffusion as `solve()` computes it and `info = dict(num_steps)` -- with `observations` (as in `solve_marginals`) also
        `data_log_likelihood` / `data_log_likelihoods`.  `smooth`, `smooth_marginals`, `sample`, `sample_dense`, `solution(t)` and
        `state_at` work on it as on a `solve()` result.

        The loop records the state behind every step into one device state per grid time (`pnmol_filter_set_recorder`, DESIGN.md
        section 20): no host round trip per step, one read-back of all means per run of equal steps.  It accepts what
        `solve_marginals` accepts (linear problems, problems whose term the device linearises, one sensor array) in the fp64
        covariance form; memory: T + 1 states of (n d)^2 doubles on the device.  linearize_at: as in `solve_marginals`."""
        if not isinstance(self.steprule, _step.Constant):
            raise TypeError("solve_on_device needs the Constant step rule")
        self._check_forcing_supported(pde)
        if not self._is_fp64_covariance_form():
            raise TypeError(f"solve_on_device() supports the fp64 covariance-form solvers of pnmol.white and pnmol.latent; "
                            f"{type(self).__module__}.{type(self).__name__} with dtype={self.dtype!r} is not one")
        plan = self._loop_plan(pde, num_steps, observations, linearize_at)
        state, lls = self._observe_at_t0(self.initialize(pde), plan)
        flt = self._device_filter
        first = state.y
        slots = [flt.new_state() for _ in plan.dts]             # one per step: the recorder fills them
        with self._loop_options(flt, plan, slots) as installed:
            # (the loop advances its state in place: it works on a copy, the initial state stays what `ys[0]` holds)
            work = state._replace(y=rv.DeviceMultivariateNormal(first.mean, first.device_state.clone()))
            _, _, _, sig, _ = self._run_device_loop(pde, work, plan.ts, plan.dts)
            lls = self._loop_consumed(flt, plan, installed, lls)
            # one read-back for all states
            means = flt.recorder_means(0, len(slots)) if slots else np.zeros((0,) + first.mean.shape)
        states = [first] + [rv.DeviceMultivariateNormal(m, s) for m, s in zip(means, slots)]
        info = dict(num_steps=len(plan.dts))
        if observations is not None:
            info.update(data_log_likelihood=float(sum(lls)), data_log_likelihoods=lls)
        return pdefilter.PDESolution(t=np.array(plan.ts), mean=np.stack([y.mean for y in states]), ys=states, info=info,
                                     diffusion_squared_calibrated=np.mean(np.array(sig)))

    def smooth_marginals(self, solution):
        """(means (T+1, d), stds (T+1, d)): the read-out of `smooth(solution, dense=None)` -- smoothed mean and marginal std of
        the PDE solution per grid time, uncalibrated -- through one `pnmol_smoother_steps` call: the whole backward pass enqueued
        at once, one synchronisation, no smoothed state kept (two internal ones rotate).  `solution`: a `solve()` or
        `solve_on_device()` result, unchanged.  Supported: what `smooth` supports."""
        ys, flt = self._walk_inputs("smooth_marginals", solution)
        t = np.asarray(solution.t, dtype=np.float64)
        if len(ys) < 2:
            y = ys[0]
            return y.mean[:1, :flt.d].copy(), np.sqrt(np.maximum(y.marginal_var[:1, :flt.d], 0.0))
        return flt.smoother_steps([y.device_state for y in ys], np.diff(t))

    # ------------------------------------------------------------------ iterated smoother
    def solve_iterated(self, pde, *, iterations=10, tol=1e-9, num_steps=None, observations=None, relaxation=1.0, start=None,
                       smooth="marginal"):
        """Iterated extended Kalman smoother (IEKS; beyond the reference): forward and backward passes repeated, every step of a
        forward pass linearised at the previous pass's SMOOTHED mean, until the trajectory stops moving.  The fixed point is the
        MAP trajectory under prior, PDE residuals and sensor data (Gauss-Newton on that objective).

        Pass 0 is `solve_on_device(pde)` -- the EK1, linearised at the predicted means -- or, with `start` (T, d),
        `solve_on_device(pde, linearize_at=start)`.  Behind every pass `smooth_marginals` gives the smoothed means `ms` (T+1, d),
        and the next pass linearises at u <- u + relaxation (ms[1:] - u), u being `start` or, without one, `ms[1:]` of pass 0.  The
        increment of a pass is max|ms_new - ms_old| / max|ms_new|; the loop ends when it is <= tol, or after `iterations` passes
        beyond pass 0.  Every pass starts from `initialize(pde)`'s state, whose update on the PDE residual at t0 keeps its own
        linearisation (at the prior mean conditioned on y0): the initial state is not iterated.

        Returns an `IteratedSolution`: `filtered` (the last pass's `PDESolution`: `smooth`, `sample`, `sample_dense` and
        `solution(t)` work on it), `means` / `stds` (T+1, d) smoothed, `smoothed` (`smooth(filtered, dense=smooth)`, or None
        for smooth=None), `increments`, `num_iterations`, `converged`, and with observations `data_log_likelihood(s)` of the last
        pass.  One forward solution is alive at a time: memory is that of `solve_on_device`.  Supported: `SemiLinearWhiteNoiseEK1`
        in the fp64 covariance form with a term the device linearises, `Constant` steps."""
        from . import latent

        if not isinstance(self.steprule, _step.Constant):
            raise TypeError("solve_iterated needs the Constant step rule")
        self._check_forcing_supported(pde)
        if (not isinstance(self, SemiLinearWhiteNoiseEK1) or isinstance(self, latent._LatentForceEK1Base)
                or not self._is_fp64_covariance_form() or self._reaction_for_device(pde) is None):
            raise TypeError(f"solve_iterated() supports pnmol.white.SemiLinearWhiteNoiseEK1 in the fp64 covariance form on a problem "
                            f"whose term the device linearises (`pde.reaction`, reaction_on_device=True); "
                            f"{type(self).__module__}.{type(self).__name__} with dtype={self.dtype!r} on this problem is not that")
        if smooth not in (None, "marginal", "full"):
            raise ValueError(f'solve_iterated(): smooth must be None, "marginal" or "full", got {smooth!r}')
        if int(iterations) < 0 or not tol >= 0.0 or not 0.0 < relaxation <= 1.0:
            raise ValueError("solve_iterated(): needs iterations >= 0, tol >= 0 and 0 < relaxation <= 1")
        _, dts = self._constant_schedule(pde, num_steps)
        points = self._checked_linearization_points(pde, start, len(dts))
        kw = dict(num_steps=num_steps, observations=observations)
        sol = self.solve_on_device(pde, linearize_at=points, **kw)
        ms, sd = self.smooth_marginals(sol)
        if points is None:
            points = ms[1:].copy()
        increments = []
        converged = not dts                                     # (no step: nothing to iterate)
        while not converged and len(increments) < int(iterations):
            points = points + relaxation * (ms[1:] - points)
            del sol                                             # (the states of the pass before: one forward solution at a time)
            sol = self.solve_on_device(pde, linearize_at=points, **kw)
            ms_new, sd = self.smooth_marginals(sol)
            increments.append(float(np.abs(ms_new - ms).max() / np.abs(ms_new).max()))
            ms = ms_new
            converged = increments[-1] <= tol
        smoothed = None if smooth is None else self.smooth(sol, dense=smooth)
        return IteratedSolution(filtered=sol, means=ms, stds=sd, smoothed=smoothed, increments=increments,
                                num_iterations=len(increments), converged=converged,
                                data_log_likelihood=sol.info.get("data_log_likelihood"),
                                data_log_likelihoods=sol.info.get("data_log_likelihoods"))

    # ------------------------------------------------------------------ backward walks (smoothing, joint draws)
    def _walk_inputs(self, who, solution):
        """What `smooth`, `sample` and `sample_dense` walk backwards: (the device-resident states of `solution`, the one filter
        that owns them).  Refuses every solver but the fp64 covariance-form ones of pnmol.white."""
        from . import latent

        if isinstance(self, latent._LatentForceEK1Base) or not self._is_fp64_covariance_form():
            raise TypeError(f"{who}() supports the fp64 white-noise solvers of pnmol.white (covariance form); "
                            f"{type(self).__module__}.{type(self).__name__} with dtype={self.dtype!r} is not one")
        ys = list(solution._ys)
        if not ys or not all(isinstance(y, rv.DeviceMultivariateNormal) for y in ys):
            raise TypeError(f"{who}() needs the device-resident states of this package's solve()")
        flt = ys[-1].device_state.filter
        if any(y.device_state.filter is not flt for y in ys):
            raise ValueError(f"{who}(): the states of the solution belong to different device filters")
        return ys, flt

    # ------------------------------------------------------------------ smoothing
    def smooth(self, solution, dense="marginal"):
        """Rauch-Tung-Striebel smoothing of a `solve()` result (kalman.py:33-46 of the reference, covariance form).

        Walks `solution`'s device-resident states backwards, one `pnmol_smoother_step` per step, with the filter that owns
        them (a later `solve()` / re-bind of this solver does not matter).  The backward pass uses the prior alone (the
        linearisation of a semilinear solver enters only through the filtered states).  Returns a `PDESolution` with the
        same `t`, `info` and `diffusion_squared_calibrated`, the smoothed `mean` and device-resident states, so
        `marginal_std` and `cov_sqrtm` work as for the filter -- and, like them, uncalibrated.  `solution` is unchanged.
        dense: what the result keeps for evaluation BETWEEN grid times (`result(t)`, `result.state_at(t)`).
        "marginal" (default): one bridge per step, ~3 n^2 d doubles and one tiny launch each -- means and marginal stds at any t;
        the smoothed states are bit for bit those of dense=None.  "full": the bridges also keep the lag-one cross-covariance
        C_k, T (n d)^2 more doubles on the device in all (as much as the states themselves), for `state_at`.  None: nothing.
        Supported: fp64 white-noise solvers (pnmol.white), constant and adaptive steps."""
        if dense not in (None, "marginal", "full"):
            raise ValueError(f'smooth(): dense must be None, "marginal" or "full", got {dense!r}')
        ys, flt = self._walk_inputs("smooth", solution)
        t = np.asarray(solution.t)
        nxt = ys[-1].device_state.clone()                       # terminal state: the filtered one
        out = [rv.DeviceMultivariateNormal(np.array(ys[-1].mean), nxt)]
        bridges = None if dense is None else []
        for k in range(len(ys) - 2, -1, -1):
            if dense is None:
                nxt = flt.smoother_step(ys[k].device_state, nxt, t[k + 1] - t[k])
            else:
                nxt, br = flt.smoother_step(ys[k].device_state, nxt, t[k + 1] - t[k], bridge=dense)
                bridges.append(br)
            out.append(rv.DeviceMultivariateNormal(nxt.mean(), nxt))
        out.reverse()
        if bridges is not None:
            bridges.reverse()
        return pdefilter.PDESolution(t=solution.t, mean=np.stack([y.mean for y in out]), ys=out, info=solution.info,
                                     diffusion_squared_calibrated=solution.diffusion_squared_calibrated, bridges=bridges,
                                     smoothed=True)

    # ------------------------------------------------------------------ functionals of the trajectory
    def functionals(self, solution, weights, *, calibrated=False):
        """The exact smoothing posterior of linear functionals q = sum_k weights[:, k] . x_k of the whole trajectory of a
        `solve()` or `solve_on_device()` result: time integrals, space-time means, differences across times (builders:
        `pnmol.functionals`).  weights: (Q, T+1, d) on the PDE solution at the T+1 grid times, or (Q, T+1, n, d) on all
        derivatives, raw coordinates; Q <= 64.  Returns a `pnmol.functionals.FunctionalPosterior` (`mean` (Q,), `cov` (Q, Q),
        `std`), uncalibrated like `smooth`; calibrated=True scales `cov` by `solution.diffusion_squared_calibrated`.

        One `pnmol_functionals` call on the filter that owns `solution`'s device-resident states: only the filtered states enter
        (the adjoint of the recursion behind `smooth`, in ascending time), nothing is smoothed, drawn or
        read back but the result.  `solution` is unchanged.  Supported: what `smooth` supports."""
        from . import functionals as _fn

        ys, flt = self._walk_inputs("functionals", solution)
        w = _fn.checked_weights(weights, len(ys) - 1, flt.n, flt.d)
        mean, cov = flt.functionals([y.device_state for y in ys], np.diff(np.asarray(solution.t, dtype=np.float64)), w)
        if calibrated:
            cov = cov * solution.diffusion_squared_calibrated
        return _fn.FunctionalPosterior(mean=mean, cov=cov)

    # ------------------------------------------------------------------ joint draws
    def sample(self, solution, num_samples, *, seed=0, noise=None, calibrated=False):
        """Joint draws of whole trajectories from the smoothing posterior of a `solve()` result.

        Walks `solution`'s device-resident filtered states backwards, one `pnmol_samples_step_back` per step, with the
        filter that owns them (a later `solve()` / re-bind of this solver does not matter): x_T ~ N(m_T, P_T), then
        x_k | x_{k+1} by the backward recursion behind `smooth` (prior alone; include/pnmol_hip.h, "Joint draws").  Returns an
        array (num_samples, T+1, n, d) in raw coordinates; `[:, :, 0]` are draws of the PDE solution.  The marginals of the
        draws are those of `smooth(solution)`; what the draws add is the coupling across time.

        noise: None (generated on the device from `seed`, step k using `step_index = k`), or a sequence of T+1 arrays of
        standard normals, `noise[k]` of shape (S, 2D) for k < T and (S, D) for k = T (D = n d).  calibrated=True draws from
        the calibrated posterior (noise scale sqrt(solution.diffusion_squared_calibrated)).  `solution` is unchanged.
        Supported: fp64 white-noise solvers (pnmol.white), constant and adaptive steps."""
        return self._sample_walk("sample", solution, num_samples, seed, noise, calibrated)[0]

    def sample_dense(self, solution, num_samples, ts, *, seed=0, noise=None, noise_dense=None, calibrated=False):
        """Joint draws of whole trajectories at the grid times AND at the times `ts` (1-d, any order, >= solution.t[0]).

        Returns (grid_draws (S, T+1, n, d), dense_draws (S, len(ts), n, d)), raw coordinates.  `grid_draws` is bit for bit
        `sample(solution, num_samples, seed=seed, noise=noise, calibrated=calibrated)`.  Given the draws at the two grid times
        around it, a time inside a step follows the prior's bridge (no measurement in between), so it is drawn by
        `pnmol_samples_interpolate` from the two neighbouring blocks alone; several times inside one step are drawn one after the
        other, each between its nearest drawn neighbours, and times beyond the last grid time forwards, each from its
        predecessor.  A time equal to a grid time returns that grid time's draws.  The inserted time `ts[q]` uses
        `step_index = T + 1 + q` of the device generator, or `noise_dense[q]` (S, D) when host noise is given (`noise` and
        `noise_dense` together, or neither).  `solution` (a `solve()` result, as for `sample`) is unchanged."""
        ts = np.atleast_1d(np.asarray(ts, dtype=np.float64))
        if ts.ndim != 1:
            raise ValueError(f"sample_dense(): ts must be 1-d, got shape {ts.shape}")
        if ts.size and (not np.all(np.isfinite(ts)) or np.any(ts < np.asarray(solution.t)[0])):
            raise ValueError("sample_dense(): times must be finite and >= solution.t[0]")
        if (noise is None) != (noise_dense is None):
            raise ValueError("sample_dense(): give noise and noise_dense together (host noise for every input) or neither")
        if noise_dense is not None and len(noise_dense) != ts.size:
            raise ValueError(f"sample_dense(): noise_dense must have one entry per time in ts ({ts.size}), got {len(noise_dense)}")
        return self._sample_walk("sample_dense", solution, num_samples, seed, noise, calibrated, ts, noise_dense)

    def _sample_walk(self, who, solution, num_samples, seed, noise, calibrated, ts=None, noise_dense=None):
        ys, flt = self._walk_inputs(who, solution)
        S, T = int(num_samples), len(ys) - 1
        if S < 1:
            raise ValueError(f"{who}(): num_samples must be at least 1, got {num_samples}")
        if noise is not None and len(noise) != T + 1:
            raise ValueError(f"{who}(): noise must have one entry per time point ({T + 1}), got {len(noise)}")
        scale = float(np.sqrt(solution.diffusion_squared_calibrated)) if calibrated else 1.0
        t = np.asarray(solution.t)
        xi = (lambda k: None) if noise is None else (lambda k: noise[k])
        block = flt.new_samples(S)
        out = np.empty((S, T + 1, flt.n, flt.d))
        # the inserted times, per grid interval (index T: beyond the last grid time), ascending inside each
        nq = 0 if ts is None else ts.size
        dense = np.empty((S, nq, flt.n, flt.d))
        where = np.searchsorted(t, ts, side="right") - 1 if nq else np.zeros(0, dtype=int)
        on_grid = t[where] == ts if nq else np.zeros(0, dtype=bool)
        todo = {}
        for q in np.argsort(ts, kind="stable") if nq else ():
            if not on_grid[q]:
                todo.setdefault(int(where[q]), []).append(int(q))
        spare = [flt.new_samples(S), flt.new_samples(S)] if todo else None

        def insert(k, left, right):
            drawn = 0                                           # blocks alternate by the draws made: `left` is never `cur`
            for i, q in enumerate(todo[k]):
                if i and ts[q] == ts[todo[k][i - 1]]:           # the same time twice: the same draws
                    dense[:, q] = dense[:, todo[k][i - 1]]
                    continue
                cur = spare[drawn % 2]
                drawn += 1
                cur.interpolate(left, right, ts[q], None if noise_dense is None else noise_dense[q], seed=seed,
                                step_index=T + 1 + q, scale=scale)
                dense[:, q] = cur.get()
                left = cur

        block.draw(ys[-1].device_state, xi(T), seed=seed, step_index=T, scale=scale)
        out[:, T] = block.get()
        if T in todo:
            insert(T, block, None)
        for k in range(T - 1, -1, -1):
            right = block.clone() if k in todo else None        # (step_back works in place)
            block.step_back(ys[k].device_state, t[k + 1] - t[k], xi(k), seed=seed, step_index=k, scale=scale)
            out[:, k] = block.get()
            if k in todo:
                insert(k, block, right)
        for q in np.flatnonzero(on_grid):
            dense[:, q] = out[:, where[q]]
        return out, dense


class LinearWhiteNoiseEK1(_WhiteNoiseEK1Base):
    """EK1 for linear PDEs u_t = L u (white.py:169-186): H = [E1 - L E0 ; B E0], no shift.  A problem with
    `pde.time_dependent_operator` (pde/coefficients.py): L is M(t)."""

    @staticmethod
    def _linearize(pde, m_at, t):
        operator = getattr(pde, "time_dependent_operator", None)
        return (pde.L if operator is None else operator.matrix(t)), np.zeros(pde.L.shape[0])


class SemiLinearWhiteNoiseEK1(_WhiteNoiseEK1Base):
    """EK1 for semilinear PDEs u_t = L u + f(t, u) (white.py:189-208): H = [E1 - (J_x + L) E0 ; B E0] and
    z = H m + [J_x m_at - f(t, m_at); 0], re-linearised at the predicted mean of every step."""

    semilinear = True

    @staticmethod
    def _linearize(pde, m_at, t):
        from .pde.reactions import Convection

        term = getattr(pde, "reaction", None)
        if isinstance(term, Convection) and pde.L.shape[0] == pde.L.shape[1]:
            # the structured host form (operator entries and shift in the device's order of operations, no dense J_x @ m):
            # the host route and the device route then produce the same operator and shift
            M, shift = term.linearization(m_at, L=pde.L)
            forcing = getattr(pde, "forcing", None)             # (every other branch reads the source through `pde.f`)
            if forcing is not None:
                shift = shift - forcing.source_values(t, pde)
            return M, shift
        fx = np.asarray(pde.f(t, m_at), dtype=np.float64)
        Jx = np.asarray(pde.df(t, m_at), dtype=np.float64)
        operator = getattr(pde, "time_dependent_operator", None)
        return (pde.L if operator is None else operator.matrix(t)) + Jx, Jx @ m_at - fx

    @staticmethod
    def _jacobian_diagonal(pde, m_at, t):
        """diag(J_x) where the problem says its Jacobian is diagonal (`df_diagonal`, pde/problems.py:11-42), else None."""
        dfd = getattr(pde, "df_diagonal", None)
        if dfd is None or pde.L.shape[0] != pde.L.shape[1]:
            return None
        return np.asarray(dfd(t, m_at), dtype=np.float64)

    # A problem with a `reaction` attribute (pde/reactions.py, a scalar `Reaction`, a coupled `SystemReaction` or a `Convection`
    # term; `pde.examples.reaction_diffusion_1d_discretized`, `reaction_diffusion_system_1d_discretized`,
    # `convection_diffusion_1d_discretized`) is linearised on
    # the device: `attempt_step` takes no host round trip and `solve_marginals` runs.  False: the host callables, as for
    # every other semilinear problem.  fp64 covariance-form white-noise solvers only; the others use the callables.
    reaction_on_device = True

    def _reaction_for_device(self, pde):
        reaction = getattr(pde, "reaction", None)
        if reaction is None or not self.reaction_on_device or not self._is_fp64_covariance_form():
            return None
        return reaction

    def solve_marginals(self, pde, *, num_steps=None, observations=None, linearize_at=None):
        self._check_forcing_supported(pde)
        if self._reaction_for_device(pde) is None:
            raise TypeError("solve_marginals keeps the loop on the device and needs a linear PDE; use solve()")
        return super().solve_marginals(pde, num_steps=num_steps, observations=observations, linearize_at=linearize_at)

    def solve_on_device(self, pde, *, num_steps=None, observations=None, linearize_at=None):
        self._check_forcing_supported(pde)
        if self._reaction_for_device(pde) is None:
            raise TypeError("solve_on_device keeps the loop on the device and needs a linear PDE; use solve()")
        return super().solve_on_device(pde, num_steps=num_steps, observations=observations, linearize_at=linearize_at)
