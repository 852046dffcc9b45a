"""Dense fp64 NumPy reference of time-dependent operators (`pnmol.pde.coefficients`, `pnmol_filter_set_operator_family`,
`_set_operator_schedule`, `_operator_at`): u_t = sum_r a_r(t) L_r u.

The reference is the oracle's own semilinear path: `f(t, x) = (M(t) - L0) x`, `df(t, x) = M(t) - L0` with L0 the oracle problem's
own L, so that the oracle linearises with J_x + L0 = M(t) and a shift (M - L0) m - (M - L0) m = 0.  The noise of the PDE rows is the
operator's: the oracle reads `pde.E_sqrtm` behind its call of `pde.f(t, .)` (evaluate_ode), so a small wrapper whose `f` remembers t
and whose `E_sqrtm` property answers for that t gives E(t0) to `initialize` and E(t + dt) to every `attempt_step`, constant and
adaptive alike.

The cases of tests/test_operator_host.py and tests/test_gpu_operator.py, fixed here.  Family (A): kappa(t) u_xx with
kappa(t) = 0.05 (1 + 0.8 sin(2 pi t / (K dt))) on the heat problem of helpers.make_pair, dt = 2^-6.  Family (B): 0.05 u_xx -
c(t) u_x with a 5-point gradient and c(t) = C_MAX sin(2 pi t / (K dt)): the union image is wider than the creation-time one, the
coefficient is zero at t0 and changes sign.  tests/test_operator_host.py establishes on the oracle alone that both are finite and
move the read-outs by at least 100 times the tolerances of the GPU tests."""

import functools

import numpy as np

import pnmol
import pnmol_oracle as oracle
from pnmol.pde import examples, reactions

DT = 2.0 ** -6
KAPPA, AMP = 0.05, 0.8
C_MAX = 1.0                          # velocity amplitude of family (B); see test_operator_host.py for what it moves
# (N, nu, bcond, K): mp = 32, one block, padded rows; 31 padded points, mp = 64; m = 257 in mp = 288 (the second block of the
# 256-thread launch holds one boundary row and padding); the n = 4 instantiations
SHAPES = [(24, 2, "neumann", 12), (33, 1, "dirichlet", 12), (255, 1, "dirichlet", 4), (40, 3, "dirichlet", 8)]
SHAPES_B = SHAPES[:2]
MEAN_RTOL, STD_RTOL = 1e-5, 1e-4     # helpers.assert_mean_std_parity


def kappa_of(K, dt=DT, amp=AMP):
    return lambda t: KAPPA * (1.0 + amp * np.sin(2.0 * np.pi * t / (K * dt)))


def velocity_of(K, dt=DT, c_max=C_MAX):
    return lambda t: c_max * np.sin(2.0 * np.pi * t / (K * dt))


def _kw(N, K, dt, bcond):
    return dict(tmax=K * dt, dx=1.0 / (N - 1), bcond=bcond, stencil_size_interior=3, stencil_size_boundary=3,
                nugget_gram_matrix_fd=0.0)


class TimeVaryingOraclePde:
    """An oracle problem whose operator and PDE-row noise follow a `TimeDependentOperator`: everything else is `opde`'s.
    extra_f / extra_df: a further term (a reaction, a source)."""

    def __init__(self, opde, operator, extra_f=None, extra_df=None):
        self._opde, self._op, self._t = opde, operator, opde.t0
        self._extra_f, self._extra_df = extra_f, extra_df
        self.L = np.array(opde.L)

    def __getattr__(self, name):
        return getattr(self._opde, name)

    def f(self, t, x):
        self._t = t
        out = (self._op.matrix(t) - self.L) @ x
        return out if self._extra_f is None else out + self._extra_f(t, x)

    def df(self, t, x):
        out = self._op.matrix(t) - self.L
        return out if self._extra_df is None else out + self._extra_df(t, x)

    @property
    def E_sqrtm(self):
        return self._op.noise_sqrtm(self._t)


def make_solver(nu, steprule, semilinear=False):
    cls = pnmol.white.SemiLinearWhiteNoiseEK1 if semilinear else pnmol.white.LinearWhiteNoiseEK1
    return cls(num_derivatives=nu, steprule=steprule, spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())


def make_osolver(nu, osteprule, cls=oracle.WhiteNoiseEK1):
    return cls(num_derivatives=nu, steprule=osteprule, semilinear=True, canonical_factor_signs=True,
               spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())


def problem(family, N, K, bcond, dt=DT, reaction=None, forcing=None, constant=False, gradient_stencil_size=5):
    """The product's problem of a family ("A" / "B").  constant: the coefficients frozen at those of t0 -- a(t) = 1 for (A),
    c(t) = 0 for (B) --, still posed as a time-dependent operator."""
    kw = dict(kernel=pnmol.kernels.SquareExponential(), reaction=reaction, forcing=forcing, **_kw(N, K, dt, bcond))
    if family == "A":
        kappa = (lambda t: KAPPA) if constant else kappa_of(K, dt)
        return examples.heat_1d_time_varying_discretized(diffusion_rate=kappa, **kw)
    velocity = (lambda t: 0.0) if constant else velocity_of(K, dt)
    return examples.advection_diffusion_1d_discretized(KAPPA, velocity=velocity, gradient_stencil_size=gradient_stencil_size, **kw)


def oracle_problem(pde, N, K, bcond, dt=DT, extra_f=None, extra_df=None):
    opde = oracle.heat_1d_discretized(kernel=oracle.SquareExponential(), diffusion_rate=KAPPA, **_kw(N, K, dt, bcond))
    return TimeVaryingOraclePde(opde, pde.time_dependent_operator, extra_f, extra_df)


def pair(family, N, nu, bcond, K, dt=DT, constant=False):
    """(pde, solver, opde, osolver) of a linear case with the Constant rule."""
    pde = problem(family, N, K, bcond, dt, constant=constant)
    return (pde, make_solver(nu, pnmol.odetools.step.Constant(dt)), oracle_problem(pde, N, K, bcond, dt),
            make_osolver(nu, oracle.Constant(dt)))


def plain_copy(pde):
    """The time-independent problem with the operator and noise of t0: `pde` without its `time_dependent_operator`."""
    import copy

    out = copy.copy(pde)
    del out.time_dependent_operator
    return out


def solve_with_sigmas(osolver, opde):
    """`osolver.solve(opde)` written out (pnmol_oracle.WhiteNoiseEK1.solve), keeping sigma^2 of every step: (Solution, (T,))."""
    ts, means, covs, d2, info = [], [], [], [], {}
    for state, info in osolver.solution_generator(opde):
        ts.append(state.t), means.append(state.y.mean), covs.append(state.y.cov_sqrtm)
        if not isinstance(state.diffusion_squared_local, list):
            d2.append(state.diffusion_squared_local)
    return oracle.Solution(np.stack(ts), np.stack(means), np.stack(covs), info, float(np.mean(np.array(d2)))), np.array(d2)


@functools.lru_cache(maxsize=None)
def _reference(family, N, nu, bcond, K, constant):
    _, _, opde, osolver = pair(family, N, nu, bcond, K, constant=constant)
    sol, sigmas = solve_with_sigmas(osolver, opde)
    return (sol,) + tuple(oracle.read_mean_and_std(sol, osolver.E0)) + (sigmas,)


def reference(family, N, nu, bcond, K, constant=False):
    """(oracle.Solution, means, stds) of a linear case, computed once per process and shared (nothing modifies it)."""
    return _reference(family, N, nu, bcond, K, constant)[:3]


def reference_sigmas(family, N, nu, bcond, K):
    """diffusion_squared_local of every step of `reference`."""
    return _reference(family, N, nu, bcond, K, False)[3]


# ------------------------------------------------------------------------------------------------ composition
LOGISTIC_RATE = 3.0
LOGISTIC = (33, 2, "neumann", 12)


def logistic_pair(forcing=None, osolver_cls=oracle.WhiteNoiseEK1, source=None):
    """Family (A) with the logistic reaction r(u) = 3 u (1 - u) on the device (N = 33); source: what `forcing` adds to f."""
    N, nu, bcond, K = LOGISTIC
    pde = problem("A", N, K, bcond, reaction=reactions.logistic(LOGISTIC_RATE), forcing=forcing)
    X = pde.mesh_spatial.points

    def f(t, x):
        out = LOGISTIC_RATE * x * (1.0 - x)
        return out if source is None else out + source(t, X)

    opde = oracle_problem(pde, N, K, bcond, extra_f=f, extra_df=lambda _t, x: np.diag(LOGISTIC_RATE * (1.0 - 2.0 * x)))
    return (pde, make_solver(nu, pnmol.odetools.step.Constant(DT), semilinear=True), opde,
            make_osolver(nu, oracle.Constant(DT), osolver_cls))


@functools.lru_cache(maxsize=None)
def logistic_reference():
    _, _, opde, osolver = logistic_pair()
    sol = osolver.solve(opde)
    return (sol,) + tuple(oracle.read_mean_and_std(sol, osolver.E0))
