"""Dense fp64 NumPy reference of the iterated EK1 smoother (`solve_iterated`, `pnmol_filter_set_linearization_points`): the oracle's
own `WhiteNoiseEK1` steps with `evaluate_ode` linearised at an injected point per step, `smooth_reference.rts_on_oracle` behind
every forward pass, and `observe_reference.drive` for the loop (so sensor data enters by the oracle's `update_sqrt`).

The cases of tests/test_iterated_host.py and tests/test_gpu_iterated.py, fixed here.  13 steps (the device loop then takes its
first step eagerly, one 10-step graph and one 2-step graph); K = 13.3 adds a runt 14th step.  The step size and the coefficients
are chosen so that, on this reference alone, the iteration (1) converges to an increment <= 1e-9 within 10 iterations, (2) moves the
EK1 result by a first increment >= 1e-4, well above the 1e-5 mean tolerance of the parity tests, and (3) reaches the same fixed point
from the start `y0` repeated -- tests/test_iterated_host.py asserts the three on the CPU.  A mild term at a small step fails (2): the
EK1 smoother is then already the fixed point to 1e-5."""

import functools
from collections import namedtuple

import numpy as np
import scipy.linalg

import pnmol
import pnmol_oracle as oracle
import observe_reference as oref
from pnmol.pde import examples, reactions
from smooth_reference import marginal_std, rts_on_oracle

ITERATIONS, TOL = 10, 1e-9

# coef is the Fisher-KPP rate r in r u (1 - u), the Allen-Cahn scale s in s (u - u^3), the Burgers speed c in
# u_t = 0.02 u_xx - c u u_x, or the Lotka-Volterra coefficients (a, b, c, d), which keep the recipe's initial values.
# Initial values: 0.5 + 0.4 cos(pi x) (Neumann), 0.8 sin(pi x) (Dirichlet), sin(pi x) (Burgers).
#
# What the reference alone gives with these values (first increment, iterations until the increment is <= 1e-9):
#   fisher-neumann         7.3e-4, 4        burgers          2.7e-4, 4
#   fisher-dirichlet-runt  8.4e-4, 5        lotka-volterra   1.9e-4, 3
#   allen-cahn             1.6e-3, 5        fisher-nu1       1.6e-3, 5
#   fisher-264             2.6e-4, 4  (rate 8 and not 10: a pass of the reference takes ~9 s at N = 264, so fewer of them)
# A step twice as long or a term twice as strong leaves the region in which the iteration contracts fast: Allen-Cahn with
# s = 6 at dt = 2^-4 oscillates between two trajectories.  Half of either brings the first increment under 1e-4.
Case = namedtuple("Case", "kind N nu bcond K dt coef")
CASES = {
    "fisher-neumann": Case("fisher", 33, 2, "neumann", 13, 2.0 ** -4, 10.0),
    "fisher-dirichlet-runt": Case("fisher", 33, 2, "dirichlet", 13.3, 2.0 ** -5, 6.0),
    "allen-cahn": Case("allen_cahn", 33, 2, "dirichlet", 13, 2.0 ** -5, 6.0),
    "burgers": Case("burgers", 33, 2, "dirichlet", 13, 2.0 ** -6, 1.0),
    "lotka-volterra": Case("lotka_volterra", 33, 2, "neumann", 13, 2.0 ** -4, (0.5, 0.4, 0.4, 0.5)),
    "fisher-nu1": Case("fisher", 33, 1, "dirichlet", 13, 2.0 ** -5, 6.0),
    "fisher-264": Case("fisher", 264, 2, "neumann", 13, 2.0 ** -4, 8.0),
}
KAPPA, KAPPA_BURGERS = 0.05, 0.02


def _y0(case):
    if case.kind == "burgers":
        return lambda x: np.sin(np.pi * x)
    if case.bcond == "neumann":
        return lambda x: 0.5 + 0.4 * np.cos(np.pi * x)
    return lambda x: 0.8 * np.sin(np.pi * x)


def _kw(case):
    return dict(tmax=case.K * case.dt, dx=1.0 / (case.N - 1), bcond=case.bcond, stencil_size_interior=3,
                stencil_size_boundary=3, y0_fun=_y0(case))


def product(name, **attrs):
    """(pde, solver) of the product for a case."""
    case = CASES[name]
    dt = case.dt
    kernel = pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise()
    if case.kind == "lotka_volterra":
        pde = examples.reaction_diffusion_system_1d_discretized(reactions.lotka_volterra(*case.coef), diffusion_rates=(0.1, 0.1),
                                                                y0_fun=examples.lotka_volterra_y0, dx=1.0 / (case.N - 1),
                                                                tmax=case.K * dt)
        kernel = pnmol.kernels.duplicate(kernel, num=2)
    elif case.kind == "burgers":
        pde = examples.convection_diffusion_1d_discretized(reactions.Convection((0.0, -case.coef)), diffusion_rate=KAPPA_BURGERS,
                                                           kernel=pnmol.kernels.SquareExponential(), nugget_gram_matrix_fd=0.0,
                                                           **_kw(case))
    else:
        term = (reactions.logistic(case.coef) if case.kind == "fisher"
                else reactions.Reaction(p=(0.0, case.coef, 0.0, -case.coef)))
        pde = examples.reaction_diffusion_1d_discretized(term, diffusion_rate=KAPPA, kernel=pnmol.kernels.SquareExponential(),
                                                         nugget_gram_matrix_fd=0.0, **_kw(case))
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=case.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                 spatial_kernel=kernel)
    for key, value in attrs.items():
        setattr(solver, key, value)
    return pde, solver


class PointwiseEK1(oracle.WhiteNoiseEK1):
    """The oracle's semilinear EK1 whose `evaluate_ode` takes m_at from an injected point when one is set: `points[k]` for the
    k-th step attempted since `set_points` (constant steps: one attempt per step).  `initialize` never sees a point."""

    points = None
    _taken = 0
    _point = None

    def set_points(self, points):
        self.points, self._taken = (None if points is None else np.asarray(points, dtype=np.float64)), 0

    def evaluate_ode(self, pde, p0, p1, m_pred, t):
        if self._point is None:
            return super().evaluate_ode(pde, p0, p1, m_pred, t)
        m_at = self._point                                      # (white.py:192-208 with m_at replaced)
        fx, Jx = pde.f(t, m_at), pde.df(t, m_at)
        H = np.vstack((p1 - Jx @ p0 - pde.L @ p0, pde.B @ p0))
        z = H @ m_pred + np.hstack((Jx @ m_at - fx, np.zeros(pde.B.shape[0])))
        return z, H, scipy.linalg.block_diag(pde.E_sqrtm, pde.R_sqrtm)

    def attempt_step(self, state, dt, pde):
        if self.points is not None:
            self._point = self.points[self._taken]
            self._taken += 1
        try:
            return super().attempt_step(state, dt, pde)
        finally:
            self._point = None


def oracle_side(name):
    """(opde, osolver) of the oracle for a case."""
    case = CASES[name]
    dt, coef = case.dt, case.coef
    kernel = oracle.Matern52() + oracle.WhiteNoise()
    if case.kind == "lotka_volterra":
        opde = oracle.lotka_volterra_1d_discretized(dx=1.0 / (case.N - 1), tmax=case.K * dt, **dict(zip("abcd", coef)))
        kernel = oracle.duplicate(kernel, 2)
    elif case.kind == "burgers":
        import convection_reference as cref

        opde = oracle.heat_1d_discretized(kernel=oracle.SquareExponential(), diffusion_rate=KAPPA_BURGERS, **_kw(case))
        G, _ = cref.oracle_gradient(opde.mesh_spatial, oracle.SquareExponential(), 3)
        opde.f = lambda _t, u: -coef * u * (G @ u)
        opde.df = lambda _t, u: -coef * (np.diag(G @ u) + u[:, None] * G)
    else:
        opde = oracle.heat_1d_discretized(kernel=oracle.SquareExponential(), diffusion_rate=KAPPA, **_kw(case))
        if case.kind == "fisher":
            opde.f = lambda _t, x: coef * x * (1.0 - x)
            opde.df = lambda _t, x: np.diag(coef * (1.0 - 2.0 * x))
        else:
            opde.f = lambda _t, x: coef * (x - x ** 3)
            opde.df = lambda _t, x: np.diag(coef * (1.0 - 3.0 * x ** 2))
    osolver = PointwiseEK1(num_derivatives=case.nu, steprule=oracle.Constant(dt), semilinear=True, canonical_factor_signs=True,
                           spatial_kernel=kernel)
    return opde, osolver


Pass = namedtuple("Pass", "solution means stds smoothed_means smoothed_stds")
Iterated = namedtuple("Iterated", "means stds increments num_iterations converged points passes last")


def forward_backward(osolver, opde, points, observations=()):
    """One pass: the filter linearised at `points` (None: the EK1), with the updates of `observations`, then the RTS pass."""
    osolver.set_points(points)
    try:
        sol, _ = oref.drive(osolver, opde, list(observations))
    finally:
        osolver.set_points(None)
    means, stds = oracle.read_mean_and_std(sol, osolver.E0)
    ms, Ps = rts_on_oracle(osolver, sol)
    n, d = sol.mean.shape[1:]
    return Pass(sol, means, stds, ms[:, 0], marginal_std(Ps, n, d)[:, 0])


def iterate(osolver, opde, iterations=ITERATIONS, tol=TOL, start=None, observations=(), relaxation=1.0):
    """The iteration of `solve_iterated` on the oracle.  `points[i]`: the table pass i was linearised at (None: the EK1 pass);
    `passes` keeps pass 0 and pass 1 (what the one-pass tests compare against), `last` the final pass."""
    points = [None if start is None else np.asarray(start, dtype=np.float64)]
    cur = forward_backward(osolver, opde, points[0], observations)
    passes = [cur]
    ms = cur.smoothed_means
    u = ms[1:].copy() if start is None else points[0]
    increments = []
    converged = False
    while not converged and len(increments) < iterations:
        u = u + relaxation * (ms[1:] - u)
        points.append(u)
        cur = forward_backward(osolver, opde, u, observations)
        if len(passes) < 2:
            passes.append(cur)
        increments.append(float(np.abs(cur.smoothed_means - ms).max() / np.abs(cur.smoothed_means).max()))
        ms = cur.smoothed_means
        converged = increments[-1] <= tol
    return Iterated(ms, cur.smoothed_stds, increments, len(increments), converged, points, passes, cur)


def sensor_setup(name, q=8):
    """Three readings of q sensors for a case: at t0, behind step 6 and on the last step; 1.05 x the EK1 reference's own filtering
    mean plus noise of the size of its median interior std, so that the data moves the means and the innovations stay well
    conditioned.  Returns the `pnmol.data.Observation`s."""
    case = CASES[name]
    ek1 = reference(name).passes[0]
    d = ek1.means.shape[1]
    C = oref.sensor_matrix(d, q)
    noise = float(np.median(ek1.stds[1:, 1:-1]))
    rng = np.random.default_rng(case.N + q)
    t = ek1.solution.t
    return [pnmol.data.Observation(t[j], C, 1.05 * (C @ ek1.means[j]) + noise * rng.standard_normal(q), noise)
            for j in (0, 6, len(t) - 1)]


@functools.lru_cache(maxsize=None)
def reference(name, start_y0=False, observed=False):
    """The reference iteration of a case, computed once per process and shared (nothing modifies it).  start_y0: from `y0`
    repeated T times; observed: with the readings of `sensor_setup`."""
    opde, osolver = oracle_side(name)
    obs = tuple(sensor_setup(name)) if observed else ()
    start = None
    if start_y0:
        T = int(np.ceil(CASES[name].K))
        start = np.tile(opde.y0, (T, 1))
    return iterate(osolver, opde, start=start, observations=obs)
