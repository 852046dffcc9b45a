"""Dense fp64 NumPy reference of driven problems (`pnmol.pde.forcing`, `pnmol_filter_set_forcing`, `pnmol_filter_force_at`;
DESIGN.md section 25): u_t = L u + r(u) + s(t, x) with boundary rows B u = g(t).

The source goes into the oracle as the reference itself would take it: `semilinear=True` with `opde.f = f + s` and an unchanged
`df`.  Boundary values are what the reference lacks: the oracle's solvers are subclassed HERE, in the test tree, and their
`evaluate_ode` takes g(t) off the boundary rows of z -- nothing else changes.

The cases of tests/test_forcing_host.py and tests/test_gpu_forcing.py, fixed here: s = 0.5 sin(pi x) cos(8 t) and
g = B y0 + 0.3 sin(6 t), so g(t0) is what the initial values give (a conflict between the 1e-10 initial observation and the
boundary rows is not the subject).  dt = 2^-7, 12 steps.  With these, on the oracle alone, the forced and the unforced means differ
at the last time by 0.16 (Dirichlet cases) and 0.04 (Neumann) on a solution of size 0.1; tests/test_forcing_host.py asserts that
every case moves by 1e3 times the parity tolerance, so a device that ignores the table cannot pass."""

import functools
from collections import namedtuple

import numpy as np

import pnmol
import pnmol_oracle as oracle
import iterated_reference as ir
import observe_reference as oref
from pnmol.pde import examples, reactions
from pnmol.pde.forcing import Forcing

DT, STEPS = 2.0 ** -7, 12
S_AMP, S_RATE, G_AMP, G_RATE = 0.5, 8.0, 0.3, 6.0
MODES = ("source", "boundary", "both")
# (N, nu, bcond): m = 22 in mp = 32; m = 35 in mp = 64 with 31 padded points; flux data with R_sqrtm
SHAPES = [(20, 1, "dirichlet"), (33, 2, "dirichlet"), (32, 2, "neumann")]
BIG = (260, 1, "dirichlet", 3)      # m = 262 in mp = 288: the second workgroup of the 256-thread launch; 3 steps
LATENT = (24, 1, "dirichlet")
MEAN_RTOL = 1e-5                    # helpers.assert_mean_std_parity: the tolerance the GPU tests apply to means


def source(t, X, species=1, scale=1.0):
    """s(t, X) = scale 0.5 sin(pi x) cos(8 t), stacked `species` times."""
    x = np.asarray(X, dtype=np.float64).reshape(-1)
    return np.tile(scale * S_AMP * np.sin(np.pi * x) * np.cos(S_RATE * t), species)


class BoundaryValues:
    """g(t) = B y0 + 0.3 sin(6 t); `bind` takes B y0 from the discretised problem."""

    g0 = None

    def bind(self, pde):
        self.g0 = np.asarray(pde.B @ pde.y0, dtype=np.float64)
        return self

    def __call__(self, t):
        return self.g0 + G_AMP * np.sin(G_RATE * t)


def make_forcing(mode, species=1, scale=1.0):
    """(Forcing, its BoundaryValues or None) for a mode of MODES."""
    g = BoundaryValues() if mode in ("boundary", "both") else None
    s = functools.partial(source, species=species, scale=scale) if mode in ("source", "both") else None
    return Forcing(source=s, boundary_values=g), g


class ForcedMixin:
    """`evaluate_ode` of an oracle solver with g(t) taken off the boundary rows of z (the last nB entries)."""

    boundary_values = None

    def evaluate_ode(self, pde, p0, p1, m_pred, t, *more):
        out = super().evaluate_ode(pde, p0, p1, m_pred, t, *more)
        if self.boundary_values is None or pde.B.shape[0] == 0:
            return out
        z = np.array(out[0], dtype=np.float64)
        z[-pde.B.shape[0]:] -= self.boundary_values(t)
        return (z,) + tuple(out[1:])


class ForcedWhiteNoiseEK1(ForcedMixin, oracle.WhiteNoiseEK1):
    pass


class ForcedLatentForceEK1(ForcedMixin, oracle.LatentForceEK1):
    pass


class ForcedPointwiseEK1(ForcedMixin, ir.PointwiseEK1):
    """... with the injected linearisation points of tests/iterated_reference.py."""


def force_oracle(opde, osolver, mode, species=1, scale=1.0):
    """Put the forcing of `mode` into an oracle pair (osolver of a Forced* class): the source through `opde.f`, the boundary
    values through the solver.  Returns the pair."""
    if mode in ("source", "both"):
        X = opde.mesh_spatial.points
        d = opde.L.shape[0]
        f, df = getattr(opde, "f", None), getattr(opde, "df", None)
        if not osolver.semilinear:                              # a linear problem: f = s, df = 0, as the reference would take it
            osolver.semilinear = True
            f, df = (lambda _t, x: np.zeros(d)), (lambda _t, x: np.zeros((d, d)))
        opde.f = lambda t, x, f=f: f(t, x) + source(t, X, species, scale)
        opde.df = df
    if mode in ("boundary", "both"):
        osolver.boundary_values = BoundaryValues().bind(opde)
    return opde, osolver


# ------------------------------------------------------------------------------------------------ linear cases
def _heat_kw(N, K, dt, bcond):
    return dict(tmax=K * dt, dx=1.0 / (N - 1), diffusion_rate=0.05, bcond=bcond, stencil_size_interior=3, stencil_size_boundary=3,
                nugget_gram_matrix_fd=0.0)


def linear_pair(N, nu, bcond, mode, K=STEPS, dt=DT):
    """(pde, solver, opde, osolver): the heat problem of helpers.make_pair, driven (mode None: as it is)."""
    kw = _heat_kw(N, K, dt, bcond)
    forcing, g = make_forcing(mode) if mode else (None, None)
    pde = examples.heat_1d_discretized(kernel=pnmol.kernels.SquareExponential(), forcing=forcing, **kw)
    if g is not None:
        g.bind(pde)
    solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=nu, steprule=pnmol.odetools.step.Constant(dt),
                                             spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    opde = oracle.heat_1d_discretized(kernel=oracle.SquareExponential(), **kw)
    osolver = ForcedWhiteNoiseEK1(num_derivatives=nu, steprule=oracle.Constant(dt), canonical_factor_signs=True,
                                  spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
    if mode:
        force_oracle(opde, osolver, mode)
    return pde, solver, opde, osolver


def latent_pair(mode, K=STEPS, dt=DT):
    """The latent-force twin (observe_reference.latent_pair), driven."""
    N, nu, bcond = LATENT
    pde, solver, opde, _ = oref.latent_pair(N, nu, dt, K, bcond, 0.05)
    forcing, g = make_forcing(mode)
    pde = examples.heat_1d_discretized(kernel=pnmol.kernels.SquareExponential(), forcing=forcing, **_heat_kw(N, K, dt, bcond))
    if g is not None:
        g.bind(pde)
    osolver = ForcedLatentForceEK1(num_derivatives=nu, steprule=oracle.Constant(dt), canonical_factor_signs=True,
                                   spatial_kernel=oracle.SquareExponential() + oracle.WhiteNoise())
    force_oracle(opde, osolver, mode)
    return pde, solver, opde, osolver


def host_route_pair(N, nu, bcond, K=STEPS, dt=DT):
    """The source-only problem WITHOUT `pde.forcing`, as it could be posed before: a semilinear problem with f(t, u) = s(t) and
    df = 0 on host callables (`reaction_on_device = False`).  (pde, solver, opde, osolver)."""
    from pnmol import diffops, mesh
    from pnmol.pde import problems

    kw = _heat_kw(N, K, dt, bcond)
    cls = {"dirichlet": problems.SemiLinearEvolutionDirichlet, "neumann": problems.SemiLinearEvolutionNeumann}[bcond]
    heat = examples.heat_1d(tmax=kw["tmax"], diffusion_rate=kw["diffusion_rate"], bcond=bcond)
    holder = {}
    pde = cls(t0=0.0, tmax=kw["tmax"], y0_fun=heat.y0_fun, bbox=heat.bbox, diffop=diffops.laplace(),
              diffop_scale=kw["diffusion_rate"], f=lambda t, x: source(t, holder["X"]),
              df=lambda _t, x: np.zeros((x.size, x.size)), df_diagonal=lambda _t, x: np.zeros(x.size))
    pde.discretize(mesh_spatial=mesh.RectangularMesh.from_bbox_1d(pde.bbox, step=kw["dx"]), kernel=pnmol.kernels.SquareExponential(),
                   stencil_size_interior=3, stencil_size_boundary=3, nugget_gram_matrix=0.0)
    holder["X"] = pde.mesh_spatial.points
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=nu, steprule=pnmol.odetools.step.Constant(dt),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    solver.reaction_on_device = False
    _, _, opde, osolver = linear_pair(N, nu, bcond, "source", K, dt)
    return pde, solver, opde, osolver


# ------------------------------------------------------------------------------------------------ composition with a term
# name: (kind, N per species, bcond, dt, coefficient(s), mode, scale of the source): the terms and step sizes of
# tests/iterated_reference.py.  The Lotka-Volterra species are of size 5 and 20 where the other solutions are of size 1: its source
# is 20 times the others', so that it moves both species by 1e3 tolerances (tests/test_forcing_host.py).
Term = namedtuple("Term", "kind N bcond dt coef mode scale")
TERMS = {
    "logistic-source": Term("fisher", 33, "neumann", 2.0 ** -4, 10.0, "source", 1.0),
    "burgers-boundary": Term("burgers", 33, "dirichlet", 2.0 ** -6, 1.0, "boundary", 1.0),
    "lotka-volterra-source": Term("lotka_volterra", 16, "neumann", 2.0 ** -4, (0.5, 0.4, 0.4, 0.5), "source", 20.0),
}
TERM_STEPS = 13


def term_pair(name, forced=True, **attrs):
    """(pde, solver, opde, osolver) of a case of TERMS (forced=False: without its forcing); osolver takes injected points
    (`set_points`)."""
    case = TERMS[name] if forced else TERMS[name]._replace(mode=None)
    as_ir = ir.Case(case.kind, case.N, 2, case.bcond, TERM_STEPS, case.dt, case.coef)
    species = 2 if case.kind == "lotka_volterra" else 1
    forcing, g = make_forcing(case.mode, species, case.scale) if case.mode else (None, None)
    kernel, okernel = pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise(), oracle.Matern52() + oracle.WhiteNoise()
    dx, tmax, coef = 1.0 / (case.N - 1), TERM_STEPS * case.dt, case.coef
    if case.kind == "lotka_volterra":
        pde = examples.reaction_diffusion_system_1d_discretized(reactions.lotka_volterra(*coef), diffusion_rates=(0.1, 0.1),
                                                                y0_fun=examples.lotka_volterra_y0, dx=dx, tmax=tmax, forcing=forcing)
        kernel, okernel = pnmol.kernels.duplicate(kernel, num=2), oracle.duplicate(okernel, 2)
        opde = oracle.lotka_volterra_1d_discretized(dx=dx, tmax=tmax, **dict(zip("abcd", coef)))
    elif case.kind == "burgers":
        import convection_reference as cref

        pde = examples.convection_diffusion_1d_discretized(reactions.Convection((0.0, -coef)), diffusion_rate=ir.KAPPA_BURGERS,
                                                           kernel=pnmol.kernels.SquareExponential(), nugget_gram_matrix_fd=0.0,
                                                           forcing=forcing, **ir._kw(as_ir))
        opde = oracle.heat_1d_discretized(kernel=oracle.SquareExponential(), diffusion_rate=ir.KAPPA_BURGERS, **ir._kw(as_ir))
        G, _ = cref.oracle_gradient(opde.mesh_spatial, oracle.SquareExponential(), 3)
        opde.f = lambda _t, u: -coef * u * (G @ u)
        opde.df = lambda _t, u: -coef * (np.diag(G @ u) + u[:, None] * G)
    else:
        pde = examples.reaction_diffusion_1d_discretized(reactions.logistic(coef), diffusion_rate=ir.KAPPA,
                                                         kernel=pnmol.kernels.SquareExponential(), nugget_gram_matrix_fd=0.0,
                                                         forcing=forcing, **ir._kw(as_ir))
        opde = oracle.heat_1d_discretized(kernel=oracle.SquareExponential(), diffusion_rate=ir.KAPPA, **ir._kw(as_ir))
        opde.f = lambda _t, x: coef * x * (1.0 - x)
        opde.df = lambda _t, x: np.diag(coef * (1.0 - 2.0 * x))
    if g is not None:
        g.bind(pde)
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(case.dt),
                                                 spatial_kernel=kernel)
    for key, value in attrs.items():
        setattr(solver, key, value)
    osolver = ForcedPointwiseEK1(num_derivatives=2, steprule=oracle.Constant(case.dt), semilinear=True,
                                 canonical_factor_signs=True, spatial_kernel=okernel)
    if case.mode:
        force_oracle(opde, osolver, case.mode, species, case.scale)
    return pde, solver, opde, osolver


def term_observations(name, q=6):
    """Three readings of one sensor array for a case of TERMS (t0, behind step 6, the last step): 1.05 x the forced oracle's own
    filtering mean plus noise of the size of its median interior std."""
    sol, means, stds = term_reference(name)
    C = oref.sensor_matrix(means.shape[1], q)
    noise = float(np.median(stds[1:, 1:-1]))
    rng = np.random.default_rng(means.shape[1] + q)
    return [pnmol.data.Observation(sol.t[j], C, 1.05 * (C @ means[j]) + noise * rng.standard_normal(q), noise)
            for j in (0, 6, len(sol.t) - 1)]


# ------------------------------------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def linear_reference(N, nu, bcond, mode, K=STEPS):
    """(oracle.Solution, means, stds) of a linear case, computed once per process and shared (nothing modifies it)."""
    _, _, opde, osolver = linear_pair(N, nu, bcond, mode, K)
    sol = osolver.solve(opde)
    return (sol,) + tuple(oracle.read_mean_and_std(sol, osolver.E0))


@functools.lru_cache(maxsize=None)
def latent_reference(mode):
    _, _, opde, osolver = latent_pair(mode)
    sol = osolver.solve(opde)
    return (sol,) + tuple(oracle.read_mean_and_std_latent(sol, osolver.E0))


@functools.lru_cache(maxsize=None)
def term_reference(name, forced=True):
    _, _, opde, osolver = term_pair(name, forced)
    sol = osolver.solve(opde)
    return (sol,) + tuple(oracle.read_mean_and_std(sol, osolver.E0))
