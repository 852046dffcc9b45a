"""The oracle side of the convection tests (tests/test_convection_host.py, tests/test_gpu_convection.py): viscous Burgers and
Burgers-Fisher problems for `pnmol_oracle`, whose recipes stop at reaction terms.  f = -u (G u) [+ rate u (1 - u)] and its dense
Jacobian -(diag(G u) + diag(u) G) [+ diag(rate (1 - 2 u))] as closed forms, G from the oracle's own `fd_coefficients` with the
kernel's first derivatives on the mesh's neighbour sets.  kappa = 0.02, dt = 2^-7, SE kernel.  Results are computed once per
case and shared; nothing modifies them."""

import numpy as np

import pnmol
import pnmol_oracle as oracle
from pnmol.pde import reactions

DT = 2.0 ** -7
KAPPA = 0.02
RATE = 1.0

# (N, nu, boundary, steps): the cases in which the convection term was checked to move the oracle's final mean by at least a
# tenth of its largest entry (tests/test_convection_host.py asserts it)
CASES = [(33, 2, "dirichlet", 24), (33, 2, "neumann", 24), (48, 1, "dirichlet", 16), (33, 3, "dirichlet", 12)]


def y0_fun(x):
    return np.sin(np.pi * x)


def kw(N, bcond, tmax):
    return dict(tmax=tmax, dx=1.0 / (N - 1), bcond=bcond, stencil_size_interior=3, stencil_size_boundary=3, y0_fun=y0_fun)


def oracle_gradient(mesh, kernel, num=3):
    """(G, uncertainty per row): kernel finite differences of d/dx on every point's `num` nearest neighbours."""
    N = mesh.shape[0]
    G, unc = np.zeros((N, N)), np.zeros(N)
    nb_pts, nb_idx = mesh.neighbours(mesh.points, num)
    for row, (x, Xn, cols) in enumerate(zip(mesh.points, nb_pts, nb_idx)):
        G[row, cols], unc[row] = oracle.fd_coefficients(x, Xn, kernel, kernel.grad_x_1d, kernel.grad_xy_1d)
    return G, unc


def oracle_problem(variant, N, bcond, tmax, gradient_stencil_size=3):
    """variant: "burgers", "burgers_fisher" or "heat" (the same data without the term)."""
    kernel = oracle.SquareExponential()
    p = oracle.heat_1d_discretized(kernel=kernel, diffusion_rate=KAPPA, **kw(N, bcond, tmax))
    G, _ = oracle_gradient(p.mesh_spatial, kernel, gradient_stencil_size)
    p.G = G
    if variant == "heat":
        p.f = lambda _t, u: np.zeros_like(u)
        p.df = lambda _t, u: np.zeros((u.size, u.size))
    elif variant == "burgers":
        p.f = lambda _t, u: -u * (G @ u)
        p.df = lambda _t, u: -(np.diag(G @ u) + u[:, None] * G)
    elif variant == "burgers_fisher":
        p.f = lambda _t, u: -u * (G @ u) + RATE * u * (1.0 - u)
        p.df = lambda _t, u: -(np.diag(G @ u) + u[:, None] * G) + np.diag(RATE * (1.0 - 2.0 * u))
    else:
        raise ValueError(variant)
    return p


class RecordingAdaptive(oracle.Adaptive):
    """The oracle's adaptive rule, keeping every scaled error norm it judges."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.norms = []

    def is_accepted(self, scaled_error_estimate):
        self.norms.append(float(scaled_error_estimate))
        return super().is_accepted(scaled_error_estimate)


_ORACLE = {}


def oracle_solve(variant, N, nu, bcond, K, adaptive=None):
    """(osolver, osol, means, stds) of the oracle for K steps of DT (adaptive: a dict of tolerances, tmax = K DT)."""
    key = (variant, N, nu, bcond, K, None if adaptive is None else tuple(sorted(adaptive.items())))
    if key not in _ORACLE:
        rule = oracle.Constant(DT) if adaptive is None else RecordingAdaptive(**adaptive)
        osolver = oracle.WhiteNoiseEK1(num_derivatives=nu, steprule=rule, semilinear=True, canonical_factor_signs=True,
                                       spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
        osol = osolver.solve(oracle_problem(variant, N, bcond, K * DT))
        _ORACLE[key] = (osolver, osol) + tuple(oracle.read_mean_and_std(osol, osolver.E0))
    return _ORACLE[key]


def term_of(variant):
    return {"burgers": reactions.burgers, "burgers_fisher": lambda: reactions.burgers_fisher(RATE)}[variant]()


def product(variant, N, nu, bcond, tmax, steprule=None, solver_cls=None, gradient_stencil_size=3, **attrs):
    """(pde, solver) of the product for the same problem."""
    pde = pnmol.pde.examples.convection_diffusion_1d_discretized(
        term_of(variant), diffusion_rate=KAPPA, kernel=pnmol.kernels.SquareExponential(), nugget_gram_matrix_fd=0.0,
        gradient_stencil_size=gradient_stencil_size, **kw(N, bcond, tmax))
    cls = solver_cls or pnmol.white.SemiLinearWhiteNoiseEK1
    solver = cls(num_derivatives=nu, steprule=steprule or pnmol.odetools.step.Constant(DT),
                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    for key, value in attrs.items():
        setattr(solver, key, value)
    return pde, solver
