"""Problem recipes (reference: src/pnmol/pde/examples.py:13-81, :347-357).

Heat equation (1-d, and a 2-d Dirichlet recipe assembled from the reference's parts), spruce-budworm (Fisher), and the
Lotka-Volterra / SIR systems of PDEs that figures 3-4 run (examples.py:84-248), with closed-form Jacobians in place of
`jax.jacfwd`.
"""

import functools

import numpy as np

from .. import diffops, discretize, kernels, mesh
from . import coefficients as _coefficients
from . import forcing as _forcing
from . import problems, reactions


def heat_1d_discretized(*, bbox=None, dx=0.05, stencil_size_interior=3, stencil_size_boundary=3, t0=0.0, tmax=5.0,
                        y0_fun=None, diffusion_rate=0.05, nugget_gram_matrix_fd=0.0, kernel=None,
                        bcond="dirichlet", forcing=None):
    """forcing: a `pnmol.pde.forcing.Forcing` (source s(t, x), boundary values g(t)) or None; it becomes `pde.forcing`."""
    heat = heat_1d(bbox=bbox, t0=t0, tmax=tmax, y0_fun=y0_fun, diffusion_rate=diffusion_rate, bcond=bcond)
    mesh_spatial = mesh.RectangularMesh.from_bbox_1d(heat.bbox, step=dx)
    if kernel is None:
        kernel = kernels.SquareExponential()
    heat.discretize(mesh_spatial=mesh_spatial, kernel=kernel, stencil_size_interior=stencil_size_interior,
                    stencil_size_boundary=stencil_size_boundary, nugget_gram_matrix=nugget_gram_matrix_fd)
    return _forcing.attach(heat, forcing)


def heat_1d(*, bbox=None, t0=0.0, tmax=5.0, y0_fun=None, diffusion_rate=0.05, bcond="dirichlet"):
    laplace = diffops.laplace()
    if bbox is None:
        bbox = [0.0, 1.0]
    bbox = np.asarray(bbox, dtype=np.float64)
    if y0_fun is None:
        bell_centered = functools.partial(gaussian_bell_1d_centered, bbox=bbox)
        y0_fun = lambda x: bell_centered(x) * sin_bell_1d(x)  # noqa: E731
    cls = {"dirichlet": problems.LinearEvolutionDirichlet, "neumann": problems.LinearEvolutionNeumann}.get(bcond)
    if cls is None:
        raise ValueError
    return cls(diffop=laplace, diffop_scale=diffusion_rate, bbox=bbox, t0=t0, tmax=tmax, y0_fun=y0_fun)


def heat_2d_dirichlet_discretized(*, nums=(64, 64), stencil_size_interior=5, stencil_size_boundary=5, t0=0.0,
                                  tmax=1.0, diffusion_rate=0.05, kernel=None, y0_fun=None):
    """2-d heat problem assembled from the reference's parts (mesh.py:100-130, mixins.py:51-54);
    the reference itself ships no 2-d recipe."""
    bbox = np.array([[0.0, 0.0], [1.0, 1.0]])
    if y0_fun is None:
        y0_fun = lambda p: (0.1 * np.sin(np.pi * p[:, 0]) * np.sin(np.pi * p[:, 1]))[:, None]  # noqa: E731
    heat = problems.LinearEvolutionDirichlet(diffop=diffops.laplace(), diffop_scale=diffusion_rate, bbox=bbox,
                                             t0=t0, tmax=tmax, y0_fun=y0_fun)
    heat.discretize(mesh_spatial=mesh.RectangularMesh.from_bbox_2d(bbox, nums=nums),
                    kernel=kernel or kernels.SquareExponential(), stencil_size_interior=stencil_size_interior,
                    stencil_size_boundary=stencil_size_boundary)
    return heat


def sir_1d_discretized(*, bbox=None, dx=0.05, t0=0.0, tmax=50.0, beta=0.3, gamma=0.07, N=1000.0, diffusion_rate_S=0.1,
                       diffusion_rate_I=0.1, diffusion_rate_R=0.1, kernel=None, nugget_gram_matrix_fd=0.0,
                       stencil_size_interior=3, stencil_size_boundary=3):
    """examples.py:84-124."""
    sir = sir_1d(bbox=bbox, t0=t0, tmax=tmax, diffusion_rate_S=diffusion_rate_S, diffusion_rate_I=diffusion_rate_I,
                 diffusion_rate_R=diffusion_rate_R, beta=beta, gamma=gamma, N=N)
    mesh_spatial = mesh.RectangularMesh.from_bbox_1d(sir.bbox, step=dx)
    if kernel is None:
        kernel = kernels.SquareExponential()
    sir.discretize_system(mesh_spatial=mesh_spatial, kernel=kernel, stencil_size_interior=stencil_size_interior,
                          stencil_size_boundary=stencil_size_boundary, nugget_gram_matrix=nugget_gram_matrix_fd)
    return sir


def sir_1d(*, bbox=None, t0=0.0, tmax=50.0, diffusion_rate_S=0.1, diffusion_rate_I=0.1, diffusion_rate_R=0.1, beta=0.3,
           gamma=0.07, N=1000.0):
    """Spatial SIR model, state [S; I; R], Neumann boundary (examples.py:127-178); `df` is the closed-form Jacobian of
    the reaction term (the reference differentiates it with jax.jacfwd)."""
    if bbox is None:
        bbox = [0.0, 1.0]
    bbox = np.asarray(bbox, dtype=np.float64)

    def y0_fun(x):
        init_infectious = 200.0 * gaussian_bell_1d_centered(x, bbox, width=0.5) + 1.0
        return np.concatenate((N * np.ones_like(init_infectious) - init_infectious, init_infectious,
                               np.zeros_like(init_infectious)))

    def f(_t, x):
        s, i, r = np.split(np.asarray(x, dtype=np.float64), 3)
        spatial_n = s + i + r
        return np.concatenate((-beta * s * i / spatial_n, beta * s * i / spatial_n - gamma * i, gamma * i))

    def df(_t, x):
        s, i, r = np.split(np.asarray(x, dtype=np.float64), 3)
        tot = s + i + r
        g = beta * s * i / tot
        gs, gi, gr = beta * i / tot - g / tot, beta * s / tot - g / tot, -g / tot
        zero = np.zeros((s.size, s.size))
        return np.block([[np.diag(-gs), np.diag(-gi), np.diag(-gr)], [np.diag(gs), np.diag(gi - gamma), np.diag(gr)],
                         [zero, np.diag(gamma * np.ones_like(i)), zero]])

    laplace = diffops.laplace()
    return problems.SystemSemiLinearEvolutionNeumann(
        diffop=(laplace, laplace, laplace), diffop_scale=(diffusion_rate_S, diffusion_rate_I, diffusion_rate_R),
        bbox=bbox, t0=t0, tmax=tmax, y0_fun=y0_fun, f=f, df=df, df_diagonal=None)


def lotka_volterra_1d_discretized(*, dx=0.05, kernel=None, nugget_gram_matrix_fd=0.0, stencil_size_interior=3,
                                  stencil_size_boundary=3, **kwargs):
    """examples.py:181-203."""
    pde = lotka_volterra_1d(**kwargs)
    mesh_spatial = mesh.RectangularMesh.from_bbox_1d(pde.bbox, step=dx)
    if kernel is None:
        kernel = kernels.SquareExponential()
    pde.discretize_system(mesh_spatial=mesh_spatial, kernel=kernel, stencil_size_interior=stencil_size_interior,
                          stencil_size_boundary=stencil_size_boundary, nugget_gram_matrix=nugget_gram_matrix_fd)
    return pde


def lotka_volterra_1d(*, bbox=None, t0=0.0, tmax=10.0, a=0.5, b=0.05, c=0.05, d=0.5, diffusion_scale_u=0.1,
                      diffusion_scale_v=0.1):
    """Predator-prey system u_t = D_u u_xx + a u - b u v, v_t = D_v v_xx + c u v - d v, state [u; v], Neumann boundary
    (examples.py:206-248, the workload of experiments/figure4.py); closed-form Jacobian instead of jax.jacfwd."""
    if bbox is None:
        bbox = [0.0, 1.0]
    bbox = np.asarray(bbox, dtype=np.float64)

    def y0_fun(x):
        return np.concatenate((5 * np.ones_like(x), 20.0 * gaussian_bell_1d(x)))

    def f_lotka_volterra(_, x):
        u, v = np.split(np.asarray(x, dtype=np.float64), 2)
        return np.concatenate((a * u - b * u * v, c * u * v - d * v))

    def df_lotka_volterra(_, x):
        u, v = np.split(np.asarray(x, dtype=np.float64), 2)
        return np.block([[np.diag(a - b * v), np.diag(-b * u)], [np.diag(c * v), np.diag(c * u - d)]])

    laplace = diffops.laplace()
    return problems.SystemSemiLinearEvolutionNeumann(
        diffop=(laplace, laplace), diffop_scale=(diffusion_scale_u, diffusion_scale_v), bbox=bbox, t0=t0, tmax=tmax,
        y0_fun=y0_fun, f=f_lotka_volterra, df=df_lotka_volterra, df_diagonal=None)


def spruce_budworm_1d_discretized(*, bbox=None, t0=0.0, tmax=10.0, diffusion_rate=1.0, y0_fun=None, dx=0.1, kernel=None,
                                  nugget_gram_matrix_fd=0.0, stencil_size_interior=3, stencil_size_boundary=3,
                                  bcond="dirichlet", growth_rate=1.0):
    """examples.py:251-289."""
    spruce = spruce_budworm_1d(bbox=bbox, t0=t0, tmax=tmax, diffusion_rate=diffusion_rate, y0_fun=y0_fun, bcond=bcond,
                               growth_rate=growth_rate)
    mesh_spatial = mesh.RectangularMesh.from_bbox_1d(spruce.bbox, step=dx)
    if kernel is None:
        kernel = kernels.SquareExponential()
    spruce.discretize(mesh_spatial=mesh_spatial, kernel=kernel, stencil_size_interior=stencil_size_interior,
                      stencil_size_boundary=stencil_size_boundary, nugget_gram_matrix=nugget_gram_matrix_fd)
    return spruce


def spruce_budworm_1d(*, bbox=None, t0=0.0, tmax=10.0, diffusion_rate=0.1, y0_fun=None, bcond="dirichlet",
                      growth_rate=1.0):
    """Fisher's equation u_t = kappa u_xx + c u (1 - u)  (examples.py:292-341); df is the (diagonal) Jacobian."""
    if bbox is None:
        bbox = [0.0, 1.0]
    bbox = np.asarray(bbox, dtype=np.float64)
    if y0_fun is None:
        y0_fun = sin_bell_1d

    def f_spruce(_, x, c=growth_rate):
        return c * x * (1.0 - x)

    def df_spruce(_, x, c=growth_rate):
        return np.diag(c * (1.0 - 2.0 * np.asarray(x)))

    def df_diagonal_spruce(_, x, c=growth_rate):   # (the reference passes df_diagonal=None; the Jacobian IS diagonal)
        return c * (1.0 - 2.0 * np.asarray(x))

    cls = {"dirichlet": problems.SemiLinearEvolutionDirichlet, "neumann": problems.SemiLinearEvolutionNeumann}.get(bcond)
    if cls is None:
        raise ValueError
    return cls(t0=t0, tmax=tmax, y0_fun=y0_fun, bbox=bbox, diffop=diffops.laplace(), diffop_scale=diffusion_rate,
               f=f_spruce, df=df_spruce, df_diagonal=df_diagonal_spruce)


def reaction_diffusion_1d_discretized(reaction, *, bbox=None, t0=0.0, tmax=10.0, diffusion_rate=1.0, y0_fun=None, dx=0.1,
                                      kernel=None, nugget_gram_matrix_fd=0.0, stencil_size_interior=3,
                                      stencil_size_boundary=3, bcond="dirichlet", forcing=None):
    """u_t = kappa u_xx + r(u) for a pointwise `reaction` (pde/reactions.py), discretised like the spruce-budworm recipe
    above: the same problem class, with f, df and df_diagonal taken from the reaction.  `pde.reaction` lets the solver
    evaluate r on the device (white.py, `SemiLinearWhiteNoiseEK1.reaction_on_device`).  forcing: a `pnmol.pde.forcing.Forcing` or
    None; it becomes `pde.forcing`, and `pde.f` includes its source."""
    if bbox is None:
        bbox = [0.0, 1.0]
    bbox = np.asarray(bbox, dtype=np.float64)
    if y0_fun is None:
        y0_fun = sin_bell_1d
    cls = {"dirichlet": problems.SemiLinearEvolutionDirichlet, "neumann": problems.SemiLinearEvolutionNeumann}.get(bcond)
    if cls is None:
        raise ValueError
    f, df, df_diagonal = reaction.callables()
    pde = cls(t0=t0, tmax=tmax, y0_fun=y0_fun, bbox=bbox, diffop=diffops.laplace(), diffop_scale=diffusion_rate,
              f=f, df=df, df_diagonal=df_diagonal)
    pde.reaction = reaction
    mesh_spatial = mesh.RectangularMesh.from_bbox_1d(pde.bbox, step=dx)
    if kernel is None:
        kernel = kernels.SquareExponential()
    pde.discretize(mesh_spatial=mesh_spatial, kernel=kernel, stencil_size_interior=stencil_size_interior,
                   stencil_size_boundary=stencil_size_boundary, nugget_gram_matrix=nugget_gram_matrix_fd)
    return _forcing.attach(pde, forcing, f)


def convection_diffusion_1d_discretized(term, *, bbox=None, t0=0.0, tmax=10.0, diffusion_rate=1.0, y0_fun=None, dx=0.1,
                                        kernel=None, nugget_gram_matrix_fd=0.0, stencil_size_interior=3,
                                        stencil_size_boundary=3, gradient_stencil_size=3, bcond="dirichlet", forcing=None):
    """u_t = kappa u_xx + c(u) u_x + r(u) for a convection `term` (pde/reactions.py, `Convection`), discretised like
    `reaction_diffusion_1d_discretized`.  The term's operator G is the kernel finite-difference gradient on the mesh's own
    neighbour sets (`gradient_stencil_size` points, interior and boundary rows alike); f and df come from the term, and
    `pde.reaction` lets the solver linearise on the device.  E_sqrtm stays the Laplacian's: the uncertainty of G's weights is
    not modelled.  forcing: as in `reaction_diffusion_1d_discretized`."""
    if bbox is None:
        bbox = [0.0, 1.0]
    bbox = np.asarray(bbox, dtype=np.float64)
    if y0_fun is None:
        y0_fun = sin_bell_1d
    cls = {"dirichlet": problems.SemiLinearEvolutionDirichlet, "neumann": problems.SemiLinearEvolutionNeumann}.get(bcond)
    if cls is None:
        raise ValueError
    f, df, df_diagonal = term.callables()
    pde = cls(t0=t0, tmax=tmax, y0_fun=y0_fun, bbox=bbox, diffop=diffops.laplace(), diffop_scale=diffusion_rate,
              f=f, df=df, df_diagonal=df_diagonal)
    pde.reaction = term
    mesh_spatial = mesh.RectangularMesh.from_bbox_1d(pde.bbox, step=dx)
    if kernel is None:
        kernel = kernels.SquareExponential()
    pde.discretize(mesh_spatial=mesh_spatial, kernel=kernel, stencil_size_interior=stencil_size_interior,
                   stencil_size_boundary=stencil_size_boundary, nugget_gram_matrix=nugget_gram_matrix_fd)
    G, _ = discretize.fd_probabilistic(diffops.gradient(), mesh_spatial=mesh_spatial, kernel=kernel,
                                       stencil_size_interior=gradient_stencil_size,
                                       stencil_size_boundary=gradient_stencil_size, nugget_gram_matrix=nugget_gram_matrix_fd)
    term.set_operator(G)
    return _forcing.attach(pde, forcing, f)


def _time_varying_base(reaction, forcing, **kw):
    """The problem the two recipes below start from, discretised with a unit diffusion rate: (pde, Laplacian, its E_sqrtm)."""
    if reaction is None:
        pde = heat_1d_discretized(diffusion_rate=1.0, forcing=forcing, **kw)
    else:
        y0_fun = heat_1d(bbox=kw["bbox"], bcond=kw["bcond"]).y0_fun        # (the initial values of the heat recipe, reaction or not)
        pde = reaction_diffusion_1d_discretized(reaction, diffusion_rate=1.0, forcing=forcing, y0_fun=y0_fun, **kw)
    return pde, pde.L, pde.E_sqrtm


def heat_1d_time_varying_discretized(*, diffusion_rate, reaction=None, forcing=None, bbox=None, dx=0.05, t0=0.0, tmax=5.0,
                                     stencil_size_interior=3, stencil_size_boundary=3, nugget_gram_matrix_fd=0.0, kernel=None,
                                     bcond="dirichlet"):
    """u_t = kappa(t) u_xx [+ r(u)] [+ s(t, x)]: `diffusion_rate` is a callable t -> kappa(t).  The problem carries
    `pde.time_dependent_operator` (pde/coefficients.py) with the one operator u_xx and its FD uncertainty; `pde.L` and
    `pde.E_sqrtm` are those of t0.  reaction: a scalar `pnmol.pde.reactions.Reaction` or None; forcing: as in
    `heat_1d_discretized`."""
    if not callable(diffusion_rate):
        raise TypeError("heat_1d_time_varying_discretized: diffusion_rate must be a callable t -> kappa(t)")
    pde, lap, lap_e = _time_varying_base(reaction, forcing, bbox=bbox, dx=dx, t0=t0, tmax=tmax, bcond=bcond, kernel=kernel,
                                         stencil_size_interior=stencil_size_interior, stencil_size_boundary=stencil_size_boundary,
                                         nugget_gram_matrix_fd=nugget_gram_matrix_fd)
    return _coefficients.attach(pde, _coefficients.TimeDependentOperator([lap], [lap_e], diffusion_rate))


def advection_diffusion_1d_discretized(diffusion_rate, *, velocity, reaction=None, forcing=None, bbox=None, dx=0.05, t0=0.0,
                                       tmax=5.0, stencil_size_interior=3, stencil_size_boundary=3, gradient_stencil_size=3,
                                       nugget_gram_matrix_fd=0.0, kernel=None, bcond="dirichlet"):
    """u_t = kappa u_xx - c(t) u_x [+ r(u)] [+ s(t, x)]: transport in a flow whose `velocity` is a callable t -> c(t).  The gradient
    is the kernel finite-difference one on its own neighbour sets (`gradient_stencil_size` points), and -- unlike the convection
    recipe above -- its FD uncertainty is part of the model: the noise of the PDE rows is diag((kappa e_lap)^2 + (c(t) e_grad)^2).
    `pde.time_dependent_operator` holds (u_xx, u_x) with the coefficients (kappa, -c(t))."""
    if not callable(velocity):
        raise TypeError("advection_diffusion_1d_discretized: velocity must be a callable t -> c(t)")
    kappa = float(diffusion_rate)
    pde, lap, lap_e = _time_varying_base(reaction, forcing, bbox=bbox, dx=dx, t0=t0, tmax=tmax, bcond=bcond, kernel=kernel,
                                         stencil_size_interior=stencil_size_interior, stencil_size_boundary=stencil_size_boundary,
                                         nugget_gram_matrix_fd=nugget_gram_matrix_fd)
    grad, grad_e = discretize.fd_probabilistic(diffops.gradient(), mesh_spatial=pde.mesh_spatial,
                                               kernel=kernel or kernels.SquareExponential(),
                                               stencil_size_interior=gradient_stencil_size,
                                               stencil_size_boundary=gradient_stencil_size, nugget_gram_matrix=nugget_gram_matrix_fd)
    operator = _coefficients.TimeDependentOperator([lap, grad], [lap_e, grad_e], lambda t: (kappa, -float(velocity(t))))
    return _coefficients.attach(pde, operator)


def burgers_1d_discretized(viscosity=0.02, **kwargs):
    """Viscous Burgers u_t = viscosity u_xx - u u_x: `convection_diffusion_1d_discretized` with `reactions.burgers()`."""
    return convection_diffusion_1d_discretized(reactions.burgers(), diffusion_rate=viscosity, **kwargs)


def reaction_diffusion_system_1d_discretized(reaction, *, diffusion_rates, y0_fun, bbox=None, t0=0.0, tmax=10.0, dx=0.05,
                                             kernel=None, nugget_gram_matrix_fd=0.0, stencil_size_interior=3,
                                             stencil_size_boundary=3, forcing=None):
    """(u_c)_t = D_c (u_c)_xx + r_c(u_0, ..., u_{C-1}) for a coupled pointwise `reaction` (pde/reactions.py, `SystemReaction`),
    Neumann boundary: the problem class and discretisation of the Lotka-Volterra / SIR recipes above, with f and df taken from
    the reaction.  `y0_fun(x)` returns the stacked initial values [u_0; ...; u_{C-1}].  `pde.reaction` lets the solver linearise on
    the device (white.py, `SemiLinearWhiteNoiseEK1.reaction_on_device`); the recipes above carry callables only.  forcing: as in
    `reaction_diffusion_1d_discretized`; its source returns the stacked values of all species."""
    diffusion_rates = tuple(float(r) for r in diffusion_rates)
    if len(diffusion_rates) != reaction.ncomp:
        raise ValueError(f"expected {reaction.ncomp} diffusion rates, one per species, got {len(diffusion_rates)}")
    if bbox is None:
        bbox = [0.0, 1.0]
    bbox = np.asarray(bbox, dtype=np.float64)
    f, df, df_diagonal = reaction.callables()
    laplace = diffops.laplace()
    pde = problems.SystemSemiLinearEvolutionNeumann(
        diffop=(laplace,) * reaction.ncomp, diffop_scale=diffusion_rates, bbox=bbox, t0=t0, tmax=tmax, y0_fun=y0_fun, f=f,
        df=df, df_diagonal=df_diagonal)
    pde.reaction = reaction
    mesh_spatial = mesh.RectangularMesh.from_bbox_1d(pde.bbox, step=dx)
    if kernel is None:
        kernel = kernels.SquareExponential()
    pde.discretize_system(mesh_spatial=mesh_spatial, kernel=kernel, stencil_size_interior=stencil_size_interior,
                          stencil_size_boundary=stencil_size_boundary, nugget_gram_matrix=nugget_gram_matrix_fd)
    return _forcing.attach(pde, forcing, f)


def lotka_volterra_y0(x):
    """The initial values of `lotka_volterra_1d`."""
    return np.concatenate((5 * np.ones_like(x), 20.0 * gaussian_bell_1d(x)))


def sir_y0(x, bbox=(0.0, 1.0), N=1000.0):
    """The initial values of `sir_1d`."""
    init_infectious = 200.0 * gaussian_bell_1d_centered(x, bbox, width=0.5) + 1.0
    return np.concatenate((N * np.ones_like(init_infectious) - init_infectious, init_infectious,
                           np.zeros_like(init_infectious)))


# Initial-condition defaults; they adhere to Dirichlet conditions (examples.py:344-357)


def gaussian_bell_1d_centered(x, bbox, width=1.0):
    midpoint = 0.5 * (bbox[1] + bbox[0])
    return np.exp(-((x - midpoint) ** 2) / width ** 2)


def gaussian_bell_1d(x):
    return np.exp(-(x ** 2))


def sin_bell_1d(x):
    return 0.1 * np.sin(np.pi * x)
