"""`pnmol_filter_set_operator` (dense M) and `pnmol_filter_set_operator_diagonal` (M = L + diag(j), L the operator given at
creation) interleaved in any order on one filter, with steps between the calls, through `step` and the graph-replayed
`steps`.  Every step is checked bit for bit against a twin filter, created with the same L, that receives every operator
as a dense upload (L + diag(j) for a diagonal call), and the steps after a diagonal call also against the oracle's
step with that operator.  The dense operators are chosen where the ELL image of the device can go wrong:
L's width with other off-diagonal values, L's width with one row's pattern moved (an entry set to exactly 0, a new one
elsewhere: the diagonal sits in another ELL slot), and a wider stencil.  Run with -m gpu."""

import types

import numpy as np
import pytest

import pnmol
import pnmol_oracle as oracle
from pnmol import _hip

pytestmark = pytest.mark.gpu

N, NU, DT = 48, 2, 2.0 ** -6


def _setup(ctx):
    kw = dict(tmax=1.0, dx=1.0 / (N - 1), diffusion_rate=0.05, bcond="dirichlet", stencil_size_interior=3,
              stencil_size_boundary=3)
    pde = pnmol.pde.examples.spruce_budworm_1d_discretized(kernel=pnmol.kernels.SquareExponential(),
                                                           nugget_gram_matrix_fd=0.0, **kw)
    solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=NU, steprule=pnmol.odetools.step.Constant(DT),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    state0 = solver.initialize(pde)
    gamma = solver.initialize_iwp(pde)[3]
    filters = [_hip.Filter(ctx, L=pde.L, B=pde.B, E_sqrtm=pde.E_sqrtm, R_sqrtm=pde.R_sqrtm, Gamma=gamma,
                           num_derivatives=NU, K=solver._gram) for _ in range(2)]
    mean0, cov0 = state0.y.mean.copy(), state0.y.device_state.cov()
    states = []
    for f in filters:
        s = f.new_state()
        s.set(state0.t, mean0, cov0)
        states.append(s)
    osolver = oracle.WhiteNoiseEK1(num_derivatives=NU, semilinear=True, steprule=oracle.Constant(DT),
                                   spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
    osolver.iwp, osolver.E0, osolver.E1, _ = osolver.initialize_iwp(pde)
    return pde, filters, states, osolver


def _operators(L):
    """M1: L's pattern, other off-diagonal values; M2: L's width, row i's pattern moved (diagonal in another slot);
    M3: a wider stencil."""
    d = L.shape[0]
    off = (L != 0) & ~np.eye(d, dtype=bool)
    M1 = L.copy()
    M1[off] *= 1.25
    i = d // 2
    assert L[i, i - 1] != 0 and L[i, i] != 0 and L[i, i + 1] != 0 and L[i, i + 2] == 0
    assert (L != 0).sum(axis=1).max() == 3
    M2 = L.copy()
    M2[i, i - 1] = 0.0
    M2[i, i + 2] = 0.5 * L[i, i + 1]
    assert (M2 != 0).sum(axis=1).max() == 3
    M3 = L.copy()
    for k in range(2, d - 2):
        M3[k, k - 2] = M3[k, k + 2] = 0.1 * L[k, k + 1]
    return M1, M2, M3


def _oracle_steps(osolver, pde, M, shift, mean, cov, t, k):
    """k covariance-form oracle steps from the device state's (mean, cov) with H_ode = E1 - M E0 and z's shift `shift`
    (the semilinear evaluate_ode with L = 0, J_x = M, f(x) = M x - shift): (mean (n, d), marginal variances (n, d),
    error) per step.  (sigma^2 is held to the twin only: the reference's own sigma^2 depends on the square-root factor
    of the input -- quirk Q1, pnmol_oracle.WhiteNoiseEK1.attempt_step -- and the device Cholesky of a covariance with
    directions of zero variance is not accurate enough to carry a 1e-10 comparison.)"""
    opde = types.SimpleNamespace(L=np.zeros_like(M), B=pde.B, E_sqrtm=pde.E_sqrtm, R_sqrtm=pde.R_sqrtm, y0=pde.y0,
                                 f=lambda _t, x: M @ x - shift, df=lambda _t, x: M)
    out = []
    for _ in range(k):
        mean, cov, _, err = oracle.covariance_form_step(osolver, opde, mean, cov, DT, t)
        t = t + DT
        out.append((mean, np.diag(cov).reshape(mean.shape, order="F"), err))
    return out


class _Run:
    """One state chain on the filter under test (operators as given) and on the twin (dense uploads only)."""

    def __init__(self, ctx):
        self.pde, (self.f, self.twin), (self.s, self.ts), self.osolver = _setup(ctx)
        self.L = self.pde.L
        for flt in (self.f, self.twin):
            flt.prepare_error_model(DT)
        self.op = (self.L, np.zeros(N))   # the operator both filters have now (dense form)
        self.after_diagonal = False

    def dense(self, M, shift):
        for flt in (self.f, self.twin):
            flt.set_operator(M, shift)
            flt.prepare_error_model(DT)
        self.op, self.after_diagonal = (M, shift), False

    def diagonal(self, j, shift):
        self.f.set_operator_diagonal(j, shift)
        self.f.prepare_error_model(DT)
        M = self.L + np.diag(j)
        self.twin.set_operator(M, shift)
        self.twin.prepare_error_model(DT)
        self.op, self.after_diagonal = (M, shift), True

    def _oracle(self, k):
        return _oracle_steps(self.osolver, self.pde, *self.op, self.s.mean(), self.s.cov(), self.s.t, k)

    def step(self):
        ref = self._oracle(1)[-1] if self.after_diagonal else None
        a, ia, ea = self.f.step(self.s, DT)
        b, ib, eb = self.twin.step(self.ts, DT)
        ma, va, mb, vb = a.mean(), a.marginal_var(), b.mean(), b.marginal_var()
        assert np.array_equal(ma, mb) and np.array_equal(va, vb) and np.array_equal(ea, eb)
        assert ia.diffusion_squared_local == ib.diffusion_squared_local and ia.t_new == ib.t_new
        if ref is not None:
            om, ovar, oerr = ref
            np.testing.assert_allclose(ma, om, rtol=1e-8, atol=1e-10 * np.abs(om).max())
            np.testing.assert_allclose(va, ovar, rtol=1e-6, atol=1e-9 * np.abs(ovar).max())
            np.testing.assert_allclose(ea, oerr, rtol=1e-7, atol=1e-10 * np.abs(oerr).max())
        self.s, self.ts = a, b

    def steps(self, k):
        ref = self._oracle(k) if self.after_diagonal else None
        ma, sa, ia = self.f.steps(self.s, k, DT)
        mb, sb, ib = self.twin.steps(self.ts, k, DT)
        assert np.array_equal(ma, mb) and np.array_equal(sa, sb)
        assert [x.diffusion_squared_local for x in ia] == [x.diffusion_squared_local for x in ib]
        assert np.array_equal(self.s.mean(), self.ts.mean()) and np.array_equal(self.s.cov(), self.ts.cov())
        if ref is not None:
            om = np.array([r[0][0] for r in ref])
            np.testing.assert_allclose(ma, om, rtol=1e-8, atol=1e-10 * np.abs(om).max())


def test_dense_then_diagonal_in_any_order(hip_ctx):
    """dense M1 (L's width and pattern) -> diagonal j1; dense M2 (L's width, a row's pattern moved) -> diagonal j2;
    dense M3 (wider) -> diagonal j3; then diagonal -> diagonal.  One step between all calls."""
    run = _Run(hip_ctx)
    rng = np.random.default_rng(7)
    M1, M2, M3 = _operators(run.L)
    run.step()
    for M in (M1, M2, M3):
        run.dense(M, 0.1 * rng.uniform(-1, 1, N))
        run.step()
        run.diagonal(rng.uniform(-1, 1, N), 0.1 * rng.uniform(-1, 1, N))
        run.step()
        run.step()
    run.diagonal(rng.uniform(-1, 1, N), 0.1 * rng.uniform(-1, 1, N))
    run.step()


@pytest.mark.parametrize("M_of", [0, 1, 2])
def test_diagonal_dense_alternating_with_graph_replayed_steps(hip_ctx, M_of):
    """diagonal -> dense -> diagonal -> dense, each followed by `steps` (graphs captured before an operator change are
    replayed after it when the width stays: the restore of L's image goes into the same buffers) and by one `step`."""
    run = _Run(hip_ctx)
    rng = np.random.default_rng(11 + M_of)
    M = _operators(run.L)[M_of]
    for _ in range(2):
        run.diagonal(rng.uniform(-1, 1, N), 0.1 * rng.uniform(-1, 1, N))
        run.steps(12)
        run.step()
        run.dense(M, 0.1 * rng.uniform(-1, 1, N))
        run.steps(12)
        run.step()
