"""Time-dependent operators (beyond the reference, whose operators are constant): u_t = sum_r a_r(t) L_r u.

A few fixed stencil operators L_r with scalar coefficients a_r(t): a conductivity that rises and falls, transport in an oscillating
flow.  A `TimeDependentOperator` carries the operators, the diagonals of the FD uncertainties that `discretize.fd_probabilistic`
returned with them, and the callable t -> (a_0, ..., a_{R-1}); the problem recipes of `pnmol.pde.examples` hang it on the problem as
`pde.time_dependent_operator`.  The solvers run the step that lands on t with M(t) and the noise
E(t) E(t)^T = diag(sum_r (a_r(t) e_{r,i})^2) (`pnmol_filter_set_operator_family`, `_set_operator_schedule`, `_operator_at`; DESIGN.md
section 27).

`matrix`, `noise_sqrtm` and `table` use the arithmetic of the device kernel in its order -- v = a_0 V_0, then v = v + a_r V_r in
ascending r, every product and sum rounded on its own -- so that host and device form the same operator, bit for bit.
"""

import numpy as np

MAX_OPERATORS = 4       # PNMOL_OPERATOR_MAXR (include/pnmol_hip.h)


class TimeDependentOperator:
    """operators: (R, d, d), R <= 4.  noise_diagonals: (R, d), or (R, d, d) diagonal matrices E_sqrtm_r.  coefficients: callable
    t -> (R,) (a scalar for R = 1)."""

    def __init__(self, operators, noise_diagonals, coefficients):
        L = np.array(operators, dtype=np.float64)
        if L.ndim == 2:
            L = L[None]
        if L.ndim != 3 or L.shape[1] != L.shape[2]:
            raise ValueError(f"TimeDependentOperator: operators must be (R, d, d), got {L.shape}")
        R, d = L.shape[0], L.shape[1]
        if not 1 <= R <= MAX_OPERATORS:
            raise ValueError(f"TimeDependentOperator: R = {R} operators, supported are 1 <= R <= {MAX_OPERATORS}")
        e = np.array(noise_diagonals, dtype=np.float64)
        if R == 1 and e.shape != (R, d) and e.shape in ((d,), (d, d)):
            e = e[None]
        if e.shape == (R, d, d):
            off = e - np.stack([np.diag(np.diag(x)) for x in e])
            if np.any(off != 0.0):
                raise ValueError("TimeDependentOperator: only diagonal E_sqrtm are accepted (an off-diagonal entry is not zero)")
            e = np.stack([np.diag(x) for x in e])
        if e.shape != (R, d):
            raise ValueError(f"TimeDependentOperator: noise_diagonals must be (R, d) or (R, d, d) = ({R}, {d}[, {d}]), got {e.shape}")
        if not np.all(np.isfinite(L)):
            r, i, k = np.argwhere(~np.isfinite(L))[0]
            raise ValueError(f"TimeDependentOperator: operator {r} is not finite at row {i}, column {k}")
        if not np.all(np.isfinite(e)):
            r, i = np.argwhere(~np.isfinite(e))[0]
            raise ValueError(f"TimeDependentOperator: the noise diagonal of operator {r} is not finite at row {i}")
        if not callable(coefficients):
            raise TypeError(f"TimeDependentOperator: coefficients must be callable, got {type(coefficients).__name__}")
        self.operators = np.ascontiguousarray(L)
        self.noise_diagonals = np.ascontiguousarray(e)
        self._coefficients = coefficients

    @property
    def num_operators(self):
        return self.operators.shape[0]

    def coefficients(self, t):
        """(a_0(t), ..., a_{R-1}(t)) as a (R,) array, validated."""
        a = np.atleast_1d(np.asarray(self._coefficients(t), dtype=np.float64))
        if a.shape != (self.num_operators,):
            raise ValueError(f"time-dependent operator: coefficients(t) at t={t} must have shape ({self.num_operators},), got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"time-dependent operator: coefficients(t) at t={t} has entries that are not finite")
        return a

    def combine(self, a):
        """sum_r a_r L_r in the kernel's order of operations."""
        a = np.asarray(a, dtype=np.float64)
        M = a[0] * self.operators[0]
        for r in range(1, self.num_operators):
            M = M + a[r] * self.operators[r]
        return M

    def noise_diagonal(self, a):
        """sqrt(sum_r (a_r e_r)^2) (d,): the squares summed in the kernel's order of operations, then one square root."""
        a = np.asarray(a, dtype=np.float64)
        t = a[0] * self.noise_diagonals[0]
        q = t * t
        for r in range(1, self.num_operators):
            t = a[r] * self.noise_diagonals[r]
            q = q + t * t
        return np.sqrt(q)

    def matrix(self, t):
        """M(t) (d, d)."""
        return self.combine(self.coefficients(t))

    def noise_sqrtm(self, t):
        """E_sqrtm(t) (d, d) diagonal: E E^T is the noise of the PDE rows of the step that lands on t."""
        return np.diag(self.noise_diagonal(self.coefficients(t)))

    def table(self, ts):
        """(T, R) for the T steps of the time grid `ts` (T + 1,): row k belongs to the step that lands on ts[k + 1]."""
        ts = np.asarray(ts, dtype=np.float64)
        if ts.ndim != 1 or ts.size < 1:
            raise ValueError(f"time-dependent operator: ts must be a 1-d time grid, got shape {ts.shape}")
        if ts.size == 1:
            return np.zeros((0, self.num_operators))
        return np.stack([self.coefficients(t) for t in ts[1:]])


def attach(pde, operator):
    """Hang `operator` on a problem of a recipe: `pde.time_dependent_operator`, with `pde.L` = M(t0) and `pde.E_sqrtm` = E(t0), so
    that `initialize` needs nothing new."""
    if not isinstance(operator, TimeDependentOperator):
        raise TypeError(f"expected a pnmol.pde.coefficients.TimeDependentOperator, got {type(operator).__name__}")
    if operator.operators.shape[1:] != pde.L.shape:
        raise ValueError(f"the operators are {operator.operators.shape[1:]}, the problem's L is {pde.L.shape}")
    pde.time_dependent_operator = operator
    pde.L = operator.matrix(pde.t0)
    pde.E_sqrtm = operator.noise_sqrtm(pde.t0)
    return pde
