"""Driven problems: a time-dependent source and time-dependent boundary values (beyond the reference, whose problems are
autonomous with B u = 0).

u_t = L u + r(u) + s(t, x) on the mesh, B u = g(t) on the boundary rows.  A `Forcing` carries the two callables; the problem
recipes of `pnmol.pde.examples` take one (`forcing=`) and hang it on the problem as `pde.forcing`.  The solvers measure the step
that lands on t against rhs(t) = [s(t, X) (d); g(t) (nB)] (`pnmol_filter_set_forcing`, `pnmol_filter_force_at`; DESIGN.md
section 25).
"""

import numpy as np


class Forcing:
    """source(t, X) -> (d,): the source at the mesh points `X = pde.mesh_spatial.points` (for a system of C species: the stacked
    values [s_0; ...; s_{C-1}], d = C N).  boundary_values(t) -> (nB,): the values g(t) of the boundary rows `pde.B u`, Dirichlet
    values or prescribed fluxes, in the order of the rows.  None: zeros."""

    def __init__(self, source=None, boundary_values=None):
        for name, fn in (("source", source), ("boundary_values", boundary_values)):
            if fn is not None and not callable(fn):
                raise TypeError(f"Forcing: {name} must be callable or None, got {type(fn).__name__}")
        self.source = source
        self.boundary_values = boundary_values

    @staticmethod
    def _checked(values, size, what, t):
        v = np.asarray(values, dtype=np.float64)
        if v.shape != (size,):
            raise ValueError(f"forcing: {what} at t={t} must have shape ({size},), got {v.shape}")
        if not np.all(np.isfinite(v)):
            raise ValueError(f"forcing: {what} at t={t} has entries that are not finite")
        return v

    def source_values(self, t, pde):
        """s(t, X) (d,), validated."""
        d = pde.L.shape[0]
        if self.source is None:
            return np.zeros(d)
        return self._checked(self.source(t, pde.mesh_spatial.points), d, "source(t, X)", t)

    def boundary(self, t, pde):
        """g(t) (nB,), validated."""
        nB = pde.B.shape[0]
        if self.boundary_values is None:
            return np.zeros(nB)
        return self._checked(self.boundary_values(t), nB, "boundary_values(t)", t)

    def rhs(self, t, pde):
        """[s(t, X); g(t)] (m,): what the step that lands on t measures against."""
        return np.concatenate((self.source_values(t, pde), self.boundary(t, pde)))

    def table(self, ts, pde):
        """(T, m) for the T steps of the time grid `ts` (T + 1,): row k belongs to the step that lands on ts[k + 1]."""
        ts = np.asarray(ts, dtype=np.float64)
        if ts.ndim != 1 or ts.size < 1:
            raise ValueError(f"forcing: ts must be a 1-d time grid, got shape {ts.shape}")
        m = pde.L.shape[0] + pde.B.shape[0]
        if ts.size == 1:
            return np.zeros((0, m))
        return np.stack([self.rhs(t, pde) for t in ts[1:]])


def attach(pde, forcing, f=None):
    """Hang `forcing` (None: nothing happens) on a problem of a recipe: `pde.forcing`, and `pde.f` with the source added (`f`: the
    unforced callable; the Jacobian does not change), so that the host-callable route and the oracle see the same PDE."""
    if forcing is None:
        return pde
    if not isinstance(forcing, Forcing):
        raise TypeError(f"forcing must be a pnmol.pde.forcing.Forcing or None, got {type(forcing).__name__}")
    pde.forcing = forcing
    if f is not None and forcing.source is not None:
        pde.f = lambda t, x: np.asarray(f(t, x), dtype=np.float64) + forcing.source_values(t, pde)
    return pde
