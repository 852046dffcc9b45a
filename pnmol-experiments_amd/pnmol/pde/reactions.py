"""Pointwise reaction terms r(u) = P(u) + A(u) / B(u) that the device evaluates itself.

A semilinear problem u_t = L u + f(t, u) whose f is a Python callable costs the EK1 a host round trip per step (predicted
mean back, f and df in NumPy, new diagonal up).  The reactions people solve on a mesh are mostly pointwise and rational --
logistic / Fisher-KPP, Allen-Cahn, Nagumo, the spruce-budworm predation term -- so a few coefficients describe them, and
`pnmol_filter_set_reaction` (include/pnmol_hip.h) hands those to the kernel that linearises on the device
(csrc/pnmol_reaction.hip).  No reference counterpart: the reference's problems carry callables only.

`Reaction.value` / `Reaction.derivative` are the host form of the same arithmetic (Horner, one rounding per operation,
r' = P' + (A' B - A B') / B^2), in the kernel's order of operations.
"""

import ctypes

import numpy as np

MAXDEG = 7   # PNMOL_REACTION_MAXDEG


class ReactionDesc(ctypes.Structure):
    """`pnmol_reaction` of include/pnmol_hip.h."""

    _fields_ = [
        ("deg_p", ctypes.c_int),
        ("deg_a", ctypes.c_int),
        ("deg_b", ctypes.c_int),
        ("p", ctypes.c_double * (MAXDEG + 1)),
        ("a", ctypes.c_double * (MAXDEG + 1)),
        ("b", ctypes.c_double * (MAXDEG + 1)),
    ]


def _coefficients(name, c):
    c = np.atleast_1d(np.asarray(c, dtype=np.float64))
    if c.ndim != 1:
        raise ValueError(f"Reaction: {name} must be a 1-d sequence of scalar coefficients, got shape {c.shape}")
    if c.size > MAXDEG + 1:
        raise ValueError(f"Reaction: {name} has degree {c.size - 1}, the largest supported is {MAXDEG}")
    if not np.all(np.isfinite(c)):
        raise ValueError(f"Reaction: {name} has a coefficient that is not finite")
    return tuple(float(x) for x in c)


def _horner(c, u):
    """(value, derivative) of the polynomial with ascending coefficients c at u; an empty c is the zero polynomial."""
    v, dv = np.zeros_like(u), np.zeros_like(u)
    deg = len(c) - 1
    if deg < 0:
        return v, dv
    v = v + c[deg]
    for k in range(deg - 1, -1, -1):
        v = v * u + c[k]
    if deg < 1:
        return v, dv
    dv = dv + deg * c[deg]
    for k in range(deg - 1, 0, -1):
        dv = dv * u + k * c[k]
    return v, dv


class Reaction:
    """r(u) = P(u) + A(u) / B(u): `p`, `a`, `b` are the coefficients of P, A, B in ascending powers (scalars, the same at
    every mesh point; degree <= 7).  `a` and `b` come together or not at all; an empty `p` is P = 0."""

    def __init__(self, p=(), a=None, b=None):
        if (a is None) != (b is None):
            raise ValueError("Reaction: the numerator a and the denominator b are given together or not at all")
        self.p = _coefficients("p", p) if len(np.atleast_1d(p)) else ()
        for name, c in (("a", a), ("b", b)):
            if c is not None and np.size(c) == 0:
                raise ValueError(f"Reaction: {name} is empty; leave a and b out for a reaction without a rational term")
        self.a = None if a is None else _coefficients("a", a)
        self.b = None if b is None else _coefficients("b", b)
        if self.b is not None and not any(self.b):
            raise ValueError("Reaction: the denominator b is identically zero")

    def __repr__(self):
        return f"Reaction(p={self.p!r}, a={self.a!r}, b={self.b!r})"

    # ------------------------------------------------------------------ host arithmetic (the kernel's, in its order)
    def _value_and_derivative(self, u):
        u = np.asarray(u, dtype=np.float64)
        r, dr = _horner(self.p, u)
        if self.a is not None:
            A, dA = _horner(self.a, u)
            B, dB = _horner(self.b, u)
            r = r + A / B
            dr = dr + (dA * B - A * dB) / (B * B)
        return r, dr

    def value(self, u):
        return self._value_and_derivative(u)[0]

    def derivative(self, u):
        return self._value_and_derivative(u)[1]

    def callables(self):
        """(f(t, u), df(t, u) as a dense diagonal matrix, df_diagonal(t, u)): what the problem classes take."""
        def f(_t, u):
            return self.value(u)

        def df(_t, u):
            return np.diag(self.derivative(u))

        def df_diagonal(_t, u):
            return self.derivative(u)

        return f, df, df_diagonal

    # ------------------------------------------------------------------ C ABI
    def to_ctypes(self):
        desc = ReactionDesc()
        desc.deg_p = len(self.p) - 1
        desc.deg_a = -1 if self.a is None else len(self.a) - 1
        desc.deg_b = -1 if self.b is None else len(self.b) - 1
        for dst, src in ((desc.p, self.p), (desc.a, self.a or ()), (desc.b, self.b or ())):
            for k, c in enumerate(src):
                dst[k] = c
        return desc

    @classmethod
    def from_ctypes(cls, desc):
        p = tuple(desc.p[: desc.deg_p + 1])
        if desc.deg_a < 0 and desc.deg_b < 0:
            return cls(p=p)
        return cls(p=p, a=tuple(desc.a[: desc.deg_a + 1]), b=tuple(desc.b[: desc.deg_b + 1]))


def logistic(rate=1.0):
    """Fisher-KPP / logistic growth: rate * u (1 - u)."""
    return Reaction(p=(0.0, rate, -rate))


def allen_cahn():
    """u - u^3."""
    return Reaction(p=(0.0, 1.0, 0.0, -1.0))


def nagumo(alpha):
    """u (1 - u) (u - alpha) = -alpha u + (1 + alpha) u^2 - u^3."""
    return Reaction(p=(0.0, -alpha, 1.0 + alpha, -1.0))


def budworm(growth, capacity):
    """Spruce budworm with predation: growth * u (1 - u / capacity) - u^2 / (1 + u^2)."""
    return Reaction(p=(0.0, growth, -growth / capacity), a=(0.0, 0.0, -1.0), b=(1.0, 0.0, 1.0))
