"""Pointwise reaction terms r(u) = P(u) + A(u) / B(u) that the device evaluates itself.

A semilinear problem u_t = L u + f(t, u) whose f is a Python callable costs the EK1 a host round trip per step (predicted
mean back, f and df in NumPy, new diagonal up).  The reactions people solve on a mesh are mostly pointwise and rational --
logistic / Fisher-KPP, Allen-Cahn, Nagumo, the spruce-budworm predation term -- so a few coefficients describe them, and
`pnmol_filter_set_reaction` (include/pnmol_hip.h) hands those to the kernel that linearises on the device
(csrc/pnmol_reaction.hip).  No reference counterpart: the reference's problems carry callables only.

`Reaction.value` / `Reaction.derivative` are the host form of the same arithmetic (Horner, one rounding per operation,
r' = P' + (A' B - A B') / B^2), in the kernel's order of operations.

`SystemReaction` (further down) is the coupled form for up to four species on one mesh -- Lotka-Volterra, SIR, Gray-Scott --,
handed over by `pnmol_filter_set_reaction_system` and linearised by k_linearize_system.

`Convection` is a Burgers-type term c(u) (G u) + r(u) with a stencil operator G -- viscous Burgers, Burgers-Fisher --, handed
over by `pnmol_filter_set_convection` and linearised by k_linearize_convection.
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


def _coefficients(name, c, who="Reaction"):
    c = np.atleast_1d(np.asarray(c, dtype=np.float64))
    if c.ndim != 1:
        raise ValueError(f"{who}: {name} must be a 1-d sequence of scalar coefficients, got shape {c.shape}")
    if c.size > MAXDEG + 1:
        raise ValueError(f"{who}: {name} has degree {c.size - 1}, the largest supported is {MAXDEG}")
    if not np.all(np.isfinite(c)):
        raise ValueError(f"{who}: {name} has a coefficient that is not finite")
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


# ---------------------------------------------------------------------------------------------------------------------------
# Convection terms: f(u)_i = c(u_i) (G u)_i + r(u_i) with a stencil operator G (a discretised gradient) -- viscous Burgers,
# Burgers-Fisher, advection-reaction (`pnmol_filter_set_convection`, k_linearize_convection).  The Jacobian
# diag(c) G + diag(c' G u + r') is not diagonal: the linearisation rewrites every entry of a stencil row.


class ConvectionDesc(ctypes.Structure):
    """`pnmol_convection` of include/pnmol_hip.h."""

    _fields_ = [("deg_c", ctypes.c_int), ("c", ctypes.c_double * (MAXDEG + 1)), ("r", ReactionDesc)]


class Convection:
    """f(u)_i = c(u_i) (G u)_i + r(u_i): `speed` holds the coefficients of c in ascending powers (scalars, the same at every
    mesh point; degree <= 7), `reaction` is an optional `Reaction` r.  The (d, d) stencil matrix G belongs to a mesh: the problem
    recipe (`pde.examples.convection_diffusion_1d_discretized`) sets it with `set_operator`.

    `linearization` is the host form of the device arithmetic, in its order of operations (every operation rounded on its own):
    g = G u summed over the non-zero entries of each row of G in ascending column order, starting from the first product; c, c',
    r, r' by Horner; q = c' g + r' (c' g alone without a reaction); off-diagonal entries L_ij + c_i G_ij, the diagonal entry
    (L_ii + c_i G_ii) + q_i; shift q u - r (the c g terms of J u - f cancel and are never formed)."""

    def __init__(self, speed, reaction=None):
        if np.size(speed) == 0:
            raise ValueError("Convection: speed is empty; a term without convection is a Reaction")
        self.speed = _coefficients("speed", speed, who="Convection")
        if reaction is not None and not isinstance(reaction, Reaction):
            raise TypeError(f"Convection: reaction must be a Reaction or None, got {type(reaction).__name__}")
        self.reaction = reaction
        self._G = None
        self._ell = None

    def __repr__(self):
        shape = None if self._G is None else self._G.shape
        return f"Convection(speed={self.speed!r}, reaction={self.reaction!r}, G={shape})"

    # ------------------------------------------------------------------ the discretised operator
    @property
    def G(self):
        return self._G

    def set_operator(self, G):
        """The stencil matrix G, (d, d): kept with its rows in compressed form (non-zero entries in ascending column order)."""
        G = np.array(G, dtype=np.float64)
        if G.ndim != 2 or G.shape[0] != G.shape[1]:
            raise ValueError(f"Convection: G must be a square matrix, got shape {G.shape}")
        if not np.all(np.isfinite(G)):
            raise ValueError("Convection: G has an entry that is not finite")
        d = G.shape[0]
        nz = G != 0.0
        count = nz.sum(axis=1)
        w = int(count.max()) if d else 0
        cols, vals = np.zeros((d, w), dtype=np.intp), np.zeros((d, w))
        for i in range(d):
            k = np.flatnonzero(nz[i])
            cols[i, :k.size], vals[i, :k.size] = k, G[i, k]
        self._G, self._ell = G, (cols, vals, count)
        return self

    def _has_reaction(self):
        return self.reaction is not None and (len(self.reaction.p) > 0 or self.reaction.a is not None)

    # ------------------------------------------------------------------ host arithmetic (the kernel's, in its order)
    def _state(self, u):
        if self._G is None:
            raise ValueError("Convection: no operator G yet (set_operator; the problem recipes set it)")
        u = np.asarray(u, dtype=np.float64)
        if u.shape != (self._G.shape[0],):
            raise ValueError(f"Convection: expected a vector of {self._G.shape[0]} entries, got shape {u.shape}")
        return u

    def _gradient(self, u):
        cols, vals, count = self._ell
        g = np.zeros_like(u)
        for e in range(cols.shape[1]):
            prod = vals[:, e] * u[cols[:, e]]
            g = np.where(e < count, prod if e == 0 else g + prod, g)
        return g

    def _parts(self, u):
        """(g, c, q, r) at u."""
        g = self._gradient(u)
        c, dc = _horner(self.speed, u)
        q = dc * g
        if self._has_reaction():
            r, dr = self.reaction._value_and_derivative(u)
            return g, c, q + dr, r
        return g, c, q, np.zeros_like(u)

    def value(self, u):
        """f(u) = c(u) (G u) + r(u)."""
        g, c, _, r = self._parts(self._state(u))
        return c * g + r if self._has_reaction() else c * g

    def linearization(self, u, L=None):
        """(J_rows, shift) of the EK1 linearisation at u: J_rows is the dense (d, d) matrix diag(c) G + diag(q) -- with `L` given,
        the operator M = L + J, formed entry by entry in the documented order -- and shift = q u - r = J u - f(u)."""
        u = self._state(u)
        _, c, q, r = self._parts(u)
        rows = c[:, None] * self._G
        if L is not None:
            L = np.asarray(L, dtype=np.float64)
            if L.shape != self._G.shape:
                raise ValueError(f"Convection: L has shape {L.shape}, G has shape {self._G.shape}")
            rows = L + rows
        idx = np.arange(u.size)
        rows[idx, idx] = rows[idx, idx] + q
        return rows, q * u - r

    def callables(self):
        """(f(t, u), df(t, u) as a dense matrix, None): what the problem classes take."""
        def f(_t, u):
            return self.value(u)

        def df(_t, u):
            return self.linearization(u)[0]

        return f, df, None

    # ------------------------------------------------------------------ C ABI
    def to_ctypes(self):
        desc = ConvectionDesc()
        desc.deg_c = len(self.speed) - 1
        for k, c in enumerate(self.speed):
            desc.c[k] = c
        if self.reaction is not None:
            desc.r = self.reaction.to_ctypes()
        else:
            desc.r.deg_p = desc.r.deg_a = desc.r.deg_b = -1
        return desc

    @classmethod
    def from_ctypes(cls, desc):
        r = desc.r
        absent = r.deg_p < 0 and r.deg_a < 0 and r.deg_b < 0
        return cls(tuple(desc.c[: desc.deg_c + 1]), None if absent else Reaction.from_ctypes(r))


# ---------------------------------------------------------------------------------------------------------------------------
# Coupled systems: C species on the same mesh, state [u_0; ...; u_{C-1}], r_c(u) = P_c(u) + A_c(u) / B_c(u) with u the C values at
# ONE mesh point (`pnmol_filter_set_reaction_system`, k_linearize_system).  The Jacobian is block-dense with diagonal blocks.

MAXCOMP = 4    # PNMOL_SYSTEM_MAXCOMP
MAXTERMS = 8   # PNMOL_SYSTEM_MAXTERMS
MAXPOW = 7


class MonomialDesc(ctypes.Structure):
    """`pnmol_monomial`."""

    _fields_ = [("coef", ctypes.c_double), ("pow", ctypes.c_int * MAXCOMP)]


class SystemPolyDesc(ctypes.Structure):
    """`pnmol_system_poly`."""

    _fields_ = [("nterms", ctypes.c_int), ("term", MonomialDesc * MAXTERMS)]


class SystemReactionDesc(ctypes.Structure):
    """`pnmol_reaction_system` of include/pnmol_hip.h."""

    _fields_ = [("ncomp", ctypes.c_int), ("p", SystemPolyDesc * MAXCOMP), ("a", SystemPolyDesc * MAXCOMP),
                ("b", SystemPolyDesc * MAXCOMP)]


def _system_poly(name, terms, ncomp):
    """Validated tuple of (coef, exponents) terms; exponents are padded to MAXCOMP."""
    terms = () if terms is None else tuple(terms)
    if len(terms) > MAXTERMS:
        raise ValueError(f"SystemReaction: {name} has {len(terms)} terms, the largest supported number is {MAXTERMS}")
    out = []
    for term in terms:
        try:
            coef, pw = term
            coef, pw = float(coef), tuple(int(e) for e in pw)
            exact = all(e == f for e, f in zip(pw, term[1]))
        except (TypeError, ValueError):
            raise ValueError(f"SystemReaction: a term of {name} is not (coefficient, exponents): {term!r}") from None
        if not exact or len(pw) > MAXCOMP:
            raise ValueError(f"SystemReaction: a term of {name} is not (coefficient, exponents): {term!r}")
        pw = pw + (0,) * (MAXCOMP - len(pw))
        if any(e < 0 or e > MAXPOW for e in pw):
            raise ValueError(f"SystemReaction: {name} has an exponent outside [0, {MAXPOW}]")
        if any(pw[ncomp:]):
            raise ValueError(f"SystemReaction: {name} has a non-zero exponent of a species >= ncomp = {ncomp}")
        if not np.isfinite(coef):
            raise ValueError(f"SystemReaction: {name} has a coefficient that is not finite")
        out.append((coef, pw))
    return tuple(out)


def _monomial(start, pw, less, u):
    """start * u_0^pw[0] * u_1^pw[1] * ..., one multiplication at a time; `less` takes one factor off that species."""
    m = np.full_like(u[0], start)
    for k in range(len(u)):
        for _ in range(pw[k] - (1 if k == less else 0)):
            m = m * u[k]
    return m


def _system_poly_eval(terms, u):
    """(value, [partial derivative by u_k for every k]) of a polynomial at the species values u (a list of arrays): the sum
    of the terms in the order given, starting from the first one."""
    v, dv = None, [None] * len(u)
    for coef, pw in terms:
        m = _monomial(coef, pw, -1, u)
        v = m if v is None else v + m
        for k in range(len(u)):
            if pw[k] >= 1:
                dm = _monomial(pw[k] * coef, pw, k, u)
                dv[k] = dm if dv[k] is None else dv[k] + dm
    zero = np.zeros_like(u[0])
    return (zero if v is None else v), [zero if x is None else x for x in dv]


class SystemReaction:
    """r_c(u) = P_c(u) + A_c(u) / B_c(u) for c < ncomp <= 4: `p`, `a`, `b` are per-component sequences of polynomials, each a
    sequence of at most 8 terms (coef, exponents) meaning coef * u_0^e_0 * u_1^e_1 ... (exponents 0..7, scalars the same at every
    mesh point; an empty sequence is the zero polynomial).  `a[c]` and `b[c]` come together or not at all (empty or None)."""

    def __init__(self, ncomp, p, a=None, b=None):
        ncomp = int(ncomp)
        if not 1 <= ncomp <= MAXCOMP:
            raise ValueError(f"SystemReaction: ncomp = {ncomp} is outside [1, {MAXCOMP}]")
        self.ncomp = ncomp
        if (a is None) != (b is None):
            raise ValueError("SystemReaction: the numerators a and the denominators b are given together or not at all")
        groups = {"p": p, "a": a if a is not None else [()] * ncomp, "b": b if b is not None else [()] * ncomp}
        for name, polys in groups.items():
            if len(polys) != ncomp:
                raise ValueError(f"SystemReaction: {name} has {len(polys)} entries for ncomp = {ncomp} components")
            setattr(self, name, tuple(_system_poly(f"{name}[{c}]", polys[c], ncomp) for c in range(ncomp)))
        for c in range(ncomp):
            if bool(self.a[c]) != bool(self.b[c]):
                raise ValueError(f"SystemReaction: the numerator a[{c}] and the denominator b[{c}] are given together or not "
                                 f"at all")
            if self.b[c] and not any(coef for coef, _ in self.b[c]):
                raise ValueError(f"SystemReaction: the denominator b[{c}] is identically zero")

    def __repr__(self):
        return f"SystemReaction(ncomp={self.ncomp}, p={self.p!r}, a={self.a!r}, b={self.b!r})"

    # ------------------------------------------------------------------ host arithmetic (the kernel's, in its order)
    def _species(self, u):
        u = np.asarray(u, dtype=np.float64)
        if u.ndim != 1 or u.shape[0] % self.ncomp:
            raise ValueError(f"SystemReaction: expected a vector of ncomp * N = {self.ncomp} * N entries, got shape {u.shape}")
        return list(u.reshape(self.ncomp, -1))

    def _value_and_jacobian(self, u):
        u = self._species(u)
        C = self.ncomp
        r, J = [], []
        for c in range(C):
            P, dP = _system_poly_eval(self.p[c], u)
            if self.a[c]:
                A, dA = _system_poly_eval(self.a[c], u)
                B, dB = _system_poly_eval(self.b[c], u)
                r.append(P + A / B)
                J.append([dP[k] + (dA[k] * B - A * dB[k]) / (B * B) for k in range(C)])
            else:
                r.append(P)
                J.append(dP)
        return u, np.array(r), np.array(J)

    def value(self, u):
        """r at the state u = [u_0; ...; u_{C-1}] (C N entries): C N entries."""
        return self._value_and_jacobian(u)[1].reshape(-1)

    def jacobian_blocks(self, u):
        """(C, C, N): entry [c, k, j] = d r_c / d u_k at mesh point j."""
        return self._value_and_jacobian(u)[2]

    def shift(self, u):
        """((J_c0 u_0 + J_c1 u_1) + ...) - r_c: the shift of the EK1 linearisation at u (C N entries)."""
        us, r, J = self._value_and_jacobian(u)
        out = []
        for c in range(self.ncomp):
            acc = J[c, 0] * us[0]
            for k in range(1, self.ncomp):
                acc = acc + J[c, k] * us[k]
            out.append(acc - r[c])
        return np.array(out).reshape(-1)

    def jacobian(self, u):
        """The dense (C N, C N) Jacobian: a block matrix of diagonals."""
        J = self.jacobian_blocks(u)
        C, N = self.ncomp, J.shape[2]
        out = np.zeros((C * N, C * N))
        idx = np.arange(N)
        for c in range(C):
            for k in range(C):
                out[c * N + idx, k * N + idx] = J[c, k]
        return out

    def callables(self):
        """(f(t, u), df(t, u) as a dense block matrix of diagonals, None): what the system problem classes take."""
        def f(_t, u):
            return self.value(u)

        def df(_t, u):
            return self.jacobian(u)

        return f, df, None

    # ------------------------------------------------------------------ C ABI
    def to_ctypes(self):
        desc = SystemReactionDesc()
        desc.ncomp = self.ncomp
        for dst, src in ((desc.p, self.p), (desc.a, self.a), (desc.b, self.b)):
            for c in range(self.ncomp):
                dst[c].nterms = len(src[c])
                for t, (coef, pw) in enumerate(src[c]):
                    dst[c].term[t].coef = coef
                    for k in range(MAXCOMP):
                        dst[c].term[t].pow[k] = pw[k]
        return desc

    @classmethod
    def from_ctypes(cls, desc):
        C = desc.ncomp

        def polys(group):
            return [[(group[c].term[t].coef, tuple(group[c].term[t].pow)) for t in range(group[c].nterms)] for c in range(C)]

        return cls(C, polys(desc.p), polys(desc.a), polys(desc.b))


def lotka_volterra(a=0.5, b=0.05, c=0.05, d=0.5):
    """Predator-prey: (a u - b u v, c u v - d v)."""
    return SystemReaction(2, p=[[(a, (1, 0)), (-b, (1, 1))], [(c, (1, 1)), (-d, (0, 1))]])


def sir(beta=0.3, gamma=0.07):
    """(-beta s i / (s + i + r), beta s i / (s + i + r) - gamma i, gamma i): no pole while the population is positive."""
    total = [(1.0, (1, 0, 0)), (1.0, (0, 1, 0)), (1.0, (0, 0, 1))]
    return SystemReaction(3, p=[[], [(-gamma, (0, 1, 0))], [(gamma, (0, 1, 0))]],
                          a=[[(-beta, (1, 1, 0))], [(beta, (1, 1, 0))], []], b=[total, total, []])


def gray_scott(feed, kill):
    """(-u v^2 + feed (1 - u), u v^2 - (feed + kill) v)."""
    return SystemReaction(2, p=[[(-1.0, (1, 2)), (feed, (0, 0)), (-feed, (1, 0))], [(1.0, (1, 2)), (-(feed + kill), (0, 1))]])


def logistic(rate=1.0):
    """Fisher-KPP / logistic growth: rate * u (1 - u)."""
    return Reaction(p=(0.0, rate, -rate))


def burgers():
    """The convection term of viscous Burgers, u_t = kappa u_xx - u u_x: c(u) = -u."""
    return Convection((0.0, -1.0))


def burgers_fisher(rate=1.0):
    """Burgers-Fisher, u_t = kappa u_xx - u u_x + rate u (1 - u): `burgers` with the logistic reaction."""
    return Convection((0.0, -1.0), reaction=logistic(rate))


def allen_cahn():
    """u - u^3."""
    return Reaction(p=(0.0, 1.0, 0.0, -1.0))


def nagumo(alpha):
    """u (1 - u) (u - alpha) = -alpha u + (1 + alpha) u^2 - u^3."""
    return Reaction(p=(0.0, -alpha, 1.0 + alpha, -1.0))


def budworm(growth, capacity):
    """Spruce budworm with predation: growth * u (1 - u / capacity) - u^2 / (1 + u^2)."""
    return Reaction(p=(0.0, growth, -growth / capacity), a=(0.0, 0.0, -1.0), b=(1.0, 0.0, 1.0))
