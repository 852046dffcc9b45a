/* pnmol_hip.h -- C ABI of the MI355X-native PNMOL white-noise EK1 filter step.
 *
 * The reference (schmidtjonathan/pnmol-experiments) is pure Python/JAX and has no
 * FFI of its own; its boundary for this path is the Python class
 * contract `pnmol.white.LinearWhiteNoiseEK1.{initialize,attempt_step,solve}`.  This header
 * is the C boundary a binding for that contract binds to; every entry point names the
 * reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - return 0 = ok, <0 = error: -1 bad argument, -2 HIP error, -3 innovation matrix not
 *     positive definite (see `pnmol_last_error`), -4 out of memory.
 *   - caller owns every host buffer; the library owns all device memory behind the
 *     opaque handles.  Matrices are row-major.
 *   - state vectors / covariances crossing this boundary use the reference's
 *     F-flattened order (`mean.reshape(-1, order="F")`, white.py:104): index j*n + i is
 *     derivative i at mesh point j.  `mean_nd` buffers are (n, d) row-major like
 *     `state.y.mean`.  Everything is in the NON-preconditioned ("raw") coordinates the
 *     reference's `PDEFilterState` carries.
 *   - one ctx <-> one device <-> one HIP stream.  A ctx is not thread-safe; different
 *     ctxs are independent (one thread or process per GPU).
 *   - Lifetimes: a handle keeps its parent alive.  Destroy in the order states -> filter(s) -> ctx.  A destroy call on
 *     a parent that still has live children does NOTHING and returns -1 (`pnmol_last_error` says how many children are
 *     left): `pnmol_filter_destroy` while any `pnmol_state`, `pnmol_samples` or `pnmol_bridge` of the filter lives, `pnmol_ctx_destroy` while any
 *     `pnmol_filter` / `pnmol_sqrt_filter` of the ctx lives, `pnmol_state_destroy` of the target of an unfinished
 *     `pnmol_filter_steps_begin`.  The handle stays valid after a refused destroy; call it again once the children are gone.
 *   - `pnmol_abi_version()` = 3 (1: before `pnmol_filter_desc.dtype`, the lifetime rule and `pnmol_filter_sweep_layout`;
 *     2: `pnmol_sqrt_filter_create` refused `dtype = 1`, which now selects the fp32 QR of include/pnmol_sqrt.h).
 *     `pnmol_smoother_step` and the joint draws (`pnmol_samples_*`, `pnmol_sample_noise`) were added within version 3:
 *     backwards-compatible additions, nothing existing changed.  So was the dense output (`pnmol_state_predict*`,
 *     `pnmol_smoother_step_bridge`, `pnmol_bridge_*`, `pnmol_samples_interpolate`, `pnmol_samples_clone`) and the measurement
 *     update (`pnmol_state_observe`), the recorder of the constant-step loop (`pnmol_filter_set_recorder`, `_recorder_pending`,
 *     `_recorder_means`), the one-call backward pass (`pnmol_smoother_steps`) and the linearisation points of the loop
 *     (`pnmol_filter_set_linearization_points`, `_linearization_pending`, `pnmol_filter_linearize_at`) and the posterior of
 *     linear functionals of the trajectory (`pnmol_functionals`), and the forcing of driven problems
 *     (`pnmol_filter_set_forcing`, `_forcing_pending`, `pnmol_filter_force_at`), and time-dependent operators
 *     (`pnmol_filter_set_operator_family`, `_set_operator_schedule`, `_operator_schedule_pending`, `pnmol_filter_operator_at`).
 *     Zero-initialise `pnmol_filter_desc`: unknown `dtype` values are rejected with -1.
 *   - dtype: fp64 (the reference runs with jax_enable_x64, src/pnmol/__init__.py:9-11); `pnmol_filter_desc.dtype = 1`
 *     keeps the covariance and its bulk kernels in fp32 (build-side option).
 */
#ifndef PNMOL_HIP_H
#define PNMOL_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pnmol_ctx pnmol_ctx;
typedef struct pnmol_filter pnmol_filter; /* model + workspace: L, B, E, R, Gamma, nu       */
typedef struct pnmol_state pnmol_state;   /* device-resident (mean, covariance, t)          */
typedef struct pnmol_samples pnmol_samples; /* S joint draws at one time point, device-resident */
typedef struct pnmol_bridge pnmol_bridge;   /* what dense output inside one step [t_k, t_k + dt] needs, device-resident */

/* library / device ----------------------------------------------------------------- */
int pnmol_abi_version(void);
int pnmol_device_count(int* count);
int pnmol_ctx_create(int device, pnmol_ctx** out);
int pnmol_ctx_destroy(pnmol_ctx* ctx); /* -1, nothing freed, while filters of ctx are alive (see Lifetimes) */
int pnmol_ctx_synchronize(pnmol_ctx* ctx);
const char* pnmol_last_error(pnmol_ctx* ctx);

/* cold-path assembly on the device ----------------------------------------------------------
 * Batched kernel finite-difference stencils, `discretize.fd_coefficients` under `jax.vmap` (discretize.py:60,75-80,177-201):
 * for every mesh point p,  weights_p = (gram_p)^-1 lk_p  (gram_p = k(X_p, X_p) + nugget I, (s,s); lk_p = L k(x_p, X_p), (s)),
 * uncertainty_p = llk_p - weights_p . lk_p  (llk_p = L L k(x_p, x_p)).  1 <= s <= 16.  LU with partial pivoting per point. */
int pnmol_fd_solve_batched(pnmol_ctx* ctx, const double* gram_nss, const double* lk_ns, const double* llk_n, int N, int s,
                           double* weights_ns, double* uncertainty_n);
/* Gamma = chol(K): `jnp.linalg.cholesky(spatial_kernel(X, X.T))` (white.py:84-85, latent.py:139) with the step's own sweep
 * kernels.  A (n,n) symmetric positive definite, row-major; L (n,n) lower triangular (upper part zeroed).
 * -3: not positive definite (the failing pivot is in `pnmol_last_error`). */
int pnmol_cholesky_lower(pnmol_ctx* ctx, const double* A_nn, int n, double* L_nn);

/* problem description = the attributes `attempt_step` reads from `pde`
 * (white.py:96-146, :169-186; pde/mixins.py:19-59) and from the solver
 * (`num_derivatives`, pdefilter.py:37-70; Gamma = chol(spatial_kernel(X, X.T)),
 * white.py:82-94). */
typedef struct pnmol_filter_desc {
    int d;                 /* mesh points = pde.L.shape[0]                            */
    int num_derivatives;   /* nu; n = nu + 1 in {2,3,4}                               */
    int nB;                /* rows of pde.B                                           */
    const double* L;       /* (d,d_state)  pde.L                                      */
    const double* B;       /* (nB,d_state) pde.B                                      */
    const double* E_sqrtm; /* (d,d)  pde.E_sqrtm                                      */
    const double* R_sqrtm; /* (nB,nB) pde.R_sqrtm                                     */
    const double* Gamma;   /* (d,d) lower; iwp.wp_diffusion_sqrtm (base/iwp.py:10)    */
    int d_state;           /* 0 or d: white-noise model.  2d: latent-force model (latent.py:11-292), whose state is
                              [u; eps] = two stacked IWPs (base/stacked_ssm.py): then L is (d, 2d) = [L, I]
                              (H_ode = E1 - L E0 - E0_eps, latent.py:253-257), B is (nB, 2d) = [B, 0], Gamma is
                              (2d, 2d) = blockdiag(chol K, E_sqrtm) (latent.py:136-153), E_sqrtm/R_sqrtm are the
                              measurement noise factors (zero: update_sqrt_no_meascov, latent.py:197).  State
                              buffers are then (n, 2d) / (2D, 2D) in the reference's glued order (latent.py:163-175). */
    int dtype;             /* 0: fp64 (the reference's arithmetic, src/pnmol/__init__.py:9-11).
                              1: fp32 covariance (BASELINE config 5's "fp32 with tolerance study"): the state
                              covariance, the predicted covariance and Q live in HBM as fp32, and the bulk of the step --
                              P- = A P A^T + Q, the stencil gather P- H^T, the down-date P = P- - W W^T (fp32 MFMA,
                              v_mfma_f32_16x16x4_f32) -- runs on them; the stencil weights, S = H P- H^T + R, its Cholesky
                              sweep (Ls, W, r), the mean and every scalar stay fp64.  Buffers crossing this boundary are
                              double either way.  Needs num_derivatives <= 2.  What it costs in accuracy: DESIGN.md
                              section 11 (tolerance study). */
    const double* K;       /* optional (d_state,d_state): the Gram matrix Gamma Gamma^T = spatial_kernel(X, X^T) of white.py:84-85
                              (base/iwp.py:49-52 uses it as Ql Ql^T = Q1 (x) K).  NULL: the library forms Gamma Gamma^T itself,
                              an O(d^3) scalar loop on the host (seconds at d = 4096); a caller that has the Gram matrix anyway
                              passes it.  Ignored by pnmol_sqrt_filter_create (the QR form works on Gamma itself). */
} pnmol_filter_desc;

int pnmol_filter_create(pnmol_ctx* ctx, const pnmol_filter_desc* desc, pnmol_filter** out);
int pnmol_filter_destroy(pnmol_filter* f); /* -1, nothing freed, while states of f are alive (see Lifetimes) */
/* Which sweep launch this filter's steps use (build-side diagnostic; no reference counterpart): *kernel is 1 or 2:
 * 1 left-looking dataflow kernel (wide matrices: N = 1024, 2-d meshes), 2 register-resident right-looking kernel
 * (d + nB <= 544); *xcd_home = the XCD its critical workgroups are placed on (XCD-local layout: the first such filter alive on
 * a device, or PNMOL_HIP_SWEEP_XL=1) or -1 (spread layout).  Timings of the two layouts differ; benchmarks report this. */
int pnmol_filter_sweep_layout(const pnmol_filter* f, int* kernel, int* xcd_home);

/* Step-invariant part of `estimate_error` (white.py:153-162) for step size dt:
 * Sq = H (Ql Ql^T) H^T + E E^T depends only on dt for a linear PDE.  The caller passes
 * Sq^-1 (m,m) and diag(Sq) (m), m = d + nB; the per-step part z^T Sq^-1 z runs on device.
 * Without it, the error estimate of a step with this dt is reported as NaN. */
int pnmol_filter_set_error_model(pnmol_filter* f, double dt, const double* Sq_inv,
                                 const double* Sq_diag);
/* The same on the device, from the operator currently set (L, or J_x + L after `pnmol_filter_set_operator`):
 * Sq is the innovation matrix of a filter whose predicted covariance is Ql Ql^T = Q1 (x) K, so the step's own
 * kernels factorise it ([Sq; I] -> [Lq; Lq^-T], Sq^-1 = Lq^-T Lq^-1); diag(Sq) is kept for the error vector.  No host
 * O(m^3) work per new dt / per semilinear step. */
int pnmol_filter_prepare_error_model(pnmol_filter* f, double dt);

/* Semilinear EK1 (`SemiLinearWhiteNoiseEK1.evaluate_ode`, white.py:189-208): the measurement rows become
 * H_ode = E1 - (J_x + L) E0 with shift b = J_x m_at - f(t, m_at), re-linearised at every step.
 * `pnmol_filter_predict_mean` returns m_at = E0 P m^- (predicted derivative-0 mean, raw coordinates) for a step
 * of size dt from `in`; the caller evaluates f and df there and passes M = J_x + L (d,d_state) and shift (d) to
 * `pnmol_filter_set_operator` (NULL shift = zeros), which replaces the stencil rows used by the following
 * `pnmol_filter_step(s)` calls.  The boundary rows B are kept. */
int pnmol_filter_predict_mean(pnmol_filter* f, const pnmol_state* in, double dt, double* m_at_d);
int pnmol_filter_set_operator(pnmol_filter* f, const double* M_dds, const double* shift_d);
/* The same for a POINTWISE nonlinearity, whose Jacobian is diagonal (`df_diagonal` of the reference's problem classes,
 * pde/problems.py; spruce budworm: pde/examples.py:292-341): M = L + diag(jdiag) with the L given at creation.  d + d numbers
 * cross the bus instead of a dense (d, d_state) matrix, the stencil rows are patched on the device (no host scan of M, no
 * stream synchronisation, captured graphs stay valid).  Valid after any `pnmol_filter_set_operator`, in any order: the first
 * call after a dense upload restores L's stencil rows first (whatever the dense operator's width or row pattern; captured
 * graphs are dropped only if the width changes).  -1 if a row of L has no diagonal entry. */
int pnmol_filter_set_operator_diagonal(pnmol_filter* f, const double* jdiag_d, const double* shift_d);

/* Pointwise reaction terms evaluated on the device --------------------------------------------------------------------------
 * For u_t = L u + r(u) with r(u) = P(u) + A(u) / B(u), the same at every mesh point: P, A, B polynomials with scalar
 * coefficients in ascending powers, degree <= PNMOL_REACTION_MAXDEG (a degree of -1: the term is absent; A and B together or
 * not at all).  Logistic / Fisher-KPP, Allen-Cahn, Nagumo and the spruce-budworm rational term have this form.  No reference
 * counterpart (its f is a callable); the arithmetic is that of `pnmol_filter_predict_mean` + `pnmol_filter_set_operator_diagonal`
 * with jdiag = r'(u), shift = r'(u) u - r(u) at the predicted mean u, r and r' = P' + (A' B - A B') / B^2 by Horner, every
 * operation rounded on its own.
 * `pnmol_filter_set_reaction` (NULL clears) stores the descriptor, restores the stencil rows of the L given at creation and a
 * zero shift, forgets the error model and drops captured graphs.  -1 (reason in `pnmol_last_error`): null filter, latent-force
 * filter (d_state != d), fp32 filter, a row of L without a diagonal entry, a degree outside [-1, 7], A without B or B without A,
 * a coefficient that is not finite, B identically zero.  While a reaction is set
 *   - `pnmol_filter_set_operator` and `pnmol_filter_set_operator_diagonal` return -1 (clear the reaction first);
 *   - every step of `pnmol_filter_steps(_begin)` is re-linearised on the device at its own predicted mean, so the constant-step
 *     loop runs semilinear problems without a host round trip.  The loop then takes self-contained steps (the next step's
 *     innovation is no longer prepared inside the previous step's read-out launch, which would precede the re-linearisation)
 *     and carries no error model: `error_sigma2` of its steps is NaN, and an error model prepared before is forgotten;
 *   - `pnmol_filter_step` is unchanged: it uses the operator that is set.  For one step call, in this order,
 *     `pnmol_filter_linearize(f, in, dt)` (enqueues the re-linearisation for a step from `in` over dt: no synchronisation, no
 *     read-back), `pnmol_filter_prepare_error_model(f, dt)` (if the error estimate is wanted: it reads the new operator) and
 *     `pnmol_filter_step(f, in, dt, ...)`.  -1: null argument, foreign state, dt <= 0, no reaction set.
 * A non-finite r(u) (a pole of A / B at a predicted value) is not trapped: it reaches the factorisation as a NaN pivot and the
 * step returns -3, as for any other innovation matrix that is not positive definite.
 * After `pnmol_filter_set_reaction(f, NULL)` the filter behaves bit for bit like one that never had a reaction. */
#define PNMOL_REACTION_MAXDEG 7
typedef struct pnmol_reaction {
    int deg_p, deg_a, deg_b; /* -1: term absent */
    double p[PNMOL_REACTION_MAXDEG + 1], a[PNMOL_REACTION_MAXDEG + 1], b[PNMOL_REACTION_MAXDEG + 1];
} pnmol_reaction;
int pnmol_filter_set_reaction(pnmol_filter* f, const pnmol_reaction* r);
int pnmol_filter_linearize(pnmol_filter* f, const pnmol_state* in, double dt);

/* Coupled pointwise reactions (systems) --------------------------------------------------------------------------------------
 * For a state [u_0; ...; u_{C-1}] of C species on the same N mesh points (d = C N, species-major) and
 * r_c(u) = P_c(u) + A_c(u) / B_c(u) with u = (u_0 .. u_{C-1}) at ONE mesh point: P_c, A_c, B_c polynomials in the C species, each a
 * sum of at most PNMOL_SYSTEM_MAXTERMS monomials coef * u_0^pow[0] * ... (exponents 0..7; a polynomial of 0 terms is zero; A_c and
 * B_c together or not at all).  Lotka-Volterra, SIR (-+beta s i / (s + i + r)) and Gray-Scott have this form.  The Jacobian has C
 * entries per row, at the same mesh point in every species block: row c N + j of M = L + J holds J_ck at column k N + j.
 * `pnmol_filter_set_reaction_system` (NULL clears) mirrors `pnmol_filter_set_reaction`: it stores the descriptor, installs the
 * widened image of the L given at creation -- every PDE row gets a slot for each of its C same-point columns (value 0 where L has
 * none), slots in ascending column order, width at most that of L plus C - 1 -- with a zero shift, forgets the error model and
 * drops captured graphs.  A filter holds one reaction of either kind: each setter replaces what the other had set, NULL to either
 * clears either, and the cleared filter behaves bit for bit like one that never had a reaction.  While a system is set the operator
 * calls are refused, `pnmol_filter_linearize` and `pnmol_filter_steps(_begin)` re-linearise as above.
 * Arithmetic (every operation rounded on its own; pnmol/pde/reactions.py, `SystemReaction`, is the same on the host): u_k as in
 * `pnmol_filter_predict_mean`; a monomial starts from coef and is multiplied by u_0 pow[0] times, then by u_1 pow[1] times, ...;
 * a polynomial is the sum of its monomials in the order given, starting from the first; the partial derivative of a monomial by
 * u_k with exponent e >= 1 starts from e * coef and takes the same multiplications with one factor u_k fewer (e = 0: the monomial
 * is skipped); J_ck = dP_k + (dA_k B - A dB_k) / (B B), r_c = P + A / B, shift_i = ((J_c0 u_0 + J_c1 u_1) + ...) - r_c.
 * -1 (reason in `pnmol_last_error`): null filter, ncomp outside [1, 4], d not a multiple of ncomp, a term count outside [0, 8], an
 * exponent outside [0, 7] or a non-zero exponent of a species >= ncomp, A_c without B_c or B_c without A_c, a coefficient that is
 * not finite, a B_c whose coefficients are all zero, latent-force filter, fp32 filter, a row of L without a diagonal entry.
 * A pole of A_c / B_c is not trapped: the step returns -3. */
#define PNMOL_SYSTEM_MAXCOMP  4
#define PNMOL_SYSTEM_MAXTERMS 8
typedef struct pnmol_monomial    { double coef; int pow[PNMOL_SYSTEM_MAXCOMP]; } pnmol_monomial;
typedef struct pnmol_system_poly { int nterms; pnmol_monomial term[PNMOL_SYSTEM_MAXTERMS]; } pnmol_system_poly; /* 0 terms: zero */
typedef struct pnmol_reaction_system {
    int ncomp;                                     /* C in 1..4; the state is [u_0; ...; u_{C-1}], d = C * N */
    pnmol_system_poly p[PNMOL_SYSTEM_MAXCOMP], a[PNMOL_SYSTEM_MAXCOMP], b[PNMOL_SYSTEM_MAXCOMP];
} pnmol_reaction_system;                           /* r_c(u) = P_c(u) + A_c(u) / B_c(u), u = (u_0..u_{C-1}) at ONE mesh point */
int pnmol_filter_set_reaction_system(pnmol_filter* f, const pnmol_reaction_system* r);   /* NULL clears */

/* Convection terms (Burgers type) --------------------------------------------------------------------------------------------
 * For u_t = L u + c(u) . (G u) + r(u): c a polynomial in ascending coefficients (degree <= 7; viscous Burgers: c = (0, -1)), r an
 * optional `pnmol_reaction` (all three degrees -1: absent; Burgers-Fisher: the logistic term), G a (d, d) stencil matrix (row
 * major; a discretised gradient on the mesh) that is fixed when the term is set.  With u the predicted mean, g = G u and
 * q_i = c'(u_i) g_i + r'(u_i), the EK1 linearisation is M = L + diag(c(u)) G + diag(q) with shift_i = q_i u_i - r(u_i): the
 * Jacobian touches every stencil entry of a row, not only its diagonal.
 * `pnmol_filter_set_convection` (a NULL term clears, G is then ignored) mirrors `pnmol_filter_set_reaction`: it stores the
 * descriptor, builds and installs the union image of the L given at creation and of G -- every PDE row has a slot for each column
 * in which L or G has an entry, in ascending column order, with G's value beside it (0 where only L has one); the stencil grows if
 * the union is wider than L -- with a zero shift, forgets the error model and drops captured graphs.  A filter holds one of
 * reaction, system or convection: each setter replaces what another had set, NULL to any of them clears, and the cleared filter
 * behaves bit for bit like one that never had a term.  While a convection term is set the operator calls are refused and
 * `pnmol_filter_linearize` and `pnmol_filter_steps(_begin)` re-linearise, as for a reaction.
 * Arithmetic (every operation rounded on its own; pnmol/pde/reactions.py, `Convection`, is the same on the host): u_i and the u of
 * every slot column as in `pnmol_filter_predict_mean`; g_i is the sum of G_ij u_j over the row's entries of G that are not zero,
 * in ascending column order, starting from the first product; c, c', r, r' by Horner as for a reaction; q = c' g + r' (c' g alone
 * without a reaction); an entry of M is L_ij + c_i G_ij, the diagonal one (L_ii + c_i G_ii) + q_i; the shift is q u - r.
 * -1 (reason in `pnmol_last_error`): null filter, a term without G, a degree outside [-1, 7], A without B or B without A, a
 * coefficient or an entry of G that is not finite, B identically zero, latent-force filter, fp32 filter, a row of L without a
 * diagonal entry.  The uncertainty of the finite-difference weights of G is not modelled (the error model keeps that of L). */
typedef struct pnmol_convection { int deg_c; double c[PNMOL_REACTION_MAXDEG + 1]; pnmol_reaction r; } pnmol_convection;
int pnmol_filter_set_convection(pnmol_filter* f, const pnmol_convection* term, const double* G_dd);   /* NULL term clears */

/* Linearisation points for the constant-step loop (iterated smoother) --------------------------------------------------------
 * `evaluate_ode` (white.py:192-208) linearises f at m_at = E0 m^-, the step's own predicted mean.  An iterated extended Kalman
 * smoother repeats the forward pass with every step linearised at the previous pass's SMOOTHED mean instead; no reference
 * counterpart.  `pnmol_filter_set_linearization_points(f, count, u_cd)`: u_cd is (count, d) row-major, derivative 0 of the PDE
 * state in raw coordinates; the table is copied to the device and the cursor goes to row 0.  While a table is set, the i-th step
 * `pnmol_filter_steps(_begin)` takes since then linearises the term at row i in place of the predicted value (for a convection
 * term the row's stencil neighbours come from the same row of the table); the arithmetic behind the point, and the rest of the
 * step, are unchanged.  Rows are consumed across calls (a schedule's runt last step is a call of its own); a call that fails
 * (-2 / -3) consumes none, `pnmol_filter_prepare_steps` consumes none.  The row is addressed on the device (a cursor word written
 * once per call plus the loop's step counter), so the captured graphs of the loop serve any position; graphs captured without a
 * table are not replayed with one, nor the reverse.  Composes with the recorder and the sensor plan in one call; the order per
 * step is linearise, step, observation update, record.  count = 0 or a NULL table clears; so does every term setter (a NULL
 * term included).  `pnmol_filter_linearize` and `pnmol_filter_step` are unchanged and consume no row.
 * -1 (reason in `pnmol_last_error`, nothing enqueued): null filter, no term set, count < 0, an entry that is not finite, called
 * between `pnmol_filter_steps_begin` and `_end`; and from `pnmol_filter_steps(_begin)`: more steps asked for than rows left.
 * `pnmol_filter_linearization_pending`: the cursor (the row the next step takes) and the number of rows (0, 0: no table).
 * `pnmol_filter_linearize_at(f, u_d)`: the host-callable counterpart of `pnmol_filter_linearize` -- d numbers go up and the same
 * kernels linearise the term there (no synchronisation; the error model is forgotten); `pnmol_filter_step` follows.  A loop over a
 * table gives the bits of this call in front of every single step.  -1: null argument, no term set. */
int pnmol_filter_set_linearization_points(pnmol_filter* f, int count, const double* u_cd);
int pnmol_filter_linearization_pending(const pnmol_filter* f, int* next, int* count);
int pnmol_filter_linearize_at(pnmol_filter* f, const double* u_d);

/* Driven problems: sources and boundary values --------------------------------------------------------------------------------
 * u_t = L u + r(u) + s(t, x) with boundary rows B u = g(t).  With rhs(t) = [s(t, X) (d); g(t) (nB)], m = d + nB numbers, the step
 * that lands on t measures z = H m^- + shift_term - rhs(t): `shift_term` is what the filter has without forcing (zero for a linear
 * filter, J u - r behind `pnmol_filter_linearize`), and the device forms fl(shift_term[i] - rhs[i]), one rounded subtraction per row
 * (without a term: -rhs[i], exact).  The PDE rows are the reference's semilinear model with f <- f + s (white.py:189-208); the
 * reference knows B u = 0 only.  H, S, the gain, the error model and the whole backward pass are untouched: forcing enters the
 * means only.  For fp64 filters, white-noise and latent-force (d_state = 2 d) -- the filters that take
 * `pnmol_filter_set_observations`.
 * `pnmol_filter_set_forcing(f, count, rhs_cm)`: rhs_cm is (count, m) row-major; row k is consumed by the k-th step
 * `pnmol_filter_steps(_begin)` takes from now on.  Rows are consumed across calls (a schedule's runt last step takes its own row);
 * a call that fails (-2 / -3) consumes none, `pnmol_filter_prepare_steps` consumes none.  The table is copied to the device (row
 * stride mp, padding zero), the cursor goes to row 0; the call synchronises.  A table that fits the one before it is overwritten in
 * place and the captured graphs replay on it; any other change of the table drops them.  The row is addressed on
 * the device (a cursor word written once per call plus the loop's step counter), so every step launches with identical arguments and
 * the loop's graphs serve any position.  While a table is set the loop takes the self-contained steps (as with a term or a sensor
 * plan: the next innovation cannot be prepared before its right-hand side is in place).  Without a term H does not change, and the
 * loop KEEPS the error model: `error_sigma2` is reported as in the unforced loop when `pnmol_filter_prepare_error_model(dt)` was
 * called; with a term the loop carries none, as ever.  Composes with a term, the table of linearisation points, the recorder and
 * the sensor plan; the order per step is linearise, force, step, observation update, record.  The term setters keep the table: it
 * belongs to the problem, not to the term.  count = 0 or a NULL table clears.  A filter without forcing enqueues what it always
 * did.  -1 (reason in `pnmol_last_error`, nothing enqueued): null filter, fp32 filter, count < 0, an entry that is not finite (row
 * and column are named), called between `pnmol_filter_steps_begin` and `_end`; and from `pnmol_filter_steps(_begin)`: more steps
 * asked for than rows left (the state is untouched).  -4: out of memory.
 * `pnmol_filter_forcing_pending`: the cursor (the row the next step takes) and the number of rows (0, 0: no table).
 * `pnmol_filter_force_at(f, rhs_m)`: the single-step counterpart -- every `pnmol_filter_step` from now on measures against these m
 * numbers, until another call replaces them or NULL returns the filter to unforced.  `pnmol_filter_step` reads the shift as it
 * stands when it is enqueued, so with a term call `pnmol_filter_linearize` / `_linearize_at` first, in any order with this call.
 * `error_sigma2` and the error estimate are reported as without forcing.  No synchronisation (the numbers wait in mapped host
 * memory of their own).  The loop takes no notice of it, and `pnmol_filter_step` takes none of the table.  A right-hand side
 * PERSISTS: it is not consumed by a step, it survives `pnmol_filter_steps`, `pnmol_filter_set_forcing` and the term setters, and
 * while it is held the operator setters refuse (below) -- `pnmol_filter_force_at(f, NULL)` behind the last forced step is the
 * caller's job.  -1: null filter, fp32 filter, an entry that is not finite, called between `pnmol_filter_steps_begin` and `_end`.
 * While a table or a single right-hand side is set, `pnmol_filter_set_operator` and `pnmol_filter_set_operator_diagonal` return
 * -1, as they do with a term. */
int pnmol_filter_set_forcing(pnmol_filter* f, int count, const double* rhs_cm);
int pnmol_filter_forcing_pending(const pnmol_filter* f, int* next, int* count);
int pnmol_filter_force_at(pnmol_filter* f, const double* rhs_m);

/* Time-dependent operators: u_t = sum_r a_r(t) L_r u ----------------------------------------------------------------------------
 * M(t) = sum_{r<R} a_r(t) L_r with R <= PNMOL_OPERATOR_MAXR fixed (d, d) stencil operators and scalar coefficients: a conductivity
 * that changes in time, transport in an oscillating flow.  The step that lands on t measures with H = [E1 - M(t) E0; B E0] and the
 * noise of its PDE rows is that of the operator, R_pde(t) = diag(sum_r (a_r(t) e_{r,i})^2), e_r the diagonal of the FD uncertainty
 * E_sqrtm_r that came with L_r (errors of different operators are taken as independent; only diagonal E_sqrtm_r).  Boundary rows,
 * their noise, the prior and the whole backward pass are untouched.  For fp64 white-noise filters (d_state = d) whose noise at
 * creation is diagonal.
 * `pnmol_filter_set_operator_family(f, R, L_Rdd, e_Rd)`: L_Rdd is (R, d, d) row-major, e_Rd (R, d).  Builds the union image of the
 * L_r on top of the operator given at creation: every PDE row gets a slot for each column in which any L_r has an entry, in
 * ascending column order, and one for the diagonal; boundary rows and padding are those of the creation-time image; the stencil
 * grows if the union is wider.  The image does not depend on the coefficients (one may be zero at t0).  Until the first
 * `pnmol_filter_operator_at` or loop step with a schedule the filter measures with the operator and the noise given at creation;
 * the shift is zeroed.  Synchronises, drops the captured graphs, forgets the error model and the schedule of a family set before.
 * R = 0 or a NULL argument clears: the creation-time image and noise come back, and the filter behaves bit for bit like one that
 * never had a family.  -1 (reason in `pnmol_last_error`, nothing enqueued): null filter, R outside [1, 4], an entry of L or e that
 * is not finite (operator, row and column are named), a latent-force or fp32 filter, noise at creation that is not diagonal, a
 * filter whose operator or shift was replaced by `pnmol_filter_set_operator(_diagonal)` (image and clearing start from the
 * creation-time operator and would lose it; setting a term, or clearing one, restores the creation-time operator and lifts the refusal), a
 * reaction system or a convection term set (both bring a widened image of their own; `pnmol_filter_set_reaction_system` and
 * `pnmol_filter_set_convection` refuse likewise while a family is set), called between `pnmol_filter_steps_begin` and `_end`.
 * -4: out of memory.
 * `pnmol_filter_set_operator_schedule(f, count, a_cR)`: a_cR is (count, R) row-major; row k is consumed by the k-th step
 * `pnmol_filter_steps(_begin)` takes from now on, with the semantics of `pnmol_filter_set_forcing`: rows are consumed across calls
 * (a runt last step takes its own row), a call that fails consumes none, `pnmol_filter_prepare_steps` consumes none, more steps
 * asked for than rows left returns -1 from `pnmol_filter_steps(_begin)` with the state untouched, count = 0 or NULL clears.  A
 * table that fits the one before it is overwritten in place and the captured graphs replay on it; the cursor goes to row 0.  The
 * row is addressed on the device (a cursor word plus the loop's step counter).  While a schedule is set the loop takes the
 * self-contained steps and carries no error model (H changes with every step); the order per step is operator, linearise, force,
 * step, observation update, record.  Composes with a pointwise reaction (`pnmol_filter_set_reaction`: the diagonal of r' goes on
 * top of M(t)), the table of linearisation points, forcing, the sensor plan and the recorder.  -1: null filter, no family set,
 * latent-force or fp32 filter, count < 0, an entry that is not finite (row and column are named), called inside a call.
 * `pnmol_filter_operator_schedule_pending`: the cursor and the number of rows (0, 0: no table).
 * `pnmol_filter_operator_at(f, a_R)`: the single-step counterpart -- the same kernel on R numbers waiting in mapped host memory,
 * enqueued at once, no synchronisation.  The operator and its noise PERSIST until another call or a loop step with a schedule
 * replaces them.  The error model is forgotten: `pnmol_filter_prepare_error_model` comes next if one is wanted, then (with a
 * reaction) `pnmol_filter_linearize`, then `pnmol_filter_step`.  -1: null filter or coefficients, no family, not finite, inside a
 * call.
 * While a family is set, `pnmol_filter_set_operator` and `pnmol_filter_set_operator_diagonal` return -1, as they do with a term or
 * forcing. */
#define PNMOL_OPERATOR_MAXR 4
int pnmol_filter_set_operator_family(pnmol_filter* f, int R, const double* L_Rdd, const double* e_Rd);
int pnmol_filter_set_operator_schedule(pnmol_filter* f, int count, const double* a_cR);
int pnmol_filter_operator_schedule_pending(const pnmol_filter* f, int* next, int* count);
int pnmol_filter_operator_at(pnmol_filter* f, const double* a_R);

/* states ----------------------------------------------------------------------------- */
int pnmol_state_create(pnmol_filter* f, pnmol_state** out);
int pnmol_state_destroy(pnmol_state* s); /* -1 for the target of an unfinished pnmol_filter_steps_begin, and for a slot of a set recorder */
int pnmol_state_clone(const pnmol_state* s, pnmol_state** out); /* reject/retry, pdefilter.py:192-223 */
/* upload `PDEFilterState(t, y=(mean, cov))`; cov = cov_sqrtm @ cov_sqrtm.T (base/rv.py:12-14) */
int pnmol_state_set(pnmol_state* s, double t, const double* mean_nd, const double* cov_DD);
/* the same from a square root: any C (D,D) with C C^T = cov, e.g. the reference's `cov_sqrtm`; C C^T is formed on the
 * device (no O(D^3) host work).  Used by `initialize` (white.py:12-80), whose factor comes from `pnmol_sqrt_update`. */
int pnmol_state_set_sqrtm(pnmol_state* s, double t, const double* mean_nd, const double* cov_sqrtm_DD);
int pnmol_state_get_time(const pnmol_state* s, double* t);
int pnmol_state_get_mean(const pnmol_state* s, double* mean_nd);       /* (n,d)            */
int pnmol_state_get_cov(const pnmol_state* s, double* cov_DD);         /* (D,D) F-order    */
/* The lower-triangular Cholesky factor C of the covariance, C C^T = cov, (D,D) in the F-flattened order -- the
 * canonical representative (positive diagonal) of what the reference carries as `cov_sqrtm` (base/rv.py:9-14; its
 * QR factors differ from it by column signs only).  Computed on the device by the step's sweep kernel; a direction
 * whose pivot falls below 1e-13 of its diagonal entry (noise-free Dirichlet node, numerically deterministic
 * combinations) gives a zero column: diag(C C^T) stays accurate (1e-6 relative or better), the off-diagonal entries of such a direction j
 * are lost, |(C C^T - cov)_ij| <= sqrt(c_ii * 1e-13 c_jj).  Never fails on indefiniteness (the covariance of the
 * recursion is PSD only up to rounding); -3 only for NaN. */
int pnmol_state_get_cov_sqrtm(const pnmol_state* s, double* C_DD);
/* diag(cov) as (n,d): what experiments/figure1.py:76-80 reads out (`stds**2`)            */
int pnmol_state_get_marginal_var(const pnmol_state* s, double* var_nd);

/* one step ----------------------------------------------------------------------------- */
typedef struct pnmol_step_out {
    double t_new;                   /* state.t + dt                                       */
    double diffusion_squared_local; /* white.py:125-128 formula with the Cholesky factor
                                       of S (positive diagonal): |Ls^-T z|^2 / m          */
    double sigma2_whitened;         /* z^T S^-1 z / m (the quasi-MLE the comment intends) */
    double error_sigma2;            /* z^T Sq^-1 z / m of estimate_error (NaN if no model)*/
    int info;                       /* -1 ok, else index of first non-positive pivot      */
} pnmol_step_out;

/* `_WhiteNoiseEK1Base.attempt_step` with `LinearWhiteNoiseEK1.evaluate_ode`
 * (white.py:96-146, :169-186).  `in` is not modified; `out` may not alias `in`.
 * `error_estimate_d` (d) optional: dt * sqrt(diag Sq) * sigma (white.py:117-129). */
int pnmol_filter_step(pnmol_filter* f, const pnmol_state* in, double dt, pnmol_state* out,
                      pnmol_step_out* info, double* error_estimate_d);

/* One backward step of the RTS smoother (kalman.py:33-46 / :49-66 of the reference, covariance form):
 * out = smoothed state at filt_k->t from the filtered state at t_k, the smoothed state at t_k + dt and the step dt the
 * forward pass took.  States of the same fp64 white-noise filter; out may not alias either input; inputs unchanged.
 * In the Nordsieck frame of dt (inputs in any frame): P- = A P A^T + Q, G = P A^T (P-)^-1, ms = m + G (ms' - A m),
 * Ps = P + G (Ps' - P-) G^T with the prior alone (Q uncalibrated, like the filter's covariances); `out` is an ordinary
 * state in that frame.  -1: bad argument (also a latent-force or fp32 filter), -3: P- not positive definite (pivot in
 * `pnmol_last_error`), -4: out of memory.  Workspace (~5 Dp^2 doubles) is allocated on the first call and kept by the
 * filter; one stream synchronisation per call. */
int pnmol_smoother_step(pnmol_filter* f, const pnmol_state* filt_k, const pnmol_state* smooth_next, double dt,
                        pnmol_state* out);

/* Measurement update: condition a state on sensor data -------------------------------------------------------------------------
 * Model y = C E0 x + e, e ~ N(0, R_sqrtm R_sqrtm^T): q linear functionals of derivative 0 of the d_state state components (white-noise
 * model: the solution u at the mesh points; latent-force model: [u; eps], so C has 2d columns).  No reference counterpart (the
 * reference solves the PDE without data); the arithmetic is the covariance-form Kalman update of kalman.py:12-30 with the step's own
 * Cholesky sweep.  With m, P of `in` and H = C E0:
 *     S = H P H^T + R R^T = Ls Ls^T,   W = P H^T Ls^-T,   w = Ls^-1 (y - H m),   m_out = m + W w,   P_out = P - W W^T,
 *     log_likelihood = log N(y; H m, S) = -1/2 (|w|^2 + 2 sum log Ls_ii + q log 2 pi),   mahalanobis = |w|^2,   logdet = log det S.
 * `in` (any frame) is not modified; `out` (another state of the same filter) is an ordinary state at in's time in in's frame.
 * C_q_ds (q, d_state) row-major; y_q (q); R_sqrtm_qq (q, q) lower triangular (the upper part is ignored) or NULL: noise-free.
 * The covariances are the uncalibrated ones the states carry (sigma^2 = 1): R is weighed against that prior.
 * fp64 filters, white-noise and latent-force.  -1: null or aliased pointers, a state of another filter, q < 1, q > d_state, an fp32
 * filter.  -3: S not positive definite, e.g. duplicate rows of C without noise (res->info and `pnmol_last_error` name the pivot; `out`
 * is undefined then).  -4: out of memory.  Workspace (~2 (Dp + q) q doubles per distinct round_up(q, 32)) is allocated on first use and
 * kept by the filter; one stream synchronisation per call. */
typedef struct pnmol_observe_out {
    double log_likelihood;
    double mahalanobis;
    double logdet;
    int info; /* -1 ok, else index of the first non-positive pivot of S */
} pnmol_observe_out;
int pnmol_state_observe(pnmol_filter* f, const pnmol_state* in, int q, const double* C_q_ds, const double* y_q,
                        const double* R_sqrtm_qq, pnmol_state* out, pnmol_observe_out* res);

/* Sensor data in the constant-step loop ------------------------------------------------------------------------------------------
 * A fixed sensor array -- C (q, d_state) and R_sqrtm (q, q) shared by all times -- that reports y_i at the times t_i: the plan of a
 * filter.  With a plan set, `pnmol_filter_steps_begin(f, s, k, dt)` walks the times the call reaches (t = s->t; t += dt per step) and
 * enqueues the update of the pending entry whose time agrees with the time behind step j (16 ulp, as everywhere) right behind that
 * step, in place on the state; later steps start from the conditioned state.  No host round trip in between and one synchronisation
 * per call, as without data.  The update is `pnmol_state_observe`'s (same model, same formulas) with y, C and R read from the plan's
 * device tables and the three scalars kept on the device until the call's copy-out: the kernels of `pnmol_state_observe` in their
 * order, bit for bit its result.  With PNMOL_HIP_OBSERVE_SINGLE_WG=1 in the environment when the plan is set, a plan of q <= 32 takes
 * a route without the sweep launch instead (one workgroup factorises S in LDS; rounding-level differences).  It measured 0.03 ms
 * slower per update than the sweep route and is therefore not the default; the switch keeps it measurable.
 * `_begin` returns -1 before anything is enqueued, `s` untouched, `pnmol_last_error` naming entry and time, when the next pending entry
 * lies before s->t, at s->t (it was never applied: apply it with `pnmol_state_observe_planned` or `pnmol_state_observe` first) or
 * strictly between two grid times of the call.  Entries behind s->t + k dt stay pending for the next call.
 * `_end` fills the results and advances the cursor; row j of means_kd / stds_kd is that of the conditioned state when an entry was
 * applied behind step j; info_k[j] keeps its meaning (the PDE residual only).  -3 when an update's innovation matrix is not positive
 * definite (entry and pivot in `pnmol_last_error`; a dropped pivot is an error here); a step's own error at or before that step
 * takes precedence.  While entries are pending the loop runs its self-contained steps (as with a nonlinear term); a filter without a
 * plan, or whose plan is cleared, takes the launches and gives the bits it always did.  A term set by `pnmol_filter_set_reaction` /
 * `_system` / `_convection` composes with a plan.  `pnmol_filter_destroy` frees the plan.
 *
 * `pnmol_filter_set_observations`: nobs = 0 or t_nobs = NULL clears.  Copies everything (t_nobs (nobs), C_q_ds (q, d_state) row-major,
 * R_sqrtm_qq (q, q) lower triangular or NULL: noise-free, y_nobs_q (nobs, q) row-major); resets the cursor to entry 0.  -1 (reason in
 * `pnmol_last_error`): null filter, fp32 filter, q < 1, q > d_state, times not strictly increasing or not finite, a non-finite entry
 * of C, R or y, R not lower triangular, an unfinished `pnmol_filter_steps_begin`.  -4: out of memory.  Synchronises the stream.
 * `pnmol_filter_observations_pending`: the cursor (index of the first entry not applied) and the number of entries (0, 0: no plan).
 * `pnmol_filter_observation_results`: results of the entries [first, first + count), which must have been applied (-1 otherwise).
 * `pnmol_state_observe_planned`: entry `index` applied to `s` IN PLACE, now, by exactly the path the loop takes (enqueue, then one
 * synchronisation), in the frame `s` is in; the time of the entry is not compared with s->t.  Does not move the cursor unless
 * index == next, in which case it advances it.  -1: null, foreign state, no plan, index outside the plan, an unfinished
 * `pnmol_filter_steps_begin`; -3 as for `pnmol_state_observe`. */
int pnmol_filter_set_observations(pnmol_filter* f, int nobs, const double* t_nobs, int q, const double* C_q_ds,
                                  const double* R_sqrtm_qq /* lower triangular; NULL: noise-free */,
                                  const double* y_nobs_q);
int pnmol_filter_observations_pending(const pnmol_filter* f, int* next, int* nobs);
int pnmol_filter_observation_results(const pnmol_filter* f, int first, int count, pnmol_observe_out* res);
int pnmol_state_observe_planned(pnmol_filter* f, pnmol_state* s, int index, pnmol_observe_out* res);

/* Dense output: the posterior BETWEEN grid times ------------------------------------------------------------------------------
 * Between two grid times there is no measurement, so given the states at the two ends of a step the state at t inside it follows
 * the bridge of the prior IWP (x) K, under the prior and under every posterior alike.  With h = dt, theta = (t - t_k) / h in (0, 1),
 * in the Nordsieck frame of h, p_a = nu - a + 1/2:
 *     A_th[a,b] = A1[a,b] th^(p_a - p_b),   Q_th[a,b] = Q1[a,b] th^(p_a + p_b)      (entry by entry; likewise with 1 - th)
 *     B+ = Q_th A_(1-th)^T Q1^-1,   B- = (I - B+ A_(1-th)) A_th,   Qb = (I - B+ A_(1-th)) Q_th (.)^T + B+ Q_(1-th) B+^T     (n x n, host)
 *     x_t | x_k, x_{k+1} ~ N((B- (x) I) x_k + (B+ (x) I) x_{k+1}, Qb (x) K)
 *     ms_t = (B- (x) I) ms_k + (B+ (x) I) ms_{k+1}
 *     Ps_t = (B-) Ps_k (B-)^T + (B-) C_k (B+)^T + ((B-) C_k (B+)^T)^T + (B+) Ps_{k+1} (B+)^T + Qb (x) K,     C_k = G_k Ps_{k+1}
 * (the same coefficients as pnmol/base/iwp.py, `bridge_coefficients`).  C_k is the lag-one cross-covariance the smoother step forms
 * anyway.  No factorisation is involved: a marginal needs the n x n blocks of Ps_k, C_k, Ps_{k+1} at equal mesh points only.
 * Like the smoother these entry points use the prior alone (uncalibrated) and serve the fp64 white-noise filters; a latent-force
 * (d_state = 2d) or fp32 filter gives -1.
 *
 * `pnmol_state_predict`: out = N(A m, A P A^T + Q) at in->t + dt, the prior carried over dt > 0 from `in` (any frame, unchanged;
 * out may not alias it), an ordinary state in the frame of dt.  No measurement, no use of the filter's step buffers or captured
 * graphs, no synchronisation.  Dense output of a filtering solution, forecasts past the last grid time.
 * `pnmol_state_predict_marginals`: mean and marginal std of all n derivatives of that prediction for nq step sizes dt_q[i] >= 0
 * at once (0: the state's own values), (nq, n, d) row-major each, raw coordinates; either output may be NULL.  One gather of the
 * state's point-diagonal blocks, one evaluation launch, the read-out copied straight into the caller's arrays, one synchronisation.  -1: a negative or non-finite dt_q. */
int pnmol_state_predict(pnmol_filter* f, const pnmol_state* in, double dt, pnmol_state* out);
int pnmol_state_predict_marginals(pnmol_filter* f, const pnmol_state* in, int nq, const double* dt_q, double* means_qnd,
                                  double* stds_qnd);
/* Exactly `pnmol_smoother_step` (same kernels, `out` bit for bit the same, same errors) that also returns a bridge for the
 * interval [filt_k->t, filt_k->t + dt].  The bridge owns, in the frame of dt: both smoothed means, the n x n blocks at equal mesh
 * points of Ps_k, C_k and Ps_{k+1}, diag K ((3 n^2 + 2 n + 1) dp doubles) and, with keep_full != 0, all of C_k (Dp^2 doubles).  It
 * references no state (it copies what it needs: one small launch, with keep_full one device copy more; the blocks of a filter's
 * bridges are carved out of device allocations of 64 blocks, each freed when the last bridge in it is destroyed) and keeps its filter alive
 * exactly as a state does.  On any error *bridge is NULL. */
int pnmol_smoother_step_bridge(pnmol_filter* f, const pnmol_state* filt_k, const pnmol_state* smooth_next, double dt,
                               pnmol_state* out, int keep_full, pnmol_bridge** bridge);
int pnmol_bridge_destroy(pnmol_bridge* b);
int pnmol_bridge_get_interval(const pnmol_bridge* b, double* t, double* dt, int* has_full); /* any output may be NULL */
/* Mean and marginal std of all n derivatives at nq times inside [t_k, t_k + dt], (nq, n, d) row-major each, raw coordinates
 * (either output may be NULL): one launch for all queries, the read-out copied straight into the caller's arrays, one
 * synchronisation.  A time equal to an end point
 * (16 ulp) returns that end's stored values, not the formula.  Variances are clamped at 0 before the root.  -1: a time outside the
 * interval or not finite, nq < 1. */
int pnmol_bridge_eval(const pnmol_bridge* b, int nq, const double* t_q, double* means_qnd, double* stds_qnd);
/* The full posterior at t_k < t < t_k + dt as an ordinary state in the frame of dt (mean, covariance, marginal variances), so that
 * `pnmol_state_get_cov`, `_cov_sqrtm`, `pnmol_samples_draw` work on it.  smooth_k / smooth_next: the smoothed states at the two
 * ends (the `out` and `smooth_next` of the step that made the bridge, in any frame, unchanged; out may alias neither).  One pass
 * over the three Dp x Dp matrices, symmetric bit for bit; no synchronisation.  -1: a bridge without keep_full, states of another
 * filter or not at the bridge's two times (16 ulp, the rule of `pnmol_samples_step_back`), t not strictly inside the interval. */
int pnmol_bridge_state(const pnmol_bridge* b, const pnmol_state* smooth_k, const pnmol_state* smooth_next, double t,
                       pnmol_state* out);

/* Joint draws of whole trajectories from the smoothing posterior ----------------------------------------------------------------
 * The posterior over the trajectory factorises backwards (the chain behind kalman.py:33-46 of the reference): in the Nordsieck
 * frame of the step dt, A = A1 (x) I, Q = Q1 (x) K (prior only, uncalibrated, as in `pnmol_smoother_step`),
 *     x_T ~ N(m_T, P_T),    x_k | x_{k+1} ~ N(m_k + G_k (x_{k+1} - A m_k), P_k - G_k P-_k G_k^T),   G_k = P_k A^T (P-_k)^-1.
 * A backward step draws from it by Matheron's rule, with C C^T = P_k and Gamma_Q = chol(Q1) (x) Gamma:
 *     xt = m_k + scale C xi_1,     x_k = xt + G_k (x_{k+1} - A xt - scale Gamma_Q xi_2),     xi_1, xi_2 ~ N(0, I_D).
 * `scale` = 1 draws from the posterior the states carry; scale = sqrt(calibrated diffusion) draws from the calibrated one (the
 * gain does not depend on the covariance scale).  C is the sweep's Cholesky factor with the dropped-pivot rule of
 * `pnmol_state_get_cov_sqrtm` (noise-free Dirichlet nodes give zero columns), after every entry of P_k has been held to
 * |P_ij| <= sqrt(P_ii P_jj) (no change to a PSD matrix; removes rounding noise around zero variances); P- >= Q is factorised strictly.  The gain is not
 * formed: the step runs the smoother's sweep [P-; P A^T; 0; I] -> [L; V; 0; L^-T] and applies V (L^-1 r) as two thin products.
 *
 * A `pnmol_samples` holds S draws at one time, as a device-resident (Dp x Sp) block in the frame of the last step taken
 * (converted on read-out, like a state); Sp = S rounded up to 64.  It keeps its filter alive exactly as a state does.  Memory:
 * 6 Dp Sp + 2 S D doubles per block; per filter, on the first draw, 2 Dp^2 doubles (P^h and its factor) + dp^2 (Gamma), and on
 * the first backward step the smoother's workspace (~9 Dp^2 doubles, shared with `pnmol_smoother_step`).  num_samples is
 * limited by memory only.
 *
 * Noise: `xi` is a host buffer of standard normals, one row per draw: (S, D) for `pnmol_samples_draw`, (S, 2D) for
 * `pnmol_samples_step_back` (xi_1 in the first D columns, xi_2 in the last D).  Column c of xi_1 is input c of the factor C,
 * which is computed in the F-flattened order (index j*n + a, the order of `pnmol_state_get_cov_sqrtm`); column a*d + j of xi_2
 * drives derivative a at mesh point j of Gamma_Q.  Which direction of the state a column moves depends on the factors: only
 * the distribution of the result is contract.  xi = NULL: generated on the device, nothing crosses the bus.
 *
 * Generator (`xi` = NULL, and `pnmol_sample_noise`): Philox4x32-10 (Salmon et al., SC'11) + Box-Muller in fp64.  For draw i
 * (row) and the pair of columns (2p, 2p+1): counter = (p, i, step_index & 0xffffffff, step_index >> 32), key = (seed &
 * 0xffffffff, seed >> 32), output words w0..w3;  u1 = ((w0 + 2^32 (w1 & 0xfffff)) + 1/2) 2^-52,  u2 = the same of (w2, w3)
 * (52 bits, exactly representable, inside (0, 1): no log(0));  column 2p = sqrt(-2 ln u1) cospi(2 u2), column 2p+1 =
 * sqrt(-2 ln u1) sinpi(2 u2).  So a value depends on (seed, step_index, i, column) only: the same arguments give the same bits,
 * the first 8 of 64 draws are the 8 draws of an 8-draw block, different seeds / step indices are independent streams.
 *
 * Errors: -1 null handles, a latent-force (d_state = 2d) or fp32 filter, a state of another filter, dt <= 0, num_samples < 1,
 * non-finite scale, `step_back` / `get` on a block that holds no draw, `step_back` whose filt_k->t + dt differs from the
 * block's time by more than 16 ulp (steps out of order); -3 / -4 / -2 as in `pnmol_smoother_step` (after -2 / -3 the block
 * holds no draw).  One stream synchronisation per call (the pivot check; `pnmol_samples_draw` has one too, for the NaN check of
 * its factor).  The input states are never modified. */
int pnmol_samples_create(pnmol_filter* f, int num_samples, pnmol_samples** out);
int pnmol_samples_destroy(pnmol_samples* x);
/* x <- m + scale C xi, C C^T = cov(s): the terminal draw (usable on any state of the filter, e.g. a smoothed one); the block
 * takes the state's time and frame.  xi_SD (S, D) or NULL (device generator with (seed, step_index)). */
int pnmol_samples_draw(pnmol_samples* x, const pnmol_state* s, const double* xi_SD, unsigned long long seed,
                       unsigned long long step_index, double scale);
/* One backward step, in place: x holds draws at filt_k->t + dt on entry and at filt_k->t on return.  xi_S2D (S, 2D) or NULL. */
int pnmol_samples_step_back(pnmol_samples* x, const pnmol_state* filt_k, double dt, const double* xi_S2D,
                            unsigned long long seed, unsigned long long step_index, double scale);
/* Draws BETWEEN (or behind) the times of drawn blocks (dense output, see "Dense output" above).  Given the draws in `left` and
 * `right`, left->t < t < right->t with no grid time strictly between them, the state at t follows the prior's bridge whatever the
 * data: in the frame of h = right->t - left->t, theta = (t - left->t) / h,
 *     x_t = (B- (x) I) x_l + (B+ (x) I) x_r + scale (chol(Qb) (x) Gamma) xi,      xi ~ N(0, I_D),
 * no posterior quantity enters.  `out` (a block of the same filter and num_samples, aliasing neither input) receives draws at t
 * that are coupled to those in `left` and `right`; it may itself serve as a neighbour of a further time (several times inside one
 * interval are NOT independent given its ends: draw them one after the other, each between its nearest drawn neighbours).
 * right = NULL: the one-sided case, draws carried forwards from `left` by the prior (B- = A1, B+ = 0, Qb = Q1 in the frame of
 * t - left->t): times beyond the last grid time.  xi_SD (S, D), column a*d + j driving derivative a at mesh point j (as xi_2 of
 * `pnmol_samples_step_back`), or NULL for the device generator with (seed, step_index).  The Gamma xi product is the batched thin
 * product of the backward step; the inputs are unchanged.  One stream synchronisation.  -1: null / aliasing / foreign blocks,
 * different num_samples, a block that holds no draw, t not strictly between the blocks' times, non-finite scale. */
int pnmol_samples_interpolate(pnmol_samples* out, const pnmol_samples* left, const pnmol_samples* right, double t,
                              const double* xi_SD, unsigned long long seed, unsigned long long step_index, double scale);
/* A copy of a block (draws, time, frame): a block has to survive the in-place `pnmol_samples_step_back` that produces its left
 * neighbour. */
int pnmol_samples_clone(const pnmol_samples* x, pnmol_samples** out);
int pnmol_samples_get(const pnmol_samples* x, double* x_Snd); /* (S, n, d) row-major, raw coordinates */
int pnmol_samples_get_time(const pnmol_samples* x, double* t);
/* The device generator by itself: out (rows, cols) row-major = what a NULL xi of that shape would have used. */
int pnmol_sample_noise(pnmol_ctx* ctx, unsigned long long seed, unsigned long long step_index, int rows, int cols, double* out);

/* k steps of constant dt with no host synchronisation in between -- the loop body of
 * `PDEFilter.solution_generator` under `step.Constant` (pdefilter.py:140-160,
 * odetools/step.py:30-55).  `s` is advanced in place.  Optional outputs, each written
 * once after the last step: means_kd / stds_kd (k,d) = `sol.mean[1:, 0]` and
 * sqrt(diag(cov) E0^T) per step (figure1.py:76-80, uncalibrated); info_k (k entries). */
int pnmol_filter_steps(pnmol_filter* f, pnmol_state* s, int k, double dt, double* means_kd,
                       double* stds_kd, pnmol_step_out* info_k);

/* The same loop split in two, so that one host thread can keep several contexts (several problems on one GPU, or
 * several GPUs) busy: `_begin` enqueues the k steps and the read-out copies and returns without waiting, `_end`
 * waits for that context's stream and fills the caller's buffers.  One `_begin` may be outstanding per filter. */
int pnmol_filter_steps_begin(pnmol_filter* f, pnmol_state* s, int k, double dt);
int pnmol_filter_steps_end(pnmol_filter* f, pnmol_state* s, double* means_kd, double* stds_kd,
                           pnmol_step_out* info_k);

/* The filtered trajectory out of the constant-step loop -------------------------------------------------------------------------
 * `PDEFilter.solve` of the reference stacks the state behind every step (pdefilter.py:140-160); through this ABI that used to take
 * one `pnmol_filter_step` call, one synchronisation, one state and one mean read-back per step.  A recorder makes the loop above do
 * it: `pnmol_filter_set_recorder(f, count, slots)` names caller-owned states of f, and slots[i] receives the state behind the i-th
 * step taken from then on -- mean, full covariance and marginal variances in the frame of dt, copied on the device behind the
 * step's read-out (one launch of k_record per step, the slot index taken from device words, so the captured graphs of the loop
 * replay as before; no host round trip).  Steps are counted across successive `pnmol_filter_steps(_begin)` calls by a cursor, like
 * the sensor plan's.  A step with a planned sensor update behind it records the conditioned state.  `_end` gives the call's slots
 * their time and frame and moves the cursor; after a -2 / -3 the cursor has moved past the call and the slots from the failing step
 * on are undefined (the sensor plan's rule).
 * count = 0 or slots = NULL clears.  The call copies the list, uploads the device table of the slots' buffers and drops the captured
 * graphs (the launch sequence differs with a recorder).  -1, nothing changed, reason in `pnmol_last_error`: a null slot, a slot of
 * another filter, a slot listed twice, an fp32 filter, a call between `pnmol_filter_steps_begin` and `_end`.  -4: out of memory.
 * With a recorder set
 *   - `pnmol_filter_steps_begin(f, s, k, dt)` returns -1 before anything is enqueued, `s` untouched, when k exceeds the slots left
 *     or `s` is one of the slots;
 *   - the loop runs its self-contained steps (as with a term or a pending sensor plan): the fused steady-state launch never writes
 *     the posterior covariance.  A filter without a recorder takes the launches it always took, and one whose recorder is cleared
 *     gives the bits of a filter that never had one;
 *   - `pnmol_state_destroy` of a slot returns -1 (clear the recorder first); `pnmol_filter_destroy` clears the recorder before its
 *     own checks.
 * fp64 filters, white-noise and latent-force, with or without a term, with or without a sensor plan; `pnmol_filter_step` records
 * nothing.  Memory: the slots themselves (Dp^2 + 2 Dp doubles each) and count Dp doubles of scratch.
 * `pnmol_filter_recorder_pending`: the cursor (the slot the next step fills) and the number of slots (0, 0: no recorder).
 * `pnmol_filter_recorder_means`: the means of the filled slots [first, first + count) as (count, n, d_state) row-major, raw
 * coordinates -- what `pnmol_state_get_mean` gives per state, gathered on the device and read back with one copy and one
 * synchronisation.  -1: no recorder, a slot that has not been filled, an unfinished `pnmol_filter_steps_begin`. */
int pnmol_filter_set_recorder(pnmol_filter* f, int count, pnmol_state* const* slots);
int pnmol_filter_recorder_pending(const pnmol_filter* f, int* next, int* count);
int pnmol_filter_recorder_means(pnmol_filter* f, int first, int count, double* means_cnd);

/* The whole backward pass of the RTS smoother in one call: what T calls of `pnmol_smoother_step` compute (kalman.py:33-46 of the
 * reference per step; the same kernels in the same order, so the same bits), for k = T-1 .. 0 enqueued back to back on the ctx
 * stream with ONE synchronisation at the end instead of one per step, no state allocated per step and no mean read back per step.
 * filt (T+1 states: the filtered trajectory, e.g. a recorder's slots behind the initial state), dt_T[k] = the step from filt[k] to
 * filt[k+1].  Each step's sweep info word is kept on the device in a per-step array before the next step resets it.
 * means_T1d / stds_T1d ((T+1, d) row-major, either may be NULL): the smoothed read-outs s0 m[j] and s0 sqrt(max(var_j, 0)) of
 * derivative 0, written on the device by k_sm_readout with the arithmetic of the loop's read-out; row T is the terminal filtered
 * state's.  out = NULL: the pass rotates two internal states (2 (Dp^2 + 2 Dp) doubles, allocated on the first such call and kept
 * by the filter), so memory does not grow with T.  out (T+1 states): out[k] receives the smoothed state at filt[k]->t in the frame
 * of dt_T[k], out[T] a copy of filt[T].
 * Returns 0, or the -2 / -3 of the first failing step in backward order (`pnmol_last_error` names the step; info_T[k], optional,
 * holds 0 / -2 / -3 per step); the outputs of the steps behind it (lower k) are undefined then.  -1 before anything is enqueued:
 * the refusals of `pnmol_smoother_step` (null, foreign state, dt <= 0, latent-force or fp32 filter), T < 1, a state listed twice
 * in out, a state of out that is one of filt.  -4: out of memory.  No bridges are made: dense output keeps
 * `pnmol_smoother_step_bridge`. */
int pnmol_smoother_steps(pnmol_filter* f, int T, pnmol_state* const* filt, const double* dt_T, pnmol_state* const* out,
                         double* means_T1d, double* stds_T1d, int* info_T);

/* The exact smoothing posterior of Q linear functionals of the whole trajectory, q = sum_k W_k x_k (k = 0 .. T, x_k the state at
 * filt[k]->t, W_k: Q x D): mean_Q (Q) and cov_QQ (Q x Q row-major, symmetric to the bit), uncalibrated like every covariance here.
 * filt (T+1 states) and dt_T as for `pnmol_smoother_steps`; w_QT1nd: the weights, (Q, T+1, n, d) row-major in raw coordinates --
 * entry (q, k, a, j) multiplies derivative a at mesh point j of x_k.  Only the filtered states enter: the adjoint of the backward
 * recursion behind `pnmol_smoother_step` runs in ascending k (csrc/pnmol_functional.hip has the recursion), so no smoothed state
 * and no gain is formed.  Per step one sweep of [P-; (A U)^T] (the Cholesky factorisation of the predicted covariance with
 * PNMOL_FUNCTIONALS_MAX_Q extra rows) and work that is thin in Q; the T steps are enqueued back to back on the ctx stream with ONE
 * synchronisation at the end.  T = 0 is valid: W_0 m_0 and W_0 P_0 W_0^T.  The workspace ((3 Dp + 320) Dp doubles and the
 * weights of the largest call) is allocated on the first call and freed with the filter.  The states are only read; a recorder, an
 * observation plan, a term, linearisation points and the captured graphs of the filter are not touched.
 * Returns 0; -2 / -3 of the first failing step (`pnmol_last_error` names it), the outputs are untouched then; -4 out of memory;
 * -1 before anything is enqueued, with the reason in `pnmol_last_error`: a null pointer, Q < 1, Q > PNMOL_FUNCTIONALS_MAX_Q,
 * T < 0, dt <= 0 or not finite, weights that are not finite, a null or foreign state, a latent-force or fp32 filter, a call
 * between `pnmol_filter_steps_begin` and `_end`. */
#define PNMOL_FUNCTIONALS_MAX_Q 64
int pnmol_functionals(pnmol_filter* f, int T, pnmol_state* const* filt, const double* dt_T, int Q, const double* w_QT1nd,
                      double* mean_Q, double* cov_QQ);

/* Optional: do the one-off host work of a following `pnmol_filter_steps(f, s, k, dt, ...)` now
 * (output buffers, capture + instantiation of the hipGraphs the step loop is replayed from). */
int pnmol_filter_prepare_steps(pnmol_filter* f, pnmol_state* s, int k, double dt);

/* timing hooks for bench.py: HIP events on the ctx stream around the last `steps` call */
int pnmol_filter_last_steps_ms(pnmol_filter* f, float* ms);

/* debugging / tests: copy an internal device buffer to the host.
 * which: 0 = predicted covariance (Dp*Dp, derivative-major padded), 1 = G work matrix,
 * 2 = F factor matrix [Ls; W; r^T], 3 = predicted mean (Dp), 4 = z (mp).  `count` doubles. */
int pnmol_filter_debug_read(pnmol_filter* f, int which, double* dst, long count);
/* Test hook: fills the buffers the sweep kernels hand data over through (F, the L_jj^-1 tiles, the feed / scratch tiles) with
 * NaN, as stale contents of an earlier launch.  A following step must give the same bits as without it
 * (tests/test_gpu_parity.py::test_stale_hand_over_buffers_are_never_read): every reader takes published data only. */
int pnmol_filter_debug_poison(pnmol_filter* f);
int pnmol_filter_dims(const pnmol_filter* f, int* d, int* n, int* m, int* dp, int* mp);

#ifdef __cplusplus
}
#endif
#endif /* PNMOL_HIP_H */
