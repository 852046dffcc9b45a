// pnmol_reaction.hip -- pointwise reaction terms evaluated on the device (`pnmol_filter_set_reaction`,
// `pnmol_filter_linearize`, include/pnmol_hip.h): the kernel, then the host side.
//
// Semilinear EK1 (white.py:189-208) for u_t = L u + r(u) with a pointwise r(u) = P(u) + A(u) / B(u) (polynomials with scalar
// coefficients): the linearisation at the predicted mean u = E0 m^- is M = L + diag(r'(u)) with shift r'(u) u - r(u).
// k_linearize forms u from the step's input mean (the arithmetic of pnmol_filter_predict_mean), evaluates r and r' by
// Horner and patches the diagonal slots of the stencil rows and the shift, as k_operator_diagonal does from a host buffer.
// Nothing crosses the bus, so the constant-step loop re-linearises in front of every step (launch_step's callers in
// pnmol_hip.hip) and stays on the device.
//
// Coupled systems of C <= 4 species (`pnmol_filter_set_reaction_system`; Lotka-Volterra, SIR): r_c depends on all species at the
// same mesh point, so row c N + j of the Jacobian has C entries, at the columns k N + j.  The setter widens the stencil image
// of L by those columns once (system_term_image), and k_linearize_system patches the C same-point slots of every row.
//
// Convection terms (`pnmol_filter_set_convection`; viscous Burgers, Burgers-Fisher): f(u)_i = c(u_i) (G u)_i + r(u_i) with a
// stencil operator G.  The Jacobian diag(c) G + diag(c' G u + r') touches every entry of a stencil row, so the setter builds the
// union image of L and G with G's value beside every slot (convection_term_image) and k_linearize_convection rewrites all slots
// of a row; the shift (c' g + r') u - r needs no product with G (the c g terms of J u - f cancel).
//
// The three kinds share the predicted value and the rational evaluation on the device, and one image (pnmol_term_image.hpp), one
// capability check and one installer (install_term) on the host; a filter holds one term (pnmol_filter::term).
//
// Linearisation points (`pnmol_filter_set_linearization_points`, `pnmol_filter_linearize_at`): an iterated smoother repeats the
// forward pass with every step linearised at the previous pass's smoothed mean.  The three kernels take their point from one
// helper (point_value): the predicted value as above, or the entry of a row of a device-resident table, which the launch finds
// from two device words and the loop's step counter (point_row) -- identical arguments at every step, as the recorder's k_record.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "pnmol_internal.hpp"
#include "pnmol_linearize_plan.hpp"
#include "pnmol_term_image.hpp"

namespace {

// what a kernel needs to form the predicted mean from the step's input mean
struct Frame {
    double c[MAXN];  // A1[0][a] * ts[a]: row 0 of the transition times the frame change of the input mean
    double s0;       // raw-coordinate scale of derivative 0 in the frame of dt
};
// where a launch takes its linearisation point from.  u == nullptr: the step's own predicted mean.  Otherwise rows of d numbers
// (derivative 0, raw coordinates): with words, row words[0] + *ctr of words[1] -- the cursor of the running call plus the loop's step
// counter, which k_predict moves only behind this launch, so the step that takes *ctr to j + 1 is linearised at row cursor + j and
// every step launches with identical arguments (the captured graphs of the loop replay at any position); without words, row 0
// (pnmol_filter_linearize_at).
struct PointSource {
    const double* u;
    const int* words;
    const int* ctr;
    int d;
};
template <class Descriptor>
struct LinearizeArgs {
    Descriptor t;
    Frame fr;
    PointSource pt;
};

// derivative 0 of the predicted mean at state component j, in raw coordinates: the arithmetic of pnmol_filter_predict_mean
__device__ __forceinline__ double predicted_value(const Frame& fr, int n, const double* __restrict__ mean, int dp, int j) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int q = 0; q < n; ++q) acc = acc + fr.c[q] * mean[(long)q * dp + j];
    return fr.s0 * acc;
}

// The row of this launch (nullptr: the predicted mean).  false: an index outside the table -- the launch reads and writes nothing
// (the host refuses such calls before they are enqueued; this is the bound of the table all the same).
__device__ __forceinline__ bool point_row(const PointSource& pt, const double*& row) {
    row = nullptr;
    if (!pt.u) return true;
    int r = 0;
    if (pt.words) {
        r = pt.words[0] + *pt.ctr;
        if (r < 0 || r >= pt.words[1]) return false;
    }
    row = pt.u + (long)r * pt.d;
    return true;
}

// the point a term is linearised at, component j: the table's entry, or the predicted value with its arithmetic untouched
__device__ __forceinline__ double point_value(const Frame& fr, int n, const double* __restrict__ mean, int dp, int j,
                                              const double* __restrict__ row) {
    return row ? row[j] : predicted_value(fr, n, mean, dp, j);
}

// value and derivative of a polynomial (ascending coefficients, degree deg; deg < 0: absent, both zero), by Horner
__device__ inline void horner(const double* __restrict__ c, int deg, double u, double& v, double& dv) {
#pragma clang fp contract(off)
    v = 0.0, dv = 0.0;
    if (deg < 0) return;
    v = c[deg];
    for (int k = deg - 1; k >= 0; --k) v = v * u + c[k];
    if (deg < 1) return;
    dv = deg * c[deg];
    for (int k = deg - 1; k >= 1; --k) dv = dv * u + k * c[k];
}

// r = P + A / B and r' = P' + (A' B - A B') / B^2 at u (without a rational part: P and P')
__device__ __forceinline__ void eval_reaction(const pnmol_reaction& t, double u, double& r, double& dr) {
#pragma clang fp contract(off)
    double P, dP, A, dA, B, dB;
    horner(t.p, t.deg_p, u, P, dP);
    r = P, dr = dP;
    if (t.deg_a >= 0) {
        horner(t.a, t.deg_a, u, A, dA);
        horner(t.b, t.deg_b, u, B, dB);
        r = P + A / B;
        dr = dP + (dA * B - A * dB) / (B * B);
    }
}

// One thread per measurement row.  Every operation is rounded on its own (no contraction into fused multiply-adds): the
// results are those of the same formulas in NumPy (pnmol/pde/reactions.py), bit for bit.
__global__ __launch_bounds__(256) void k_linearize(LinearizeArgs<pnmol_reaction> a, int n, const double* __restrict__ mean,
                                                   double* __restrict__ ell_val, const double* __restrict__ base_val,
                                                   const int* __restrict__ slot, double* __restrict__ shift, int d, int dp,
                                                   int mp) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp) return;
    const double* row;
    if (!point_row(a.pt, row)) return;
    if (i >= d) {
        shift[i] = 0.0;
        return;
    }
    const double u = point_value(a.fr, n, mean, dp, i, row);
    double r, dr;
    eval_reaction(a.t, u, r, dr);
    const long e = (long)slot[i] * mp + i;
    ell_val[e] = base_val[e] - dr;
    shift[i] = dr * u - r;
}

// ---- coupled systems: r_c(u) = P_c(u) + A_c(u) / B_c(u) of the C species at one mesh point (pnmol_filter_set_reaction_system)
constexpr int SC = PNMOL_SYSTEM_MAXCOMP;

// coef * u_0^pw[0] * u_1^pw[1] * ..., one multiplication at a time, species by species; `less` takes one factor off that species
__device__ __forceinline__ double monomial(double start, const int (&pw)[SC], int less, const double (&u)[SC]) {
#pragma clang fp contract(off)
    double m = start;
#pragma unroll
    for (int k = 0; k < SC; ++k) {
        const int cnt = pw[k] - (k == less ? 1 : 0);
        for (int e = 0; e < cnt; ++e) m = m * u[k];
    }
    return m;
}

// value and the SC partial derivatives of a polynomial: the sum of its terms in the order given, starting from the first one
// (a term whose exponent of u_k is 0 is no term of the k-th derivative).  The descriptor sits in the kernel-argument segment and
// every index into it is uniform across the wave; u and the sums stay in registers (all loops over species are unrolled).
__device__ __forceinline__ void poly_eval(const pnmol_system_poly& p, const double (&u)[SC], double& v, double (&dv)[SC]) {
#pragma clang fp contract(off)
    v = 0.0;
#pragma unroll
    for (int k = 0; k < SC; ++k) dv[k] = 0.0;
    bool first = true, dfirst[SC];
#pragma unroll
    for (int k = 0; k < SC; ++k) dfirst[k] = true;
    for (int t = 0; t < p.nterms; ++t) {
        const double coef = p.term[t].coef;
        int pw[SC];
#pragma unroll
        for (int k = 0; k < SC; ++k) pw[k] = p.term[t].pow[k];
        const double m = monomial(coef, pw, -1, u);
        v = first ? m : v + m;
        first = false;
#pragma unroll
        for (int k = 0; k < SC; ++k) {
            if (pw[k] >= 1) {
                const double dm = monomial(pw[k] * coef, pw, k, u);
                dv[k] = dfirst[k] ? dm : dv[k] + dm;
                dfirst[k] = false;
            }
        }
    }
}

// One thread per measurement row i = c N + j: the C species at point j, r_c and its C partial derivatives, the C same-point slots
// of the row and its shift.  Every operation is rounded on its own, in the order of SystemReaction (pnmol/pde/reactions.py).
__global__ __launch_bounds__(256) void k_linearize_system(LinearizeArgs<pnmol_reaction_system> a, int n, int N,
                                                          const double* __restrict__ mean, double* __restrict__ ell_val,
                                                          const double* __restrict__ base_val, const int* __restrict__ slot,
                                                          double* __restrict__ shift, int d, int dp, int mp) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp) return;
    const double* row;
    if (!point_row(a.pt, row)) return;
    if (i >= d) {
        shift[i] = 0.0;
        return;
    }
    const int C = a.t.ncomp;
    const int c = i / N, j = i - c * N;
    double u[SC];
#pragma unroll
    for (int k = 0; k < SC; ++k) u[k] = k < C ? point_value(a.fr, n, mean, dp, k * N + j, row) : 0.0;
    double r = 0.0, J[SC];
#pragma unroll
    for (int k = 0; k < SC; ++k) J[k] = 0.0;
    // the component is uniform across a wave except where a wave straddles two species blocks: the descriptor is indexed by the
    // loop counter, never by the thread's own c
#pragma unroll
    for (int cc = 0; cc < SC; ++cc) {
        if (cc == c) {
            double P, dP[SC];
            poly_eval(a.t.p[cc], u, P, dP);
            r = P;
#pragma unroll
            for (int k = 0; k < SC; ++k) J[k] = dP[k];
            if (a.t.a[cc].nterms > 0) {
                double A, dA[SC], B, dB[SC];
                poly_eval(a.t.a[cc], u, A, dA);
                poly_eval(a.t.b[cc], u, B, dB);
                r = P + A / B;
#pragma unroll
                for (int k = 0; k < SC; ++k) J[k] = dP[k] + (dA[k] * B - A * dB[k]) / (B * B);
            }
        }
    }
    double Ju = J[0] * u[0];
#pragma unroll
    for (int k = 0; k < SC; ++k) {
        if (k < C) {
            const long e = (long)slot[(long)k * mp + i] * mp + i;
            ell_val[e] = base_val[e] - J[k];
            if (k >= 1) Ju = Ju + J[k] * u[k];
        }
    }
    shift[i] = Ju - r;
}

// ---- convection terms: f(u)_i = c(u_i) (G u)_i + r(u_i) (pnmol_filter_set_convection)
// One thread per measurement row i: u_i and the u of the row's slot columns (recomputed per slot: one launch, no grid-wide
// dependency), g_i = (G u)_i over the entries of G that are not zero in slot (= ascending column) order starting from the first
// product, c, c', r, r' by Horner, q = c' g + r'; every slot becomes base - c G, the diagonal one loses q as well, and the shift
// is q u - r.  Every operation is rounded on its own, in the order of Convection.linearization (pnmol/pde/reactions.py).
// img_col / img_val / img_g: the union image of the creation-time operator and G (w slots, packed to the front of every row).
__global__ __launch_bounds__(256) void k_linearize_convection(LinearizeArgs<pnmol_convection> a, int n, int w,
                                                              const double* __restrict__ mean, double* __restrict__ ell_val,
                                                              const int* __restrict__ img_col, const double* __restrict__ img_val,
                                                              const double* __restrict__ img_g, const int* __restrict__ slot,
                                                              double* __restrict__ shift, int d, int dp, int mp) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp) return;
    const double* row;
    if (!point_row(a.pt, row)) return;
    if (i >= d) {
        shift[i] = 0.0;
        return;
    }
    const double u = point_value(a.fr, n, mean, dp, i, row);
    double g = 0.0;
    bool first = true;
    for (int e = 0; e < w; ++e) {
        const int col = img_col[(long)e * mp + i];
        if (col < 0) break;
        const double gv = img_g[(long)e * mp + i];
        if (gv == 0.0) continue;
        const double prod = gv * point_value(a.fr, n, mean, dp, col, row);
        g = first ? prod : g + prod;
        first = false;
    }
    double cu, dcu, r, dr;
    horner(a.t.c, a.t.deg_c, u, cu, dcu);
    eval_reaction(a.t.r, u, r, dr);
    double q = dcu * g;
    if (a.t.r.deg_p >= 0 || a.t.r.deg_a >= 0) q = q + dr;
    const int ds = slot[i];
    for (int e = 0; e < w; ++e) {
        const long at = (long)e * mp + i;
        if (img_col[at] < 0) break;
        double v = img_val[at] - cu * img_g[at];
        if (e == ds) v = v - q;
        ell_val[at] = v;
    }
    shift[i] = q * u - r;
}

bool all_finite(const double* c, int deg) {
    for (int k = 0; k <= deg; ++k)
        if (!std::isfinite(c[k])) return false;
    return true;
}

// why a reaction descriptor is refused, or nullptr
const char* reaction_descriptor_fault(const pnmol_reaction* r) {
    const int degs[3] = {r->deg_p, r->deg_a, r->deg_b};
    for (int g : degs)
        if (g < -1 || g > PNMOL_REACTION_MAXDEG) return "a degree outside [-1, 7]";
    if ((r->deg_a < 0) != (r->deg_b < 0)) return "the numerator a and the denominator b are given together or not at all";
    if (!(all_finite(r->p, r->deg_p) && all_finite(r->a, r->deg_a) && all_finite(r->b, r->deg_b)))
        return "a coefficient is not finite";
    if (r->deg_b >= 0) {
        bool zero = true;
        for (int k = 0; k <= r->deg_b; ++k) zero = zero && r->b[k] == 0.0;
        if (zero) return "the denominator b is identically zero";
    }
    return nullptr;
}

// why a system descriptor is refused, or nullptr
const char* system_descriptor_fault(const pnmol_reaction_system* r) {
    if (r->ncomp < 1 || r->ncomp > PNMOL_SYSTEM_MAXCOMP) return "ncomp outside [1, 4]";
    for (int c = 0; c < r->ncomp; ++c) {
        const pnmol_system_poly* polys[3] = {&r->p[c], &r->a[c], &r->b[c]};
        for (const pnmol_system_poly* p : polys)
            if (p->nterms < 0 || p->nterms > PNMOL_SYSTEM_MAXTERMS) return "a term count outside [0, 8]";
        for (const pnmol_system_poly* p : polys)
            for (int t = 0; t < p->nterms; ++t)
                for (int k = 0; k < PNMOL_SYSTEM_MAXCOMP; ++k) {
                    if (p->term[t].pow[k] < 0 || p->term[t].pow[k] > 7) return "an exponent outside [0, 7]";
                    if (k >= r->ncomp && p->term[t].pow[k] != 0) return "a non-zero exponent of a species >= ncomp";
                }
        if ((r->a[c].nterms > 0) != (r->b[c].nterms > 0))
            return "the numerator a[c] and the denominator b[c] are given together or not at all";
        for (const pnmol_system_poly* p : polys)
            for (int t = 0; t < p->nterms; ++t)
                if (!std::isfinite(p->term[t].coef)) return "a coefficient is not finite";
        if (r->b[c].nterms > 0) {
            bool zero = true;
            for (int t = 0; t < r->b[c].nterms; ++t) zero = zero && r->b[c].term[t].coef == 0.0;
            if (zero) return "a denominator b[c] is identically zero";
        }
    }
    return nullptr;
}

// what every term setter asks of the filter once the descriptor is in order (`path`: what the filter lacks), or empty
std::string capability_fault(const pnmol_filter* f, const char* path) {
    if (f->ds != f->d) return std::string("a latent-force filter (d_state != d) has no ") + path;
    if (f->p32) return std::string("an fp32 filter has no ") + path;
    if (!f->base_has_diag) return "a row of the operator given at creation has no diagonal entry";
    return {};
}

// a reaction system and a convection term widen the image themselves, and so does a time-dependent operator: one at a time
const char* const FAMILY_HOLDS_THE_IMAGE =
    "a time-dependent operator is set (pnmol_filter_set_operator_family): clear it first, both bring a widened image of their own";

int refuse(pnmol_filter* f, const char* who, const std::string& why) {
    f->ctx->err = std::string(who) + why;
    return -1;
}

// the descriptor as the kernels take it: coefficients above a degree are zero
void copy_canonical(pnmol_reaction* dst, const pnmol_reaction* r) {
    std::memset(dst, 0, sizeof(*dst));
    dst->deg_p = r->deg_p, dst->deg_a = r->deg_a, dst->deg_b = r->deg_b;
    for (int k = 0; k <= r->deg_p; ++k) dst->p[k] = r->p[k];
    for (int k = 0; k <= r->deg_a; ++k) dst->a[k] = r->a[k];
    for (int k = 0; k <= r->deg_b; ++k) dst->b[k] = r->b[k];
}

void free_term_image(pnmol_filter* f) {
    TermImage& im = f->term_img;
    for (void* q : {(void*)im.col, (void*)im.val, (void*)im.g, (void*)im.slot})
        if (q) (void)hipFree(q);
    im = TermImage{};
}

template <class T>
int upload(pnmol_ctx* ctx, T** dst, const std::vector<T>& src) {
    if (src.empty()) return 0;
    HIPCHK(ctx, hipMalloc(dst, sizeof(T) * src.size()));
    HIPCHK(ctx, hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return 0;
}

// The filter's image for a system of ncomp species or a convection term with G: the base image read back, widened on the host
// (pnmol_term_image.hpp) and kept on the device.  The caller has synchronised the stream: the image replaced here may have been
// read.  The image names its kind only once it is complete.
int build_image(pnmol_filter* f, TermKind kind, int ncomp, const double* G) {
    pnmol_ctx* ctx = f->ctx;
    const int d = f->d, mp = f->mp, bw = f->base_w;
    std::vector<int> bcol((size_t)bw * mp);
    std::vector<double> bval((size_t)bw * mp);
    HIPCHK(ctx, hipMemcpy(bcol.data(), f->ell_col_base, sizeof(int) * bcol.size(), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(bval.data(), f->ell_val_base, sizeof(double) * bval.size(), hipMemcpyDeviceToHost));
    const TermImageHost h = kind == TermKind::system ? system_term_image(bcol, bval, bw, d, mp, ncomp)
                                                     : convection_term_image(bcol, bval, bw, d, mp, G);
    free_term_image(f);
    TermImage& im = f->term_img;
    if (int rc = upload(ctx, &im.col, h.col)) return rc;
    if (int rc = upload(ctx, &im.val, h.val)) return rc;
    if (int rc = upload(ctx, &im.g, h.g)) return rc;
    if (int rc = upload(ctx, &im.slot, h.slot)) return rc;
    im.w = h.w, im.slot_rows = (int)(h.slot.size() / mp), im.kind = kind, im.ncomp = ncomp;
    return 0;
}

// the image of a system or a convection term into ell_col / ell_val (grown if it is wider), and a zero shift
int put_term_image(pnmol_filter* f, TermKind kind, int ncomp, const double* G) {
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    const int mp = f->mp;
    TermImage& im = f->term_img;
    const bool reuse = kind == TermKind::system && im.kind == kind && im.ncomp == ncomp;
    if (!reuse || im.w > f->ell_cap) {
        HIPCHK(ctx, hipStreamSynchronize(st));  // the buffers replaced below may still be read
        if (!reuse)
            if (int rc = build_image(f, kind, ncomp, G)) return rc;
        if (int rc = pnmol_ell_reserve(f, im.w)) return rc;
    }
    HIPCHK(ctx, hipMemcpyAsync(f->ell_col, im.col, sizeof(int) * (size_t)im.w * mp, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(f->ell_val, im.val, sizeof(double) * (size_t)im.w * mp, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(f->shift, 0, sizeof(double) * mp, st));
    f->ellw = im.w;
    f->ell_is_base = 0;  // (pnmol_ell_restore_base copies the columns back)
    return 0;
}

// Make `kind` (none: clear) the filter's term; its descriptor is in place.  The descriptor travels by value in the captured
// launches, width and pointers are baked in too, and the loop's launch sequence differs with and without a term: the graphs go.
// A failure leaves no half-installed term: no image, no term, the operator given at creation.
// A table of linearisation points belongs to the term it was set for: it goes with it.
int install_term(pnmol_filter* f, TermKind kind, int ncomp = 0, const double* G = nullptr) {
    pnmol_drop_graphs(f);
    if (f->lin_points.rows) {
        HIPCHK(f->ctx, hipStreamSynchronize(f->ctx->stream));  // (a launch that reads the table may still be in flight)
        loop_table_clear(f, &f->lin_points);
    }
    const bool image = kind == TermKind::system || kind == TermKind::convection;
    // (a time-dependent operator, pnmol_operator.hip: its image with the current operator is what a pointwise reaction patches)
    const int rc = image ? put_term_image(f, kind, ncomp, G)
                         : (pnmol_operator_family_set(f) ? pnmol_operator_put_image(f) : pnmol_ell_restore_base(f, true));
    f->sq_dt = -1.0;  // the error model belongs to the operator that was set
    f->term = rc ? TermKind::none : kind;
    if (rc) {
        const std::string err = f->ctx->err;
        free_term_image(f);
        if (pnmol_operator_family_set(f)) (void)pnmol_operator_put_image(f);
        else (void)pnmol_ell_restore_base(f, true);
        f->ctx->err = err;
    }
    return rc;
}

// k_linearize (k_linearize_system, k_linearize_convection) on the ctx stream for one step over dt from `mean` (in the frame
// frame_dt), the point taken from `pt`
int enqueue_linearize(pnmol_filter* f, const double* mean, double frame_dt, double dt, const PointSource& pt) {
    Frame fr;
    for (int q = 0; q < MAXN; ++q) fr.c[q] = 0.0;
    for (int q = 0; q < f->n; ++q) {
        const double so = frame_dt == 0.0 ? 1.0 : nordsieck_scale(f->nu, q, frame_dt);
        fr.c[q] = f->iwp.A1[q] * (so / nordsieck_scale(f->nu, q, dt));
    }
    fr.s0 = nordsieck_scale(f->nu, 0, dt);
    const unsigned blocks = (unsigned)((f->mp + 255) / 256);
    hipStream_t st = f->ctx->stream;
    const TermImage& im = f->term_img;
    switch (f->term) {
        case TermKind::none: return -1;
        case TermKind::scalar: {
            // (a time-dependent operator: the current operator and the union image's diagonal slots in place of the base ones)
            const double* base_val = f->ell_val_base;
            const int* slot = f->ell_diag_slot;
            pnmol_operator_linearize_base(f, &base_val, &slot);
            k_linearize<<<blocks, 256, 0, st>>>({f->reaction, fr, pt}, f->n, mean, f->ell_val, base_val, slot, f->shift, f->d, f->dp,
                                                f->mp);
            break;
        }
        case TermKind::system:
            k_linearize_system<<<blocks, 256, 0, st>>>({f->sys, fr, pt}, f->n, f->d / f->sys.ncomp, mean, f->ell_val, im.val, im.slot,
                                                       f->shift, f->d, f->dp, f->mp);
            break;
        case TermKind::convection:
            k_linearize_convection<<<blocks, 256, 0, st>>>({f->cv, fr, pt}, f->n, im.w, mean, f->ell_val, im.col, im.val, im.g,
                                                           im.slot, f->shift, f->d, f->dp, f->mp);
            break;
    }
    HIPCHK(f->ctx, hipGetLastError());
    return 0;
}

}  // namespace

void pnmol_reaction_free_ws(pnmol_filter* f) {
    free_term_image(f);
}

int pnmol_reaction_enqueue(pnmol_filter* f, const double* mean, double frame_dt, double dt, bool loop_step) {
    // only a step of the loop takes its point from the table: the words that name the row belong to the running call
    const LoopTable& l = f->lin_points;
    const PointSource pt = loop_step && l.plan.set() ? PointSource{l.rows, l.words, f->ctr, f->d}
                                                     : PointSource{nullptr, nullptr, nullptr, f->d};
    return enqueue_linearize(f, mean, frame_dt, dt, pt);
}

extern "C" {

int pnmol_filter_set_linearization_points(pnmol_filter* f, int count, const double* u_cd) {
    static const char* who = "pnmol_filter_set_linearization_points: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    const std::string why = linearize_plan_validate(count, u_cd, f->d, has_term(f), f->pending_state != nullptr);
    if (!why.empty()) return refuse(f, who, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (a launch that reads the table may still be in flight)
    if (count == 0 || !u_cd) {
        loop_table_clear(f, &f->lin_points);
        return 0;
    }
    // (a table that fits is overwritten in place: the captured graphs address it through the words)
    return loop_table_install(f, &f->lin_points, who, count, f->d, u_cd);
}

int pnmol_filter_linearization_pending(const pnmol_filter* f, int* next, int* count) {
    return f ? loop_table_pending(f->lin_points, next, count) : -1;
}

int pnmol_filter_linearize_at(pnmol_filter* f, const double* u_d) {
    static const char* who = "pnmol_filter_linearize_at: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    if (!u_d) return refuse(f, who, "bad argument (null point)");
    if (!has_term(f)) return refuse(f, who, "no term set (pnmol_filter_set_reaction, _set_reaction_system, _set_convection)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the staging buffer of pnmol_filter_set_operator_diagonal (refused while a term is set, so free for this): the kernels read the
    // mapped host memory as a table of one row.  It may still be read by the previous call's launch: wait for that launch.
    HIPCHK(ctx, hipEventSynchronize(f->ev_op));
    std::memcpy(f->h_op, u_d, sizeof(double) * (size_t)f->d);
    if (int rc = enqueue_linearize(f, nullptr, 0.0, 1.0, PointSource{f->h_op_dev, nullptr, nullptr, f->d})) return rc;
    HIPCHK(ctx, hipEventRecord(f->ev_op, ctx->stream));
    f->sq_dt = -1.0;  // the operator changed: pnmol_filter_prepare_error_model comes next
    return 0;
}

int pnmol_filter_set_reaction(pnmol_filter* f, const pnmol_reaction* r) {
    static const char* who = "pnmol_filter_set_reaction: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    if (r) {
        const char* fault = reaction_descriptor_fault(r);
        const std::string why = fault ? fault : capability_fault(f, "pointwise reaction path");
        if (!why.empty()) return refuse(f, who, why);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!r) return has_term(f) ? install_term(f, TermKind::none) : 0;  // NULL to any setter clears any kind
    copy_canonical(&f->reaction, r);
    return install_term(f, TermKind::scalar);
}

int pnmol_filter_set_reaction_system(pnmol_filter* f, const pnmol_reaction_system* r) {
    static const char* who = "pnmol_filter_set_reaction_system: ";
    if (!f) return -1;
    if (!r) return pnmol_filter_set_reaction(f, nullptr);
    pnmol_ctx* ctx = f->ctx;
    const char* fault = system_descriptor_fault(r);
    if (!fault && f->d % r->ncomp != 0) fault = "d is not a multiple of ncomp";
    if (!fault && pnmol_operator_family_set(f)) fault = FAMILY_HOLDS_THE_IMAGE;
    const std::string why = fault ? fault : capability_fault(f, "pointwise reaction path");
    if (!why.empty()) return refuse(f, who, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::memset(&f->sys, 0, sizeof(f->sys));
    f->sys.ncomp = r->ncomp;
    for (int c = 0; c < r->ncomp; ++c) {
        const pnmol_system_poly* src[3] = {&r->p[c], &r->a[c], &r->b[c]};
        pnmol_system_poly* dst[3] = {&f->sys.p[c], &f->sys.a[c], &f->sys.b[c]};
        for (int g = 0; g < 3; ++g) {
            dst[g]->nterms = src[g]->nterms;
            for (int t = 0; t < src[g]->nterms; ++t) dst[g]->term[t] = src[g]->term[t];
        }
    }
    return install_term(f, TermKind::system, r->ncomp);
}

int pnmol_filter_set_convection(pnmol_filter* f, const pnmol_convection* term, const double* G_dd) {
    static const char* who = "pnmol_filter_set_convection: ";
    if (!f) return -1;
    if (!term) return pnmol_filter_set_reaction(f, nullptr);
    pnmol_ctx* ctx = f->ctx;
    const char* fault = nullptr;
    if (!G_dd) fault = "a convection term needs its operator G";
    if (!fault && (term->deg_c < -1 || term->deg_c > PNMOL_REACTION_MAXDEG)) fault = "a degree outside [-1, 7]";
    if (!fault) fault = reaction_descriptor_fault(&term->r);
    if (!fault && !all_finite(term->c, term->deg_c)) fault = "a coefficient is not finite";
    if (!fault && pnmol_operator_family_set(f)) fault = FAMILY_HOLDS_THE_IMAGE;
    std::string why = fault ? fault : capability_fault(f, "convection path");
    if (why.empty())
        for (size_t k = 0; k < (size_t)f->d * f->d && why.empty(); ++k)
            if (!std::isfinite(G_dd[k])) why = "an entry of G is not finite";
    if (!why.empty()) return refuse(f, who, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::memset(&f->cv, 0, sizeof(f->cv));
    f->cv.deg_c = term->deg_c;
    for (int k = 0; k <= term->deg_c; ++k) f->cv.c[k] = term->c[k];
    copy_canonical(&f->cv.r, &term->r);
    return install_term(f, TermKind::convection, 0, G_dd);
}

int pnmol_filter_linearize(pnmol_filter* f, const pnmol_state* in, double dt) {
    static const char* who = "pnmol_filter_linearize: ";
    if (!f || !in || in->f != f || !(dt > 0.0)) {
        if (f) f->ctx->err = std::string(who) + "bad argument (null, foreign state or dt <= 0)";
        return -1;
    }
    pnmol_ctx* ctx = f->ctx;
    if (!has_term(f)) return refuse(f, who, "no reaction set (pnmol_filter_set_reaction)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = pnmol_reaction_enqueue(f, in->mean, in->frame_dt, dt, false)) return rc;
    f->sq_dt = -1.0;  // the operator changed: pnmol_filter_prepare_error_model comes next
    return 0;
}

}  // extern "C"
