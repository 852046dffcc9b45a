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
// of L by those columns once (build_system_image), and k_linearize_system patches the C same-point slots of every row.
//
// Convection terms (`pnmol_filter_set_convection`; viscous Burgers, Burgers-Fisher): f(u)_i = c(u_i) (G u)_i + r(u_i) with a
// stencil operator G.  The Jacobian diag(c) G + diag(c' G u + r') touches every entry of a stencil row, so the setter builds the
// union image of L and G with G's value beside every slot (build_convection_image) and k_linearize_convection rewrites all slots
// of a row; the shift (c' g + r') u - r needs no product with G (the c g terms of J u - f cancel).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "pnmol_internal.hpp"

namespace {

struct LinearizeArgs {
    pnmol_reaction r;
    double c[MAXN];  // A1[0][a] * ts[a]: row 0 of the transition times the frame change of the input mean
    double s0;       // raw-coordinate scale of derivative 0 in the frame of dt
};

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

// One thread per measurement row.  Every operation is rounded on its own (no contraction into fused multiply-adds): the
// results are those of the same formulas in NumPy (pnmol/pde/reactions.py), bit for bit.
__global__ __launch_bounds__(256) void k_linearize(LinearizeArgs a, int n, const double* __restrict__ mean,
                                                   double* __restrict__ ell_val, const double* __restrict__ base_val,
                                                   const int* __restrict__ slot, double* __restrict__ shift, int d, int dp,
                                                   int mp) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp) return;
    if (i >= d) {
        shift[i] = 0.0;
        return;
    }
    double acc = 0.0;
    for (int q = 0; q < n; ++q) acc = acc + a.c[q] * mean[(long)q * dp + i];
    const double u = a.s0 * acc;
    double P, dP, A, dA, B, dB;
    horner(a.r.p, a.r.deg_p, u, P, dP);
    double r = P, dr = dP;
    if (a.r.deg_a >= 0) {
        horner(a.r.a, a.r.deg_a, u, A, dA);
        horner(a.r.b, a.r.deg_b, u, B, dB);
        r = P + A / B;
        dr = dP + (dA * B - A * dB) / (B * B);
    }
    const long e = (long)slot[i] * mp + i;
    ell_val[e] = base_val[e] - dr;
    shift[i] = dr * u - r;
}

// ---- coupled systems: r_c(u) = P_c(u) + A_c(u) / B_c(u) of the C species at one mesh point (pnmol_filter_set_reaction_system)
struct LinearizeSystemArgs {
    pnmol_reaction_system r;
    double c[MAXN];  // as in LinearizeArgs
    double s0;
};

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
__global__ __launch_bounds__(256) void k_linearize_system(LinearizeSystemArgs a, int n, int N, const double* __restrict__ mean,
                                                          double* __restrict__ ell_val, const double* __restrict__ base_val,
                                                          const int* __restrict__ slot, double* __restrict__ shift, int d,
                                                          int dp, int mp) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp) return;
    if (i >= d) {
        shift[i] = 0.0;
        return;
    }
    const int C = a.r.ncomp;
    const int c = i / N, j = i - c * N;
    double u[SC];
#pragma unroll
    for (int k = 0; k < SC; ++k) {
        u[k] = 0.0;
        if (k < C) {
            double acc = 0.0;
            for (int q = 0; q < n; ++q) acc = acc + a.c[q] * mean[(long)q * dp + (long)k * N + j];
            u[k] = a.s0 * acc;
        }
    }
    double r = 0.0, J[SC];
#pragma unroll
    for (int k = 0; k < SC; ++k) J[k] = 0.0;
    // the component is uniform across a wave except where a wave straddles two species blocks: the descriptor is indexed by the
    // loop counter, never by the thread's own c
#pragma unroll
    for (int cc = 0; cc < SC; ++cc) {
        if (cc == c) {
            double P, dP[SC];
            poly_eval(a.r.p[cc], u, P, dP);
            r = P;
#pragma unroll
            for (int k = 0; k < SC; ++k) J[k] = dP[k];
            if (a.r.a[cc].nterms > 0) {
                double A, dA[SC], B, dB[SC];
                poly_eval(a.r.a[cc], u, A, dA);
                poly_eval(a.r.b[cc], u, B, dB);
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
struct LinearizeConvectionArgs {
    pnmol_convection t;
    double c[MAXN];  // as in LinearizeArgs
    double s0;
};

// derivative 0 of the predicted mean at mesh point j, in raw coordinates: k_linearize's arithmetic
__device__ __forceinline__ double predicted_value(const double (&c)[MAXN], double s0, int n, const double* __restrict__ mean,
                                                  int dp, int j) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int q = 0; q < n; ++q) acc = acc + c[q] * mean[(long)q * dp + j];
    return s0 * acc;
}

// One thread per measurement row i: u_i and the u of the row's slot columns (recomputed per slot: one launch, no grid-wide
// dependency), g_i = (G u)_i over the entries of G that are not zero in slot (= ascending column) order starting from the first
// product, c, c', r, r' by Horner, q = c' g + r'; every slot becomes base - c G, the diagonal one loses q as well, and the shift
// is q u - r.  Every operation is rounded on its own, in the order of Convection.linearization (pnmol/pde/reactions.py).
// img_col / img_val / img_g: the union image of the creation-time operator and G (w slots, packed to the front of every row).
__global__ __launch_bounds__(256) void k_linearize_convection(LinearizeConvectionArgs a, int n, int w,
                                                              const double* __restrict__ mean, double* __restrict__ ell_val,
                                                              const int* __restrict__ img_col, const double* __restrict__ img_val,
                                                              const double* __restrict__ img_g, const int* __restrict__ slot,
                                                              double* __restrict__ shift, int d, int dp, int mp) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp) return;
    if (i >= d) {
        shift[i] = 0.0;
        return;
    }
    const double u = predicted_value(a.c, a.s0, n, mean, dp, i);
    double g = 0.0;
    bool first = true;
    for (int e = 0; e < w; ++e) {
        const int col = img_col[(long)e * mp + i];
        if (col < 0) break;
        const double gv = img_g[(long)e * mp + i];
        if (gv == 0.0) continue;
        const double prod = gv * predicted_value(a.c, a.s0, n, mean, dp, col);
        g = first ? prod : g + prod;
        first = false;
    }
    double cu, dcu, P, dP, A, dA, B, dB;
    horner(a.t.c, a.t.deg_c, u, cu, dcu);
    horner(a.t.r.p, a.t.r.deg_p, u, P, dP);
    double r = P, dr = dP;
    if (a.t.r.deg_a >= 0) {
        horner(a.t.r.a, a.t.r.deg_a, u, A, dA);
        horner(a.t.r.b, a.t.r.deg_b, u, B, dB);
        r = P + A / B;
        dr = dP + (dA * B - A * dB) / (B * B);
    }
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

// the stencil rows of the operator given at creation and a zero shift (what pnmol_filter_set_operator_diagonal restores
// after a dense upload), on the ctx stream
int restore_base_operator(pnmol_filter* f) {
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    const int mp = f->mp;
    if (!f->ell_is_base || f->ellw != f->base_w)
        HIPCHK(ctx, hipMemcpyAsync(f->ell_col, f->ell_col_base, sizeof(int) * (size_t)f->base_w * mp, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(f->ell_val, f->ell_val_base, sizeof(double) * (size_t)f->base_w * mp, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(f->shift, 0, sizeof(double) * mp, st));
    f->ellw = f->base_w;
    f->ell_is_base = 1;
    return 0;
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

void free_system_image(pnmol_filter* f) {
    for (void* q : {(void*)f->sys_col, (void*)f->sys_val, (void*)f->sys_slot})
        if (q) (void)hipFree(q);
    f->sys_col = nullptr, f->sys_val = nullptr, f->sys_slot = nullptr;
    f->sys_w = 0, f->sys_img_ncomp = 0;
}

// The widened image of the operator given at creation for C species: every PDE row i = c N + j has a slot for each column
// k N + j (the value of L there, or 0), slots in ascending column order as build_ell leaves them; boundary rows as they are.
// Built on the host from the base image (read back once per C) and kept on the device beside the (C, mp) slot table.
int build_system_image(pnmol_filter* f, int C) {
    pnmol_ctx* ctx = f->ctx;
    const int d = f->d, mp = f->mp, bw = f->base_w, N = d / C;
    std::vector<int> bcol((size_t)bw * mp);
    std::vector<double> bval((size_t)bw * mp);
    HIPCHK(ctx, hipMemcpy(bcol.data(), f->ell_col_base, sizeof(int) * bcol.size(), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(bval.data(), f->ell_val_base, sizeof(double) * bval.size(), hipMemcpyDeviceToHost));
    std::vector<std::vector<std::pair<int, double>>> rows((size_t)mp);
    int w = 1;
    for (int i = 0; i < mp; ++i) {
        auto& row = rows[i];
        for (int e = 0; e < bw; ++e)
            if (bcol[(size_t)e * mp + i] >= 0) row.emplace_back(bcol[(size_t)e * mp + i], bval[(size_t)e * mp + i]);
        if (i < d) {
            const int j = i % N;
            for (int k = 0; k < C; ++k) {
                const int col = k * N + j;
                bool have = false;
                for (const auto& cv : row) have = have || cv.first == col;
                if (!have) row.emplace_back(col, 0.0);
            }
            std::stable_sort(row.begin(), row.end(), [](const std::pair<int, double>& x, const std::pair<int, double>& y) {
                return x.first < y.first;
            });
        }
        w = std::max(w, (int)row.size());
    }
    std::vector<int> ecol((size_t)w * mp, -1), slot((size_t)C * mp, 0);
    std::vector<double> eval((size_t)w * mp, 0.0);
    for (int i = 0; i < mp; ++i)
        for (int e = 0; e < (int)rows[i].size(); ++e) {
            ecol[(size_t)e * mp + i] = rows[i][e].first;
            eval[(size_t)e * mp + i] = rows[i][e].second;
            if (i < d && rows[i][e].first % N == i % N) slot[(size_t)(rows[i][e].first / N) * mp + i] = e;
        }
    free_system_image(f);
    HIPCHK(ctx, hipMalloc(&f->sys_col, sizeof(int) * ecol.size()));
    HIPCHK(ctx, hipMalloc(&f->sys_val, sizeof(double) * eval.size()));
    HIPCHK(ctx, hipMalloc(&f->sys_slot, sizeof(int) * slot.size()));
    HIPCHK(ctx, hipMemcpy(f->sys_col, ecol.data(), sizeof(int) * ecol.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(f->sys_val, eval.data(), sizeof(double) * eval.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(f->sys_slot, slot.data(), sizeof(int) * slot.size(), hipMemcpyHostToDevice));
    f->sys_w = w;
    f->sys_img_ncomp = C;
    return 0;
}

void free_convection_image(pnmol_filter* f) {
    for (void* q : {(void*)f->cv_col, (void*)f->cv_val, (void*)f->cv_g, (void*)f->cv_slot})
        if (q) (void)hipFree(q);
    f->cv_col = nullptr, f->cv_val = nullptr, f->cv_g = nullptr, f->cv_slot = nullptr;
    f->cv_w = 0;
}

// The union image of the operator given at creation and G (d x d, row major): every PDE row has a slot for each column in which
// either has an entry (the value of -L there, or 0), slots in ascending column order as build_ell leaves them, and G's value
// beside each slot; boundary rows as they are.  Built on the host from the base image and kept on the device beside the table
// of the diagonal slots.  The caller has synchronised the stream: the buffers replaced here may have been read.
int build_convection_image(pnmol_filter* f, const double* G) {
    pnmol_ctx* ctx = f->ctx;
    const int d = f->d, mp = f->mp, bw = f->base_w;
    std::vector<int> bcol((size_t)bw * mp);
    std::vector<double> bval((size_t)bw * mp);
    HIPCHK(ctx, hipMemcpy(bcol.data(), f->ell_col_base, sizeof(int) * bcol.size(), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(bval.data(), f->ell_val_base, sizeof(double) * bval.size(), hipMemcpyDeviceToHost));
    std::vector<std::vector<std::pair<int, double>>> rows((size_t)mp);
    int w = 1;
    for (int i = 0; i < mp; ++i) {
        auto& row = rows[i];
        for (int e = 0; e < bw; ++e)
            if (bcol[(size_t)e * mp + i] >= 0) row.emplace_back(bcol[(size_t)e * mp + i], bval[(size_t)e * mp + i]);
        if (i < d) {
            for (int k = 0; k < d; ++k) {
                if (G[(size_t)i * d + k] == 0.0) continue;
                bool have = false;
                for (const auto& cv : row) have = have || cv.first == k;
                if (!have) row.emplace_back(k, 0.0);
            }
            std::stable_sort(row.begin(), row.end(), [](const std::pair<int, double>& x, const std::pair<int, double>& y) {
                return x.first < y.first;
            });
        }
        w = std::max(w, (int)row.size());
    }
    std::vector<int> ecol((size_t)w * mp, -1), slot((size_t)mp, 0);
    std::vector<double> eval((size_t)w * mp, 0.0), eg((size_t)w * mp, 0.0);
    for (int i = 0; i < mp; ++i)
        for (int e = 0; e < (int)rows[i].size(); ++e) {
            const int col = rows[i][e].first;
            ecol[(size_t)e * mp + i] = col;
            eval[(size_t)e * mp + i] = rows[i][e].second;
            if (i < d && col < d) eg[(size_t)e * mp + i] = G[(size_t)i * d + col];
            if (i < d && col == i) slot[i] = e;
        }
    free_convection_image(f);
    HIPCHK(ctx, hipMalloc(&f->cv_col, sizeof(int) * ecol.size()));
    HIPCHK(ctx, hipMalloc(&f->cv_val, sizeof(double) * eval.size()));
    HIPCHK(ctx, hipMalloc(&f->cv_g, sizeof(double) * eg.size()));
    HIPCHK(ctx, hipMalloc(&f->cv_slot, sizeof(int) * slot.size()));
    HIPCHK(ctx, hipMemcpy(f->cv_col, ecol.data(), sizeof(int) * ecol.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(f->cv_val, eval.data(), sizeof(double) * eval.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(f->cv_g, eg.data(), sizeof(double) * eg.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(f->cv_slot, slot.data(), sizeof(int) * slot.size(), hipMemcpyHostToDevice));
    f->cv_w = w;
    return 0;
}

}  // namespace

void pnmol_reaction_free_ws(pnmol_filter* f) {
    free_system_image(f);
    free_convection_image(f);
}

int pnmol_reaction_enqueue(pnmol_filter* f, const double* mean, double frame_dt, double dt) {
    double c[MAXN];
    for (int q = 0; q < MAXN; ++q) c[q] = 0.0;
    for (int q = 0; q < f->n; ++q) {
        const double so = frame_dt == 0.0 ? 1.0 : nordsieck_scale(f->nu, q, frame_dt);
        c[q] = f->iwp.A1[q] * (so / nordsieck_scale(f->nu, q, dt));
    }
    const unsigned blocks = (unsigned)((f->mp + 255) / 256);
    if (f->cv_set) {
        LinearizeConvectionArgs a;
        a.t = f->cv;
        std::memcpy(a.c, c, sizeof(c));
        a.s0 = nordsieck_scale(f->nu, 0, dt);
        k_linearize_convection<<<blocks, 256, 0, f->ctx->stream>>>(a, f->n, f->cv_w, mean, f->ell_val, f->cv_col, f->cv_val,
                                                                   f->cv_g, f->cv_slot, f->shift, f->d, f->dp, f->mp);
    } else if (f->sys_set) {
        LinearizeSystemArgs a;
        a.r = f->sys;
        std::memcpy(a.c, c, sizeof(c));
        a.s0 = nordsieck_scale(f->nu, 0, dt);
        k_linearize_system<<<blocks, 256, 0, f->ctx->stream>>>(a, f->n, f->d / f->sys.ncomp, mean, f->ell_val, f->sys_val,
                                                               f->sys_slot, f->shift, f->d, f->dp, f->mp);
    } else {
        LinearizeArgs a;
        a.r = f->reaction;
        std::memcpy(a.c, c, sizeof(c));
        a.s0 = nordsieck_scale(f->nu, 0, dt);
        k_linearize<<<blocks, 256, 0, f->ctx->stream>>>(a, f->n, mean, f->ell_val, f->ell_val_base, f->ell_diag_slot, f->shift,
                                                        f->d, f->dp, f->mp);
    }
    HIPCHK(f->ctx, hipGetLastError());
    return 0;
}

extern "C" {

int pnmol_filter_set_reaction(pnmol_filter* f, const pnmol_reaction* r) {
    static const char* who = "pnmol_filter_set_reaction: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    if (r) {
        const char* why = reaction_descriptor_fault(r);
        if (!why && f->ds != f->d) why = "a latent-force filter (d_state != d) has no pointwise reaction path";
        if (!why && f->p32) why = "an fp32 filter has no pointwise reaction path";
        if (!why && !f->base_has_diag) why = "a row of the operator given at creation has no diagonal entry";
        if (why) {
            ctx->err = std::string(who) + why;
            return -1;
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!r && !f->has_reaction) return 0;
    // the coefficients travel by value in the captured k_linearize launches, and the loop's launch sequence differs with and
    // without a reaction
    pnmol_drop_graphs(f);
    if (int rc = restore_base_operator(f)) return rc;
    f->sq_dt = -1.0;  // the error model belongs to the operator that was set
    f->has_reaction = r != nullptr;
    f->sys_set = false;  // (a filter holds one term of any kind)
    f->cv_set = false;
    if (r) {
        std::memset(&f->reaction, 0, sizeof(f->reaction));
        f->reaction.deg_p = r->deg_p, f->reaction.deg_a = r->deg_a, f->reaction.deg_b = r->deg_b;
        for (int k = 0; k <= r->deg_p; ++k) f->reaction.p[k] = r->p[k];
        for (int k = 0; k <= r->deg_a; ++k) f->reaction.a[k] = r->a[k];
        for (int k = 0; k <= r->deg_b; ++k) f->reaction.b[k] = r->b[k];
    }
    return 0;
}

int pnmol_filter_set_reaction_system(pnmol_filter* f, const pnmol_reaction_system* r) {
    static const char* who = "pnmol_filter_set_reaction_system: ";
    if (!f) return -1;
    if (!r) return pnmol_filter_set_reaction(f, nullptr);  // NULL to either setter clears either kind
    pnmol_ctx* ctx = f->ctx;
    const char* why = system_descriptor_fault(r);
    if (!why && f->d % r->ncomp != 0) why = "d is not a multiple of ncomp";
    if (!why && f->ds != f->d) why = "a latent-force filter (d_state != d) has no pointwise reaction path";
    if (!why && f->p32) why = "an fp32 filter has no pointwise reaction path";
    if (!why && !f->base_has_diag) why = "a row of the operator given at creation has no diagonal entry";
    if (why) {
        ctx->err = std::string(who) + why;
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int mp = f->mp;
    pnmol_drop_graphs(f);  // the descriptor travels by value in the captured launches; width and pointers are baked in too
    if (f->sys_img_ncomp != r->ncomp || f->sys_w > f->ell_cap) {
        HIPCHK(ctx, hipStreamSynchronize(st));  // the buffers replaced below may still be read
        if (f->sys_img_ncomp != r->ncomp)
            if (int rc = build_system_image(f, r->ncomp)) {
                free_system_image(f);
                return rc;
            }
        if (f->sys_w > f->ell_cap) {
            if (f->ell_col) (void)hipFree(f->ell_col);
            if (f->ell_val) (void)hipFree(f->ell_val);
            f->ell_col = nullptr, f->ell_val = nullptr, f->ell_cap = 0, f->ellw = 0, f->ell_is_base = 0;
            HIPCHK(ctx, hipMalloc(&f->ell_col, sizeof(int) * (size_t)f->sys_w * mp));
            HIPCHK(ctx, hipMalloc(&f->ell_val, sizeof(double) * (size_t)f->sys_w * mp));
            f->ell_cap = f->sys_w;
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(f->ell_col, f->sys_col, sizeof(int) * (size_t)f->sys_w * mp, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(f->ell_val, f->sys_val, sizeof(double) * (size_t)f->sys_w * mp, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(f->shift, 0, sizeof(double) * mp, st));
    f->ellw = f->sys_w;
    f->ell_is_base = 0;  // (restore_base_operator copies the columns back)
    f->sq_dt = -1.0;     // the error model belongs to the operator that was set
    f->has_reaction = true;
    f->sys_set = true;
    f->cv_set = false;
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
    return 0;
}

int pnmol_filter_set_convection(pnmol_filter* f, const pnmol_convection* term, const double* G_dd) {
    static const char* who = "pnmol_filter_set_convection: ";
    if (!f) return -1;
    if (!term) return pnmol_filter_set_reaction(f, nullptr);  // NULL to any setter clears any kind
    pnmol_ctx* ctx = f->ctx;
    const char* why = nullptr;
    if (!G_dd) why = "a convection term needs its operator G";
    if (!why && (term->deg_c < -1 || term->deg_c > PNMOL_REACTION_MAXDEG)) why = "a degree outside [-1, 7]";
    if (!why) why = reaction_descriptor_fault(&term->r);
    if (!why && !all_finite(term->c, term->deg_c)) why = "a coefficient is not finite";
    if (!why && f->ds != f->d) why = "a latent-force filter (d_state != d) has no convection path";
    if (!why && f->p32) why = "an fp32 filter has no convection path";
    if (!why && !f->base_has_diag) why = "a row of the operator given at creation has no diagonal entry";
    if (!why)
        for (size_t k = 0; k < (size_t)f->d * f->d && !why; ++k)
            if (!std::isfinite(G_dd[k])) why = "an entry of G is not finite";
    if (why) {
        ctx->err = std::string(who) + why;
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int mp = f->mp;
    pnmol_drop_graphs(f);  // the descriptor travels by value in the captured launches; width and pointers are baked in too
    HIPCHK(ctx, hipStreamSynchronize(st));  // the image replaced below may still be read
    f->cv_set = false;
    if (int rc = build_convection_image(f, G_dd)) {
        // no image: leave the filter without a term, on the operator given at creation
        free_convection_image(f);
        f->has_reaction = false, f->sys_set = false;
        (void)restore_base_operator(f);
        f->sq_dt = -1.0;
        return rc;
    }
    if (f->cv_w > f->ell_cap) {
        if (f->ell_col) (void)hipFree(f->ell_col);
        if (f->ell_val) (void)hipFree(f->ell_val);
        f->ell_col = nullptr, f->ell_val = nullptr, f->ell_cap = 0, f->ellw = 0, f->ell_is_base = 0;
        HIPCHK(ctx, hipMalloc(&f->ell_col, sizeof(int) * (size_t)f->cv_w * mp));
        HIPCHK(ctx, hipMalloc(&f->ell_val, sizeof(double) * (size_t)f->cv_w * mp));
        f->ell_cap = f->cv_w;
    }
    HIPCHK(ctx, hipMemcpyAsync(f->ell_col, f->cv_col, sizeof(int) * (size_t)f->cv_w * mp, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(f->ell_val, f->cv_val, sizeof(double) * (size_t)f->cv_w * mp, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(f->shift, 0, sizeof(double) * mp, st));
    f->ellw = f->cv_w;
    f->ell_is_base = 0;  // (restore_base_operator copies the columns back)
    f->sq_dt = -1.0;     // the error model belongs to the operator that was set
    f->has_reaction = true;
    f->sys_set = false;
    f->cv_set = true;
    std::memset(&f->cv, 0, sizeof(f->cv));
    f->cv.deg_c = term->deg_c;
    for (int k = 0; k <= term->deg_c; ++k) f->cv.c[k] = term->c[k];
    f->cv.r.deg_p = term->r.deg_p, f->cv.r.deg_a = term->r.deg_a, f->cv.r.deg_b = term->r.deg_b;
    for (int k = 0; k <= term->r.deg_p; ++k) f->cv.r.p[k] = term->r.p[k];
    for (int k = 0; k <= term->r.deg_a; ++k) f->cv.r.a[k] = term->r.a[k];
    for (int k = 0; k <= term->r.deg_b; ++k) f->cv.r.b[k] = term->r.b[k];
    return 0;
}

int pnmol_filter_linearize(pnmol_filter* f, const pnmol_state* in, double dt) {
    static const char* who = "pnmol_filter_linearize: ";
    if (!f || !in || in->f != f || !(dt > 0.0)) {
        if (f) f->ctx->err = std::string(who) + "bad argument (null, foreign state or dt <= 0)";
        return -1;
    }
    pnmol_ctx* ctx = f->ctx;
    if (!f->has_reaction) {
        ctx->err = std::string(who) + "no reaction set (pnmol_filter_set_reaction)";
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = pnmol_reaction_enqueue(f, in->mean, in->frame_dt, dt)) return rc;
    f->sq_dt = -1.0;  // the operator changed: pnmol_filter_prepare_error_model comes next
    return 0;
}

}  // extern "C"
