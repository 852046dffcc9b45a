// pnmol_reaction.hip -- pointwise reaction terms evaluated on the device (`pnmol_filter_set_reaction`,
// `pnmol_filter_linearize`, include/pnmol_hip.h): the kernel, then the host side.
//
// Semilinear EK1 (white.py:189-208) for u_t = L u + r(u) with a pointwise r(u) = P(u) + A(u) / B(u) (polynomials with scalar
// coefficients): the linearisation at the predicted mean u = E0 m^- is M = L + diag(r'(u)) with shift r'(u) u - r(u).
// k_linearize forms u from the step's input mean (the arithmetic of pnmol_filter_predict_mean), evaluates r and r' by
// Horner and patches the diagonal slots of the stencil rows and the shift, as k_operator_diagonal does from a host buffer.
// Nothing crosses the bus, so the constant-step loop re-linearises in front of every step (launch_step's callers in
// pnmol_hip.hip) and stays on the device.
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

}  // namespace

int pnmol_reaction_enqueue(pnmol_filter* f, const double* mean, double frame_dt, double dt) {
    LinearizeArgs a;
    a.r = f->reaction;
    for (int q = 0; q < MAXN; ++q) a.c[q] = 0.0;
    for (int q = 0; q < f->n; ++q) {
        const double so = frame_dt == 0.0 ? 1.0 : nordsieck_scale(f->nu, q, frame_dt);
        a.c[q] = f->iwp.A1[q] * (so / nordsieck_scale(f->nu, q, dt));
    }
    a.s0 = nordsieck_scale(f->nu, 0, dt);
    k_linearize<<<(unsigned)((f->mp + 255) / 256), 256, 0, f->ctx->stream>>>(a, f->n, mean, f->ell_val, f->ell_val_base,
                                                                             f->ell_diag_slot, f->shift, f->d, f->dp, f->mp);
    HIPCHK(f->ctx, hipGetLastError());
    return 0;
}

extern "C" {

int pnmol_filter_set_reaction(pnmol_filter* f, const pnmol_reaction* r) {
    static const char* who = "pnmol_filter_set_reaction: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    if (r) {
        const char* why = nullptr;
        const int degs[3] = {r->deg_p, r->deg_a, r->deg_b};
        for (int g : degs)
            if (g < -1 || g > PNMOL_REACTION_MAXDEG) why = "a degree outside [-1, 7]";
        if (!why && (r->deg_a < 0) != (r->deg_b < 0)) why = "the numerator a and the denominator b are given together or not at all";
        if (!why && !(all_finite(r->p, r->deg_p) && all_finite(r->a, r->deg_a) && all_finite(r->b, r->deg_b)))
            why = "a coefficient is not finite";
        if (!why && r->deg_b >= 0) {
            bool zero = true;
            for (int k = 0; k <= r->deg_b; ++k) zero = zero && r->b[k] == 0.0;
            if (zero) why = "the denominator b is identically zero";
        }
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
    if (r) {
        std::memset(&f->reaction, 0, sizeof(f->reaction));
        f->reaction.deg_p = r->deg_p, f->reaction.deg_a = r->deg_a, f->reaction.deg_b = r->deg_b;
        for (int k = 0; k <= r->deg_p; ++k) f->reaction.p[k] = r->p[k];
        for (int k = 0; k <= r->deg_a; ++k) f->reaction.a[k] = r->a[k];
        for (int k = 0; k <= r->deg_b; ++k) f->reaction.b[k] = r->b[k];
    }
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
