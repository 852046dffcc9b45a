// pnmol_functional.hip -- the posterior of linear functionals of the whole trajectory (`pnmol_functionals`,
// include/pnmol_hip.h): kernels, then host side.
//
// The smoothing posterior is the backward Markov chain x_T ~ N(m_T, P_T), x_k | x_{k+1} ~ N(m_k + G_k (x_{k+1} - A m_k),
// P_k - G_k P-_{k+1} G_k^T) with G_k = P_k A^T (P-_{k+1})^-1.  For q = sum_k W_k x_k (W_k: Q x D) the adjoint of that recursion
// runs in ASCENDING k on the filtered states alone.  In the Nordsieck frame of the step h_k, with Lam_0 = W_0^T:
//     U = P Lam,   Y = L^-1 A U  (L L^T = P-),   Mu = L^-T Y  (= G^T Lam)
//     mean += Lam^T m - Mu^T (A m),   cov += Lam^T U - Y^T Y,   Lam_{k+1} = W_{k+1}^T + Mu
// and at the end mean += Lam_T^T m_T, cov += Lam_T^T P_T Lam_T.  No smoothed state, no D x D gain, no D x D x D product.
// The factorisation is the forward step's own sweep (pnmol_hip.hip) of the tall matrix [P-; (A U)^T]: the FQ rows (A U)^T ride
// under P- and come out as Y^T = (A U)^T L^-T; the identity rows of the smoother's sweep are not there.  This file holds what
// surrounds it: the block transform with the frame change (k_fn_build; its predict is predict_block of pnmol_tile.hpp), the
// weights and the frame change of the dual vector (k_fn_lam), the thin products and Gram terms on tile_product (k_fn_thin,
// k_fn_gram), the blocked back-substitution Mu^T = Y^T L^-1 (k_fn_backsub) and the accumulation (k_fn_accum, k_fn_out).
// Layouts are the forward step's: derivative-major (a, j) -> a*dp + j, Dp = n*dp, row-major, zero padding, unit pivots on the
// padded points.  Every thin matrix is kept TRANSPOSED, FQ = 64 rows (functionals, zero rows behind Q) of Dp: that is the
// layout of the sweep's extra rows, and the row operand of tile_product.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pnmol_internal.hpp"
#include "pnmol_tile.hpp"

constexpr int FQ = PNMOL_FUNCTIONALS_MAX_Q;  // rows of every thin matrix
static_assert(FQ == BM && FQ % NB == 0, "a thin matrix is one tile of tile_product high and whole row blocks of the sweep");

// The buffers of a pass, kept by the filter from the first call on
struct FunctionalWs {
    SweepWs sweep;            // [P- (cb row blocks); (A U)^T (FQ / 32)] -> [L; Y^T]
    double* Ph = nullptr;     // P^h (Dp x Dp)
    double* thin = nullptr;   // Lam^T | U^T | Mu^T (FQ x Dp each), m^h | A m^h (Dp each), cov (FQ x FQ), mean (FQ)
    double* part = nullptr;   // partial Gram tiles: 2 x nsplit x FQ x FQ
    int nsplit = 0;
    double* w = nullptr;      // the weights of the call (grown on demand)
    size_t w_cap = 0;
    double* out = nullptr;    // mean (FQ) | cov (FQ x FQ) | info words of out_steps steps, and its pinned host image
    double* out_pin = nullptr;
    int out_steps = -1;
};

namespace {

constexpr long GRAM_CHUNK = 256;  // K range of one partial Gram tile

struct FnConsts {
    double A1[SM_MAXN * SM_MAXN];  // IwpConsts.A1
    double Q1[SM_MAXN * SM_MAXN];  // IwpConsts.Q1
    double ts[SM_MAXN];            // frame change of the filtered state into the frame of h
    double sc[SM_MAXN];            // raw weights into the frame of h (a dual vector takes the scale of the frame itself)
    double cm[SM_MAXN];            // Mu of the step before into the frame of h: s_h / s_before (the transposed inverse of x's change)
};

// P (frame of the filtered state) -> frame of h:  Ph = P^h,  Gs rows [0, Dp) = P- = A1 P^h A1^T + Q1 K  (+1 on the diagonal of
// the padded points: the sweep needs a pivot).  k_sm_build of pnmol_smooth.hip without the successor and without P A^T.
template <int N>
__global__ __launch_bounds__(256) void k_fn_build(const double* __restrict__ P, const double* __restrict__ Kg, FnConsts c, int d,
                                                  int dp, double* __restrict__ Gs, double* __restrict__ Ph) {
    const int k = blockIdx.x * 32 + threadIdx.x;
    const int j = blockIdx.y * 8 + threadIdx.y;
    const long Dp = (long)N * dp;
    double X[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const long idx = ((long)a * dp + j) * Dp + (long)b * dp + k;
            X[a][b] = c.ts[a] * c.ts[b] * P[idx];
            Ph[idx] = X[a][b];
        }
    double XA[N][N], Pm[N][N];
    predict_block<N>(X, c.A1, c.Q1, Kg[(long)j * dp + k], XA, Pm);
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b)
            Gs[((long)a * dp + j) * Dp + (long)b * dp + k] = (a == b && j == k && j >= d) ? 1.0 : Pm[a][b];
}

// mh = ts m (frame of h), Amh = A1 mh  (one workgroup)
template <int N>
__global__ __launch_bounds__(256) void k_fn_vec(const double* __restrict__ m, FnConsts c, int dp, double* __restrict__ mh,
                                                double* __restrict__ Amh) {
    for (int j = threadIdx.x; j < dp; j += 256) {
        double x[N];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            x[a] = c.ts[a] * m[a * dp + j];
            mh[a * dp + j] = x[a];
        }
#pragma unroll
        for (int a = 0; a < N; ++a) {
            double s = 0.0;
#pragma unroll
            for (int e = 0; e < N; ++e) s += c.A1[a * SM_MAXN + e] * x[e];
            Amh[a * dp + j] = s;
        }
    }
}

// Lam^T = sc W_k [+ cm Mu^T]: row q, column a dp + j.  W: (Q, T1, n, d) row-major, raw coordinates; rows q >= Q and the padded
// points are zero.
__global__ __launch_bounds__(256) void k_fn_lam(const double* __restrict__ W, int Q, long T1, long k, int n, int d, int dp,
                                                FnConsts c, const double* __restrict__ Mut, double* __restrict__ Lamt) {
    const long Dp = (long)n * dp;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= FQ * Dp) return;
    const int q = (int)(e / Dp), i = (int)(e % Dp), a = i / dp, j = i % dp;
    double v = 0.0;
    if (q < Q && j < d) {
        v = c.sc[a] * W[(((long)q * T1 + k) * n + a) * d + j];
        if (Mut) v += c.cm[a] * Mut[e];
    }
    Lamt[e] = v;
}

// Out^T = Lam^T B  (FQ x Dp; B = P^h or a state's P, Dp x Dp): one 64-column tile per workgroup, K = Dp
__global__ __launch_bounds__(256) void k_fn_thin(const double* __restrict__ Lamt, const double* __restrict__ B,
                                                 double* __restrict__ Out, long Dp) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    const int tid = threadIdx.x;
    const long c0 = (long)blockIdx.x * BM;
    d4 acc[2][2];
    tile_zero(acc);
    tile_product<false>(Lamt, Dp, FQ, B, Dp, Dp, Dp, 0, 1.0, 0, c0, acc, sA, sB, tid);
    tile_each(acc, 0, c0, tid, [&](long row, long col, double v) {
        if (col < Dp) Out[row * Dp + col] = v;
    });
}

// (A U)^T: row q, column a dp + j = sum_b A1[a][b] U^T[q][b dp + j], into the sweep's extra rows
template <int N>
__global__ __launch_bounds__(256) void k_fn_au(const double* __restrict__ Ut, FnConsts c, int dp, double* __restrict__ rows) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)FQ * dp) return;
    const long Dp = (long)N * dp;
    const long q = e / dp, j = e % dp;
    double u[N];
#pragma unroll
    for (int b = 0; b < N; ++b) u[b] = Ut[q * Dp + (long)b * dp + j];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < N; ++b) s += c.A1[a * SM_MAXN + b] * u[b];
        rows[q * Dp + (long)a * dp + j] = s;
    }
}

// One stage of the back-substitution Mu^T = Y^T L^-1 (in place in M, FQ x Dp, which holds Y^T on entry of the first stage), in
// panels of 64 columns from the last one upwards.  Stage s (launched with s + 1 workgroups, the stages in stream order):
//   workgroup b <= s:  M[:, panel b] -= M[:, panel s+1] L[panel s+1, panel b]      (the panel solved by the stage before)
//   workgroup s, then: the panel's own 32-column tiles J1 = 2s + 1, J0 = 2s:
//                      M_J1 = M_J1 Linv_J1,   M_J0 = (M_J0 - M_J1 L[J1, J0]) Linv_J0
// with the L_jj^-1 tiles the sweep stores (Linv, lower triangular) and the off-diagonal tiles of L.  Every product is
// tile_product's (fp64 MFMA); a stage reads only what earlier stages or its own workgroup wrote.
__global__ __launch_bounds__(256) void k_fn_backsub(double* M, const double* __restrict__ L, const double* __restrict__ Linv,
                                                    long Dp, int s, int npanels) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    const int tid = threadIdx.x, b = blockIdx.x;
    const long c0 = (long)b * BM;
    d4 acc[2][2];
    if (s + 1 < npanels) {
        const long k0 = (long)(s + 1) * BM, k1 = k0 + BM < Dp ? k0 + BM : Dp;
        tile_zero(acc);
        tile_product<false>(M, Dp, FQ, L, Dp, Dp, k1, k0, -1.0, 0, c0, acc, sA, sB, tid);
        tile_each(acc, 0, c0, tid, [&](long row, long col, double v) { M[row * Dp + col] += v; });  // (c0 + 63 < k0 <= Dp)
    }
    if (b != s) return;
    const bool two = c0 + NB < Dp;  // the panel has a second tile (Dp is a multiple of 32, not always of 64)
    if (two) {
        __syncthreads();  // the panel as updated above
        tile_zero(acc);
        tile_product<false>(M + c0 + NB, Dp, FQ, Linv + (long)(2 * s + 1) * NB * NB, NB, NB, NB, 0, 1.0, 0, 0, acc, sA, sB, tid);
        __syncthreads();  // everybody has read M_J1
        tile_each(acc, 0, 0, tid, [&](long row, long col, double v) {
            if (col < NB) M[row * Dp + c0 + NB + col] = v;
        });
        __syncthreads();
        tile_zero(acc);
        tile_product<false>(M + c0 + NB, Dp, FQ, L + (c0 + NB) * Dp + c0, Dp, NB, NB, 0, -1.0, 0, 0, acc, sA, sB, tid);
        tile_each(acc, 0, 0, tid, [&](long row, long col, double v) {
            if (col < NB) M[row * Dp + c0 + col] += v;
        });
    }
    __syncthreads();
    tile_zero(acc);
    tile_product<false>(M + c0, Dp, FQ, Linv + (long)(2 * s) * NB * NB, NB, NB, NB, 0, 1.0, 0, 0, acc, sA, sB, tid);
    __syncthreads();  // everybody has read M_J0
    tile_each(acc, 0, 0, tid, [&](long row, long col, double v) {
        if (col < NB) M[row * Dp + c0 + col] = v;
    });
}

// Partial Gram tiles over the K range [x chunk, (x + 1) chunk): y = 0: Lam^T U, y = 1: Y^T Y  (FQ x FQ each, NT products of the
// transposed thin matrices).  part: (2, nsplit, FQ, FQ)
__global__ __launch_bounds__(256) void k_fn_gram(const double* __restrict__ Lamt, const double* __restrict__ Ut,
                                                 const double* __restrict__ Yt, long Dp, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    const int tid = threadIdx.x;
    const long k0 = (long)blockIdx.x * GRAM_CHUNK, k1 = k0 + GRAM_CHUNK < Dp ? k0 + GRAM_CHUNK : Dp;
    const double* A = blockIdx.y ? Yt : Lamt;
    const double* B = blockIdx.y ? Yt : Ut;
    d4 acc[2][2];
    tile_zero(acc);
    tile_product<true>(A, Dp, FQ, B, Dp, FQ, k1, k0, 1.0, 0, 0, acc, sA, sB, tid);
    double* out = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * FQ * FQ;
    tile_each(acc, 0, 0, tid, [&](long row, long col, double v) { out[row * FQ + col] = v; });
}

// cov += (sum of the partial tiles of Lam^T U) - (that of Y^T Y): each summed on its own in the order of the K ranges, subtracted
// once.  mean += Lam^T m^h - Mu^T (A m^h), the two dot products reduced per wave, then over the four waves in a fixed order.
// both = 0 (the terminal term): no Y, no Mu.  One workgroup per functional (row q of cov, entry q of mean); the first one also
// keeps the step's sweep info word, which the next step's sweep resets.
__global__ __launch_bounds__(256) void k_fn_accum(const double* __restrict__ part, int nsplit, int both,
                                                  const double* __restrict__ Lamt, const double* __restrict__ mh,
                                                  const double* __restrict__ Mut, const double* __restrict__ Amh, long Dp,
                                                  double* __restrict__ cov, double* __restrict__ mean,
                                                  const int* __restrict__ sweep_info, int* __restrict__ info_step) {
    __shared__ double red[2][4];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, q = blockIdx.x;
    if (tid < FQ) {
        const int e = q * FQ + tid;
        double g1 = 0.0, g2 = 0.0;
        for (int s = 0; s < nsplit; ++s) g1 += part[(long)s * FQ * FQ + e];
        if (both)
            for (int s = 0; s < nsplit; ++s) g2 += part[(long)(nsplit + s) * FQ * FQ + e];
        cov[e] += g1 - g2;
    }
    double s1 = 0.0, s2 = 0.0;
    for (long i = tid; i < Dp; i += 256) s1 += Lamt[q * Dp + i] * mh[i];
    if (both)
        for (long i = tid; i < Dp; i += 256) s2 += Mut[q * Dp + i] * Amh[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s1 += __shfl_xor(s1, o), s2 += __shfl_xor(s2, o);
    if (l == 0) red[0][w] = s1, red[1][w] = s2;
    __syncthreads();
    if (tid == 0) {
        mean[q] += ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) - ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
        if (q == 0 && sweep_info) *info_step = *sweep_info;
    }
}

// out = [mean (Q) | cov (Q x Q)], the covariance as the mean of the accumulator and its transpose: symmetric to the bit
__global__ __launch_bounds__(256) void k_fn_out(const double* __restrict__ cov, const double* __restrict__ mean, int Q,
                                                double* __restrict__ out) {
    for (int e = threadIdx.x; e < Q * Q; e += 256) {
        const int q = e / Q, r = e % Q;
        out[FQ + e] = 0.5 * (cov[q * FQ + r] + cov[r * FQ + q]);
    }
    if (threadIdx.x < Q) out[threadIdx.x] = mean[threadIdx.x];
}

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -2; }

int launch_build(hipStream_t st, int n, const double* P, const double* m, const double* Kg, const FnConsts& c, int d, int dp,
                 double* Gs, double* Ph, double* mh, double* Amh) {
    const dim3 grid(dp / 32, dp / 8), blk(32, 8);
    switch (n) {
        case 2:
            if (P) k_fn_build<2><<<grid, blk, 0, st>>>(P, Kg, c, d, dp, Gs, Ph);
            k_fn_vec<2><<<1, 256, 0, st>>>(m, c, dp, mh, Amh);
            break;
        case 3:
            if (P) k_fn_build<3><<<grid, blk, 0, st>>>(P, Kg, c, d, dp, Gs, Ph);
            k_fn_vec<3><<<1, 256, 0, st>>>(m, c, dp, mh, Amh);
            break;
        case 4:
            if (P) k_fn_build<4><<<grid, blk, 0, st>>>(P, Kg, c, d, dp, Gs, Ph);
            k_fn_vec<4><<<1, 256, 0, st>>>(m, c, dp, mh, Amh);
            break;
        default: return -1;
    }
    return launched();
}

int launch_au(hipStream_t st, int n, const double* Ut, const FnConsts& c, int dp, double* rows) {
    const unsigned grid = (unsigned)(((long)FQ * dp + 255) / 256);
    switch (n) {
        case 2: k_fn_au<2><<<grid, 256, 0, st>>>(Ut, c, dp, rows); break;
        case 3: k_fn_au<3><<<grid, 256, 0, st>>>(Ut, c, dp, rows); break;
        case 4: k_fn_au<4><<<grid, 256, 0, st>>>(Ut, c, dp, rows); break;
        default: return -1;
    }
    return launched();
}

size_t out_doubles(int steps) { return (size_t)FQ + (size_t)FQ * FQ + ((size_t)steps + 1) / 2 + 1; }

int ensure_ws(pnmol_filter* f, int T, size_t wcount) {
    pnmol_ctx* ctx = f->ctx;
    const auto fail = [&](hipError_t e, const char* what) {
        ctx->err = std::string("pnmol_functionals: ") + what + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? -4 : -2;
    };
    if (!f->fn_ws) {
        FunctionalWs* w = new FunctionalWs();
        const long Dp = f->Dp;
        const int cb = (int)(Dp / NB);
        w->nsplit = (int)((Dp + GRAM_CHUNK - 1) / GRAM_CHUNK);
        const size_t thin = (size_t)3 * FQ * Dp + 2 * (size_t)Dp + (size_t)FQ * FQ + FQ;
        // (rt > cb: sweep_ws_alloc zeroes G and plants the error model's identity in its last cb row blocks, here across rows
        // of P- and the extra rows.  Nothing relies on either: k_fn_build and k_fn_au rewrite every element of G in every step.)
        hipError_t e = sweep_ws_alloc(&w->sweep, ctx, cb + FQ / NB, cb);
        if (e == hipSuccess) e = hipMalloc(&w->Ph, sizeof(double) * (size_t)Dp * Dp);
        if (e == hipSuccess) e = hipMalloc(&w->thin, sizeof(double) * thin);
        if (e == hipSuccess) e = hipMalloc(&w->part, sizeof(double) * (size_t)2 * w->nsplit * FQ * FQ);
        if (e != hipSuccess) {
            f->fn_ws = w;
            pnmol_functional_free_ws(f);
            return fail(e, "workspace");
        }
        f->fn_ws = w;
    }
    FunctionalWs* w = f->fn_ws;
    if (wcount > w->w_cap) {
        if (w->w) (void)hipFree(w->w);
        w->w = nullptr, w->w_cap = 0;
        const hipError_t e = hipMalloc(&w->w, sizeof(double) * wcount);
        if (e != hipSuccess) {
            w->w = nullptr;
            return fail(e, "weights");
        }
        w->w_cap = wcount;
    }
    if (T > w->out_steps) {
        if (w->out) (void)hipFree(w->out);
        if (w->out_pin) (void)hipHostFree(w->out_pin);
        w->out = w->out_pin = nullptr, w->out_steps = -1;
        hipError_t e = hipMalloc(&w->out, sizeof(double) * out_doubles(T));
        if (e == hipSuccess) e = hipHostMalloc(&w->out_pin, sizeof(double) * out_doubles(T), hipHostMallocDefault);
        if (e != hipSuccess) {
            if (w->out) (void)hipFree(w->out);
            w->out = nullptr;
            return fail(e, "read-out buffers");
        }
        w->out_steps = T;
    }
    return 0;
}

inline double frame_scale(const pnmol_filter* f, int a, double frame_dt) {
    return frame_dt == 0.0 ? 1.0 : nordsieck_scale(f->nu, a, frame_dt);
}

}  // namespace

void pnmol_functional_free_ws(pnmol_filter* f) {
    FunctionalWs* w = f->fn_ws;
    if (!w) return;
    sweep_ws_free(&w->sweep);
    for (void* p : {(void*)w->Ph, (void*)w->thin, (void*)w->part, (void*)w->w, (void*)w->out})
        if (p) (void)hipFree(p);
    if (w->out_pin) (void)hipHostFree(w->out_pin);
    delete w;
    f->fn_ws = nullptr;
}

int pnmol_functionals(pnmol_filter* f, int T, pnmol_state* const* filt, const double* dt_T, int Q, const double* w_QT1nd,
                      double* mean_Q, double* cov_QQ) {
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    const auto refuse = [&](const std::string& why) {
        ctx->err = "pnmol_functionals: bad argument (" + why + ")";
        return -1;
    };
    if (T < 0) return refuse("T < 0");
    if (!filt || !w_QT1nd || !mean_Q || !cov_QQ || (T > 0 && !dt_T)) return refuse("null pointer");
    if (Q < 1) return refuse("Q < 1");
    if (Q > FQ) return refuse("Q = " + std::to_string(Q) + " above PNMOL_FUNCTIONALS_MAX_Q = " + std::to_string(FQ));
    if (f->ds != f->d || f->p32) return refuse("latent-force or fp32 filter");
    if (f->pending_k > 0) return refuse("unfinished pnmol_filter_steps_begin");
    for (int k = 0; k <= T; ++k) {
        if (!filt[k]) return refuse("null state at index " + std::to_string(k));
        if (filt[k]->f != f) return refuse("foreign state at index " + std::to_string(k));
    }
    for (int k = 0; k < T; ++k)
        if (!(dt_T[k] > 0.0) || !std::isfinite(dt_T[k])) return refuse("dt <= 0 or not finite at step " + std::to_string(k));
    const int n = f->n, d = f->d, dp = f->dp;
    const size_t wcount = (size_t)Q * ((size_t)T + 1) * n * d;
    for (size_t i = 0; i < wcount; ++i)
        if (!std::isfinite(w_QT1nd[i])) return refuse("weights not finite");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = ensure_ws(f, T, wcount);
    if (rc != 0) return rc;
    FunctionalWs* ws = f->fn_ws;
    const SweepWs& sw = ws->sweep;
    const long Dp = f->Dp;
    double *Lamt = ws->thin, *Ut = Lamt + FQ * Dp, *Mut = Ut + FQ * Dp, *mh = Mut + FQ * Dp, *Amh = mh + Dp;
    double *cov = Amh + Dp, *mean = cov + FQ * FQ;
    int* info_dev = reinterpret_cast<int*>(ws->out + FQ + FQ * FQ);
    const double* Yt = sw.F + Dp * Dp;
    const unsigned ntile = (unsigned)((Dp + BM - 1) / BM), nlam = (unsigned)((FQ * Dp + 255) / 256);
    const int npanels = (int)ntile;
    FnConsts c{};
    std::memcpy(c.A1, f->iwp.A1, sizeof(c.A1));
    std::memcpy(c.Q1, f->iwp.Q1, sizeof(c.Q1));

    // From here on work is enqueued that reads the caller's states: every way out synchronises the stream first.  what: the
    // message (NULL: the callee has set pnmol_last_error itself)
    const auto failed = [&](int code, int k, const char* what = "kernel launch failed") {
        if (what) ctx->err = std::string("pnmol_functionals: ") + what + " at step " + std::to_string(k);
        (void)hipStreamSynchronize(st);
        return code;
    };
    const auto hip_failed = [&](hipError_t e, const char* call, int k) {
        ctx->err = std::string("pnmol_functionals: ") + call + " at step " + std::to_string(k) + ": " + hipGetErrorString(e);
        (void)hipStreamSynchronize(st);
        return -2;
    };
    const auto launch_code = [](int rc) { return rc == -1 ? "unsupported number of derivatives" : "kernel launch failed"; };
    if (hipError_t e = hipMemcpyAsync(ws->w, w_QT1nd, sizeof(double) * wcount, hipMemcpyHostToDevice, st); e != hipSuccess)
        return hip_failed(e, "copy of the weights", 0);
    if (hipError_t e = hipMemsetAsync(cov, 0, sizeof(double) * (FQ * FQ + FQ), st); e != hipSuccess)
        return hip_failed(e, "hipMemsetAsync", 0);
    double before = 0.0;  // the frame Mu^T is in
    for (int k = 0; k < T; ++k) {
        const double h = dt_T[k];
        for (int a = 0; a < n; ++a) {
            c.ts[a] = frame_ratio(f, a, filt[k]->frame_dt, h);
            c.sc[a] = nordsieck_scale(f->nu, a, h);
            c.cm[a] = k > 0 ? c.sc[a] / frame_scale(f, a, before) : 0.0;
        }
        rc = launch_build(st, n, filt[k]->P, filt[k]->mean, f->Kg, c, d, dp, sw.G, ws->Ph, mh, Amh);
        if (rc != 0) return failed(rc, k, launch_code(rc));
        k_fn_lam<<<nlam, 256, 0, st>>>(ws->w, Q, (long)T + 1, k, n, d, dp, c, k > 0 ? Mut : nullptr, Lamt);
        k_fn_thin<<<ntile, 256, 0, st>>>(Lamt, ws->Ph, Ut, Dp);
        if ((rc = launched()) != 0) return failed(rc, k);
        if ((rc = launch_au(st, n, Ut, c, dp, sw.G + Dp * Dp)) != 0) return failed(rc, k, launch_code(rc));
        if ((rc = sweep_ws_enqueue(f, sw, st, 0, "pnmol_functionals")) != 0) return failed(rc, k, nullptr);
        if (hipError_t e = hipMemcpyAsync(Mut, Yt, sizeof(double) * FQ * Dp, hipMemcpyDeviceToDevice, st); e != hipSuccess)
            return hip_failed(e, "copy of Y", k);
        for (int s = npanels - 1; s >= 0; --s) k_fn_backsub<<<(unsigned)(s + 1), 256, 0, st>>>(Mut, sw.F, sw.Linv, Dp, s, npanels);
        k_fn_gram<<<dim3((unsigned)ws->nsplit, 2), 256, 0, st>>>(Lamt, Ut, Yt, Dp, ws->part);
        k_fn_accum<<<FQ, 256, 0, st>>>(ws->part, ws->nsplit, 1, Lamt, mh, Mut, Amh, Dp, cov, mean, sw.info, info_dev + k);
        if ((rc = launched()) != 0) return failed(rc, k);
        before = h;
    }
    // the terminal term, in the frame of filt[T] itself: mean += Lam_T^T m_T, cov += Lam_T^T P_T Lam_T
    const pnmol_state* last = filt[T];
    for (int a = 0; a < n; ++a) {
        c.ts[a] = 1.0;
        c.sc[a] = frame_scale(f, a, last->frame_dt);
        c.cm[a] = T > 0 ? c.sc[a] / frame_scale(f, a, before) : 0.0;
    }
    rc = launch_build(st, n, nullptr, last->mean, f->Kg, c, d, dp, nullptr, nullptr, mh, Amh);
    if (rc != 0) return failed(rc, T, launch_code(rc));
    k_fn_lam<<<nlam, 256, 0, st>>>(ws->w, Q, (long)T + 1, T, n, d, dp, c, T > 0 ? Mut : nullptr, Lamt);
    k_fn_thin<<<ntile, 256, 0, st>>>(Lamt, last->P, Ut, Dp);
    k_fn_gram<<<dim3((unsigned)ws->nsplit, 1), 256, 0, st>>>(Lamt, Ut, Ut, Dp, ws->part);
    k_fn_accum<<<FQ, 256, 0, st>>>(ws->part, ws->nsplit, 0, Lamt, mh, nullptr, nullptr, Dp, cov, mean, nullptr, nullptr);
    k_fn_out<<<1, 256, 0, st>>>(cov, mean, Q, ws->out);
    if ((rc = launched()) != 0) return failed(rc, T);
    if (hipError_t e = hipMemcpyAsync(ws->out_pin, ws->out, sizeof(double) * out_doubles(T), hipMemcpyDeviceToHost, st); e != hipSuccess)
        return hip_failed(e, "copy of the result", T);
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipGetLastError());
    const int* inf = reinterpret_cast<const int*>(ws->out_pin + FQ + FQ * FQ);
    for (int k = 0; k < T; ++k)
        if (int bad = sweep_info_result(ctx, inf[k], Dp, ("pnmol_functionals: step " + std::to_string(k)).c_str(),
                                        "predicted covariance not positive definite", "a dependency wait of the sweep timed out"))
            return bad;
    std::memcpy(mean_Q, ws->out_pin, sizeof(double) * Q);
    std::memcpy(cov_QQ, ws->out_pin + FQ, sizeof(double) * (size_t)Q * Q);
    return 0;
}
