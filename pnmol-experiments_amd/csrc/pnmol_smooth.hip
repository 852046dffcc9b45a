// pnmol_smooth.hip -- the Rauch-Tung-Striebel backward step (`pnmol_smoother_step`, include/pnmol_hip.h): kernels, then host side.
//
// Reference: src/pnmol/base/kalman.py:33-46 (smoother_step_traditional), in the Nordsieck frame of the step h that the
// forward step used.  With P = P_k (filtered), A = A1 (x) I, Q = Q1 (x) K:
//     P- = A P A^T + Q,   [P-; P A^T; 0; I]  --sweep-->  [L; V; 0; T]    (L L^T = P-,  V = P A^T L^-T,  T = L^-T)
//     G  = V T^T  (= P A^T P-^-1),   C = G Ps,   Ps_k = P - V V^T + C G^T,   ms_k = m + G (ms - A m)
// The sweep is the forward step's own Cholesky launch (pnmol_hip.hip); this file holds what surrounds it: the n x n block
// transform with the frame change (k_sm_build; its predict is predict_block of pnmol_tile.hpp), the vector part (k_sm_vec,
// k_sm_mean), one LDS-staged fp64 MFMA GEMM for every product (k_sm_gemm, on tile_product of pnmol_tile.hpp) and the mirror of
// the lower-half results with the marginal variances (k_sm_mirror).
// Layouts are the forward step's: derivative-major (a, j) -> a*dp + j, Dp = n*dp, row-major, zero padding.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pnmol_internal.hpp"
#include "pnmol_tile.hpp"

namespace {

// P (frame of the filtered state) and Ps (frame of the smoothed successor) -> frame of h:
//   Gs rows [0, Dp):     P- = A1 P^h A1^T + Q1 K   (+1 on the diagonal of the padded points: the sweep needs a pivot)
//   Gs rows [Dp, 2Dp):   P^h A1^T
//   Pout:                P^h  (the accumulator of Ps_k)
//   Psh:                 Ps^h
template <int N>
__global__ __launch_bounds__(256) void k_sm_build(const double* __restrict__ P, const double* __restrict__ Ps,
                                                  const double* __restrict__ Kg, SmoothConsts c, int d, int dp,
                                                  double* __restrict__ Gs, double* __restrict__ Pout, double* __restrict__ Psh) {
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
            Pout[idx] = X[a][b];
            Psh[idx] = c.tsn[a] * c.tsn[b] * Ps[idx];
        }
    double XA[N][N], Pm[N][N];
    predict_block<N>(X, c.A1, c.Q1, Kg[(long)j * dp + k], XA, Pm);
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            Gs[(Dp + (long)a * dp + j) * Dp + (long)b * dp + k] = XA[a][b];
            Gs[((long)a * dp + j) * Dp + (long)b * dp + k] = (a == b && j == k && j >= d) ? 1.0 : Pm[a][b];
        }
}

// mh = ts m (frame of h), dm = tsn ms - A1 mh  (one workgroup)
template <int N>
__global__ __launch_bounds__(256) void k_sm_vec(const double* __restrict__ m, const double* __restrict__ ms, SmoothConsts c,
                                                int dp, double* __restrict__ mh, double* __restrict__ dm) {
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
            dm[a * dp + j] = c.tsn[a] * ms[a * dp + j] - s;
        }
    }
}

// mout = mh + G dm: one wave per row
__global__ __launch_bounds__(256) void k_sm_mean(const double* __restrict__ G, const double* __restrict__ mh,
                                                 const double* __restrict__ dm, double* __restrict__ mout, long Dp) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (row >= Dp) return;
    double s = 0.0;
    for (long i = l; i < Dp; i += 64) s += G[row * Dp + i] * dm[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0) mout[row] = mh[row] + s;
}

// C (+)= alpha1 op(A1) op(B1) [+ alpha2 A2 B2^T] on 64 x 64 tiles, M = N = K = Dp (a multiple of 32, not always of 64:
// the edge tiles load zeros and store nothing outside).  op(B) = B^T (nt) or B.  lower: tiles above the diagonal are
// skipped (symmetric results; k_sm_mirror fills them).  b_upper_nt: B is upper triangular and op(B) = B^T, so column
// tile j0 only needs k >= j0.  The tile routine is tile_product of pnmol_tile.hpp.
struct GemmArgs {
    const double* A1;
    const double* B1;
    const double* A2;  // optional second product (always NT)
    const double* B2;
    double* C;
    long n;  // Dp
    double alpha1, alpha2;
    int nt1, lower, accumulate, b_upper_nt;
};

__global__ __launch_bounds__(256) void k_sm_gemm(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (g.lower && bj > bi) return;
    const int tid = threadIdx.x;
    const long r0 = (long)bi * BM, c0 = (long)bj * BM, n = g.n;
    d4 acc[2][2];
    tile_zero(acc);
    const long kbeg = g.b_upper_nt ? c0 : 0;
    if (g.nt1) tile_product<true>(g.A1, n, n, g.B1, n, n, n, kbeg, g.alpha1, r0, c0, acc, sA, sB, tid);  // (uniform branch)
    else tile_product<false>(g.A1, n, n, g.B1, n, n, n, kbeg, g.alpha1, r0, c0, acc, sA, sB, tid);
    if (g.A2) tile_product<true>(g.A2, n, n, g.B2, n, n, n, 0, g.alpha2, r0, c0, acc, sA, sB, tid);
    tile_each(acc, r0, c0, tid, [&](long row, long col, double v) {
        if (row < n && col < n) {
            double* p = g.C + row * n + col;
            *p = g.accumulate ? *p + v : v;
        }
    });
}

// upper half of P from its lower half (32 x 32 tiles through LDS) and var = diag(P)
__global__ __launch_bounds__(256) void k_sm_mirror(double* __restrict__ P, double* __restrict__ var, long n) {
    __shared__ double s[32][33];
    const int ti = blockIdx.y, tj = blockIdx.x;  // target tile (ti, tj), tj >= ti
    if (tj < ti) return;
    const int tx = threadIdx.x, ty = threadIdx.y;  // 32 x 8
    for (int r = ty; r < 32; r += 8) s[r][tx] = P[((long)tj * 32 + r) * n + (long)ti * 32 + tx];  // source tile (tj, ti)
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long row = (long)ti * 32 + r, col = (long)tj * 32 + tx;
        if (tj > ti || tx > r) P[row * n + col] = s[tx][r];
        if (tj == ti && tx == r) var[row] = s[r][r];
    }
}

// P^h, P- and P^h A^T into Pout / the sweep's tall matrix Gs, Ps^h into Psh, mh = m^h, dm = ms^h - A m^h
int launch_build(hipStream_t st, int n, const double* P, const double* Ps, const double* m, const double* ms, const double* Kg,
                 const SmoothConsts& c, int d, int dp, double* Gs, double* Pout, double* Psh, double* mh, double* dm) {
    const dim3 grid(dp / 32, dp / 8), blk(32, 8);
    switch (n) {
        case 2:
            k_sm_build<2><<<grid, blk, 0, st>>>(P, Ps, Kg, c, d, dp, Gs, Pout, Psh);
            k_sm_vec<2><<<1, 256, 0, st>>>(m, ms, c, dp, mh, dm);
            break;
        case 3:
            k_sm_build<3><<<grid, blk, 0, st>>>(P, Ps, Kg, c, d, dp, Gs, Pout, Psh);
            k_sm_vec<3><<<1, 256, 0, st>>>(m, ms, c, dp, mh, dm);
            break;
        case 4:
            k_sm_build<4><<<grid, blk, 0, st>>>(P, Ps, Kg, c, d, dp, Gs, Pout, Psh);
            k_sm_vec<4><<<1, 256, 0, st>>>(m, ms, c, dp, mh, dm);
            break;
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// from the sweep's V = P A^T L^-T and T = L^-T: G, C = G Ps^h, Pout = P^h - V V^T + C G^T (mirrored), var, mout = mh + G dm
int launch_finish(hipStream_t st, long Dp, const double* V, const double* T, const double* Psh, const double* mh, const double* dm,
                  double* G, double* C, double* Pout, double* mout, double* var) {
    const unsigned nt = (unsigned)((Dp + BM - 1) / BM);
    const dim3 grid(nt, nt);
    // G = V T^T  (T = L^-T upper triangular: column tile j0 needs k >= j0)
    k_sm_gemm<<<grid, 256, 0, st>>>(GemmArgs{V, T, nullptr, nullptr, G, Dp, 1.0, 0.0, 1, 0, 0, 1});
    // C = G Ps^h
    k_sm_gemm<<<grid, 256, 0, st>>>(GemmArgs{G, Psh, nullptr, nullptr, C, Dp, 1.0, 0.0, 0, 0, 0, 0});
    // Ps_k = P^h - V V^T + C G^T  (lower half, accumulated onto P^h)
    k_sm_gemm<<<grid, 256, 0, st>>>(GemmArgs{V, V, C, G, Pout, Dp, -1.0, 1.0, 1, 1, 1, 0});
    k_sm_mirror<<<dim3((unsigned)(Dp / 32), (unsigned)(Dp / 32)), dim3(32, 8), 0, st>>>(Pout, var, Dp);
    k_sm_mean<<<(unsigned)((Dp + 3) / 4), 256, 0, st>>>(G, mh, dm, mout, Dp);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// the tail of a smoother step: the sweep's info word, one stream synchronisation
int smoother_step_wait(pnmol_filter* f, const pnmol_state* filt_k, double dt, pnmol_state* out) {
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    int inf = 0;
    HIPCHK(ctx, hipMemcpyAsync(&inf, f->sm_sweep.info, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipGetLastError());
    out->t = filt_k->t;
    out->frame_dt = dt;
    return sweep_info_result(ctx, inf, f->Dp, "pnmol_smoother_step", "predicted covariance not positive definite",
                             "a dependency wait of the sweep timed out");
}

int smoother_step_impl(pnmol_filter* f, const pnmol_state* filt_k, const pnmol_state* smooth_next, double dt, pnmol_state* out,
                       int keep_full, pnmol_bridge** bridge) {
    if (bridge) *bridge = nullptr;
    if (!f || !filt_k || !smooth_next || !out || out == filt_k || out == smooth_next || filt_k->f != f || smooth_next->f != f ||
        out->f != f || !(dt > 0.0) || f->ds != f->d || f->p32) {
        if (f) f->ctx->err = "pnmol_smoother_step: bad argument (null, aliasing, foreign state, dt <= 0, latent-force or fp32 filter)";
        return -1;
    }
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = pnmol_smooth_ensure_ws(f);
    if (rc != 0) return rc;
    // everything in the Nordsieck frame of dt: ts / tsn move the two inputs there (as k_predict's IwpConsts.ts)
    SmoothConsts c{};
    std::memcpy(c.A1, f->iwp.A1, sizeof(c.A1));
    std::memcpy(c.Q1, f->iwp.Q1, sizeof(c.Q1));
    for (int a = 0; a < f->n; ++a) {
        c.ts[a] = frame_ratio(f, a, filt_k->frame_dt, dt);
        c.tsn[a] = frame_ratio(f, a, smooth_next->frame_dt, dt);
    }
    const long Dp = f->Dp;
    const SweepWs& sw = f->sm_sweep;
    double *mh = f->sm_vec, *dm = f->sm_vec + Dp;
    rc = launch_build(st, f->n, filt_k->P, smooth_next->P, filt_k->mean, smooth_next->mean, f->Kg, c, f->d, f->dp, sw.G, out->P,
                      f->sm_Psh, mh, dm);
    if (rc != 0) {
        ctx->err = "pnmol_smoother_step: kernel launch failed";
        return rc;
    }
    if ((rc = sweep_ws_enqueue(f, sw, st, 0, "pnmol_smoother_step")) != 0) return rc;
    const double* V = sw.F + Dp * Dp;
    const double* T = sw.F + (2 * Dp + NB) * Dp;
    rc = launch_finish(st, Dp, V, T, f->sm_Psh, mh, dm, f->sm_gain, f->sm_C, out->P, out->mean, out->var);
    if (rc != 0) {
        ctx->err = "pnmol_smoother_step: kernel launch failed";
        return rc;
    }
    if (bridge) {
        rc = pnmol_dense_make_bridge(f, filt_k, smooth_next, dt, out, c.tsn, keep_full, bridge);
        if (rc != 0) return rc;
    }
    rc = smoother_step_wait(f, filt_k, dt, out);
    if (rc != 0 && bridge && *bridge) {
        pnmol_bridge_destroy(*bridge);
        *bridge = nullptr;
    }
    return rc;
}

// Row `row` of the smoothed read-outs of a whole backward pass (pnmol_smoother_steps), the arithmetic of the loop's k_readout:
// s0 m[j] and s0 sqrt(max(var[j], 0)) of derivative 0.  Thread 0 also keeps the step's sweep info word, which the next step's
// sweep resets (sweep_info = NULL: the terminal row, which no sweep made).
__global__ __launch_bounds__(256) void k_sm_readout(const double* __restrict__ mean, const double* __restrict__ var, double s0,
                                                    int d, double* __restrict__ means_row, double* __restrict__ stds_row,
                                                    const int* __restrict__ sweep_info, int* __restrict__ info_step) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < d) {
        means_row[j] = s0 * mean[j];
        stds_row[j] = s0 * sqrt(fmax(var[j], 0.0));
    }
    if (j == 0 && sweep_info) *info_step = *sweep_info;
}

// the buffers of pnmol_smoother_steps: the read-out of `rows` rows (grown on demand) and, for a pass that keeps no states, the two
// rotating ones
int smoother_steps_ensure(pnmol_filter* f, int rows, bool rotate) {
    pnmol_ctx* ctx = f->ctx;
    const size_t Dp = (size_t)f->Dp;
    if (rows > f->sm_ro_rows) {
        if (f->sm_ro) (void)hipFree(f->sm_ro);
        if (f->sm_ro_pin) (void)hipHostFree(f->sm_ro_pin);
        f->sm_ro = f->sm_ro_pin = nullptr, f->sm_ro_rows = 0;
        const size_t bytes = sizeof(double) * ((size_t)2 * rows * f->d + (size_t)rows);
        hipError_t e = hipMalloc(&f->sm_ro, bytes);
        if (e == hipSuccess) e = hipHostMalloc(&f->sm_ro_pin, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            if (f->sm_ro) (void)hipFree(f->sm_ro);
            f->sm_ro = nullptr;
            ctx->err = std::string("pnmol_smoother_steps: read-out buffers: ") + hipGetErrorString(e);
            return e == hipErrorOutOfMemory ? -4 : -2;
        }
        f->sm_ro_rows = rows;
    }
    for (int i = 0; rotate && i < 2; ++i)
        if (!f->sm_rot[i]) {
            const hipError_t e = hipMalloc(&f->sm_rot[i], sizeof(double) * (Dp * Dp + 2 * Dp));
            if (e != hipSuccess) {
                f->sm_rot[i] = nullptr;
                ctx->err = std::string("pnmol_smoother_steps: rotating states: ") + hipGetErrorString(e);
                return e == hipErrorOutOfMemory ? -4 : -2;
            }
        }
    return 0;
}

}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------------------
// The tall matrix of the backward step has the error model's layout with Dp columns: [P- (cb); P A^T (cb); zero block; I (cb)],
// so the forward step's sweep launch factorises it as it is (strict pivots: P- >= Q1 (x) K is positive definite; the padded
// points carry a unit pivot).  Allocated on first use, with G, C, Ps^h (Dp x Dp) and [m^h | dm] (2 Dp).
void pnmol_smooth_free_ws(pnmol_filter* f) {
    sweep_ws_free(&f->sm_sweep);
    for (void* p : {(void*)f->sm_gain, (void*)f->sm_C, (void*)f->sm_Psh, (void*)f->sm_vec})
        if (p) (void)hipFree(p);
    f->sm_gain = f->sm_C = f->sm_Psh = f->sm_vec = nullptr;
    for (void* p : {(void*)f->sm_rot[0], (void*)f->sm_rot[1], (void*)f->sm_ro})
        if (p) (void)hipFree(p);
    if (f->sm_ro_pin) (void)hipHostFree(f->sm_ro_pin);
    f->sm_rot[0] = f->sm_rot[1] = f->sm_ro = f->sm_ro_pin = nullptr;
    f->sm_ro_rows = 0;
}

int pnmol_smooth_ensure_ws(pnmol_filter* f) {
    if (f->sm_sweep.G) return 0;
    const long Dp = f->Dp;
    const int cb = (int)(Dp / NB);
    const size_t sq = (size_t)Dp * Dp;
    hipError_t e = sweep_ws_alloc(&f->sm_sweep, f->ctx, 3 * cb + 1, cb);
    if (e == hipSuccess) e = hipMalloc(&f->sm_gain, sizeof(double) * sq);
    if (e == hipSuccess) e = hipMalloc(&f->sm_C, sizeof(double) * sq);
    if (e == hipSuccess) e = hipMalloc(&f->sm_Psh, sizeof(double) * sq);
    if (e == hipSuccess) e = hipMalloc(&f->sm_vec, sizeof(double) * 2 * (size_t)Dp);
    if (e != hipSuccess) {
        f->ctx->err = std::string("pnmol_smoother_step: workspace: ") + hipGetErrorString(e);
        pnmol_smooth_free_ws(f);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    return 0;
}

int pnmol_smoother_step(pnmol_filter* f, const pnmol_state* filt_k, const pnmol_state* smooth_next, double dt,
                        pnmol_state* out) {
    return smoother_step_impl(f, filt_k, smooth_next, dt, out, 0, nullptr);
}

int pnmol_smoother_step_bridge(pnmol_filter* f, const pnmol_state* filt_k, const pnmol_state* smooth_next, double dt,
                               pnmol_state* out, int keep_full, pnmol_bridge** bridge) {
    if (!bridge) {
        if (f) f->ctx->err = "pnmol_smoother_step_bridge: bad argument (null bridge pointer)";
        return -1;
    }
    return smoother_step_impl(f, filt_k, smooth_next, dt, out, keep_full, bridge);
}

// The whole backward pass: what T calls of pnmol_smoother_step compute, enqueued back to back with one synchronisation at the end.
int pnmol_smoother_steps(pnmol_filter* f, int T, pnmol_state* const* filt, const double* dt_T, pnmol_state* const* out,
                         double* means_T1d, double* stds_T1d, int* info_T) {
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    const auto refuse = [&](const std::string& why) {
        ctx->err = "pnmol_smoother_steps: " + why;
        return -1;
    };
    if (T < 1 || !filt || !dt_T) return refuse("bad argument (T < 1, or no filtered states, or no step sizes)");
    if (f->ds != f->d || f->p32) return refuse("bad argument (latent-force or fp32 filter)");
    for (int k = 0; k <= T; ++k) {
        if (!filt[k] || (out && !out[k])) return refuse("bad argument (null state at index " + std::to_string(k) + ")");
        if (filt[k]->f != f || (out && out[k]->f != f)) return refuse("bad argument (foreign state at index " + std::to_string(k) + ")");
    }
    for (int k = 0; k < T; ++k)
        if (!(dt_T[k] > 0.0)) return refuse("bad argument (dt <= 0 at step " + std::to_string(k) + ")");
    if (out) {
        std::vector<const pnmol_state*> in(filt, filt + T + 1), res(out, out + T + 1);
        std::sort(in.begin(), in.end());
        std::sort(res.begin(), res.end());
        if (std::adjacent_find(res.begin(), res.end()) != res.end()) return refuse("bad argument (aliasing: a state listed twice in out)");
        for (const pnmol_state* s : res)
            if (std::binary_search(in.begin(), in.end(), s)) return refuse("bad argument (aliasing: a state of out is one of filt)");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = pnmol_smooth_ensure_ws(f);
    if (rc != 0) return rc;
    if ((rc = smoother_steps_ensure(f, T + 1, out == nullptr)) != 0) return rc;
    const long Dp = f->Dp;
    const int d = f->d, rows = T + 1;
    const size_t sq = (size_t)Dp * Dp;
    double *ro_means = f->sm_ro, *ro_stds = f->sm_ro + (size_t)rows * d;
    int* ro_info = reinterpret_cast<int*>(f->sm_ro + (size_t)2 * rows * d);
    const unsigned rblocks = (unsigned)((d + 255) / 256);
    const SweepWs& sw = f->sm_sweep;
    double *mh = f->sm_vec, *dm = f->sm_vec + Dp;
    const double* V = sw.F + Dp * Dp;
    const double* T_ = sw.F + (2 * Dp + NB) * Dp;
    SmoothConsts c{};
    std::memcpy(c.A1, f->iwp.A1, sizeof(c.A1));
    std::memcpy(c.Q1, f->iwp.Q1, sizeof(c.Q1));

    // row T: the terminal filtered state (a copy of it in out[T])
    const pnmol_state* last = filt[T];
    const double *nP = last->P, *nM = last->mean, *nV = last->var;
    double nframe = last->frame_dt;
    if (out) {
        HIPCHK(ctx, hipMemcpyAsync(out[T]->P, last->P, sizeof(double) * sq, hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(out[T]->mean, last->mean, sizeof(double) * Dp, hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(out[T]->var, last->var, sizeof(double) * Dp, hipMemcpyDeviceToDevice, st));
    }
    k_sm_readout<<<rblocks, 256, 0, st>>>(nM, nV, nframe == 0.0 ? 1.0 : nordsieck_scale(f->nu, 0, nframe), d,
                                          ro_means + (size_t)T * d, ro_stds + (size_t)T * d, nullptr, nullptr);
    for (int k = T - 1; k >= 0; --k) {
        const double dt = dt_T[k];
        for (int a = 0; a < f->n; ++a) {
            c.ts[a] = frame_ratio(f, a, filt[k]->frame_dt, dt);
            c.tsn[a] = frame_ratio(f, a, nframe, dt);
        }
        double* base = out ? nullptr : f->sm_rot[(T - 1 - k) & 1];
        double* oP = out ? out[k]->P : base;
        double* oM = out ? out[k]->mean : base + sq;
        double* oV = out ? out[k]->var : base + sq + Dp;
        rc = launch_build(st, f->n, filt[k]->P, nP, filt[k]->mean, nM, f->Kg, c, f->d, f->dp, sw.G, oP, f->sm_Psh, mh, dm);
        if (rc == 0) rc = sweep_ws_enqueue(f, sw, st, 0, "pnmol_smoother_steps");
        if (rc == 0) rc = launch_finish(st, Dp, V, T_, f->sm_Psh, mh, dm, f->sm_gain, f->sm_C, oP, oM, oV);
        if (rc == 0) {
            k_sm_readout<<<rblocks, 256, 0, st>>>(oM, oV, nordsieck_scale(f->nu, 0, dt), d, ro_means + (size_t)k * d,
                                                  ro_stds + (size_t)k * d, sw.info, ro_info + k);
            if (hipGetLastError() != hipSuccess) rc = -2;
        }
        if (rc != 0) {
            if (rc != -1) ctx->err = "pnmol_smoother_steps: kernel launch failed at step " + std::to_string(k);
            (void)hipStreamSynchronize(st);
            return rc;
        }
        nP = oP, nM = oM, nV = oV, nframe = dt;
    }
    const size_t bytes = sizeof(double) * ((size_t)2 * rows * d + (size_t)rows);
    HIPCHK(ctx, hipMemcpyAsync(f->sm_ro_pin, f->sm_ro, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipGetLastError());
    if (means_T1d) std::memcpy(means_T1d, f->sm_ro_pin, sizeof(double) * (size_t)rows * d);
    if (stds_T1d) std::memcpy(stds_T1d, f->sm_ro_pin + (size_t)rows * d, sizeof(double) * (size_t)rows * d);
    if (out) {
        out[T]->t = last->t, out[T]->frame_dt = last->frame_dt;
        for (int k = 0; k < T; ++k) out[k]->t = filt[k]->t, out[k]->frame_dt = dt_T[k];
    }
    const int* inf = reinterpret_cast<const int*>(f->sm_ro_pin + (size_t)2 * rows * d);
    int first_rc = 0;
    for (int k = T - 1; k >= 0; --k) {  // backward order: the first step that failed is the one with the largest k
        const int code = inf[k] == -2 ? -2 : (inf[k] < Dp ? -3 : 0);
        if (info_T) info_T[k] = code;
        if (code != 0 && first_rc == 0)
            first_rc = sweep_info_result(ctx, inf[k], Dp, ("pnmol_smoother_steps: step " + std::to_string(k)).c_str(),
                                         "predicted covariance not positive definite", "a dependency wait of the sweep timed out");
    }
    return first_rc;
}
