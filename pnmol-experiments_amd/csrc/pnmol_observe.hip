// pnmol_observe.hip -- conditioning a state on sensor data (`pnmol_state_observe`, include/pnmol_hip.h): kernels, then host side.
//
// Model: y = C E0 x + e, e ~ N(0, R R^T): q linear functionals of derivative 0 of the state components.  With m, P in the
// frame the state carries (sc[0] = raw-coordinate scale of derivative 0), H = sc[0] C acting on derivative block 0:
//     B = P[:, block 0] H^T  (Dp x q),   S = H B[block 0] + R R^T,   v = y - H m[block 0]
//     [S; B; v^T]  --sweep-->  [Ls; W = B Ls^-T; w^T = v^T Ls^-T]          (the forward step's own Cholesky launch, strict pivots)
//     m_out = m + W w,   P_out = P - W W^T,   log p(y) = -1/2 (|w|^2 + 2 sum log Ls_ii + q log 2 pi)
// Columns are padded to qp (a multiple of 32, at least 64: the smallest tall shape the sweep runs elsewhere); the padded pivots
// carry a unit diagonal, the padded rows of H are zero.  Every product runs on one LDS-staged fp64 MFMA tile routine
// (tile_product of pnmol_tile.hpp, which the smoother's GEMM uses too): the thin product B (k_ob_thin), S and the v^T row
// block (k_ob_build), and the down-date P - W W^T on lower 64 x 64 tiles, mirrored through LDS, with the marginal variances
// (k_ob_syrk).
// Layouts are the forward step's: derivative-major (a, j) -> a*dp + j, Dp = n*dp, row-major, zero padding.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "pnmol_internal.hpp"
#include "pnmol_tile.hpp"

namespace {

constexpr int LDO = BM + 1;  // LDS row pitch of an output tile image

// B = P[:, block 0] H^T into the rows [qp, qp + Dp) of the sweep's tall matrix (Gb: row pitch qp).  Hp: qp x dp, the rows of
// H = sc[0] C padded with zeros, so the contraction runs over the dp columns of derivative block 0.
__global__ __launch_bounds__(256) void k_ob_thin(const double* __restrict__ P, long Dp, int dp, const double* __restrict__ Hp,
                                                 int qp, double* __restrict__ Gb) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.y * BM, c0 = (long)blockIdx.x * BM;
    d4 acc[2][2];
    tile_zero(acc);
    tile_product<true>(P, Dp, Dp, Hp, dp, qp, dp, 0, 1.0, r0, c0, acc, sA, sB, tid);
    tile_each(acc, r0, c0, tid, [&](long row, long col, double v) {
        if (row < Dp && col < qp) Gb[row * qp + col] = v;
    });
}

// The rest of the tall matrix.  Blocks [0, nS^2): a 64 x 64 tile of S = Hp B[block 0] + Rp Rp^T (rows [0, qp) of G; Rp = R
// padded with zeros, or NULL: noise-free; unit diagonal on the padded pivots q .. qp).  The qp / 4 blocks behind them: one
// wave per column r of the last row block, whose first row is v^T = (y - H m[block 0])^T and whose other 31 rows are zero.
__global__ __launch_bounds__(256) void k_ob_build(const double* __restrict__ Hp, int dp, const double* __restrict__ Gb,
                                                  const double* __restrict__ Rp, const double* __restrict__ yv,
                                                  const double* __restrict__ m, int q, int qp, int nS, double* __restrict__ G,
                                                  double* __restrict__ Gv) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    if ((int)blockIdx.x >= nS * nS) {
        const int r = ((int)blockIdx.x - nS * nS) * 4 + w;
        if (r >= qp) return;
        double s = 0.0;
        for (int j = l; j < dp; j += 64) s += Hp[(long)r * dp + j] * m[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (l < NB) Gv[(long)l * qp + r] = (l == 0 && r < q) ? yv[r] - s : 0.0;
        return;
    }
    const long r0 = (long)(blockIdx.x / nS) * BM, c0 = (long)(blockIdx.x % nS) * BM;
    d4 acc[2][2];
    tile_zero(acc);
    tile_product<false>(Hp, dp, qp, Gb, qp, qp, dp, 0, 1.0, r0, c0, acc, sA, sB, tid);
    if (Rp) tile_product<true>(Rp, qp, qp, Rp, qp, qp, qp, 0, 1.0, r0, c0, acc, sA, sB, tid);
    tile_each(acc, r0, c0, tid, [&](long row, long col, double v) {
        if (row < qp && col < qp) G[row * qp + col] = (row == col && row >= q) ? 1.0 : v;
    });
}

// Pout = Pin - W W^T (W: Dp x qp) and var = diag(Pout).  One workgroup per lower 64 x 64 tile (Dp is a multiple of 32, not
// always of 64: the edge tiles load zeros and store nothing outside): the product on the MFMA, then the tile goes through LDS
// so that Pin is read and the tile and its mirror image are written in full rows -- P is read once and written once.
// (the body: Pin and Pout carry no __restrict__ here, so that the in-place kernel below may hand the same matrix in as both.  In
// place is safe: a workgroup reads only the tile it then writes, and the mirror image comes out of LDS.)
__device__ __forceinline__ void ob_syrk_tile(const double* __restrict__ W, int qp, const double* Pin, double* Pout,
                                             double* __restrict__ var, long Dp) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    __shared__ double sT[BM * LDO];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    const int tid = threadIdx.x;
    const long r0 = (long)bi * BM, c0 = (long)bj * BM;
    const bool diag = bi == bj;
    d4 acc[2][2];
    tile_zero(acc);
    tile_product<true>(W, qp, Dp, W, qp, Dp, qp, 0, 1.0, r0, c0, acc, sA, sB, tid);
    tile_each(acc, 0, 0, tid, [&](long r, long c, double v) { sT[r * LDO + c] = v; });  // (tile-local)
    __syncthreads();
    // the tile itself (a diagonal tile: its lower half), rows of 64 consecutive doubles
    for (int e = tid; e < BM * BM; e += 256) {
        const int r = e >> 6, c = e & 63;
        const long row = r0 + r, col = c0 + c;
        if (row >= Dp || col >= Dp || (diag && c > r)) continue;
        const double v = Pin[row * Dp + col] - sT[r * LDO + c];
        Pout[row * Dp + col] = v;
        sT[r * LDO + c] = v;
        if (diag && r == c) var[row] = v;
    }
    __syncthreads();
    // its mirror image (a diagonal tile: the strict upper half)
    for (int e = tid; e < BM * BM; e += 256) {
        const int r = e >> 6, c = e & 63;
        const long row = c0 + r, col = r0 + c;
        if (row >= Dp || col >= Dp || (diag && c <= r)) continue;
        Pout[row * Dp + col] = sT[c * LDO + r];
    }
}

__global__ __launch_bounds__(256) void k_ob_syrk(const double* __restrict__ W, int qp, const double* __restrict__ Pin,
                                                 double* __restrict__ Pout, double* __restrict__ var, long Dp) {
    ob_syrk_tile(W, qp, Pin, Pout, var, Dp);
}
// P -= W W^T in place (the constant-step loop updates the state on whichever ping-pong buffer is current)
__global__ __launch_bounds__(256) void k_ob_syrk_inplace(const double* __restrict__ W, int qp, double* P, double* __restrict__ var,
                                                         long Dp) {
    ob_syrk_tile(W, qp, P, P, var, Dp);
}

// mout = m + W w: one wave per row (a row is read and written by the same lane: safe in place, through ob_mean_row's plain pointers)
__device__ __forceinline__ void ob_mean_row(const double* __restrict__ W, const double* __restrict__ wv, const double* m, double* mout,
                                            long Dp, int qp) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (row >= Dp) return;
    double s = 0.0;
    for (int i = l; i < qp; i += 64) s += W[row * qp + i] * wv[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0) mout[row] = m[row] + s;
}
__global__ __launch_bounds__(256) void k_ob_mean(const double* __restrict__ W, const double* __restrict__ wv,
                                                 const double* __restrict__ m, double* __restrict__ mout, long Dp, int qp) {
    ob_mean_row(W, wv, m, mout, Dp, qp);
}
__global__ __launch_bounds__(256) void k_ob_mean_inplace(const double* __restrict__ W, const double* __restrict__ wv, double* m,
                                                         long Dp, int qp) {
    ob_mean_row(W, wv, m, m, Dp, qp);
}

// res = [|w|^2, 2 sum log Ls_ii, k + 1 for the first pivot k < q that the sweep dropped or that is not finite (0: none)]
// (one workgroup; a dropped pivot leaves a zero on the diagonal of Ls)
__global__ __launch_bounds__(256) void k_ob_scalars(const double* __restrict__ Ls, const double* __restrict__ wv, int q, int qp,
                                                    double* __restrict__ res) {
    __shared__ double red[3][4];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    double maha = 0.0, ld = 0.0, bad = 0.0;
    for (int r = tid; r < q; r += 256) {
        const double x = wv[r], d = Ls[(long)r * qp + r];
        maha += x * x;
        const bool ok = d > 0.0 && d < __builtin_inf();
        if (ok) ld += log(d);
        else if (bad == 0.0) bad = (double)(r + 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        maha += __shfl_xor(maha, o);
        ld += __shfl_xor(ld, o);
        const double other = __shfl_xor(bad, o);
        if (other != 0.0 && (bad == 0.0 || other < bad)) bad = other;
    }
    if (l == 0) red[0][w] = maha, red[1][w] = ld, red[2][w] = bad;
    __syncthreads();
    if (tid == 0) {
        double b = 0.0;
        for (int i = 0; i < 4; ++i)
            if (red[2][i] != 0.0 && (b == 0.0 || red[2][i] < b)) b = red[2][i];
        res[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        res[1] = 2.0 * (red[1][0] + red[1][1] + red[1][2] + red[1][3]);
        res[2] = b;
    }
}

// ---- the sensor plan of the constant-step loop (pnmol_filter_set_observations) ----------------------------------------------------
// C stays unscaled on the device; the derivative-0 scale sc0 of H = sc0 C (the frame the state is in) is a launch argument.

// sweep route (the default): Hs = sc0 C, the product pnmol_state_observe forms on the host -- the same bits
__global__ __launch_bounds__(256) void k_ob_scale(const double* __restrict__ C, double sc0, long count, double* __restrict__ Hs) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < count) Hs[e] = sc0 * C[e];
}

constexpr int QB = 32;       // padded rows of the single-workgroup route (q <= 32, PNMOL_HIP_OBSERVE_SINGLE_WG=1)
constexpr int LDQ = QB + 1;  // LDS row pitch of a QB x QB matrix

// single-workgroup route, 1: Bw = sc0 P[:, block 0] C^T (Dp x 32, row pitch 32); C: 32 x dp, rows >= q zero.  One workgroup per 64
// rows; the right half of the 64 x 64 tile is computed from zeros and not stored.
__global__ __launch_bounds__(256) void k_obq_thin(const double* __restrict__ P, long Dp, int dp, const double* __restrict__ C,
                                                  double sc0, double* __restrict__ Bw) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * BM;
    d4 acc[2][2];
    tile_zero(acc);
    tile_product<true>(P, Dp, Dp, C, dp, QB, dp, 0, sc0, r0, 0, acc, sA, sB, tid);
    tile_each(acc, r0, 0, tid, [&](long row, long col, double v) {
        if (row < Dp && col < QB) Bw[row * QB + col] = v;
    });
}

// single-workgroup route, 2 (one workgroup): S = sc0 C Bw[block 0] + R R^T (unit diagonal on the padded pivots q .. 31), its
// Cholesky factor in LDS in plain fp64 (right-looking, two barriers per column; the sweep's pivot rule: a pivot that is not above
// 1e-13 of its diagonal entry, or not finite, is dropped -- zero column of Ls, zero row and column of Ls^-1 -- and reported),
// X = Ls^-1 (one lane per column), v = y - sc0 C m[block 0], w = X v, and res = [|w|^2, 2 sum log Ls_ii, first dropped pivot + 1
// (0: none), the "no failure" info word of the sweep route].
__global__ __launch_bounds__(256) void k_obq_factor(const double* __restrict__ C, int dp, const double* __restrict__ Bw,
                                                    const double* __restrict__ R, const double* __restrict__ y,
                                                    const double* __restrict__ m, double sc0, int q, double* __restrict__ Xout,
                                                    double* __restrict__ wout, double* __restrict__ res) {
    __shared__ __attribute__((aligned(16))) double sA[BK * LDT];
    __shared__ __attribute__((aligned(16))) double sB[BK * LDT];
    __shared__ double sS[QB * LDQ], sX[QB * LDQ], sv[QB], sd[QB], sl[QB], sw[QB];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    d4 acc[2][2];
    tile_zero(acc);
    tile_product<false>(C, dp, QB, Bw, QB, QB, dp, 0, sc0, 0, 0, acc, sA, sB, tid);
    if (R) tile_product<true>(R, QB, QB, R, QB, QB, QB, 0, 1.0, 0, 0, acc, sA, sB, tid);
    tile_each(acc, 0, 0, tid, [&](long row, long col, double v) {
        if (row < QB && col < QB) sS[row * LDQ + col] = (row == col && row >= q) ? 1.0 : v;
    });
    // v: wave w takes the rows 8 w .. 8 w + 7
    for (int r = 8 * w; r < 8 * w + 8; ++r) {
        double s = 0.0;
        for (int j = l; j < dp; j += 64) s += C[(long)r * dp + j] * m[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (l == 0) sv[r] = r < q ? y[r] - sc0 * s : 0.0;
    }
    __syncthreads();
    if (tid < QB) sd[tid] = fabs(sS[tid * LDQ + tid]);
    double bad = 0.0;
    for (int k = 0; k < QB; ++k) {
        __syncthreads();  // (the trailing update of column k - 1; sd)
        const double p = sS[k * LDQ + k];
        const bool drop = !(p > 1e-13 * sd[k]) || !(p < __builtin_inf());
        const double lk = drop ? 0.0 : sqrt(p);
        if (drop && bad == 0.0 && k < q) bad = (double)(k + 1);
        if (tid < QB && tid > k) sS[tid * LDQ + k] = drop ? 0.0 : sS[tid * LDQ + k] / lk;
        if (tid == 0) sl[k] = lk;
        __syncthreads();
        for (int e = tid; e < QB * QB; e += 256) {
            const int i = e >> 5, j = e & 31;
            if (j > k && i >= j) sS[i * LDQ + j] -= sS[i * LDQ + k] * sS[j * LDQ + k];
        }
    }
    __syncthreads();
    if (tid < QB) {
        const int j = tid;
        for (int i = 0; i < QB; ++i) {
            double x = 0.0;
            if (i == j) x = sl[j] > 0.0 ? 1.0 / sl[j] : 0.0;
            else if (i > j) {
                double s = 0.0;
                for (int k = j; k < i; ++k) s += sS[i * LDQ + k] * sX[k * LDQ + j];
                x = sl[i] > 0.0 ? -s / sl[i] : 0.0;
            }
            sX[i * LDQ + j] = x;
        }
    }
    __syncthreads();
    if (tid < QB) {
        double s = 0.0;
        for (int j = 0; j <= tid; ++j) s += sX[tid * LDQ + j] * sv[j];
        sw[tid] = s;
        wout[tid] = s;
    }
    for (int e = tid; e < QB * QB; e += 256) Xout[e] = sX[(e >> 5) * LDQ + (e & 31)];
    __syncthreads();
    if (tid == 0) {
        double maha = 0.0, ld = 0.0;
        for (int r = 0; r < q; ++r) {
            maha += sw[r] * sw[r];
            if (sl[r] > 0.0) ld += log(sl[r]);
        }
        res[0] = maha, res[1] = 2.0 * ld, res[2] = bad, res[3] = (double)0x7f7f7f7f;
    }
}

// single-workgroup route, 3: W = Bw X^T (X = Ls^-1 lower triangular) and m += W w; eight rows per workgroup, one lane per entry
__global__ __launch_bounds__(256) void k_obq_gain(const double* __restrict__ Bw, const double* __restrict__ X,
                                                  const double* __restrict__ wv, double* __restrict__ W, double* __restrict__ mean,
                                                  long Dp) {
    __shared__ double sX[QB * LDQ], sBr[8 * QB], sw[QB];
    const int tid = threadIdx.x, r = tid >> 5, j = tid & 31;
    const long row = (long)blockIdx.x * 8 + r;
    for (int e = tid; e < QB * QB; e += 256) sX[(e >> 5) * LDQ + (e & 31)] = X[e];
    if (tid < QB) sw[tid] = wv[tid];
    sBr[tid] = row < Dp ? Bw[row * QB + j] : 0.0;
    __syncthreads();
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < QB; ++k) s += sBr[r * QB + k] * sX[j * LDQ + k];  // (X is zero above its diagonal)
    if (row < Dp) W[row * QB + j] = s;
    double t = s * sw[j];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (j == 0 && row < Dp) mean[row] += t;
}

// Behind an update of the loop: the step's record slot again, from the conditioned state (k_readout's arithmetic, raw coordinates),
// and (sweep route) the sweep's info word into the entry's result slot -- the next update's sweep resets the word.
__global__ __launch_bounds__(256) void k_ob_finish(const double* __restrict__ mean, const double* __restrict__ var, double s0, int d,
                                                   double* __restrict__ means, double* __restrict__ stds,
                                                   const int* __restrict__ info, double* __restrict__ res) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (means && j < d) {
        means[j] = s0 * mean[j];
        stds[j] = s0 * sqrt(fmax(var[j], 0.0));
    }
    if (info && j == 0) res[3] = (double)*info;
}

// results of the entries [first, first + count) into the mapped staging buffer (pnmol_state_observe_planned; the loop's own
// copy-out kernel carries them otherwise)
__global__ void k_ob_results_out(const double* __restrict__ res, double* __restrict__ out, int first, int count) {
    for (int e = threadIdx.x; e < 4 * count; e += blockDim.x) out[4 * first + e] = res[4 * first + e];
}

// padded column count of a q-row update
inline int observe_qp(int q) { return std::max(2 * NB, round_up(q, NB)); }

}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------------------
// One workspace per padded column count qp, kept by the filter (at most d_state / 32 of them): the sweep's tall matrix
// [S (cb); B (Dp / 32); v^T block] with cb = qp / 32 column blocks, and one device block [Hp (qp x dp) | Rp (qp x qp) | y (qp) |
// res (4)] with its host image.  sweep_ws_alloc plants an identity in the last cb row blocks of G, as the error model's layout
// has one there; every call overwrites all of G.
void pnmol_observe_free_ws(pnmol_filter* f) {
    for (ObserveWs* w : f->ob_ws) {
        sweep_ws_free(&w->sweep);
        if (w->dev) (void)hipFree(w->dev);
        delete w;
    }
    f->ob_ws.clear();
}

namespace {

int observe_ensure_ws(pnmol_filter* f, int qp, ObserveWs** out) {
    for (ObserveWs* w : f->ob_ws)
        if (w->qp == qp) {
            *out = w;
            return 0;
        }
    ObserveWs* w = new ObserveWs();
    w->qp = qp;
    const int cb = qp / NB;
    const size_t doubles = (size_t)qp * f->dp + (size_t)qp * qp + (size_t)qp + 4;
    hipError_t e = sweep_ws_alloc(&w->sweep, f->ctx, cb + (int)(f->Dp / NB) + 1, cb);
    if (e == hipSuccess) e = hipMalloc(&w->dev, sizeof(double) * doubles);
    if (e != hipSuccess) {
        f->ctx->err = std::string("pnmol_state_observe: workspace: ") + hipGetErrorString(e);
        sweep_ws_free(&w->sweep);
        if (w->dev) (void)hipFree(w->dev);
        delete w;
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    w->host.assign(doubles - 4, 0.0);
    f->ob_ws.push_back(w);
    *out = w;
    return 0;
}

}  // namespace

int pnmol_state_observe(pnmol_filter* f, const pnmol_state* in, int q, const double* C_q_ds, const double* y_q,
                        const double* R_sqrtm_qq, pnmol_state* out, pnmol_observe_out* res) {
    static const char* who = "pnmol_state_observe";
    if (res) {
        res->log_likelihood = res->mahalanobis = res->logdet = std::nan("");
        res->info = -1;
    }
    if (!f || !in || !out || !C_q_ds || !y_q || !res || out == in || in->f != f || out->f != f || q < 1 || q > f->ds || f->p32) {
        if (f)
            f->ctx->err = std::string(who) + ": bad argument (null, aliasing, foreign state, q < 1, q > d_state or fp32 filter)";
        return -1;
    }
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int qp = observe_qp(q), dp = f->dp, ds = f->ds;
    const long Dp = f->Dp;
    ObserveWs* w = nullptr;
    int rc = observe_ensure_ws(f, qp, &w);
    if (rc != 0) return rc;

    // H = sc[0] C, R (its lower triangle) and y, padded with zeros: one copy to the device
    double sc[MAXN];
    frame_scales(in, sc);
    double* hH = w->host.data();
    double* hR = hH + (size_t)qp * dp;
    double* hy = hR + (size_t)qp * qp;
    std::fill(w->host.begin(), w->host.end(), 0.0);
    for (int r = 0; r < q; ++r) {
        for (int j = 0; j < ds; ++j) hH[(size_t)r * dp + j] = sc[0] * C_q_ds[(size_t)r * ds + j];
        if (R_sqrtm_qq)
            for (int k = 0; k <= r; ++k) hR[(size_t)r * qp + k] = R_sqrtm_qq[(size_t)r * q + k];
        hy[r] = y_q[r];
    }
    double* dH = w->dev;
    double* dR = dH + (size_t)qp * dp;
    double* dy = dR + (size_t)qp * qp;
    double* dres = dy + qp;
    HIPCHK(ctx, hipMemcpyAsync(dH, hH, sizeof(double) * w->host.size(), hipMemcpyHostToDevice, st));

    const SweepWs& sw = w->sweep;
    double* Gb = sw.G + (size_t)qp * qp;          // rows of B
    double* Gv = sw.G + ((size_t)qp + Dp) * qp;   // the v^T row block
    const unsigned nS = (unsigned)((qp + BM - 1) / BM), nP = (unsigned)((Dp + BM - 1) / BM);
    k_ob_thin<<<dim3(nS, nP), 256, 0, st>>>(in->P, Dp, dp, dH, qp, Gb);
    k_ob_build<<<nS * nS + (unsigned)(qp / 4), 256, 0, st>>>(dH, dp, Gb, R_sqrtm_qq ? dR : nullptr, dy, in->mean, q, qp, (int)nS,
                                                             sw.G, Gv);
    if (hipGetLastError() != hipSuccess) {
        ctx->err = std::string(who) + ": kernel launch failed";
        return -2;
    }
    if ((rc = sweep_ws_enqueue(f, sw, st, 0, who)) != 0) return rc;
    const double* Wm = sw.F + (size_t)qp * qp;
    const double* wv = sw.F + ((size_t)qp + Dp) * qp;
    k_ob_syrk<<<dim3(nP, nP), 256, 0, st>>>(Wm, qp, in->P, out->P, out->var, Dp);
    k_ob_mean<<<(unsigned)((Dp + 3) / 4), 256, 0, st>>>(Wm, wv, in->mean, out->mean, Dp, qp);
    k_ob_scalars<<<1, 256, 0, st>>>(sw.F, wv, q, qp, dres);
    if (hipGetLastError() != hipSuccess) {
        ctx->err = std::string(who) + ": kernel launch failed";
        return -2;
    }
    // the sweep's info word and the three scalars: one stream synchronisation
    int inf = 0;
    double hres[4] = {0.0, 0.0, 0.0, 0.0};
    HIPCHK(ctx, hipMemcpyAsync(&inf, sw.info, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hres, dres, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipGetLastError());
    out->t = in->t;
    out->frame_dt = in->frame_dt;
    rc = sweep_info_result(ctx, inf, qp, who, "innovation matrix not positive definite", "a dependency wait of the sweep timed out");
    if (rc == 0 && hres[2] != 0.0) {
        inf = (int)hres[2] - 1;
        rc = sweep_info_result(ctx, inf, qp, who, "innovation matrix not positive definite");
    }
    if (rc != 0) {
        if (rc == -3) res->info = inf;
        return rc;
    }
    res->mahalanobis = hres[0];
    res->logdet = hres[1];
    res->log_likelihood = -0.5 * (hres[0] + hres[1] + q * std::log(2.0 * 3.14159265358979323846));
    return 0;
}

// ---- sensor data in the constant-step loop ----------------------------------------------------------------------------------------
// The plan (pnmol_observe_plan.hpp holds its host logic) with its device tables: C (qp x dp, unscaled), R (qp x qp), y (nobs x qp),
// the result slots (4 doubles per entry: |w|^2, 2 sum log Ls_ii, bad pivot + 1, the sweep's info word) and their mapped host image.
// qp = 32: the single-workgroup route with its own workspace [Bw (Dp x 32) | W (Dp x 32) | X (32 x 32) | w (32)]; otherwise the
// sweep route in the ObserveWs of that qp.
struct ObservePlanDev {
    ObservePlan plan;
    double *dC = nullptr, *dR = nullptr, *dy = nullptr, *dres = nullptr, *ws = nullptr;
    double *h_res = nullptr, *h_res_dev = nullptr;
};

namespace {

void plan_dev_free(ObservePlanDev* pd) {
    if (!pd) return;
    for (double* p : {pd->dC, pd->dR, pd->dy, pd->dres, pd->ws})
        if (p) (void)hipFree(p);
    if (pd->h_res) (void)hipHostFree(pd->h_res);
    delete pd;
}

// PNMOL_HIP_OBSERVE_SINGLE_WG=1 (read when a plan is set; include/pnmol_hip.h): plans of q <= 32 take the single-workgroup route.
// The default is the sweep route for every q: it measured 0.03 ms faster per update.
bool observe_single_workgroup() {
    const char* e = std::getenv("PNMOL_HIP_OBSERVE_SINGLE_WG");
    return e && std::atoi(e) != 0;
}

int plan_result(pnmol_ctx* ctx, ObservePlan* p, int entry, const double* slot, const char* who) {
    ObservePlanResult& r = p->results[(size_t)entry];
    r = ObservePlanResult{};
    r.applied = true;
    r.mahalanobis = slot[0], r.logdet = slot[1];
    const int inf = (int)slot[3];
    const std::string what = "innovation matrix of entry " + std::to_string(entry) + " not positive definite";
    int rc = sweep_info_result(ctx, inf, p->qp, who, what.c_str(), "a dependency wait of the sweep timed out");
    if (rc == -2) r.stuck = 1;
    if (rc == -3) r.bad_pivot = inf;
    if (rc == 0 && slot[2] != 0.0) {
        r.bad_pivot = (int)slot[2] - 1;
        rc = sweep_info_result(ctx, r.bad_pivot, p->qp, who, what.c_str());
    }
    return rc;
}

void plan_fill_out(const ObservePlan& p, int entry, pnmol_observe_out* o) {
    const ObservePlanResult& r = p.results[(size_t)entry];
    o->log_likelihood = o->mahalanobis = o->logdet = std::nan("");
    o->info = r.bad_pivot;
    if (!r.applied || r.bad_pivot >= 0 || r.stuck) return;
    o->mahalanobis = r.mahalanobis;
    o->logdet = r.logdet;
    o->log_likelihood = -0.5 * (r.mahalanobis + r.logdet + p.q * std::log(2.0 * 3.14159265358979323846));
}

}  // namespace

void pnmol_observe_plan_free(pnmol_filter* f) {
    plan_dev_free(f->ob_plan);
    f->ob_plan = nullptr;
}

bool pnmol_observe_plan_pending(const pnmol_filter* f) { return f->ob_plan && f->ob_plan->plan.pending(); }

const double* pnmol_observe_plan_results_dev(const pnmol_filter* f, double** host_dev, int* first, int* count) {
    if (!f->ob_plan || f->ob_plan->plan.call_count == 0) return nullptr;
    *host_dev = f->ob_plan->h_res_dev, *first = f->ob_plan->plan.next, *count = f->ob_plan->plan.call_count;
    return f->ob_plan->dres;
}

int pnmol_observe_plan_begin(pnmol_filter* f, const pnmol_state* s, int k, double dt, std::vector<int>* entry_of_step) {
    if (!pnmol_observe_plan_pending(f)) {
        entry_of_step->assign((size_t)k, -1);
        if (f->ob_plan) f->ob_plan->plan.call_entry.clear(), f->ob_plan->plan.call_count = 0;
        return 0;
    }
    ObservePlan& p = f->ob_plan->plan;
    std::string err;
    int count = 0;
    if (observe_plan_walk(p, s->t, k, dt, entry_of_step, &count, &err) != 0) {
        f->ctx->err = "pnmol_filter_steps_begin: observation " + err;
        return -1;
    }
    p.call_entry = *entry_of_step;
    p.call_count = count;
    return 0;
}

int pnmol_observe_plan_cursor(const pnmol_filter* f) { return f->ob_plan ? f->ob_plan->plan.next : 0; }

void pnmol_observe_plan_rewind(pnmol_filter* f, int next) {
    if (!f->ob_plan) return;
    ObservePlan& p = f->ob_plan->plan;
    p.next = std::min(std::max(next, 0), p.nobs);
    for (int i = p.next; i < p.nobs; ++i) p.results[(size_t)i] = ObservePlanResult{};
}

void pnmol_observe_plan_abandon(pnmol_filter* f) {
    if (f->ob_plan) f->ob_plan->plan.call_entry.clear(), f->ob_plan->plan.call_count = 0;
}

int pnmol_observe_plan_enqueue(pnmol_filter* f, int entry, double* P, double* mean, double* var, double frame_dt, int rec_slot) {
    static const char* who = "pnmol_filter_steps_begin";
    ObservePlanDev* pd = f->ob_plan;
    const ObservePlan& p = pd->plan;
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    const int q = p.q, qp = p.qp, dp = f->dp;
    const long Dp = f->Dp;
    double sc[MAXN];
    frame_scales(f, frame_dt, sc);
    const double* dy = pd->dy + (size_t)entry * qp;
    double* dres = pd->dres + (size_t)4 * entry;
    const unsigned nP = (unsigned)((Dp + BM - 1) / BM);
    const int* info = nullptr;
    if (qp == QB) {
        double* Bw = pd->ws;
        double* Wm = Bw + (size_t)Dp * QB;
        double* X = Wm + (size_t)Dp * QB;
        double* wv = X + QB * QB;
        k_obq_thin<<<nP, 256, 0, st>>>(P, Dp, dp, pd->dC, sc[0], Bw);
        k_obq_factor<<<1, 256, 0, st>>>(pd->dC, dp, Bw, p.noisy ? pd->dR : nullptr, dy, mean, sc[0], q, X, wv, dres);
        k_obq_gain<<<(unsigned)((Dp + 7) / 8), 256, 0, st>>>(Bw, X, wv, Wm, mean, Dp);
        k_ob_syrk_inplace<<<dim3(nP, nP), 256, 0, st>>>(Wm, QB, P, var, Dp);
    } else {
        ObserveWs* w = nullptr;
        int rc = observe_ensure_ws(f, qp, &w);
        if (rc != 0) return rc;
        const SweepWs& sw = w->sweep;
        double* dH = w->dev;  // (the H block of the workspace; pnmol_state_observe uploads its own image in front of every call)
        double* Gb = sw.G + (size_t)qp * qp;
        double* Gv = sw.G + ((size_t)qp + Dp) * qp;
        const unsigned nS = (unsigned)((qp + BM - 1) / BM);
        const long nH = (long)qp * dp;
        k_ob_scale<<<(unsigned)((nH + 255) / 256), 256, 0, st>>>(pd->dC, sc[0], nH, dH);
        k_ob_thin<<<dim3(nS, nP), 256, 0, st>>>(P, Dp, dp, dH, qp, Gb);
        k_ob_build<<<nS * nS + (unsigned)(qp / 4), 256, 0, st>>>(dH, dp, Gb, p.noisy ? pd->dR : nullptr, dy, mean, q, qp, (int)nS, sw.G,
                                                                 Gv);
        if (hipGetLastError() != hipSuccess) {
            ctx->err = std::string(who) + ": observation kernel launch failed";
            return -2;
        }
        if ((rc = sweep_ws_enqueue(f, sw, st, 0, who)) != 0) return rc;
        const double* Wm = sw.F + (size_t)qp * qp;
        const double* wv = sw.F + ((size_t)qp + Dp) * qp;
        k_ob_syrk_inplace<<<dim3(nP, nP), 256, 0, st>>>(Wm, qp, P, var, Dp);
        k_ob_mean_inplace<<<(unsigned)((Dp + 3) / 4), 256, 0, st>>>(Wm, wv, mean, Dp, qp);
        k_ob_scalars<<<1, 256, 0, st>>>(sw.F, wv, q, qp, dres);
        info = sw.info;
    }
    if (rec_slot >= 0 || info)
        k_ob_finish<<<(unsigned)((f->d + 255) / 256), 256, 0, st>>>(
            mean, var, sc[0], f->d, rec_slot >= 0 ? f->rec_means + (size_t)rec_slot * f->d : nullptr,
            rec_slot >= 0 ? f->rec_stds + (size_t)rec_slot * f->d : nullptr, info, dres);
    if (hipGetLastError() != hipSuccess) {
        ctx->err = std::string(who) + ": observation kernel launch failed";
        return -2;
    }
    return 0;
}

int pnmol_observe_plan_collect(pnmol_filter* f, int* step) {
    *step = -1;
    if (!f->ob_plan) return 0;
    ObservePlan& p = f->ob_plan->plan;
    int rc = 0;
    std::string first_err;
    for (size_t j = 0; j < p.call_entry.size(); ++j) {
        const int e = p.call_entry[j];
        if (e < 0) continue;
        const int r = plan_result(f->ctx, &p, e, f->ob_plan->h_res + (size_t)4 * e, "pnmol_filter_steps_end");
        if (r != 0 && rc == 0) rc = r, *step = (int)j, first_err = f->ctx->err + " (update behind step " + std::to_string(j) + ")";
    }
    observe_plan_advance(&p, p.call_count);
    p.call_entry.clear(), p.call_count = 0;
    if (rc != 0) f->ctx->err = first_err;
    return rc;
}

extern "C" {

int pnmol_filter_set_observations(pnmol_filter* f, int nobs, const double* t_nobs, int q, const double* C_q_ds, const double* R_sqrtm_qq,
                                  const double* y_nobs_q) {
    static const char* who = "pnmol_filter_set_observations";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    if (f->pending_state) {
        ctx->err = std::string(who) + ": a pnmol_filter_steps_begin call is unfinished";
        return -1;
    }
    const bool clears = nobs < 1 || !t_nobs;
    if (!clears && f->p32) {
        ctx->err = std::string(who) + ": an fp32 filter takes no observations";
        return -1;
    }
    const std::string why = observe_plan_validate(nobs, t_nobs, q, f->ds, C_q_ds, R_sqrtm_qq, y_nobs_q);
    if (!why.empty()) {
        ctx->err = std::string(who) + ": " + why;
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier plan's tables may still be read)
    pnmol_observe_plan_free(f);
    if (clears) return 0;
    ObservePlanDev* pd = new ObservePlanDev();
    const int qp = observe_plan_qp(q, observe_single_workgroup()), dp = f->dp;
    observe_plan_fill(&pd->plan, nobs, t_nobs, q, f->ds, dp, qp, C_q_ds, R_sqrtm_qq, y_nobs_q);
    const ObservePlan& p = pd->plan;
    const size_t nres = (size_t)4 * nobs;
    hipError_t e = hipMalloc(&pd->dC, sizeof(double) * p.C.size());
    if (e == hipSuccess) e = hipMalloc(&pd->dR, sizeof(double) * p.R.size());
    if (e == hipSuccess) e = hipMalloc(&pd->dy, sizeof(double) * p.y.size());
    if (e == hipSuccess) e = hipMalloc(&pd->dres, sizeof(double) * nres);
    if (e == hipSuccess && qp == QB) e = hipMalloc(&pd->ws, sizeof(double) * ((size_t)2 * f->Dp * QB + QB * QB + QB));
    if (e == hipSuccess) e = hipHostMalloc(&pd->h_res, sizeof(double) * nres, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&pd->h_res_dev), pd->h_res, 0);
    if (e == hipSuccess) e = hipMemcpy(pd->dC, p.C.data(), sizeof(double) * p.C.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pd->dR, p.R.data(), sizeof(double) * p.R.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pd->dy, p.y.data(), sizeof(double) * p.y.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(pd->dres, 0, sizeof(double) * nres);
    if (e != hipSuccess) {
        ctx->err = std::string(who) + ": " + hipGetErrorString(e);
        plan_dev_free(pd);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    std::memset(pd->h_res, 0, sizeof(double) * nres);
    f->ob_plan = pd;
    if (qp != QB) {  // the sweep route's workspace now, not inside the loop
        ObserveWs* w = nullptr;
        const int rc = observe_ensure_ws(f, qp, &w);
        if (rc != 0) {
            pnmol_observe_plan_free(f);
            return rc;
        }
    }
    return 0;
}

int pnmol_filter_observations_pending(const pnmol_filter* f, int* next, int* nobs) {
    if (!f) return -1;
    if (next) *next = f->ob_plan ? f->ob_plan->plan.next : 0;
    if (nobs) *nobs = f->ob_plan ? f->ob_plan->plan.nobs : 0;
    return 0;
}

int pnmol_filter_observation_results(const pnmol_filter* f, int first, int count, pnmol_observe_out* res) {
    if (!f) return -1;
    const int nobs = f->ob_plan ? f->ob_plan->plan.nobs : 0;
    if (!res || first < 0 || count < 0 || first + count > nobs) {
        f->ctx->err = "pnmol_filter_observation_results: bad argument (null, or entries outside the plan)";
        return -1;
    }
    for (int i = 0; i < count; ++i) {
        if (!f->ob_plan->plan.results[(size_t)(first + i)].applied) {
            f->ctx->err = "pnmol_filter_observation_results: entry " + std::to_string(first + i) + " has not been applied";
            return -1;
        }
        plan_fill_out(f->ob_plan->plan, first + i, &res[i]);
    }
    return 0;
}

int pnmol_state_observe_planned(pnmol_filter* f, pnmol_state* s, int index, pnmol_observe_out* res) {
    static const char* who = "pnmol_state_observe_planned";
    if (res) {
        res->log_likelihood = res->mahalanobis = res->logdet = std::nan("");
        res->info = -1;
    }
    if (!f || !s || !res || s->f != f || !f->ob_plan || index < 0 || index >= f->ob_plan->plan.nobs || f->pending_state) {
        if (f)
            f->ctx->err = std::string(who) + ": bad argument (null, foreign state, no plan, index outside the plan, or an unfinished "
                                             "pnmol_filter_steps_begin)";
        return -1;
    }
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ObservePlanDev* pd = f->ob_plan;
    int rc = pnmol_observe_plan_enqueue(f, index, s->P, s->mean, s->var, s->frame_dt, -1);
    if (rc != 0) return rc;
    k_ob_results_out<<<1, 64, 0, ctx->stream>>>(pd->dres, pd->h_res_dev, index, 1);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    rc = plan_result(ctx, &pd->plan, index, pd->h_res + (size_t)4 * index, who);
    if (index == pd->plan.next) observe_plan_advance(&pd->plan, 1);
    plan_fill_out(pd->plan, index, res);
    return rc;
}

}  // extern "C"
