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
__global__ __launch_bounds__(256) void k_ob_syrk(const double* __restrict__ W, int qp, const double* __restrict__ Pin,
                                                 double* __restrict__ Pout, double* __restrict__ var, long Dp) {
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

// mout = m + W w: one wave per row
__global__ __launch_bounds__(256) void k_ob_mean(const double* __restrict__ W, const double* __restrict__ wv,
                                                 const double* __restrict__ m, double* __restrict__ mout, long Dp, int qp) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (row >= Dp) return;
    double s = 0.0;
    for (int i = l; i < qp; i += 64) s += W[row * qp + i] * wv[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0) mout[row] = m[row] + s;
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
