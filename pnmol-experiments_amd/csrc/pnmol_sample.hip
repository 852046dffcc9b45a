// pnmol_sample.hip -- the joint posterior draws (`pnmol_samples_*`, include/pnmol_hip.h): kernels, then host side.
//
// One backward step of the draw (Matheron's rule), in the Nordsieck frame of the step h, with P = P_k (filtered),
// A = A1 (x) I, Q = Q1 (x) K, C C^T = P (lenient sweep), Gamma_Q = chol(Q1) (x) Gamma:
//     xt = m + s C xi_1,    r = x_{k+1} - A xt - s Gamma_Q xi_2,    x_k = xt + G r,    G = P A^T (P-)^-1
// The gain is never formed: the smoother's sweep [P-; P A^T; 0; I] -> [L; V; 0; T] (T = L^-T) gives G r = V (T^T r), two
// thin products.  This file holds what surrounds the two sweeps (pnmol_hip.hip): the block transform with the frame change
// (k_sp_build; its predict is predict_block of pnmol_tile.hpp, shared with the smoother), the counter-based generator
// (k_sp_noise), the thin product on the fp64 MFMA (k_sp_thin), the n x n mixes (k_sp_resid) and the read-out (k_sp_get).
// Layouts: a sample block is Dp x Sp row-major, row = state component (derivative-major (a, j) -> a*dp + j like a mean),
// column = draw; Sp is a multiple of 64; padding rows and columns are zero.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pnmol_internal.hpp"
#include "pnmol_tile.hpp"

namespace {

// ---- build ----------------------------------------------------------------------------------------------------------------
// P (frame of the filtered state) -> frame of h:
//   Gc:                  P^h in POINT-major order ((a, j) -> j N + a), +1 on the diagonal of the padded points (the lenient
//                        sweep drops what is not positive)
//   Gs rows [0, Dp):     P- = A1 P^h A1^T + Q1 K   (+1 on the diagonal of the padded points)
//   Gs rows [Dp, 2Dp):   P^h A1^T
// (k_sm_build of pnmol_smooth.hip without the smoothed successor; the predict is predict_block of pnmol_tile.hpp)
template <int N>
__global__ __launch_bounds__(256) void k_sp_build(const double* __restrict__ P, const double* __restrict__ Kg, SampleConsts c,
                                                  int d, int dp, double* __restrict__ Gc, double* __restrict__ Gs) {
    const int k = blockIdx.x * 32 + threadIdx.x;
    const int j = blockIdx.y * 8 + threadIdx.y;
    const long Dp = (long)N * dp;
    const bool pad = (j == k && j >= d);
    // The covariance-form recursion leaves rounding noise where the exact covariance is zero (noise-free Dirichlet nodes:
    // a diagonal entry of -3e-27 beside off-diagonal entries of 1e-21 has been seen).  Such a row is not the row of any PSD
    // matrix, and a factor of it would spread its off-diagonal noise over the node.  Every entry is therefore held to
    // the Cauchy-Schwarz bound |P_ij| <= sqrt(P_ii P_jj) of its own diagonal (a negative diagonal entry counts as zero),
    // which changes nothing in a matrix that is PSD.
    double dj[N], dk[N];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        dj[a] = fmax(c.ts[a] * c.ts[a] * P[((long)a * dp + j) * (Dp + 1)], 0.0);
        dk[a] = fmax(c.ts[a] * c.ts[a] * P[((long)a * dp + k) * (Dp + 1)], 0.0);
    }
    double X[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const long idx = ((long)a * dp + j) * Dp + (long)b * dp + k;
            const double v = c.ts[a] * c.ts[b] * P[idx], lim = sqrt(dj[a] * dk[b]);
            X[a][b] = fmin(fmax(v, -lim), lim);
            // (the factor's input is point-major, index j N + a: the order pnmol_state_get_cov_sqrtm factorises in)
            Gc[((long)j * N + a) * Dp + (long)k * N + b] = (pad && a == b) ? 1.0 : X[a][b];
        }
    if (!Gs) return;
    double XA[N][N], Pm[N][N];
    predict_block<N>(X, c.A1, c.Q1, Kg[(long)j * dp + k], XA, Pm);
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            Gs[(Dp + (long)a * dp + j) * Dp + (long)b * dp + k] = XA[a][b];
            Gs[((long)a * dp + j) * Dp + (long)b * dp + k] = (a == b && pad) ? 1.0 : Pm[a][b];
        }
}

// mh = ts m
__global__ __launch_bounds__(256) void k_sp_mean(const double* __restrict__ m, SampleConsts c, int n, int dp,
                                                 double* __restrict__ mh) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n * dp) mh[e] = c.ts[e / dp] * m[e];
}

// ---- generator ------------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with Box-Muller in fp64.
// The map is part of the C ABI (include/pnmol_hip.h, "generator").
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// components 2p and 2p + 1 of draw i
__device__ __forceinline__ void normal_pair(unsigned long long seed, unsigned long long step_index, unsigned i, unsigned p,
                                            double& z0, double& z1) {
    unsigned c[4] = {p, i, (unsigned)step_index, (unsigned)(step_index >> 32)};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    // 52 bits + 1/2: exactly representable, inside (0, 1)
    const double u1 = ((double)(((unsigned long long)(c[1] & 0xFFFFFu) << 32) | c[0]) + 0.5) * 0x1p-52;
    const double u2 = ((double)(((unsigned long long)(c[3] & 0xFFFFFu) << 32) | c[2]) + 0.5) * 0x1p-52;
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    z0 = r * cs, z1 = r * sn;
}

// row of the noise block for column c of the caller's noise: xi_1 (c < D) is the input of the point-major factor as it
// comes (its real columns are the first D); xi_2 is derivative-major with the padding of a mean
__device__ __forceinline__ long noise_row(int c, int d, int dp, int n) {
    const int D = n * d, cc = c - D;
    return c < D ? (long)c : (long)n * dp + (long)(cc / d) * dp + cc % d;
}

// thread -> (pair p, draw i), i fastest
__global__ __launch_bounds__(256) void k_sp_noise(unsigned long long seed, unsigned long long step_index, int rows, int cols,
                                                  int d, int dp, int n, int Sp, double* __restrict__ Xi,
                                                  double* __restrict__ dense) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const int np = (cols + 1) / 2;
    if (e >= (long)rows * np) return;
    const int i = (int)(e % rows), p = (int)(e / rows);
    double z[2];
    normal_pair(seed, step_index, (unsigned)i, (unsigned)p, z[0], z[1]);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = 2 * p + q;
        if (c >= cols) break;
        if (Xi) Xi[noise_row(c, d, dp, n) * Sp + i] = z[q];
        else dense[(long)i * cols + c] = z[q];
    }
}

__global__ __launch_bounds__(256) void k_sp_scatter(const double* __restrict__ stage, int rows, int cols, int d, int dp, int n,
                                                    int Sp, double* __restrict__ Xi) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)rows * cols) return;
    const int i = (int)(e % rows), c = (int)(e / rows);
    Xi[noise_row(c, d, dp, n) * Sp + i] = stage[(long)i * cols + c];
}

// ---- thin product ---------------------------------------------------------------------------------------------------------
// Y = [add] + [addvec 1^T] + alpha op(M) X:  M (rows x rows) against a (rows x Sp) block.  A workgroup owns BR = 16 rows of
// op(M) and a slab of SW columns of X, so M is streamed from memory once per slab (once in all for Sp <= 256); X stays in
// the L2.  Both operands go through LDS in k-steps of BK, the next step's loads in flight while this one is multiplied;
// four waves, wave w takes the 16 x 16 tiles w, w + 4, ... of the slab (v_mfma_f64_16x16x4_f64).
constexpr int BR = 16;
struct ThinArgs {
    const double* M;
    const double* X;
    double* Y;
    const double* add;
    const double* addvec;
    double alpha;
    long rows;
    int Sp, trans, lower;
    int perm_n;  // > 0: op(M)'s rows are point-major (j perm_n + a); the result goes to row a (rows / perm_n) + j
};

template <int SW, int BK>
__global__ __launch_bounds__(256) void k_sp_thin(ThinArgs g) {
    constexpr int LDA = BR + 1, LDB = SW + 4;
    constexpr int AE = BR * BK / 256;  // elements of the M block per thread
    constexpr int BE = BK * SW / 1024;  // 4-element groups of the X block per thread
    constexpr int TPW = SW / 64;        // output tiles per wave
    static_assert(AE >= 1 && BE >= 1, "block too small for 256 threads");
    __shared__ __attribute__((aligned(16))) double sA[BK * LDA];  // [k][row]
    __shared__ __attribute__((aligned(16))) double sB[BK * LDB];  // [k][col]
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const long n = g.rows, r0 = (long)blockIdx.x * BR;
    const int c0 = blockIdx.y * SW, Sp = g.Sp;
    const long boff = (long)blockIdx.z * n * Sp;
    const double* __restrict__ M = g.M;
    const double* __restrict__ X = g.X + boff;
    const long kend = g.lower ? ((r0 + BR + BK - 1) / BK) * BK : n;  // (rows is a multiple of 32 >= BK's granularity)

    double va[AE];
    double vb[BE][4];
    auto load = [&](long k0) {
#pragma unroll
        for (int q = 0; q < AE; ++q) {
            const int e = tid + 256 * q;
            long i, k;  // element (row i, column k) of op(M)
            if (g.trans) i = r0 + (e % BR), k = k0 + e / BR;   // M[k][i]: 16 consecutive doubles per k
            else i = r0 + e / BK, k = k0 + (e % BK);           // M[i][k]: BK consecutive doubles per row
            double v = 0.0;
            if (k < n && !(g.lower && k > i)) v = g.trans ? M[k * n + i] : M[i * n + k];
            va[q] = v;
        }
#pragma unroll
        for (int q = 0; q < BE; ++q) {
            const int e = tid + 256 * q;
            const long k = k0 + e / (SW / 4);
            const int c = c0 + 4 * (e % (SW / 4));
            if (k < n && c < Sp) {
                const double2* p = reinterpret_cast<const double2*>(X + k * Sp + c);
                const double2 a = p[0], b = p[1];
                vb[q][0] = a.x, vb[q][1] = a.y, vb[q][2] = b.x, vb[q][3] = b.y;
            } else {
                vb[q][0] = vb[q][1] = vb[q][2] = vb[q][3] = 0.0;
            }
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int q = 0; q < AE; ++q) {
            const int e = tid + 256 * q;
            if (g.trans) sA[(e / BR) * LDA + (e % BR)] = va[q];
            else sA[(e % BK) * LDA + e / BK] = va[q];
        }
#pragma unroll
        for (int q = 0; q < BE; ++q) {
            const int e = tid + 256 * q;
            double* s = sB + (e / (SW / 4)) * LDB + 4 * (e % (SW / 4));
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = vb[q][t];
        }
    };

    d4 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t] = d4{0, 0, 0, 0};
    load(0);
    for (long k0 = 0; k0 < kend; k0 += BK) {
        __syncthreads();
        put();
        __syncthreads();
        if (k0 + BK < kend) load(k0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const int kr = kk + (l >> 4);
            const double a = sA[kr * LDA + (l & 15)];
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const double b = sB[kr * LDB + (w + 4 * t) * 16 + (l & 15)];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
    }
    // the accumulators are read behind the loop's exit branch: wait states by hand (as in tile_product of pnmol_tile.hpp;
    // tests/test_isa_hazards.py scans this file)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int col = c0 + (w + 4 * t) * 16 + (l & 15);
        if (col >= Sp) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            long row = r0 + (l >> 4) + 4 * r;
            if (g.perm_n > 0) row = (row % g.perm_n) * (n / g.perm_n) + row / g.perm_n;
            double v = g.alpha * acc[t][r];
            if (g.add) v += g.add[boff + row * Sp + col];
            if (g.addvec) v += g.addvec[(long)blockIdx.z * n + row];
            g.Y[boff + row * Sp + col] = v;
        }
    }
}

// ---- small block operations -----------------------------------------------------------------------------------------------
// R = tsn x_next - A1 xt - scale Lq W   (thread -> point j, draw i)
template <int N>
__global__ __launch_bounds__(256) void k_sp_resid(SampleConsts c, double scale, int dp, int Sp, const double* __restrict__ xnext,
                                                  const double* __restrict__ xt, const double* __restrict__ W,
                                                  double* __restrict__ R) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long per = (long)dp * Sp;
    if (e >= per) return;
    double x[N], wv[N];
#pragma unroll
    for (int a = 0; a < N; ++a) x[a] = xt[a * per + e], wv[a] = W[a * per + e];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double s = c.tsn[a] * xnext[a * per + e];
#pragma unroll
        for (int b = 0; b < N; ++b) s -= c.A1[a * SM_MAXN + b] * x[b];
#pragma unroll
        for (int b = 0; b < N; ++b)
            if (b <= a) s -= scale * c.Lq[a * SM_MAXN + b] * wv[b];
        R[a * per + e] = s;
    }
}

struct Scales {
    double sc[SM_MAXN];
};
__global__ __launch_bounds__(256) void k_sp_get(int n, int d, int dp, int Sp, int S, Scales sc, const double* __restrict__ X,
                                                double* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long D = (long)n * d;
    if (e >= D * S) return;
    const int i = (int)(e % S);  // draws fastest: coalesced reads
    const long c = e / S;
    const int a = (int)(c / d), j = (int)(c % d);
    out[(long)i * D + c] = sc.sc[a] * X[((long)a * dp + j) * Sp + i];
}

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -2; }

// Gc = P^h, point-major, with unit pivots on the padded points (input of the lenient sweep), Gs (may be null) = [P-; P^h A^T], mh = m^h
int launch_build(hipStream_t st, int n, const double* P, const double* m, const double* Kg, const SampleConsts& c,
                              int d, int dp, double* Gc, double* Gs, double* mh) {
    const dim3 grid(dp / 32, dp / 8), blk(32, 8);
    switch (n) {
        case 2: k_sp_build<2><<<grid, blk, 0, st>>>(P, Kg, c, d, dp, Gc, Gs); break;
        case 3: k_sp_build<3><<<grid, blk, 0, st>>>(P, Kg, c, d, dp, Gc, Gs); break;
        case 4: k_sp_build<4><<<grid, blk, 0, st>>>(P, Kg, c, d, dp, Gc, Gs); break;
        default: return -1;
    }
    k_sp_mean<<<(n * dp + 255) / 256, 256, 0, st>>>(m, c, n, dp, mh);
    return launched();
}

// standard normals of (seed, step_index) for `rows` draws x `cols` components: into the noise block Xi (component c < D ->
// row c, the input of the point-major factor; c >= D -> row Dp + ((c - D) / d) dp + (c - D) % d), or, Xi == null, into dense (rows, cols) row-major.
// n = 0: every component is placed derivative-major, c -> row (c / d) dp + c % d of Xi (the noise of pnmol_samples_interpolate)
int launch_noise(hipStream_t st, unsigned long long seed, unsigned long long step_index, int rows, int cols, int d,
                              int dp, int n, int Sp, double* Xi, double* dense) {
    const long work = (long)rows * ((cols + 1) / 2);
    k_sp_noise<<<(unsigned)((work + 255) / 256), 256, 0, st>>>(seed, step_index, rows, cols, d, dp, n, Sp, Xi, dense);
    return launched();
}

// the same placement for host-supplied noise: stage (rows, cols) row-major on the device -> Xi
int launch_scatter(hipStream_t st, const double* stage, int rows, int cols, int d, int dp, int n, int Sp, double* Xi) {
    const long work = (long)rows * cols;
    k_sp_scatter<<<(unsigned)((work + 255) / 256), 256, 0, st>>>(stage, rows, cols, d, dp, n, Sp, Xi);
    return launched();
}

// Y = [add] + [addvec 1^T] + alpha op(M) X for `batch` stacked (rows x Sp) blocks of X / Y (M rows x rows, row-major, the same
// for every block).  trans: op(M) = M^T; lower: op(M) is lower triangular (what lies above the diagonal is not read);
// perm_n > 0: the rows of op(M) are point-major (j perm_n + a) and the result is stored derivative-major.
int launch_thin(hipStream_t st, const double* M, const double* X, double* Y, const double* add, const double* addvec,
                             double alpha, long rows, int Sp, int trans, int lower, int batch, int perm_n) {
    const ThinArgs g{M, X, Y, add, addvec, alpha, rows, Sp, trans, lower, perm_n};
    if (Sp <= 64) k_sp_thin<64, 32><<<dim3((unsigned)(rows / BR), 1, (unsigned)batch), 256, 0, st>>>(g);
    else k_sp_thin<256, 16><<<dim3((unsigned)(rows / BR), (unsigned)((Sp + 255) / 256), (unsigned)batch), 256, 0, st>>>(g);
    return launched();
}

// R = tsn x_next - A1 xt - scale Lq W  (n x n mixes of the derivative blocks, elementwise over points and draws)
int launch_resid(hipStream_t st, int n, const SampleConsts& c, double scale, int dp, int Sp, const double* xnext,
                              const double* xt, const double* W, double* R) {
    const unsigned grid = (unsigned)(((long)dp * Sp + 255) / 256);
    switch (n) {
        case 2: k_sp_resid<2><<<grid, 256, 0, st>>>(c, scale, dp, Sp, xnext, xt, W, R); break;
        case 3: k_sp_resid<3><<<grid, 256, 0, st>>>(c, scale, dp, Sp, xnext, xt, W, R); break;
        case 4: k_sp_resid<4><<<grid, 256, 0, st>>>(c, scale, dp, Sp, xnext, xt, W, R); break;
        default: return -1;
    }
    return launched();
}

// out (S, n, d) row-major = sc[a] X[(a dp + j) Sp + i]
int launch_get(hipStream_t st, int n, int d, int dp, int Sp, int S, const double* sc, const double* X, double* out) {
    Scales s{};
    for (int a = 0; a < n; ++a) s.sc[a] = sc[a];
    const long work = (long)n * d * S;
    k_sp_get<<<(unsigned)((work + 255) / 256), 256, 0, st>>>(n, d, dp, Sp, S, s, X, out);
    return launched();
}

// the noise of a call into Xi, laid out for n (see launch_noise): host-supplied (rows of `cols` components) or generated on the device
int fill_noise(pnmol_samples* x, double* Xi, int n, const double* xi, int cols, unsigned long long seed, unsigned long long step_index,
               const char* who) {
    pnmol_filter* f = x->f;
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    int rc;
    if (xi) {
        HIPCHK(ctx, hipMemcpyAsync(x->stage, xi, sizeof(double) * (size_t)x->S * cols, hipMemcpyHostToDevice, st));
        rc = launch_scatter(st, x->stage, x->S, cols, f->d, f->dp, n, x->Sp, Xi);
    } else {
        rc = launch_noise(st, seed, step_index, x->S, cols, f->d, f->dp, n, x->Sp, Xi, nullptr);
    }
    if (rc != 0) ctx->err = std::string(who) + ": kernel launch failed";
    return rc;
}

// Allocated on first use: the square lenient sweep P^h -> C (dropped-pivot rule of pnmol_state_get_cov_sqrtm), Gamma (dp x dp,
// from the host copy kept at creation), m^h (Dp), and the side stream of a backward step with its two events.
int ensure_sampler_ws(pnmol_filter* f, const char* who) {
    if (f->sp_sweep.G) return 0;
    pnmol_ctx* ctx = f->ctx;
    const int cb = (int)(f->Dp / NB);
    const size_t gq = (size_t)f->dp * f->dp;
    hipError_t e = sweep_ws_alloc(&f->sp_sweep, ctx, cb, cb);
    if (e == hipSuccess) e = hipMalloc(&f->sp_Gamma, sizeof(double) * gq);
    if (e == hipSuccess) e = hipMalloc(&f->sp_mh, sizeof(double) * (size_t)f->Dp);
    if (e == hipSuccess) e = hipMemcpy(f->sp_Gamma, f->hGamma.data(), sizeof(double) * gq, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->sp_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->sp_ev_built, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->sp_ev_swept, hipEventDisableTiming);
    if (e != hipSuccess) {
        ctx->err = std::string(who) + ": workspace: " + hipGetErrorString(e);
        pnmol_sample_free_ws(f);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    return 0;
}

// the info word(s) of the call's sweep(s): one stream synchronisation
int finish_sampler_call(pnmol_filter* f, bool main_sweep, const char* who) {
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    static const char* wait = "a dependency wait of the sweep timed out";
    int inf_c = 0, inf_m = 0x7f7f7f7f;
    HIPCHK(ctx, hipMemcpyAsync(&inf_c, f->sp_sweep.info, sizeof(int), hipMemcpyDeviceToHost, st));
    if (main_sweep) HIPCHK(ctx, hipMemcpyAsync(&inf_m, f->sm_sweep.info, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipGetLastError());
    // (a timeout of either sweep is reported before a pivot of the first)
    int rc = sweep_info_result(ctx, inf_m == -2 ? -2 : inf_c, f->Dp, who, "covariance not positive semi-definite (NaN?)", wait);
    if (rc == 0) rc = sweep_info_result(ctx, inf_m, f->Dp, who, "predicted covariance not positive definite", wait);
    return rc;
}

}  // namespace

void pnmol_sample_free_ws(pnmol_filter* f) {
    sweep_ws_free(&f->sp_sweep);
    if (f->sp_Gamma) (void)hipFree(f->sp_Gamma);
    if (f->sp_mh) (void)hipFree(f->sp_mh);
    f->sp_Gamma = f->sp_mh = nullptr;
    if (f->sp_ev_built) (void)hipEventDestroy(f->sp_ev_built);
    if (f->sp_ev_swept) (void)hipEventDestroy(f->sp_ev_swept);
    if (f->sp_stream) (void)hipStreamDestroy(f->sp_stream);
    f->sp_ev_built = f->sp_ev_swept = nullptr;
    f->sp_stream = nullptr;
}

// ---- joint posterior draws ---------------------------------------------------------------------------------------------
int pnmol_samples_create(pnmol_filter* f, int num_samples, pnmol_samples** out) {
    if (out) *out = nullptr;
    if (!f || !out || num_samples < 1 || f->ds != f->d || f->p32) {
        if (f) f->ctx->err = "pnmol_samples_create: bad argument (null, num_samples < 1, latent-force or fp32 filter)";
        return -1;
    }
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pnmol_samples* x = new pnmol_samples();
    x->f = f;
    x->S = num_samples;
    x->Sp = round_up(num_samples, 64);
    f->samples.fetch_add(1);
    const size_t blk = sizeof(double) * (size_t)f->Dp * x->Sp;
    const size_t D = (size_t)f->n * f->d;
    hipError_t e = hipMalloc(&x->X, blk);
    if (e == hipSuccess) e = hipMalloc(&x->Xi, 2 * blk);
    if (e == hipSuccess) e = hipMalloc(&x->Xt, blk);
    if (e == hipSuccess) e = hipMalloc(&x->R, blk);
    if (e == hipSuccess) e = hipMalloc(&x->Y, blk);
    if (e == hipSuccess) e = hipMalloc(&x->stage, sizeof(double) * (size_t)x->S * 2 * D);
    // (on the ctx stream, like pnmol_state_create; the padding rows and columns of the noise are never written again)
    if (e == hipSuccess) e = hipMemsetAsync(x->X, 0, blk, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(x->Xi, 0, 2 * blk, ctx->stream);
    if (e != hipSuccess) {
        ctx->err = std::string("pnmol_samples_create: ") + hipGetErrorString(e);
        pnmol_samples_destroy(x);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    *out = x;
    return 0;
}

int pnmol_samples_destroy(pnmol_samples* x) {
    if (!x) return -1;
    x->f->samples.fetch_sub(1);
    hipSetDevice(x->f->ctx->device);
    for (void* p : {(void*)x->X, (void*)x->Xi, (void*)x->Xt, (void*)x->R, (void*)x->Y, (void*)x->stage})
        if (p) (void)hipFree(p);
    delete x;
    return 0;
}

int pnmol_samples_draw(pnmol_samples* x, const pnmol_state* s, const double* xi_SD, unsigned long long seed,
                       unsigned long long step_index, double scale) {
    static const char* who = "pnmol_samples_draw";
    if (!x || !s || s->f != x->f || !std::isfinite(scale)) {
        if (x) x->f->ctx->err = std::string(who) + ": bad argument (null, state of another filter, non-finite scale)";
        return -1;
    }
    pnmol_filter* f = x->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = ensure_sampler_ws(f, who);
    if (rc != 0) return rc;
    x->drawn = false;
    const long Dp = f->Dp;
    SampleConsts c{};
    for (int a = 0; a < f->n; ++a) c.ts[a] = 1.0;  // the draw stays in the state's own frame
    rc = launch_build(st, f->n, s->P, s->mean, f->Kg, c, f->d, f->dp, f->sp_sweep.G, nullptr, f->sp_mh);
    if (rc != 0) {
        ctx->err = std::string(who) + ": kernel launch failed";
        return rc;
    }
    if ((rc = sweep_ws_enqueue(f, f->sp_sweep, st, 1, who)) != 0) return rc;
    if ((rc = fill_noise(x, x->Xi, f->n, xi_SD, f->n * f->d, seed, step_index, who)) != 0) return rc;
    // x = m + scale C xi
    rc = launch_thin(st, f->sp_sweep.F, x->Xi, x->X, nullptr, f->sp_mh, scale, Dp, x->Sp, 0, 1, 1, f->n);
    if (rc != 0) {
        ctx->err = std::string(who) + ": kernel launch failed";
        return rc;
    }
    if ((rc = finish_sampler_call(f, false, who)) != 0) return rc;
    x->t = s->t, x->frame_dt = s->frame_dt, x->drawn = true;
    return 0;
}

int pnmol_samples_step_back(pnmol_samples* x, const pnmol_state* filt_k, double dt, const double* xi_S2D,
                            unsigned long long seed, unsigned long long step_index, double scale) {
    static const char* who = "pnmol_samples_step_back";
    if (!x || !filt_k || filt_k->f != x->f || !(dt > 0.0) || !std::isfinite(dt) || !std::isfinite(scale) || !x->drawn) {
        if (x)
            x->f->ctx->err = std::string(who) + ": bad argument (null, state of another filter, dt <= 0, non-finite scale, or a "
                                                "block that holds no draw yet)";
        return -1;
    }
    pnmol_filter* f = x->f;
    pnmol_ctx* ctx = f->ctx;
    if (const double tn = filt_k->t + dt; !times_agree(tn, x->t, dt)) {
        ctx->err = std::string(who) + ": the block holds draws at t = " + std::to_string(x->t) + ", not at filt_k->t + dt = " +
                   std::to_string(tn) + " (steps out of order?)";
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = ensure_sampler_ws(f, who);
    if (rc == 0) rc = pnmol_smooth_ensure_ws(f);
    if (rc != 0) return rc;
    const long Dp = f->Dp;
    const int Sp = x->Sp;
    SampleConsts c{};
    std::memcpy(c.A1, f->iwp.A1, sizeof(c.A1));
    std::memcpy(c.Q1, f->iwp.Q1, sizeof(c.Q1));
    small_cholesky(f->n, c.Q1, c.Lq);  // (positive definite)
    for (int a = 0; a < f->n; ++a) {
        c.ts[a] = frame_ratio(f, a, filt_k->frame_dt, dt);
        c.tsn[a] = frame_ratio(f, a, x->frame_dt, dt);
    }
    auto failed = [&](int code) {
        ctx->err = std::string(who) + ": kernel launch failed";
        x->drawn = false;  // the block may be half written
        if (f->sp_stream) (void)hipStreamSynchronize(f->sp_stream);  // (nothing of this call may outlive it)
        return code;
    };
    // C_k sweep -> xt, r -> main sweep -> V (T^T r)
    rc = launch_build(st, f->n, filt_k->P, filt_k->mean, f->Kg, c, f->d, f->dp, f->sp_sweep.G, f->sm_sweep.G, f->sp_mh);
    if (rc != 0) return failed(rc);
    // The main sweep needs nothing of what follows on the ctx stream before `T^T r`.  Where both sweeps are the left-looking
    // kernel (more than 17 column blocks; its workgroups wait for earlier-dispatched ones of their own launch only, so two
    // launches in flight cannot block each other) it runs beside the factorisation of P^h; the register-resident kernel of
    // the small problems wants its workgroups co-resident and stays in line.
    const bool beside = f->sm_sweep.left_looking;
    hipStream_t sw = beside ? f->sp_stream : st;
    if (beside) {
        HIPCHK(ctx, hipEventRecord(f->sp_ev_built, st));
        HIPCHK(ctx, hipStreamWaitEvent(sw, f->sp_ev_built, 0));
        if ((rc = sweep_ws_enqueue(f, f->sm_sweep, sw, 0, who)) != 0) return rc;
        HIPCHK(ctx, hipEventRecord(f->sp_ev_swept, sw));
    }
    if ((rc = sweep_ws_enqueue(f, f->sp_sweep, st, 1, who)) != 0) return rc;
    if ((rc = fill_noise(x, x->Xi, f->n, xi_S2D, 2 * f->n * f->d, seed, step_index, who)) != 0) return rc;
    rc = launch_thin(st, f->sp_sweep.F, x->Xi, x->Xt, nullptr, f->sp_mh, scale, Dp, Sp, 0, 1, 1, f->n);  // xt = m^h + s C xi_1
    if (rc == 0) rc = launch_thin(st, f->sp_Gamma, x->Xi + Dp * Sp, x->R, nullptr, nullptr, 1.0, f->dp, Sp, 0, 1, f->n, 0);
    if (rc == 0) rc = launch_resid(st, f->n, c, scale, f->dp, Sp, x->X, x->Xt, x->R, x->Y);
    if (rc != 0) return failed(rc);
    if (beside) HIPCHK(ctx, hipStreamWaitEvent(st, f->sp_ev_swept, 0));
    else if ((rc = sweep_ws_enqueue(f, f->sm_sweep, st, 0, who)) != 0) return rc;
    const double* V = f->sm_sweep.F + Dp * Dp;
    const double* T = f->sm_sweep.F + (2 * Dp + NB) * Dp;
    rc = launch_thin(st, T, x->Y, x->R, nullptr, nullptr, 1.0, Dp, Sp, 1, 1, 1, 0);        // y = T^T r = L^-1 r
    if (rc == 0) rc = launch_thin(st, V, x->R, x->X, x->Xt, nullptr, 1.0, Dp, Sp, 0, 0, 1, 0);  // x = xt + V y
    if (rc != 0) return failed(rc);
    x->drawn = false;
    if ((rc = finish_sampler_call(f, true, who)) != 0) return rc;
    x->t = filt_k->t, x->frame_dt = dt, x->drawn = true;
    return 0;
}

int pnmol_samples_clone(const pnmol_samples* x, pnmol_samples** out) {
    if (out) *out = nullptr;
    if (!x || !out) return -1;
    int rc = pnmol_samples_create(x->f, x->S, out);
    if (rc != 0) return rc;
    pnmol_ctx* ctx = x->f->ctx;
    pnmol_samples* o = *out;
    HIPCHK(ctx, hipMemcpyAsync(o->X, x->X, sizeof(double) * (size_t)x->f->Dp * x->Sp, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    o->t = x->t, o->frame_dt = x->frame_dt, o->drawn = x->drawn;
    return 0;
}

int pnmol_samples_interpolate(pnmol_samples* out, const pnmol_samples* left, const pnmol_samples* right, double t,
                              const double* xi_SD, unsigned long long seed, unsigned long long step_index, double scale) {
    static const char* who = "pnmol_samples_interpolate";
    if (!out || !left || out == left || out == right || left->f != out->f || (right && right->f != out->f) || left->S != out->S ||
        (right && right->S != out->S) || !left->drawn || (right && !right->drawn) || !std::isfinite(scale) || !std::isfinite(t) ||
        !(t > left->t) || (right && !(t < right->t))) {
        if (out)
            out->f->ctx->err = std::string(who) + ": bad argument (null, aliasing blocks, blocks of another filter or size, a block "
                                                  "that holds no draw, non-finite scale, or t not strictly between the blocks' times)";
        return -1;
    }
    pnmol_filter* f = out->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int rc = ensure_sampler_ws(f, who);
    if (rc != 0) return rc;
    // frame of h = t_r - t_l (two-sided) or of h = t - t_l (one-sided: the prior carried forwards, B+ = 0, Qb = Q1)
    const double h = (right ? right->t : t) - left->t;
    DenseDrawMix c{};
    double Bm[MAXN * MAXN] = {0}, Bp[MAXN * MAXN] = {0}, Qb[MAXN * MAXN] = {0};
    if (right) {
        bridge_coefficients(f, (t - left->t) / h, Bm, Bp, Qb);
    } else {
        std::memcpy(Bm, f->iwp.A1, sizeof(Bm));
        std::memcpy(Qb, f->iwp.Q1, sizeof(Qb));
    }
    small_cholesky(f->n, Qb, c.Ls, true);  // (chol(Qb), positive semi-definite)
    for (int a = 0; a < f->n; ++a)
        for (int b = 0; b < f->n; ++b) {
            c.BmS[a * MAXN + b] = Bm[a * MAXN + b] * frame_ratio(f, b, left->frame_dt, h);
            if (right) c.BpS[a * MAXN + b] = Bp[a * MAXN + b] * frame_ratio(f, b, right->frame_dt, h);
            c.Ls[a * MAXN + b] *= scale;
        }
    out->drawn = false;
    const long Dp = f->Dp;
    const int Sp = out->Sp, D = f->n * f->d;
    double* Xi2 = out->Xi + Dp * Sp;  // derivative-major noise rows (the xi_2 half of the block's noise buffer)
    if ((rc = fill_noise(out, Xi2, 0, xi_SD, D, seed, step_index, who)) != 0) return rc;
    rc = launch_thin(st, f->sp_Gamma, Xi2, out->R, nullptr, nullptr, 1.0, f->dp, Sp, 0, 1, f->n, 0);
    if (rc == 0) rc = pnmol_dense_launch_draw_mix(st, f->n, c, f->dp, Sp, left->X, right ? right->X : nullptr, out->R, out->X);
    if (rc != 0) {
        ctx->err = std::string(who) + ": kernel launch failed";
        return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipGetLastError());
    out->t = t, out->frame_dt = h, out->drawn = true;
    return 0;
}

int pnmol_samples_get(const pnmol_samples* x, double* x_Snd) {
    if (!x || !x_Snd || !x->drawn) {
        if (x) x->f->ctx->err = "pnmol_samples_get: bad argument (null, or a block that holds no draw)";
        return -1;
    }
    pnmol_filter* f = x->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double sc[MAXN];
    frame_scales(f, x->frame_dt, sc);
    if (launch_get(ctx->stream, f->n, f->d, f->dp, x->Sp, x->S, sc, x->X, x->stage) != 0) {
        ctx->err = "pnmol_samples_get: kernel launch failed";
        return -2;
    }
    HIPCHK(ctx, hipMemcpyAsync(x_Snd, x->stage, sizeof(double) * (size_t)x->S * f->n * f->d, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int pnmol_samples_get_time(const pnmol_samples* x, double* t) {
    if (!x || !t || !x->drawn) return -1;
    *t = x->t;
    return 0;
}

int pnmol_sample_noise(pnmol_ctx* ctx, unsigned long long seed, unsigned long long step_index, int rows, int cols, double* out) {
    if (!ctx || !out || rows < 1 || cols < 1) {
        if (ctx) ctx->err = "pnmol_sample_noise: bad argument";
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double* dev = nullptr;
    const size_t bytes = sizeof(double) * (size_t)rows * cols;
    hipError_t e = hipMalloc(&dev, bytes);
    if (e != hipSuccess) {
        ctx->err = std::string("pnmol_sample_noise: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    int rc = launch_noise(ctx->stream, seed, step_index, rows, cols, 1, 1, 1, 0, nullptr, dev);
    if (rc == 0) e = hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (rc == 0 && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(dev);
    if (rc != 0 || e != hipSuccess) {
        ctx->err = std::string("pnmol_sample_noise: ") + (rc != 0 ? "kernel launch failed" : hipGetErrorString(e));
        return -2;
    }
    return 0;
}
