// pnmol_sample.hip -- kernels of the joint posterior draws (`pnmol_samples_*`, include/pnmol_hip.h).
//
// One backward step of the draw (Matheron's rule), in the Nordsieck frame of the step h, with P = P_k (filtered),
// A = A1 (x) I, Q = Q1 (x) K, C C^T = P (lenient sweep), Gamma_Q = chol(Q1) (x) Gamma:
//     xt = m + s C xi_1,    r = x_{k+1} - A xt - s Gamma_Q xi_2,    x_k = xt + G r,    G = P A^T (P-)^-1
// The gain is never formed: the smoother's sweep [P-; P A^T; 0; I] -> [L; V; 0; T] (T = L^-T) gives G r = V (T^T r), two
// thin products.  This file holds what surrounds the two sweeps (pnmol_hip.hip): the block transform with the frame change
// (k_sp_build), the counter-based generator (k_sp_noise), the thin product on the fp64 MFMA (k_sp_thin), the n x n mixes
// (k_sp_resid) and the read-out (k_sp_get).
// Layouts: a sample block is Dp x Sp row-major, row = state component (derivative-major (a, j) -> a*dp + j like a mean),
// column = draw; Sp is a multiple of 64; padding rows and columns are zero.
#include <hip/hip_runtime.h>

#include "pnmol_internal.hpp"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

// ---- build ----------------------------------------------------------------------------------------------------------------
// P (frame of the filtered state) -> frame of h:
//   Gc:                  P^h in POINT-major order ((a, j) -> j N + a), +1 on the diagonal of the padded points (the lenient
//                        sweep drops what is not positive)
//   Gs rows [0, Dp):     P- = A1 P^h A1^T + Q1 K   (+1 on the diagonal of the padded points)
//   Gs rows [Dp, 2Dp):   P^h A1^T
// (k_sm_build of pnmol_smooth.hip without the smoothed successor)
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
    const double kjk = Kg[(long)j * dp + k];
    double XA[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double s = 0.0;
#pragma unroll
            for (int e = 0; e < N; ++e) s += X[a][e] * c.A1[b * SM_MAXN + e];
            XA[a][b] = s;
            Gs[(Dp + (long)a * dp + j) * Dp + (long)b * dp + k] = s;
        }
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double s = c.Q1[a * SM_MAXN + b] * kjk;
#pragma unroll
            for (int e = 0; e < N; ++e) s += c.A1[a * SM_MAXN + e] * XA[e][b];
            if (a == b && pad) s = 1.0;
            Gs[((long)a * dp + j) * Dp + (long)b * dp + k] = s;
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
    // the accumulators are read behind the loop's exit branch: wait states by hand (as in pnmol_smooth.hip's gemm_pass;
    // tests/test_sample_isa_hazards.py scans this file)
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

}  // namespace

int pnmol_sample_launch_build(hipStream_t st, int n, const double* P, const double* m, const double* Kg, const SampleConsts& c,
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

int pnmol_sample_launch_noise(hipStream_t st, unsigned long long seed, unsigned long long step_index, int rows, int cols, int d,
                              int dp, int n, int Sp, double* Xi, double* dense) {
    const long work = (long)rows * ((cols + 1) / 2);
    k_sp_noise<<<(unsigned)((work + 255) / 256), 256, 0, st>>>(seed, step_index, rows, cols, d, dp, n, Sp, Xi, dense);
    return launched();
}

int pnmol_sample_launch_scatter(hipStream_t st, const double* stage, int rows, int cols, int d, int dp, int n, int Sp, double* Xi) {
    const long work = (long)rows * cols;
    k_sp_scatter<<<(unsigned)((work + 255) / 256), 256, 0, st>>>(stage, rows, cols, d, dp, n, Sp, Xi);
    return launched();
}

int pnmol_sample_launch_thin(hipStream_t st, const double* M, const double* X, double* Y, const double* add, const double* addvec,
                             double alpha, long rows, int Sp, int trans, int lower, int batch, int perm_n) {
    const ThinArgs g{M, X, Y, add, addvec, alpha, rows, Sp, trans, lower, perm_n};
    if (Sp <= 64) k_sp_thin<64, 32><<<dim3((unsigned)(rows / BR), 1, (unsigned)batch), 256, 0, st>>>(g);
    else k_sp_thin<256, 16><<<dim3((unsigned)(rows / BR), (unsigned)((Sp + 255) / 256), (unsigned)batch), 256, 0, st>>>(g);
    return launched();
}

int pnmol_sample_launch_resid(hipStream_t st, int n, const SampleConsts& c, double scale, int dp, int Sp, const double* xnext,
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

int pnmol_sample_launch_get(hipStream_t st, int n, int d, int dp, int Sp, int S, const double* sc, const double* X, double* out) {
    Scales s{};
    for (int a = 0; a < n; ++a) s.sc[a] = sc[a];
    const long work = (long)n * d * S;
    k_sp_get<<<(unsigned)((work + 255) / 256), 256, 0, st>>>(n, d, dp, Sp, S, s, X, out);
    return launched();
}
