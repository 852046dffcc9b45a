// Private to the library, device-only: what the kernels behind the forward step (pnmol_smooth.hip, pnmol_sample.hip,
// pnmol_dense.hip, pnmol_observe.hip) share -- the LDS-staged fp64 MFMA product of one 64 x 64 output tile with its epilogue
// walk, and the n x n block predict of one pair of mesh points.  Everything is __device__ __forceinline__ in the unnamed
// namespace (as IwpConsts in pnmol_internal.hpp): no symbol of its own.
#pragma once
#include <hip/hip_runtime.h>

#include "pnmol_internal.hpp"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int BM = 64;       // output tile (rows = cols)
constexpr int BK = 16;       // K step staged in LDS
constexpr int LDT = BM + 2;  // LDS row pitch of a k-major operand tile (doubles)

// a 64 x 16 block of X (rows r0.., cols k0.., row pitch ld; rows >= nrows read as zero): thread -> row tid / 4, four consecutive k
__device__ __forceinline__ void stage_rows(const double* __restrict__ X, long ld, long nrows, long r0, long k0, double (&v)[4],
                                           int tid) {
    const long r = r0 + (tid >> 2);
    const long k = k0 + 4 * (tid & 3);
    if (r < nrows) {
        const double2* p = reinterpret_cast<const double2*>(X + r * ld + k);
        const double2 a = p[0], b = p[1];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else {
        v[0] = v[1] = v[2] = v[3] = 0.0;
    }
}
// a 16 x 64 block of X (rows k0.., cols c0..; cols >= ncols read as zero): thread -> row tid / 16, four consecutive columns
__device__ __forceinline__ void stage_cols(const double* __restrict__ X, long ld, long ncols, long c0, long k0, double (&v)[4],
                                           int tid) {
    const long k = k0 + (tid >> 4);
    const long c = c0 + 4 * (tid & 15);
    if (c < ncols) {
        const double2* p = reinterpret_cast<const double2*>(X + k * ld + c);
        const double2 a = p[0], b = p[1];
        v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    } else {
        v[0] = v[1] = v[2] = v[3] = 0.0;
    }
}
__device__ __forceinline__ void put_rows(double* s, const double (&v)[4], int tid) {  // s[k][row]
    const int r = tid >> 2, k = 4 * (tid & 3);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[(k + e) * LDT + r] = v[e];
}
__device__ __forceinline__ void put_cols(double* s, const double (&v)[4], int tid) {  // s[k][col]
    const int k = tid >> 4, c = 4 * (tid & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[k * LDT + c + e] = v[e];
}

// acc += alpha * the 64 x 64 tile (r0, c0) of A op(B) over the K blocks [kbeg, K) (both multiples of BK).  A: rows x K, row
// pitch lda, rows >= arows zero.  NT: op(B) = B^T, B: cols x K like A (rows >= bext zero).  !NT: B: K x cols, row pitch ldb,
// columns >= bext zero (a multiple of 4).  Four waves, 2 x 2, each 32 x 32 = 2 x 2 blocks of v_mfma_f64_16x16x4_f64; the next K
// block is in flight while this one is multiplied.  The partial product is summed over K on its own and enters acc once.
// sA, sB: BK * LDT doubles of LDS each, 16-byte aligned; all 256 threads of the workgroup call this together.
template <bool NT>
__device__ __forceinline__ void tile_product(const double* __restrict__ A, long lda, long arows, const double* __restrict__ B,
                                             long ldb, long bext, long K, long kbeg, double alpha, long r0, long c0,
                                             d4 (&acc)[2][2], double* sA, double* sB, int tid) {
    const int l = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    double va[4], vb[4];
    stage_rows(A, lda, arows, r0, kbeg, va, tid);
    if (NT) stage_rows(B, ldb, bext, c0, kbeg, vb, tid);
    else stage_cols(B, ldb, bext, c0, kbeg, vb, tid);
    d4 part[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) part[i][j] = d4{0, 0, 0, 0};
    for (long k0 = kbeg; k0 < K; k0 += BK) {
        __syncthreads();
        put_rows(sA, va, tid);
        if (NT) put_rows(sB, vb, tid);
        else put_cols(sB, vb, tid);
        __syncthreads();
        if (k0 + BK < K) {  // next block in flight while this one is multiplied
            stage_rows(A, lda, arows, r0, k0 + BK, va, tid);
            if (NT) stage_rows(B, ldb, bext, c0, k0 + BK, vb, tid);
            else stage_cols(B, ldb, bext, c0, k0 + BK, vb, tid);
        }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const int kr = kk + (l >> 4);
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = sA[kr * LDT + wr * 32 + i * 16 + (l & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = sB[kr * LDT + wc * 32 + j * 16 + (l & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) part[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], part[i][j], 0, 0, 0);
        }
    }
    // the accumulators are read behind the loop's exit branch: wait states by hand (mfma_result_guard in pnmol_hip.hip;
    // tests/test_isa_hazards.py scans every translation unit that includes this)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] += alpha * part[i][j];
}

__device__ __forceinline__ void tile_zero(d4 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4{0, 0, 0, 0};
}

// f(row, col, value) for every element of this wave's 32 x 32 share of the tile at (r0, c0)
template <class F>
__device__ __forceinline__ void tile_each(const d4 (&acc)[2][2], long r0, long c0, int tid, F f) {
    const int l = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long col = c0 + wc * 32 + j * 16 + (l & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) f(r0 + wr * 32 + i * 16 + (l >> 4) + 4 * r, col, acc[i][j][r]);
        }
}

// The predict of one n x n block (a pair of mesh points j, k; X in the frame of the step):
//   XA = X A1^T  (rows of P A^T),   Pm = A1 XA + Q1 K(j, k)
// A1, Q1: row pitch SM_MAXN.  Loads, clamps, the pivots of the padded points and the stores are the caller's.
// Every sum is spelled out in fma(): left to contraction, Q1 K + A1[a][0] XA[0][b] rounds one product or the other, and the
// compiler's choice is not the same in every caller.  The smoother, the draws and the dense output must agree to the bit.
template <int N>
__device__ __forceinline__ void predict_block(const double (&X)[N][N], const double (&A1)[SM_MAXN * SM_MAXN],
                                              const double (&Q1)[SM_MAXN * SM_MAXN], double kjk, double (&XA)[N][N],
                                              double (&Pm)[N][N]) {
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double s = 0.0;
#pragma unroll
            for (int e = 0; e < N; ++e) s = __builtin_fma(X[a][e], A1[b * SM_MAXN + e], s);
            XA[a][b] = s;
        }
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double s = __builtin_fma(Q1[a * SM_MAXN + b], kjk, A1[a * SM_MAXN] * XA[0][b]);
#pragma unroll
            for (int e = 1; e < N; ++e) s = __builtin_fma(A1[a * SM_MAXN + e], XA[e][b], s);
            Pm[a][b] = s;
        }
}

}  // namespace
