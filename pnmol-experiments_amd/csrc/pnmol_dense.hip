// pnmol_dense.hip -- the dense output between grid times (`pnmol_bridge_*`, `pnmol_state_predict*`, include/pnmol_hip.h;
// DESIGN.md section 14): kernels, then host side.
//
// Between two grid times there is no measurement, so the posterior at t given the two neighbouring states is the bridge of the
// prior IWP (x) K, whose gains are n x n matrices Kronecker the identity (pnmol/base/iwp.py, bridge_coefficients):
//     x_t | x_l, x_r ~ N((Bm (x) I) x_l + (Bp (x) I) x_r, Qb (x) K)
//     Ps_t = Bm Pl Bm^T + Bm C Bp^T + (Bm C Bp^T)^T + Bp Pr Bp^T + Qb (x) K,     C = Cov(x_l, x_r | data)
// block by block over pairs of mesh points: no factorisation, no product longer than n.  Everything here is element-wise in the
// mesh points and memory-bound; no MFMA (of pnmol_tile.hpp this file uses predict_block alone, in k_dn_predict).  Layouts are
// the forward step's: derivative-major (a, j) -> a*dp + j, Dp = n*dp, row-major, zero padding (dp is a multiple of 32).
#include <hip/hip_runtime.h>

#include <cstring>

#include "pnmol_internal.hpp"
#include "pnmol_tile.hpp"

namespace {

// point-diagonal n x n blocks of the three matrices, the two means and diag K: one thread per mesh point
template <int N>
__global__ __launch_bounds__(256) void k_dn_gather(const double* __restrict__ Pl, const double* __restrict__ Cx,
                                                   const double* __restrict__ Pr, const double* __restrict__ ml,
                                                   const double* __restrict__ mr, const double* __restrict__ Kg, DenseFrames c,
                                                   int dp, double* __restrict__ blk) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= dp) return;
    const long Dp = (long)N * dp;
    double* bl = blk;
    double* bc = blk + (long)N * N * dp;
    double* br = blk + 2L * N * N * dp;
    double* vl = blk + 3L * N * N * dp;
    double* vr = vl + (long)N * dp;
#pragma unroll
    for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const long idx = ((long)a * dp + j) * Dp + (long)b * dp + j;
            bl[(long)(a * N + b) * dp + j] = c.sl[a] * c.sl[b] * Pl[idx];
            if (Cx) bc[(long)(a * N + b) * dp + j] = Cx[idx];  // (C is given in the frame of the interval)
            if (Pr) br[(long)(a * N + b) * dp + j] = c.sr[a] * c.sr[b] * Pr[idx];
        }
        vl[(long)a * dp + j] = c.sl[a] * ml[(long)a * dp + j];
        if (mr) vr[(long)a * dp + j] = c.sr[a] * mr[(long)a * dp + j];
    }
    vr[(long)N * dp + j] = Kg[(long)j * dp + j];
}

// mean and marginal std of every derivative at (query blockIdx.y, mesh point j); the per-query constants are uniform over the
// workgroup (scalar loads from the table), the stores run along j: rows of the (nq, n, d) outputs
template <int N>
__global__ __launch_bounds__(256) void k_dn_eval(const double* __restrict__ blk, const DenseQuery* __restrict__ table, int one_sided,
                                                 int d, int dp, double* __restrict__ means, double* __restrict__ stds) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int q = blockIdx.y;
    if (j >= d) return;
    const DenseQuery& t = table[q];
    const double* bl = blk;
    const double* bc = blk + (long)N * N * dp;
    const double* br = blk + 2L * N * N * dp;
    const double* vl = blk + 3L * N * N * dp;
    const double* vr = vl + (long)N * dp;
    double* mo = means + (long)q * N * d + j;
    double* so = stds + (long)q * N * d + j;
    if (t.knot != 0) {  // an end point: its stored values (the order of operations of pnmol_state_get_mean / _marginal_var)
        const double* v = t.knot == 1 ? vl : vr;
        const double* p = t.knot == 1 ? bl : br;
#pragma unroll
        for (int a = 0; a < N; ++a) {
            mo[(long)a * d] = t.sc[a] * v[(long)a * dp + j];
            const double var = t.sc[a] * t.sc[a] * p[(long)(a * N + a) * dp + j];
            so[(long)a * d] = sqrt(fmax(var, 0.0));
        }
        return;
    }
    const double kjj = vr[(long)N * dp + j];
    double xl[N], xr[N], pl[N][N], pc[N][N], pr[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        xl[a] = vl[(long)a * dp + j];
        xr[a] = one_sided ? 0.0 : vr[(long)a * dp + j];
#pragma unroll
        for (int b = 0; b < N; ++b) {
            pl[a][b] = bl[(long)(a * N + b) * dp + j];
            pc[a][b] = one_sided ? 0.0 : bc[(long)(a * N + b) * dp + j];
            pr[a][b] = one_sided ? 0.0 : br[(long)(a * N + b) * dp + j];
        }
    }
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double m = 0.0, v = t.qbd[a] * kjj;
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const double bm = t.Bm[a * SM_MAXN + b], bp = t.Bp[a * SM_MAXN + b];
            m += bm * xl[b] + bp * xr[b];
            double ul = 0.0, uc = 0.0, ur = 0.0;  // rows b of Pl Bm^T, C Bp^T, Pr Bp^T at column a
#pragma unroll
            for (int e = 0; e < N; ++e) {
                ul += pl[b][e] * t.Bm[a * SM_MAXN + e];
                uc += pc[b][e] * t.Bp[a * SM_MAXN + e];
                ur += pr[b][e] * t.Bp[a * SM_MAXN + e];
            }
            v += bm * (ul + 2.0 * uc) + bp * ur;
        }
        mo[(long)a * d] = t.sc[a] * m;
        so[(long)a * d] = t.sc[a] * sqrt(fmax(v, 0.0));
    }
}

// the predict half of the smoother's block transform (predict_block of pnmol_tile.hpp): Pout = A1 (ts ts^T o P) A1^T + Q1 K,
// block by block
template <int N>
__global__ __launch_bounds__(256) void k_dn_predict(const double* __restrict__ P, const double* __restrict__ Kg, SmoothConsts c,
                                                    int dp, double* __restrict__ Pout, double* __restrict__ var) {
    const int k = blockIdx.x * 32 + threadIdx.x;
    const int j = blockIdx.y * 8 + threadIdx.y;
    const long Dp = (long)N * dp;
    double X[N][N], XA[N][N], Pm[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) X[a][b] = c.ts[a] * c.ts[b] * P[((long)a * dp + j) * Dp + (long)b * dp + k];
    predict_block<N>(X, c.A1, c.Q1, Kg[(long)j * dp + k], XA, Pm);
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            Pout[((long)a * dp + j) * Dp + (long)b * dp + k] = Pm[a][b];
            if (a == b && j == k) var[(long)a * dp + j] = Pm[a][b];
        }
}

// mout = L1 (sl o ml) [+ L2 (sr o mr)]: the n x n mixes of the derivative rows of one or two mean vectors
struct MeanMats {
    double L1[SM_MAXN * SM_MAXN], L2[SM_MAXN * SM_MAXN];
};
template <int N>
__global__ __launch_bounds__(256) void k_dn_mean(const double* __restrict__ ml, const double* __restrict__ mr, MeanMats mm,
                                                      DenseFrames c, int dp, double* __restrict__ mout) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= dp) return;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < N; ++b) {
            s += mm.L1[a * SM_MAXN + b] * c.sl[b] * ml[(long)b * dp + j];
            if (mr) s += mm.L2[a * SM_MAXN + b] * c.sr[b] * mr[(long)b * dp + j];
        }
        mout[(long)a * dp + j] = s;
    }
}

// R += Lm[:, c] (x[:] Rm^T): row c of an n x n operand block X (two neighbouring mesh points k, k+1 per lane) enters Lm X Rm^T
template <int N>
__device__ __forceinline__ void mix_row(double2 (&R)[N][N], const double2 (&x)[N], int c, const double* Lm, const double* Rm) {
#pragma unroll
    for (int b = 0; b < N; ++b) {
        double2 t = {0.0, 0.0};
#pragma unroll
        for (int e = 0; e < N; ++e) {
            t.x += x[e].x * Rm[b * SM_MAXN + e];
            t.y += x[e].y * Rm[b * SM_MAXN + e];
        }
#pragma unroll
        for (int a = 0; a < N; ++a) {
            R[a][b].x += Lm[a * SM_MAXN + c] * t.x;
            R[a][b].y += Lm[a * SM_MAXN + c] * t.y;
        }
    }
}

// The full covariance at t.  One workgroup per pair of 32-point tiles (J, K), J >= K; of the symmetric operands Pl, Pr it reads
// tile (J, K) only, of C the tiles (J, K) and (K, J), the second transposed through LDS (one row of n sub-blocks at a time); it
// writes tile (J, K) and, through the same LDS buffer, its mirror image (K, J), so that the result is symmetric bit for bit.  On a
// diagonal tile the entries on or below the diagonal of the (point, derivative) order are the ones that are kept and mirrored.
// 512 lanes: lane -> row j of the tile and two neighbouring points k (16-byte accesses; the 16 lanes of a row cover its 32 points
// = two whole 128-byte lines).  A lane holds one n x n block of double2 (32 registers' worth of doubles at n = 4) plus one
// operand row.
template <int N>
__global__ __launch_bounds__(512) void k_dn_state(const double* __restrict__ Pl, const double* __restrict__ Pr,
                                                  const double* __restrict__ C, const double* __restrict__ Kg, DenseMix c, int dp,
                                                  double* __restrict__ Pout, double* __restrict__ var) {
    __shared__ double s[N][32][33];
    // the five n x n matrices, read as LDS broadcasts inside the loop over operand rows: as 80 uniform registers they do not fit
    // beside the accumulators (the first form of this kernel spilled 269 registers at n = 4)
    __shared__ double cm[5 * SM_MAXN * SM_MAXN];
    const int J = blockIdx.y, K = blockIdx.x;
    if (K > J) return;
    const int tid = threadIdx.x, kl = 2 * (tid & 15), jl = tid >> 4;
    if (tid < 5 * SM_MAXN * SM_MAXN) cm[tid] = reinterpret_cast<const double*>(&c)[tid];
    const double* cBmS = cm;
    const double* cBpS = cm + SM_MAXN * SM_MAXN;
    const double* cBm = cm + 2 * SM_MAXN * SM_MAXN;
    const double* cBp = cm + 3 * SM_MAXN * SM_MAXN;
    const long Dp = (long)N * dp;
    const int j0 = J * 32, k0 = K * 32;
    const bool diag = J == K;
    double2 R[N][N];
    {
        const double2 kk = *reinterpret_cast<const double2*>(Kg + (long)(j0 + jl) * dp + k0 + kl);
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int b = 0; b < N; ++b) R[a][b] = double2{c.Qb[a * SM_MAXN + b] * kk.x, c.Qb[a * SM_MAXN + b] * kk.y};
    }
#pragma unroll 1
    for (int cc = 0; cc < N; ++cc) {
        // sub-blocks (e, cc) of tile (K, J) of C, transposed: s[e][j][k] = C[(e, k0 + k), (cc, j0 + j)]  (this lane: row k = jl of
        // the source tile, its columns j = kl, kl + 1)
        __syncthreads();
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const double2 v = *reinterpret_cast<const double2*>(C + ((long)e * dp + k0 + jl) * Dp + (long)cc * dp + j0 + kl);
            s[e][kl][jl] = v.x;
            s[e][kl + 1][jl] = v.y;
        }
        __syncthreads();
        const long row = ((long)cc * dp + j0 + jl) * Dp + k0 + kl;
        double2 x[N];
#pragma unroll
        for (int e = 0; e < N; ++e) x[e] = *reinterpret_cast<const double2*>(Pl + row + (long)e * dp);
        mix_row<N>(R, x, cc, cBmS, cBmS);
#pragma unroll
        for (int e = 0; e < N; ++e) x[e] = *reinterpret_cast<const double2*>(Pr + row + (long)e * dp);
        mix_row<N>(R, x, cc, cBpS, cBpS);
#pragma unroll
        for (int e = 0; e < N; ++e) x[e] = *reinterpret_cast<const double2*>(C + row + (long)e * dp);
        mix_row<N>(R, x, cc, cBm, cBp);
#pragma unroll
        for (int e = 0; e < N; ++e) x[e] = double2{s[e][jl][kl], s[e][jl][kl + 1]};
        mix_row<N>(R, x, cc, cBp, cBm);
    }
    // tile (J, K)
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double* p = Pout + ((long)a * dp + j0 + jl) * Dp + (long)b * dp + k0 + kl;
            if (!diag) {
                *reinterpret_cast<double2*>(p) = R[a][b];
            } else {
                if (jl > kl || (jl == kl && a >= b)) p[0] = R[a][b].x;
                if (jl > kl + 1 || (jl == kl + 1 && a >= b)) p[1] = R[a][b].y;
                if (a == b && jl == kl) var[(long)a * dp + j0 + jl] = R[a][a].x;
                if (a == b && jl == kl + 1) var[(long)a * dp + j0 + jl] = R[a][a].y;
            }
        }
    // its mirror image: entry ((b, k), (a, j)) of the result = R_jk[a][b]
#pragma unroll
    for (int a = 0; a < N; ++a) {
        __syncthreads();
#pragma unroll
        for (int b = 0; b < N; ++b) {
            s[b][kl][jl] = R[a][b].x;  // s[b][k][j]
            s[b][kl + 1][jl] = R[a][b].y;
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const int kt = jl, jt = kl;  // target row (b, k0 + kt), columns (a, j0 + jt), (a, j0 + jt + 1)
            double* p = Pout + ((long)b * dp + k0 + kt) * Dp + (long)a * dp + j0 + jt;
            const double2 v = {s[b][kt][jt], s[b][kt][jt + 1]};
            if (!diag) {
                *reinterpret_cast<double2*>(p) = v;
            } else {
                if (jt > kt || (jt == kt && a > b)) p[0] = v.x;
                if (jt + 1 > kt || (jt + 1 == kt && a > b)) p[1] = v.y;
            }
        }
    }
}

// out = BmS xl [+ BpS xr] + Ls W, element-wise over (point, draw): the mix of pnmol_samples_interpolate
template <int N>
__global__ __launch_bounds__(256) void k_dn_draw_mix(DenseDrawMix c, int dp, int Sp, const double* __restrict__ xl,
                                                     const double* __restrict__ xr, const double* __restrict__ W,
                                                     double* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long per = (long)dp * Sp;
    if (e >= per) return;
    double l[N], r[N], w[N];
#pragma unroll
    for (int a = 0; a < N; ++a) l[a] = xl[a * per + e], r[a] = xr ? xr[a * per + e] : 0.0, w[a] = W[a * per + e];
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < N; ++b) {
            s += c.BmS[a * SM_MAXN + b] * l[b] + c.BpS[a * SM_MAXN + b] * r[b];
            if (b <= a) s += c.Ls[a * SM_MAXN + b] * w[b];
        }
        out[a * per + e] = s;
    }
}

#define DN_SWITCH(n, CALL)          \
    switch (n) {                    \
        case 2: { constexpr int N = 2; CALL; } break; \
        case 3: { constexpr int N = 3; CALL; } break; \
        case 4: { constexpr int N = 4; CALL; } break; \
        default: return -1;         \
    }

// blk <- point-diagonal blocks of sl sl^T o Pl, Cx (as it is), sr sr^T o Pr, sl o ml, sr o mr, diag K (Cx / Pr / mr may be null:
// the one-sided case, their part of blk is left alone)
int launch_gather(hipStream_t st, int n, const double* Pl, const double* Cx, const double* Pr, const double* ml,
                              const double* mr, const double* Kg, const DenseFrames& c, int dp, double* blk) {
    const unsigned g = (unsigned)((dp + 255) / 256);
    DN_SWITCH(n, (k_dn_gather<N><<<g, 256, 0, st>>>(Pl, Cx, Pr, ml, mr, Kg, c, dp, blk)));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// means / stds (nq, n, d) row-major on the device from blk and the table of nq rows; one_sided: the Bp terms are skipped
int launch_eval(hipStream_t st, int n, int d, int dp, int nq, const double* blk, const DenseQuery* table, int one_sided,
                            double* means, double* stds) {
    // (gridDim.y is limited to 65535)
    for (int q0 = 0; q0 < nq; q0 += 65535) {
        const int nn = nq - q0 < 65535 ? nq - q0 : 65535;
        const dim3 grid((unsigned)((d + 255) / 256), (unsigned)nn);
        DN_SWITCH(n, (k_dn_eval<N><<<grid, 256, 0, st>>>(blk, table + q0, one_sided, d, dp, means + (long)q0 * n * d,
                                                         stds + (long)q0 * n * d)));
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Pout = A1 (ts ts^T o P) A1^T + Q1 (x) K, var = diag, mout = A1 (ts o m)   (c.ts: frame change of the input; c.tsn unused)
int launch_predict(hipStream_t st, int n, const double* P, const double* m, const double* Kg, const SmoothConsts& c,
                               int dp, double* Pout, double* var, double* mout) {
    const dim3 grid(dp / 32, dp / 8), blk(32, 8);
    MeanMats mm{};
    DenseFrames fr{};
    for (int a = 0; a < SM_MAXN; ++a) fr.sl[a] = c.ts[a];
    for (int i = 0; i < SM_MAXN * SM_MAXN; ++i) mm.L1[i] = c.A1[i];
    DN_SWITCH(n, (k_dn_predict<N><<<grid, blk, 0, st>>>(P, Kg, c, dp, Pout, var),
                  k_dn_mean<N><<<(unsigned)((dp + 255) / 256), 256, 0, st>>>(m, nullptr, mm, fr, dp, mout)));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Pout = BmS Pl BmS^T + Bm C Bp^T + (Bm C Bp^T)^T + BpS Pr BpS^T + Qb (x) K (both halves, var = diag), mout = Bm ml + Bp mr
int launch_state(hipStream_t st, int n, const double* Pl, const double* Pr, const double* C, const double* Kg,
                             const double* ml, const double* mr, const DenseMix& c, int dp, double* Pout, double* var, double* mout) {
    const dim3 grid(dp / 32, dp / 32);
    MeanMats mm{};
    DenseFrames fr{};
    for (int a = 0; a < SM_MAXN; ++a) fr.sl[a] = fr.sr[a] = 1.0;  // (the bridge's means are in the frame of the interval)
    for (int i = 0; i < SM_MAXN * SM_MAXN; ++i) mm.L1[i] = c.Bm[i], mm.L2[i] = c.Bp[i];
    DN_SWITCH(n, (k_dn_state<N><<<grid, 512, 0, st>>>(Pl, Pr, C, Kg, c, dp, Pout, var),
                  k_dn_mean<N><<<(unsigned)((dp + 255) / 256), 256, 0, st>>>(ml, mr, mm, fr, dp, mout)));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int pnmol_dense_launch_draw_mix(hipStream_t st, int n, const DenseDrawMix& c, int dp, int Sp, const double* xl, const double* xr,
                                const double* W, double* out) {
    const unsigned grid = (unsigned)(((long)dp * Sp + 255) / 256);
    DN_SWITCH(n, (k_dn_draw_mix<N><<<grid, 256, 0, st>>>(c, dp, Sp, xl, xr, W, out)));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
void pnmol_dense_free_ws(pnmol_filter* f) {
    if (f->dn_scratch) (void)hipFree(f->dn_scratch);
    if (f->dn_slab) {  // (no bridge is alive: the slab is empty)
        if (f->dn_slab->base) (void)hipFree(f->dn_slab->base);
        delete f->dn_slab;
    }
    f->dn_scratch = nullptr, f->dn_cap = 0, f->dn_slab = nullptr;
}

// Enqueued behind the smoother step, before the next one reuses its buffers: the point-diagonal blocks of Ps_k (out),
// C_k = G Ps^h (sm_C) and Ps^h_{k+1} (the product k_sm_build formed), the two means, diag K; with keep_full all of C_k.
int pnmol_dense_make_bridge(pnmol_filter* f, const pnmol_state* filt_k, const pnmol_state* smooth_next, double dt,
                            const pnmol_state* out, const double* tsn, int keep_full, pnmol_bridge** bridge) {
    static const char* who = "pnmol_smoother_step_bridge";
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    const size_t sq = (size_t)f->Dp * f->Dp;
    pnmol_bridge* br = new pnmol_bridge();
    br->f = f, br->t = filt_k->t, br->dt = dt;
    f->bridges.fetch_add(1);
    auto fail = [&](int code, const std::string& why) {
        ctx->err = std::string(who) + ": " + why;
        (void)hipStreamSynchronize(st);
        pnmol_bridge_destroy(br);
        return code;
    };
    const size_t slot = pnmol_dense_block_doubles(f->n, f->dp);
    hipError_t e = hipSuccess;
    if (!f->dn_slab || f->dn_slab->used == BRIDGE_SLAB_SLOTS) {  // (a full slab now belongs to its bridges alone)
        BridgeSlab* sl = new BridgeSlab();
        e = hipMalloc(&sl->base, sizeof(double) * slot * BRIDGE_SLAB_SLOTS);
        if (e == hipSuccess) f->dn_slab = sl;
        else delete sl;
    }
    if (e == hipSuccess) {
        br->slab = f->dn_slab;
        br->blk = br->slab->base + slot * br->slab->used;
        br->slab->used += 1, br->slab->live += 1;
        if (keep_full) e = hipMalloc(&br->Cfull, sizeof(double) * sq);
    }
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? -4 : -2, hipGetErrorString(e));
    DenseFrames fr{};
    for (int a = 0; a < f->n; ++a) fr.sl[a] = 1.0, fr.sr[a] = tsn[a];
    if (launch_gather(st, f->n, out->P, f->sm_C, smooth_next->P, out->mean, smooth_next->mean, f->Kg, fr, f->dp,
                                  br->blk) != 0)
        return fail(-2, "kernel launch failed");
    if (keep_full) {
        e = hipMemcpyAsync(br->Cfull, f->sm_C, sizeof(double) * sq, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return fail(-2, hipGetErrorString(e));
    }
    *bridge = br;
    return 0;
}

int pnmol_bridge_destroy(pnmol_bridge* b) {
    if (!b) return -1;
    b->f->bridges.fetch_sub(1);
    hipSetDevice(b->f->ctx->device);
    if (BridgeSlab* sl = b->slab) {
        sl->live -= 1;
        if (sl->live == 0) {
            if (sl == b->f->dn_slab && sl->used < BRIDGE_SLAB_SLOTS) {
                sl->used = 0;  // (readers and the next writer of a block are on the ctx stream: ordered)
            } else {
                if (sl == b->f->dn_slab) b->f->dn_slab = nullptr;
                (void)hipFree(sl->base);
                delete sl;
            }
        }
    }
    if (b->Cfull) (void)hipFree(b->Cfull);
    delete b;
    return 0;
}

int pnmol_bridge_get_interval(const pnmol_bridge* b, double* t, double* dt, int* has_full) {
    if (!b) return -1;
    if (t) *t = b->t;
    if (dt) *dt = b->dt;
    if (has_full) *has_full = b->Cfull != nullptr;
    return 0;
}

namespace {

// (A_th, Q_th): the IWP over the fraction th of a step, in the Nordsieck frame of the whole step (pnmol/base/iwp.py,
// _partial_interval): entry by entry, every exponent that meets a non-zero entry is >= 0
void partial_interval(const pnmol_filter* f, double th, double* A, double* Q) {
    for (int a = 0; a < f->n; ++a)
        for (int b = 0; b < f->n; ++b) {
            A[a * MAXN + b] = b >= a ? f->iwp.A1[a * MAXN + b] * std::pow(th, b - a) : 0.0;
            Q[a * MAXN + b] = f->iwp.Q1[a * MAXN + b] * std::pow(th, 2 * f->nu + 1 - a - b);
        }
}

}  // namespace

// pnmol/base/iwp.py, bridge_coefficients: Bp = Q_th A_c^T Q1^-1, M = I - Bp A_c, Bm = M A_th, Qb = M Q_th M^T + Bp Q_c Bp^T
void bridge_coefficients(const pnmol_filter* f, double th, double* Bm, double* Bp, double* Qb) {
    const int n = f->n;
    double A[MAXN * MAXN], Q[MAXN * MAXN], Ac[MAXN * MAXN], Qc[MAXN * MAXN], L[MAXN * MAXN] = {0}, M[MAXN * MAXN];
    partial_interval(f, th, A, Q);
    partial_interval(f, 1.0 - th, Ac, Qc);
    small_cholesky(n, f->iwp.Q1, L);  // (positive definite: cond <= 1.6e4 at n = 4)
    for (int col = 0; col < n; ++col) {  // column col of X = Q1^-1 (A_c Q_th); Bp = X^T
        double y[MAXN];
        for (int a = 0; a < n; ++a) {
            double v = 0.0;
            for (int e = 0; e < n; ++e) v += Ac[a * MAXN + e] * Q[e * MAXN + col];
            y[a] = v;
        }
        for (int a = 0; a < n; ++a) {
            for (int e = 0; e < a; ++e) y[a] -= L[a * MAXN + e] * y[e];
            y[a] /= L[a * MAXN + a];
        }
        for (int a = n - 1; a >= 0; --a) {
            for (int e = a + 1; e < n; ++e) y[a] -= L[e * MAXN + a] * y[e];
            y[a] /= L[a * MAXN + a];
        }
        for (int a = 0; a < n; ++a) Bp[col * MAXN + a] = y[a];
    }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            double v = a == b ? 1.0 : 0.0;
            for (int e = 0; e < n; ++e) v -= Bp[a * MAXN + e] * Ac[e * MAXN + b];
            M[a * MAXN + b] = v;
        }
    double MQ[MAXN * MAXN], BQ[MAXN * MAXN];
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            double v = 0.0, w = 0.0, u = 0.0;
            for (int e = 0; e < n; ++e) {
                v += M[a * MAXN + e] * A[e * MAXN + b];
                w += M[a * MAXN + e] * Q[e * MAXN + b];
                u += Bp[a * MAXN + e] * Qc[e * MAXN + b];
            }
            Bm[a * MAXN + b] = v, MQ[a * MAXN + b] = w, BQ[a * MAXN + b] = u;
        }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b) {
            double v = 0.0;
            for (int e = 0; e < n; ++e) v += MQ[a * MAXN + e] * M[b * MAXN + e] + BQ[a * MAXN + e] * Bp[b * MAXN + e];
            Qb[a * MAXN + b] = Qb[b * MAXN + a] = v;
        }
}

namespace {

int ensure_dense_scratch(pnmol_filter* f, size_t bytes, const char* who) {
    if (bytes <= f->dn_cap) return 0;
    if (f->dn_scratch) (void)hipFree(f->dn_scratch);
    f->dn_scratch = nullptr, f->dn_cap = 0;
    const hipError_t e = hipMalloc(&f->dn_scratch, bytes);
    if (e != hipSuccess) {
        f->ctx->err = std::string(who) + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    f->dn_cap = bytes;
    return 0;
}

// table -> device, one launch, the read-out: means / stds (nq, n, d)
int run_dense_eval(pnmol_filter* f, const double* blk_dev, bool blk_in_scratch, const std::vector<DenseQuery>& table, int one_sided,
                   double* means, double* stds, const char* who) {
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    const size_t nq = table.size(), no = nq * (size_t)f->n * f->d;
    const size_t blk_bytes = blk_in_scratch ? sizeof(double) * pnmol_dense_block_doubles(f->n, f->dp) : 0;
    char* base = static_cast<char*>(f->dn_scratch);
    double* out_dev = reinterpret_cast<double*>(base + blk_bytes);
    DenseQuery* tab_dev = reinterpret_cast<DenseQuery*>(base + blk_bytes + 2 * no * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(tab_dev, table.data(), sizeof(DenseQuery) * nq, hipMemcpyHostToDevice, st));
    if (launch_eval(st, f->n, f->d, f->dp, (int)nq, blk_dev, tab_dev, one_sided, out_dev, out_dev + no) != 0) {
        ctx->err = std::string(who) + ": kernel launch failed";
        return -2;
    }
    // straight into the caller's arrays (no host staging: at 10 000 queries the read-out is 123 MB), one synchronisation
    if (means) HIPCHK(ctx, hipMemcpyAsync(means, out_dev, sizeof(double) * no, hipMemcpyDeviceToHost, st));
    if (stds) HIPCHK(ctx, hipMemcpyAsync(stds, out_dev + no, sizeof(double) * no, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

}  // namespace

int pnmol_bridge_eval(const pnmol_bridge* b, int nq, const double* t_q, double* means_qnd, double* stds_qnd) {
    static const char* who = "pnmol_bridge_eval";
    if (!b || nq < 1 || !t_q || (!means_qnd && !stds_qnd)) {
        if (b) b->f->ctx->err = std::string(who) + ": bad argument (null, nq < 1)";
        return -1;
    }
    pnmol_filter* f = b->f;
    pnmol_ctx* ctx = f->ctx;
    std::vector<DenseQuery> table((size_t)nq);
    for (int q = 0; q < nq; ++q) {
        const double t = t_q[q];
        const bool at_l = times_agree(t, b->t, b->dt), at_r = times_agree(t, b->t + b->dt, b->dt);
        if (!std::isfinite(t) || (!at_l && !at_r && !(t > b->t && t < b->t + b->dt))) {
            ctx->err = std::string(who) + ": query time " + std::to_string(t) + " is not inside the bridge's interval [" +
                       std::to_string(b->t) + ", " + std::to_string(b->t + b->dt) + "]";
            return -1;
        }
        DenseQuery& e = table[(size_t)q];
        std::memset(&e, 0, sizeof(e));
        for (int a = 0; a < f->n; ++a) e.sc[a] = nordsieck_scale(f->nu, a, b->dt);
        const double th = (t - b->t) / b->dt;
        e.knot = (at_l || !(th > 0.0)) ? 1 : ((at_r || !(th < 1.0)) ? 2 : 0);
        if (e.knot == 0) {
            double Qb[MAXN * MAXN];
            bridge_coefficients(f, th, e.Bm, e.Bp, Qb);
            for (int a = 0; a < f->n; ++a) e.qbd[a] = Qb[a * MAXN + a];
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t no = (size_t)nq * f->n * f->d;
    int rc = ensure_dense_scratch(f, 2 * no * sizeof(double) + sizeof(DenseQuery) * (size_t)nq, who);
    if (rc != 0) return rc;
    return run_dense_eval(f, b->blk, false, table, 0, means_qnd, stds_qnd, who);
}

int pnmol_state_predict(pnmol_filter* f, const pnmol_state* in, double dt, pnmol_state* out) {
    if (!f || !in || !out || in == out || in->f != f || out->f != f || !(dt > 0.0) || !std::isfinite(dt) || f->ds != f->d || f->p32) {
        if (f) f->ctx->err = "pnmol_state_predict: bad argument (null, aliasing, foreign state, dt <= 0, latent-force or fp32 filter)";
        return -1;
    }
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SmoothConsts c{};
    std::memcpy(c.A1, f->iwp.A1, sizeof(c.A1));
    std::memcpy(c.Q1, f->iwp.Q1, sizeof(c.Q1));
    for (int a = 0; a < f->n; ++a) c.ts[a] = frame_ratio(f, a, in->frame_dt, dt);
    if (launch_predict(ctx->stream, f->n, in->P, in->mean, f->Kg, c, f->dp, out->P, out->var, out->mean) != 0) {
        ctx->err = "pnmol_state_predict: kernel launch failed";
        return -2;
    }
    out->t = in->t + dt;
    out->frame_dt = dt;
    return 0;
}

int pnmol_state_predict_marginals(pnmol_filter* f, const pnmol_state* in, int nq, const double* dt_q, double* means_qnd,
                                  double* stds_qnd) {
    static const char* who = "pnmol_state_predict_marginals";
    if (!f || !in || in->f != f || nq < 1 || !dt_q || (!means_qnd && !stds_qnd) || f->ds != f->d || f->p32) {
        if (f) f->ctx->err = std::string(who) + ": bad argument (null, foreign state, nq < 1, latent-force or fp32 filter)";
        return -1;
    }
    pnmol_ctx* ctx = f->ctx;
    std::vector<DenseQuery> table((size_t)nq);
    double sin[MAXN];
    frame_scales(in, sin);
    for (int q = 0; q < nq; ++q) {
        const double dt = dt_q[q];
        if (!std::isfinite(dt) || dt < 0.0) {
            ctx->err = std::string(who) + ": dt_q[" + std::to_string(q) + "] = " + std::to_string(dt) + " is negative or not finite";
            return -1;
        }
        DenseQuery& e = table[(size_t)q];
        std::memset(&e, 0, sizeof(e));
        if (dt == 0.0) {  // the state itself
            e.knot = 1;
            for (int a = 0; a < f->n; ++a) e.sc[a] = sin[a];
            continue;
        }
        // frame of dt: x_t ~ N(A1 (ts o m), A1 (ts ts^T o P) A1^T + Q1 (x) K), ts = frame change of the input
        for (int a = 0; a < f->n; ++a) {
            e.sc[a] = nordsieck_scale(f->nu, a, dt);
            e.qbd[a] = f->iwp.Q1[a * MAXN + a];
            for (int b2 = 0; b2 < f->n; ++b2) e.Bm[a * MAXN + b2] = f->iwp.A1[a * MAXN + b2] * (sin[b2] / nordsieck_scale(f->nu, b2, dt));
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t no = (size_t)nq * f->n * f->d, nb = pnmol_dense_block_doubles(f->n, f->dp);
    int rc = ensure_dense_scratch(f, (nb + 2 * no) * sizeof(double) + sizeof(DenseQuery) * (size_t)nq, who);
    if (rc != 0) return rc;
    double* blk = static_cast<double*>(f->dn_scratch);
    DenseFrames fr{};
    for (int a = 0; a < f->n; ++a) fr.sl[a] = fr.sr[a] = 1.0;  // (the block stays in the state's frame; Bm carries the change)
    if (launch_gather(ctx->stream, f->n, in->P, nullptr, nullptr, in->mean, nullptr, f->Kg, fr, f->dp, blk) != 0) {
        ctx->err = std::string(who) + ": kernel launch failed";
        return -2;
    }
    return run_dense_eval(f, blk, true, table, 1, means_qnd, stds_qnd, who);
}

int pnmol_bridge_state(const pnmol_bridge* b, const pnmol_state* smooth_k, const pnmol_state* smooth_next, double t,
                       pnmol_state* out) {
    static const char* who = "pnmol_bridge_state";
    if (!b || !smooth_k || !smooth_next || !out || out == smooth_k || out == smooth_next || smooth_k->f != b->f ||
        smooth_next->f != b->f || out->f != b->f) {
        if (b) b->f->ctx->err = std::string(who) + ": bad argument (null, aliasing, state of another filter)";
        return -1;
    }
    pnmol_filter* f = b->f;
    pnmol_ctx* ctx = f->ctx;
    if (!b->Cfull) {
        ctx->err = std::string(who) + ": this bridge was made without keep_full (no cross-covariance C_k)";
        return -1;
    }
    if (!times_agree(smooth_k->t, b->t, b->dt) || !times_agree(smooth_next->t, b->t + b->dt, b->dt)) {
        ctx->err = std::string(who) + ": the states sit at t = " + std::to_string(smooth_k->t) + " and " +
                   std::to_string(smooth_next->t) + ", not at the two ends of the bridge's interval";
        return -1;
    }
    const double th = (t - b->t) / b->dt;
    if (!std::isfinite(t) || !(th > 0.0) || !(th < 1.0)) {
        ctx->err = std::string(who) + ": t = " + std::to_string(t) + " is not strictly inside the bridge's interval (at its ends "
                   "the posterior is the state given)";
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DenseMix c{};
    bridge_coefficients(f, th, c.Bm, c.Bp, c.Qb);
    for (int a = 0; a < f->n; ++a)
        for (int e = 0; e < f->n; ++e) {
            c.BmS[a * MAXN + e] = c.Bm[a * MAXN + e] * frame_ratio(f, e, smooth_k->frame_dt, b->dt);
            c.BpS[a * MAXN + e] = c.Bp[a * MAXN + e] * frame_ratio(f, e, smooth_next->frame_dt, b->dt);
        }
    const double* ml = b->blk + 3 * (size_t)f->n * f->n * f->dp;
    if (launch_state(ctx->stream, f->n, smooth_k->P, smooth_next->P, b->Cfull, f->Kg, ml, ml + (size_t)f->n * f->dp, c,
                                 f->dp, out->P, out->var, out->mean) != 0) {
        ctx->err = std::string(who) + ": kernel launch failed";
        return -2;
    }
    out->t = t;
    out->frame_dt = b->dt;
    return 0;
}
