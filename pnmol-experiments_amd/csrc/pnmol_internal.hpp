// Private to the library: what the translation units under csrc/ share.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

struct pnmol_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // Lifetime rule of the C ABI (include/pnmol_hip.h, "Lifetimes"): a handle keeps its parent alive.  `children` counts
    // the live pnmol_filter / pnmol_sqrt_filter objects of this ctx; pnmol_ctx_destroy refuses (-1) while it is not zero.
    std::atomic<int> children{0};
};

// The RTS smoother step (pnmol_smoother_step; kernels in pnmol_smooth.hip, host side and sweep in pnmol_hip.hip).
constexpr int SM_MAXN = 4;
struct SmoothConsts {
    double A1[SM_MAXN * SM_MAXN];  // IWP transition in the Nordsieck frame (IwpConsts.A1)
    double Q1[SM_MAXN * SM_MAXN];  // IwpConsts.Q1
    double ts[SM_MAXN];            // frame change of the filtered state into the frame of h
    double tsn[SM_MAXN];           // frame change of the smoothed successor into the frame of h
};
// P^h, P- and P^h A^T into Pout / the sweep's tall matrix Gs, Ps^h into Psh, mh = m^h, dm = ms^h - A m^h
int pnmol_smooth_launch_build(hipStream_t st, int n, const double* P, const double* Ps, const double* m, const double* ms,
                              const double* Kg, const SmoothConsts& c, int d, int dp, double* Gs, double* Pout, double* Psh,
                              double* mh, double* dm);
// from the sweep's V = P A^T L^-T and T = L^-T: G, C = G Ps^h, Pout = P^h - V V^T + C G^T (mirrored), var, mout = mh + G dm
int pnmol_smooth_launch_finish(hipStream_t st, long Dp, const double* V, const double* T, const double* Psh, const double* mh,
                               const double* dm, double* G, double* C, double* Pout, double* mout, double* var);

// Joint posterior draws (pnmol_samples_*; kernels in pnmol_sample.hip, host side in pnmol_hip.hip).  A sample block is
// Dp x Sp row-major (row = state component, derivative-major like a mean; column = draw, Sp = S rounded up to 64), the
// noise block 2 Dp x Sp (xi_1 over xi_2), padding zero.
struct SampleConsts {
    double A1[SM_MAXN * SM_MAXN];  // IwpConsts.A1
    double Q1[SM_MAXN * SM_MAXN];  // IwpConsts.Q1
    double Lq[SM_MAXN * SM_MAXN];  // chol(Q1), lower
    double ts[SM_MAXN];            // frame change of the filtered state into the frame of h
    double tsn[SM_MAXN];           // frame change of the sample block into the frame of h
};
// Gc = P^h, point-major, with unit pivots on the padded points (input of the lenient sweep), Gs (may be null) = [P-; P^h A^T], mh = m^h
int pnmol_sample_launch_build(hipStream_t st, int n, const double* P, const double* m, const double* Kg, const SampleConsts& c,
                              int d, int dp, double* Gc, double* Gs, double* mh);
// standard normals of (seed, step_index) for `rows` draws x `cols` components: into the noise block Xi (component c < D ->
// row c, the input of the point-major factor; c >= D -> row Dp + ((c - D) / d) dp + (c - D) % d), or, Xi == null, into dense (rows, cols) row-major.
// n = 0: every component is placed derivative-major, c -> row (c / d) dp + c % d of Xi (the noise of pnmol_samples_interpolate)
int pnmol_sample_launch_noise(hipStream_t st, unsigned long long seed, unsigned long long step_index, int rows, int cols, int d,
                              int dp, int n, int Sp, double* Xi, double* dense);
// the same placement for host-supplied noise: stage (rows, cols) row-major on the device -> Xi
int pnmol_sample_launch_scatter(hipStream_t st, const double* stage, int rows, int cols, int d, int dp, int n, int Sp, double* Xi);
// Y = [add] + [addvec 1^T] + alpha op(M) X for `batch` stacked (rows x Sp) blocks of X / Y (M rows x rows, row-major, the same
// for every block).  trans: op(M) = M^T; lower: op(M) is lower triangular (what lies above the diagonal is not read);
// perm_n > 0: the rows of op(M) are point-major (j perm_n + a) and the result is stored derivative-major.
int pnmol_sample_launch_thin(hipStream_t st, const double* M, const double* X, double* Y, const double* add, const double* addvec,
                             double alpha, long rows, int Sp, int trans, int lower, int batch, int perm_n);
// R = tsn x_next - A1 xt - scale Lq W  (n x n mixes of the derivative blocks, elementwise over points and draws)
int pnmol_sample_launch_resid(hipStream_t st, int n, const SampleConsts& c, double scale, int dp, int Sp, const double* xnext,
                              const double* xt, const double* W, double* R);
// out (S, n, d) row-major = sc[a] X[(a dp + j) Sp + i]
int pnmol_sample_launch_get(hipStream_t st, int n, int d, int dp, int Sp, int S, const double* sc, const double* X, double* out);

// Dense output between grid times (pnmol_bridge_*, pnmol_state_predict*; kernels in pnmol_dense.hip, host side in pnmol_hip.hip).
// Point-diagonal block of an interval, the storage of a pnmol_bridge: [Pl | Cx | Pr] (each N*N rows of dp: entry (a, b) of the
// n x n block of the matrix at equal mesh points), [ml | mr] (N rows of dp each), diag K (dp).
inline size_t pnmol_dense_block_doubles(int n, int dp) { return (size_t)(3 * n * n + 2 * n + 1) * dp; }
struct DenseFrames {
    double sl[SM_MAXN];  // frame change applied to the left operand (mean: sl[a], covariance: sl[a] sl[b])
    double sr[SM_MAXN];  // the same for the right operand
};
// one row of the evaluation table: x_t = Bm x_l + Bp x_r + N(0, Qb (x) K), read out in raw coordinates through sc
struct DenseQuery {
    double Bm[SM_MAXN * SM_MAXN];
    double Bp[SM_MAXN * SM_MAXN];
    double qbd[SM_MAXN];  // diag Qb
    double sc[SM_MAXN];   // raw-coordinate scale of derivative a
    int knot;             // 0: the formula; 1 / 2: the stored values of the left / right end point
    int pad;
};
// the n x n matrices of the full-covariance kernel: BmS = Bm diag(sl), BpS = Bp diag(sr) carry the frame changes of Pl and Pr
struct DenseMix {
    double BmS[SM_MAXN * SM_MAXN], BpS[SM_MAXN * SM_MAXN], Bm[SM_MAXN * SM_MAXN], Bp[SM_MAXN * SM_MAXN], Qb[SM_MAXN * SM_MAXN];
};
// blk <- point-diagonal blocks of sl sl^T o Pl, Cx (as it is), sr sr^T o Pr, sl o ml, sr o mr, diag K (Cx / Pr / mr may be null:
// the one-sided case, their part of blk is left alone)
int pnmol_dense_launch_gather(hipStream_t st, int n, const double* Pl, const double* Cx, const double* Pr, const double* ml,
                              const double* mr, const double* Kg, const DenseFrames& c, int dp, double* blk);
// means / stds (nq, n, d) row-major on the device from blk and the table of nq rows; one_sided: the Bp terms are skipped
int pnmol_dense_launch_eval(hipStream_t st, int n, int d, int dp, int nq, const double* blk, const DenseQuery* table, int one_sided,
                            double* means, double* stds);
// Pout = A1 (ts ts^T o P) A1^T + Q1 (x) K, var = diag, mout = A1 (ts o m)   (c.ts: frame change of the input; c.tsn unused)
int pnmol_dense_launch_predict(hipStream_t st, int n, const double* P, const double* m, const double* Kg, const SmoothConsts& c,
                               int dp, double* Pout, double* var, double* mout);
// Pout = BmS Pl BmS^T + Bm C Bp^T + (Bm C Bp^T)^T + BpS Pr BpS^T + Qb (x) K (both halves, var = diag), mout = Bm ml + Bp mr
int pnmol_dense_launch_state(hipStream_t st, int n, const double* Pl, const double* Pr, const double* C, const double* Kg,
                             const double* ml, const double* mr, const DenseMix& c, int dp, double* Pout, double* var, double* mout);
// The draw at t between (or behind) drawn neighbours: out = BmS xl [+ BpS xr] + Ls W on (Dp x Sp) sample blocks, the n x n mixes
// of the derivative blocks element-wise over points and draws (W = Gamma xi per derivative block; Ls lower triangular, scaled)
struct DenseDrawMix {
    double BmS[SM_MAXN * SM_MAXN], BpS[SM_MAXN * SM_MAXN], Ls[SM_MAXN * SM_MAXN];
};
int pnmol_dense_launch_draw_mix(hipStream_t st, int n, const DenseDrawMix& c, int dp, int Sp, const double* xl, const double* xr,
                                const double* W, double* out);
