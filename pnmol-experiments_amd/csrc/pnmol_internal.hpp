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
// row c, the input of the point-major factor; c >= D -> row Dp + ((c - D) / d) dp + (c - D) % d), or, Xi == null, into dense (rows, cols) row-major
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
