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
