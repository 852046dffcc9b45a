// pnmol_ctx.hip -- the "library / device" section of include/pnmol_hip.h (ABI version, device count, contexts, last error) and
// the FD-weight solver of its "cold-path assembly on the device" section (`pnmol_fd_solve_batched`, k_fd_solve).
#include <hip/hip_runtime.h>

#include <string>

#include "pnmol_internal.hpp"

namespace {

// Batched kernel finite-difference stencils (discretize.py:177-201): per mesh point p an s x s system
//     w_p = (k(X_p, X_p) + eta I)^-1 Lk(x_p, X_p),     u_p = LLk(x_p, x_p) - w_p . Lk(x_p, X_p)
// (X_p = the s stencil neighbours; the reference vmaps jnp.linalg.solve over the points).  One thread per point: LU with
// partial pivoting in registers, like LAPACK's getf2 on the s x s matrix (same pivot rule, same update order).
constexpr int FD_MAXS = 16;
__global__ __launch_bounds__(128) void k_fd_solve(const double* __restrict__ gram, const double* __restrict__ dk,
                                                  const double* __restrict__ llk, int N, int s, double* __restrict__ w,
                                                  double* __restrict__ unc) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    double A[FD_MAXS][FD_MAXS], b[FD_MAXS];
    for (int i = 0; i < s; ++i) {
        for (int k = 0; k < s; ++k) A[i][k] = gram[((long)p * s + i) * s + k];
        b[i] = dk[(long)p * s + i];
    }
    for (int c = 0; c < s; ++c) {
        int piv = c;
        double best = fabs(A[c][c]);
        for (int i = c + 1; i < s; ++i)
            if (fabs(A[i][c]) > best) best = fabs(A[i][c]), piv = i;
        if (piv != c) {
            for (int k = 0; k < s; ++k) {
                const double t = A[c][k];
                A[c][k] = A[piv][k], A[piv][k] = t;
            }
            const double t = b[c];
            b[c] = b[piv], b[piv] = t;
        }
        const double inv = 1.0 / A[c][c];
        for (int i = c + 1; i < s; ++i) {
            const double f = A[i][c] * inv;
            A[i][c] = f;
            for (int k = c + 1; k < s; ++k) A[i][k] -= f * A[c][k];
        }
    }
    for (int i = 1; i < s; ++i)          // L y = P b
        for (int k = 0; k < i; ++k) b[i] -= A[i][k] * b[k];
    for (int i = s - 1; i >= 0; --i) {   // U x = y
        for (int k = i + 1; k < s; ++k) b[i] -= A[i][k] * b[k];
        b[i] /= A[i][i];
    }
    double dot = 0.0;
    for (int i = 0; i < s; ++i) {
        w[(long)p * s + i] = b[i];
        dot += b[i] * dk[(long)p * s + i];
    }
    unc[p] = llk[p] - dot;
}

}  // namespace

extern "C" {

// 2: pnmol_filter_desc.dtype, lifetime rule (refused destroys), pnmol_filter_sweep_layout; 3: pnmol_sqrt_filter_create takes dtype = 1
int pnmol_abi_version(void) { return 3; }

int pnmol_device_count(int* count) {
    if (!count) return -1;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) {
        *count = 0;
        return -2;
    }
    *count = c;
    return 0;
}

int pnmol_ctx_create(int device, pnmol_ctx** out) {
    if (!out) return -1;
    *out = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || device < 0 || device >= c) return -2;
    if (hipSetDevice(device) != hipSuccess) return -2;
    pnmol_ctx* ctx = new pnmol_ctx();
    ctx->device = device;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return -2;
    }
    *out = ctx;
    return 0;
}

int pnmol_ctx_destroy(pnmol_ctx* ctx) {
    if (!ctx) return -1;
    if (ctx->children.load() != 0) {  // (lifetime rule, include/pnmol_hip.h: filters first)
        ctx->err = "pnmol_ctx_destroy: " + std::to_string(ctx->children.load()) + " filter(s) of this ctx are still alive";
        return -1;
    }
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return 0;
}

int pnmol_ctx_synchronize(pnmol_ctx* ctx) {
    if (!ctx) return -1;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

const char* pnmol_last_error(pnmol_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int pnmol_fd_solve_batched(pnmol_ctx* ctx, const double* gram_nss, const double* lk_ns, const double* llk_n, int N, int s,
                           double* weights_ns, double* uncertainty_n) {
    if (!ctx || !gram_nss || !lk_ns || !llk_n || !weights_ns || !uncertainty_n || N < 1 || s < 1 || s > FD_MAXS) {
        if (ctx) ctx->err = "pnmol_fd_solve_batched: bad argument (need N >= 1, 1 <= s <= 16, non-null buffers)";
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    double* d = nullptr;
    const size_t nG = (size_t)N * s * s, nV = (size_t)N * s;
    HIPCHK(ctx, hipMalloc(&d, sizeof(double) * (nG + 2 * nV + 2 * (size_t)N)));
    double *dG = d, *dK = dG + nG, *dL = dK + nV, *dW = dL + N, *dU = dW + nV;
    hipError_t e = hipMemcpyAsync(dG, gram_nss, sizeof(double) * nG, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dK, lk_ns, sizeof(double) * nV, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dL, llk_n, sizeof(double) * N, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        k_fd_solve<<<(unsigned)((N + 127) / 128), 128, 0, st>>>(dG, dK, dL, N, s, dW, dU);
        e = hipMemcpyAsync(weights_ns, dW, sizeof(double) * nV, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(uncertainty_n, dU, sizeof(double) * N, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    (void)hipFree(d);
    if (e != hipSuccess) {
        ctx->err = std::string("pnmol_fd_solve_batched: ") + hipGetErrorString(e);
        return -2;
    }
    return 0;
}

}  // extern "C"
