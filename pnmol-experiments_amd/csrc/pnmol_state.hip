// pnmol_state.hip -- the "states" section of include/pnmol_hip.h: creation, upload and read-back of a filter state
// (`pnmol_state_create` .. `pnmol_state_get_cov`), with the two kernels only these functions launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "pnmol_internal.hpp"
#include "pnmol_tile.hpp"

namespace {

// Covariance in the reference's state order (index j n + a, raw coordinates) as a (Dq x Dq) matrix padded with the
// identity: input of the on-device Cholesky behind pnmol_state_get_cov_sqrtm.
__global__ __launch_bounds__(256) void k_cov_reference_order(const void* __restrict__ P, double* __restrict__ Gc, int n,
                                                             int d, int dp, long Dq, const double* __restrict__ sc, int p32) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= Dq * Dq) return;
    const long r = e / Dq, c = e % Dq, D = (long)n * d, Dp = (long)n * dp;
    double v = (r == c) ? 1.0 : 0.0;
    if (r < D && c < D) {
        const int j = (int)(r / n), a = (int)(r % n), k = (int)(c / n), b = (int)(c % n);
        const long idx = ((long)a * dp + j) * Dp + (long)b * dp + k;
        v = sc[a] * sc[b] * (p32 ? (double)static_cast<const float*>(P)[idx] : static_cast<const double*>(P)[idx]);
    }
    Gc[e] = v;
}

}  // namespace

extern "C" {

int pnmol_state_create(pnmol_filter* f, pnmol_state** out) {
    if (!f || !out) return -1;
    *out = nullptr;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pnmol_state* s = new pnmol_state();
    s->f = f;
    f->states.fetch_add(1);
    const size_t Dp = (size_t)f->Dp;
    if (hipMalloc(&s->mean, sizeof(double) * Dp) != hipSuccess || hipMalloc(&s->var, sizeof(double) * Dp) != hipSuccess ||
        hipMalloc(&s->P, f->psz * Dp * Dp) != hipSuccess) {
        ctx->err = "pnmol_state_create: hipMalloc failed";
        pnmol_state_destroy(s);
        return -4;
    }
    // (on the ctx stream, which is non-blocking: a memset on the null stream is not ordered against the kernels that write
    // this state next, and with a second stream alive in the process it has been seen to land after them)
    hipMemsetAsync(s->mean, 0, sizeof(double) * Dp, ctx->stream);
    hipMemsetAsync(s->var, 0, sizeof(double) * Dp, ctx->stream);
    hipMemsetAsync(s->P, 0, f->psz * Dp * Dp, ctx->stream);
    *out = s;
    return 0;
}

int pnmol_state_destroy(pnmol_state* s) {
    if (!s) return -1;
    if (s->f->pending_state == s) {
        s->f->ctx->err = "pnmol_state_destroy: this state is the target of an unfinished pnmol_filter_steps_begin";
        return -1;
    }
    if (pnmol_record_holds(s)) {
        s->f->ctx->err = "pnmol_state_destroy: this state is a slot of the recorder its filter has set (clear the recorder first)";
        return -1;
    }
    s->f->states.fetch_sub(1);
    hipSetDevice(s->f->ctx->device);
    if (s->mean) hipFree(s->mean);
    if (s->var) hipFree(s->var);
    if (s->P) hipFree(s->P);
    delete s;
    return 0;
}

int pnmol_state_clone(const pnmol_state* s, pnmol_state** out) {
    if (!s || !out) return -1;
    int rc = pnmol_state_create(s->f, out);
    if (rc != 0) return rc;
    pnmol_ctx* ctx = s->f->ctx;
    pnmol_state* o = *out;
    const size_t Dp = (size_t)s->f->Dp;
    HIPCHK(ctx, hipMemcpyAsync(o->mean, s->mean, sizeof(double) * Dp, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(o->var, s->var, sizeof(double) * Dp, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(o->P, s->P, s->f->psz * Dp * Dp, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    o->t = s->t, o->frame_dt = s->frame_dt;
    return 0;
}

int pnmol_state_set(pnmol_state* s, double t, const double* mean_nd, const double* cov_DD) {
    if (!s || !mean_nd || !cov_DD) return -1;
    pnmol_filter* f = s->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int n = f->n, d = f->ds, dp = f->dp;
    const long D = (long)n * d, Dp = f->Dp;
    std::vector<double> hm((size_t)Dp, 0.0), hv((size_t)Dp, 0.0), hP((size_t)Dp * Dp, 0.0);
    for (int a = 0; a < n; ++a)
        for (int j = 0; j < d; ++j) {
            hm[(size_t)a * dp + j] = mean_nd[(size_t)a * d + j];
            hv[(size_t)a * dp + j] = cov_DD[((size_t)j * n + a) * D + (size_t)j * n + a];
        }
    for (int a = 0; a < n; ++a)
        for (int j = 0; j < d; ++j) {
            const double* src = cov_DD + ((size_t)j * n + a) * D;
            double* dst = &hP[((size_t)a * dp + j) * Dp];
            for (int b = 0; b < n; ++b)
                for (int k = 0; k < d; ++k) dst[(size_t)b * dp + k] = src[(size_t)k * n + b];
        }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(s->mean, hm.data(), sizeof(double) * hm.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(s->var, hv.data(), sizeof(double) * hv.size(), hipMemcpyHostToDevice));
    if (f->p32) {
        std::vector<float> hPf(hP.begin(), hP.end());
        HIPCHK(ctx, hipMemcpy(s->P, hPf.data(), sizeof(float) * hPf.size(), hipMemcpyHostToDevice));
    } else {
        HIPCHK(ctx, hipMemcpy(s->P, hP.data(), sizeof(double) * hP.size(), hipMemcpyHostToDevice));
    }
    s->t = t;
    s->frame_dt = 0.0;
    return 0;
}

namespace {
// P = C C^T written straight into the state's derivative-major padded layout, C (D x D, any square root) in the
// reference's F-flattened order: P[(a dp + j)(Dp) + (b dp + k)] = sum_c C[j n + a][c] C[k n + b][c].  One 32x32 tile of
// points (j, k) for one derivative pair (a, b) per block, on the MFMA; also the marginal variances.
__global__ __launch_bounds__(256) void k_cct_layout(void* __restrict__ P, double* __restrict__ var,
                                                    const double* __restrict__ C, int d, int n, int dp, long Dp, int p32) {
    __shared__ double sA[32][33], sB[32][33];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, fr = lane & 15, fk = lane >> 4, wr = w >> 1, wc = w & 1;
    const int tx = t & 31, ty = t >> 5;
    const int a = blockIdx.z / n, b = blockIdx.z % n, j0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const long D = (long)n * d;
    d4 acc = {0, 0, 0, 0};
    for (long c0 = 0; c0 < D; c0 += 32) {
        for (int r = ty; r < 32; r += 8) {
            const int j = j0 + r, k = k0 + r;
            const long c = c0 + tx;
            sA[r][tx] = (j < d && c < D) ? C[((long)j * n + a) * D + c] : 0.0;
            sB[r][tx] = (k < d && c < D) ? C[((long)k * n + b) * D + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < 8; ++st)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sA[wr * 16 + fr][4 * st + fk], sB[wc * 16 + fr][4 * st + fk], acc, 0, 0, 0);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + wr * 16 + fk + 4 * r, k = k0 + wc * 16 + fr;
        if (j < d && k < d) {
            const long idx = ((long)a * dp + j) * Dp + (long)b * dp + k;
            if (p32) static_cast<float*>(P)[idx] = (float)acc[r];
            else static_cast<double*>(P)[idx] = acc[r];
            if (a == b && j == k) var[(long)a * dp + j] = acc[r];
        }
    }
}
}  // namespace

int pnmol_state_set_sqrtm(pnmol_state* s, double t, const double* mean_nd, const double* cov_sqrtm_DD) {
    if (!s || !mean_nd || !cov_sqrtm_DD) return -1;
    pnmol_filter* f = s->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int n = f->n, d = f->ds, dp = f->dp;
    const long D = (long)n * d, Dp = f->Dp;
    std::vector<double> hm((size_t)Dp, 0.0);
    for (int a = 0; a < n; ++a)
        for (int j = 0; j < d; ++j) hm[(size_t)a * dp + j] = mean_nd[(size_t)a * d + j];
    double* dC = nullptr;
    if (hipMalloc(&dC, sizeof(double) * (size_t)D * D) != hipSuccess) return -4;
    int rc = 0;
    do {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = -2; break; }
        if (hipMemcpy(s->mean, hm.data(), sizeof(double) * hm.size(), hipMemcpyHostToDevice) != hipSuccess) { rc = -2; break; }
        if (hipMemcpy(dC, cov_sqrtm_DD, sizeof(double) * (size_t)D * D, hipMemcpyHostToDevice) != hipSuccess) { rc = -2; break; }
        if (hipMemsetAsync(s->P, 0, f->psz * (size_t)Dp * Dp, ctx->stream) != hipSuccess) { rc = -2; break; }
        if (hipMemsetAsync(s->var, 0, sizeof(double) * (size_t)Dp, ctx->stream) != hipSuccess) { rc = -2; break; }
        hipLaunchKernelGGL(k_cct_layout, dim3((d + 31) / 32, (d + 31) / 32, n * n), dim3(256), 0, ctx->stream, (void*)s->P, s->var,
                           dC, d, n, dp, Dp, f->p32);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = -2; break; }
    } while (0);
    hipFree(dC);
    if (rc) {
        ctx->err = std::string("pnmol_state_set_sqrtm: ") + hipGetErrorString(hipGetLastError());
        return rc;
    }
    s->t = t;
    s->frame_dt = 0.0;
    return 0;
}

int pnmol_state_get_time(const pnmol_state* s, double* t) {
    if (!s || !t) return -1;
    *t = s->t;
    return 0;
}

int pnmol_state_get_mean(const pnmol_state* s, double* mean_nd) {
    if (!s || !mean_nd) return -1;
    pnmol_filter* f = s->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> hm((size_t)f->Dp);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(hm.data(), s->mean, sizeof(double) * hm.size(), hipMemcpyDeviceToHost));
    double sc[MAXN];
    frame_scales(s, sc);
    for (int a = 0; a < f->n; ++a)
        for (int j = 0; j < f->ds; ++j) mean_nd[(size_t)a * f->ds + j] = sc[a] * hm[(size_t)a * f->dp + j];
    return 0;
}

int pnmol_state_get_cov_sqrtm(const pnmol_state* s, double* C_DD) {
    if (!s || !C_DD) return -1;
    pnmol_filter* f = s->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int n = f->n, d = f->ds;
    const long D = (long)n * d;
    const int Dq = round_up((int)D, NB), cb = Dq / NB;
    SweepWs ws;
    double* dsc = nullptr;
    hipError_t e = sweep_ws_alloc(&ws, ctx, cb, cb);
    if (e == hipSuccess) e = hipMalloc(&dsc, sizeof(double) * MAXN);
    int rc = 0, inf = 0;
    std::vector<double> hF;
    if (e == hipSuccess) {
        double sc[MAXN];
        frame_scales(s, sc);
        e = hipMemcpy(dsc, sc, sizeof(double) * MAXN, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            k_cov_reference_order<<<(unsigned)(((long)Dq * Dq + 255) / 256), 256, 0, st>>>(s->P, ws.G, n, d, f->dp, Dq, dsc, f->p32);
            rc = sweep_ws_enqueue(f, ws, st, 1, "pnmol_state_get_cov_sqrtm");  // (lenient: a covariance may be singular)
            hF.resize((size_t)Dq * Dq);
            if (rc == 0) e = hipMemcpyAsync(hF.data(), ws.F, sizeof(double) * hF.size(), hipMemcpyDeviceToHost, st);
            if (rc == 0 && e == hipSuccess) e = hipMemcpyAsync(&inf, ws.info, sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e == hipSuccess) e = hipGetLastError();
        }
    }
    sweep_ws_free(&ws);
    if (dsc) (void)hipFree(dsc);
    if (rc != 0) return rc;
    if (e != hipSuccess) {
        ctx->err = std::string("pnmol_state_get_cov_sqrtm: ") + hipGetErrorString(e);
        return -2;
    }
    if ((rc = sweep_info_result(ctx, inf, Dq, "pnmol_state_get_cov_sqrtm", "covariance not positive semi-definite")) != 0) return rc;
    for (long r = 0; r < D; ++r) std::memcpy(C_DD + r * D, &hF[(size_t)r * Dq], sizeof(double) * D);
    return 0;
}

int pnmol_state_get_marginal_var(const pnmol_state* s, double* var_nd) {
    if (!s || !var_nd) return -1;
    pnmol_filter* f = s->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> hv((size_t)f->Dp);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(hv.data(), s->var, sizeof(double) * hv.size(), hipMemcpyDeviceToHost));
    double sc[MAXN];
    frame_scales(s, sc);
    for (int a = 0; a < f->n; ++a)
        for (int j = 0; j < f->ds; ++j) var_nd[(size_t)a * f->ds + j] = sc[a] * sc[a] * hv[(size_t)a * f->dp + j];
    return 0;
}

int pnmol_state_get_cov(const pnmol_state* s, double* cov_DD) {
    if (!s || !cov_DD) return -1;
    pnmol_filter* f = s->f;
    pnmol_ctx* ctx = f->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int n = f->n, d = f->ds, dp = f->dp;
    const long D = (long)n * d, Dp = f->Dp;
    std::vector<double> hP((size_t)Dp * Dp);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (f->p32) {
        std::vector<float> hPf(hP.size());
        HIPCHK(ctx, hipMemcpy(hPf.data(), s->P, sizeof(float) * hPf.size(), hipMemcpyDeviceToHost));
        std::copy(hPf.begin(), hPf.end(), hP.begin());
    } else {
        HIPCHK(ctx, hipMemcpy(hP.data(), s->P, sizeof(double) * hP.size(), hipMemcpyDeviceToHost));
    }
    double sc[MAXN];
    frame_scales(s, sc);
    for (int a = 0; a < n; ++a)
        for (int j = 0; j < d; ++j) {
            double* dst = cov_DD + ((size_t)j * n + a) * D;
            const double* src = &hP[((size_t)a * dp + j) * Dp];
            for (int b = 0; b < n; ++b)
                for (int k = 0; k < d; ++k) dst[(size_t)k * n + b] = sc[a] * sc[b] * src[(size_t)b * dp + k];
        }
    return 0;
}

}  // extern "C"
