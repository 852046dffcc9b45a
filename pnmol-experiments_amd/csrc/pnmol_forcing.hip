// pnmol_forcing.hip -- driven problems: sources and boundary values (`pnmol_filter_set_forcing`, `pnmol_filter_force_at`,
// include/pnmol_hip.h): the kernel, then the host side.
//
// u_t = L u + r(u) + s(t, x) with boundary rows B u = g(t): the step that lands on t measures z = H m^- + shift_term - rhs(t) with
// rhs = [s (d); g (nB)].  Only the shift differs from the unforced step: H, S, the gain and the error model are untouched.  k_force
// writes fshift[i] = shift[i] - rhs[i] (one rounded subtraction; without a term shift is zero and the result is -rhs[i], exact) into a
// buffer of its own, and the forced step reads that buffer where the unforced one reads `shift`.  So the shift the term kernels or
// the operator setters wrote stays what it was, a launch repeated is harmless, and clearing the forcing restores nothing.
//
// The loop's table (`pnmol_filter_set_forcing`): rows of mp numbers on the device, the row of a step found from two device words and
// the loop's step counter, as the linearisation points are (pnmol_reaction.hip) -- identical arguments at every step, so the loop's
// graphs capture once.  A single step (`pnmol_filter_force_at`): the right-hand side sits in mapped host memory of its own, which the
// launch in front of pnmol_filter_step reads as a table of one row.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "pnmol_forcing_plan.hpp"
#include "pnmol_internal.hpp"

// what a forced step needs beside the loop's table (pnmol_filter::forcing_rows: rows of mp, padding zero)
struct ForcingDev {
    double* fshift = nullptr;   // device, mp: the shift a forced step measures with
    double* h_one = nullptr;    // mapped host memory, mp: the right-hand side of pnmol_filter_force_at
    double* h_one_dev = nullptr;
    hipEvent_t ev_one = nullptr;  // behind the last launch that read h_one
    bool single = false;        // pnmol_filter_force_at holds a right-hand side
};

namespace {

// One thread per measurement row.  words: row words[0] + *ctr of words[1] -- the cursor of the running call plus the loop's step
// counter, which k_predict moves only behind this launch; without words, row 0.  An index outside the table: the launch reads and
// writes nothing (the host refuses such calls before they are enqueued; this is the bound of the table all the same).
__global__ __launch_bounds__(256) void k_force(const double* __restrict__ rhs, const int* __restrict__ words,
                                               const int* __restrict__ ctr, const double* __restrict__ shift,
                                               double* __restrict__ fshift, int m, int mp) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp) return;
    long r = 0;
    if (words) {
        r = (long)words[0] + *ctr;
        if (r < 0 || r >= words[1]) return;
    }
    fshift[i] = i < m ? shift[i] - rhs[r * mp + i] : 0.0;
}

int refuse(pnmol_filter* f, const char* who, const std::string& why) {
    f->ctx->err = std::string(who) + why;
    return -1;
}

// what both kinds of forcing share: the shift buffer, the staging row and its event.  -4: out of memory, -2: another failure.
int ensure_dev(pnmol_filter* f, const char* who) {
    if (f->forcing) return 0;
    ForcingDev* v = new ForcingDev();
    const size_t row = sizeof(double) * (size_t)f->mp;
    hipError_t e = hipMalloc(&v->fshift, row);
    if (e == hipSuccess) e = hipMemset(v->fshift, 0, row);
    if (e == hipSuccess) e = hipHostMalloc(&v->h_one, row, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&v->h_one_dev), v->h_one, 0);
    if (e == hipSuccess) e = hipEventCreate(&v->ev_one);
    if (e != hipSuccess) {
        f->ctx->err = std::string(who) + hipGetErrorString(e);
        f->forcing = v;
        pnmol_forcing_free(f);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    std::memset(v->h_one, 0, row);
    f->forcing = v;
    return 0;
}

int enqueue_force(pnmol_filter* f, const double* rhs, const int* words, const int* ctr) {
    ForcingDev* v = f->forcing;
    k_force<<<(unsigned)((f->mp + 255) / 256), 256, 0, f->ctx->stream>>>(rhs, words, ctr, f->shift, v->fshift, f->m, f->mp);
    HIPCHK(f->ctx, hipGetLastError());
    return 0;
}

}  // namespace

// (the caller knows the stream idle, or the filter out of use)
void pnmol_forcing_free(pnmol_filter* f) {
    ForcingDev* v = f->forcing;
    if (!v) return;
    if (v->fshift) (void)hipFree(v->fshift);
    if (v->h_one) (void)hipHostFree(v->h_one);
    if (v->ev_one) (void)hipEventDestroy(v->ev_one);
    delete v;
    f->forcing = nullptr;
}

bool pnmol_forcing_table_set(const pnmol_filter* f) { return f->forcing_rows.plan.set(); }
bool pnmol_forcing_set(const pnmol_filter* f) { return pnmol_forcing_table_set(f) || (f->forcing && f->forcing->single); }

const double* pnmol_forcing_enqueue_loop(pnmol_filter* f, int* rc) {
    *rc = 0;
    if (!pnmol_forcing_table_set(f)) return nullptr;
    ForcingDev* v = f->forcing;
    *rc = enqueue_force(f, f->forcing_rows.rows, f->forcing_rows.words, f->ctr);
    return v->fshift;
}

const double* pnmol_forcing_enqueue_single(pnmol_filter* f, int* rc) {
    *rc = 0;
    if (!f->forcing || !f->forcing->single) return nullptr;
    ForcingDev* v = f->forcing;
    *rc = enqueue_force(f, v->h_one_dev, nullptr, nullptr);
    if (*rc == 0 && hipEventRecord(v->ev_one, f->ctx->stream) != hipSuccess) {
        f->ctx->err = "pnmol_filter_step: forcing: hipEventRecord failed";
        *rc = -2;
    }
    return v->fshift;
}

extern "C" {

int pnmol_filter_set_forcing(pnmol_filter* f, int count, const double* rhs_cm) {
    static const char* who = "pnmol_filter_set_forcing: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    const std::string why = forcing_plan_validate(count, rhs_cm, f->m, f->p32 != 0, f->pending_state != nullptr);
    if (!why.empty()) return refuse(f, who, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (a launch that reads the table may still be in flight)
    if (count == 0 || !rhs_cm) {
        loop_table_clear(f, &f->forcing_rows);
        if (f->forcing && !f->forcing->single) pnmol_forcing_free(f);
        return 0;
    }
    if (int rc = ensure_dev(f, who)) return rc;
    std::vector<double> pad;
    try {
        pad.resize((size_t)count * (size_t)f->mp);
    } catch (const std::bad_alloc&) {
        ctx->err = std::string(who) + "out of host memory";
        return -4;
    }
    forcing_plan_pad(rhs_cm, count, f->m, f->mp, pad.data());
    // (a table that fits is overwritten in place and the captured graphs replay on it: they address it through the words)
    return loop_table_install(f, &f->forcing_rows, who, count, f->mp, pad.data());
}

int pnmol_filter_forcing_pending(const pnmol_filter* f, int* next, int* count) {
    return f ? loop_table_pending(f->forcing_rows, next, count) : -1;
}

int pnmol_filter_force_at(pnmol_filter* f, const double* rhs_m) {
    static const char* who = "pnmol_filter_force_at: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    const std::string why = forcing_plan_validate_one(rhs_m, f->m, f->p32 != 0, f->pending_state != nullptr);
    if (!why.empty()) return refuse(f, who, why);
    if (!rhs_m) {
        if (f->forcing) f->forcing->single = false;  // (a table, if set, stays: it belongs to the loop)
        return 0;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure_dev(f, who)) return rc;
    ForcingDev* v = f->forcing;
    // the staging row may still be read by the launch of the previous step: wait for that launch, not for the stream
    HIPCHK(ctx, hipEventSynchronize(v->ev_one));
    std::memcpy(v->h_one, rhs_m, sizeof(double) * (size_t)f->m);
    v->single = true;
    return 0;
}

}  // extern "C"
