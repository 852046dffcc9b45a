// pnmol_operator.hip -- time-dependent operators (`pnmol_filter_set_operator_family`, `pnmol_filter_set_operator_schedule`,
// `pnmol_filter_operator_at`, include/pnmol_hip.h): the kernel, then the host side.
//
// u_t = sum_r a_r(t) L_r u with R <= 4 fixed stencil operators and scalar coefficients: the step that lands on t measures with
// H = [E1 - M(t) E0; B E0], M(t) = sum_r a_r(t) L_r, and the noise of its PDE rows is that of the operator,
// R_pde(t) = diag(sum_r (a_r(t) e_{r,i})^2) with e_r the diagonal of the FD uncertainty that came with L_r.  The family setter builds
// the union ELL image of the L_r once (pnmol_operator_plan.hpp) with R value planes beside it; k_operator_at forms the entries of a
// step from R numbers and writes them where the step reads its operator (ell_val, rdiag) and into a plane of its own, which a
// pointwise reaction linearises on top of (k_linearize, pnmol_reaction.hip, takes it in place of the creation-time values).
//
// The loop's table (`pnmol_filter_set_operator_schedule`): rows of coefficients on the device, the row of a step found from two
// device words and the loop's step counter, as the right-hand sides are (pnmol_forcing.hip) -- identical arguments at every step, so
// the loop's graphs capture once.  A single step (`pnmol_filter_operator_at`): the coefficients sit in mapped host memory, which the
// launch reads as a table of one row.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "pnmol_internal.hpp"
#include "pnmol_operator_plan.hpp"

static_assert(OPERATOR_MAXR == PNMOL_OPERATOR_MAXR, "the plan header and the C ABI agree on the number of operators");

// host logic in pnmol_operator_plan.hpp; image and planes live on the device.  The schedule is the loop's table
// pnmol_filter::op_schedule (rows of OPERATOR_MAXR, padding zero), which goes with the family it was set for.
struct OperatorDev {
    int R = 0, w = 0;
    int* col = nullptr;          // w x mp: the union image's columns
    double* val = nullptr;       // w x mp: the base values in it (boundary rows; PDE rows: the operator given at creation)
    double* planes = nullptr;    // R x w x mp: L_r per slot
    double* e = nullptr;         // R x mp: noise diagonals
    int* slot = nullptr;         // mp: the diagonal slot of every PDE row
    double* cur = nullptr;       // w x mp: the current operator, as ell_val holds it without a reaction's diagonal
    double* rdiag0 = nullptr;    // mp: the noise given at creation
    double* h_one = nullptr;     // mapped host memory, OPERATOR_MAXR: the coefficients of pnmol_filter_operator_at
    double* h_one_dev = nullptr;
    hipEvent_t ev_one = nullptr;  // behind the last launch that read h_one
};

namespace {

// One thread per measurement row, over the slots of the row; the image is column-major, so loads and stores coalesce across i.
// coef: rows of OPERATOR_MAXR numbers; with words, row words[0] + *ctr of words[1] -- the cursor of the running call plus the loop's
// step counter, which k_predict moves only behind this launch; without words, row 0.  An index outside the table: the launch reads
// and writes nothing (the host refuses such calls before they are enqueued; this is the bound of the table all the same).
// PDE rows i < d: v = a_0 V_0, then v = v + a_r V_r in ascending r, every product and sum rounded on its own (the arithmetic of
// TimeDependentOperator.matrix, pnmol/pde/coefficients.py); the image holds Hv = [-M; B] (build_ell), so -v is written.  Their noise:
// rdiag[i] = sum_r (a_r e_{r,i})^2 in the same order.  Rows i >= d copy the base image and keep their rdiag.
__global__ __launch_bounds__(256) void k_operator_at(const double* __restrict__ coef, const int* __restrict__ words,
                                                     const int* __restrict__ ctr, int R, int w, const int* __restrict__ col,
                                                     const double* __restrict__ base, const double* __restrict__ planes,
                                                     const double* __restrict__ e, double* __restrict__ ell_val,
                                                     double* __restrict__ cur, double* __restrict__ rdiag, int d, int mp) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp) return;
    long row = 0;
    if (words) {
        row = (long)words[0] + *ctr;
        if (row < 0 || row >= words[1]) return;
    }
    double a[OPERATOR_MAXR];
#pragma unroll
    for (int r = 0; r < OPERATOR_MAXR; ++r) a[r] = r < R ? coef[row * OPERATOR_MAXR + r] : 0.0;
    const long plane = (long)w * mp;
    for (int s = 0; s < w; ++s) {
        const long at = (long)s * mp + i;
        double out = base[at];
        if (i < d && col[at] >= 0) {
            double v = a[0] * planes[at];
#pragma unroll
            for (int r = 1; r < OPERATOR_MAXR; ++r)
                if (r < R) v = v + a[r] * planes[r * plane + at];
            out = -v;
        }
        ell_val[at] = out;
        cur[at] = out;
    }
    if (i < d) {
        double t = a[0] * e[i];
        double q = t * t;
#pragma unroll
        for (int r = 1; r < OPERATOR_MAXR; ++r)
            if (r < R) {
                t = a[r] * e[(long)r * mp + i];
                q = q + t * t;
            }
        rdiag[i] = q;
    }
}

int refuse(pnmol_filter* f, const char* who, const std::string& why) {
    f->ctx->err = std::string(who) + why;
    return -1;
}

OperatorFilterFacts facts_of(const pnmol_filter* f) {
    OperatorFilterFacts x;
    x.latent = f->ds != f->d;
    x.fp32 = f->p32 != 0;
    x.dense_noise = f->Rdense != nullptr;
    x.call_running = f->pending_state != nullptr;
    x.wide_term = f->term == TermKind::system || f->term == TermKind::convection;
    x.no_diag = !f->base_has_diag;
    x.replaced = f->op_replaced != 0;
    return x;
}

int enqueue_operator(pnmol_filter* f, const double* coef, const int* words, const int* ctr) {
    OperatorDev* v = f->op_family;
    k_operator_at<<<(unsigned)((f->mp + 255) / 256), 256, 0, f->ctx->stream>>>(coef, words, ctr, v->R, v->w, v->col, v->val, v->planes,
                                                                               v->e, f->ell_val, v->cur, f->rdiag, f->d, f->mp);
    HIPCHK(f->ctx, hipGetLastError());
    return 0;
}

template <class T>
hipError_t upload(T** dst, const std::vector<T>& src) {
    hipError_t e = hipMalloc(dst, sizeof(T) * src.size());
    if (e == hipSuccess) e = hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice);
    return e;
}

void free_dev(OperatorDev* v) {
    if (!v) return;
    for (void* q : {(void*)v->col, (void*)v->val, (void*)v->planes, (void*)v->e, (void*)v->slot, (void*)v->cur, (void*)v->rdiag0})
        if (q) (void)hipFree(q);
    if (v->h_one) (void)hipHostFree(v->h_one);
    if (v->ev_one) (void)hipEventDestroy(v->ev_one);
    delete v;
}

// the base image and the creation-time noise back where the step reads them (the caller has synchronised and dropped the graphs)
int restore_plain(pnmol_filter* f, const OperatorDev* v) {
    if (int rc = pnmol_ell_restore_base(f, true)) return rc;
    HIPCHK(f->ctx, hipMemcpyAsync(f->rdiag, v->rdiag0, sizeof(double) * (size_t)f->mp, hipMemcpyDeviceToDevice, f->ctx->stream));
    f->sq_dt = -1.0;
    return 0;
}

}  // namespace

// (the caller knows the stream idle, or the filter out of use)
void pnmol_operator_free(pnmol_filter* f) {
    free_dev(f->op_family);
    f->op_family = nullptr;
}

bool pnmol_operator_family_set(const pnmol_filter* f) { return f->op_family != nullptr; }
bool pnmol_operator_schedule_set(const pnmol_filter* f) { return f->op_schedule.plan.set(); }

void pnmol_operator_linearize_base(const pnmol_filter* f, const double** base_val, const int** slot) {
    if (!f->op_family) return;
    *base_val = f->op_family->cur;
    *slot = f->op_family->slot;
}

int pnmol_operator_put_image(pnmol_filter* f) {
    pnmol_ctx* ctx = f->ctx;
    hipStream_t st = ctx->stream;
    OperatorDev* v = f->op_family;
    const size_t cells = (size_t)v->w * f->mp;
    if (v->w > f->ell_cap) HIPCHK(ctx, hipStreamSynchronize(st));  // the buffers replaced below may still be read
    if (int rc = pnmol_ell_reserve(f, v->w)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(f->ell_col, v->col, sizeof(int) * cells, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(f->ell_val, v->cur, sizeof(double) * cells, hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(f->shift, 0, sizeof(double) * (size_t)f->mp, st));
    f->ellw = v->w;
    f->ell_is_base = 0;  // (pnmol_ell_restore_base copies the columns back)
    return 0;
}

int pnmol_operator_enqueue_loop(pnmol_filter* f) {
    if (!pnmol_operator_schedule_set(f)) return 0;
    return enqueue_operator(f, f->op_schedule.rows, f->op_schedule.words, f->ctr);
}

extern "C" {

int pnmol_filter_set_operator_family(pnmol_filter* f, int R, const double* L_Rdd, const double* e_Rd) {
    static const char* who = "pnmol_filter_set_operator_family: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    const std::string why = operator_family_validate(R, L_Rdd, e_Rd, f->d, facts_of(f));
    if (!why.empty()) return refuse(f, who, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (a launch that reads the image may still be in flight)
    pnmol_drop_graphs(f);  // (width, pointers and the loop's launch sequence are baked into them)
    if (R == 0 || !L_Rdd || !e_Rd) {
        if (!f->op_family) return 0;
        OperatorDev* old = f->op_family;
        f->op_family = nullptr;  // (a scalar reaction linearises on the base image again)
        const int rc = restore_plain(f, old);
        if (rc == 0) (void)hipStreamSynchronize(ctx->stream);  // (the copy above reads old->rdiag0)
        free_dev(old);
        loop_table_clear(f, &f->op_schedule);  // (its schedule goes with it)
        return rc;
    }
    const int d = f->d, mp = f->mp, bw = f->base_w;
    OperatorImageHost h;
    std::vector<int> bcol((size_t)bw * mp);
    std::vector<double> bval((size_t)bw * mp);
    HIPCHK(ctx, hipMemcpy(bcol.data(), f->ell_col_base, sizeof(int) * bcol.size(), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(bval.data(), f->ell_val_base, sizeof(double) * bval.size(), hipMemcpyDeviceToHost));
    try {
        h = operator_family_image(bcol, bval, bw, d, mp, R, L_Rdd, e_Rd);
    } catch (const std::bad_alloc&) {
        ctx->err = std::string(who) + "out of host memory";
        return -4;
    }
    OperatorDev* v = new OperatorDev();
    v->R = R, v->w = h.img.w;
    const size_t row = sizeof(double) * (size_t)mp;
    hipError_t e = upload(&v->col, h.img.col);
    if (e == hipSuccess) e = upload(&v->val, h.img.val);
    if (e == hipSuccess) e = upload(&v->cur, h.img.val);
    if (e == hipSuccess) e = upload(&v->planes, h.planes);
    if (e == hipSuccess) e = upload(&v->e, h.e);
    if (e == hipSuccess) e = upload(&v->slot, h.img.slot);
    if (e == hipSuccess) e = hipMalloc(&v->rdiag0, row);
    // the noise given at creation: f->rdiag holds it unless a family is being replaced
    if (e == hipSuccess) e = hipMemcpy(v->rdiag0, f->op_family ? f->op_family->rdiag0 : f->rdiag, row, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipHostMalloc(&v->h_one, sizeof(double) * OPERATOR_MAXR, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&v->h_one_dev), v->h_one, 0);
    if (e == hipSuccess) e = hipEventCreate(&v->ev_one);
    if (e != hipSuccess) {  // (nothing is installed: the family set before, if any, stays as it was)
        ctx->err = std::string(who) + hipGetErrorString(e);
        free_dev(v);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    std::memset(v->h_one, 0, sizeof(double) * OPERATOR_MAXR);
    OperatorDev* old = f->op_family;
    f->op_family = v;
    int rc = pnmol_operator_put_image(f);
    if (rc == 0) rc = hipMemcpyAsync(f->rdiag, v->rdiag0, row, hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess ? 0 : -2;
    if (rc == 0) rc = hipStreamSynchronize(ctx->stream) == hipSuccess ? 0 : -2;
    free_dev(old);
    loop_table_clear(f, &f->op_schedule);  // (the schedule of the family before goes with it)
    f->sq_dt = -1.0;  // the error model belongs to the operator that was set
    if (rc != 0) {  // no half-installed family: the operator given at creation
        const std::string err = ctx->err.empty() ? std::string(who) + "installing the image failed" : ctx->err;
        f->op_family = nullptr;
        (void)restore_plain(f, v);
        (void)hipStreamSynchronize(ctx->stream);
        free_dev(v);
        ctx->err = err;
    }
    return rc;
}

int pnmol_filter_set_operator_schedule(pnmol_filter* f, int count, const double* a_cR) {
    static const char* who = "pnmol_filter_set_operator_schedule: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    OperatorDev* v = f->op_family;
    const std::string why = operator_schedule_validate(count, a_cR, v ? v->R : 0, facts_of(f));
    if (!why.empty()) return refuse(f, who, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (a launch that reads the table may still be in flight)
    if (count == 0 || !a_cR) {
        loop_table_clear(f, &f->op_schedule);
        return 0;
    }
    std::vector<double> pad;
    try {
        pad.resize((size_t)count * OPERATOR_MAXR);
    } catch (const std::bad_alloc&) {
        ctx->err = std::string(who) + "out of host memory";
        return -4;
    }
    operator_schedule_pad(a_cR, count, v->R, pad.data());
    // (a table that fits is overwritten in place and the captured graphs replay on it: they address it through the words)
    return loop_table_install(f, &f->op_schedule, who, count, OPERATOR_MAXR, pad.data());
}

int pnmol_filter_operator_schedule_pending(const pnmol_filter* f, int* next, int* count) {
    return f ? loop_table_pending(f->op_schedule, next, count) : -1;
}

int pnmol_filter_operator_at(pnmol_filter* f, const double* a_R) {
    static const char* who = "pnmol_filter_operator_at: ";
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    OperatorDev* v = f->op_family;
    const std::string why = operator_at_validate(a_R, v ? v->R : 0, facts_of(f));
    if (!why.empty()) return refuse(f, who, why);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the staging row may still be read by the launch of the previous call: wait for that launch, not for the stream
    HIPCHK(ctx, hipEventSynchronize(v->ev_one));
    for (int r = 0; r < OPERATOR_MAXR; ++r) v->h_one[r] = r < v->R ? a_R[r] : 0.0;
    if (int rc = enqueue_operator(f, v->h_one_dev, nullptr, nullptr)) return rc;
    HIPCHK(ctx, hipEventRecord(v->ev_one, ctx->stream));
    f->sq_dt = -1.0;  // the operator changed: pnmol_filter_prepare_error_model comes next
    return 0;
}

}  // extern "C"
