// pnmol_record.hip -- the recorder of the constant-step loop (`pnmol_filter_set_recorder`, include/pnmol_hip.h): the state behind
// every step of `pnmol_filter_steps(_begin)` copied into caller-owned states on the device, so that a constant-step run keeps the
// filtered trajectory (what `PDEFilter.solve` stacks per step, pdefilter.py:140-160 of the reference) without leaving the loop.
//
// One launch of k_record per step, behind the step's read-out launch.  The slot comes from device words only -- the cursor word
// written once per call plus the loop's step counter -- so every step launches with identical arguments and the captured graphs
// of the loop (pnmol_hip.hip, get_graph) stay replayable at any position.  Host logic (validation, cursor): pnmol_record_plan.hpp.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pnmol_internal.hpp"
#include "pnmol_record_plan.hpp"

struct RecordSlot {  // what a slot state owns, as the device sees it
    double* mean;    // Dp
    double* P;       // Dp * Dp
    double* var;     // Dp
};

struct RecordDev {
    RecordPlan plan;
    std::vector<pnmol_state*> states;  // plan.slots with their type
    RecordSlot* table = nullptr;       // device: count entries
    int* cursor = nullptr;             // device: plan.next of the running call
    double* gather = nullptr;          // device: count * Dp, the means of a read-back (pnmol_filter_recorder_means)
    std::vector<double> host;          // ... and their host image
};

namespace {

// 16 bytes at a time: Dp is a multiple of 32, so Dp and Dp^2 doubles are whole pieces, and every buffer comes from hipMalloc
inline __device__ void copy_pieces(double2* __restrict__ dst, const double2* __restrict__ src, long pieces, long first, long stride) {
    for (long e = first; e < pieces; e += stride) dst[e] = src[e];
}

// slot (*cursor + *ctr - 1) <- (P, mean, var).  ctr: the loop's step counter, which k_predict has moved to (steps taken in this
// call, this one included) by the time this launch runs.  An index outside the table is not written (the host refuses such calls
// before they are enqueued; this is the bound of the table all the same).
__global__ __launch_bounds__(256) void k_record(const RecordSlot* __restrict__ table, int count, const int* __restrict__ cursor,
                                                const int* __restrict__ ctr, const double* __restrict__ P,
                                                const double* __restrict__ mean, const double* __restrict__ var, long Dp) {
    const int slot = *cursor + *ctr - 1;
    if (slot < 0 || slot >= count) return;
    const RecordSlot s = table[slot];
    const long first = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    copy_pieces(reinterpret_cast<double2*>(s.P), reinterpret_cast<const double2*>(P), Dp * Dp / 2, first, stride);
    copy_pieces(reinterpret_cast<double2*>(s.mean), reinterpret_cast<const double2*>(mean), Dp / 2, first, stride);
    copy_pieces(reinterpret_cast<double2*>(s.var), reinterpret_cast<const double2*>(var), Dp / 2, first, stride);
}

__global__ void k_record_cursor(int* __restrict__ cursor, int next) { *cursor = next; }

// out[i * Dp + e] = mean of slot first + i: the means of a run of slots side by side for one copy to the host
__global__ __launch_bounds__(256) void k_record_gather(const RecordSlot* __restrict__ table, int first, long Dp,
                                                       double* __restrict__ out) {
    const double* m = table[first + blockIdx.y].mean;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < Dp; e += (long)gridDim.x * 256) out[(long)blockIdx.y * Dp + e] = m[e];
}

void free_dev(RecordDev* r) {
    if (!r) return;
    for (void* p : {(void*)r->table, (void*)r->cursor, (void*)r->gather})
        if (p) (void)hipFree(p);
    delete r;
}

}  // namespace

bool pnmol_record_active(const pnmol_filter* f) { return f->rec_plan != nullptr; }

bool pnmol_record_holds(const pnmol_state* s) { return s->f->rec_plan != nullptr && s->f->rec_plan->plan.holds(s); }

void pnmol_record_free(pnmol_filter* f) {
    free_dev(f->rec_plan);
    f->rec_plan = nullptr;
}

int pnmol_record_begin(pnmol_filter* f, const pnmol_state* s, int k) {
    if (!f->rec_plan) return 0;
    const std::string why = record_plan_begin(f->rec_plan->plan, k, s);
    if (why.empty()) return 0;
    f->ctx->err = "pnmol_filter_steps_begin: recorder: " + why;
    return -1;
}

int pnmol_record_enqueue_cursor(pnmol_filter* f) {
    RecordDev* r = f->rec_plan;
    if (!r) return 0;
    k_record_cursor<<<1, 1, 0, f->ctx->stream>>>(r->cursor, r->plan.next);
    HIPCHK(f->ctx, hipGetLastError());
    return 0;
}

int pnmol_record_enqueue(pnmol_filter* f, const double* P, const double* mean, const double* var) {
    RecordDev* r = f->rec_plan;
    if (!r) return 0;
    const long Dp = f->Dp, pieces = Dp * Dp / 2;
    const unsigned grid = (unsigned)std::min<long>(1024, (pieces + 255) / 256);
    k_record<<<grid, 256, 0, f->ctx->stream>>>(r->table, r->plan.count, r->cursor, f->ctr, P, mean, var, Dp);
    HIPCHK(f->ctx, hipGetLastError());
    return 0;
}

void pnmol_record_collect(pnmol_filter* f, double t0, int k, double dt) {
    RecordDev* r = f->rec_plan;
    if (!r) return;
    double t = t0;
    for (int j = 0; j < k; ++j) {
        t += dt;  // (the accumulation of pnmol_filter_steps_end)
        const int slot = record_plan_slot(r->plan, j);
        if (slot >= r->plan.count) break;
        r->states[(size_t)slot]->t = t;
        r->states[(size_t)slot]->frame_dt = dt;
    }
    record_plan_advance(&r->plan, k);
}

int pnmol_record_cursor(const pnmol_filter* f) { return f->rec_plan ? f->rec_plan->plan.next : 0; }

void pnmol_record_rewind(pnmol_filter* f, int next) {
    if (f->rec_plan) f->rec_plan->plan.next = next;
}

extern "C" {

int pnmol_filter_set_recorder(pnmol_filter* f, int count, pnmol_state* const* slots) {
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    const bool clears = count < 1 || !slots;
    std::vector<const void*> owners;
    if (!clears)
        for (int i = 0; i < count; ++i) owners.push_back(slots[i] ? slots[i]->f : nullptr);
    const std::string why = record_plan_validate(count, reinterpret_cast<const void* const*>(slots), owners.data(), f, f->p32 != 0,
                                                 f->pending_state != nullptr);
    if (!why.empty()) {
        ctx->err = "pnmol_filter_set_recorder: " + why;
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (clears) {
        if (f->rec_plan) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (a launch that reads the table may still be in flight)
            pnmol_drop_graphs(f);
            pnmol_record_free(f);
        }
        return 0;
    }
    RecordDev* r = new RecordDev();
    record_plan_fill(&r->plan, count, reinterpret_cast<const void* const*>(slots));
    r->states.assign(slots, slots + count);
    std::vector<RecordSlot> host((size_t)count);
    for (int i = 0; i < count; ++i) host[(size_t)i] = RecordSlot{slots[i]->mean, slots[i]->P, slots[i]->var};
    hipError_t e = hipMalloc(&r->table, sizeof(RecordSlot) * (size_t)count);
    if (e == hipSuccess) e = hipMalloc(&r->cursor, sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&r->gather, sizeof(double) * (size_t)count * (size_t)f->Dp);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (the table of a recorder this one replaces may be in use)
    if (e == hipSuccess) e = hipMemcpy(r->table, host.data(), sizeof(RecordSlot) * (size_t)count, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(r->cursor, 0, sizeof(int));
    if (e != hipSuccess) {
        ctx->err = std::string("pnmol_filter_set_recorder: ") + hipGetErrorString(e);
        free_dev(r);
        return e == hipErrorOutOfMemory ? -4 : -2;
    }
    pnmol_drop_graphs(f);  // (the loop's launch sequence differs with a recorder, and k_record's table is baked into a graph)
    pnmol_record_free(f);
    f->rec_plan = r;
    return 0;
}

int pnmol_filter_recorder_pending(const pnmol_filter* f, int* next, int* count) {
    if (!f) return -1;
    if (next) *next = f->rec_plan ? f->rec_plan->plan.next : 0;
    if (count) *count = f->rec_plan ? f->rec_plan->plan.count : 0;
    return 0;
}

int pnmol_filter_recorder_means(pnmol_filter* f, int first, int count, double* means_cnd) {
    if (!f) return -1;
    pnmol_ctx* ctx = f->ctx;
    RecordDev* r = f->rec_plan;
    if (!r || !means_cnd || first < 0 || count < 1 || first + count > r->plan.next || f->pending_state) {
        ctx->err = "pnmol_filter_recorder_means: bad argument (no recorder, null, slots that have not been filled, or an unfinished "
                   "pnmol_filter_steps_begin)";
        return -1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long Dp = f->Dp;
    k_record_gather<<<dim3((unsigned)((Dp + 255) / 256), (unsigned)count), 256, 0, ctx->stream>>>(r->table, first, Dp, r->gather);
    HIPCHK(ctx, hipGetLastError());
    r->host.resize((size_t)count * (size_t)Dp);
    HIPCHK(ctx, hipMemcpyAsync(r->host.data(), r->gather, sizeof(double) * r->host.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < count; ++i) {
        double sc[MAXN];
        frame_scales(r->states[(size_t)(first + i)], sc);
        const double* hm = &r->host[(size_t)i * (size_t)Dp];
        double* out = means_cnd + (size_t)i * f->n * f->ds;
        for (int a = 0; a < f->n; ++a)
            for (int j = 0; j < f->ds; ++j) out[(size_t)a * f->ds + j] = sc[a] * hm[(size_t)a * f->dp + j];
    }
    return 0;
}

}  // extern "C"
