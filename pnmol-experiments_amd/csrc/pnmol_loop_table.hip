// pnmol_loop_table.hip -- the per-step tables of the constant-step loop (LoopTable, pnmol_cursor_plan.hpp): linearisation points
// (pnmol_reaction.hip), right-hand sides (pnmol_forcing.hip) and operator coefficients (pnmol_operator.hip).  One upload path, one
// rule for the captured graphs (loop_table_change) and the tables' part of pnmol_filter_steps_begin / _end, over the list the filter
// holds (pnmol_filter::loop_tables).  What is refused of a table, its padding and the kernel that reads a row stay with its owner.
#include <hip/hip_runtime.h>

#include "pnmol_internal.hpp"

namespace {

// the two words a row-reading kernel adds the loop's step counter to: once per call, in front of its steps
__global__ void k_loop_table_cursor(int* __restrict__ words, int next, int count) {
    words[0] = next;
    words[1] = count;
}

int fail(pnmol_ctx* ctx, const char* who, hipError_t e) {
    ctx->err = std::string(who) + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? -4 : -2;
}

}  // namespace

int loop_table_install(pnmol_filter* f, LoopTable* tab, const char* who, int count, int stride, const double* padded_rows) {
    pnmol_ctx* ctx = f->ctx;
    const CursorPlan was = tab->plan;
    const int cap = tab->cap;
    const size_t bytes = sizeof(double) * (size_t)count * (size_t)stride;
    if (!tab->words) {
        hipError_t e = hipMalloc(&tab->words, 2 * sizeof(int));
        if (e == hipSuccess) e = hipMemset(tab->words, 0, 2 * sizeof(int));
        if (e != hipSuccess) return fail(ctx, who, e);
    }
    if (loop_table_change(was, cap, count).replace) {
        double* fresh = nullptr;
        const hipError_t e = hipMalloc(&fresh, bytes);
        if (e != hipSuccess) return fail(ctx, who, e);  // (nothing is installed: the table set before, if any, stays as it was)
        if (tab->rows) (void)hipFree(tab->rows);
        tab->rows = fresh, tab->cap = count;
    }
    tab->stride = stride;
    tab->plan = CursorPlan{};
    const hipError_t e = hipMemcpy(tab->rows, padded_rows, bytes, hipMemcpyHostToDevice);
    if (loop_table_change(was, cap, count, e == hipSuccess).drop_graphs) pnmol_drop_graphs(f);
    if (e != hipSuccess) {  // (the table is half overwritten: no table is left set)
        ctx->err = std::string(who) + hipGetErrorString(e);
        return -2;
    }
    cursor_plan_fill(&tab->plan, count, true);
    return 0;
}

void loop_table_clear(pnmol_filter* f, LoopTable* tab) {
    if (loop_table_change(tab->plan, tab->cap, 0).drop_graphs) pnmol_drop_graphs(f);
    if (tab->rows) (void)hipFree(tab->rows);
    if (tab->words) (void)hipFree(tab->words);
    *tab = LoopTable{};
}

int loop_table_pending(const LoopTable& tab, int* next, int* count) {
    if (next) *next = tab.plan.next;
    if (count) *count = tab.plan.count;
    return 0;
}

void loop_tables_free(pnmol_filter* f) {
    for (const LoopTableRef& t : f->loop_tables) loop_table_clear(f, t.tab);
}

int loop_tables_begin(pnmol_filter* f, int k) {
    for (const LoopTableRef& t : f->loop_tables) {
        const std::string why = cursor_plan_begin(t.tab->plan, k, t.name.rows);
        if (why.empty()) continue;
        f->ctx->err = std::string("pnmol_filter_steps_begin: ") + t.name.label + ": " + why;
        return -1;
    }
    return 0;
}

int loop_tables_enqueue_cursors(pnmol_filter* f) {
    for (const LoopTableRef& t : f->loop_tables) {
        if (!t.tab->plan.set()) continue;
        k_loop_table_cursor<<<1, 1, 0, f->ctx->stream>>>(t.tab->words, t.tab->plan.next, t.tab->plan.count);
        HIPCHK(f->ctx, hipGetLastError());
    }
    return 0;
}

void loop_tables_collect(pnmol_filter* f, int k, bool ok) {
    for (const LoopTableRef& t : f->loop_tables) cursor_plan_collect(&t.tab->plan, k, ok);
}

LoopCursors loop_tables_cursors(const pnmol_filter* f) {
    LoopCursors c;
    for (int i = 0; i < LOOP_TABLES; ++i) c.next[i] = f->loop_tables[i].tab->plan.next;
    return c;
}

void loop_tables_rewind(pnmol_filter* f, const LoopCursors& c) {
    for (int i = 0; i < LOOP_TABLES; ++i) cursor_plan_rewind(&f->loop_tables[i].tab->plan, c.next[i]);
}
