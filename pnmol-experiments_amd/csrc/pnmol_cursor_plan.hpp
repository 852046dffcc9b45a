// pnmol_cursor_plan.hpp -- a device-resident table whose rows the steps of the constant-step loop consume one by one: the host side
// that the table of linearisation points, the table of right-hand sides and the schedule of operator coefficients share.  The
// refusal of one pnmol_filter_steps_begin call, the step -> row mapping over split calls (the runt last step of a schedule arrives
// as a call of its own), the cursor, which a call that failed -- or a rehearsal -- puts back, and what a set call does to the table
// it finds.  What a table holds, and so what is refused of it, is its owner's business (pnmol_linearize_plan.hpp,
// pnmol_forcing_plan.hpp, pnmol_operator_plan.hpp).  Nothing of HIP in here: tests/cursor_plan_check.cpp builds it on its own under
// the sanitizers.
#pragma once
#include <algorithm>
#include <string>

struct CursorPlan {
    int count = 0;  // rows of the table
    int next = 0;   // cursor: the row the next step taken consumes
    bool set() const { return count > 0; }
    int left() const { return count - next; }
};

// the plan of a table of `count` rows (have: the caller was given one); the cursor goes to row 0
inline void cursor_plan_fill(CursorPlan* p, int count, bool have) {
    *p = CursorPlan{};
    if (count > 0 && have) p->count = count;
}

// "" or why a call of k steps is refused (`rows`: what a row is, in the plural).  Touches nothing of the plan.
inline std::string cursor_plan_begin(const CursorPlan& p, int k, const char* rows) {
    if (!p.set() || k <= p.left()) return "";
    return std::to_string(k) + " step(s) asked for, " + std::to_string(p.left()) + " of " + std::to_string(p.count) + " " + rows +
           " left";
}

// the row step j of the running call consumes
inline int cursor_plan_row(const CursorPlan& p, int j) { return p.next + j; }

// a call of k steps has been collected.  ok: its rows are consumed.  Failed: the cursor stays where the call began -- the state the
// call leaves behind is no input for the rows that follow, and the caller who restores the state repeats the call on the same rows.
inline void cursor_plan_collect(CursorPlan* p, int k, bool ok) {
    if (ok) p->next = std::min(p->count, p->next + std::max(k, 0));
}

// put the cursor back (pnmol_filter_prepare_steps rehearses a call); a value outside [0, count] is clamped
inline void cursor_plan_rewind(CursorPlan* p, int next) { p->next = std::max(0, std::min(p->count, next)); }

// A table of the loop as the filter holds it (pnmol_loop_table.hip installs, clears and walks it): the plan above and where the rows
// live.  The kernel that reads a row finds it from `words` and the loop's step counter, so every step launches with identical
// arguments and the captured graphs of the loop replay at any position.
struct LoopTable {
    CursorPlan plan;
    double* rows = nullptr;   // device: cap rows of `stride` doubles
    int* words = nullptr;     // device: [plan.next of the running call, plan.count]
    int cap = 0, stride = 0;
};

// the tables a filter holds, in the order in which pnmol_filter_steps_begin refuses: what steps_begin's error calls the table,
// and what a row of it is, in the plural
struct LoopTableName {
    const char* label;
    const char* rows;
};
constexpr LoopTableName LOOP_POINTS{"linearisation points", "linearisation point(s)"};
constexpr LoopTableName LOOP_FORCING{"forcing", "right-hand side(s)"};
constexpr LoopTableName LOOP_SCHEDULE{"operator schedule", "row(s) of coefficients"};

// What a set call of `count` rows (0: clear) does to a table with plan p and room for cap rows.  replace: the rows do not fit and
// move to a fresh allocation (made first; if that fails nothing changes, the graphs included); otherwise they are overwritten in
// place.  drop_graphs: the captured graphs of the loop go -- they hold the address of the rows, and the loop's launch sequence
// differs with and without a table: so when the rows move, when the table goes from set to unset or back, and when the copy failed
// (copy_ok false: no table is left set).  Otherwise they stay and replay on the new rows.
struct LoopTableChange {
    bool replace, drop_graphs;
};
inline LoopTableChange loop_table_change(const CursorPlan& p, int cap, int count, bool copy_ok = true) {
    if (count <= 0) return {false, p.set()};
    const bool replace = count > cap;
    return {replace, replace || !p.set() || !copy_ok};
}
