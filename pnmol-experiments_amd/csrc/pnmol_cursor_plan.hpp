// pnmol_cursor_plan.hpp -- a device-resident table whose rows the steps of the constant-step loop consume one by one: the host side
// that the table of linearisation points (pnmol_linearize_plan.hpp) and the table of right-hand sides (pnmol_forcing_plan.hpp) share.
// The refusal of one pnmol_filter_steps_begin call, the step -> row mapping over split calls (the runt last step of a schedule arrives
// as a call of its own) and the cursor, which a call that failed -- or a rehearsal -- puts back.  What a table holds, and so what is
// refused of it, is its owner's business.  Nothing of HIP in here.
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
