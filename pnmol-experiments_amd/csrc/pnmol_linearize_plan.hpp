// pnmol_linearize_plan.hpp -- host side of the table of linearisation points of the constant-step loop
// (pnmol_filter_set_linearization_points, pnmol_reaction.hip): validation of a table, the refusals of one pnmol_filter_steps_begin
// call, the step -> row mapping over split calls (the runt last step of a schedule arrives as a call of its own) and the cursor,
// which a call that failed -- or a rehearsal -- puts back.  Nothing of HIP in here: tests/linearize_plan_check.cpp builds it on its
// own under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>

struct LinearizePlan {
    int count = 0;  // rows of the table
    int next = 0;   // cursor: the row the next step taken is linearised at
    bool set() const { return count > 0; }
    int left() const { return count - next; }
};

// "" or why the arguments of pnmol_filter_set_linearization_points are refused.  count = 0 or no table: clears (refused only
// inside a call).  has_term / call_running: what the filter says of itself; u: (count, d) row-major.
inline std::string linearize_plan_validate(int count, const double* u, int d, bool has_term, bool call_running) {
    if (call_running) return "called between pnmol_filter_steps_begin and pnmol_filter_steps_end";
    if (count < 0) return "count < 0";
    if (count == 0 || !u) return "";
    if (!has_term) return "no term set (pnmol_filter_set_reaction, _set_reaction_system, _set_convection)";
    for (long r = 0; r < count; ++r)
        for (long j = 0; j < d; ++j)
            if (!std::isfinite(u[r * d + j]))
                return "the point of row " + std::to_string(r) + " is not finite at component " + std::to_string(j);
    return "";
}

// the plan from validated arguments; the cursor goes to row 0
inline void linearize_plan_fill(LinearizePlan* p, int count, const double* u) {
    *p = LinearizePlan{};
    if (count > 0 && u) p->count = count;
}

// "" or why a call of k steps is refused.  Touches nothing of the plan.
inline std::string linearize_plan_begin(const LinearizePlan& p, int k) {
    if (!p.set() || k <= p.left()) return "";
    return std::to_string(k) + " step(s) asked for, " + std::to_string(p.left()) + " of " + std::to_string(p.count) +
           " linearisation point(s) left";
}

// the row step j of the running call is linearised at
inline int linearize_plan_row(const LinearizePlan& p, int j) { return p.next + j; }

// a call of k steps has been collected.  ok: its rows are consumed.  Failed: the cursor stays where the call began -- the state the
// call leaves behind is no input for the rows that follow, and the caller who restores the state repeats the call on the same rows.
inline void linearize_plan_collect(LinearizePlan* p, int k, bool ok) {
    if (ok) p->next = std::min(p->count, p->next + std::max(k, 0));
}

// put the cursor back (pnmol_filter_prepare_steps rehearses a call); a value outside [0, count] is clamped
inline void linearize_plan_rewind(LinearizePlan* p, int next) { p->next = std::max(0, std::min(p->count, next)); }
