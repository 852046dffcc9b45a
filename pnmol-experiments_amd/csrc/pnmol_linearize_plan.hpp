// pnmol_linearize_plan.hpp -- host side of the table of linearisation points of the constant-step loop
// (pnmol_filter_set_linearization_points, pnmol_reaction.hip): validation of a table, the refusals of one pnmol_filter_steps_begin
// call, the step -> row mapping over split calls (the runt last step of a schedule arrives as a call of its own) and the cursor,
// which a call that failed -- or a rehearsal -- puts back.  The cursor is that of every table of the loop (pnmol_cursor_plan.hpp); what
// is refused of a table of points is said here.  Nothing of HIP in here: tests/linearize_plan_check.cpp builds it on its own under
// the sanitizers.
#pragma once
#include <cmath>
#include <string>

#include "pnmol_cursor_plan.hpp"

using LinearizePlan = CursorPlan;  // next: the row the next step taken is linearised at

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
inline void linearize_plan_fill(LinearizePlan* p, int count, const double* u) { cursor_plan_fill(p, count, u != nullptr); }

// "" or why a call of k steps is refused.  Touches nothing of the plan.
inline std::string linearize_plan_begin(const LinearizePlan& p, int k) { return cursor_plan_begin(p, k, "linearisation point(s)"); }

// the row step j of the running call is linearised at
inline int linearize_plan_row(const LinearizePlan& p, int j) { return cursor_plan_row(p, j); }

// a call of k steps has been collected: its rows are consumed, unless it failed (pnmol_cursor_plan.hpp)
inline void linearize_plan_collect(LinearizePlan* p, int k, bool ok) { cursor_plan_collect(p, k, ok); }

// put the cursor back (pnmol_filter_prepare_steps rehearses a call); a value outside [0, count] is clamped
inline void linearize_plan_rewind(LinearizePlan* p, int next) { cursor_plan_rewind(p, next); }
