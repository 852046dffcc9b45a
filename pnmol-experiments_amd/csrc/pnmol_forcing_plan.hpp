// pnmol_forcing_plan.hpp -- host side of the table of right-hand sides of the constant-step loop (pnmol_filter_set_forcing,
// pnmol_forcing.hip): validation of a table, the refusals of one pnmol_filter_steps_begin call, the step -> row mapping over split
// calls (the runt last step of a schedule takes its own row) and the cursor, which a call that failed -- or a rehearsal -- puts
// back.  The cursor is that of every table of the loop (pnmol_cursor_plan.hpp); what is refused of a table of right-hand sides is said
// here.  Nothing of HIP in here: tests/forcing_plan_check.cpp builds it on its own under the sanitizers.
#pragma once
#include <cmath>
#include <string>

#include "pnmol_cursor_plan.hpp"

using ForcingPlan = CursorPlan;  // next: the row the next step taken measures against

// "" or why the arguments of pnmol_filter_set_forcing are refused.  count = 0 or no table: clears (refused only inside a call).
// fp32 / call_running: what the filter says of itself; rhs: (count, m) row-major, [source (d); boundary values (nB)].
inline std::string forcing_plan_validate(int count, const double* rhs, int m, bool fp32, bool call_running) {
    if (fp32) return "an fp32 filter takes no forcing";
    if (call_running) return "called between pnmol_filter_steps_begin and pnmol_filter_steps_end";
    if (count < 0) return "count < 0";
    if (count == 0 || !rhs) return "";
    for (long r = 0; r < count; ++r)
        for (long j = 0; j < m; ++j)
            if (!std::isfinite(rhs[r * m + j]))
                return "the right-hand side of row " + std::to_string(r) + " is not finite at column " + std::to_string(j);
    return "";
}

// "" or why the right-hand side of pnmol_filter_force_at is refused (NULL: back to unforced)
inline std::string forcing_plan_validate_one(const double* rhs, int m, bool fp32, bool call_running) {
    if (fp32) return "an fp32 filter takes no forcing";
    if (call_running) return "called between pnmol_filter_steps_begin and pnmol_filter_steps_end";
    for (long j = 0; rhs && j < m; ++j)
        if (!std::isfinite(rhs[j])) return "the right-hand side is not finite at column " + std::to_string(j);
    return "";
}

// the table as the device holds it: row stride mp, the padding zero
inline void forcing_plan_pad(const double* rhs, int count, int m, int mp, double* out) {
    for (long r = 0; r < count; ++r)
        for (long j = 0; j < mp; ++j) out[r * mp + j] = j < m ? rhs[r * m + j] : 0.0;
}

// the plan from validated arguments; the cursor goes to row 0
inline void forcing_plan_fill(ForcingPlan* p, int count, const double* rhs) { cursor_plan_fill(p, count, rhs != nullptr); }

// "" or why a call of k steps is refused.  Touches nothing of the plan.
inline std::string forcing_plan_begin(const ForcingPlan& p, int k) { return cursor_plan_begin(p, k, "right-hand side(s)"); }

// the row step j of the running call measures against
inline int forcing_plan_row(const ForcingPlan& p, int j) { return cursor_plan_row(p, j); }

// a call of k steps has been collected: its rows are consumed, unless it failed (pnmol_cursor_plan.hpp)
inline void forcing_plan_collect(ForcingPlan* p, int k, bool ok) { cursor_plan_collect(p, k, ok); }

// put the cursor back (pnmol_filter_prepare_steps rehearses a call); a value outside [0, count] is clamped
inline void forcing_plan_rewind(ForcingPlan* p, int next) { cursor_plan_rewind(p, next); }
