// pnmol_linearize_plan.hpp -- host side of the table of linearisation points of the constant-step loop
// (pnmol_filter_set_linearization_points, pnmol_reaction.hip): what is refused of a table of points.  The table itself and its cursor
// are those of every table of the loop (pnmol_cursor_plan.hpp).  Nothing of HIP in here: tests/linearize_plan_check.cpp builds it on
// its own under the sanitizers.
#pragma once
#include <cmath>
#include <string>

#include "pnmol_cursor_plan.hpp"

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
