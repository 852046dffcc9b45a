// pnmol_forcing_plan.hpp -- host side of the table of right-hand sides of the constant-step loop (pnmol_filter_set_forcing,
// pnmol_forcing.hip): what is refused of a table of right-hand sides, and its padded image.  The table itself and its cursor are
// those of every table of the loop (pnmol_cursor_plan.hpp).  Nothing of HIP in here: tests/forcing_plan_check.cpp builds it on its
// own under the sanitizers.
#pragma once
#include <cmath>
#include <string>

#include "pnmol_cursor_plan.hpp"

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
