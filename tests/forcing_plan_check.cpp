// The host side of the loop's table of right-hand sides (csrc/pnmol_forcing_plan.hpp) on its own: built with
// -fsanitize=address,undefined and run by tests/test_forcing_host.py.  Checks every refusal of the validation, the padded image of
// a table, the step -> row mapping over split calls and a runt last step, the cursor after a failed call and a rehearsal, and the
// refusal of a call; exits non-zero on the first violation.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pnmol_forcing_plan.hpp"

namespace {

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s: line %d: %s\n", g_case, __LINE__, #cond);        \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)
const char* g_case = "";

bool contains(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

ForcingPlan plan_of(int count, int m) {
    const std::vector<double> rhs((size_t)count * m, 0.25);
    REQUIRE(forcing_plan_validate(count, rhs.data(), m, false, false).empty());
    ForcingPlan p;
    forcing_plan_fill(&p, count, rhs.data());
    return p;
}

void check_validation() {
    g_case = "validation";
    const int count = 4, m = 3;  // (an exact-size table: a read past row count - 1 or column m - 1 is the sanitizer's)
    std::vector<double> rhs((size_t)count * m, 1.5);
    REQUIRE(forcing_plan_validate(count, rhs.data(), m, false, false).empty());
    REQUIRE(contains(forcing_plan_validate(count, rhs.data(), m, true, false), "fp32 filter"));
    REQUIRE(contains(forcing_plan_validate(0, nullptr, m, true, false), "fp32 filter"));
    REQUIRE(contains(forcing_plan_validate(count, rhs.data(), m, false, true), "between pnmol_filter_steps_begin"));
    REQUIRE(contains(forcing_plan_validate(-1, rhs.data(), m, false, false), "count < 0"));
    REQUIRE(contains(forcing_plan_validate(-1, nullptr, m, false, false), "count < 0"));
    for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                       -std::numeric_limits<double>::infinity()}) {
        std::vector<double> v = rhs;
        v[(size_t)2 * m + 1] = bad;
        REQUIRE(contains(forcing_plan_validate(count, v.data(), m, false, false), "row 2 is not finite at column 1"));
        v = rhs;
        v.back() = bad;  // the last entry of the table is looked at
        REQUIRE(contains(forcing_plan_validate(count, v.data(), m, false, false), "row 3 is not finite at column 2"));
        std::vector<double> one(rhs.begin(), rhs.begin() + m);
        REQUIRE(forcing_plan_validate_one(one.data(), m, false, false).empty());
        one[2] = bad;
        REQUIRE(contains(forcing_plan_validate_one(one.data(), m, false, false), "not finite at column 2"));
    }
    REQUIRE(forcing_plan_validate_one(nullptr, m, false, false).empty());  // NULL: back to unforced
    REQUIRE(contains(forcing_plan_validate_one(rhs.data(), m, false, true), "between pnmol_filter_steps_begin"));
    REQUIRE(contains(forcing_plan_validate_one(nullptr, m, false, true), "between"));
    REQUIRE(contains(forcing_plan_validate_one(nullptr, m, true, false), "fp32 filter"));
    // clearing: count = 0 or no table; refused only inside a call
    REQUIRE(forcing_plan_validate(0, rhs.data(), m, false, false).empty());
    REQUIRE(forcing_plan_validate(0, nullptr, m, false, false).empty());
    REQUIRE(forcing_plan_validate(7, nullptr, m, false, false).empty());
    REQUIRE(contains(forcing_plan_validate(0, nullptr, m, false, true), "between"));
    ForcingPlan p = plan_of(count, m);
    REQUIRE(p.set() && p.count == 4 && p.next == 0 && p.left() == 4);
    forcing_plan_fill(&p, 0, nullptr);
    REQUIRE(!p.set() && p.count == 0 && p.next == 0);
    REQUIRE(forcing_plan_begin(p, 1000).empty());  // no table: nothing to refuse
    forcing_plan_collect(&p, 5, true);
    REQUIRE(p.next == 0);
}

// the device image: row stride mp, padding zero (exact-size buffers on both sides)
void check_padding() {
    g_case = "padding";
    const int count = 3, m = 5, mp = 8;
    std::vector<double> rhs((size_t)count * m);
    for (size_t e = 0; e < rhs.size(); ++e) rhs[e] = 1.0 + (double)e;
    std::vector<double> pad((size_t)count * mp, -7.0);
    forcing_plan_pad(rhs.data(), count, m, mp, pad.data());
    for (int r = 0; r < count; ++r)
        for (int j = 0; j < mp; ++j) REQUIRE(pad[(size_t)r * mp + j] == (j < m ? rhs[(size_t)r * m + j] : 0.0));
}

// 14 steps in calls of 13 + 1 (the runt last step is a call of its own: another dt), and in calls of 10 + 2 + 1 + 1
void check_mapping() {
    g_case = "mapping";
    for (const std::vector<int>& calls : {std::vector<int>{13, 1}, std::vector<int>{10, 2, 1, 1}}) {
        ForcingPlan p = plan_of(14, 2);
        int taken = 0;
        for (int k : calls) {
            REQUIRE(forcing_plan_begin(p, k).empty());
            for (int j = 0; j < k; ++j) REQUIRE(forcing_plan_row(p, j) == taken + j);
            forcing_plan_collect(&p, k, true);
            taken += k;
            REQUIRE(p.next == taken && p.left() == 14 - taken);
        }
        REQUIRE(p.left() == 0);
        REQUIRE(contains(forcing_plan_begin(p, 1), "1 step(s) asked for, 0 of 14 right-hand side(s) left"));
        forcing_plan_collect(&p, 4, true);  // never past the end
        REQUIRE(p.next == 14);
        forcing_plan_collect(&p, -2, true);
        REQUIRE(p.next == 14);
    }
}

void check_call_refusals_and_rewinding() {
    g_case = "call refusals, rewinding";
    ForcingPlan p = plan_of(6, 5);
    REQUIRE(forcing_plan_begin(p, 6).empty());
    REQUIRE(contains(forcing_plan_begin(p, 7), "7 step(s) asked for, 6 of 6"));
    forcing_plan_collect(&p, 4, true);
    REQUIRE(forcing_plan_begin(p, 2).empty());
    REQUIRE(contains(forcing_plan_begin(p, 3), "3 step(s) asked for, 2 of 6"));
    REQUIRE(p.next == 4 && p.count == 6);  // a refused call leaves the plan as it was
    // a call that failed consumes no row: the repeated call maps to the same rows
    forcing_plan_collect(&p, 2, false);
    REQUIRE(p.next == 4 && forcing_plan_row(p, 0) == 4 && forcing_plan_row(p, 1) == 5);
    forcing_plan_collect(&p, 2, true);
    REQUIRE(p.next == 6);
    // a rehearsal: the cursor is read, the call collected, the cursor put back; values outside the table are clamped
    forcing_plan_rewind(&p, 4);
    REQUIRE(p.next == 4 && p.left() == 2);
    forcing_plan_rewind(&p, -3);
    REQUIRE(p.next == 0);
    forcing_plan_rewind(&p, 99);
    REQUIRE(p.next == 6);
}

}  // namespace

int main() {
    check_validation();
    check_padding();
    check_mapping();
    check_call_refusals_and_rewinding();
    std::puts("forcing plan: ok");
    return 0;
}
