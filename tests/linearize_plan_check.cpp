// The host side of the loop's table of linearisation points (csrc/pnmol_linearize_plan.hpp) on its own: built with
// -fsanitize=address,undefined and run by tests/test_iterated_host.py.  Checks the step -> row mapping over split calls and a runt
// last step, the cursor after a failed call and a rehearsal, every refusal of the validation and of a call; exits non-zero on the
// first violation.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pnmol_linearize_plan.hpp"

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

LinearizePlan plan_of(int count, int d) {
    const std::vector<double> u((size_t)count * d, 0.25);
    REQUIRE(linearize_plan_validate(count, u.data(), d, true, false).empty());
    LinearizePlan p;
    linearize_plan_fill(&p, count, u.data());
    return p;
}

void check_validation() {
    g_case = "validation";
    const int count = 4, d = 3;  // (an exact-size table: a read past row count - 1 or component d - 1 is the sanitizer's)
    std::vector<double> u((size_t)count * d, 1.5);
    REQUIRE(linearize_plan_validate(count, u.data(), d, true, false).empty());
    REQUIRE(contains(linearize_plan_validate(count, u.data(), d, false, false), "no term set"));
    REQUIRE(contains(linearize_plan_validate(count, u.data(), d, true, true), "between pnmol_filter_steps_begin"));
    REQUIRE(contains(linearize_plan_validate(-1, u.data(), d, true, false), "count < 0"));
    REQUIRE(contains(linearize_plan_validate(-1, nullptr, d, false, false), "count < 0"));
    for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                       -std::numeric_limits<double>::infinity()}) {
        std::vector<double> v = u;
        v[(size_t)2 * d + 1] = bad;
        REQUIRE(contains(linearize_plan_validate(count, v.data(), d, true, false), "row 2 is not finite at component 1"));
        v = u;
        v.back() = bad;  // the last entry of the table is looked at
        REQUIRE(contains(linearize_plan_validate(count, v.data(), d, true, false), "row 3 is not finite at component 2"));
    }
    // clearing: count = 0 or no table; refused only inside a call, and never for the lack of a term
    REQUIRE(linearize_plan_validate(0, u.data(), d, false, false).empty());
    REQUIRE(linearize_plan_validate(0, nullptr, d, false, false).empty());
    REQUIRE(linearize_plan_validate(7, nullptr, d, false, false).empty());
    REQUIRE(contains(linearize_plan_validate(0, nullptr, d, true, true), "between"));
    LinearizePlan p = plan_of(count, d);
    REQUIRE(p.set() && p.count == 4 && p.next == 0 && p.left() == 4);
    linearize_plan_fill(&p, 0, nullptr);
    REQUIRE(!p.set() && p.count == 0 && p.next == 0);
    REQUIRE(linearize_plan_begin(p, 1000).empty());  // no table: nothing to refuse
    linearize_plan_collect(&p, 5, true);
    REQUIRE(p.next == 0);
}

// 14 steps in calls of 13 + 1 (the runt last step is a call of its own: another dt), and in calls of 10 + 2 + 1 + 1
void check_mapping() {
    g_case = "mapping";
    for (const std::vector<int>& calls : {std::vector<int>{13, 1}, std::vector<int>{10, 2, 1, 1}}) {
        LinearizePlan p = plan_of(14, 2);
        int taken = 0;
        for (int k : calls) {
            REQUIRE(linearize_plan_begin(p, k).empty());
            for (int j = 0; j < k; ++j) REQUIRE(linearize_plan_row(p, j) == taken + j);
            linearize_plan_collect(&p, k, true);
            taken += k;
            REQUIRE(p.next == taken && p.left() == 14 - taken);
        }
        REQUIRE(p.left() == 0);
        REQUIRE(contains(linearize_plan_begin(p, 1), "1 step(s) asked for, 0 of 14 linearisation point(s) left"));
        linearize_plan_collect(&p, 4, true);  // never past the end
        REQUIRE(p.next == 14);
        linearize_plan_collect(&p, -2, true);
        REQUIRE(p.next == 14);
    }
}

void check_call_refusals_and_rewinding() {
    g_case = "call refusals, rewinding";
    LinearizePlan p = plan_of(6, 5);
    REQUIRE(linearize_plan_begin(p, 6).empty());
    REQUIRE(contains(linearize_plan_begin(p, 7), "7 step(s) asked for, 6 of 6"));
    linearize_plan_collect(&p, 4, true);
    REQUIRE(linearize_plan_begin(p, 2).empty());
    REQUIRE(contains(linearize_plan_begin(p, 3), "3 step(s) asked for, 2 of 6"));
    REQUIRE(p.next == 4 && p.count == 6);  // a refused call leaves the plan as it was
    // a call that failed consumes no row: the repeated call maps to the same rows
    linearize_plan_collect(&p, 2, false);
    REQUIRE(p.next == 4 && linearize_plan_row(p, 0) == 4 && linearize_plan_row(p, 1) == 5);
    linearize_plan_collect(&p, 2, true);
    REQUIRE(p.next == 6);
    // a rehearsal: the cursor is read, the call collected, the cursor put back; values outside the table are clamped
    linearize_plan_rewind(&p, 4);
    REQUIRE(p.next == 4 && p.left() == 2);
    linearize_plan_rewind(&p, -3);
    REQUIRE(p.next == 0);
    linearize_plan_rewind(&p, 99);
    REQUIRE(p.next == 6);
}

}  // namespace

int main() {
    check_validation();
    check_mapping();
    check_call_refusals_and_rewinding();
    std::puts("linearize plan: ok");
    return 0;
}
