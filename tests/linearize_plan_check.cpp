// The host side of the loop's table of linearisation points (csrc/pnmol_linearize_plan.hpp) on its own: built with
// -fsanitize=address,undefined and run by tests/test_iterated_host.py.  Checks every refusal of the validation; exits non-zero on
// the first violation.  The table's cursor is that of every table of the loop: tests/cursor_plan_check.cpp.
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
}

}  // namespace

int main() {
    check_validation();
    std::puts("linearize plan: ok");
    return 0;
}
