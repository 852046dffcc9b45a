// The host side of the loop's table of right-hand sides (csrc/pnmol_forcing_plan.hpp) on its own: built with
// -fsanitize=address,undefined and run by tests/test_forcing_host.py.  Checks every refusal of the validation and the padded image
// of a table; exits non-zero on the first violation.  The table's cursor is that of every table of the loop:
// tests/cursor_plan_check.cpp.
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

}  // namespace

int main() {
    check_validation();
    check_padding();
    std::puts("forcing plan: ok");
    return 0;
}
