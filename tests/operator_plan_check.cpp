// The host side of time-dependent operators (csrc/pnmol_operator_plan.hpp) on its own: built with -fsanitize=address,undefined and
// run by tests/test_operator_host.py.  Checks every refusal of the three validations, the padded image of a table, the union image
// of a family (columns ascending and packed, a slot for every entry of any operator and for the diagonal whatever the
// coefficients, value planes, boundary rows and padding untouched, the width growing past the base); exits non-zero on the first
// violation.  The schedule's cursor is that of every table of the loop: tests/cursor_plan_check.cpp.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pnmol_operator_plan.hpp"

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
    const int R = 2, d = 3;
    std::vector<double> L((size_t)R * d * d, 0.5), e((size_t)R * d, 0.1);
    const OperatorFilterFacts ok;
    REQUIRE(operator_family_validate(R, L.data(), e.data(), d, ok).empty());
    REQUIRE(operator_family_validate(4, std::vector<double>(4 * 9, 1.0).data(), std::vector<double>(12, 1.0).data(), d, ok).empty());
    REQUIRE(contains(operator_family_validate(5, L.data(), e.data(), d, ok), "R outside [1, 4]"));
    REQUIRE(contains(operator_family_validate(-1, L.data(), e.data(), d, ok), "R outside [1, 4]"));
    // clearing: R = 0 or a NULL argument; refused only where the filter has no such path or inside a call
    REQUIRE(operator_family_validate(0, nullptr, nullptr, d, ok).empty());
    REQUIRE(operator_family_validate(2, nullptr, e.data(), d, ok).empty());
    OperatorFilterFacts f = ok;
    f.latent = true;
    REQUIRE(contains(operator_family_validate(R, L.data(), e.data(), d, f), "latent-force"));
    REQUIRE(contains(operator_schedule_validate(1, e.data(), R, f), "latent-force"));
    REQUIRE(contains(operator_at_validate(e.data(), R, f), "latent-force"));
    f = ok, f.fp32 = true;
    REQUIRE(contains(operator_family_validate(R, L.data(), e.data(), d, f), "fp32"));
    REQUIRE(contains(operator_schedule_validate(1, e.data(), R, f), "fp32"));
    REQUIRE(contains(operator_at_validate(e.data(), R, f), "fp32"));
    f = ok, f.call_running = true;
    REQUIRE(contains(operator_family_validate(R, L.data(), e.data(), d, f), "between pnmol_filter_steps_begin"));
    REQUIRE(contains(operator_family_validate(0, nullptr, nullptr, d, f), "between"));
    REQUIRE(contains(operator_schedule_validate(0, nullptr, R, f), "between"));
    REQUIRE(contains(operator_at_validate(e.data(), R, f), "between"));
    f = ok, f.dense_noise = true;
    REQUIRE(contains(operator_family_validate(R, L.data(), e.data(), d, f), "not diagonal"));
    f = ok, f.wide_term = true;
    REQUIRE(contains(operator_family_validate(R, L.data(), e.data(), d, f), "reaction system or a convection term"));
    REQUIRE(operator_family_validate(0, nullptr, nullptr, d, f).empty());
    f = ok, f.replaced = true;
    REQUIRE(contains(operator_family_validate(R, L.data(), e.data(), d, f), "operator given at creation was replaced"));
    REQUIRE(operator_family_validate(0, nullptr, nullptr, d, f).empty());
    f = ok, f.no_diag = true;
    REQUIRE(contains(operator_family_validate(R, L.data(), e.data(), d, f), "no diagonal entry"));
    for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
        std::vector<double> v = L;
        v[(size_t)(1 * d + 2) * d + 1] = bad;
        REQUIRE(contains(operator_family_validate(R, v.data(), e.data(), d, ok), "operator 1 is not finite at row 2, column 1"));
        v = L, v.back() = bad;
        REQUIRE(contains(operator_family_validate(R, v.data(), e.data(), d, ok), "operator 1 is not finite at row 2, column 2"));
        v = e, v[(size_t)1 * d + 0] = bad;
        REQUIRE(contains(operator_family_validate(R, L.data(), v.data(), d, ok), "noise diagonal of operator 1 is not finite at row 0"));
        std::vector<double> a((size_t)3 * R, 1.0);
        REQUIRE(operator_schedule_validate(3, a.data(), R, ok).empty());
        a[(size_t)2 * R + 1] = bad;
        REQUIRE(contains(operator_schedule_validate(3, a.data(), R, ok), "row 2 is not finite at column 1"));
        std::vector<double> one(R, -1.0);
        REQUIRE(operator_at_validate(one.data(), R, ok).empty());
        one[1] = bad;
        REQUIRE(contains(operator_at_validate(one.data(), R, ok), "not finite at column 1"));
    }
    std::vector<double> a((size_t)3 * R, 0.0);  // (zero and negative coefficients are coefficients)
    a[1] = -2.0;
    REQUIRE(operator_schedule_validate(3, a.data(), R, ok).empty());
    REQUIRE(contains(operator_schedule_validate(3, a.data(), 0, ok), "no operator family set"));
    REQUIRE(contains(operator_schedule_validate(-1, a.data(), R, ok), "count < 0"));
    REQUIRE(operator_schedule_validate(0, nullptr, 0, ok).empty());
    REQUIRE(operator_schedule_validate(5, nullptr, 0, ok).empty());
    REQUIRE(contains(operator_at_validate(nullptr, R, ok), "null coefficients"));
    REQUIRE(contains(operator_at_validate(a.data(), 0, ok), "no operator family set"));
}

void check_padding() {
    g_case = "padding";
    const int count = 3, R = 3;
    std::vector<double> a((size_t)count * R);
    for (size_t k = 0; k < a.size(); ++k) a[k] = 1.0 + (double)k;
    std::vector<double> pad((size_t)count * OPERATOR_MAXR, -7.0);
    operator_schedule_pad(a.data(), count, R, pad.data());
    for (int r = 0; r < count; ++r)
        for (int j = 0; j < OPERATOR_MAXR; ++j) REQUIRE(pad[(size_t)r * OPERATOR_MAXR + j] == (j < R ? a[(size_t)r * R + j] : 0.0));
}

// N = 6 points, two Dirichlet boundary rows, mp = 32: a tridiagonal base (build_ell's image of -L0: rows 0 and 5 two entries wide), a
// tridiagonal L_0 and a 5-point L_1 whose stencil is cut at the ends
void check_image() {
    g_case = "image";
    const int d = 6, nB = 2, mp = 32, bw = 3, R = 2;
    std::vector<int> bcol((size_t)bw * mp, -1);
    std::vector<double> bval((size_t)bw * mp, 0.0);
    std::vector<double> L((size_t)R * d * d, 0.0), e((size_t)R * d);
    for (int i = 0; i < d; ++i) {
        int s = 0;
        for (int k = 0; k < d; ++k) {
            if (std::abs(i - k) <= 1) {
                L[((size_t)0 * d + i) * d + k] = i == k ? -2.0 : 1.0;
                bcol[(size_t)s * mp + i] = k, bval[(size_t)s * mp + i] = i == k ? 0.1 : -0.05, ++s;
            }
            if (std::abs(i - k) <= 2 && i != k) L[((size_t)1 * d + i) * d + k] = 0.25 * (k - i);  // (no diagonal entry: G)
        }
        e[i] = 0.01 * (i + 1), e[(size_t)d + i] = 0.002 * (i + 1);
    }
    bcol[(size_t)0 * mp + d] = 0, bval[(size_t)0 * mp + d] = 1.0;          // boundary rows: u_0, u_5
    bcol[(size_t)0 * mp + d + 1] = d - 1, bval[(size_t)0 * mp + d + 1] = 1.0;
    const OperatorImageHost h = operator_family_image(bcol, bval, bw, d, mp, R, L.data(), e.data());
    const int w = h.img.w;
    REQUIRE(w == 5);  // wider than the base
    REQUIRE(h.img.col.size() == (size_t)w * mp && h.img.val.size() == (size_t)w * mp && h.img.slot.size() == (size_t)mp);
    REQUIRE(h.planes.size() == (size_t)R * w * mp && h.e.size() == (size_t)R * mp);
    for (int i = 0; i < d; ++i) {
        int s = 0, last = -1;
        for (int k = 0; k < d; ++k) {
            if (std::abs(i - k) > 2) continue;  // the union of the two stencils, the diagonal included
            const size_t at = (size_t)s * mp + i;
            REQUIRE(h.img.col[at] == k && k > last);
            last = k;
            REQUIRE(h.img.val[at] == (std::abs(i - k) <= 1 ? (i == k ? 0.1 : -0.05) : 0.0));  // base values, 0 in an added slot
            REQUIRE(h.planes[(size_t)0 * w * mp + at] == L[((size_t)0 * d + i) * d + k]);
            REQUIRE(h.planes[(size_t)1 * w * mp + at] == L[((size_t)1 * d + i) * d + k]);
            if (k == i) REQUIRE(h.img.slot[i] == s);
            ++s;
        }
        for (; s < w; ++s) {
            REQUIRE(h.img.col[(size_t)s * mp + i] == -1);
            for (int r = 0; r < R; ++r) REQUIRE(h.planes[((size_t)r * w + s) * mp + i] == 0.0);
        }
        REQUIRE(h.e[i] == e[i] && h.e[(size_t)mp + i] == e[(size_t)d + i]);
    }
    for (int i = d; i < mp; ++i) {  // boundary rows and padding: the base image, nothing in the planes
        for (int s = 0; s < w; ++s) {
            const size_t at = (size_t)s * mp + i;
            REQUIRE(h.img.col[at] == (s < bw ? bcol[at] : -1) && h.img.val[at] == (s < bw ? bval[at] : 0.0));
            for (int r = 0; r < R; ++r) REQUIRE(h.planes[((size_t)r * w + s) * mp + i] == 0.0);
        }
        REQUIRE(h.e[i] == 0.0 && h.e[(size_t)mp + i] == 0.0);
        (void)nB;
    }
    // the base has no diagonal entry in a row (an operator whose coefficient was zero at creation): the slot is there all the same
    std::vector<int> ncol((size_t)1 * mp, -1);
    std::vector<double> nval((size_t)1 * mp, 0.0);
    for (int i = 0; i < d; ++i) ncol[i] = (i + 1) % d, nval[i] = 1.0;
    const OperatorImageHost g = operator_family_image(ncol, nval, 1, d, mp, 1, L.data() + (size_t)d * d, e.data());
    for (int i = 0; i < d; ++i) REQUIRE(g.img.col[(size_t)g.img.slot[i] * mp + i] == i);
}

}  // namespace

int main() {
    check_validation();
    check_padding();
    check_image();
    std::puts("operator plan: ok");
    return 0;
}
