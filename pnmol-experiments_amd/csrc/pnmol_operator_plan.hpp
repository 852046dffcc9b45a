// pnmol_operator_plan.hpp -- host side of a time-dependent operator M(t) = sum_r a_r(t) L_r (pnmol_filter_set_operator_family,
// pnmol_filter_set_operator_schedule, pnmol_filter_operator_at; pnmol_operator.hip): validation of a family and of a table of
// coefficients, its padded image and the union image of the L_r with its value planes.  The table itself and its cursor are those of
// every table of the loop (pnmol_cursor_plan.hpp).  Nothing of HIP in here: tests/operator_plan_check.cpp builds it on its own under
// the sanitizers.
#pragma once
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "pnmol_cursor_plan.hpp"
#include "pnmol_term_image.hpp"

constexpr int OPERATOR_MAXR = 4;  // (PNMOL_OPERATOR_MAXR, include/pnmol_hip.h)

// what the filter says of itself to the three setters
struct OperatorFilterFacts {
    bool latent = false;        // d_state != d
    bool fp32 = false;
    bool dense_noise = false;   // the measurement noise given at creation is not diagonal
    bool call_running = false;  // between pnmol_filter_steps_begin and pnmol_filter_steps_end
    bool wide_term = false;     // a reaction system or a convection term is set: an image of its own
    bool no_diag = false;       // a row of the operator given at creation has no diagonal entry
    bool replaced = false;      // pnmol_filter_set_operator(_diagonal) has replaced the operator or shift given at creation
};

inline std::string operator_plan_capability(const OperatorFilterFacts& f) {
    if (f.latent) return "a latent-force filter (d_state != d) has no time-dependent operator";
    if (f.fp32) return "an fp32 filter has no time-dependent operator";
    if (f.call_running) return "called between pnmol_filter_steps_begin and pnmol_filter_steps_end";
    return "";
}

// "" or why the arguments of pnmol_filter_set_operator_family are refused.  R = 0 or a NULL argument: clears (refused only inside a
// call).  L: (R, d, d) row-major; e: (R, d), the diagonals of the E_sqrtm_r.
inline std::string operator_family_validate(int R, const double* L, const double* e, int d, const OperatorFilterFacts& f) {
    const std::string cap = operator_plan_capability(f);
    if (!cap.empty()) return cap;
    if (R == 0 || !L || !e) return "";
    if (R < 1 || R > OPERATOR_MAXR) return "R outside [1, 4]";
    if (f.dense_noise) return "the measurement noise given at creation is not diagonal";
    if (f.no_diag) return "a row of the operator given at creation has no diagonal entry";
    if (f.replaced)
        return "the operator given at creation was replaced (pnmol_filter_set_operator, pnmol_filter_set_operator_diagonal): the "
               "family's image and a cleared family start from the creation-time operator and would lose it";
    if (f.wide_term)
        return "a reaction system or a convection term is set (clear it first: both bring a widened image of their own)";
    for (long r = 0; r < R; ++r)
        for (long i = 0; i < d; ++i) {
            for (long k = 0; k < d; ++k)
                if (!std::isfinite(L[(r * d + i) * d + k]))
                    return "operator " + std::to_string(r) + " is not finite at row " + std::to_string(i) + ", column " +
                           std::to_string(k);
            if (!std::isfinite(e[r * d + i]))
                return "the noise diagonal of operator " + std::to_string(r) + " is not finite at row " + std::to_string(i);
        }
    return "";
}

// "" or why a table of coefficients (count, R) row-major is refused.  count = 0 or no table: clears.  R = 0: no family is set.
inline std::string operator_schedule_validate(int count, const double* a, int R, const OperatorFilterFacts& f) {
    const std::string cap = operator_plan_capability(f);
    if (!cap.empty()) return cap;
    if (count < 0) return "count < 0";
    if (count == 0 || !a) return "";
    if (R == 0) return "no operator family set (pnmol_filter_set_operator_family)";
    for (long r = 0; r < count; ++r)
        for (long j = 0; j < R; ++j)
            if (!std::isfinite(a[r * R + j]))
                return "the coefficient of row " + std::to_string(r) + " is not finite at column " + std::to_string(j);
    return "";
}

// "" or why the coefficients of pnmol_filter_operator_at are refused
inline std::string operator_at_validate(const double* a, int R, const OperatorFilterFacts& f) {
    const std::string cap = operator_plan_capability(f);
    if (!cap.empty()) return cap;
    if (!a) return "bad argument (null coefficients)";
    if (R == 0) return "no operator family set (pnmol_filter_set_operator_family)";
    for (long j = 0; j < R; ++j)
        if (!std::isfinite(a[j])) return "the coefficient of row 0 is not finite at column " + std::to_string(j);
    return "";
}

// the table as the device holds it: row stride OPERATOR_MAXR, the padding zero
inline void operator_schedule_pad(const double* a, int count, int R, double* out) {
    for (long r = 0; r < count; ++r)
        for (long j = 0; j < OPERATOR_MAXR; ++j) out[r * OPERATOR_MAXR + j] = j < R ? a[r * R + j] : 0.0;
}

// The union image of a family: the base image (boundary rows, padding and the base values of its own columns) with a slot in every
// PDE row for each column in which any L_r has an entry, and for the diagonal.  Never a function of the coefficients: an operator
// whose coefficient is zero at t0 has its slots all the same.
struct OperatorImageHost {
    TermImageHost img;           // col, val (base values, 0 in an added slot), slot (1 x mp: the diagonal slots), w
    std::vector<double> planes;  // R x w x mp: L_r's value in every slot of a PDE row, 0 elsewhere
    std::vector<double> e;       // R x mp: the noise diagonals, 0 behind d
};

inline OperatorImageHost operator_family_image(const std::vector<int>& bcol, const std::vector<double>& bval, int bw, int d, int mp,
                                               int R, const double* L, const double* e) {
    OperatorImageHost out;
    out.img = build_term_image(bcol, bval, bw, d, mp, 1, false, [=](int i, std::vector<std::pair<int, double>>& add) {
        for (int k = 0; k < d; ++k) {
            bool any = k == i;
            for (int r = 0; r < R && !any; ++r) any = L[((size_t)r * d + i) * d + k] != 0.0;
            if (any) add.emplace_back(k, 0.0);
        }
    });
    const int w = out.img.w;
    out.planes.assign((size_t)R * w * mp, 0.0);
    out.e.assign((size_t)R * mp, 0.0);
    for (int r = 0; r < R; ++r)
        for (int i = 0; i < d; ++i) {
            for (int s = 0; s < w; ++s) {
                const int col = out.img.col[(size_t)s * mp + i];
                if (col >= 0) out.planes[((size_t)r * w + s) * mp + i] = L[((size_t)r * d + i) * d + col];
            }
            out.e[(size_t)r * mp + i] = e[(size_t)r * d + i];
        }
    return out;
}
