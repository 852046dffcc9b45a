// The host side of the sensor plan (csrc/pnmol_observe_plan.hpp) on its own: built with -fsanitize=address,undefined and run by
// tests/test_observe_plan_host.py.  Checks the entry -> step mapping for split calls and a runt last step, every refusal of the
// walk and of the validation, and that padding leaves zeros; exits non-zero on the first violation.
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "pnmol_observe_plan.hpp"

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

// grid times as the loop accumulates them
std::vector<double> grid(double t0, int k, double dt) {
    std::vector<double> ts{t0};
    for (int j = 0; j < k; ++j) ts.push_back(ts.back() + dt);
    return ts;
}

ObservePlan make_plan(const std::vector<double>& times, int q, int ds, int dp, bool noisy, bool single_workgroup = true) {
    std::vector<double> C((size_t)q * ds), R((size_t)q * q, 0.0), y(times.size() * (size_t)q);
    for (size_t e = 0; e < C.size(); ++e) C[e] = 1.0 + (double)e;
    for (int r = 0; r < q; ++r)
        for (int c = 0; c <= r; ++c) R[(size_t)r * q + c] = 0.5 + r + 0.25 * c;
    for (size_t e = 0; e < y.size(); ++e) y[e] = -1.0 - (double)e;
    REQUIRE(observe_plan_validate((int)times.size(), times.data(), q, ds, C.data(), noisy ? R.data() : nullptr, y.data()).empty());
    ObservePlan p;
    observe_plan_fill(&p, (int)times.size(), times.data(), q, ds, dp, observe_plan_qp(q, single_workgroup), C.data(),
                      noisy ? R.data() : nullptr, y.data());
    return p;
}

void check_padding() {
    g_case = "padding";
    REQUIRE(observe_plan_qp(1, true) == 32 && observe_plan_qp(32, true) == 32 && observe_plan_qp(33, true) == 64);
    REQUIRE(observe_plan_qp(64, true) == 64 && observe_plan_qp(65, true) == 96 && observe_plan_qp(576, true) == 576);
    REQUIRE(observe_plan_qp(1, false) == 64 && observe_plan_qp(32, false) == 64 && observe_plan_qp(33, false) == 64);
    REQUIRE(observe_plan_qp(65, false) == 96);
    for (int q : {1, 3, 32, 33}) {
        const int ds = 40, dp = 64;
        for (int variant = 0; variant < 4; ++variant) {  // noisy or not, on either padding (32 or 64 columns for q <= 32)
            const bool noisy = variant & 1;
            const ObservePlan p = make_plan({0.25, 0.5, 0.75}, q, ds, dp, noisy, (variant & 2) != 0);
            REQUIRE(p.qp == ((q <= 32 && (variant & 2)) ? 32 : 64));
            const int qp = p.qp;
            REQUIRE(p.nobs == 3 && p.q == q && p.next == 0 && p.pending() && p.noisy == noisy);
            REQUIRE(p.C.size() == (size_t)qp * dp && p.R.size() == (size_t)qp * qp && p.y.size() == (size_t)3 * qp);
            for (int r = 0; r < qp; ++r)
                for (int j = 0; j < dp; ++j)
                    REQUIRE(p.C[(size_t)r * dp + j] == ((r < q && j < ds) ? 1.0 + (double)(r * ds + j) : 0.0));
            for (int r = 0; r < qp; ++r)
                for (int c = 0; c < qp; ++c)
                    REQUIRE(p.R[(size_t)r * qp + c] == ((noisy && r < q && c <= r) ? 0.5 + r + 0.25 * c : 0.0));
            for (int i = 0; i < 3; ++i)
                for (int r = 0; r < qp; ++r) REQUIRE(p.y[(size_t)i * qp + r] == (r < q ? -1.0 - (double)(i * q + r) : 0.0));
            for (const auto& res : p.results) REQUIRE(!res.applied && res.bad_pivot == -1);
        }
    }
}

void check_mapping() {
    g_case = "mapping";
    const double dt = 1.0 / 128.0, t0 = 0.1;
    const auto ts = grid(t0, 12, dt);
    // data behind the steps 1, 2, 7, 12 (1-based) of twelve
    ObservePlan p = make_plan({ts[1], ts[2], ts[7], ts[12]}, 3, 32, 32, true);
    std::vector<int> map;
    int count = 0;
    std::string err;
    REQUIRE(observe_plan_walk(p, t0, 12, dt, &map, &count, &err) == 0 && count == 4 && map.size() == 12);
    for (int j = 0; j < 12; ++j) REQUIRE(map[j] == (j == 0 ? 0 : j == 1 ? 1 : j == 6 ? 2 : j == 11 ? 3 : -1));
    REQUIRE(p.next == 0);  // (the walk touches nothing)
    // split calls: 5 steps, then 7 from the time the first call reached
    REQUIRE(observe_plan_walk(p, t0, 5, dt, &map, &count, &err) == 0 && count == 2 && map.size() == 5);
    REQUIRE(map[0] == 0 && map[1] == 1 && map[2] == -1 && map[3] == -1 && map[4] == -1);
    observe_plan_advance(&p, count);
    REQUIRE(p.next == 2 && p.pending());
    REQUIRE(observe_plan_walk(p, ts[5], 7, dt, &map, &count, &err) == 0 && count == 2);
    for (int j = 0; j < 7; ++j) REQUIRE(map[j] == (j == 1 ? 2 : j == 6 ? 3 : -1));
    observe_plan_advance(&p, count);
    REQUIRE(p.next == 4 && !p.pending());
    REQUIRE(observe_plan_walk(p, ts[12], 3, dt, &map, &count, &err) == 0 && count == 0 && map == std::vector<int>(3, -1));
    observe_plan_advance(&p, 5);
    REQUIRE(p.next == 4);
    // an entry up to 16 ulp off its grid time is that grid time; every step carries data
    std::vector<double> all(ts.begin() + 1, ts.end());
    all[3] *= 1.0 + 4 * std::numeric_limits<double>::epsilon();
    ObservePlan pe = make_plan(all, 1, 32, 32, false);
    REQUIRE(observe_plan_walk(pe, t0, 12, dt, &map, &count, &err) == 0 && count == 12);
    for (int j = 0; j < 12; ++j) REQUIRE(map[j] == j);
    // a runt last step: six steps of dt, then one of 0.5 dt in a call of its own; data at step 6 and at tmax
    g_case = "runt step";
    const auto t6 = grid(0.0, 6, dt);
    const double tmax = 6.5 * dt, runt = tmax - t6[6];
    ObservePlan pr = make_plan({t6[6], tmax}, 2, 32, 32, true);
    REQUIRE(observe_plan_walk(pr, 0.0, 6, dt, &map, &count, &err) == 0 && count == 1 && map[5] == 0);
    observe_plan_advance(&pr, count);
    REQUIRE(observe_plan_walk(pr, t6[6], 1, runt, &map, &count, &err) == 0 && count == 1 && map[0] == 1);
    // entries behind the call stay pending
    ObservePlan pl = make_plan({ts[8]}, 2, 32, 32, true);
    REQUIRE(observe_plan_walk(pl, t0, 5, dt, &map, &count, &err) == 0 && count == 0 && pl.pending());
}

void check_refusals() {
    g_case = "walk refusals";
    const double dt = 1.0 / 16.0, t0 = 1.0;
    const auto ts = grid(t0, 8, dt);
    std::vector<int> map;
    int count = 0;
    std::string err;
    ObservePlan inside = make_plan({ts[2], ts[4] + 0.25 * dt}, 2, 32, 32, true);
    REQUIRE(observe_plan_walk(inside, t0, 8, dt, &map, &count, &err) == -1);
    REQUIRE(contains(err, "entry 1") && contains(err, "strictly between") && contains(err, "step 4"));
    REQUIRE(observe_plan_walk(inside, t0, 4, dt, &map, &count, &err) == 0 && count == 1);  // (the call ends in front of it)
    ObservePlan before = make_plan({ts[0] - dt, ts[3]}, 2, 32, 32, true);
    REQUIRE(observe_plan_walk(before, t0, 8, dt, &map, &count, &err) == -1 && contains(err, "entry 0") && contains(err, "before"));
    ObservePlan at = make_plan({ts[0], ts[3]}, 2, 32, 32, true);
    REQUIRE(observe_plan_walk(at, t0, 8, dt, &map, &count, &err) == -1 && contains(err, "entry 0") && contains(err, "never applied"));
    observe_plan_advance(&at, 1);  // applied by pnmol_state_observe_planned
    REQUIRE(observe_plan_walk(at, t0, 8, dt, &map, &count, &err) == 0 && count == 1 && map[2] == 1);
    ObservePlan twice = make_plan({ts[3], ts[3] * (1.0 + 2 * std::numeric_limits<double>::epsilon())}, 2, 32, 32, true);
    REQUIRE(observe_plan_walk(twice, t0, 8, dt, &map, &count, &err) == -1 && contains(err, "entry 1"));
    // by more than 16 ulp off the grid: inside a step
    ObservePlan off = make_plan({ts[3] * (1.0 + 1e-9)}, 2, 32, 32, true);
    REQUIRE(observe_plan_walk(off, t0, 8, dt, &map, &count, &err) == -1 && contains(err, "strictly between"));

    g_case = "validation";
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int q = 2, ds = 4;
    const std::vector<double> t{0.5, 1.0}, C(q * ds, 1.0), R{0.1, 0.0, 0.05, 0.2}, y(2 * q, 1.0);
    auto v = [&](const std::vector<double>& tt, int qq, const std::vector<double>& CC, const double* RR, const std::vector<double>& yy) {
        return observe_plan_validate((int)tt.size(), tt.data(), qq, ds, CC.data(), RR, yy.data());
    };
    REQUIRE(v(t, q, C, R.data(), y).empty() && v(t, q, C, nullptr, y).empty());
    REQUIRE(observe_plan_validate(0, t.data(), q, ds, C.data(), R.data(), y.data()).empty());      // clears
    REQUIRE(observe_plan_validate(2, nullptr, q, ds, C.data(), R.data(), y.data()).empty());       // clears
    REQUIRE(contains(v(t, 0, C, R.data(), y), "q = 0") && contains(v(t, ds + 1, C, R.data(), y), "d_state"));
    REQUIRE(contains(v({1.0, 0.5}, q, C, R.data(), y), "strictly increasing"));
    REQUIRE(contains(v({0.5, 0.5}, q, C, R.data(), y), "strictly increasing"));
    REQUIRE(contains(v({0.5, nan}, q, C, R.data(), y), "not finite") && contains(v({0.5, inf}, q, C, R.data(), y), "not finite"));
    std::vector<double> Cb = C, yb = y, Rb = R, Ru = R;
    Cb[5] = inf, yb[3] = nan, Rb[2] = nan, Ru[1] = 1e-3;
    REQUIRE(contains(v(t, q, Cb, R.data(), y), "C has"));
    REQUIRE(contains(v(t, q, C, R.data(), yb), "y has") && contains(v(t, q, C, R.data(), yb), "entry 1"));
    REQUIRE(contains(v(t, q, C, Rb.data(), y), "R has"));
    REQUIRE(contains(v(t, q, C, Ru.data(), y), "not lower triangular"));
}

}  // namespace

int main() {
    check_padding();
    check_mapping();
    check_refusals();
    std::printf("observe plan: ok\n");
    return 0;
}
