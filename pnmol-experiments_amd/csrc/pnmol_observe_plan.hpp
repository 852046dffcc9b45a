// pnmol_observe_plan.hpp -- host side of the sensor plan of the constant-step loop (pnmol_filter_set_observations,
// pnmol_observe.hip): validation, padding of C / R / y, the walk that maps plan entries to the steps of one
// pnmol_filter_steps_begin call (with its refusals), and the cursor.  Nothing of HIP in here: tests/observe_plan_check.cpp builds it
// on its own under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

// two times are the same grid point (dt: the step they are measured against)
inline bool times_agree(double a, double b, double dt) {
    return std::fabs(a - b) <= 16.0 * 2.220446049250313e-16 * std::max({std::fabs(a), std::fabs(b), std::fabs(dt)});
}

inline std::string observe_plan_time(double t) {
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", t);
    return b;
}

constexpr int OBP_NB = 32;  // column padding (the factorisation block)

// padded column count of a q-row update in the loop: what pnmol_state_observe pads to (a multiple of 32, at least 64: the sweep's
// smallest tall shape) -- or, single_workgroup and q <= 32, the 32 columns of the single-workgroup Cholesky route (measured the
// slower one, DESIGN.md section 19: selected by a switch, not by default)
inline int observe_plan_qp(int q, bool single_workgroup) {
    if (q <= OBP_NB && single_workgroup) return OBP_NB;
    return std::max(2 * OBP_NB, (q + OBP_NB - 1) / OBP_NB * OBP_NB);
}

// what an applied update leaves behind: |w|^2, 2 sum log Ls_ii, first bad pivot + 1 (0: none), the sweep's info word (sweep route)
struct ObservePlanResult {
    double mahalanobis = 0.0, logdet = 0.0;
    int bad_pivot = -1;  // -1 ok
    int stuck = 0;       // the sweep's dependency wait timed out
    bool applied = false;
};

struct ObservePlan {
    int nobs = 0, q = 0, qp = 0, ds = 0, dp = 0;
    bool noisy = false;
    int next = 0;                 // cursor: the first entry that has not been applied
    std::vector<double> t;        // nobs
    std::vector<double> C;        // qp x dp: the rows of C (unscaled) padded with zeros
    std::vector<double> R;        // qp x qp: the lower triangle of R padded with zeros (all zero when noise-free)
    std::vector<double> y;        // nobs x qp, padded with zeros
    std::vector<ObservePlanResult> results;  // nobs
    std::vector<int> call_entry;  // the running call: entry behind step j, or -1
    int call_count = 0;           // entries the running call applies
    bool pending() const { return next < nobs; }
};

// "" or why the arguments of pnmol_filter_set_observations are refused (the filter's own checks -- null, fp32 -- are the caller's)
inline std::string observe_plan_validate(int nobs, const double* t, int q, int ds, const double* C, const double* R, const double* y) {
    if (nobs < 1 || !t) return "";  // clears
    if (q < 1 || q > ds) return "q = " + std::to_string(q) + " must lie in [1, d_state = " + std::to_string(ds) + "]";
    if (!C || !y) return "C and y must be given";
    for (int i = 0; i < nobs; ++i) {
        if (!std::isfinite(t[i])) return "time of entry " + std::to_string(i) + " is not finite";
        if (i > 0 && !(t[i] > t[i - 1])) return "times must be strictly increasing (entry " + std::to_string(i) + ")";
    }
    for (size_t e = 0; e < (size_t)q * ds; ++e)
        if (!std::isfinite(C[e])) return "C has an entry that is not finite";
    for (size_t e = 0; e < (size_t)nobs * q; ++e)
        if (!std::isfinite(y[e])) return "y has an entry that is not finite (entry " + std::to_string(e / q) + ")";
    if (R)
        for (int r = 0; r < q; ++r)
            for (int c = 0; c < q; ++c) {
                const double v = R[(size_t)r * q + c];
                if (!std::isfinite(v)) return "R has an entry that is not finite";
                if (c > r && v != 0.0) return "R is not lower triangular";
            }
    return "";
}

// the plan's tables from validated arguments; the cursor goes to entry 0
inline void observe_plan_fill(ObservePlan* p, int nobs, const double* t, int q, int ds, int dp, int qp, const double* C,
                              const double* R, const double* y) {
    *p = ObservePlan{};
    p->nobs = nobs, p->q = q, p->qp = qp, p->ds = ds, p->dp = dp, p->noisy = R != nullptr;
    p->t.assign(t, t + nobs);
    p->C.assign((size_t)qp * dp, 0.0);
    p->R.assign((size_t)qp * qp, 0.0);
    p->y.assign((size_t)nobs * qp, 0.0);
    p->results.assign((size_t)nobs, ObservePlanResult{});
    for (int r = 0; r < q; ++r) {
        for (int j = 0; j < ds; ++j) p->C[(size_t)r * dp + j] = C[(size_t)r * ds + j];
        if (R)
            for (int k = 0; k <= r; ++k) p->R[(size_t)r * qp + k] = R[(size_t)r * q + k];
    }
    for (int i = 0; i < nobs; ++i)
        for (int r = 0; r < q; ++r) p->y[(size_t)i * qp + r] = y[(size_t)i * q + r];
}

// The steps of one call from a state at t0: t = t0; t += dt per step (the accumulation pnmol_filter_steps_end uses).
// entry_of_step[j] = the pending entry whose time agrees with the time behind step j, or -1; *count = how many were mapped.
// -1 with *err naming entry and time when a pending entry lies before t0, at t0 (it was never applied) or strictly between two
// grid times of the call.  Entries behind the last step stay pending.  Touches nothing of the plan.
inline int observe_plan_walk(const ObservePlan& p, double t0, int k, double dt, std::vector<int>* entry_of_step, int* count,
                             std::string* err) {
    entry_of_step->assign((size_t)k, -1);
    *count = 0;
    int i = p.next;
    if (i >= p.nobs) return 0;
    auto name = [&](int e) { return "entry " + std::to_string(e) + " (t = " + observe_plan_time(p.t[e]) + ")"; };
    if (times_agree(p.t[i], t0, dt)) {
        *err = name(i) + " lies at the state's time and was never applied: apply it with pnmol_state_observe_planned first";
        return -1;
    }
    if (p.t[i] < t0) {
        *err = name(i) + " lies before the state's time " + observe_plan_time(t0);
        return -1;
    }
    double t = t0;
    for (int j = 0; j < k && i < p.nobs; ++j) {
        const double tprev = t;
        t += dt;
        if (times_agree(p.t[i], t, dt)) {
            (*entry_of_step)[j] = i++;
            ++*count;
            if (i < p.nobs && times_agree(p.t[i], t, dt)) {
                *err = name(i) + " agrees with the same grid time as the entry before it";
                return -1;
            }
        } else if (p.t[i] < t) {
            *err = name(i) + " lies strictly between the grid times " + observe_plan_time(tprev) + " and " + observe_plan_time(t) +
                   " of this call (step " + std::to_string(j) + ")";
            return -1;
        }
    }
    return 0;
}

// a call that was enqueued has been collected: its entries are applied
inline void observe_plan_advance(ObservePlan* p, int count) { p->next = std::min(p->nobs, p->next + count); }
