// Host-side walk through the C ABI of libpnmol_hip under AddressSanitizer + UBSan, against tests/asan/hip_mock.c (no GPU:
// kernels do not run, results are zeros).  Every call's return code is printed; the run passes when the sanitizers stay
// silent and the process exits 0.  Exercises: descriptor validation, filter/state creation for all sizes of n, layout
// conversions of set/get (the index arithmetic), ELL rebuilds (set_operator, dense and wide rows), error model, step and
// steps bookkeeping (graph capture path included), the lifetime rule in every wrong order, the square-root entry points,
// and (walk_posterior) the smoother with and without bridges, bridge slabs, dense output, joint draws and their lifetime rule.
// Against the mock a sweep's info word stays as the host set it ("no failure"), so those success paths are reachable.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pnmol_hip.h"
#include "pnmol_sqrt.h"

static int fails = 0;
#define EXPECT(call, want)                                                              \
    do {                                                                                \
        const int rc__ = (call);                                                        \
        std::printf("%-70s -> %d%s\n", #call, rc__, rc__ == (want) ? "" : "   UNEXPECTED"); \
        if (rc__ != (want)) ++fails;                                                    \
    } while (0)
#define ANY(call)                                        \
    do {                                                 \
        const int rc__ = (call);                         \
        std::printf("%-70s -> %d\n", #call, rc__);       \
    } while (0)

// a heat-like problem of d points with two boundary rows
struct Problem {
    static constexpr int nB = 2;
    std::vector<double> L, B, E, R, Gm;
    pnmol_filter_desc desc{};
    Problem(int d, int nu) : L(d * d, 0.0), B(nB * d, 0.0), E(d * d, 0.0), R(nB * nB, 0.0), Gm(d * d, 0.0) {
        for (int i = 0; i < d; ++i) {
            L[i * d + i] = -2.0;
            if (i) L[i * d + i - 1] = 1.0;
            if (i + 1 < d) L[i * d + i + 1] = 1.0;
            E[i * d + i] = 1e-3;
            for (int k = 0; k <= i; ++k) Gm[i * d + k] = (i == k) ? 1.0 : 0.1 / (1 + i - k);
        }
        B[0] = 1.0, B[nB * d - 1] = 1.0;
        desc.d = d, desc.num_derivatives = nu, desc.nB = nB, desc.L = L.data(), desc.B = B.data();
        desc.E_sqrtm = E.data(), desc.R_sqrtm = R.data(), desc.Gamma = Gm.data();
    }
};

// Smoother, dense output and joint draws on the filter f of n x d components; filt is a state of f at t = 0.25.
static void walk_posterior(pnmol_ctx* ctx, pnmol_filter* f, const pnmol_state* filt, int n, int d) {
    const int D = n * d, S = 5;
    const double t0 = 0.25, dt = 0.1;
    std::vector<double> mean(D, 0.5), cov((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i) cov[(size_t)i * D + i] = 2.0 + i;
    pnmol_state *nxt = nullptr, *out = nullptr, *mid = nullptr;
    EXPECT(pnmol_state_create(f, &nxt), 0);
    EXPECT(pnmol_state_create(f, &out), 0);
    EXPECT(pnmol_state_create(f, &mid), 0);
    EXPECT(pnmol_state_set(nxt, t0 + dt, mean.data(), cov.data()), 0);
    // smoother step, without and with a bridge
    EXPECT(pnmol_smoother_step(nullptr, filt, nxt, dt, out), -1);
    EXPECT(pnmol_smoother_step(f, filt, nxt, dt, nxt), -1);   // aliasing
    EXPECT(pnmol_smoother_step(f, filt, nxt, 0.0, out), -1);  // dt <= 0
    EXPECT(pnmol_smoother_step(f, filt, nxt, dt, out), 0);
    pnmol_bridge *b0 = nullptr, *b1 = nullptr;
    EXPECT(pnmol_smoother_step_bridge(f, filt, nxt, dt, out, 0, nullptr), -1);
    EXPECT(pnmol_smoother_step_bridge(f, filt, nxt, -dt, out, 0, &b0), -1);
    EXPECT(pnmol_smoother_step_bridge(f, filt, nxt, dt, out, 0, &b0), 0);
    EXPECT(pnmol_smoother_step_bridge(f, filt, nxt, dt, out, 1, &b1), 0);
    EXPECT(pnmol_filter_destroy(f), -1);  // bridges alive
    double bt = 0.0, bdt = 0.0;
    int full = -1;
    EXPECT(pnmol_bridge_get_interval(b1, &bt, &bdt, &full), 0);
    EXPECT(pnmol_bridge_get_interval(b0, nullptr, nullptr, &full), 0);
    EXPECT(pnmol_bridge_get_interval(nullptr, &bt, &bdt, &full), -1);
    const double tq[3] = {t0, t0 + 0.3 * dt, t0 + dt}, tbad[1] = {t0 + 2 * dt};
    std::vector<double> qm((size_t)3 * D), qs((size_t)3 * D);
    EXPECT(pnmol_bridge_eval(b0, 3, tq, qm.data(), qs.data()), 0);
    EXPECT(pnmol_bridge_eval(b1, 3, tq, nullptr, qs.data()), 0);
    EXPECT(pnmol_bridge_eval(b0, 1, tbad, qm.data(), qs.data()), -1);
    EXPECT(pnmol_bridge_eval(b0, 0, tq, qm.data(), qs.data()), -1);
    EXPECT(pnmol_bridge_eval(nullptr, 3, tq, qm.data(), qs.data()), -1);
    EXPECT(pnmol_bridge_state(b1, out, nxt, t0 + 0.5 * dt, mid), 0);
    EXPECT(pnmol_bridge_state(b0, out, nxt, t0 + 0.5 * dt, mid), -1);  // made without keep_full
    EXPECT(pnmol_bridge_state(b1, out, nxt, t0, mid), -1);             // not strictly inside
    EXPECT(pnmol_bridge_state(b1, nxt, out, t0 + 0.5 * dt, mid), -1);  // states at the wrong ends
    EXPECT(pnmol_bridge_state(b1, out, nxt, t0 + 0.5 * dt, out), -1);  // aliasing
    // more bridges than one slab holds (64), destroyed in creation order, then another lot in reverse order
    for (int reverse = 0; reverse < 2; ++reverse) {
        std::vector<pnmol_bridge*> many(70, nullptr);
        int bad = 0;
        for (auto& b : many) bad += pnmol_smoother_step_bridge(f, filt, nxt, dt, out, 0, &b) != 0;
        for (int i = 0; i < 70; ++i) bad += pnmol_bridge_destroy(many[reverse ? 69 - i : i]) != 0;
        EXPECT(bad, 0);
    }
    EXPECT(pnmol_bridge_destroy(b1), 0);
    EXPECT(pnmol_bridge_destroy(b0), 0);
    EXPECT(pnmol_bridge_destroy(nullptr), -1);
    // prediction behind a state
    const double dq[3] = {0.0, 0.5 * dt, dt}, dneg[1] = {-dt};
    EXPECT(pnmol_state_predict(f, filt, dt, mid), 0);
    EXPECT(pnmol_state_predict(f, mid, dt, mid), -1);   // aliasing
    EXPECT(pnmol_state_predict(f, filt, -dt, mid), -1);
    EXPECT(pnmol_state_predict_marginals(f, filt, 3, dq, qm.data(), qs.data()), 0);
    EXPECT(pnmol_state_predict_marginals(f, mid, 3, dq, qm.data(), nullptr), 0);  // a state in a Nordsieck frame
    EXPECT(pnmol_state_predict_marginals(f, filt, 1, dneg, qm.data(), qs.data()), -1);
    EXPECT(pnmol_state_predict_marginals(f, filt, 0, dq, qm.data(), qs.data()), -1);
    EXPECT(pnmol_state_predict_marginals(f, filt, 3, dq, nullptr, nullptr), -1);
    // joint draws: terminal draw at nxt, one step back to filt, draws in between and behind
    pnmol_samples *x = nullptr, *xr = nullptr, *z = nullptr, *z2 = nullptr;
    std::vector<double> xi((size_t)S * 2 * D, 0.25), got((size_t)S * D);
    double ts = 0.0;
    EXPECT(pnmol_samples_create(f, 0, &x), -1);
    EXPECT(pnmol_samples_create(nullptr, S, &x), -1);
    EXPECT(pnmol_samples_create(f, S, &x), 0);
    EXPECT(pnmol_samples_create(f, S, &z), 0);
    EXPECT(pnmol_filter_destroy(f), -1);  // sample blocks alive
    EXPECT(pnmol_samples_get(x, got.data()), -1);             // holds no draw yet
    EXPECT(pnmol_samples_get_time(x, &ts), -1);
    EXPECT(pnmol_samples_step_back(x, filt, dt, nullptr, 1, 0, 1.0), -1);
    EXPECT(pnmol_samples_draw(x, nullptr, nullptr, 1, 0, 1.0), -1);
    EXPECT(pnmol_samples_draw(x, nxt, xi.data(), 0, 0, 1.0), 0);   // host noise
    EXPECT(pnmol_samples_draw(x, nxt, nullptr, 1, 0, 1.0), 0);     // device generator
    EXPECT(pnmol_samples_clone(x, &xr), 0);
    EXPECT(pnmol_samples_clone(nullptr, &z2), -1);
    EXPECT(pnmol_samples_step_back(x, filt, 0.0, nullptr, 1, 1, 1.0), -1);
    EXPECT(pnmol_samples_step_back(x, filt, dt, nullptr, 1, 1, 1.0), 0);
    EXPECT(pnmol_samples_step_back(x, filt, dt, nullptr, 1, 2, 1.0), -1);  // out of order: the block is at filt's time now
    EXPECT(pnmol_samples_draw(x, nxt, nullptr, 1, 0, 1.0), 0);
    EXPECT(pnmol_samples_step_back(x, filt, dt, xi.data(), 0, 0, 1.0), 0);  // host noise
    EXPECT(pnmol_samples_interpolate(z, x, xr, t0 + 0.5 * dt, nullptr, 1, 3, 1.0), 0);
    EXPECT(pnmol_samples_interpolate(z, x, xr, t0 + 0.5 * dt, xi.data(), 0, 0, 1.0), 0);
    EXPECT(pnmol_samples_interpolate(z, xr, nullptr, t0 + 2 * dt, nullptr, 1, 4, 1.0), 0);  // behind the last block
    EXPECT(pnmol_samples_interpolate(z, x, xr, t0 + 2 * dt, nullptr, 1, 3, 1.0), -1);      // not strictly between
    EXPECT(pnmol_samples_interpolate(x, x, xr, t0 + 0.5 * dt, nullptr, 1, 3, 1.0), -1);    // aliasing
    EXPECT(pnmol_samples_get(z, got.data()), 0);
    EXPECT(pnmol_samples_get(x, nullptr), -1);
    EXPECT(pnmol_samples_get_time(z, &ts), 0);
    EXPECT(pnmol_samples_destroy(z), 0);
    EXPECT(pnmol_samples_destroy(xr), 0);
    EXPECT(pnmol_samples_destroy(x), 0);
    EXPECT(pnmol_samples_destroy(nullptr), -1);
    std::vector<double> noise(4 * 6);
    EXPECT(pnmol_sample_noise(ctx, 1, 2, 4, 6, noise.data()), 0);
    EXPECT(pnmol_sample_noise(ctx, 1, 2, 0, 6, noise.data()), -1);
    EXPECT(pnmol_sample_noise(nullptr, 1, 2, 4, 6, noise.data()), -1);
    EXPECT(pnmol_state_destroy(mid), 0);
    EXPECT(pnmol_state_destroy(out), 0);
    EXPECT(pnmol_state_destroy(nxt), 0);
}

int main() {
    pnmol_ctx* ctx = nullptr;
    EXPECT(pnmol_ctx_create(0, &ctx), 0);
    EXPECT(pnmol_ctx_create(5, nullptr), -1);
    for (int nu = 1; nu <= 3; ++nu)
        for (int d : {5, 33, 70}) {
            const int nB = Problem::nB, n = nu + 1, D = n * d;
            Problem pb(d, nu);
            pnmol_filter_desc& desc = pb.desc;
            const std::vector<double>& L = pb.L;
            pnmol_filter* f = nullptr;
            desc.dtype = 3;
            EXPECT(pnmol_filter_create(ctx, &desc, &f), -1);
            desc.dtype = 0;
            desc.d = 0;
            EXPECT(pnmol_filter_create(ctx, &desc, &f), -1);
            desc.d = d;
            EXPECT(pnmol_filter_create(ctx, &desc, &f), 0);
            int dd, nn, mm, dp, mp, kern, home;
            EXPECT(pnmol_filter_dims(f, &dd, &nn, &mm, &dp, &mp), 0);
            EXPECT(pnmol_filter_sweep_layout(f, &kern, &home), 0);
            pnmol_state *s0 = nullptr, *s1 = nullptr, *s2 = nullptr;
            EXPECT(pnmol_state_create(f, &s0), 0);
            EXPECT(pnmol_state_create(f, &s1), 0);
            std::vector<double> mean(n * d), cov((size_t)D * D, 0.0), out((size_t)D * D), v(n * d);
            for (int i = 0; i < n * d; ++i) mean[i] = std::sin(0.1 * i);
            for (int i = 0; i < D; ++i) cov[(size_t)i * D + i] = 1.0 + i;
            EXPECT(pnmol_state_set(s0, 0.25, mean.data(), cov.data()), 0);
            EXPECT(pnmol_state_set_sqrtm(s0, 0.25, mean.data(), cov.data()), 0);
            EXPECT(pnmol_state_clone(s0, &s2), 0);
            EXPECT(pnmol_state_get_mean(s0, v.data()), 0);
            EXPECT(pnmol_state_get_cov(s0, out.data()), 0);
            EXPECT(pnmol_state_get_marginal_var(s0, v.data()), 0);
            ANY(pnmol_state_get_cov_sqrtm(s0, out.data()));     // (mock: the factorisation kernel does not run)
            pnmol_step_out so{};
            std::vector<double> err(d);
            EXPECT(pnmol_filter_step(f, s0, 0.1, s0, &so, err.data()), -1);   // aliasing
            EXPECT(pnmol_filter_step(f, s0, -1.0, s1, &so, err.data()), -1);  // dt <= 0
            ANY(pnmol_filter_step(f, s0, 0.1, s1, &so, err.data()));          // (mock: info word 0 -> "not positive definite")
            ANY(pnmol_filter_prepare_error_model(f, 0.1));
            std::vector<double> sq((size_t)(d + nB) * (d + nB), 0.0), sqd(d + nB, 1.0);
            EXPECT(pnmol_filter_set_error_model(f, 0.1, sq.data(), sqd.data()), 0);
            std::vector<double> m_at(d), Mdense((size_t)d * d, 0.5), shift(d, 0.1);
            EXPECT(pnmol_filter_predict_mean(f, s0, 0.1, m_at.data()), 0);
            EXPECT(pnmol_filter_set_operator(f, Mdense.data(), shift.data()), 0);   // dense Jacobian: wide ELL, reallocation
            EXPECT(pnmol_filter_set_operator(f, L.data(), nullptr), 0);             // back to the stencil
            walk_posterior(ctx, f, s2, n, d);
            for (int k : {1, 2, 3, 13, 24}) {
                std::vector<double> means((size_t)k * d), stds((size_t)k * d);
                std::vector<pnmol_step_out> infos(k);
                ANY(pnmol_filter_prepare_steps(f, s0, k, 0.05));
                ANY(pnmol_filter_steps(f, s0, k, 0.05, means.data(), stds.data(), infos.data()));
            }
            EXPECT(pnmol_filter_steps(f, s0, 0, 0.05, nullptr, nullptr, nullptr), -1);
            EXPECT(pnmol_filter_steps_begin(f, s0, 4, 0.05), 0);
            EXPECT(pnmol_state_destroy(s0), -1);                 // target of an unfinished steps_begin
            ANY(pnmol_filter_steps_end(f, s0, nullptr, nullptr, nullptr));
            EXPECT(pnmol_filter_steps_end(f, s0, nullptr, nullptr, nullptr), -1);   // nothing pending
            // lifetime rule, every wrong order
            EXPECT(pnmol_ctx_destroy(ctx), -1);
            EXPECT(pnmol_filter_destroy(f), -1);
            EXPECT(pnmol_state_destroy(s0), 0);
            EXPECT(pnmol_state_destroy(s1), 0);
            EXPECT(pnmol_filter_destroy(f), -1);
            EXPECT(pnmol_state_destroy(s2), 0);
            EXPECT(pnmol_filter_destroy(f), 0);
            // the square-root side
            pnmol_sqrt_filter* q = nullptr;
            desc.dtype = 1;  // (fp32 QR form)
            EXPECT(pnmol_sqrt_filter_create(ctx, &desc, &q), 0);
            EXPECT(pnmol_sqrt_filter_destroy(q), 0);
            desc.dtype = 0;
            EXPECT(pnmol_sqrt_filter_create(ctx, &desc, &q), 0);
            EXPECT(pnmol_ctx_destroy(ctx), -1);
            ANY(pnmol_sqrt_filter_set_state(q, 0.0, mean.data(), cov.data()));
            pnmol_step_out qo{};
            ANY(pnmol_sqrt_filter_step(q, 0.1, &qo, err.data()));
            { double tq = 0.0; ANY(pnmol_sqrt_filter_get_state(q, &tq, mean.data(), out.data())); }
            EXPECT(pnmol_sqrt_filter_destroy(q), 0);
            std::vector<double> A((size_t)(2 * D) * D, 0.3), Rr((size_t)D * D);
            ANY(pnmol_qr_r(ctx, A.data(), 2 * D, D, Rr.data()));
            ANY(pnmol_sqrt_propagate_cholesky_factor(ctx, cov.data(), D, D, cov.data(), D, Rr.data()));
        }
    {   // more than 17 column blocks: a backward sampling step runs its main sweep on the side stream
        const int d = 200, nu = 2;
        Problem pb(d, nu);
        pnmol_filter* f = nullptr;
        pnmol_state* s = nullptr;
        EXPECT(pnmol_filter_create(ctx, &pb.desc, &f), 0);
        EXPECT(pnmol_state_create(f, &s), 0);
        std::vector<double> mean((nu + 1) * d, 0.1), cov((size_t)(nu + 1) * d * (nu + 1) * d, 0.0);
        EXPECT(pnmol_state_set(s, 0.25, mean.data(), cov.data()), 0);
        walk_posterior(ctx, f, s, nu + 1, d);
        EXPECT(pnmol_state_destroy(s), 0);
        EXPECT(pnmol_filter_destroy(f), 0);
    }
    EXPECT(pnmol_ctx_destroy(ctx), 0);
    EXPECT(pnmol_filter_destroy(nullptr), -1);
    EXPECT(pnmol_state_destroy(nullptr), -1);
    std::printf("%s (%d unexpected return codes)\n", fails ? "FAILED" : "ok", fails);
    return fails ? 1 : 0;
}
