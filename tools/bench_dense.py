"""Dense output between grid times on the GPU: median wall-clock ms of synchronised calls, heat problem,
nu = 2, dt = 2^-7, fp64.  One JSON line per measurement (`what` says which):

  bridge_state   `pnmol_bridge_state` (the full covariance at t inside a step) into a preallocated state, against (a) the textbook
                 route on the same states in the same process, `pnmol_state_predict` + `pnmol_smoother_step` over (1 - theta) h,
                 and (b) the same block formula in torch-ROCm (`einsum` over (n, dp, n, dp) views), with the largest relative
                 difference of (b); GB/s counts the minimal traffic 3 Dp^2 * 8 bytes over the wall time of the call
  call           `PDESolution.__call__` with 1 / 100 / 10 000 query times spread over a smoothed solution of --call-steps steps
  smooth         `smooth()` with dense = None / "marginal" / "full", alternating, per step (against the parent commit:
                 tools/ab_smooth.sh)
  interpolate    `pnmol_samples_interpolate` beside `pnmol_samples_step_back` at the same S

    python tools/bench_dense.py --mesh-n 256 512 1024 --reps 7
"""

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pnmol-experiments_amd"))


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--theta", type=float, default=0.37)
    ap.add_argument("--call-n", type=int, default=256, help="mesh size of the __call__ / smooth measurements")
    ap.add_argument("--call-steps", type=int, default=100)
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--only", nargs="+", default=["bridge_state", "call", "smooth", "interpolate"])
    ap.add_argument("--no-torch", action="store_true", help="skip the library path (profiling runs)")
    args = ap.parse_args()
    if not args.no_torch:
        import torch                                    # (before the library: one HIP runtime per process)
    import pnmol
    from pnmol.base.iwp import bridge_coefficients

    dt = 2.0 ** -7

    def problem(N, steps):
        pde = pnmol.pde.examples.heat_1d_discretized(dx=1.0 / (N - 1), tmax=steps * dt, diffusion_rate=0.05,
                                                     kernel=pnmol.kernels.SquareExponential(), bcond="dirichlet")
        solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
        return solver, solver.solve(pde)

    for N in args.mesh_n if "bridge_state" in args.only else ():
        solver, sol = problem(N, 3)
        ssol = solver.smooth(sol, dense="full")
        flt = sol._ys[-1].device_state.filter
        lib, ctx = flt.lib, flt.ctx
        n, d, dp = flt.n, flt.d, flt.dims()["dp"]
        k, th = 1, args.theta
        br, sk, sn, fk = ssol.bridges[k], ssol._ys[k].device_state, ssol._ys[k + 1].device_state, sol._ys[k].device_state
        t = sol.t[k] + th * dt
        out, pred, tb = flt.new_state(), flt.new_state(), flt.new_state()

        def bridge():
            ctx.check(lib.pnmol_bridge_state(br.handle, sk.handle, sn.handle, float(t), out.handle), "pnmol_bridge_state")
            ctx.synchronize()

        def textbook():
            ctx.check(lib.pnmol_state_predict(flt.handle, fk.handle, th * dt, pred.handle), "pnmol_state_predict")
            ctx.check(lib.pnmol_smoother_step(flt.handle, pred.handle, sn.handle, (1 - th) * dt, tb.handle), "pnmol_smoother_step")

        ms_b, ms_t = _median_ms(bridge, args.reps), _median_ms(textbook, args.reps)
        Dp = n * dp
        P_b, P_t = out.cov(), tb.cov()
        rec = {"what": "bridge_state", "N": N, "nu": args.nu, "D": n * d, "bridge_ms": round(ms_b, 4),
               "textbook_ms": round(ms_t, 4), "min_bytes": 3 * Dp * Dp * 8,
               "bridge_GBps_wall": round(3 * Dp * Dp * 8 / (ms_b * 1e-3) / 1e9, 1),
               "rel_diff_textbook": float(np.abs(P_b - P_t).max() / np.abs(P_t).max())}
        if not args.no_torch:
            dev = torch.device("cuda")
            s, _ = solver.iwp.nordsieck_preconditioner_1d_raw(dt)
            sc = np.repeat(s, d)
            perm = np.array([j * n + q for q in range(n) for j in range(d)])   # derivative-major <- point-major
            frame = lambda P: np.ascontiguousarray((P[np.ix_(perm, perm)] / np.outer(sc, sc)).reshape(n, d, n, d))
            tt = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
            Pl, Pr = tt(frame(sk.cov())), tt(frame(sn.cov()))
            # C_k through the bridge's own product is not exposed; the library path gets the cross-covariance of the textbook
            # pass over the whole step instead: G_k Ps_{k+1} with G_k = P_k A^T (P-)^-1 (float64 NumPy, outside the timing)
            import scipy.linalg
            A1 = np.flip(scipy.linalg.pascal(n, kind="lower")).astype(np.float64)
            Q1 = np.flip(scipy.linalg.hilbert(n))
            A, Q = np.kron(A1, np.eye(d)), np.kron(Q1, solver._gram)
            Pk = frame(fk.cov()).reshape(n * d, n * d)
            G = scipy.linalg.cho_solve(scipy.linalg.cho_factor(A @ Pk @ A.T + Q, lower=True), A @ Pk).T
            C = tt((G @ frame(sn.cov()).reshape(n * d, n * d)).reshape(n, d, n, d))
            Bm, Bp, Qb = (tt(x) for x in bridge_coefficients(th, args.nu))
            Kt = tt(solver._gram)

            def lib_state():
                X = torch.einsum("ac,cjek,be->ajbk", Bm, C, Bp)
                R = (torch.einsum("ac,cjek,be->ajbk", Bm, Pl, Bm) + torch.einsum("ac,cjek,be->ajbk", Bp, Pr, Bp) + X
                     + X.permute(2, 3, 0, 1) + torch.einsum("ab,jk->ajbk", Qb, Kt))
                torch.cuda.synchronize()
                return R

            rec["torch_ms"] = round(_median_ms(lib_state, args.reps), 4)
            R = lib_state().cpu().numpy().reshape(n * d, n * d)
            rec["rel_diff_torch"] = float(np.abs(frame(P_b).reshape(n * d, n * d) - R).max() / np.abs(R).max())
        print(json.dumps(rec), flush=True)
        del ssol, sol, out, pred, tb

    if "call" in args.only or "smooth" in args.only:
        solver, sol = problem(args.call_n, args.call_steps)
        T = len(sol.t) - 1
    if "smooth" in args.only:
        solver.smooth(sol, dense="full")                    # workspace + first launches
        res = {None: [], "marginal": [], "full": []}
        for _ in range(args.reps):
            for mode in res:
                t0 = time.perf_counter()
                s = solver.smooth(sol, dense=mode)
                res[mode].append(time.perf_counter() - t0)
                del s
        med = {m: 1e3 * float(np.median(v)) / T for m, v in res.items()}
        spread = {m: 1e3 * (max(v) - min(v)) / T for m, v in res.items()}
        flt = sol._ys[-1].device_state.filter
        dp = flt.dims()["dp"]
        print(json.dumps({"what": "smooth", "N": args.call_n, "steps": T, "none_ms_per_step": round(med[None], 4),
                          "marginal_ms_per_step": round(med["marginal"], 4), "full_ms_per_step": round(med["full"], 4),
                          "none_spread_ms_per_step": round(spread[None], 4),
                          "marginal_bytes_per_step": (3 * flt.n ** 2 + 2 * flt.n + 1) * dp * 8,
                          "full_extra_bytes_per_step": (flt.n * dp) ** 2 * 8}), flush=True)
    if "call" in args.only:
        ssol = solver.smooth(sol)
        rng = np.random.default_rng(0)
        for nq in (1, 100, 10000):
            ts = rng.uniform(sol.t[0], sol.t[-1], nq)
            touched = len(np.unique(np.searchsorted(sol.t, ts, side="right") - 1))
            ms = _median_ms(lambda: ssol(ts), args.reps)
            # the split: time inside `pnmol_bridge_eval` (table upload, launch, read-out, synchronisation) against the host side
            # of `__call__` (grouping, scatter into the result); kernel and copy times are in the profiler's statistics
            inside = [0.0]
            orig = pnmol._hip.Bridge.eval

            def timed(self, tq):
                t0 = time.perf_counter()
                r = orig(self, tq)
                inside[0] += time.perf_counter() - t0
                return r

            pnmol._hip.Bridge.eval = timed
            try:
                for _ in range(args.reps):
                    ssol(ts)
            finally:
                pnmol._hip.Bridge.eval = orig
            print(json.dumps({"what": "call", "N": args.call_n, "steps": T, "queries": nq, "intervals_touched": touched,
                              "ms": round(ms, 4), "ms_per_interval": round(ms / touched, 4),
                              "ms_in_bridge_eval": round(1e3 * inside[0] / args.reps, 4),
                              "bytes_back": 2 * nq * ssol.mean.shape[1] * ssol.mean.shape[2] * 8}), flush=True)
        del ssol
    if "interpolate" in args.only:
        for N in args.mesh_n:
            solver, sol = problem(N, 3)
            flt = sol._ys[-1].device_state.filter
            a, b = sol._ys[-2].device_state, sol._ys[-1].device_state
            for S in args.samples:
                right, left, mid = flt.new_samples(S), flt.new_samples(S), flt.new_samples(S)
                right.draw(b, seed=1, step_index=1)
                left.draw(b, seed=1, step_index=1)

                def back():
                    left.draw(b, seed=1, step_index=1)
                    t0 = time.perf_counter()
                    left.step_back(a, dt, seed=1, step_index=0)
                    return time.perf_counter() - t0

                back()
                ms_back = 1e3 * float(np.median([back() for _ in range(args.reps)]))
                ms_int = _median_ms(lambda: mid.interpolate(left, right, a.t + 0.4 * dt, seed=1, step_index=5), args.reps)
                print(json.dumps({"what": "interpolate", "N": N, "S": S, "interpolate_ms": round(ms_int, 4),
                                  "step_back_ms": round(ms_back, 4)}), flush=True)
                del right, left, mid


if __name__ == "__main__":
    main()
