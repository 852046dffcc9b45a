"""The filtered trajectory out of the device loop and the backward pass in one call (csrc/pnmol_record.hip, `pnmol_smoother_steps`;
DESIGN.md section 20): ms per step of

  forward   (a) `solve()`: one `attempt_step` per step (a synchronisation, a state allocation and a mean read-back each),
            (b) `solve_on_device()`: the constant-step loop with the recorder set (k_record behind every step),
            (c) `solve_marginals()`: the loop alone (read-outs only; the fused steady-state loop for the linear problem),
  backward  (s) `smooth(sol, dense=None)`: one `pnmol_smoother_step` per step,
            (m) `smooth_marginals(sol)`: the whole pass in one `pnmol_smoother_steps` call,

on a `solve()` solution of the same problem.  Heat (`--problem heat`) and logistic reaction-diffusion (`--problem logistic`, the
recipe of bench.py's semilinear row with the term linearised on the device), nu = 2, dt = 2^-7.  Every figure is the median over
--reps runs of --steps steps, host wall clock around work that ends in a stream synchronisation, after a warm-up run of the same
shape (graph capture, first launches); `spread_ms` holds max - min of the repeats; (b) and (c) also report the device-event time
of their loop (`*_loop_event_ms`: what is left of the wall clock is host work -- for (b) the allocation of the T states, the copy
of the initial state, the read-back of the means and the `PDESolution`).  The initial state is computed once outside
the timed region (`initialize` is O(d^3) host work that all three forward routes share) and every run starts from a copy of it.
One JSON line per problem and size.

--tree PATH measures the package of another checkout of this project (one that was built there), e.g. an export of the parent
commit: what that tree lacks ((b), (m)) is left out of its lines.

    python tools/bench_record.py --problem heat logistic --sizes 256 512 --steps 40 --reps 7
"""

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent


def problem(name, N, tmax, pnmol):
    from pnmol.pde import examples, reactions

    kw = dict(dx=1.0 / (N - 1), tmax=tmax, diffusion_rate=0.05, kernel=pnmol.kernels.SquareExponential())
    if name == "heat":
        return examples.heat_1d_discretized(y0_fun=examples.sin_bell_1d, **kw), pnmol.white.LinearWhiteNoiseEK1
    return examples.reaction_diffusion_1d_discretized(reactions.logistic(1.0), **kw), pnmol.white.SemiLinearWhiteNoiseEK1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", nargs="+", choices=["heat", "logistic"], default=["heat", "logistic"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512], help="mesh points N")
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tree", type=pathlib.Path, default=ROOT, help="root of the (built) checkout whose package is measured")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    sys.path.insert(0, str(args.tree.resolve() / "pnmol-experiments_amd"))
    import pnmol
    from pnmol.base import rv

    dt, K = 2.0 ** -7, args.steps
    for name in args.problem:
        for N in args.sizes:
            pde, cls = problem(name, N, K * dt, pnmol)
            solver = cls(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                         spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
            first = solver.initialize(pde)                      # binds the device filter; every run starts from a copy of this
            pool = []
            solver.initialize = lambda _pde: pool.pop()
            row = {"problem": name, "N": N, "nu": args.nu, "dt": dt, "steps": K, "reps": args.reps,
                   "tree": "this" if args.tree.resolve() == ROOT else str(args.tree)}
            spread = {}

            def timed(tag, run, keep=False):
                runs = args.reps + 1                            # (one warm-up run)
                pool[:] = [first._replace(y=rv.DeviceMultivariateNormal(first.y.mean, first.y.device_state.clone()))
                           for _ in range(runs)]
                ts, out = [], None
                for i in range(runs):
                    t0 = time.perf_counter()
                    out = run()                                 # (each of them ends in a stream synchronisation)
                    ts.append((time.perf_counter() - t0) / K)
                    if not keep:
                        out = None
                ts = ts[1:]
                spread[tag] = round(1e3 * float(np.ptp(ts)), 4)
                return round(1e3 * float(np.median(ts)), 4), out

            row["a_solve_ms"], sol = timed("a", lambda: solver.solve(pde), keep=True)
            assert len(sol.t) == K + 1
            # (b), (c): also the device-event time of the last run's loop -- one `pnmol_filter_steps` call, all steps being equal
            if hasattr(solver, "solve_on_device"):
                row["b_solve_on_device_ms"], _ = timed("b", lambda: solver.solve_on_device(pde))
                row["b_loop_event_ms"] = round(solver._device_filter.last_steps_ms() / K, 4)
            row["c_solve_marginals_ms"], _ = timed("c", lambda: solver.solve_marginals(pde))
            row["c_loop_event_ms"] = round(solver._device_filter.last_steps_ms() / K, 4)
            row["s_smooth_ms"], _ = timed("s", lambda: solver.smooth(sol, dense=None))
            if hasattr(solver, "smooth_marginals"):
                row["m_smooth_marginals_ms"], _ = timed("m", lambda: solver.smooth_marginals(sol))
                row["m_over_s"] = round(row["m_smooth_marginals_ms"] / row["s_smooth_ms"], 4)
                row["saved_per_backward_step_ms"] = round(row["s_smooth_ms"] - row["m_smooth_marginals_ms"], 4)
            if "b_solve_on_device_ms" in row:
                row["b_over_a"] = round(row["b_solve_on_device_ms"] / row["a_solve_ms"], 4)
                row["b_over_c"] = round(row["b_solve_on_device_ms"] / row["c_solve_marginals_ms"], 4)
            row["spread_ms"] = spread
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
