"""The iterated EK1 smoother (csrc/pnmol_reaction.hip, `pnmol_filter_set_linearization_points`, `solve_iterated`; DESIGN.md section
22): per problem and size,

  (a) `solve_on_device(pde)`: ms per forward step of the plain loop -- every step linearised at its own predicted mean.  This is the
      yardstick: with --tree it is measured on another (built) checkout, e.g. an export of the parent commit,
  (b) `solve_on_device(pde, linearize_at=points)`: ms per forward step with a table of linearisation points,
  (c) one whole iteration, ms: (b) + `smooth_marginals` (the backward pass in one call),
  (d) the host route for one iteration, ms: `linearize_at(points[k])` + `pnmol_filter_step` per step, then `smooth(dense=None)`,
  (e) `solve_iterated(pde, iterations=2, tol=0, smooth=None)` as a user calls it, ms per pass (three passes): what (c) leaves out --
      `initialize` (O(d^3) on the host), the new device filter and the graph capture of every pass -- is in it.

Fisher-KPP (u_t = 0.05 u_xx + u (1 - u)) and viscous Burgers (u_t = 0.02 u_xx - u u_x), nu = 2, dt = 2^-7.  The points are the
smoothed means of a plain pass.  Every figure is the median over --reps runs, host wall clock around work that ends in a stream
synchronisation, after a warm-up run of the same shape; `spread_ms` holds max - min of the repeats; (a) and (b) also report the
device-event time of their loop.  For (a) - (d) the initial state is computed once outside the timed region and every run starts
from a copy of it on the one bound filter.  One JSON line per problem and size; a tree without the feature prints (a) alone.

    python tools/bench_iterated.py --problem fisher burgers --sizes 256 512 --steps 100 --reps 5
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

    if name == "fisher":
        return examples.reaction_diffusion_1d_discretized(reactions.logistic(1.0), dx=1.0 / (N - 1), tmax=tmax, diffusion_rate=0.05,
                                                          kernel=pnmol.kernels.SquareExponential())
    return examples.convection_diffusion_1d_discretized(reactions.burgers(), diffusion_rate=0.02, dx=1.0 / (N - 1), tmax=tmax)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", nargs="+", choices=["fisher", "burgers"], default=["fisher", "burgers"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512], help="mesh points N")
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", type=pathlib.Path, default=ROOT, help="root of the (built) checkout whose package is measured")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    sys.path.insert(0, str(args.tree.resolve() / "pnmol-experiments_amd"))
    import pnmol
    from pnmol import pdefilter
    from pnmol.base import rv

    dt, K = 2.0 ** -7, args.steps
    for name in args.problem:
        for N in args.sizes:
            pde = problem(name, N, K * dt, pnmol)
            solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                         spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
            first = solver.initialize(pde)                      # binds the device filter; every run starts from a copy of this
            flt = solver._device_filter
            pool = []
            solver.initialize = lambda _pde: pool.pop()
            row = {"problem": name, "N": N, "nu": args.nu, "dt": dt, "steps": K, "reps": args.reps,
                   "tree": "this" if args.tree.resolve() == ROOT else str(args.tree)}
            spread = {}

            def timed(tag, run, per):
                runs = args.reps + 1                            # (one warm-up run)
                pool[:] = [first._replace(y=rv.DeviceMultivariateNormal(first.y.mean, first.y.device_state.clone()))
                           for _ in range(runs)]
                ts = []
                for _ in range(runs):
                    t0 = time.perf_counter()
                    run()                                       # (each of them ends in a stream synchronisation)
                    ts.append((time.perf_counter() - t0) / per)
                ts = ts[1:]
                spread[tag] = round(1e3 * float(np.ptp(ts)), 4)
                return round(1e3 * float(np.median(ts)), 4)

            row["a_plain_forward_step_ms"] = timed("a", lambda: solver.solve_on_device(pde), K)
            row["a_loop_event_ms"] = round(flt.last_steps_ms() / K, 4)
            if hasattr(solver, "solve_iterated"):
                pool[:] = [first._replace(y=rv.DeviceMultivariateNormal(first.y.mean, first.y.device_state.clone()))]
                sol = solver.solve_on_device(pde)
                ts = np.asarray(sol.t)
                points = solver.smooth_marginals(sol)[0][1:]
                del sol
                row["b_table_forward_step_ms"] = timed("b", lambda: solver.solve_on_device(pde, linearize_at=points), K)
                row["b_loop_event_ms"] = round(flt.last_steps_ms() / K, 4)
                row["c_iteration_ms"] = timed("c", lambda: solver.smooth_marginals(solver.solve_on_device(pde, linearize_at=points)), 1)

                def host_route():
                    state = pool.pop()
                    dev, ys = state.y.device_state, [state.y]
                    for k in range(K):
                        flt.linearize_at(points[k])
                        dev, _, _ = flt.step(dev, dt, want_error=False)
                        ys.append(rv.DeviceMultivariateNormal(dev.mean(), dev))
                    sol = pdefilter.PDESolution(t=ts, mean=np.stack([y.mean for y in ys]), ys=ys, info={},
                                                diffusion_squared_calibrated=1.0)
                    return solver.smooth(sol, dense=None)

                row["d_host_route_iteration_ms"] = timed("d", host_route, 1)
                del solver.initialize                           # (e): the solver as it is, `initialize` in every pass
                row["e_solve_iterated_pass_ms"] = timed("e", lambda: solver.solve_iterated(pde, iterations=2, tol=0.0, smooth=None), 3)
                row["b_over_a"] = round(row["b_table_forward_step_ms"] / row["a_plain_forward_step_ms"], 4)
                row["c_over_d"] = round(row["c_iteration_ms"] / row["d_host_route_iteration_ms"], 4)
            row["spread_ms"] = spread
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
