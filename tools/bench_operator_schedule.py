"""Time-dependent operators u_t = kappa(t) u_xx (csrc/pnmol_operator.hip): ms per step of
  (1) the loop with the family (A) and a schedule of coefficients set (`pnmol_filter_set_operator_family`,
      `pnmol_filter_set_operator_schedule`; what `solve_marginals` runs on a problem with `pde.time_dependent_operator`),
  (2) the linear loop on the same filter with the family cleared (the fused steady-state loop): (1) - (2) is the cost of leaving
      the fused route plus the k_operator_at launch,
  (3) the host-callable route for the same problem: `SemiLinearWhiteNoiseEK1.attempt_step` with f(t, u) = (M(t) - L0) u,
      df = M(t) - L0 and no `pde.time_dependent_operator` -- the predicted mean comes back and the dense (d, d) operator goes up in
      every step (and the noise stays that of t0).  This route uses nothing of the feature, so `--routes 3` runs unchanged on a
      checkout that lacks it: the baseline.
Heat problem, kappa(t) = 0.05 (1 + 0.8 sin(2 pi t / (steps dt))), nu = 2, dt = 2^-7.  The routes alternate inside every repeat; a
figure is the median over --reps repeats of --steps steps, host wall clock around work that ends in a stream synchronisation, after
a warm-up of the same shape (graph capture, first launches); (1) and (2) also report the device-event time of the loop; `spread_ms`
holds max - min of the repeats.  One JSON line per size.

    python tools/bench_operator_schedule.py --sizes 256 512 --steps 100 --reps 5
"""

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pnmol-experiments_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512], help="mesh points N")
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--routes", type=int, nargs="+", default=[1, 2, 3], choices=[1, 2, 3])
    ap.add_argument("--label", default=None, help="a tag for the line, e.g. the commit the figures were taken on")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import pnmol
    from pnmol import diffops, mesh
    from pnmol.pde import examples, problems

    dt, K = 2.0 ** -7, args.steps
    kappa = lambda t: 0.05 * (1.0 + 0.8 * np.sin(2.0 * np.pi * t / (K * dt)))              # noqa: E731
    kernel = lambda: pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise()                  # noqa: E731
    for N in args.sizes:
        kw = dict(dx=1.0 / (N - 1), tmax=1e3, kernel=pnmol.kernels.SquareExponential())
        row = {"N": N, "nu": args.nu, "dt": dt, "steps": K, "reps": args.reps}
        if args.label:
            row["label"] = args.label
        runs = {}                                               # route -> callable() -> (wall s per step, event ms per step or None)

        def loop_of(flt, dev):
            def run():
                t0 = time.perf_counter()
                _, _, infos = flt.steps(dev, K, dt)            # (synchronises once, at the end)
                wall = (time.perf_counter() - t0) / K
                assert all(o.info == -1 for o in infos)
                return wall, flt.last_steps_ms() / K
            return run

        if 1 in args.routes:
            pde = examples.heat_1d_time_varying_discretized(diffusion_rate=kappa, **kw)
            solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                     spatial_kernel=kernel())
            dev = solver.initialize(pde).y.device_state
            flt = solver._device_filter
            row["m"] = flt.m
            rows = (K + 3) + K + args.reps * K                  # one table for warm-up and repeats: the graphs capture once
            flt.set_operator_schedule(pde.time_dependent_operator.table(dt * np.arange(rows + 1)))
            flt.steps(dev, K + 3, dt)                           # warm-up: frame change, graph capture, first launches
            flt.steps(dev, K, dt)
            runs[1] = loop_of(flt, dev)
        if 2 in args.routes:                                    # a filter of the same problem, its family cleared
            pde2 = examples.heat_1d_time_varying_discretized(diffusion_rate=kappa, **kw)
            solver2 = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                      spatial_kernel=kernel())
            dev2 = solver2.initialize(pde2).y.device_state
            flt2 = solver2._device_filter
            flt2.clear_operator_family()
            flt2.prepare_error_model(dt)
            flt2.steps(dev2, K + 3, dt)
            flt2.steps(dev2, K, dt)
            runs[2] = loop_of(flt2, dev2)
        if 3 in args.routes:
            holder = {}
            hpde = problems.SemiLinearEvolutionDirichlet(
                t0=0.0, tmax=1e3, y0_fun=examples.heat_1d().y0_fun, bbox=np.array([0.0, 1.0]), diffop=diffops.laplace(),
                diffop_scale=0.05, f=lambda t, x: (kappa(t) * holder["L"] - holder["L0"]) @ x,
                df=lambda t, x: kappa(t) * holder["L"] - holder["L0"], df_diagonal=None)
            hpde.discretize(mesh_spatial=mesh.RectangularMesh.from_bbox_1d(hpde.bbox, step=kw["dx"]), kernel=kw["kernel"],
                            stencil_size_interior=3, stencil_size_boundary=3, nugget_gram_matrix=0.0)
            holder["L0"], holder["L"] = hpde.L, hpde.L / 0.05
            hsolver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                          spatial_kernel=kernel())
            hsolver.reaction_on_device = False
            state = {"st": hsolver.initialize(hpde)}
            for _ in range(3):
                state["st"], _ = hsolver.attempt_step(state["st"], dt, hpde)

            def host():
                st = state["st"]
                t0 = time.perf_counter()
                for _ in range(K):
                    st, _ = hsolver.attempt_step(st, dt, hpde)  # (every step synchronises: its scalars come back)
                state["st"] = st
                return (time.perf_counter() - t0) / K, None
            runs[3] = host
        wall = {r: [] for r in runs}
        event = {r: [] for r in runs}
        for _ in range(args.reps):                              # the routes alternate inside a repeat
            for r, run in runs.items():
                w, e = run()
                wall[r].append(w), event[r].append(e)
        names = {1: "operator_loop", 2: "linear_loop", 3: "host_callable_route"}
        for r in runs:
            row[names[r] + "_ms"] = 1e3 * float(np.median(wall[r]))
            if event[r][0] is not None:
                row[names[r] + "_event_ms"] = float(np.median(event[r]))
        if 1 in runs and 2 in runs:
            row["operator_over_linear"] = row["operator_loop_ms"] / row["linear_loop_ms"]
        if 1 in runs and 3 in runs:
            row["operator_over_host"] = row["operator_loop_ms"] / row["host_callable_route_ms"]
        row["spread_ms"] = {names[r]: round(1e3 * float(np.ptp(wall[r])), 4) for r in runs}
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) and k != "dt" else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
