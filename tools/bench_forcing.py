"""Driven problems u_t = L u + s(t, x) (csrc/pnmol_forcing.hip): ms per step of
  (1) the forced linear loop: `pnmol_filter_steps` with a table of right-hand sides set (`pnmol_filter_set_forcing`; what
      `solve_marginals` runs on a problem with `pde.forcing`),
  (2) the unforced linear loop on the same filter, the table cleared (the fused steady-state loop): (1) - (2) is the cost of leaving
      the fused route plus the k_force launch,
  (3) the host-callable route for the same source-only problem: `SemiLinearWhiteNoiseEK1.attempt_step` with f(t, u) = s(t),
      df = 0 and no `pde.forcing` -- the predicted mean comes back and the dense (d, d) operator goes up in every step.  This route
      uses nothing of the forcing feature, so `--routes 3` runs unchanged on a checkout that lacks it: the baseline.
Heat problem, kappa = 0.05, nu = 2, dt = 2^-7, s = 0.5 sin(pi x) cos(8 t).  Every figure is the median over --reps runs of --steps
steps, host wall clock around work that ends in a stream synchronisation, after a warm-up run of the same shape (graph capture,
first launches); (1) and (2) also report the device-event time of the loop; `spread_ms` holds max - min of the repeats.  One JSON
line per size.

    python tools/bench_forcing.py --sizes 256 512 --steps 100 --reps 5
"""

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pnmol-experiments_amd"))


def source(t, X):
    return 0.5 * np.sin(np.pi * np.asarray(X, dtype=np.float64).reshape(-1)) * np.cos(8.0 * t)


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
    kernel = lambda: pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise()                  # noqa: E731
    for N in args.sizes:
        kw = dict(dx=1.0 / (N - 1), tmax=1e3, diffusion_rate=0.05, kernel=pnmol.kernels.SquareExponential())
        row = {"N": N, "nu": args.nu, "dt": dt, "steps": K, "reps": args.reps}
        if args.label:
            row["label"] = args.label
        spread = {}

        def loop(flt, dev, tag):
            flt.steps(dev, K + 3, dt)                           # warm-up: frame change, graph capture, first launches
            flt.steps(dev, K, dt)
            wall, event = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                _, _, infos = flt.steps(dev, K, dt)            # (synchronises once, at the end)
                wall.append((time.perf_counter() - t0) / K)
                event.append(flt.last_steps_ms() / K)
                assert all(o.info == -1 for o in infos)
            spread[tag] = 1e3 * float(np.ptp(wall))
            return 1e3 * float(np.median(wall)), float(np.median(event))

        if 1 in args.routes or 2 in args.routes:
            pde = examples.heat_1d_discretized(y0_fun=examples.sin_bell_1d, **kw)
            solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                     spatial_kernel=kernel())
            dev = solver.initialize(pde).y.device_state
            start = dev.clone()                                 # (the loops advance their state in place)
            flt = solver._device_filter
            flt.prepare_error_model(dt)
            row["m"] = flt.m
            if 1 in args.routes:
                rows = (K + 3) + K + args.reps * K              # one table for warm-up and repeats: the graphs capture once
                ts = dt * np.arange(1, rows + 1)
                table = np.zeros((rows, flt.m))
                table[:, :flt.d] = np.stack([source(t, pde.mesh_spatial.points) for t in ts])
                flt.set_forcing(table)
                row["forced_linear_loop_ms"], row["forced_linear_loop_event_ms"] = loop(flt, dev, "forced")
                assert flt.forcing_pending() == (rows, rows)
                flt.clear_forcing()
            if 2 in args.routes:                                # the same filter, its table cleared, from the same initial state
                assert flt is solver._device_filter and flt.forcing_pending() == (0, 0)
                row["unforced_linear_loop_ms"], row["unforced_linear_loop_event_ms"] = loop(flt, start, "unforced")
        if 3 in args.routes:
            cls = problems.SemiLinearEvolutionDirichlet
            holder = {}
            hpde = cls(t0=0.0, tmax=1e3, y0_fun=examples.sin_bell_1d, bbox=np.array([0.0, 1.0]), diffop=diffops.laplace(),
                       diffop_scale=0.05, f=lambda t, x: source(t, holder["X"]), df=lambda _t, x: np.zeros((x.size, x.size)),
                       df_diagonal=None)
            hpde.discretize(mesh_spatial=mesh.RectangularMesh.from_bbox_1d(hpde.bbox, step=kw["dx"]), kernel=kw["kernel"],
                            stencil_size_interior=3, stencil_size_boundary=3, nugget_gram_matrix=0.0)
            holder["X"] = hpde.mesh_spatial.points
            hsolver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                          spatial_kernel=kernel())
            hsolver.reaction_on_device = False
            st = hsolver.initialize(hpde)
            for _ in range(3):
                st, _ = hsolver.attempt_step(st, dt, hpde)
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                for _ in range(K):
                    st, _ = hsolver.attempt_step(st, dt, hpde)  # (every step synchronises: its scalars come back)
                ts.append((time.perf_counter() - t0) / K)
            spread["host"] = 1e3 * float(np.ptp(ts))
            row["host_callable_route_ms"] = 1e3 * float(np.median(ts))
        if "forced_linear_loop_ms" in row and "unforced_linear_loop_ms" in row:
            row["forced_over_unforced"] = row["forced_linear_loop_ms"] / row["unforced_linear_loop_ms"]
        if "forced_linear_loop_ms" in row and "host_callable_route_ms" in row:
            row["forced_over_host"] = row["forced_linear_loop_ms"] / row["host_callable_route_ms"]
        row["spread_ms"] = {k: round(v, 4) for k, v in spread.items()}
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) and k != "dt" else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
