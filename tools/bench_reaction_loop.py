"""Semilinear steps with the reaction term on the device (csrc/pnmol_reaction.hip): ms per step of
  (a) `attempt_step` with the host callables (`reaction_on_device = False`: predicted mean back, f / df in NumPy, 2d numbers up),
  (b) `attempt_step` linearised on the device (`pnmol_filter_linearize`),
  (c) the constant-step loop with a reaction set (`pnmol_filter_steps`, what `solve_marginals` runs),
  (d) the same loop on the linear problem of the same size (the fused steady-state loop): the floor (c) cannot beat.
(a) and (b) are what `solve()` does per step and (c), (d) what `solve_marginals` does per run, timed as bench.py's semilinear
row times them -- at `attempt_step` and `Filter.steps` --, so the per-step state wrapping of `solve()` and the time-grid
building of `solve_marginals` on the host are outside the figures.
Problem: the spruce-budworm recipe of bench.py's semilinear row (u_t = 0.05 u_xx + u (1 - u), nu = 2, dt = 2^-7) as a
`pnmol.pde.reactions.logistic` reaction.  Every figure is the median over --reps runs of --steps steps, host wall clock around
work that ends in a stream synchronisation, after a warm-up run of the same shape (graph capture, first launches); (c) and (d)
also report the device-event time of the loop.  One JSON line per N.

    python tools/bench_reaction_loop.py --mesh-n 256 512 --steps 40 --reps 7
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
    ap.add_argument("--mesh-n", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import pnmol
    from pnmol.pde import reactions

    dt, K = 2.0 ** -7, args.steps
    kernel = lambda: pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise()
    for N in args.mesh_n:
        kw = dict(dx=1.0 / (N - 1), tmax=1e3, diffusion_rate=0.05, kernel=pnmol.kernels.SquareExponential())
        pde = pnmol.pde.examples.reaction_diffusion_1d_discretized(reactions.logistic(1.0), **kw)
        lin = pnmol.pde.examples.heat_1d_discretized(y0_fun=pnmol.pde.examples.sin_bell_1d, **kw)
        row = {"N": N, "nu": args.nu, "dt": dt, "steps": K, "reps": args.reps}

        def single_steps(on_device):
            solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                         spatial_kernel=kernel())
            solver.reaction_on_device = on_device
            st = solver.initialize(pde)
            assert (solver._device_filter.reaction is not None) == on_device
            for _ in range(3):
                st, _ = solver.attempt_step(st, dt, pde)
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                for _ in range(K):
                    st, _ = solver.attempt_step(st, dt, pde)   # (every step synchronises: its scalars come back)
                ts.append((time.perf_counter() - t0) / K)
            return 1e3 * float(np.median(ts)), st.y.mean[0]

        def loop(solver, problem):
            dev = solver.initialize(problem).y.device_state
            flt = solver._device_filter
            flt.steps(dev, K + 3, dt)                           # warm-up: frame change, graph capture, first launches
            flt.steps(dev, K, dt)
            wall, event = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                _, _, infos = flt.steps(dev, K, dt)            # (synchronises once, at the end)
                wall.append((time.perf_counter() - t0) / K)
                event.append(flt.last_steps_ms() / K)
                assert all(o.info == -1 for o in infos)
            return 1e3 * float(np.median(wall)), float(np.median(event))

        row["a_host_callables_ms"], m_host = single_steps(False)
        row["b_device_linearised_step_ms"], m_dev = single_steps(True)
        row["a_b_final_means_equal"] = bool(np.array_equal(m_host, m_dev))
        semi = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                   spatial_kernel=kernel())
        row["c_reaction_loop_ms"], row["c_reaction_loop_event_ms"] = loop(semi, pde)
        linear = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                 spatial_kernel=kernel())
        row["d_linear_loop_ms"], row["d_linear_loop_event_ms"] = loop(linear, lin)
        row["c_over_a"] = row["c_reaction_loop_ms"] / row["a_host_callables_ms"]
        row["c_over_d"] = row["c_reaction_loop_ms"] / row["d_linear_loop_ms"]
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
