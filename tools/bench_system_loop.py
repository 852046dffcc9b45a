"""Semilinear steps of coupled systems with the reaction on the device (csrc/pnmol_reaction.hip, k_linearize_system; DESIGN.md
section 17): ms per step of
  (a) `attempt_step` with the host callables (`reaction_on_device = False`: predicted mean back, f / df in NumPy, the dense
      (d, d) operator scanned on the host and uploaded) -- the only route before `pnmol_filter_set_reaction_system`,
  (b) `attempt_step` linearised on the device (`pnmol_filter_linearize`),
  (c) the constant-step loop with the system set (`pnmol_filter_steps`, what `solve_marginals` runs),
  (d) the linear loop on the same filter after clearing the system (the fused steady-state loop on L alone): the floor of (c).
Problems: Lotka-Volterra at N = 256 (d = 512, m = 516, stencil width 4) and SIR at N = 170 (d = 510, m = 516, width 5), nu = 2,
dt = 2^-7, the fused-sweep size of bench.py's headline.  Timed as tools/bench_reaction_loop.py times the scalar reaction -- at
`attempt_step` and `Filter.steps` --: every figure is the median over --reps runs of --steps steps, host wall clock around work
that ends in a stream synchronisation, after a warm-up run of the same shape (graph capture, first launches); (c) and (d) also
report the device-event time of the loop.  One JSON line per problem.

    python tools/bench_system_loop.py --steps 40 --reps 7
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
    ap.add_argument("--problems", nargs="+", default=["lotka_volterra:256", "sir:170"], help="name:N")
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import pnmol
    from pnmol.pde import examples, reactions

    systems = {"lotka_volterra": (2, reactions.lotka_volterra, examples.lotka_volterra_y0),
               "sir": (3, reactions.sir, examples.sir_y0)}
    dt, K = 2.0 ** -7, args.steps
    for spec in args.problems:
        name, N = spec.split(":")[0], int(spec.split(":")[1])
        C, make, y0 = systems[name]
        pde = examples.reaction_diffusion_system_1d_discretized(make(), diffusion_rates=(0.1,) * C, y0_fun=y0, dx=1.0 / (N - 1),
                                                                tmax=1e3)
        row = {"problem": name, "N": N, "d": int(pde.L.shape[0]), "m": int(pde.L.shape[0] + pde.B.shape[0]), "nu": args.nu,
               "dt": dt, "steps": K, "reps": args.reps}

        def solver_for(on_device):
            kernel = pnmol.kernels.duplicate(pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise(), num=C)
            solver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                         spatial_kernel=kernel)
            solver.reaction_on_device = on_device
            return solver

        def single_steps(on_device):
            solver = solver_for(on_device)
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

        def loop(flt, dev):
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
        row["a_b_final_means_rel_diff"] = float(np.abs(m_host - m_dev).max() / np.abs(m_host).max())
        semi = solver_for(True)
        dev = semi.initialize(pde).y.device_state
        mean0, cov0 = dev.mean(), dev.cov()
        flt = semi._device_filter
        row["c_system_loop_ms"], row["c_system_loop_event_ms"] = loop(flt, dev)
        flt.set_reaction(None)                                  # the same filter, now linear: L alone
        dev = flt.new_state()
        dev.set(pde.t0, mean0, cov0)
        row["d_linear_loop_ms"], row["d_linear_loop_event_ms"] = loop(flt, dev)
        row["c_over_a"] = row["c_system_loop_ms"] / row["a_host_callables_ms"]
        row["b_over_a"] = row["b_device_linearised_step_ms"] / row["a_host_callables_ms"]
        row["c_over_d"] = row["c_system_loop_ms"] / row["d_linear_loop_ms"]
        keep = ("a_b_final_means_rel_diff", "dt")                # (not times: printed in full)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) and k not in keep else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
