"""Sensor data inside the device-resident constant-step loop (`pnmol_filter_set_observations`, csrc/pnmol_observe.hip; DESIGN.md
section 19): ms per step of
  (a) the `solve(pde, observations=...)` route: `attempt_step` per step and `_observe` (`pnmol_state_observe`) behind every
      --every-th step, each ending in its own synchronisation,
  (b) the loop with the plan (`Filter.steps` with `set_observations`: what `solve_marginals(pde, observations=...)` runs),
  (c) the linear loop without data on the same filter (the fused steady-state loop),
and ms per call of
  (d) `pnmol_state_observe` alone on the state the loop left (preallocated output state),
  (p) `pnmol_state_observe_planned` on that state: the sweep route (the default) and, for q <= 32, the single-workgroup route
      (PNMOL_HIP_OBSERVE_SINGLE_WG=1 set around `set_observations`).
The cost of one in-loop update is ((b) - (c)) * every.  Every figure is the median over --reps runs (of --steps steps for (a) .. (c)),
host wall clock around work that ends in a stream synchronisation, after a warm-up run of the same shape (graph capture, first
launches, workspaces); (b) and (c) also report the device-event time of the loop, and `spread_ms` holds max - min of the repeats.
Setting the plan (a cold call that copies the tables) is outside the timed region, as the solver sets it once per solve.
Heat problem, nu = 2, dt = 2^-7, fp64; q sensors that average two neighbouring nodes, data = the sensors' current mean plus noise of
std 1e-6.  One JSON line per (N, q, every).  --parts a d runs on a library without the plan (the parent of this feature).

    python tools/bench_observe_loop.py --mesh-n 256 512 --q 8 64 --every 1 4 --steps 40 --reps 7
"""

import argparse
import ctypes
import json
import os
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pnmol-experiments_amd"))

NOISE = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--q", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--every", type=int, nargs="+", default=[1, 4], help="data behind every k-th step")
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parts", nargs="+", default=["a", "b", "c", "d", "p"], choices=["a", "b", "c", "d", "p"])
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import pnmol
    from pnmol import _hip, data

    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    dt, K = 2.0 ** -7, args.steps
    for N in args.mesh_n:
        pde = pnmol.pde.examples.heat_1d_discretized(dx=1.0 / (N - 1), tmax=1e3, diffusion_rate=0.05,
                                                     kernel=pnmol.kernels.SquareExponential(), bcond="dirichlet")

        def bound():
            solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                     spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
            return solver, solver.initialize(pde)

        for q in args.q:
            if q > N:
                continue
            left = np.round(np.linspace(1, N - 3, q)).astype(int)
            C = np.zeros((q, N))
            C[np.arange(q), left] = C[np.arange(q), left + 1] = 0.5
            R = NOISE * np.eye(q)
            rng = np.random.default_rng(q)
            reading = lambda mean0: C @ mean0 + NOISE * rng.standard_normal(q)
            for every in args.every:
                row = {"N": N, "nu": args.nu, "q": q, "every": every, "dt": dt, "steps": K, "reps": args.reps}
                spread = {}

                if "a" in args.parts:
                    solver, st = bound()

                    def host_route(st):
                        for j in range(K):
                            st, _ = solver.attempt_step(st, dt, pde)                    # (synchronises: its scalars come back)
                            if (j + 1) % every == 0:
                                st, _ = solver._observe(st, data.Observation(st.t, C, reading(st.y.mean[0]), NOISE))
                        return st

                    st = host_route(st)
                    ts = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        st = host_route(st)
                        ts.append((time.perf_counter() - t0) / K)
                    row["a_solve_route_ms"] = 1e3 * float(np.median(ts))
                    spread["a"] = 1e3 * float(np.ptp(ts))

                solver, st = bound()
                flt, dev = solver._device_filter, st.y.device_state
                flt.prepare_error_model(dt)

                def loop(tag, planned):
                    wall, event = [], []
                    for rep in range(args.reps + 2):                                    # two warm-up runs
                        if planned:
                            t, times = dev.t, []
                            for j in range(K):
                                t += dt                                                 # (the loop's own accumulation)
                                if (j + 1) % every == 0:
                                    times.append(t)
                            base = reading(dev.mean()[0])
                            flt.set_observations(times, C, np.tile(base, (len(times), 1)), R)
                        t0 = time.perf_counter()
                        _, _, infos = flt.steps(dev, K, dt)                             # (synchronises once, at the end)
                        w = (time.perf_counter() - t0) / K
                        assert all(o.info == -1 for o in infos)
                        if planned:
                            assert flt.observations_pending() == (len(times), len(times))
                        if rep >= 2:
                            wall.append(w), event.append(flt.last_steps_ms() / K)
                    spread[tag] = 1e3 * float(np.ptp(wall))
                    return 1e3 * float(np.median(wall)), float(np.median(event))

                if "b" in args.parts:
                    row["b_plan_loop_ms"], row["b_plan_loop_event_ms"] = loop("b", True)
                    flt.clear_observations()
                if "c" in args.parts:
                    flt.steps(dev, K + 3, dt)                                           # (back in the fused loop: its graphs)
                    row["c_linear_loop_ms"], row["c_linear_loop_event_ms"] = loop("c", False)
                if "b" in args.parts and "c" in args.parts:
                    row["update_in_loop_ms"] = (row["b_plan_loop_ms"] - row["c_linear_loop_ms"]) * every
                    row["update_in_loop_event_ms"] = (row["b_plan_loop_event_ms"] - row["c_linear_loop_event_ms"]) * every
                if "b" not in args.parts and "c" not in args.parts:
                    flt.steps(dev, 4, dt)                                               # (a state in the frame of dt)
                if "d" in args.parts:
                    y = reading(dev.mean()[0])
                    out, res = flt.new_state(), _hip.ObserveOut()
                    call = lambda: flt.lib.pnmol_state_observe(flt.handle, dev.handle, q, dp(C), dp(y), dp(R), out.handle,
                                                               ctypes.byref(res))
                    assert call() == 0                                                  # workspace + first launch
                    ts = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        rc = call()
                        ts.append(time.perf_counter() - t0)
                        assert rc == 0
                    row["d_observe_alone_ms"] = 1e3 * float(np.median(ts))
                    spread["d"] = 1e3 * float(np.ptp(ts))
                if "p" in args.parts:
                    for key, single in (("p_planned_ms", False), ("p_planned_single_wg_ms", True)):
                        if single and q > 32:
                            continue
                        if single:
                            os.environ["PNMOL_HIP_OBSERVE_SINGLE_WG"] = "1"             # (read by set_observations)
                        twin = dev.clone()
                        base = reading(twin.mean()[0])
                        flt.set_observations(twin.t + dt * np.arange(1, args.reps + 2), C, np.tile(base, (args.reps + 1, 1)), R)
                        os.environ.pop("PNMOL_HIP_OBSERVE_SINGLE_WG", None)
                        flt.observe_planned(twin, 0)                                    # first launch
                        ts = []
                        for i in range(1, args.reps + 1):
                            t0 = time.perf_counter()
                            res = flt.observe_planned(twin, i)                          # (in place; synchronises once)
                            ts.append(time.perf_counter() - t0)
                            assert res.info == -1
                        flt.clear_observations()
                        row[key] = 1e3 * float(np.median(ts))
                        spread[key[:-3]] = 1e3 * float(np.ptp(ts))
                if "a" in args.parts and "b" in args.parts:
                    row["b_over_a"] = row["b_plan_loop_ms"] / row["a_solve_route_ms"]
                row["spread_ms"] = {k: round(v, 4) for k, v in spread.items()}
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) and k != "dt" else v) for k, v in row.items()}),
                      flush=True)


if __name__ == "__main__":
    main()
