"""Semilinear steps with the nonlinear term linearised on the device (csrc/pnmol_reaction.hip; DESIGN.md sections 16-18): ms per
step of
  (a) `attempt_step` through the host route (`reaction_on_device = False`: predicted mean back, f / df in NumPy, then the diagonal
      up (reaction) or the dense (d, d) operator scanned on the host and uploaded (system, convection)),
  (b) `attempt_step` linearised on the device (`pnmol_filter_linearize`),
  (c) the constant-step loop with the term set (`pnmol_filter_steps`, what `solve_marginals` runs),
  (d) the linear loop of the same size (the fused steady-state loop): the floor (c) cannot beat -- the same filter after clearing
      the term (system, convection), the heat problem of the same size (reaction).
(a) and (b) are what `solve()` does per step and (c), (d) what `solve_marginals` does per run, timed as bench.py's semilinear row
times them -- at `attempt_step` and `Filter.steps` --, so the per-step state wrapping of `solve()` and the time-grid building of
`solve_marginals` on the host are outside the figures.  Every figure is the median over --reps runs of --steps steps, host wall
clock around work that ends in a stream synchronisation, after a warm-up run of the same shape (graph capture, first launches);
(c) and (d) also report the device-event time of the loop, and `spread_ms` holds max - min of the repeats of (a) .. (d).  nu = 2,
dt = 2^-7.  One JSON line per size, with the keys each kind has printed since its first profile (profiles/reaction,
profiles/reaction_system, profiles/convection).

  --kind reaction    u_t = 0.05 u_xx + u (1 - u), the recipe of bench.py's semilinear row, as `reactions.logistic`
  --kind system      --term lotka_volterra (2 species; N = 256: d = 512, m = 516, width 4) or sir (3; N = 170: d = 510, width 5)
  --kind convection  --term burgers or burgers_fisher, viscosity 0.02, y0 = 0.1 sin(pi x), Dirichlet

    python tools/bench_term_loop.py --kind convection --sizes 256 512 --steps 40 --reps 7
"""

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pnmol-experiments_amd"))

TERMS = {"reaction": ["logistic"], "system": ["lotka_volterra", "sir"], "convection": ["burgers", "burgers_fisher"]}


def problem(kind, args, N, pnmol):
    """(pde, solver kernel, head of the row, key of (a), the linear problem of (d) or None: the same filter, cleared,
    keys printed in full)."""
    from pnmol.pde import examples, reactions

    one = lambda: pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise()
    if kind == "reaction":
        kw = dict(dx=1.0 / (N - 1), tmax=1e3, diffusion_rate=0.05, kernel=pnmol.kernels.SquareExponential())
        pde = examples.reaction_diffusion_1d_discretized(reactions.logistic(1.0), **kw)
        lin = examples.heat_1d_discretized(y0_fun=examples.sin_bell_1d, **kw)
        return pde, one, {"N": N}, "a_host_callables_ms", lin, ()
    if kind == "system":
        C, y0 = {"lotka_volterra": (2, examples.lotka_volterra_y0), "sir": (3, examples.sir_y0)}[args.term]
        pde = examples.reaction_diffusion_system_1d_discretized(getattr(reactions, args.term)(), diffusion_rates=(0.1,) * C,
                                                                y0_fun=y0, dx=1.0 / (N - 1), tmax=1e3)
        head = {"problem": args.term, "N": N, "d": int(pde.L.shape[0]), "m": int(pde.L.shape[0] + pde.B.shape[0])}
        return pde, lambda: pnmol.kernels.duplicate(one(), num=C), head, "a_host_callables_ms", None, ("a_b_final_means_rel_diff", "dt")
    term = getattr(reactions, args.term)()
    pde = examples.convection_diffusion_1d_discretized(term, diffusion_rate=0.02, dx=1.0 / (N - 1), tmax=1e3,
                                                       gradient_stencil_size=args.gradient_stencil_size)
    width = int(((term.G != 0.0) | (pde.L != 0.0)).sum(axis=1).max())
    head = {"term": args.term, "N": N, "m": int(pde.L.shape[0] + pde.B.shape[0]), "width": width}
    return pde, one, head, "a_dense_host_route_ms", None, ("dt",)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=sorted(TERMS), required=True)
    ap.add_argument("--term", help="system: lotka_volterra (default) or sir; convection: burgers (default) or burgers_fisher")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512], help="mesh points N")
    ap.add_argument("--gradient-stencil-size", type=int, default=3)
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    args.term = args.term or TERMS[args.kind][0]
    if args.term not in TERMS[args.kind]:
        ap.error(f"--kind {args.kind} takes --term {' | '.join(TERMS[args.kind])}")
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import pnmol

    dt, K, kind = 2.0 ** -7, args.steps, args.kind
    for N in args.sizes:
        pde, kernel, head, a_key, lin, in_full = problem(kind, args, N, pnmol)
        row = dict(head, nu=args.nu, dt=dt, steps=K, reps=args.reps)
        spread = {}                                             # max - min of the --reps wall-clock figures of (a) .. (d), ms

        def solver_for(on_device, cls=pnmol.white.SemiLinearWhiteNoiseEK1):
            solver = cls(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt), spatial_kernel=kernel())
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
            spread["b" if on_device else "a"] = 1e3 * float(np.ptp(ts))
            return 1e3 * float(np.median(ts)), st.y.mean[0]

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

        row[a_key], m_host = single_steps(False)
        row["b_device_linearised_step_ms"], m_dev = single_steps(True)
        row["a_b_final_means_equal"] = bool(np.array_equal(m_host, m_dev))
        if kind == "system":
            row["a_b_final_means_rel_diff"] = float(np.abs(m_host - m_dev).max() / np.abs(m_host).max())
        semi = solver_for(True)
        dev = semi.initialize(pde).y.device_state
        mean0, cov0 = dev.mean(), dev.cov()
        flt = semi._device_filter
        c_key = f"c_{kind}_loop"
        row[c_key + "_ms"], row[c_key + "_event_ms"] = loop(flt, dev, "c")
        if lin is None:
            flt.set_reaction(None)                              # the same filter, now linear: L alone
            dev = flt.new_state()
            dev.set(pde.t0, mean0, cov0)
        else:
            linear = solver_for(True, pnmol.white.LinearWhiteNoiseEK1)
            dev, flt = linear.initialize(lin).y.device_state, linear._device_filter
        row["d_linear_loop_ms"], row["d_linear_loop_event_ms"] = loop(flt, dev, "d")
        row["c_over_a"] = row[c_key + "_ms"] / row[a_key]
        if kind != "reaction":
            row["b_over_a"] = row["b_device_linearised_step_ms"] / row[a_key]
        row["c_over_d"] = row[c_key + "_ms"] / row["d_linear_loop_ms"]
        row["spread_ms"] = {k: round(v, 4) for k, v in spread.items()}
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) and k not in in_full else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
