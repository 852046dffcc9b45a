"""Posterior of linear functionals on the GPU: median wall-clock ms of synchronised calls, heat problem,
nu = 2, dt = 2^-7, fp64, on a `solve_on_device` result of --steps steps.  One line per mesh size:

  smoother pass   `smooth_marginals` (one `pnmol_smoother_steps` call: the kernels of `pnmol_smoother_step`) per step
  functionals     `solver.functionals(sol, W)` for Q = 8 and Q = 64 per step.  A call also uploads the weights and carries the
                  terminal term (two thin launches), so the figure is the whole call over the steps, not a kernel time.
  host route      (--host-route-n) what the call replaces: `smooth(sol, dense="full")` on the device, every smoothed and filtered
                  covariance read back, the gains G_k = P_k A^T (P-)^-1 applied on the host through a Cholesky solve per step
                  (thin: Cov(x_k, x_l) W_l^T = G_k ... G_{l-1} Ps_l W_l^T), and the largest relative difference of its
                  covariance against the device's.

    python tools/bench_functionals.py --mesh-n 256 512 1024 --host-route-n 512
"""

import argparse
import pathlib
import statistics
import sys
import time

import numpy as np
import scipy.linalg

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (ROOT / "tests", ROOT / "oracle", ROOT / "pnmol-experiments_amd"):
    sys.path.insert(0, str(p))

DT = 2.0 ** -7


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def host_route(solver, sol, W, iwp):
    """(mean, cov) of the functionals W (Q, T+1, d) by smoothing on the device and assembling on the host."""
    A, Ql = iwp.preconditioned_discretize
    Qm = Ql @ Ql.T
    ssol = solver.smooth(sol, dense="full")
    T, n = len(sol.t) - 1, ssol.mean.shape[1]
    Ps = [y.device_state.cov() for y in ssol._ys]
    Wf = np.zeros((W.shape[0], T + 1, Ps[0].shape[0]))
    Wf[:, :, ::n] = W                                           # flat state index j n + a, derivative 0
    gains = []
    for k in range(T):
        Pc, _ = iwp.nordsieck_preconditioner(sol.t[k + 1] - sol.t[k])
        s = np.diag(Pc).copy()
        Ph = sol._ys[k].device_state.cov() / np.outer(s, s)
        gains.append((s, Ph, scipy.linalg.cho_factor(A @ Ph @ A.T + Qm, lower=True)))

    def gain(k, Z):
        s, Ph, cf = gains[k]
        # G_k Z in raw coordinates.  x_raw = s x_h, so G_raw = S G_h S^-1 with G_h = P^h A^T (P-)^-1.
        return s[:, None] * (Ph @ (A.T @ scipy.linalg.cho_solve(cf, Z / s[:, None])))

    mean = sum(Wf[:, k] @ ssol.mean[k].reshape(-1, order="F") for k in range(T + 1))
    cov = np.zeros((W.shape[0],) * 2)
    for l in range(T + 1):
        Z = Ps[l] @ Wf[:, l].T
        cov += Wf[:, l] @ Z
        for k in range(l - 1, -1, -1):
            Z = gain(k, Z)
            X = Wf[:, k] @ Z
            cov += X + X.T
    return mean, 0.5 * (cov + cov.T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-route-n", type=int, nargs="*", default=[512])
    args = ap.parse_args()
    from helpers import make_pair

    K = args.steps
    for N in args.mesh_n:
        pde, solver, opde, osolver = make_pair(N, args.nu, DT, K, "dirichlet")
        sol = solver.solve_on_device(pde)
        rng = np.random.default_rng(0)
        line = [f"N={N} nu={args.nu} Dp={(args.nu + 1) * ((N + 31) // 32) * 32} steps={K}"]
        med, lo, hi = timed(lambda: solver.smooth_marginals(sol), args.reps)
        line.append(f"smoother pass {1e3 * med / K:.3f} ms/step (min {1e3 * lo / K:.3f}, max {1e3 * hi / K:.3f})")
        for Q in (8, 64):
            W = rng.standard_normal((Q, K + 1, N))
            med, lo, hi = timed(lambda: solver.functionals(sol, W), args.reps)
            line.append(f"functionals Q={Q} {1e3 * med / K:.3f} ms/step (min {1e3 * lo / K:.3f}, max {1e3 * hi / K:.3f})")
        print(" | ".join(line), flush=True)
        if N in args.host_route_n:
            iwp = osolver.initialize_iwp(opde)[0]
            W = rng.standard_normal((8, K + 1, N))
            post = solver.functionals(sol, W)
            med, lo, hi = timed(lambda: host_route(solver, sol, W, iwp), 3, warmup=1)
            _, cov = host_route(solver, sol, W, iwp)
            diff = float(np.abs(cov - post.cov).max() / np.abs(post.cov).max())
            print(f"N={N} host route Q=8: {1e3 * med:.0f} ms per call = {1e3 * med / K:.1f} ms/step (min {1e3 * lo:.0f}, max "
                  f"{1e3 * hi:.0f} ms per call); largest |cov - device cov| / max|cov| = {diff:.1e}", flush=True)


if __name__ == "__main__":
    main()
