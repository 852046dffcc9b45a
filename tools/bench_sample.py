"""One backward step of the joint posterior draw (`pnmol_samples_step_back`, device-generated noise) on the GPU: median
wall-clock ms per step for S draws, against (a) `pnmol_smoother_step` on the same states in the same process and (b) the same
sampling step written with torch-ROCm library calls (torch.linalg.cholesky / solve_triangular / matmul / randn, the style
of tools/bench_smooth.py), with the largest relative difference of the two results at equal host-supplied noise.  The
difference is taken with xi_1 = 0: the filtered covariance is singular, its factor is not unique, and two factors map the
same xi_1 to different (equally distributed) draws; the process-noise factor chol(Q1) (x) chol(K) is unique.  (The torch
path factorises P_k + 1e-13 diag(P_k) to get through its strict Cholesky.)  Heat problem, nu = 2, dt = 2^-7, fp64.
One JSON line per (N, S).

    python tools/bench_sample.py --mesh-n 256 512 1024 --samples 1 64 1024 --reps 7
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
    ap.add_argument("--mesh-n", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3, help="filter steps before the timed backward steps")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-torch", action="store_true", help="skip the library path (profiling runs)")
    args = ap.parse_args()
    import scipy.linalg
    if not args.no_torch:
        import torch                                    # (before the library: one HIP runtime per process)
    import pnmol

    for N in args.mesh_n:
        dt = 2.0 ** -7
        pde = pnmol.pde.examples.heat_1d_discretized(dx=1.0 / (N - 1), tmax=args.steps * dt, diffusion_rate=0.05,
                                                     kernel=pnmol.kernels.SquareExponential(), bcond="dirichlet")
        solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
        sol = solver.solve(pde)
        flt = sol._ys[-1].device_state.filter
        a, b = sol._ys[-2].device_state, sol._ys[-1].device_state
        n, d = flt.n, flt.d
        D = n * d
        flt.smoother_step(a, b, dt)                     # workspace + first launch
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            flt.smoother_step(a, b, dt)                 # (synchronises once: the pivot check)
            ts.append(time.perf_counter() - t0)
        smooth_ms = 1e3 * float(np.median(ts))

        if not args.no_torch:
            dev = torch.device("cuda")
            s, _ = solver.iwp.nordsieck_preconditioner_1d_raw(dt)
            perm = np.array([j * n + q for q in range(n) for j in range(d)])   # derivative-major <- point-major
            sc = np.repeat(s, d)
            m_k, P_k = a.mean().reshape(-1) / sc, a.cov()[np.ix_(perm, perm)] / np.outer(sc, sc)
            m_n = b.mean().reshape(-1) / sc
            A1 = np.flip(scipy.linalg.pascal(n, kind="lower")).astype(np.float64)
            Q1 = np.flip(scipy.linalg.hilbert(n))
            t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
            A, Q = t(np.kron(A1, np.eye(d))), t(np.kron(Q1, solver._gram))
            Pk, mk = t(P_k), t(m_k)
            LQ = torch.linalg.cholesky(Q)

            def lib_step(x_next, xi1, xi2):             # columns = draws
                C = torch.linalg.cholesky_ex(Pk + 1e-13 * torch.diag(torch.diagonal(Pk)))[0]
                AP = A @ Pk
                L = torch.linalg.cholesky(AP @ A.T + Q)
                xt = mk[:, None] + C @ xi1
                r = x_next - A @ xt - LQ @ xi2
                y = torch.linalg.solve_triangular(L, r, upper=False)
                V = torch.linalg.solve_triangular(L, AP, upper=False).T       # P A^T L^-T
                return xt + V @ y

        for S in args.samples:
            blk = flt.new_samples(S)
            blk.draw(b, seed=1, step_index=1)
            blk.step_back(a, dt, seed=1, step_index=0)  # workspace + first launch
            ts = []
            for _ in range(args.reps):
                blk.draw(b, seed=1, step_index=1)
                t0 = time.perf_counter()
                blk.step_back(a, dt, seed=1, step_index=0)   # (synchronises once: the pivot checks)
                ts.append(time.perf_counter() - t0)
            ms = 1e3 * float(np.median(ts))
            rec = {"N": N, "nu": args.nu, "D": D, "S": S, "sample_ms_per_step": round(ms, 3),
                   "smoother_ms_per_step": round(smooth_ms, 3), "sample_over_smoother": round(ms / smooth_ms, 3)}
            if not args.no_torch:
                xn = t(np.tile(m_n[:, None], (1, S)))
                lib_step(xn, torch.randn(D, S, dtype=torch.float64, device=dev), torch.randn(D, S, dtype=torch.float64, device=dev))
                torch.cuda.synchronize()
                tl = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    lib_step(xn, torch.randn(D, S, dtype=torch.float64, device=dev),
                             torch.randn(D, S, dtype=torch.float64, device=dev))
                    torch.cuda.synchronize()
                    tl.append(time.perf_counter() - t0)
                # equal noise: terminal draw with zero noise (= the mean), xi_1 = 0, xi_2 random
                xi2 = np.random.default_rng(0).standard_normal((S, D))
                blk.draw(b, np.zeros((S, D)))
                blk.step_back(a, dt, np.hstack((np.zeros((S, D)), xi2)))
                hip = (blk.get().reshape(S, D) / sc).T
                lib = lib_step(xn, torch.zeros(D, S, dtype=torch.float64, device=dev), t(xi2.T)).cpu().numpy()
                rec["torch_ms_per_step"] = round(1e3 * float(np.median(tl)), 3)
                rec["max_rel_diff"] = float(np.abs(hip - lib).max() / np.abs(hip - m_k[:, None]).max())
            print(json.dumps(rec), flush=True)
            del blk


if __name__ == "__main__":
    main()
