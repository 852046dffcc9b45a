"""Measurement update (`pnmol_state_observe`) on the GPU: ms per update (median of --reps calls into a preallocated output
state, host padding and upload of C, y, R included), the share of the time the unavoidable 16 Dp^2 bytes (P read once, written
once) would take at the HBM rate, and the same update written with torch-ROCm library calls (matmul / torch.linalg.cholesky /
solve_triangular, inputs already on the device) on the same inputs, with the largest difference of the two outputs.
Heat problem, nu = 2, dt = 2^-7, fp64, the state after a few filter steps; q sensors that average two neighbouring nodes, noise
std 1e-6.  One JSON line per (N, q); q > N is skipped.

    python tools/bench_observe.py --mesh-n 256 512 1024 --q 8 64 512 --reps 5
"""

import argparse
import ctypes
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "pnmol-experiments_amd"))

HBM_TBS = 8.0   # spec rate of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-n", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--q", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--nu", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3, help="filter steps before the timed updates")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import pnmol
    from pnmol import _hip

    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for N in args.mesh_n:
        dt = 2.0 ** -7
        pde = pnmol.pde.examples.heat_1d_discretized(dx=1.0 / (N - 1), tmax=args.steps * dt, diffusion_rate=0.05,
                                                     kernel=pnmol.kernels.SquareExponential(), bcond="dirichlet")
        solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=args.nu, steprule=pnmol.odetools.step.Constant(dt),
                                                 spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
        sol = solver.solve(pde)
        state = sol._ys[-1].device_state
        flt = state.filter
        n, d = flt.n, flt.d
        D, Dp = n * d, n * flt.dims()["dp"]
        s, _ = solver.iwp.nordsieck_preconditioner_1d_raw(dt)
        perm = np.array([j * n + a for a in range(n) for j in range(d)])   # derivative-major <- point-major
        sc = np.repeat(s, d)
        frame = lambda mu, P: (mu.reshape(-1) / sc, P[np.ix_(perm, perm)] / np.outer(sc, sc))
        m_in, P_in = frame(state.mean(), state.cov())
        dev = torch.device("cuda")
        t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
        Pt, mt = t(P_in), t(m_in)
        for q in args.q:
            if q > d:
                continue
            left = np.round(np.linspace(1, d - 3, q)).astype(int) if q < d else None
            C = np.eye(d) if left is None else np.zeros((q, d))
            if left is not None:
                C[np.arange(q), left] = C[np.arange(q), left + 1] = 0.5
            rng = np.random.default_rng(q)
            y = C @ state.mean()[0] + 1e-6 * rng.standard_normal(q)
            R = 1e-6 * np.eye(q)
            out, res = flt.new_state(), _hip.ObserveOut()
            call = lambda: flt.lib.pnmol_state_observe(flt.handle, state.handle, q, dp(C), dp(y), dp(R), out.handle,
                                                       ctypes.byref(res))
            assert call() == 0                                  # workspace + first launch
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                rc = call()                                     # (synchronises once: the pivot check and the scalars)
                ts.append(time.perf_counter() - t0)
                assert rc == 0
            ms = 1e3 * float(np.median(ts))
            hm, hP = frame(out.mean(), out.cov())

            # library path: the same update in the frame of the state, derivative-major, on torch-ROCm
            H = np.zeros((q, D))
            H[:, :d] = s[0] * C
            Ht, yt, RRt = t(H), t(y), t(R @ R.T)

            def lib_update():
                HP = Ht @ Pt
                L = torch.linalg.cholesky(HP @ Ht.T + RRt)
                W = torch.linalg.solve_triangular(L, HP, upper=False).T
                w = torch.linalg.solve_triangular(L, (yt - Ht @ mt)[:, None], upper=False)[:, 0]
                ll = -0.5 * (w @ w + 2.0 * torch.log(torch.diagonal(L)).sum() + q * np.log(2.0 * np.pi))
                return mt + W @ w, Pt - W @ W.T, ll

            lib_update()
            torch.cuda.synchronize()
            tl = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                lm, lP, lll = lib_update()
                lll = float(lll)                                # (the scalar comes back, as the HIP call's does)
                tl.append(time.perf_counter() - t0)
            lib_ms = 1e3 * float(np.median(tl))
            floor_ms = 16.0 * Dp * Dp / (HBM_TBS * 1e12) * 1e3
            inc = hm - m_in
            print(json.dumps({"N": N, "nu": args.nu, "q": q, "Dp": Dp, "hip_ms": round(ms, 3), "torch_ms": round(lib_ms, 3),
                              "hbm_floor_ms": round(floor_ms, 4), "floor_share": round(floor_ms / ms, 3),
                              "max_rel_diff_mean_increment": float(np.abs(inc - (lm.cpu().numpy() - m_in)).max() / np.abs(inc).max()),
                              "max_rel_diff_cov": float(np.abs(hP - lP.cpu().numpy()).max() / np.abs(hP).max()),
                              "rel_diff_log_likelihood": abs(res.log_likelihood - lll) / abs(lll)}), flush=True)


if __name__ == "__main__":
    main()
