"""`solver.smooth(sol)` per step with the package of the tree given as the first argument (this repository or an export of
another commit of it, built): one JSON line.  tools/ab_smooth.sh alternates two trees with it.

    python tools/bench_smooth_ab.py TREE [N] [STEPS] [LABEL]
"""
import json
import os
import sys
import time

import numpy as np

tree = os.path.abspath(sys.argv[1])
N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
label = sys.argv[4] if len(sys.argv) > 4 else tree
sys.path.insert(0, tree + "/pnmol-experiments_amd")
import pnmol  # noqa: E402

assert pnmol.__file__.startswith(tree), pnmol.__file__
dt = 2.0 ** -7
pde = pnmol.pde.examples.heat_1d_discretized(dx=1.0 / (N - 1), tmax=steps * dt, diffusion_rate=0.05,
                                             kernel=pnmol.kernels.SquareExponential(), bcond="dirichlet")
solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=2, steprule=pnmol.odetools.step.Constant(dt),
                                         spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
sol = solver.solve(pde)
s = solver.smooth(sol)                                  # workspace + first launches
del s
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    s = solver.smooth(sol)                              # (each tree's default: bridges where the tree has them)
    ts.append((time.perf_counter() - t0) / steps * 1e3)
    del s
print(json.dumps({"what": "smooth_ab", "tree": label, "N": N, "steps": steps, "median_ms_per_step": round(float(np.median(ts)), 4),
                  "min": round(min(ts), 4), "max": round(max(ts), 4)}), flush=True)
