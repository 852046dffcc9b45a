"""bench.py -- filter steps/sec of the PNMOL white-noise EK1 hot path on MI355X.

`python bench.py --gpus N --steps K --warmup W`  (N>1: launched by torch.distributed.run, one rank
per GPU).  A "step" is one predict+update of the filter (white.py:96-146) on the 1-D heat problem
N=512, nu=2 (BASELINE.json metric / configs).  Each rank owns ONE independent problem of the
diffusion-coefficient sweep kappa_g = 0.01 * 10^(g/7): weak scaling, no collective
in the data path; RCCL only gathers the per-rank read-outs at the end.

Prints ONE JSON line (rank 0).  The timed region is K steps in device calls of at most SEGMENT steps, each bracketed
by a barrier and a device sync on both sides, max over ranks; a plain run times it once, so exactly K steps are timed
and `value` / `ms_per_step` are that region's.  `roofline` prices the whole step against the fp64 MFMA peak with the
ALGORITHMIC flop count F_alg of SURVEY.md section 8d (never the padded/dense count).
`--dump-outputs DIR` writes the read-outs of the last timed call to DIR/<name>.npy (see dump_outputs).

`--full` adds what the headline figure does not need: the timed region is repeated `--repeats` (5) times and `value` /
`ms_per_step` are the MEDIAN repeat (`ms_per_step_all` lists them); `cpu_baseline` times the oracle (reference
algorithm as written, NumPy/LAPACK) on this box's cores.  At N=1 the --full line also carries (each driver-timed
inside this run):
  batch8_on_1gpu   the 8-problem kappa sweep on this ONE GPU, problems one after the other and all in flight
                   -- the 1-GPU baseline north_star's ">= 6x at 8 GPUs on an 8-problem batch" refers to
  secondary        ms/step at N=256, N=1024 (fp64) and on the 64x64 2-d mesh (fp64 and fp32 covariance): BASELINE configs 2, 3, 5;
                   the semilinear step; the square-root (QR) form at the headline size in fp64 and with the fp32 QR
  library_baseline_ms_per_step   the same step written with torch-ROCm library calls (tools/torch_library_step.py)
"""

import argparse
import json
import os
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "pnmol-experiments_amd"))

import numpy as np  # noqa: E402

PEAK_FP64_MFMA_TFLOPS = 78.6   # MI355X fp64 matrix peak (vendor figure)
MESH_N, NU, DT = 512, 2, 2.0 ** -7


def f_alg(D, m, n):
    """Algorithmic flops of one covariance-form step."""
    return m ** 3 / 3 + m ** 2 * D + D ** 2 * m + 4 * n * D ** 2 + 8 * (D * m + m ** 2)


def build_problem(kappa, K, mesh_n=None):
    import pnmol
    N = MESH_N if mesh_n is None else mesh_n
    pde = pnmol.pde.examples.heat_1d_discretized(
        bbox=[0.0, 1.0], dx=1.0 / (N - 1), stencil_size_interior=3, stencil_size_boundary=3, t0=0.0,
        tmax=K * DT, diffusion_rate=kappa, kernel=pnmol.kernels.SquareExponential(), nugget_gram_matrix_fd=0.0,
        bcond="dirichlet")
    solver = pnmol.white.LinearWhiteNoiseEK1(
        num_derivatives=NU, steprule=pnmol.odetools.step.Constant(DT),
        spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
    return pde, solver


def cpu_baseline(seconds_budget=20.0):
    """Oracle (reference algorithm as written: dense Nordsieck products + two QRs per step) on the same
    workload, bounded sample."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import pnmol_oracle as o
    limit_blas_threads()
    pde = o.heat_1d_discretized(bbox=[0.0, 1.0], dx=1.0 / (MESH_N - 1), tmax=100 * DT, diffusion_rate=0.05,
                                kernel=o.SquareExponential(), bcond="dirichlet")
    s = o.WhiteNoiseEK1(num_derivatives=NU, steprule=o.Constant(DT), spatial_kernel=o.Matern52() + o.WhiteNoise())
    state = s.initialize(pde)
    state, _ = s.attempt_step(state, DT, pde)          # warm-up (BLAS threads, caches)
    n, t0 = 0, time.perf_counter()
    while True:
        state, _ = s.attempt_step(state, DT, pde)
        n += 1
        el = time.perf_counter() - t0
        if el > seconds_budget or n >= 100:
            break
    try:
        from threadpoolctl import threadpool_info
        cores = max([t.get("num_threads", 1) for t in threadpool_info()] or [1])   # BLAS threads actually used
    except Exception:
        cores = os.cpu_count()
    # beside it: the same step in covariance/Cholesky form with LAPACK potrf/trsm and dense GEMMs -- what
    # the CPU does once the QR formulation's extra work is removed (a few steps are enough, it is ~10x faster)
    cov_rate = None
    try:
        mean, cov, t = state.y.mean, state.y.cov_sqrtm @ state.y.cov_sqrtm.T, state.t
        t1, m = time.perf_counter(), 0
        while m < 8 and time.perf_counter() - t1 < 6.0:
            mean, cov, _, _ = o.covariance_form_step(s, pde, mean, cov, DT, t)
            t, m = t + DT, m + 1
        cov_rate = m / (time.perf_counter() - t1)
    except Exception:
        pass
    return {"value": n / el, "unit": "steps/s", "cores": cores, "kind": "port", "covariance_form_value": cov_rate,
            "sample": f"{n} steps of the N={MESH_N}, nu={NU} workload after 1 warm-up step; NumPy/SciPy "
                      f"(LAPACK, threaded BLAS on the CPUs the container allows), square-root form as written"}


def cpu_quota():
    """CPUs this process may use: the cgroup quota if there is one (the GPU boxes show 256 cores but allow 16)."""
    n = os.cpu_count() or 1
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(int(q) / int(per))))
    except Exception:
        pass
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    return n


def limit_blas_threads():
    """BLAS threads = the CPUs we are actually allowed (more only burns the cgroup quota and gets throttled).
    Call after the BLAS users (numpy, scipy.linalg: separate OpenBLAS copies) are imported.  Only ever LOWERS a pool:
    an OpenBLAS that started with OMP_NUM_THREADS=1 (what `torch.distributed.run` exports to its workers) has buffers
    for one thread, and raising its thread count afterwards segfaults inside the next LAPACK call."""
    try:
        import scipy.linalg  # noqa: F401
        from threadpoolctl import threadpool_info, threadpool_limits
        local_ranks = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))   # ranks of this node share the quota
        want = max(1, cpu_quota() // local_ranks)
        current = [int(p.get("num_threads", want)) for p in threadpool_info()]
        threadpool_limits(limits=max(1, min([want] + current)))
    except Exception:
        pass


def _hip_device_count():
    import ctypes
    from pnmol import _hip
    n = ctypes.c_int(0)
    _hip.load_library().pnmol_device_count(ctypes.byref(n))
    return n.value


def _bound_problem(kappa, K, device, mesh_n=None):
    """(context, device filter, device state) of one problem of the sweep, initialised and ready to step."""
    from pnmol import _hip
    pde, solver = build_problem(kappa, K, mesh_n)
    ctx = _hip.Context(device)                        # own stream per problem
    solver._context = ctx
    state = solver.initialize(pde)
    solver._ensure_error_model(pde, DT)
    return ctx, solver._device_filter, state.y.device_state


def batch8_on_one_gpu(device, K):
    """north_star's 8-problem batch (kappa sweep, N=512, nu=2) on ONE GPU: problems one after the other, and all eight in
    flight (one stream each).  Steps/s of the whole batch; device work only (state resident, graphs prepared)."""
    from pnmol import batch
    probs = [_bound_problem(batch.diffusion_sweep(g, 8), 2 * K + 4, device) for g in range(8)]
    for _, flt, dev in probs:
        flt.steps(dev, 2, DT)
        flt.prepare_steps(dev, K, DT)
    time.sleep(0.2)
    for ctx, _, _ in probs:
        ctx.synchronize()
    t0 = time.perf_counter()
    for ctx, flt, dev in probs:                       # serial: each problem alone on the device
        flt.steps_begin(dev, K, DT)
        flt.steps_end(dev, want_means=True, want_stds=True)
    serial = time.perf_counter() - t0
    for _, flt, dev in probs:
        flt.prepare_steps(dev, K, DT)
    for ctx, _, _ in probs:
        ctx.synchronize()
    t0 = time.perf_counter()
    for _, flt, dev in probs:                         # concurrent: enqueue all, then collect
        flt.steps_begin(dev, K, DT)
    res = [flt.steps_end(dev, want_means=True, want_stds=True) for _, flt, dev in probs]
    conc = time.perf_counter() - t0
    ok = all(np.all(np.isfinite(m)) and all(o.info == -1 for o in infos) for m, _, infos in res)
    return {"problems": 8, "steps_each": K, "serial_steps_per_s": 8 * K / serial, "concurrent_steps_per_s": 8 * K / conc,
            "valid": bool(ok)}


def secondary_points(device):
    """BASELINE configs 1, 2 and 4 (fp64): ms per step of the device loop, HIP events on the launch stream."""
    out = []
    for mesh_n, K in ((256, 40), (1024, 20)):
        try:
            ctx, flt, dev = _bound_problem(0.05, K + 4, device, mesh_n)
            flt.steps(dev, 2, DT)
            flt.prepare_steps(dev, K, DT)
            flt.steps(dev, K, DT)
            ms = flt.last_steps_ms() / K
            n, d = NU + 1, mesh_n
            out.append({"workload": f"1-D heat N={mesh_n} nu={NU}", "ms_per_step": ms,
                        "frac_of_fp64_mfma_peak": f_alg(n * d, d + 2, n) / (ms * 1e-3) / 1e12 / PEAK_FP64_MFMA_TFLOPS})
            del ctx, flt, dev
        except Exception as e:   # a secondary point must never take the headline line down
            out.append({"workload": f"1-D heat N={mesh_n} nu={NU}", "error": repr(e)[:200]})
    # BASELINE config 5's mesh in fp64 and in its stated precision (fp32 covariance)
    for dtype in ("f64", "f32"):
        name = f"2-D heat 64x64 mesh nu=1 ({'fp64' if dtype == 'f64' else 'fp32 covariance'})"
        try:
            import pnmol
            dt2, K = 2.0 ** -9, 4
            pde = pnmol.pde.examples.heat_2d_dirichlet_discretized(nums=(64, 64), tmax=(K + 2) * dt2, diffusion_rate=0.05,
                                                                   kernel=pnmol.kernels.SquareExponential())
            solver = pnmol.white.LinearWhiteNoiseEK1(num_derivatives=1, steprule=pnmol.odetools.step.Constant(dt2),
                                                     spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
            solver.dtype = dtype
            state = solver.initialize(pde)
            flt, dev = solver._device_filter, state.y.device_state
            solver._ensure_error_model(pde, dt2)
            flt.steps(dev, 1, dt2)
            flt.prepare_steps(dev, K, dt2)
            flt.steps(dev, K, dt2)
            ms = flt.last_steps_ms() / K
            dd = flt.dims()
            D, mm, nn = dd["n"] * dd["d"], dd["m"], dd["n"]
            row = {"workload": name, "ms_per_step": ms}
            if dtype == "f64":
                row["frac_of_fp64_mfma_peak"] = f_alg(D, mm, nn) / (ms * 1e-3) / 1e12 / PEAK_FP64_MFMA_TFLOPS
            out.append(row)
            del solver, state, flt, dev
        except Exception as e:
            out.append({"workload": name, "error": repr(e)[:200]})
    try:
        # semilinear EK1 (white.py:189-208) on the reference's spruce-budworm recipe: one attempt_step per call -- predicted
        # mean to the host, f / df there (Python callables, as in the reference), new stencil rows to the device, step
        import pnmol
        dts, K, Ns = 2.0 ** -7, 20, 256
        spde = pnmol.pde.examples.spruce_budworm_1d_discretized(dx=1.0 / (Ns - 1), tmax=(K + 4) * dts, diffusion_rate=0.05,
                                                                kernel=pnmol.kernels.SquareExponential())
        row = {"workload": f"spruce budworm N={Ns} nu={NU}, SemiLinearWhiteNoiseEK1.attempt_step (host wall clock per step)"}
        for key, diagonal in (("ms_per_step", True), ("ms_per_step_dense_operator_upload", False)):
            ssolver = pnmol.white.SemiLinearWhiteNoiseEK1(num_derivatives=NU, steprule=pnmol.odetools.step.Constant(dts),
                                                          spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
            if not diagonal:
                spde.df_diagonal = None
            st = ssolver.initialize(spde)
            for _ in range(3):
                st, _ = ssolver.attempt_step(st, dts, spde)
            t0 = time.perf_counter()
            for _ in range(K):
                st, _ = ssolver.attempt_step(st, dts, spde)
            row[key] = 1e3 * (time.perf_counter() - t0) / K
        out.append(row)
    except Exception as e:
        out.append({"workload": "spruce budworm semilinear step", "error": repr(e)[:200]})
    # the step in the reference's own square-root (QR) form on the headline problem (pnmol.sqrtform): fp64, and
    # the fp32 build of the QR -- the fp32 mode for nu = 2 (section 11).  Steady state: the first two steps of a call
    # (two QRs each, and the step-invariant rows) are run before the timed ones.
    for dtype in ("f64", "f32"):
        name = f"1-D heat N={MESH_N} nu={NU}, square-root (QR) form, {'fp64' if dtype == 'f64' else 'fp32 QR'}"
        try:
            import pnmol
            K = 10
            pde, _ = build_problem(0.05, K + 3)
            s = pnmol.sqrtform.LinearWhiteNoiseEK1(num_derivatives=NU, steprule=pnmol.odetools.step.Constant(DT),
                                                    spatial_kernel=pnmol.kernels.Matern52() + pnmol.kernels.WhiteNoise())
            s.dtype = dtype
            st = s.initialize(pde)
            s._load(st, pde)
            s._sqrt_filter.steps(3, DT)
            s._sqrt_filter.steps(K, DT)
            out.append({"workload": name, "ms_per_step": s._sqrt_filter.last_steps_ms() / K})
            del s, st
        except Exception as e:
            out.append({"workload": name, "error": repr(e)[:200]})
    return out


def library_baseline_ms():
    """tools/torch_library_step.py (rocBLAS / rocSOLVER through torch) in a child process with a time limit: the first
    `import torch` on a fresh box can take minutes."""
    try:
        out = subprocess.run([sys.executable, str(ROOT / "tools" / "torch_library_step.py"), "--steps", "30"],
                             capture_output=True, text=True, timeout=float(os.environ.get("PNMOL_BENCH_LIB_TIMEOUT", "240")))
        return json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"]
    except Exception:
        return None


DUMP_BYTES = 64 * 10 ** 6   # cap on what --dump-outputs writes
# Longest device call.  In fp64 the covariance form of the bench problems stops being positive definite after ~1650
# steps at kappa = 0.05 (~1300 at kappa = 0.1, the top of the sweep), so longer runs are cut into calls that each
# restart from the same state (see main).
SEGMENT = 500


def segments(k):
    """k steps as near-equal device calls of at most SEGMENT steps."""
    n = -(-k // SEGMENT)
    return [k // n + (i < k % n) for i in range(n)]


def dump_outputs(outdir, results):
    """The read-outs of the last timed call as its caller receives them (`Filter.steps_end`), stacked over this rank's
    problems: means / stds (B, K, d) and the per-step scalars of `StepOut` (B, K), all float64.  Above DUMP_BYTES the K
    steps are cut to a fixed seeded sample (in step order; `t_new` says which steps were kept)."""
    arrays = {"means": np.stack([r[0] for r in results]), "stds": np.stack([r[1] for r in results])}
    for name in ("t_new", "diffusion_squared_local", "sigma2_whitened", "error_sigma2"):
        arrays[name] = np.array([[getattr(o, name) for o in infos] for _, _, infos in results])
    k = arrays["means"].shape[1]
    per_step = sum(a[:, 0].nbytes for a in arrays.values())
    if per_step * k > DUMP_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(k, DUMP_BYTES // per_step, replace=False))
        arrays = {name: a[:, rows] for name, a in arrays.items()}
    os.makedirs(outdir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(outdir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: 5 timed repeats (median reported), the CPU "
                         "baseline and, at N=1, batch8_on_1gpu, the secondary points and the library baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the read-outs of the last timed call (rank 0's problems) to DIR/<name>.npy")
    ap.add_argument("--repeats", type=int, default=None,
                    help="timed repeats of the K-step region; the median is reported (default 1, 5 with --full)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full without batch8_on_1gpu, the secondary points and the library baseline (N=1 only has them)")
    ap.add_argument("--problems-per-gpu", type=int, default=1,
                    help="independent problems run concurrently on each GPU (one context/stream and host thread each); "
                         "the headline metric uses 1")
    ap.add_argument("--mesh-n", type=int, default=MESH_N,
                    help="secondary measurement points (BASELINE configs 256 / 1024); the headline metric is 512")
    args = ap.parse_args()
    globals()["MESH_N"] = args.mesh_n
    repeats = max(1, args.repeats if args.repeats is not None else (5 if args.full else 1))

    limit_blas_threads()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # PNMOL_BENCH_FORCE_DIST=1: initialise the process group and run every collective of the N>1 path with ONE rank
    # (no short-circuit): proves on a one-GPU box that RCCL loads beside libpnmol_hip.so's own HIP context and that
    # device tensors round-trip through all_gather / all_reduce (profiles/r03_nccl_world1.log).
    force_dist = os.environ.get("PNMOL_BENCH_FORCE_DIST", "0") == "1"
    if force_dist and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if world > 1 or force_dist:
        import torch
        import torch.distributed as dist
        ndev = max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_rank % ndev)
        # "nccl" is RCCL on ROCm.  PNMOL_BENCH_BACKEND=gloo is only for rehearsing N>1 ranks on a 1-GPU box.
        backend = os.environ.get("PNMOL_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank % ndev))
        else:
            dist.init_process_group(backend)
    coll_dev = "cuda" if os.environ.get("PNMOL_BENCH_BACKEND", "nccl") == "nccl" else "cpu"
    os.environ["PNMOL_HIP_DEVICE"] = str(local_rank)

    from pnmol import batch
    B = max(1, args.problems_per_gpu)
    device = local_rank % max(1, _hip_device_count())
    # one problem per rank: problem g of the 8-problem diffusion sweep (kappa = 0.05 for the single-GPU headline);
    # with --problems-per-gpu B every rank owns B consecutive problems of a (world*B)-problem sweep
    probs, kappas = [], []
    for b in range(B):
        gidx = rank * B + b
        kappa = 0.05 if world * B == 1 else batch.diffusion_sweep(gidx, max(world * B, 8))
        kappas.append(kappa)
        probs.append(_bound_problem(kappa, args.warmup + args.steps * repeats, device))

    def sync_all():
        for ctx, _, _ in probs:
            ctx.synchronize()
        if dist is not None:
            import torch
            dist.barrier()
            torch.cuda.synchronize()

    def run_all(states, k, outputs):
        # enqueue every problem's k steps (asynchronous), then collect: the streams run concurrently on the device
        for (_, flt, _), st in zip(probs, states):
            flt.steps_begin(st, k, DT)
        return [flt.steps_end(st, want_means=outputs, want_stds=outputs) for (_, flt, _), st in zip(probs, states)]

    # The host-side setup above (LAPACK on many threads) can exhaust the container's CPU quota; the kernel then
    # throttles the whole process for the rest of the 100 ms period, which shows up as a 20-90 ms hole in a 10-20 ms
    # timed region (seen in 1 of 6 runs at N=256).  Let the quota refill before the device work.  The pause comes
    # before the warm-up, not before the timed region: a timed region that follows an idle GPU ran 1-4 % slower.
    time.sleep(float(os.environ.get("PNMOL_BENCH_SETTLE", "0.3")))
    # Device calls of at most SEGMENT steps: the first warm-up call advances the problems; every later call (warm-up or
    # timed) runs on an exact copy of where that call ended, so no problem is ever stepped past 2 * SEGMENT steps.
    starts = [dev for _, _, dev in probs]
    for i, k in enumerate(segments(args.warmup)):
        run_all(starts if i == 0 else [s.clone() for s in starts], k, False)
    walls, devs, results = [], [], None
    for rep in range(repeats):
        wall = dev_ms = 0.0
        for k in segments(args.steps):
            states = None                                 # (frees the previous call's copies first)
            states = [s.clone() for s in starts]
            for (_, flt, _), st in zip(probs, states):
                flt.prepare_steps(st, k, DT)              # host work and a rehearsal (buffers, hipGraph instantiation)
            sync_all()
            t0 = time.perf_counter()
            results = run_all(states, k, True)            # k steps per problem, one host sync at the end
            sync_all()
            wall += time.perf_counter() - t0
            dev_ms += max(p[1].last_steps_ms() for p in probs)  # HIP events on each problem's stream
        if dist is not None:
            wall = batch.max_over_ranks(wall, dist, device=coll_dev, force=force_dist)
        walls.append(wall)
        devs.append(dev_ms)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, results)
    order = np.argsort(walls)
    med = int(order[len(order) // 2])
    wall, dev_ms = walls[med], devs[med]
    means, stds, infos = results[0]
    for mm_, ss_, ii_ in results[1:]:
        means, stds = np.concatenate([means, mm_]), np.concatenate([stds, ss_])
        infos = list(infos) + list(ii_)

    sig = np.array([o.diffusion_squared_local for o in infos])
    ok = bool(np.all(np.isfinite(means)) and np.all(np.isfinite(stds)) and all(o.info == -1 for o in infos))
    kappa_by_rank = [kappas]
    if dist is not None:
        # the final gather of the per-problem read-outs -- the only collective of the path (RCCL over xGMI)
        gathered = batch.gather_readouts(np.concatenate([means.ravel(), stds.ravel(), sig]), dist, device=coll_dev, force=force_dist)
        assert gathered.shape[0] == world, f"gathered read-outs of {gathered.shape[0]} ranks, world is {world}"
        kappa_by_rank = batch.gather_readouts(np.array(kappas), dist, device=coll_dev, force=force_dist).tolist()
        ok = bool(batch.max_over_ranks(0.0 if ok else 1.0, dist, device=coll_dev, force=force_dist) == 0.0) and bool(np.all(np.isfinite(gathered)))

    if rank == 0:
        n, d = NU + 1, MESH_N
        D, m = n * d, d + 2
        steps_per_s = world * B * args.steps / wall
        flops = f_alg(D, m, n)
        # B = 1: HIP events on the launch stream.  B > 1: the streams overlap only partially, so the honest
        # per-step device time is the wall time of the whole batch divided by all its steps.
        step_ms_dev = dev_ms / args.steps if B == 1 else 1e3 * wall / (args.steps * B)
        achieved = flops / (step_ms_dev * 1e-3) / 1e12
        traffic, traffic_src = None, None
        try:   # HBM bytes per step from the committed PMC profile (rocprofv3 cannot run inside this process)
            if MESH_N == 512:
                tj = json.load(open(ROOT / "profiles" / "traffic.json"))
                traffic, traffic_src = tj["hbm_bytes_per_step"], tj.get("source")
        except Exception:
            pass
        line = {
            "metric": f"filter steps/sec, 1D heat N={MESH_N} nu={NU} (white-noise EK1 predict+update)",
            "value": steps_per_s, "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * wall / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "repeats": len(walls), "ms_per_step_all": [1e3 * w / args.steps for w in walls],
            "config": {"workload": f"1-D heat equation, N={MESH_N} mesh, IWP(nu={NU}) EK1, Dirichlet, dt=2^-7, "
                                   f"one problem per GPU (kappa sweep), D={D}, m={m}",
                       "steps_in_one_call": args.steps, "valid": ok, "problems_per_gpu": B,
                       "device_ms_per_step": step_ms_dev, "kappa_by_rank": kappa_by_rank,
                       "sweep_layout": probs[0][1].sweep_layout(),
                       "collectives": ("%s, one rank, forced" % os.environ.get("PNMOL_BENCH_BACKEND", "nccl")) if (force_dist and world == 1)
                                      else (os.environ.get("PNMOL_BENCH_BACKEND", "nccl") if world > 1 else None)},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_FP64_MFMA_TFLOPS, "traffic": traffic, "traffic_source": traffic_src,
                         "note": "unit = one filter step (the kernel graph of one predict+update): F_alg = %.4g "
                                 "flop/step (SURVEY 8d), duration = HIP events on the launch stream / steps (median "
                                 "repeat); traffic = HBM bytes/step from the committed PMC profile (not of this run), "
                                 "B_alg = %.3g" % (flops, 3 * D * D * 8)},
        }
        if world == 1:
            line["cpu_baseline"] = cpu_baseline() if args.full and not args.no_cpu_baseline else None
            if args.full and not args.no_extras and B == 1 and MESH_N == 512:
                del probs[:], starts[:], states[:]            # release the headline problem's device memory first
                line["batch8_on_1gpu"] = batch8_on_one_gpu(device, min(args.steps, SEGMENT // 2))  # steps each problem 2 + 2K times
                line["secondary"] = secondary_points(device)
                line["library_baseline_ms_per_step"] = library_baseline_ms()
        else:
            line["cpu_baseline"] = None      # (reported by the N=1 line, with batch8_on_1gpu as the scaling reference)
        print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
