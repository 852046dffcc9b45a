"""Stage parity of the forward step on whole states: `pnmol_filter_step` and the constant-step loop `pnmol_filter_steps` through
the public API, on uploaded synthetic inputs, compared with the extended-precision truth of tests/forward_reference.py on EVERY
entry -- all n derivative rows of the mean, the whole covariance, the three scalars and the error estimate -- in the Nordsieck
frame of the step, at the smallest shape on either side of every boundary of the sweep launch (`forward_reference.CASES`).
Run with -m gpu.

No number is hard-coded: for each case and quantity the bound is `stage_reference.bound(e64)` = 16 max(e64, 2^-52), where e64 is
the error of the fp64 NumPy restatement of the same step against the same truth (for a scalar: the largest over eight orders of
the measurement rows), computed here from the reference alone and printed beside the device's figure (DESIGN.md section 23;
profiles/forward_parity/README.md has the measured table).  The device is compared with the truth, never with the restatement.
The only other constants are the input conditions cond(S), cond(P-) of tests/test_forward_reference_host.py, asserted on the
CPU wherever an input is made inside a test.

The read-outs of the loop are derivative-0 means and stds; a std is compared through its square (the variance, in the metric of
the covariance): the std of a noise-free Dirichlet node is the root of a rounding residual of P- - W W^T, which no bound of the
form c e64 holds.

Out of scope: `k_w_gemm` (the rows of W as a GEMM behind the sweep) needs mp % 128 == 0 with CB > 17, D about 1280, and stays on
test_gpu_downdate_big.py::test_w_as_a_gemm_behind_the_sweep; fp32 covariances stay on their own tolerance model (DESIGN.md
section 11, test_gpu_fp32.py)."""

import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import forward_reference as fw
from stage_figures import Figures as _Figures, compare_state

pytestmark = pytest.mark.gpu

IDS = {c: fw.case_id(c) for c in fw.CASES + [fw.DD_BIG_CASE]}
CHILD = pathlib.Path(__file__).with_name("forward_child.py")
_ALIVE = []     # solvers of the filters made with an environment switch set (a filter lives as long as its solver)


def _cases(cases):
    return dict(argvalues=cases, ids=[IDS[c] for c in cases])


def Figures(test, case):
    return _Figures(test, case, resolve=fw.forward_case)


def _filter(c):
    """The case's own filter, made on first use with no switch set and kept for the process."""
    if getattr(c, "flt", None) is None:
        c.solver.initialize(c.pde)
        c.flt = c.solver._device_filter
    return c.flt


def _filter_with(case, name, value):
    """A fresh filter of the case created while the environment switch `name` = value (read by `pnmol_filter_create`)."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        pde, solver, _, _ = fw.problem(case)
        solver.initialize(pde)
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old
    _ALIVE.append(solver)
    return solver._device_filter


def _upload(flt, t, state):
    s = flt.new_state()
    s.set(t, *state)
    return s


class _Arrays:
    """mean, covariance and variances that a child process wrote, with the read-out methods of a device state."""

    def __init__(self, m, P, v):
        self._m, self._P, self._v = m, P, v

    def mean(self):
        return self._m

    def cov(self):
        return self._P

    def marginal_var(self):
        return self._v


def _compare_posterior(fig, name, c, state, truth, q):
    """Whole mean and covariance against the truth; var = diag(cov) to the bit.  cov = cov^T holds to rounding, not to the bit, on
    every path measured (fused pairs, `k_downdate`, `k_downdate_big`, first and steady steps of the loop: 53 of 53 states): an
    off-diagonal pair of tiles is computed once and mirrored, but a diagonal tile starts from the tile of P-, whose two triangles
    the predict associates differently, and keeps both.  So nothing is asserted to the bit here; both
    triangles are compared with the truth, and which of the two it is gets printed."""
    m, P, v = compare_state(fig, name, fw.Frame(c, c.h), state, truth.m, truth.P, q.m, q.P, symmetric=False)
    print(f"STAGE {fig.head} | {name} cov == cov^T to the bit: {np.array_equal(P, P.T)}")
    return m, P, v


def _compare_scalars(fig, name, c, truth, ys, scalars, err):
    for k in fw.SCALARS:
        fig.add(f"{name} {k}", ys[k], fw.rel_scalar(scalars[k], getattr(truth, k)))
    fig.add(f"{name} error estimate", ys["error"], fw.vec_error(err, truth.error))


def _scalars(info):
    return {k: getattr(info, k) for k in fw.SCALARS}


def _step(flt, c, fig, name, s, truth, q, ys):
    """One `step` from the device state s against (truth, restatement, scalar yardsticks); returns the result's bits."""
    t_in, m_in, P_in, v_in = s.t, s.mean(), s.cov(), s.marginal_var()
    if flt.error_model_dt != c.h:
        flt.prepare_error_model(c.h)
    out, info, err = flt.step(s, c.h)
    assert info.info == -1 and info.t_new == t_in + c.h and out.t == t_in + c.h
    m, P, v = _compare_posterior(fig, name, c, out, truth, q)
    _compare_scalars(fig, name, c, truth, ys, _scalars(info), err)
    assert s.t == t_in and np.array_equal(s.mean(), m_in) and np.array_equal(s.cov(), P_in)      # the input is unchanged
    assert np.array_equal(s.marginal_var(), v_in)
    return m, P, v, tuple(_scalars(info).values()), err


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _first_step_reference(case, kind="base"):
    c = fw.forward_case(*case)
    op = fw.operator(case, kind)
    truth = fw.chain_truth(case, 1, kind)[0]
    q = fw.restate_step(c, *c.filt, c.h, 0.0, op)
    return c, truth, q, fw.scalar_yardsticks(c, truth, *fw.frame64(c, *c.filt, c.h), op)


# ---- a. one step from raw inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_cases(fw.CASES))
def test_step_from_raw_inputs(hip_ctx, case):
    t0 = time.perf_counter()
    c, truth, q, ys = _first_step_reference(case)
    t1 = time.perf_counter()
    flt = _filter(c)
    layout, sh = flt.sweep_layout(), fw.shape(case)
    dims = flt.dims()
    assert (dims["m"], dims["mp"], dims["dp"]) == (sh["m"], sh["mp"], sh["dp"])
    assert layout["kernel"] == ("k_sweep_rl" if sh["CB"] <= 17 else "k_sweep")
    fig = Figures("step", case)
    _step(flt, c, fig, "posterior", _upload(flt, 0.0, c.filt), truth, q, ys)
    print(f"STAGE step {IDS[case]} | layout {layout} | host reference {t1 - t0:.2f} s | device part {time.perf_counter() - t1:.2f} s")
    fig.check()


# ---- b. a frame change in front of the step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_cases(fw.FRAME_CASES))
def test_step_with_the_input_in_another_frame(hip_ctx, case):
    """The input sits in the frame of 0.6 h (made on the device by `predict`); the step is taken with h, so `launch_step` rescales
    by c.ts != 1.  The truth starts from the raw mean() and cov() read back from that state: the stage is judged on its own input."""
    c = fw.forward_case(*case)
    flt = _filter(c)
    s = flt.predict(_upload(flt, 0.0, c.filt), 0.6 * c.h)
    raw = (s.mean(), s.cov())
    truth = fw.step_truth(c, *raw, c.h)
    cond = float(np.linalg.cond(truth.S.astype(np.float64)))
    print(f"STAGE step other frame {IDS[case]} | cond(S) = {cond:.2e}, cond(P-) = {np.linalg.cond(truth.Pm.astype(np.float64)):.2e}")
    assert cond <= fw.COND_S_MAX[c.nu]
    q = fw.restate_step(c, *raw, c.h)
    fig = Figures("step other frame", case)
    _step(flt, c, fig, "posterior", s, truth, q, fw.scalar_yardsticks(c, truth, *fw.frame64(c, *raw, c.h)))
    fig.check()


# ---- c. the constant-step loop ------------------------------------------------------------------------------------------------
def _loop_reference(case, K):
    c = fw.forward_case(*case)
    truths, qs = fw.chain_truth(case, K), fw.restate_chain(c, K)
    starts = [fw.frame64(c, *c.filt, c.h)] + [(q.m, q.P) for q in qs[:-1]]
    return c, truths, qs, [fw.scalar_yardsticks(c, t, *s0)["diffusion_squared_local"] for t, s0 in zip(truths, starts)]


def _compare_loop(fig, c, ref, means, stds, dsl, final):
    """The read-outs of every step (derivative 0: mean, std through its square) and its diffusion_squared_local, then the final
    whole state."""
    _, truths, qs, ydsl = ref
    s0 = fw.sr.scales(c.nu, c.h)[0][0]
    for k, (t, q) in enumerate(zip(truths, qs)):
        m_scale, P_scale = np.abs(t.m).max(), np.abs(t.P).max()
        m0, v0 = t.m[0::c.n], np.diag(t.P)[0::c.n]
        fig.add(f"step {k} mean[0]", float(np.abs(q.m[0::c.n] - m0).max() / m_scale),
                float(np.abs(means[k].astype(fw.LD) / s0 - m0).max() / m_scale))
        fig.add(f"step {k} std[0]^2", float(np.abs(np.maximum(np.diag(q.P)[0::c.n], 0.0) - v0).max() / P_scale),
                float(np.abs((stds[k].astype(fw.LD) / s0) ** 2 - v0).max() / P_scale))
        fig.add(f"step {k} diffusion_squared_local", ydsl[k], fw.rel_scalar(dsl[k], t.diffusion_squared_local))
    return _compare_posterior(fig, "final", c, final, truths[-1], qs[-1])


def _run_loop(flt, c, K):
    s = _upload(flt, 0.0, c.filt)
    if flt.error_model_dt != c.h:
        flt.prepare_error_model(c.h)
    means, stds, infos = flt.steps(s, K, c.h)
    assert all(o.info == -1 for o in infos) and [o.t_new for o in infos] == [(k + 1) * c.h for k in range(K)] and s.t == K * c.h
    return means, stds, [o.diffusion_squared_local for o in infos], s


@pytest.mark.parametrize("case", **_cases(fw.LOOP_CASES))
def test_loop_of_three_steps(hip_ctx, case):
    """`steps(state, 3, h)` from raw inputs against the three-step truth chain.  The state is uploaded in frame 0, so step 0 is
    STEP_FIRST and the others STEP_STEADY, whose P- the previous step's down-date epilogue made; at nu = 3 the loop is not fused
    (STEP_FULL throughout).  The same call on a fresh upload replays the captured graph and must give the same bits."""
    K = 3
    t0 = time.perf_counter()
    ref = _loop_reference(case, K)
    t1 = time.perf_counter()
    c = ref[0]
    flt = _filter(c)
    means, stds, dsl, s = _run_loop(flt, c, K)
    fig = Figures("loop", case)
    m, P, v = _compare_loop(fig, c, ref, means, stds, dsl, s)
    means2, stds2, dsl2, s2 = _run_loop(flt, c, K)
    assert _same_bits((means, stds, dsl, m, P, v), (means2, stds2, dsl2, s2.mean(), s2.cov(), s2.marginal_var()))
    print(f"STAGE loop {IDS[case]} | host reference {t1 - t0:.2f} s | device part {time.perf_counter() - t1:.2f} s")
    fig.check()


# ---- d. other operators -------------------------------------------------------------------------------------------------------
def _operator_step(case, kind, install):
    """The plain step, the step with another operator against the truth with that operator, and the plain step again after the
    base operator is restored: it must give the first one's bits (those test (a) compares with the truth)."""
    c, truth0, q0, ys0 = _first_step_reference(case)
    flt = _filter(c)
    fig = Figures("step", case)
    plain = _step(flt, c, fig, "posterior", _upload(flt, 0.0, c.filt), truth0, q0, ys0)
    _, truth, q, ys = _first_step_reference(case, kind)
    try:
        install(flt, c)
        assert flt.error_model_dt is None
        _step(flt, c, fig, f"{kind} posterior", _upload(flt, 0.0, c.filt), truth, q, ys)
    finally:
        flt.set_operator_diagonal(np.zeros(c.d))       # (M = L + 0: restores L's stencil rows and a zero shift)
    again = _step(flt, c, Figures("step", case), "posterior", _upload(flt, 0.0, c.filt), truth0, q0, ys0)
    assert _same_bits(plain, again)
    fig.check()


@pytest.mark.parametrize("case", **_cases(fw.DIAGONAL_CASES))
def test_step_with_a_diagonal_operator_update(hip_ctx, case):
    """`set_operator_diagonal(j, shift)`, j uniform in [-1, 1] * 0.5 max|diag L| (tests/test_forward_reference_host.py holds
    cond(S) of this operator to the input condition: the factor 0.5 did not have to shrink), and a random shift, which enters
    the residual as z = H m- + shift (include/pnmol_hip.h)."""
    kind = f"diagonal{fw.DIAGONAL_FACTOR}"

    def install(flt, c):
        _, j, shift = fw.diagonal_operator(c)
        flt.set_operator_diagonal(j, shift)

    _operator_step(case, kind, install)


def test_step_with_a_dense_operator_update(hip_ctx):
    """`set_operator(M, shift)` with M = L + a dense perturbation of the size of the diagonal one (every stencil row becomes d
    wide), at nu = 3."""
    kind = f"dense{fw.DIAGONAL_FACTOR}"

    def install(flt, c):
        op = fw.operator(c.key, kind)
        flt.set_operator(op.M, op.shift)

    _operator_step(fw.DENSE_CASE, kind, install)


# ---- e. the sweep followed by a down-date launch ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_cases(fw.SWEEP1_CASES))
def test_step_and_loop_with_the_down_date_behind_the_sweep(hip_ctx, case):
    """PNMOL_HIP_SWEEP=1 at n <= 3: the sweep alone, then `k_downdate`, in `step` and in the loop (not fused then: STEP_FULL).
    Same truth, same bound."""
    c, truth, q, ys = _first_step_reference(case)
    flt = _filter_with(case, "PNMOL_HIP_SWEEP", "1")
    fig = Figures("step sweep_mode 1", case)
    _step(flt, c, fig, "posterior", _upload(flt, 0.0, c.filt), truth, q, ys)
    means, stds, dsl, s = _run_loop(flt, c, 3)
    _compare_loop(fig, c, _loop_reference(case, 3), means, stds, dsl, s)
    fig.check()


def test_step_with_the_large_problem_down_date(hip_ctx):
    """PNMOL_HIP_DD_BIG=1 at dp = 128, Dp = 256, mp = 128: `k_downdate_big` with a diagonal and an off-diagonal 128-tile."""
    case = fw.DD_BIG_CASE
    c, truth, q, ys = _first_step_reference(case)
    flt = _filter_with(case, "PNMOL_HIP_DD_BIG", "1")
    dims = flt.dims()
    assert dims["dp"] == 128 and dims["mp"] == 128 and c.n * dims["dp"] == 256
    fig = Figures("step dd_big", case)
    _step(flt, c, fig, "posterior", _upload(flt, 0.0, c.filt), truth, q, ys)
    fig.check()


# ---- f. both layouts of k_sweep_rl, each in a process of its own --------------------------------------------------------------
@pytest.mark.parametrize("xl", [1, 0], ids=["xcd-local", "spread"])
def test_both_layouts_in_fresh_processes(hip_ctx, xl):
    """Which filter of a process gets the XCD-local layout depends on what is alive, so tests/forward_child.py runs in a fresh
    child process with PNMOL_HIP_SWEEP_XL forced to 1 or 0, takes one `step` and one `steps(.., 3, ..)` per case, asserts the
    layout it got and writes the results; they are held to the same truths and bounds as above.  No retry: a non-zero exit or a
    timeout fails the test with the child's output."""
    cases = fw.LAYOUT_CASES
    refs = {case: (_first_step_reference(case), _loop_reference(case, 3)) for case in cases}
    env = dict(os.environ, PNMOL_HIP_SWEEP_XL=str(xl))
    with tempfile.TemporaryDirectory() as tmp:
        out = pathlib.Path(tmp) / "forward_child.npz"
        cmd = [sys.executable, str(CHILD), str(out), str(xl)] + [",".join(map(str, c)) for c in cases]
        t0 = time.perf_counter()
        try:
            run = subprocess.run(cmd, env=env, timeout=240, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"forward_child.py timed out:\n{e.stdout}")
        print(f"STAGE layouts xl = {xl} | child process {time.perf_counter() - t0:.2f} s")
        assert run.returncode == 0, f"forward_child.py exited with {run.returncode}:\n{run.stdout}"
        data = dict(np.load(out))
    figs = []
    for case in cases:
        (c, truth, q, ys), loop_ref = refs[case]
        key = IDS[case]
        assert (int(data[f"{key}/xcd_home"]) >= 0) == bool(xl)
        fig = Figures(f"layout xl = {xl}", case)
        _compare_posterior(fig, "step", c, _Arrays(data[f"{key}/step_mean"], data[f"{key}/step_cov"], data[f"{key}/step_var"]),
                           truth, q)
        _compare_scalars(fig, "step", c, truth, ys, dict(zip(fw.SCALARS, data[f"{key}/step_scalars"])), data[f"{key}/step_error"])
        _compare_loop(fig, c, loop_ref, data[f"{key}/loop_means"], data[f"{key}/loop_stds"], data[f"{key}/loop_dsl"],
                      _Arrays(data[f"{key}/loop_mean"], data[f"{key}/loop_cov"], data[f"{key}/loop_var"]))
        figs.append(fig)
    for fig in figs:
        fig.check()
