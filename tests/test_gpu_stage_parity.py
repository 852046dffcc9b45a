"""Stage parity of the post-filter kernels on whole states: `pnmol_smoother_step`, `pnmol_state_predict`, `pnmol_bridge_state`,
`pnmol_samples_draw` and `pnmol_samples_step_back`, one or two calls each on uploaded synthetic inputs, compared with the
extended-precision truths of tests/stage_reference.py on EVERY entry -- all n derivative rows of a mean, the whole covariance --
in the Nordsieck frame of the step.  Run with -m gpu.

No number is hard-coded: for each case and quantity the bound is `stage_reference.bound(e64)` = 16 max(e64, 2^-52), where e64 is
the error of the fp64 NumPy restatement of the same stage against the same truth, computed here from the reference alone and
printed beside the device's figure (profiles/stage_parity/README.md has the measured table).  The device
is compared with the truth, never with the restatement.

Out of scope: `pnmol_bridge_eval`, `pnmol_state_predict_marginals` and `pnmol_samples_interpolate` give marginals or n x n mixes
of what is checked here and keep their tests in test_gpu_dense.py."""

import functools

import numpy as np
import pytest

import stage_reference as sr
from stage_figures import Figures, compare_state as _compare_state

pytestmark = pytest.mark.gpu

IDS = [sr.case_id(c) for c in sr.CASES]
THETAS = (0.03, 0.5, 0.97)


def _pick(*idx):
    return dict(argvalues=[sr.CASES[i] for i in idx], ids=[IDS[i] for i in idx])


@functools.lru_cache(maxsize=None)
def _stage(case):
    """Inputs, truths and the restated smoother step of a case, shared by the tests (read-only)."""
    c = sr.synthetic_case(*case)
    g = sr.gain_truth(c, c.filt[0], c.filt[1], c.h)
    return c, g, sr.rts_truth(c, c.filt, c.succ, c.h, g), sr.restate_rts(c, c.filt, c.succ, c.h)


def _filter(c):
    if getattr(c, "flt", None) is None:
        c.solver.initialize(c.pde)
        c.flt = c.solver._device_filter
    return c.flt


def _upload(flt, t, state):
    s = flt.new_state()
    s.set(t, *state)
    return s


# ---- a. pnmol_smoother_step from raw inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.CASES, ids=IDS)
def test_smoother_step_from_raw_inputs(hip_ctx, case):
    c, _, rts, q = _stage(case)
    flt = _filter(c)
    filt, succ = _upload(flt, 0.0, c.filt), _upload(flt, c.h, c.succ)
    out = flt.smoother_step(filt, succ, c.h)
    assert out.t == 0.0
    fig = Figures("smoother_step", case)
    m, P, v = _compare_state(fig, "smoothed", sr.Frame(c, c.h), out, rts.ms, rts.Ps, q.ms, q.Ps)
    for dev, (m0, P0) in ((filt, c.filt), (succ, c.succ)):                      # the inputs are unchanged, bit for bit
        assert np.array_equal(dev.mean(), m0) and np.array_equal(dev.cov(), P0)
        assert np.array_equal(sr.flat(dev.marginal_var()), np.diag(P0))
    if case == sr.CASES[2]:                                                     # the bridge variant returns the same bits
        out2, bridge = flt.smoother_step(filt, succ, c.h, bridge="marginal")
        assert np.array_equal(out2.mean(), m) and np.array_equal(out2.cov(), P) and np.array_equal(out2.marginal_var(), v)
        assert (bridge.t, bridge.dt) == (0.0, c.h)
    fig.check()


# ---- b. mixed frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_pick(1, 3, 5))
def test_smoother_step_with_inputs_in_other_frames(hip_ctx, case):
    """filt_k sits in the frame of 0.7 h (made by `predict`), smooth_next in that of 1.9 h (made by an earlier smoother step), the
    step under test is taken with h.  The truth starts from the raw mean() and cov() read back from those two device states: the
    stage is judged on its own input; the elementwise rescaling of the read-back (<= 2 ulp) lies inside the tolerance."""
    c = sr.synthetic_case(*case)
    flt = _filter(c)
    filt = flt.predict(_upload(flt, 0.0, c.filt), 0.7 * c.h)
    succ = flt.smoother_step(_upload(flt, 0.0, c.term), _upload(flt, 1.9 * c.h, c.succ), 1.9 * c.h)
    filt_raw, succ_raw = (filt.mean(), filt.cov()), (succ.mean(), succ.cov())
    out = flt.smoother_step(filt, succ, c.h)
    rts = sr.rts_truth(c, filt_raw, succ_raw, c.h)
    q = sr.restate_rts(c, filt_raw, succ_raw, c.h)
    fig = Figures("smoother_step mixed frames", case)
    _compare_state(fig, "smoothed", sr.Frame(c, c.h), out, rts.ms, rts.Ps, q.ms, q.Ps)
    assert np.array_equal(filt.cov(), filt_raw[1]) and np.array_equal(succ.cov(), succ_raw[1])
    assert np.array_equal(filt.mean(), filt_raw[0]) and np.array_equal(succ.mean(), succ_raw[0])
    fig.check()


# ---- c. pnmol_state_predict --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.CASES, ids=IDS)
def test_state_predict(hip_ctx, case):
    c = sr.synthetic_case(*case)
    flt = _filter(c)
    s = _upload(flt, 0.0, c.filt)
    fig = Figures("state_predict", case)
    for f in (0.3, 1.0, 2.5):
        dt = f * c.h
        out = flt.predict(s, dt)
        assert out.t == dt
        m_true, P_true = sr.predict_truth(c, *c.filt, dt)
        m64, P64 = sr.restate_predict(c, *c.filt, dt)
        # (k_dn_predict evaluates every n x n block on its own, A1 (X A1^T) + Q1 K: the blocks (j, k) and (k, j) associate their
        # sums differently, so the two triangles agree to rounding, not to the bit; both are compared with the truth)
        _compare_state(fig, f"dt = {f} h", sr.Frame(c, dt), out, m_true, P_true, m64, P64, symmetric=False)
    assert np.array_equal(s.cov(), c.filt[1]) and np.array_equal(s.mean(), c.filt[0])
    fig.check()


# ---- d. pnmol_bridge_state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_pick(1, 2, 3))
def test_bridge_state(hip_ctx, case):
    c, _, rts, q = _stage(case)
    flt = _filter(c)
    filt, succ = _upload(flt, 0.0, c.filt), _upload(flt, c.h, c.succ)
    out, bridge = flt.smoother_step(filt, succ, c.h, bridge="full")
    fr = sr.Frame(c, c.h)
    fig = Figures("bridge_state", case)
    for th in THETAS:
        st = bridge.state(out, succ, th * c.h)
        assert st.t == th * c.h
        m_true, P_true = sr.bridge_truth(c, rts, th)
        m64, P64 = sr.restate_bridge(c, q, th)
        _compare_state(fig, f"theta = {th}", fr, st, m_true, P_true, m64, P64)
    fig.check()


# ---- e. pnmol_samples_draw ---------------------------------------------------------------------------------------------------
def _draw_factor_columns(flt, c, state, S):
    """A block of S >= D + 1 draws with noise [0; I_D; 0]: column 0 is the mean, the deviations of the next D from it are the
    columns of the factor.  Returns (block, draws (S, n, d))."""
    xi = np.zeros((S, c.D))
    xi[1:c.D + 1] = np.eye(c.D)
    blk = flt.new_samples(S)
    blk.draw(state, xi)
    return blk, blk.get()


@pytest.mark.parametrize("case", **_pick(0, 1, 2, 3, 4, 5))
def test_samples_draw_factor(hip_ctx, case):
    c = sr.synthetic_case(*case)
    flt = _filter(c)
    _, X = _draw_factor_columns(flt, c, _upload(flt, c.h, c.term), c.D + 1)
    assert np.array_equal(X[0], c.term[0])                                      # column 0 equals the mean
    fr = sr.Frame(c, c.h)
    P_true = fr.cov(c.term[1])
    dev = fr.draws(X[1:] - X[0])
    d64 = fr.flat(sr.restate_draw(c, *c.term))
    fig = Figures("samples_draw", case)
    CCt = dev @ dev.T
    fig.add("C C^T", sr.cov_error(d64 @ d64.T, P_true), sr.cov_error(CCt, P_true), CCt, P_true)
    fig.check()


# ---- f. pnmol_samples_step_back, the affine part -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_pick(0, 1, 2, 3, 4, 5))
def test_samples_step_back_affine_part(hip_ctx, case):
    """Zero noise: every column must equal a + G x' for its own x', over all derivative rows."""
    c, g, _, _ = _stage(case)
    flt = _filter(c)
    S = c.D + 1
    blk, Xn = _draw_factor_columns(flt, c, _upload(flt, c.h, c.term), S)
    blk.step_back(_upload(flt, 0.0, c.filt), c.h, np.zeros((S, 2 * c.D)))
    assert blk.t == 0.0
    fr = sr.Frame(c, c.h)
    bd = sr.backward_draw_truth(c, c.filt, c.h, g)
    Xn_raw = np.stack([sr.flat(x) for x in Xn], axis=1)
    X_true = bd.a[:, None] + bd.G @ fr.flat(Xn_raw)
    fig = Figures("samples_step_back affine", case)
    fig.add("a + G x'", sr.vec_error(sr.restate_step_back_affine(c, c.filt, Xn_raw, c.h), X_true),
            sr.vec_error(fr.draws(blk.get()), X_true))
    fig.check()


# ---- g. pnmol_samples_step_back, the law -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,scale", [(sr.CASES[i], 1.0) for i in range(5)] + [(sr.CASES[1], 3.7)],
                         ids=[IDS[i] for i in range(5)] + [IDS[1] + "-scale3.7"])
def test_samples_step_back_law(hip_ctx, case, scale):
    """S = 2 D + 1 draws from one successor point (a terminal draw with zero noise), stepped back with noise [0; I_2D]: the
    deviations from column 0 are the columns of B, and B B^T is the conditional covariance P - G P- G^T (times scale^2), whole
    matrix.  At N = 96 Sp = 640 > 256: the multi-slab path of k_sp_thin."""
    c, g, _, _ = _stage(case)
    flt = _filter(c)
    S = 2 * c.D + 1
    term = flt.new_samples(S)
    term.draw(_upload(flt, c.h, c.term), np.zeros((S, c.D)), scale=scale)
    blk = term.clone()
    xi = np.zeros((S, 2 * c.D))
    xi[1:] = np.eye(2 * c.D)
    blk.step_back(_upload(flt, 0.0, c.filt), c.h, xi, scale=scale)
    Xt = term.get()                                                             # the cloned-from block is untouched
    assert term.t == c.h and all(np.array_equal(x, c.term[0]) for x in Xt)
    X = blk.get()
    fr = sr.Frame(c, c.h)
    bd = sr.backward_draw_truth(c, c.filt, c.h, g)
    cov_true = sr.LD(scale) * sr.LD(scale) * bd.cov
    B = fr.draws(X[1:] - X[0])
    B64 = sr.restate_step_back_law(c, c.filt, sr.flat(c.term[0]), c.h, scale).astype(sr.LD)
    fig = Figures(f"samples_step_back law scale {scale}", case)
    BBt = B @ B.T
    fig.add("B B^T", sr.cov_error(B64 @ B64.T, cov_true), sr.cov_error(BBt, cov_true), BBt, cov_true)
    fig.check()
