"""Stage parity of the square-root filter step on whole states: `pnmol_sqrt_filter_step` and `pnmol_sqrt_filter_steps` through
`pnmol._hip.SqrtFilter` alone, on uploaded synthetic factors, compared with the extended-precision truth of
tests/sqrt_reference.py -- the whole covariance C C^T, the same scaled entry by entry to its own standard deviations, all n
derivative rows of the mean, the scalars and the error estimate -- in the Nordsieck frame of the step, at the smallest shape on
either side of every boundary of the step's QRs (`sqrt_reference.CASES`).  Run with -m gpu.

No number is hard-coded: for each case and quantity the bound is 16 max(e64, 2^-52), where e64 is the error of the fp64 NumPy
restatement of the same step against the same truth (the larger of its two routes; for a scalar also over eight orders of the
measurement rows), computed here from the reference alone and printed beside the device's figure (DESIGN.md section 26;
profiles/sqrt_parity/README.md has the measured table).  The fp32 QR is held to 16 max(e32, 2^-23) in the same way.  The device
is compared with the truth, never with the restatement, and never entry by entry of the factor: the posterior is singular to
working precision, so only C C^T is defined (`sqrt_reference`).

What is asserted to the bit: the read-back factor is lower triangular with a non-negative diagonal, and a first step after the
base operator is set again repeats the first step's bits."""

import numpy as np
import pytest

import sqrt_reference as sq
from pnmol import _hip
from stage_figures import Figures as _Figures

pytestmark = pytest.mark.gpu

IDS = {c: sq.case_id(c) for c in sq.CASES}


def _cases(cases):
    return dict(argvalues=cases, ids=[IDS[c] for c in cases])


class Figures(_Figures):
    """The table of stage_figures with the floor of the QR's number format in the bound."""

    def __init__(self, test, case, dtype="f64"):
        super().__init__(test, case, resolve=sq.forward_case)
        self.dtype = dtype

    def add(self, name, e, dev):
        if self.dtype == "f64":
            return super().add(name, e, dev)
        self.rows.append((name, float(e), float(dev)))
        print(f"STAGE {self.head} | {name} | e32 {e:.2e} | device {dev:.2e} | ratio {dev / max(e, sq.EPS32):.2f}")

    def check(self):
        for name, e, dev in self.rows:
            assert dev <= sq.bound_for(e, self.dtype), f"{self.head}: {name}: device {dev:.3e} > 16 max(e = {e:.3e}, floor)"


def _filter(ctx, sc, dtype="f64"):
    """A fresh filter of the case: its first step takes the two QRs as written."""
    return _hip.SqrtFilter(ctx, **sq.filter_arguments(sc), dtype=dtype)


def _read_state(flt, t_expected):
    """(mean (D,), factor) read back; the factor is lower triangular to the bit with diag >= 0."""
    t, mean, C = flt.get_state()
    assert t == t_expected
    assert np.all(np.triu(C, 1) == 0) and np.all(np.diag(C) >= 0)
    return sq.flat(mean), C


def _step(flt, sc, fig, name, truth, ys):
    """One `step` of the state the filter holds against (truth, yardsticks); returns the result's bits."""
    c = sc.c
    t_in = flt.get_state(factor=False)[0]
    flt.prepare_error_model(c.h)
    info, err = flt.step(c.h, want_error=True)
    assert info.info == -1 and info.t_new == t_in + c.h
    mean, C = _read_state(flt, t_in + c.h)
    for k, v in sq.state_errors(c, truth, mean, C).items():
        if k in ("cov", "scaled", "mean"):
            fig.add(f"{name} {k}", ys[k], v)
    for k in sq.SCALARS:
        fig.add(f"{name} {k}", ys[k], sq.rel_scalar(getattr(info, k), getattr(truth, k)))
    fig.add(f"{name} error estimate", ys["error"], sq.vec_error(err, truth.error))
    return mean, C, tuple(getattr(info, k) for k in sq.SCALARS), err


def _upload(flt, sc, factor="tri"):
    flt.set_state(0.0, sc.mean, sc.factors[factor])


def _first_step(flt, sc, fig, name, factor="tri", kind="base", dtype="f64"):
    """Upload and step.  On a fresh filter, or behind `set_operator`, this is the step as written: two QRs."""
    _upload(flt, sc, factor)
    return _step(flt, sc, fig, name, sq.chain_truth(sc.key, 1, factor, kind)[0], sq.yardsticks(sc.key, 1, factor, kind, dtype)[0])


def _one_qr_step(flt, sc, fig, name, factor="tri", kind="base", dtype="f64", taken=0):
    """Warm-up steps until two have been taken with this (h, operator) -- the second of them builds Rc --, then the raw inputs
    again (`set_state` keeps the step history, so the next step takes the one-QR path) and the step that is compared."""
    if taken == 0:
        _upload(flt, sc, factor)
    for _ in range(2 - taken):
        assert flt.step(sc.c.h).info == -1
    return _first_step(flt, sc, fig, name, factor, kind, dtype)


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


# ---- a. the first step of a fresh filter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_cases(sq.CASES))
def test_first_step_from_a_triangular_factor(hip_ctx, case):
    """Two QRs: structured member lists in the predict QR, dense ones in the update QR."""
    sc = sq.sqrt_case(*case)
    fig = Figures("first step", case)
    _first_step(_filter(hip_ctx, sc), sc, fig, "posterior")
    fig.check()


# ---- b. the one-QR step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_cases(sq.CASES))
def test_one_qr_step_from_a_triangular_factor(hip_ctx, case):
    """The default from the second step on: dense rows on the triangle Rc, the `stacked_tri` member lists."""
    sc = sq.sqrt_case(*case)
    fig = Figures("one-QR step", case)
    _one_qr_step(_filter(hip_ctx, sc), sc, fig, "posterior")
    fig.check()


# ---- c. a dense factor of the same covariance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_cases(sq.DENSE_FIRST_CASES))
def test_first_step_from_a_dense_factor(hip_ctx, case):
    """`cl_tri` false: the dense member lists in the predict QR.  The truth is that of the uploaded dense factor."""
    sc = sq.sqrt_case(*case)
    fig = Figures("first step dense factor", case)
    _first_step(_filter(hip_ctx, sc), sc, fig, "posterior", "dense")
    fig.check()


@pytest.mark.parametrize("case", **_cases(sq.DENSE_ONE_QR_CASES))
def test_one_qr_step_from_a_dense_factor(hip_ctx, case):
    """`cl_tri` false in front of the one-QR step ((H T1)^T over whole columns of T1)."""
    sc = sq.sqrt_case(*case)
    fig = Figures("one-QR step dense factor", case)
    _one_qr_step(_filter(hip_ctx, sc), sc, fig, "posterior", "dense")
    fig.check()


# ---- d. the device loop --------------------------------------------------------------------------------------------------------
def _loop(ctx, case, dtype="f64"):
    """`steps(3, h)` on a fresh filter against the three-step chain: step 0 takes two QRs, step 1 builds Rc and is the first one-QR
    step, step 2 the steady one.  Per step the read-outs (derivative-0 mean, std through its square), both scalars and t_new; then
    the final whole state, and the last std against the row sums of squares of the read-back factor (the same sum in another
    order)."""
    K = sq.LOOP_STEPS
    sc = sq.resolve(case)
    c = sc.c
    truths, ys = sq.chain_truth(case, K), sq.yardsticks(case, K, "tri", "base", dtype)
    flt = _filter(ctx, sc, dtype)
    _upload(flt, sc)
    means, stds, infos = flt.steps(K, c.h)
    fig = Figures("loop", case, dtype)
    s0 = sq.sr.scales(c.nu, c.h)[0][0]
    assert [o.info for o in infos] == [-1] * K and [o.t_new for o in infos] == [(k + 1) * c.h for k in range(K)]
    for k, (t, y) in enumerate(zip(truths, ys)):
        fig.add(f"step {k} mean[0]", y["mean0"], float(np.abs(means[k].astype(sq.LD) / s0 - t.m[0::c.n]).max() / np.abs(t.m).max()))
        fig.add(f"step {k} std[0]^2", y["var0"],
                float(np.abs((stds[k].astype(sq.LD) / s0) ** 2 - np.diag(t.P)[0::c.n]).max() / np.abs(t.P).max()))
        for name in sq.SCALARS[:2]:
            fig.add(f"step {k} {name}", y[name], sq.rel_scalar(getattr(infos[k], name), getattr(t, name)))
    mean, C = _read_state(flt, K * c.h)
    for k, v in sq.state_errors(c, truths[-1], mean, C).items():
        if k in ("cov", "scaled", "mean"):
            fig.add(f"final {k}", ys[-1][k], v)
    rows = (C[0::c.n].astype(sq.LD) ** 2).sum(axis=1)
    assert np.all(np.abs(stds[-1].astype(sq.LD) ** 2 - rows) <= 4.0 * sq.EPS * rows)
    assert np.array_equal(means[-1], mean[0::c.n])
    fig.check()


@pytest.mark.parametrize("case", **_cases(sq.LOOP_CASES))
def test_loop_of_three_steps(hip_ctx, case):
    _loop(hip_ctx, case)


# ---- e. other operators --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind", sq.OPERATOR_CASES, ids=[f"{sq.case_id(c)}-{k}" for c, k in sq.OPERATOR_CASES])
def test_steps_with_another_operator(hip_ctx, case, kind):
    """`set_operator(M, shift)`: a diagonal update, a dense one (rows of H longer than 8: the MFMA products `k_rht`, `k_sq_tht`), and
    two banded ones on either side of the ELL width limit (8 entries a row of H: the gather kernels at full width; 9: the dense
    kernels).  A first step, then the one-QR step; after the base operator is set again a first step repeats the first one's bits."""
    sc = sq.sqrt_case(*case)
    op = sq.operator(case, kind)
    assert (sq.row_width(op) <= sq.SQ_ELLW) == (kind in ("diagonal", "band7"))
    flt = _filter(hip_ctx, sc)
    fig = Figures(f"operator {kind}", case)
    plain = _first_step(flt, sc, fig, "base first step")
    flt.set_operator(op.M, op.shift)
    _first_step(flt, sc, fig, "first step", "tri", kind)
    _one_qr_step(flt, sc, fig, "one-QR step", "tri", kind, taken=1)
    flt.set_operator(sc.c.L, None)
    again = _first_step(flt, sc, fig, "base first step again")
    assert _same_bits(plain, again)
    fig.check()


# ---- f. the launch switches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_cases(sq.SWITCH_CASES))
@pytest.mark.parametrize("name,value", sq.SWITCHES, ids=[f"{n}={v}" for n, v in sq.SWITCHES])
def test_switches_hold_the_same_bound(hip_ctx, monkeypatch, name, value, case):
    """Each A/B switch of the step and of the device QR against the truth, under the bound of the default sequence.  The library
    reads them per step (`PNMOL_SQRT_ELL` when an operator is uploaded, so the filter is made behind the switch)."""
    monkeypatch.setenv(name, value)
    sc = sq.sqrt_case(*case)
    fig = Figures(f"{name}={value}", case)
    flt = _filter(hip_ctx, sc)
    _first_step(flt, sc, fig, "first step")
    _one_qr_step(flt, sc, fig, "second sequence", taken=1)
    fig.check()


# ---- g. the fp32 QR ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_cases(sq.F32_CASES))
def test_fp32_qr_steps(hip_ctx, case):
    """`dtype="f32"`: pre-arrays and QRs in fp32, everything else fp64; held to 16 max(e32, 2^-23), e32 from the restatement with
    both pre-arrays rounded to float32 and the QRs in float32."""
    sc = sq.sqrt_case(*case)
    fig = Figures("fp32 QR", case, "f32")
    flt = _filter(hip_ctx, sc, "f32")
    _first_step(flt, sc, fig, "first step", dtype="f32")
    _one_qr_step(flt, sc, fig, "one-QR step", dtype="f32", taken=1)
    fig.check()


@pytest.mark.parametrize("case", **_cases(sq.F32_CASES))
def test_fp32_qr_loop_of_three_steps(hip_ctx, case):
    _loop(hip_ctx, case, "f32")


# ---- h. the latent-force layout ------------------------------------------------------------------------------------------------
LATENT_IDS = [f"latent-{sq.case_id(c)}" for c in sq.LATENT_CASES]


@pytest.mark.parametrize("case", sq.LATENT_CASES, ids=LATENT_IDS)
def test_latent_force_layout_steps(hip_ctx, case):
    """ds = 2d: L = [L, I], B = [B, 0], Gamma = blockdiag(chol K, E_sqrtm), zero noise factors (`update_sqrt_no_meascov`), a
    synthetic state over all n * 2d components; the first step and the one-QR step against the dense longdouble truth."""
    sc = sq.resolve(case)
    fig = Figures("latent", case)
    flt = _filter(hip_ctx, sc)
    _first_step(flt, sc, fig, "first step")
    _one_qr_step(flt, sc, fig, "one-QR step", taken=1)
    fig.check()


@pytest.mark.parametrize("case", sq.LATENT_CASES, ids=LATENT_IDS)
def test_latent_force_layout_loop_of_three_steps(hip_ctx, case):
    """The loop's read-out has width 2d: u, and eps behind it."""
    _loop(hip_ctx, case)
