"""The stage references by themselves (tests/stage_reference.py), no GPU: the synthetic inputs meet the conditions that make a
rounding-level bound possible, every fp64 restatement of the device's algebra sits within 1e-12 of its extended-precision truth,
and the truths agree with the older dense references (smooth_reference, dense_reference, sample_reference) on the same inputs
within those references' own fp64 error.  The conditions are conditions on the inputs, not measurements: the seed is fixed; if a
case misses one, its seed or eigenvalue range changes, not the condition."""

import types

import numpy as np
import pytest

import stage_reference as sr
from dense_reference import bridge_on_oracle, predict
from pnmol.base.iwp import bridge_coefficients
from sample_reference import sample_step
from smooth_reference import rts_step

COND_MAX = 1e4          # cond(P-)
EIG_RATIO_MIN = 1e-3    # smallest / largest eigenvalue of the conditional covariance of a backward draw
RESTATEMENT_MAX = 1e-12
THETAS = (0.03, 0.5, 0.97)
DTS = (0.3, 1.0, 2.5)
IDS = [sr.case_id(c) for c in sr.CASES]


def _step(case):
    c = sr.synthetic_case(*case)
    g = sr.gain_truth(c, c.filt[0], c.filt[1], c.h)
    return c, g, sr.rts_truth(c, c.filt, c.succ, c.h, g), sr.backward_draw_truth(c, c.filt, c.h, g)


@pytest.mark.parametrize("case", sr.CASES, ids=IDS)
def test_inputs_are_well_conditioned_and_restatements_sit_at_rounding_level(case):
    c, g, rts, bd = _step(case)
    i = sr.CASES.index(case)
    cond = float(np.linalg.cond(g.Pm.astype(np.float64)))
    ev = np.linalg.eigvalsh(bd.cov.astype(np.float64))
    fig = {}
    q = sr.restate_rts(c, c.filt, c.succ, c.h)
    fig["smooth cov"], fig["smooth mean"] = sr.cov_error(q.Ps, rts.Ps), sr.vec_error(q.ms, rts.ms)
    fig["gain"], fig["cross"] = sr.cov_error(q.G, rts.G), sr.cov_error(q.C, rts.C)
    for f in DTS:
        mt, Pt = sr.predict_truth(c, *c.filt, f * c.h)
        mq, Pq = sr.restate_predict(c, *c.filt, f * c.h)
        fig[f"predict {f} cov"], fig[f"predict {f} mean"] = sr.cov_error(Pq, Pt), sr.vec_error(mq, mt)
    if i in (1, 2, 3):
        for th in THETAS:
            mt, Pt = sr.bridge_truth(c, rts, th)
            mq, Pq = sr.restate_bridge(c, q, th)
            fig[f"bridge {th} cov"], fig[f"bridge {th} mean"] = sr.cov_error(Pq, Pt), sr.vec_error(mq, mt)
    if i < 6:
        fr = sr.Frame(c, c.h)
        dev = fr.flat(sr.restate_draw(c, *c.term))
        fig["draw cov"] = sr.cov_error(dev @ dev.T, fr.cov(c.term[1]))
        Xn = sr.flat(c.term[0])[:, None] + np.hstack((np.zeros((c.D, 1)), np.linalg.cholesky(c.term[1])))
        fig["step back affine"] = sr.vec_error(sr.restate_step_back_affine(c, c.filt, Xn, c.h), bd.a[:, None] + bd.G @ fr.flat(Xn))
    if i < 5:
        for scale in ((1.0, 3.7) if i == 1 else (1.0,)):
            B = sr.restate_step_back_law(c, c.filt, sr.flat(c.term[0]), c.h, scale).astype(sr.LD)
            fig[f"step back law {scale}"] = sr.cov_error(B @ B.T, scale * scale * bd.cov)
    print(f"stage reference {sr.case_id(case)}: D = {c.D}, Dp = {sr.padded_dim(case)}, cond(P-) = {cond:.2e}, "
          f"eigenvalue ratio = {ev[0] / ev[-1]:.2e}; e64: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert cond <= COND_MAX
    assert ev[0] >= EIG_RATIO_MIN * ev[-1]
    assert max(sr.refinement_steps) <= sr.REFINEMENT_FLOOR
    for k, v in fig.items():
        assert v <= RESTATEMENT_MAX, k


@pytest.mark.parametrize("case", sr.CASES, ids=IDS)
def test_truths_agree_with_the_dense_references(case):
    """`rts_step`, `predict` and `sample_step` on the same raw inputs, in the metric of the stage tests, within the fp64 error of
    those references (the bound of the restatements: they are fp64 restatements in another order)."""
    c, g, rts, bd = _step(case)
    fr = sr.Frame(c, c.h)
    m, P = sr.flat(c.filt[0]), c.filt[1]
    ms, Ps = rts_step(m, P, sr.flat(c.succ[0]), c.succ[1], c.A, c.Q, c.Pc, c.Pcinv)
    fig = {"rts cov": sr.cov_error(fr.cov(Ps), rts.Ps), "rts mean": sr.vec_error(fr.flat(ms), rts.ms)}
    for f in DTS:
        frd = sr.Frame(c, f * c.h)
        mp, Pp = predict(c.osolver, m, P, f * c.h)
        mt, Pt = sr.predict_truth(c, *c.filt, f * c.h)
        fig[f"predict {f} cov"], fig[f"predict {f} mean"] = sr.cov_error(frd.cov(Pp), Pt), sr.vec_error(frd.flat(mp), mt)
    a, G, B = sample_step(m, P, c.A, c.Q, c.Ql, c.Pc, c.Pcinv)
    Bh = fr.flat(B)
    fig["draw offset"] = sr.vec_error(fr.flat(a), bd.a)
    fig["draw gain"] = sr.cov_error(fr.sinv[:, None] * G.astype(sr.LD) / fr.sinv[None, :], bd.G)
    fig["draw law"] = sr.cov_error(Bh @ Bh.T, bd.cov)
    print(f"truths against the dense references {sr.case_id(case)}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v <= RESTATEMENT_MAX, k


@pytest.mark.parametrize("case", sr.CASES[1:4], ids=IDS[1:4])
def test_bridge_truth_agrees_with_the_bridge_on_a_two_point_trajectory(case):
    """`dense_reference.bridge_on_oracle` with the product's host coefficients on the trajectory (filt, succ): its RTS pass makes
    the smoothed state at t_0 from the same two inputs.  The truth's coefficients come from Gaussian conditioning in mpmath."""
    c, g, rts, _ = _step(case)
    fr = sr.Frame(c, c.h)
    osol = types.SimpleNamespace(t=np.array([0.0, c.h]), mean=np.stack((c.filt[0], c.succ[0])),
                                 cov_sqrtm=[np.linalg.cholesky(c.filt[1]), np.linalg.cholesky(c.succ[1])])
    for th in THETAS:
        m, P = bridge_on_oracle(c.osolver, osol, 0, th, bridge_coefficients)
        mt, Pt = sr.bridge_truth(c, rts, th)
        ec, em = sr.cov_error(fr.cov(P), Pt), sr.vec_error(fr.vec(m), mt)
        print(f"bridge {sr.case_id(case)} theta = {th}: cov {ec:.2e}, mean {em:.2e}")
        assert ec <= RESTATEMENT_MAX and em <= RESTATEMENT_MAX


@pytest.mark.parametrize("nu", [1, 2, 3])
def test_bridge_coefficients_by_conditioning(nu):
    """The coefficients derived by conditioning reproduce the prior (B- + B+ A1 = A_theta: no information from the right when
    x_r = A1 x_l) and agree with the closed forms of include/pnmol_hip.h, restated in fp64 here and in the product's host code,
    to cond(Q1) eps (cond(Q1) = 1.6e4 at nu = 3)."""
    full =sr.synthetic_case(*[x for x in sr.CASES if x[1] == nu][0])
    for th in THETAS:
        Bm, Bp, Qb = sr.bridge_coefficients_truth(full, th)
        p = nu - np.arange(nu + 1) + 0.5
        A_th = full.A1x * sr.LD(th) ** (p[:, None] - p[None, :]).astype(sr.LD)
        assert np.abs(Bm + Bp @ full.A1x - A_th).max() <= 1e-17 * np.abs(A_th).max() * 16
        assert np.abs(Qb - Qb.T).max() <= 1e-18 * np.abs(Qb).max() * 16
        for other in (sr.bridge_coefficients64(full, th), bridge_coefficients(th, nu)):
            for X, Y in zip(other, (Bm, Bp, Qb)):
                assert np.abs(X - Y).max() <= 16 * sr.EPS * np.linalg.cond(full.LQ1 @ full.LQ1.T) * max(np.abs(Y).max(), 1.0)
