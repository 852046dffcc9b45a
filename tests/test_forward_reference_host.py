"""The forward-step reference by itself (tests/forward_reference.py), no GPU: the case list means what its table says, the
synthetic inputs meet the conditions that make a rounding-level bound possible, and the extended-precision truth agrees with
`oracle.attempt_step` from the same state.  The conditions are conditions on the inputs, not measurements: the seed is fixed; a
case that misses one is repaired on the input side (eigenvalue range, size of an operator's perturbation), not by the condition."""

import copy
import time

import numpy as np
import pytest

import forward_reference as fw
import pnmol_oracle as oracle
import stage_reference as sr

ALL = fw.CASES + [fw.DD_BIG_CASE]
IDS = [fw.case_id(c) for c in ALL]
OPERATOR_CASES = [(c, f"diagonal{fw.DIAGONAL_FACTOR}") for c in fw.DIAGONAL_CASES] + [(fw.DENSE_CASE, f"dense{fw.DIAGONAL_FACTOR}")]
OPERATOR_IDS = [f"{fw.case_id(c)}-{k}" for c, k in OPERATOR_CASES]


def _cond(X):
    return float(np.linalg.cond(np.asarray(X, dtype=np.float64)))


def test_case_table_follows_from_the_shapes():
    """m, CB and nreal of the table follow from (N, nu); each case sits where its comment says: at the last shape of one launch
    configuration or at the first of the next."""
    assert len(set(fw.CASES)) == 10
    for case in fw.CASES:
        s = fw.shape(case)
        assert (s["m"], s["CB"], s["nreal"]) == fw.TABLE[case[:2]], case
        assert s["mp"] == 32 * s["CB"] and 0 < s["nreal"] <= 32
    sh = {c[:2]: fw.shape(c) for c in fw.CASES}
    assert sh[(20, 1)]["CB"] == 1 and sh[(20, 1)]["dp"] - 20 == 12
    assert sh[(30, 2)]["m"] == sh[(30, 2)]["mp"] == 32
    assert sh[(31, 2)]["nreal"] < 8 and sh[(38, 3)]["nreal"] == 8 and sh[(38, 3)]["n"] == 4        # short_last_panel(): nreal < 8
    assert sh[(286, 1)]["CB"] == 9 and sh[(287, 2)]["CB"] == 10                                      # k_sweep_rl<.., 9> | <.., 17>
    assert sh[(350, 1)]["CB"] == 11 and sh[(351, 1)]["CB"] == 12                                     # S_SPLIT_FROM = 11: CB > 11 splits
    assert sh[(542, 1)]["CB"] == 17 and sh[(543, 1)]["CB"] == 18                                     # k_sweep_rl | k_sweep
    assert all(c[1] <= 2 for c in fw.LOOP_CASES[:-1]) and fw.LOOP_CASES[-1][1] == 3                  # fused_loop(): n <= 3
    b = fw.shape(fw.DD_BIG_CASE)
    assert (b["dp"], b["Dp"], b["mp"]) == (128, 256, 128)                                            # k_downdate_big: Dp % 128 = 0
    for group in (fw.FRAME_CASES, fw.LOOP_CASES, fw.DIAGONAL_CASES, fw.SWEEP1_CASES, fw.LAYOUT_CASES, [fw.DENSE_CASE]):
        assert set(group) <= set(fw.CASES)


def _conditions(case, truths, label):
    c = fw.forward_case(*case)
    cond_s = [_cond(t.S) for t in truths]
    cond_pm = [_cond(t.Pm) for t in truths]
    print(f"forward reference {label}: D = {c.D}, m = {c.m}, cond(S) = " + ", ".join(f"{x:.2e}" for x in cond_s) +
          "; cond(P-) = " + ", ".join(f"{x:.2e}" for x in cond_pm) + f"; last refinement step <= {max(sr.refinement_steps):.1e}")
    assert max(cond_s) <= fw.COND_S_MAX[c.nu]
    assert cond_pm[0] <= fw.COND_PM_MAX                                  # (first step; a chain's P- is what the filter makes of it)
    assert max(sr.refinement_steps) <= sr.REFINEMENT_FLOOR


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_inputs_are_well_conditioned(case):
    t0 = time.perf_counter()
    K = 3 if case in fw.LOOP_CASES else 1
    truths = fw.chain_truth(case, K)
    print(f"host time of {K} truth step(s) with the case: {time.perf_counter() - t0:.2f} s")
    _conditions(case, truths, fw.case_id(case))


@pytest.mark.parametrize("case,kind", OPERATOR_CASES, ids=OPERATOR_IDS)
def test_inputs_with_other_operators_are_well_conditioned(case, kind):
    _conditions(case, fw.chain_truth(case, 1, kind), f"{fw.case_id(case)} {kind}")


def _oracle_step(c, op):
    """`oracle.attempt_step` from the case's state, set through a Cholesky factor of the uploaded P; another operator enters as
    the semilinear problem with df = M - L and f(x) = (M - L) x - shift (so that its b = J m_at - f is the shift)."""
    opde, osolver = c.opde, c.osolver
    if op is not c.base:
        J = op.M - c.L
        opde = copy.copy(c.opde)
        opde.f, opde.df = (lambda _t, x: J @ x - op.shift), (lambda _t, x: J)
        osolver = copy.copy(c.osolver)
        osolver.semilinear = True
    state = oracle.FilterState(t=0.0, y=oracle.MVN(c.filt[0], np.linalg.cholesky(c.filt[1])), error_estimate=None,
                               reference_state=None, diffusion_squared_local=[])
    new, _ = osolver.attempt_step(state, c.h, opde)
    return new


@pytest.mark.parametrize("case,kind", [(c, "base") for c in ALL] + OPERATOR_CASES, ids=IDS + OPERATOR_IDS)
def test_truth_agrees_with_the_oracle(case, kind):
    """Mean, cov_sqrtm cov_sqrtm^T, diffusion_squared_local and the error estimate of `oracle.attempt_step` (QR form, fp64)
    against the truth, in the metric of the GPU test.  The tolerance is what two fp64 routes allow: `bound(e64)` of the
    restatement, the covariance-form route, for the same quantity."""
    c = fw.forward_case(*case)
    op = fw.operator(case, kind)
    t = fw.chain_truth(case, 1, kind)[0]
    q = fw.restate_step(c, *c.filt, c.h, 0.0, op)
    ys = fw.scalar_yardsticks(c, t, *fw.frame64(c, *c.filt, c.h), op)
    new = _oracle_step(c, op)
    frame = fw.Frame(c, c.h)
    fig = {"mean": (fw.vec_error(q.m, t.m), fw.vec_error(frame.vec(new.y.mean), t.m)),
           "cov": (fw.cov_error(q.P, t.P), fw.cov_error(frame.cov(new.y.cov_sqrtm @ new.y.cov_sqrtm.T), t.P)),
           "diffusion_squared_local": (ys["diffusion_squared_local"], fw.rel_scalar(new.diffusion_squared_local, t.diffusion_squared_local)),
           "error": (ys["error"], fw.vec_error(new.error_estimate, t.error))}
    print(f"truth against the oracle {fw.case_id(case)} {kind}: " +
          ", ".join(f"{k} e64 {a:.2e} oracle {b:.2e}" for k, (a, b) in fig.items()))
    for k, (e64, err) in fig.items():
        assert err <= fw.bound(e64), k


def test_scalars_of_the_truth_do_not_depend_on_the_row_order():
    """`sigma2_whitened` and `error_sigma2` with the measurement rows permuted inside the truth's refined solves agree to
    longdouble rounding times cond(S); the restated `diffusion_squared_local` comes out the same in every order although the
    factor it is defined by depends on the order (the QR that brings each order's factor back to the factor of S)."""
    case = fw.CASES[2]
    c = fw.forward_case(*case)
    t = fw.chain_truth(case, 1)[0]
    Sq = fw.error_model_truth(c, c.base)
    rng = np.random.default_rng(5)
    f = fw._front(c, *fw.frame64(c, *c.filt, c.h), c.base)
    for _ in range(4):
        p = rng.permutation(c.m)
        v = sr._solve_refined(t.S[np.ix_(p, p)], t.z[p])
        vq = sr._solve_refined(Sq[np.ix_(p, p)], t.z[p])
        assert fw.rel_scalar(t.z[p] @ v / c.m, t.sigma2_whitened) <= 1e-19 * _cond(t.S) * 16
        assert fw.rel_scalar(t.z[p] @ vq / c.m, t.error_sigma2) <= 1e-19 * _cond(Sq) * 16
        q = fw._back(c, f, c.base, p)
        assert fw.rel_scalar(q.diffusion_squared_local, t.diffusion_squared_local) <= sr.EPS * _cond(t.S)     # (first-order bound of an fp64 solve)
        assert not np.array_equal(q.Ls, fw._back(c, f, c.base).Ls)
