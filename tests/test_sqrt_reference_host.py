"""The square-root step's reference by itself (tests/sqrt_reference.py), no GPU: the case list means what its table says -- sizes,
tree levels per QR and path, the panels of the one-QR step that lie in the triangle, the solve blocks --, the synthetic inputs
meet the conditions that make a rounding-level bound possible, and the truth from an uploaded factor agrees with
`oracle.attempt_step` from the same (mean, cov_sqrtm).  The conditions are conditions on the inputs, not measurements: the seed
is fixed; a case that misses one is repaired on the input side, not by the condition."""

import time

import numpy as np
import pytest

import pnmol_oracle as oracle
import sqrt_reference as sq
import stage_reference as sr

IDS = [sq.case_id(c) for c in sq.CASES]
OPERATOR_IDS = [f"{sq.case_id(c)}-{k}" for c, k in sq.OPERATOR_CASES]
PINNED = [c for c in sq.CASES if c[:2] in ((20, 1), (31, 2), (38, 3))]


def _cond(X):
    return float(np.linalg.cond(np.asarray(X, dtype=np.float64)))


def test_case_table_follows_from_the_shapes():
    """D, m, nb2 of the table follow from (N, nu); the member-list arithmetic of `qr_inplace`, restated in `sqrt_reference.shape`,
    puts each case where its comment says."""
    assert len(set(sq.CASES)) == 10
    sh = {}
    for case in sq.CASES:
        s = sh[case[:2]] = sq.shape(case)
        assert (s["D"], s["m"], s["D"] + s["m"], s["nb2"]) == sq.TABLE[case[:2]], case
        assert s["Dtop"] == (s["D"] + 31) // 32 * 32 and s["solve_blocks"] == (s["m"] + 31) // 32
        # a dense QR's first panel has all its row blocks as members; the error model's QR is as tall as the update's
        assert s["qrs"]["update"][0][0] == s["nb2"] == s["qrs"]["error_model"][0][0]
    lv = {k: v["levels"] for k, v in sh.items()}
    one = dict(predict_tri=1, predict_dense=1, update=1, one_qr=1, error_model=1)
    assert lv[(20, 1)] == one and sh[(20, 1)]["Dtop"] == 64 > sh[(20, 1)]["D"]
    assert sh[(20, 1)]["solve_blocks"] == 1 and sh[(20, 1)]["in_triangle"] == []            # never p >= stacked_tri
    assert sh[(30, 2)]["m"] == 32 and sh[(30, 2)]["solve_blocks"] == 1 and sh[(30, 2)]["in_triangle"] == [3]
    assert all(sh[k]["in_triangle"] for k in sh if k != (20, 1))                                # every other case reaches it
    assert sh[(31, 2)]["m"] == 33 and sh[(31, 2)]["solve_blocks"] == 2                         # second diagonal block of one row
    assert sh[(32, 1)]["Dtop"] == sh[(32, 1)]["D"] and all(sh[k]["Dtop"] > sh[k]["D"] for k in sh if k != (32, 1))
    assert sh[(38, 3)]["n"] == 4
    assert lv[(84, 1)]["update"] == 1 and lv[(85, 1)]["update"] == 2                            # nb2 = 8 | 9
    q = sh[(100, 2)]["qrs"]
    assert [p for p, (cnt, _) in enumerate(q["predict_tri"]) if cnt > 8] == list(range(6, 10))   # two levels from panel 6 on
    assert lv[(100, 2)]["predict_tri"] == 2 and lv[(100, 2)]["one_qr"] == 2
    assert all(lv[k]["predict_tri"] == 1 for k in sh if sh[k]["D"] < 300)
    assert lv[(682, 1)]["update"] == 2 and lv[(683, 1)]["update"] == 3                          # nb2 = 64 | 65
    assert max(max(v.values()) for v in lv.values()) == 3
    for k, s in sh.items():       # every panel in the triangle carries the blocks p - stacked_tri .. min(p, nbot - 1)
        st, nbot = s["Dtop"] // 32, s["nb2"]
        assert s["in_triangle"] == list(range(st, nbot))
        assert all(s["qrs"]["one_qr"][p][0] == min(p, nbot - 1) - (p - st) + 1 for p in s["in_triangle"])
    for group in (sq.LARGE_CASES, sq.DENSE_FIRST_CASES, sq.DENSE_ONE_QR_CASES, sq.LOOP_CASES, sq.SWITCH_CASES, sq.F32_CASES,
                  [c for c, _ in sq.OPERATOR_CASES]):
        assert set(group) <= set(sq.CASES)
    assert not set(sq.LARGE_CASES) & set(sq.LOOP_CASES + sq.DENSE_FIRST_CASES + sq.SWITCH_CASES + sq.F32_CASES)


def _conditions(case, truths, label):
    """cond(S) under the cap of its nu, every refined solve at its floor, and the indices the scaled metric leaves out: none with
    Neumann conditions, the derivative-0 entries of the two boundary nodes with Dirichlet conditions."""
    c = sq.resolve(case).c
    cond_s = [_cond(t.S) for t in truths]
    print(f"sqrt reference {label}: D = {c.D}, m = {c.m}, cond(S) = " + ", ".join(f"{x:.2e}" for x in cond_s) +
          f"; last refinement step <= {max(sr.refinement_steps):.1e}")
    assert max(cond_s) <= sq.COND_S_MAX[c.nu]
    assert max(sr.refinement_steps) <= sr.REFINEMENT_FLOOR
    expected = [0, (case[0] - 1) * c.n] if case[2] == "dirichlet" else []
    for t in truths:
        assert list(sq.excluded_indices(t.P)) == expected


@pytest.mark.parametrize("case", sq.CASES, ids=IDS)
def test_inputs_are_well_conditioned(case):
    t0 = time.perf_counter()
    K = sq.LOOP_STEPS if case in sq.LOOP_CASES else 1
    truths = sq.chain_truth(case, K)
    print(f"host time of {K} truth step(s) with the case: {time.perf_counter() - t0:.2f} s")
    _conditions(case, truths, sq.case_id(case))
    # the uploaded factor stands for the synthetic covariance: C C^T = P to rounding, in the frame
    sc = sq.sqrt_case(*case)
    fr = sq.Frame(sc.c, sc.c.h)
    assert sq.cov_error(sq.uploaded_state(case)[1], fr.cov(sc.c.filt[1])) <= 16 * sq.EPS


@pytest.mark.parametrize("case", sq.DENSE_FIRST_CASES, ids=[sq.case_id(c) for c in sq.DENSE_FIRST_CASES])
def test_dense_factor_inputs_are_well_conditioned(case):
    sc = sq.sqrt_case(*case)
    C = sc.factors["dense"]
    assert np.count_nonzero(np.triu(C, 1)) == C.shape[0] * (C.shape[0] - 1) // 2        # dense: `cl_tri` false
    _conditions(case, sq.chain_truth(case, 1, "dense"), f"{sq.case_id(case)} dense factor")
    assert sq.cov_error(sq.uploaded_state(case, "dense")[1], sq.uploaded_state(case)[1]) <= 16 * sq.EPS


@pytest.mark.parametrize("case,kind", sq.OPERATOR_CASES, ids=OPERATOR_IDS)
def test_inputs_with_other_operators_are_well_conditioned(case, kind):
    op = sq.operator(case, kind)
    width = dict(diagonal=4, dense=case[0] + 1, band7=sq.SQ_ELLW, band8=sq.SQ_ELLW + 1)[kind]    # either side of the ELL limit
    assert sq.row_width(op) == width
    _conditions(case, sq.chain_truth(case, 1, "tri", kind), f"{sq.case_id(case)} {kind}")


@pytest.mark.parametrize("case", PINNED, ids=[sq.case_id(c) for c in PINNED])
def test_truth_agrees_with_the_oracle(case):
    """Mean, cov_sqrtm cov_sqrtm^T (whole and scaled) and diffusion_squared_local of `oracle.attempt_step` from the uploaded
    (mean, factor) against the truth, in the metrics of the GPU test, under `bound(e64)` of the restatement."""
    sc = sq.sqrt_case(*case)
    c = sc.c
    t, ys = sq.chain_truth(case)[0], sq.yardsticks(case)[0]
    state = oracle.FilterState(t=0.0, y=oracle.MVN(sc.mean, sc.factors["tri"]), error_estimate=None, reference_state=None,
                               diffusion_squared_local=[])
    new, _ = c.osolver.attempt_step(state, c.h, c.opde)
    fig = sq.state_errors(c, t, sq.flat(new.y.mean), new.y.cov_sqrtm)
    fig["diffusion_squared_local"] = sq.rel_scalar(new.diffusion_squared_local, t.diffusion_squared_local)
    fig["error"] = sq.vec_error(new.error_estimate, t.error)
    print(f"truth against the oracle {sq.case_id(case)}: " + ", ".join(f"{k} e64 {ys[k]:.2e} oracle {v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v <= sq.bound(ys[k]), k


# ---- the latent-force layout ---------------------------------------------------------------------------------------------------
LATENT_IDS = [f"latent-{sq.case_id(c)}" for c in sq.LATENT_CASES]


@pytest.mark.parametrize("case", sq.LATENT_CASES, ids=LATENT_IDS)
def test_latent_inputs_are_well_conditioned(case):
    sc = sq.resolve(case)
    c = sc.c
    assert (c.D, c.m) == {24: (144, 26), 43: (172, 45)}[case[0]] and c.d == 2 * case[0] and c.npde == case[0]
    assert c.D % 32 != 0 and (c.m > 32) == (case[0] == 43)                                # padded rows; one | two solve blocks
    assert not sc.filter_arguments["E_sqrtm"].any() and not sc.filter_arguments["R_sqrtm"].any()      # `update_sqrt_no_meascov`
    _conditions(case, sq.chain_truth(case, sq.LOOP_STEPS), f"latent {sq.case_id(case)}")


@pytest.mark.parametrize("case", sq.LATENT_CASES, ids=LATENT_IDS)
def test_latent_truth_agrees_with_the_oracle(case):
    """`oracle.LatentForceEK1.attempt_step` from the same glued mean and factor against the dense longdouble truth."""
    sc = sq.resolve(case)
    c = sc.c
    t, ys = sq.chain_truth(case)[0], sq.yardsticks(case)[0]
    osolver = oracle.LatentForceEK1(num_derivatives=c.nu, steprule=oracle.Constant(c.h), semilinear=False, canonical_factor_signs=True,
                                    spatial_kernel=oracle.Matern52() + oracle.WhiteNoise())
    osolver.state_iwp, osolver.lf_iwp, osolver.E0, osolver.E1, _ = osolver.initialize_iwp_latent(c.opde)
    state = oracle.FilterState(t=0.0, y=oracle.MVN(sc.mean, sc.factors["tri"]), error_estimate=None, reference_state=None,
                               diffusion_squared_local=[])
    new, _ = osolver.attempt_step(state, c.h, c.opde)
    fig = sq.state_errors(c, t, sq.flat(new.y.mean), new.y.cov_sqrtm)
    fig["diffusion_squared_local"] = sq.rel_scalar(new.diffusion_squared_local, t.diffusion_squared_local)
    print(f"latent truth against the oracle {sq.case_id(case)}: " + ", ".join(f"{k} e64 {ys[k]:.2e} oracle {v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v <= sq.bound(ys[k]), k
