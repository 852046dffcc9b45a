"""What the whole-state GPU tests share (tests/test_gpu_stage_parity.py, tests/test_gpu_forward_parity.py): the table of
(quantity, e64, device figure) with its final assertion, and the comparison of a device state with a truth."""

import numpy as np

import stage_reference as sr


class Figures:
    """Collects (quantity, e64, device figure), prints them, and asserts device <= bound(e64) at the end."""

    def __init__(self, test, case, resolve=sr.synthetic_case):
        """case: the (N, nu, bcond) key; resolve(*case): its case object, which the per-tile error map needs."""
        self.head, self.case, self.resolve, self.rows = f"{test} {sr.case_id(case)}", case, resolve, []

    def add(self, name, e64, dev, X=None, X_true=None):
        self.rows.append((name, float(e64), float(dev)))
        print(f"STAGE {self.head} | {name} | e64 {e64:.2e} | device {dev:.2e} | ratio {dev / max(e64, sr.EPS):.2f}")
        if dev > sr.bound(e64) and X is not None:
            np.set_printoptions(linewidth=250, precision=1)
            print("per-tile error map (device layout, 64 x 64 tiles):\n", sr.tile_error_map(X, X_true, self.resolve(*self.case)))

    def check(self):
        for name, e64, dev in self.rows:
            assert dev <= sr.bound(e64), f"{self.head}: {name}: device {dev:.3e} > 16 max(e64 = {e64:.3e}, 2^-52)"


def compare_state(fig, name, fr, state, m_true, P_true, m64, P64, symmetric=True):
    """Whole mean, whole covariance (both triangles) and marginal variances of a device state against a truth (frame `fr`);
    var = diag(cov) to the bit, and cov = cov^T to the bit where the kernel mirrors its result (`symmetric`)."""
    P, m, v = state.cov(), state.mean(), state.marginal_var()
    assert not symmetric or np.array_equal(P, P.T)
    assert np.array_equal(sr.flat(v), np.diag(P))
    Ph = fr.cov(P)
    e_cov = sr.cov_error(P64, P_true)
    fig.add(f"{name} cov", e_cov, sr.cov_error(Ph, P_true), Ph, P_true)
    fig.add(f"{name} var", e_cov, float(np.abs(np.diag(Ph) - np.diag(P_true)).max() / np.abs(P_true).max()))
    fig.add(f"{name} mean", sr.vec_error(m64, m_true), sr.vec_error(fr.vec(m), m_true))
    return m, P, v
