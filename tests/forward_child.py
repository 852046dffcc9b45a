"""Child process of tests/test_gpu_forward_parity.py::test_both_layouts_in_fresh_processes (a plain script, not a test module):

    python forward_child.py OUT.npz XL N,nu,bcond [N,nu,bcond ...]

Rebuilds the named cases of tests/forward_reference.py from their seeds, creates each case's filter in this fresh process (the
parent sets PNMOL_HIP_SWEEP_XL = XL in the environment), asserts that the filter got the XCD-local layout (XL = 1) or the spread
one (XL = 0), takes one `step` and one `steps(.., 3, ..)` from the raw inputs and writes mean, covariance, variances and scalars
to OUT.npz.  Any error ends the process at once with a non-zero exit status; nothing is started after it."""

import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "pnmol-experiments_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402

import forward_reference as fw  # noqa: E402


def main(out, xl, names):
    data = {}
    for name in names:
        N, nu, bcond = name.split(",")
        case = (int(N), int(nu), bcond)
        c = fw.forward_case(*case)
        c.solver.initialize(c.pde)
        flt = c.solver._device_filter
        layout = flt.sweep_layout()
        assert layout["kernel"] == "k_sweep_rl" and (layout["xcd_home"] >= 0) == bool(xl), (case, layout)
        key = fw.case_id(case)
        data[f"{key}/xcd_home"] = np.array(layout["xcd_home"])
        flt.prepare_error_model(c.h)
        s = flt.new_state()
        s.set(0.0, *c.filt)
        o, info, err = flt.step(s, c.h)
        assert info.info == -1, (case, info.info)
        data[f"{key}/step_mean"], data[f"{key}/step_cov"], data[f"{key}/step_var"] = o.mean(), o.cov(), o.marginal_var()
        data[f"{key}/step_scalars"] = np.array([getattr(info, k) for k in fw.SCALARS])
        data[f"{key}/step_error"] = err
        means, stds, infos = flt.steps(s, 3, c.h)
        assert all(i.info == -1 for i in infos), (case, [i.info for i in infos])
        data[f"{key}/loop_means"], data[f"{key}/loop_stds"] = means, stds
        data[f"{key}/loop_dsl"] = np.array([i.diffusion_squared_local for i in infos])
        data[f"{key}/loop_mean"], data[f"{key}/loop_cov"], data[f"{key}/loop_var"] = s.mean(), s.cov(), s.marginal_var()
        print(f"forward_child {key}: layout {layout}", flush=True)
    np.savez(out, **data)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3:])
