"""The input-dimension sweep of tests/test_gpu_input_dims.py is not vacuous: on the oracle alone, every one of the d lengthscales and
every one of the d input coordinates moves what the sweep compares by more than the sweep's gates, so a device kernel that dropped,
duplicated or mis-scaled one coordinate would fail them.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dims_problem as P  # noqa: E402

N, C, NOISE = 200, 518, 1e-4                            # the shape of test_fixed_hyps_every_dimension


@pytest.mark.parametrize("d", [1, 8, 17, 32])
def test_every_lengthscale_moves_the_posterior_beyond_the_gates(d):
    """l_q -> 1.01 l_q, one coordinate q at a time (all three outputs at once): in every output the variances move by at least 10 x the
    variance gate and the means leave the mean gate.  Measured: smallest variance move 1.5e-7 (d = 1), 4.5e-5 (d = 8), 9.0e-5 (d = 17),
    1.2e-4 (d = 32); smallest excess of the mean over its gate 9.9e-6 (d = 1)."""
    p, ref = P.oracle(d, N, C, NOISE)
    mean, var = P.predict_once(ref, p["Xc"])
    var_move, excess = np.inf, np.inf
    for q in range(d):
        ls = [l.copy() for l in p["lengthscales"]]
        for l in ls:
            l[q] *= 1.01
        mean_q, var_q = P.predict_once(P.fit_oracle(p, ls), p["Xc"])
        for j in range(len(P.KINDS)):
            dv, ex = np.abs(var_q[j] - var[j]).max(), P.mean_excess(mean_q[j], mean[j])
            assert dv >= 10 * P.VAR_GATE, (q, j, dv)
            assert ex > 0.0, (q, j, ex)
            var_move, excess = min(var_move, dv), min(excess, ex)
    print("d %d: smallest variance move %.3g (gate %.1g), smallest mean excess over its gate %.3g" % (d, var_move, P.VAR_GATE, excess))


@pytest.mark.parametrize("d", [1, 8, 17, 32])
def test_every_coordinate_has_a_gradient(d):
    p, ref = P.oracle(d, N, C, NOISE)
    Xg = p["Xc"][:40]                                   # the gradient candidates of the sweep (tile path; its first 7 take the small path)
    dmean, dvar = ref.posterior_mean_gradient(Xg), ref.posterior_variance_gradient(Xg)
    assert dmean.shape == dvar.shape == (len(P.KINDS), 40, d)
    for q in range(d):
        for j in range(len(P.KINDS)):
            assert np.abs(dmean[j, :7, q]).max() > 0.0 and np.abs(dvar[j, :7, q]).max() > 0.0, (q, j)
            assert np.abs(dmean[j, :, q]).max() > 0.0 and np.abs(dvar[j, :, q]).max() > 0.0, (q, j)


def test_acquisition_inputs_have_a_gradient_in_every_coordinate():
    """The supports the sweep hands to maEI and uEI_noiseless give, for every d, an oracle acquisition gradient that is non-zero in each
    of the d coordinates (dims_problem.acquisition_inputs raises when no pair of candidates does)."""
    for d in range(1, 33):
        for key, (support, acq, dacq) in P.acquisition_inputs(d, N, C, NOISE).items():
            assert support.shape == (2, len(P.KINDS)) and dacq.shape == (P.N_ACQ, d)
            assert acq.max() >= 1e-6 and np.abs(dacq).max(0).min() >= 1e-4, (d, key)
