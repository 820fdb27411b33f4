"""The input dimension d = 1 ... 32 through every kernel that takes it as a template argument (predict.hip: cross_kernel<D, KID, STORE>,
grad_kernel<D>, cross_small_kernel<D, KID>; fit.hip: build_train_lds_kernel<D, KID>, kalpha_dd_kernel<D, KID>, hypgrad_kernel<D, KID>;
kg.hip: cov_grad_kernel<D>) and through the paths that fork on the runtime d (acq_mc_grad_kernel's lane < d, the [d][128] staging of
post_cov_f64_kernel, fused against replicated inference and fused against streamed HMC at d = 16 | 17, HS_MAXP at d = 32), each against
the oracle (oracle.cpu_ref) on the problem of tests/dims_problem.py: one kernel family per output, ARD lengthscales distinct per
coordinate.  tests/test_input_dims_cpu.py shows on the oracle alone that every coordinate moves these comparisons beyond their gates.

Every tolerance is the project's own, taken from the test named next to it.  Every figure -- the largest error per check and
per d -- is printed before its assertion: run with -s to keep them as the record later kernel work compares with.
Run on the MI355X box: python -m pytest tests/test_gpu_input_dims.py -m gpu"""
import os
import sys

import numpy as np
import pytest
from scipy.linalg import lapack

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dims_problem as P  # noqa: E402
import kg_ref as K  # noqa: E402

from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = P.KINDS
M = len(KINDS)
BOUNDARY = [1, 8, 9, 16, 17, 32]                        # both sides of cross_kernel's D <= 8 loop and of the d <= 16 fused paths, and the ends
SMALL = (200, 518, 1e-4)                                # N, C, noise of the every-dimension model


@pytest.fixture(scope="module")
def B():
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


def _close(d, what, got, want, rtol, atol):
    """np.testing.assert_allclose, the largest error and the largest error / allowance printed first."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    err = np.abs(got - want)
    print("d %2d %-34s max |delta| %.3g, of its allowance %.3g" % (d, what, err.max(), np.max(err / (atol + rtol * np.abs(want)))))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg="d = %d: %s" % (d, what))


def _var_close(d, what, got, want, gate):
    err = np.abs(got - want).max()
    print("d %2d %-34s max |delta| %.3g (gate %.3g)" % (d, what, err, gate))
    assert err <= gate, "d = %d: %s: %g > %g" % (d, what, err, gate)


def _check_train_kernel(d, model, p):
    """test_mixed_kernel_families_fixed_hyps: rtol 1e-12, atol 1e-14."""
    for j in range(M):
        _close(d, "train kernel, %s" % KINDS[j], model.get_train_kernel(j), R.kern_K(KINDS[j], p["X"], None, p["variances"][j], p["lengthscales"][j]),
               1e-12, 1e-14)


def _check_fit_and_predict(d, model, p, ref):
    """test_random_shapes.  Returns the device's (mean, variance) of all candidates."""
    Xc = p["Xc"]
    _close(d, "log-marginal", model.log_marginal, [o.log_marginal for o in ref.output], 1e-9, 1e-9)
    mean, var = model.predict(Xc)
    rm, rv = ref.predict(Xc)
    assert mean.shape == var.shape == (M, Xc.shape[0])
    _close(d, "mean, %d candidates" % len(Xc), mean, rm, P.MEAN_RTOL, P.MEAN_ATOL)
    _var_close(d, "variance, %d candidates" % len(Xc), var, rv, P.VAR_GATE * max(p["variances"]))
    _close(d, "noiseless variance", model.posterior_variance_noiseless(Xc), ref.posterior_variance_noiseless(Xc), 1e-5, 1e-8)
    _close(d, "mean at evaluated points", model.posterior_mean_at_evaluated_points(), ref.posterior_mean_at_evaluated_points(), 1e-6, 1e-7)
    return mean, var, rm, rv


def _check_hyper_gradients(d, model, ref):
    """test_mixed_kernel_families_fixed_hyps, every lengthscale component on its own."""
    dv, dl, dn = model.log_likelihood_gradients()
    assert dl.shape == (M, d)
    for j, o in enumerate(ref.output):
        rdv, rdl, rdn = o.lml_gradients()
        _close(d, "d lml / d variance, %s" % KINDS[j], dv[j], rdv, 1e-6, 1e-7)
        print("d %2d %-34s max |delta| %.3g" % (d, "d lml / d lengthscale, %s" % KINDS[j], np.abs(dl[j] - rdl).max()))
        for q in range(d):
            np.testing.assert_allclose(dl[j, q], rdl[q], rtol=1e-6, atol=1e-6, err_msg="d = %d: d lml / d l_%d, %s" % (d, q, KINDS[j]))
        _close(d, "d lml / d noise, %s" % KINDS[j], dn[j], rdn, 1e-6, 1e-5 * max(1.0, abs(float(rdn))))


def _check_per_coordinate(d, what, got, want, rtol, atol):
    assert got.shape == want.shape and got.shape[-1] == d
    print("d %2d %-34s max |delta| %.3g (largest |value| %.3g)" % (d, what, np.abs(got - want).max(), np.abs(want).max()))
    for q in range(d):
        np.testing.assert_allclose(got[..., q], want[..., q], rtol=rtol, atol=atol, err_msg="d = %d: %s, coordinate %d" % (d, what, q))


@pytest.mark.parametrize("d", list(range(1, 33)))
def test_fixed_hyps_every_dimension(B, d):
    """N = 200 (row block 0 full, row block 1 ragged), C = 518 (column workgroup 0 full: the full-tile loop; workgroup 1 ragged: the guarded
    loop), one mixed-family model per d."""
    p, ref = P.oracle(d, *SMALL)
    Xc = p["Xc"]
    model = P.mixed_model(B, p)
    assert np.all(model.jitter == 0.0)
    _check_train_kernel(d, model, p)
    mean, var, rm, rv = _check_fit_and_predict(d, model, p, ref)
    _check_hyper_gradients(d, model, ref)

    # the small path (<= 16 candidates: cross_small_kernel) against the oracle, and its means against the tile path's, bit for bit (the
    # invariant predict.hip states at cross_small_kernel)
    for n in (16, 5):
        mean_s, var_s = model.predict(Xc[:n])
        _close(d, "small path mean, %d candidates" % n, mean_s, rm[:, :n], P.MEAN_RTOL, P.MEAN_ATOL)
        _var_close(d, "small path variance, %d candidates" % n, var_s, rv[:, :n], P.VAR_GATE * max(p["variances"]))
        print("d %2d %-34s %d of %d means differ from the %d-candidate call" % (d, "small path, %d candidates" % n, np.sum(mean_s != mean[:, :n]),
                                                                                  mean_s.size, len(Xc)))
        np.testing.assert_array_equal(mean_s, mean[:, :n])

    # input gradients, per coordinate (test_random_shapes): 40 candidates take the tile path, 7 the small path
    for n in (40, 7):
        dm, dv = model.posterior_mean_gradient(Xc[:n]), model.posterior_variance_gradient(Xc[:n])
        _check_per_coordinate(d, "d mean / dx, %d candidates" % n, dm, ref.posterior_mean_gradient(Xc[:n]), 1e-5, 1e-6)
        _check_per_coordinate(d, "d variance / dx, %d candidates" % n, dv, ref.posterior_variance_gradient(Xc[:n]), 1e-4, 1e-7)

    # acquisition gradients (test_gradients_finite_differences): closed form, and Monte-Carlo -- lane q < d of acq_mc_grad_kernel owns
    # coordinate q.  The supports are dims_problem.acquisition_inputs': the oracle's gradient is non-zero in every coordinate.
    acq_in = P.acquisition_inputs(d, *SMALL)
    X7 = Xc[:P.N_ACQ]
    theta, ra, rda = acq_in["ma"]
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=P.ACQ_PROB), linear=True)
    a, da = B.maEI(model, None, utility=U)._compute_acq_withGradients(X7)
    _close(d, "maEI", a, ra, 1e-5, 1e-10)
    _check_per_coordinate(d, "d maEI / dx", da, rda, 1e-4, 1e-8)
    theta, ra, rda = acq_in["mc"]
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=P.ACQ_PROB), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq.W_samples = p["W"]
    a, da = acq._compute_acq_withGradients(X7)
    _close(d, "uEI_noiseless, neg_sq_dist", a, ra, 1e-5, 1e-10)
    _check_per_coordinate(d, "d uEI_noiseless / dx", da, rda, 1e-4, 1e-8)

    # the fp32 store variant of cross_kernel (test_predict_f32: |dvar| <= 2e-5 against fp64, means in fp64 whatever the option says)
    model.set_option("predict_f32", 1)
    try:
        mean32, var32 = model.predict(Xc)
    finally:
        model.set_option("predict_f32", 0)
    print("d %2d %-34s max |delta| %.3g against fp64 (gate 2e-05)" % (d, "fp32 variance contraction", np.abs(var32 - var).max()))
    assert np.abs(var32 - var).max() <= 2e-5 and var32.min() >= 1e-10
    np.testing.assert_array_equal(mean32, mean)


@pytest.mark.parametrize("d", BOUNDARY)
def test_large_model_paths_by_dimension(B, d):
    """N = 1100 (Np = 1152: build_train_lds_kernel has interior tiles, hypgrad_kernel its 64-row blocks, cross_kernel eight full row blocks
    and a ragged one), C = 1030 (two full column workgroups and a ragged one), noise 1e-3 (test_hyper_gradients_multi_tile)."""
    p = P.problem(d, 1100, 1030, 1e-3)
    ref = P.fit_oracle(p)
    model = P.mixed_model(B, p)
    assert np.all(model.jitter == 0.0)
    _check_train_kernel(d, model, p)
    _close(d, "log-marginal", model.log_marginal, [o.log_marginal for o in ref.output], 1e-8, 0.0)                 # test_odd_block_counts
    dv, dl, dn = model.log_likelihood_gradients()                                                                  # test_hyper_gradients_multi_tile
    for j, o in enumerate(ref.output):
        rdv, rdl, rdn = o.lml_gradients()
        _close(d, "d lml / d variance, %s" % KINDS[j], dv[j], rdv, 1e-6, 0.0)
        _check_per_coordinate(d, "d lml / d lengthscale, %s" % KINDS[j], dl[j], rdl, 1e-6, 1e-7)
        _close(d, "d lml / d noise, %s" % KINDS[j], dn[j], rdn, 1e-6, 0.0)
    mean, var = model.predict(p["Xc"])
    for sl, name in ((slice(0, 256), "[:256]"), (slice(1024, None), "[1024:]")):                                  # test_odd_block_counts
        rm, rv = ref.predict(p["Xc"][sl])
        _close(d, "mean, candidates %s" % name, mean[:, sl], rm, 1e-5, 1e-5)
        _var_close(d, "variance, candidates %s" % name, var[:, sl], rv, 1e-8)


@pytest.mark.parametrize("d", BOUNDARY)
def test_covariances_by_dimension(B, d):
    """posterior_covariance_between_points (n1 = 130, n2 = 70: ragged 128-tiles, [d][128] staging) against the oracle's k(X1, X2) -
    k(X1, X) Ky^-1 k(X, X2), and the covariance gradient (cov_grad_kernel<D>: 5 candidates, 9 reference points) against the restatement of
    tests/kg_ref.py; the gates of test_gpu_kg.py: |delta| <= 1e-8 sigma_f^2 + 1e-10, gradients rtol 1e-6, atol 1e-9 x their scale."""
    p, ref = P.oracle(d, *SMALL)
    model = P.mixed_model(B, p)
    Xc = p["Xc"]
    X1, X2, Xg, A = Xc[:130], Xc[130:200], Xc[200:205], Xc[205:214]
    want = np.empty((M, 130, 70))
    for j, f in enumerate(ref.output):
        V1 = lapack.dtrtrs(np.asfortranarray(f.L), R.kern_K(f.kind, f.X, X1, f.variance, f.lengthscale), lower=1)[0]
        V2 = lapack.dtrtrs(np.asfortranarray(f.L), R.kern_K(f.kind, f.X, X2, f.variance, f.lengthscale), lower=1)[0]
        want[j] = R.kern_K(f.kind, X1, X2, f.variance, f.lengthscale) - V1.T.dot(V2)
    got = model.posterior_covariance_between_points(X1, X2)
    assert got.shape == want.shape
    gate = 1e-8 * max(p["variances"]) + 1e-10
    assert np.abs(want).max() > 1e3 * gate              # (covariances the gate means something for: 6.5e-5 at d = 1, 0.06 ... 0.1 beyond)
    _close(d, "covariance, 130 x 70 points", got, want, 0.0, gate)
    la = K.LookAhead(ref.output)
    want_g = la.cov_grad(Xg, A)                         # (m, 5, 9, d)
    scale = np.abs(want_g).max()
    assert np.all(np.abs(want_g).max(axis=(0, 1, 2)) > 1e-6 * scale)          # (every coordinate carries a gradient)
    got_g = model._cov_to_ref(Xg, A, grad=True)[1]
    _check_per_coordinate(d, "covariance gradient, 5 x 9 points", got_g, want_g, 1e-6, 1e-9 * scale)
    for a in range(len(A)):                             # the drop-in method takes one reference point at a time
        np.testing.assert_allclose(model.posterior_covariance_gradient(Xg, A[a:a + 1]), want_g[:, :, a, :], rtol=1e-6, atol=1e-9 * scale,
                                   err_msg="d = %d: posterior_covariance_gradient, reference point %d" % (d, a))


@pytest.mark.parametrize("d", [15, 16, 17, 32])
def test_inference_boundary_dimensions(B, d):
    """_infer through the fused launch (d <= 16) and the replicated path (d >= 17, or option fused_infer = 0) against the oracle: the
    log-marginal and all 2 + d gradients, with the tolerances of test_fused_inference_equals_two_call_path.  From d = 17 on the fused
    launch must not be taken: the option makes no difference at all."""
    N, kinds = 100, ["matern52", "rbf"]
    p = P.problem(d, N, 8, 1e-4)
    X, Ys = p["X"], p["Y"][:2]
    cls = {"rbf": B.kern.RBF, "matern52": B.kern.Matern52}
    kern = [cls[k](d, variance=0.7 + 0.3 * j, lengthscale=p["lengthscales"][j], ARD=True) for j, k in enumerate(kinds)]
    model = B.multi_outputGP(2, kernel=kern, noise_var=[None] * 2, fixed_hyps=False, n_samples=2)
    model._X, model._Y = X, Ys
    model._create_sampler_state()
    params = [o.expanded(d) for o in model._sampler_outputs]
    fused = model._infer(params)
    model.set_option("fused_infer", 0)
    try:
        plain = model._infer(params)
    finally:
        model.set_option("fused_infer", 1)
    for name, res in (("fused_infer 1", fused), ("fused_infer 0", plain)):
        for j, (v, ls, nz) in enumerate(params):
            fit = R.GPFit(kinds[j], X, Ys[j], v, ls, nz)
            dv, dl, dn = fit.lml_gradients()
            _close(d, "%s: log-marginal, %s" % (name, kinds[j]), res[0][j], fit.log_marginal, 1e-9, 0.0)
            _close(d, "%s: d / d variance" % name, res[1][j], dv, 1e-6, 1e-8)
            _check_per_coordinate(d, "%s: d / d lengthscale" % name, res[2][j], dl, 1e-6, 1e-7 * max(1.0, np.abs(dl).max()))
            _close(d, "%s: d / d noise" % name, res[3][j], dn, 1e-6, 1e-6)
    if d > 16:
        for a, b in zip(fused, plain):
            np.testing.assert_array_equal(a, b)
    else:
        assert any(np.any(a != b) for a, b in zip(fused, plain))           # (two different kernels did the work)
        np.testing.assert_allclose(fused[0], plain[0], rtol=1e-12)
        for a, b in zip(fused[1:], plain[1:]):
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max())


@pytest.mark.parametrize("d", [16, 17, 32])
def test_hmc_by_dimension(B, d):
    """The device chain (fused at d = 16, streamed at d = 17 and 32; ARD and free noise: 2 + d parameters, all of HS_MAXP at d = 32) equals
    the lockstep host loop: chains, final parameters, accept and diverged flags, with the tolerances of test_streamed_hmc_equals_lockstep.
    Step size 0.02: on the lockstep path every one of the 4 draws of both outputs is accepted (checked there alone)."""
    from bocf_amd import hyper as H
    N, m, ns, iters, step = 100, 2, 4, 4, 0.02
    p = P.problem(d, N, 8, 1e-4)
    X, Ys = p["X"], p["Y"][:m]
    res = []
    for path in ("lockstep", "device"):
        model = B.multi_outputGP(m, fixed_hyps=False, n_samples=2, ARD=[True] * m, exact_feval=[False] * m)
        model._X, model._Y = X, Ys
        model._create_sampler_state()
        outs = model._sampler_outputs
        assert all(o.param_array.size == 2 + d and not o.fixed.any() for o in outs)
        draws = H.LockstepSampler.draw(outs, ns, rng=np.random.RandomState(19))
        sampler = H.LockstepSampler(outs, model._infer, d, device_hmc=model._device_hmc if path == "device" else None)
        chains = sampler.hmc([dr[1] for dr in draws], [dr[2] for dr in draws], hmc_iters=iters, stepsize=step)
        res.append((chains, sampler.accepted.copy(), [o.param_array.copy() for o in outs], sampler.diverged.copy(), sampler.device_hmc))
    assert res[0][1].sum() > 0                              # the lockstep chain moved
    assert res[1][4] is not None                            # (the device chain served the model: no silent host loop)
    for j in range(m):
        assert res[1][0][j].shape == (ns, 2 + d)
        print("d %2d HMC output %d: chains max |delta| %.3g, final parameters max |delta| %.3g, accepted %d of %d"
              % (d, j, np.abs(res[1][0][j] - res[0][0][j]).max(), np.abs(res[1][2][j] - res[0][2][j]).max(), res[0][1][j], ns))
        np.testing.assert_allclose(res[1][0][j], res[0][0][j], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(res[1][2][j], res[0][2][j], rtol=1e-7, atol=1e-10)
    np.testing.assert_array_equal(res[1][1], res[0][1])
    np.testing.assert_array_equal(res[1][3], res[0][3])


def test_dimension_33_is_refused(B):
    """Every switch (d) in the launchers ends in default: break -- a dimension beyond 32 must never get that far.  The library refuses it
    in the fixed-hyper fit and in the inference, with its own message; the process then serves d = 32 as if nothing had happened."""
    p = R.synthetic_problem(40, 33, 2, 8, 4, 33, 1e-4)
    kern = [B.kern.RBF(33, variance=1.0, lengthscale=p["lengthscales"][j], ARD=True) for j in range(2)]
    model = B.multi_outputGP(2, kernel=kern, noise_var=list(p["noise"]), fixed_hyps=True)
    with pytest.raises(B._ffi.BocfHipError, match="bocf_fit.*N, d or m out of range"):
        model.updateModel(p["X"], p["Y"])
    with pytest.raises(RuntimeError):
        model.predict(p["Xc"])
    learner = B.multi_outputGP(2, kernel=kern, noise_var=[None] * 2, fixed_hyps=False, n_samples=2)
    learner._X, learner._Y = p["X"], p["Y"]
    learner._create_sampler_state()
    with pytest.raises(B._ffi.BocfHipError, match="bocf_infer.*N, d or m out of range"):
        learner._infer([o.expanded(33) for o in learner._sampler_outputs])
    d = 32
    p, ref = P.oracle(d, *SMALL)
    model = P.mixed_model(B, p)
    _check_train_kernel(d, model, p)
    _check_fit_and_predict(d, model, p, ref)
