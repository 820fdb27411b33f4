"""Leave-one-out cross-validation on the device (bocf_loo, bocf_loo_utility, multi_outputGP.loo* / select_kernels) against the NumPy
restatement tests/loo_ref.py -- never against another device path alone.

Gates.  Per case and output the floor e_ref is the distance of loo_ref.loo_formula on the oracle's fp64 factor
from the long-double brute force (N explicit factorizations): made from references only.  The device must be within 100 e_ref of the
long-double truth, never asked for better than 1e-13 -- absolute in the mean of O(1) targets, relative to the with-noise variance,
relative to 1 + |lpd|.  The factor 100 covers the explicit inverse (about 4 x dtrtrs) and the reduction order.
The expected utilities are checked against the restatement evaluated on the device's own (gated) leave-one-out moments, to
64 eps (S + 8 m) times the largest |U| met: a handful of roundings per term and an S-term sum.
Worst figures measured on an MI355X: DESIGN.md section 20."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_ref as LR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

pytestmark = pytest.mark.gpu

KERN = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
KID = {"rbf": _ffi.KERN_RBF, "se": _ffi.KERN_SE, "matern52": _ffi.KERN_MATERN52, "matern32": _ffi.KERN_MATERN32}
UTIL = {"linear": _ffi.UTIL_LINEAR, "neg_sq_dist": _ffi.UTIL_NEG_SQ_DIST, "neg_sum_exp": _ffi.UTIL_NEG_SUM_EXP,
        "neg_exp_cos": _ffi.UTIL_NEG_EXP_COS, "rosenbrock": _ffi.UTIL_ROSENBROCK}
MIX3 = ("se", "matern52", "matern32")                     # a different family per output
BOTH, NOISELESS = _ffi.ADD_NOISE | _ffi.CLIP, _ffi.CLIP

#         N   d  kinds                 (wave start 64, tile 128, padding: N = 1, 2, 63 .. 65, 127 .. 129, 257)
CASES = [(1, 1, ("se",)), (2, 3, MIX3), (63, 1, MIX3), (64, 3, ("rbf",)), (65, 3, MIX3), (127, 1, ("matern52",)), (128, 3, MIX3),
         (129, 1, MIX3), (257, 3, ("matern32",))]
IDS = ["N%d-d%d-m%d" % (N, d, len(k)) for N, d, k in CASES]
SEED = 77


def _model(kinds, X, Y, var, ls, noise):
    d = X.shape[1]
    model = B.multi_outputGP(len(kinds), kernel=[KERN[k](d, variance=var[j], lengthscale=ls[j], ARD=True) for j, k in enumerate(kinds)],
                             noise_var=list(noise), fixed_hyps=True)
    model.updateModel(X, [y[:, None] for y in Y])
    return model


def _ref_model(ref, kinds, upto=None):
    n = slice(None, upto)
    return _model(kinds, ref["X"][n], ref["Y"][:, n], ref["var"], ref["ls"], ref["noise"])


def _device(model, flags):
    """(mean, var, lpd, lpd_sum) of all resident factorizations straight from bocf_loo."""
    model._ensure_fitted()
    M, N = model.output_dim * model._H, model._X.shape[0]
    mean, var, lpd, tot = np.empty((M, N)), np.empty((M, N)), np.empty((M, N)), np.empty(M)
    _ffi.check(_ffi.load().bocf_loo(model._context().handle, flags, _ffi.dptr(mean), _ffi.dptr(var), _ffi.dptr(lpd), _ffi.dptr(tot)), "bocf_loo")
    return mean, var, lpd, tot


def _gate(label, model, ref, rows=None):
    """Both flag combinations of bocf_loo against the truth of `ref`, output by output (rows: the device rows of ref's outputs)."""
    with_noise, without = _device(model, BOTH), _device(model, NOISELESS)
    np.testing.assert_array_equal(with_noise[0], without[0])
    np.testing.assert_array_equal(with_noise[2], without[2])           # the density is that of the noisy prediction whatever the flags
    for j, truth in enumerate(ref["truth"]):
        r = j if rows is None else rows[j]
        floor = ref["floor"][j]
        want0 = np.maximum(truth[2], np.longdouble(1e-10))             # BOCF_CLIP (the with-noise variance is far above it)
        dev = (with_noise[0][r], with_noise[1][r], without[1][r], with_noise[2][r])
        dist = LR.distances(dev, (truth[0], truth[1], want0, truth[3]), ref["noise"][j])
        dist0 = LR.distances(dev, (truth[0], truth[1], want0, truth[3]), ref["noise"][j], with_noise=False)[1]
        print("%s output %d: floor (mean, var, lpd) %s, device %s, noiseless var %.1e" % (label, j, ["%.1e" % v for v in floor],
                                                                                        ["%.1e" % v for v in dist], dist0))
        for k in range(3):
            assert dist[k] <= LR.gate(floor[k]), (label, j, k, dist[k], floor[k])
        assert dist0 <= LR.gate(floor[1]), (label, j, dist0, floor[1])
        # the sums: N terms in a fixed order, each within its gate
        tot = float(np.sum(truth[3]))
        assert abs(with_noise[3][r] - tot) <= LR.gate(floor[2]) * float(np.sum(1 + np.abs(truth[3]))), (label, j)
        np.testing.assert_array_equal(with_noise[3][r], without[3][r])


# ---- bocf_loo against the long-double brute force ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,kinds", CASES, ids=IDS)
def test_loo_against_the_long_double_brute_force(N, d, kinds):
    ref = LR.reference(N, d, kinds, SEED)
    model = _ref_model(ref, kinds)
    assert np.all(model.jitter == 0)
    _gate("N %d d %d" % (N, d), model, ref)


def test_two_hyper_sample_groups_with_different_lengthscales():
    N, d, kinds, H = 65, 3, MIX3, 2
    refs = [LR.reference(N, d, kinds, SEED), LR.reference(N, d, kinds, SEED, 0.25)]
    m = len(kinds)
    model = B.multi_outputGP(m, fixed_hyps=False, n_samples=H)
    model._X, model._Y = np.ascontiguousarray(refs[0]["X"]), [y[:, None].copy() for y in refs[0]["Y"]]
    model._kernel_ids = [KID[k] for k in kinds]
    model._instances = [[(refs[h]["var"][j], refs[h]["ls"][j], refs[h]["noise"][j]) for j in range(m)] for h in range(H)]
    model._fit()
    for h in range(H):
        _gate("group %d" % h, model, refs[h], rows=[h * m + j for j in range(m)])
    # the model class: the current hyper-sample answers, or all of them
    mean, var, lpd = model.loo(all_hyper_samples=True)
    assert mean.shape == var.shape == lpd.shape == (H, m, N)
    model.set_hyperparameters(1)
    for a, b in zip(model.loo(), (mean[1], var[1], lpd[1])):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(model.loo_log_likelihood(all_hyper_samples=True)[1], model.loo_log_likelihood())
    assert np.all(np.abs(model.loo_log_likelihood() - lpd[1].sum(1)) <= 1e-13 * np.abs(lpd[1]).sum(1))       # N terms, a fixed order
    assert not np.array_equal(mean[0], mean[1])


@pytest.mark.parametrize("N,d,kinds", [(128, 3, MIX3), (130, 1, ("matern52",))], ids=["127to128", "129to130"])
def test_loo_after_an_append(N, d, kinds):
    ref = LR.reference(N, d, kinds, SEED)
    model = _ref_model(ref, kinds, upto=N - 1)
    lib = _ffi.load()
    lml = np.zeros(len(kinds))
    rc = lib.bocf_append(model._context().handle, _ffi.dptr(_ffi.f64(ref["X"][-1])), _ffi.dptr(_ffi.f64(ref["Y"])), _ffi.dptr(lml))
    assert rc == 0, "the append was refused: this case must run on the bordered factor"
    model._X, model._Y = np.ascontiguousarray(ref["X"]), [y[:, None].copy() for y in ref["Y"]]
    _gate("append to %d" % N, model, ref)


def test_loo_after_new_targets():
    N, d, kinds = 65, 3, MIX3
    ref = LR.reference(N, d, kinds, SEED)
    model = _model(kinds, ref["X"], np.cos(ref["Y"]) + 1.0, ref["var"], ref["ls"], ref["noise"])
    before = _device(model, BOTH)
    lml = np.zeros(len(kinds))
    _ffi.check(_ffi.load().bocf_update_targets(model._context().handle, _ffi.dptr(_ffi.f64(ref["Y"])), _ffi.dptr(lml)), "bocf_update_targets")
    model._Y = [y[:, None].copy() for y in ref["Y"]]
    _gate("new targets", model, ref)
    np.testing.assert_array_equal(before[1], _device(model, BOTH)[1])  # same R: the variances do not depend on the targets


def test_loo_of_a_jittered_fit(probes):
    """The diagonal-shift hook of the probes build takes 2e-8 off diag(Ky): the noise-free SE output loses definiteness and takes the first
    jitter rung.  The model is then Ky = K + (1e-8 + jitter - 2e-8) I, and its leave-one-out results must be that model's."""
    N, d, kinds, hook = 65, 1, ("se",), 2e-8
    X, Y, var, ls, nz = LR.problem(N, d, kinds, SEED, 0.6, 0.0)
    model = B.multi_outputGP(1, kernel=[B.kern.SE(d, variance=var[0], lengthscale=ls[0], ARD=True)], noise_var=[0.0], fixed_hyps=True)
    model.set_option("test_diag_shift_1e12", int(round(hook * 1e12)))
    model.updateModel(X, [y[:, None] for y in Y])
    assert model.jitter[0] > 0
    ref = LR.reference(N, d, kinds, SEED, 0.6, 0.0, float(model.jitter[0]) - hook)
    _gate("jitter %.1e" % model.jitter[0], model, ref)


def test_loo_of_an_output_sharded_fit(probes):
    N, d, kinds = 65, 3, MIX3
    ref = LR.reference(N, d, kinds, SEED)
    model = B.multi_outputGP(len(kinds), kernel=[KERN[k](d, variance=ref["var"][j], lengthscale=ref["ls"][j], ARD=True) for j, k in enumerate(kinds)],
                             noise_var=list(ref["noise"]), fixed_hyps=True)
    model.set_option("shard_fit_simulate", 2)
    model.set_option("shard_fit", 1)
    model.updateModel(ref["X"], [y[:, None] for y in ref["Y"]])
    _gate("sharded", model, ref)


def test_two_calls_are_bit_identical_and_null_outputs_are_allowed():
    ref = LR.reference(129, 1, MIX3, SEED)
    model = _ref_model(ref, MIX3)
    a, b = _device(model, BOTH), _device(model, BOTH)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    lib, h = _ffi.load(), model._context().handle
    assert lib.bocf_loo(h, BOTH, None, None, None, None) == 0
    only = np.empty_like(a[1])
    assert lib.bocf_loo(h, BOTH, None, _ffi.dptr(only), None, None) == 0
    np.testing.assert_array_equal(only, a[1])
    # unclipped, and the clip itself: a variance below 1e-10 cannot be provoked at these noises, so clip against the raw call
    raw = _device(model, 0)
    np.testing.assert_array_equal(np.maximum(raw[1], 1e-10), _device(model, NOISELESS)[1])
    np.testing.assert_allclose(_device(model, _ffi.ADD_NOISE)[1] - raw[1], np.repeat(ref["noise"][:, None], 129, 1), rtol=1e-9)


def test_surrounding_state_is_left_as_it_was():
    ref = LR.reference(65, 3, MIX3, SEED)
    model = _ref_model(ref, MIX3)
    rng = np.random.RandomState(9)
    Xc, W, theta = rng.uniform(size=(200, 3)), rng.normal(size=(16, 3)), rng.normal(size=(2, 3))
    acq = model.acq_mc(Xc, _ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, theta, None, W=W)
    top = model.select_topk(8)
    lib, h = _ffi.load(), model._context().handle
    mean, var = np.empty((3, 200)), np.empty((3, 200))
    _ffi.check(lib.bocf_predict(h, BOTH, _ffi.dptr(mean), _ffi.dptr(var)), "bocf_predict")
    # ... the leave-one-out calls in between
    _device(model, BOTH)
    model.set_eu_samples(rng.normal(size=(2, 10, 3)))
    out = np.empty((2, 65))
    _ffi.check(lib.bocf_loo_utility(h, 0, BOTH, _ffi.EU_MC, _ffi.UTIL_NEG_SQ_DIST, None, 0, _ffi.dptr(_ffi.f64(theta)), 3, 2, _ffi.dptr(out)), "bocf_loo_utility")
    # the acquisition vector, the candidates, the Monte-Carlo samples and the posterior are served as before
    again = model.select_topk(8)
    np.testing.assert_array_equal(top[0], again[0])
    np.testing.assert_array_equal(top[1], again[1])
    mean2, var2 = np.empty((3, 200)), np.empty((3, 200))
    _ffi.check(lib.bocf_predict(h, BOTH, _ffi.dptr(mean2), _ffi.dptr(var2)), "bocf_predict")
    np.testing.assert_array_equal(mean, mean2)
    np.testing.assert_array_equal(var, var2)
    np.testing.assert_array_equal(acq, model._acq_mc_resident(_ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, theta, None, 200))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_entry_point_and_leaves_the_context_usable():
    lib, dp = _ffi.load(), _ffi.dptr
    ref = LR.reference(65, 3, MIX3, SEED)
    N, m = 65, 3
    th3, th2, out = _ffi.f64(np.zeros((2, 3))), _ffi.f64(np.zeros((2, 2))), np.empty((33, N))

    def bad(rc, name, text):
        msg = lib.bocf_last_error().decode()
        assert rc < 0 and name in msg and text in msg, (rc, msg, text)

    def util(h, group=0, flags=BOTH, mode=_ffi.EU_CLOSED, kind=_ffi.UTIL_NEG_SQ_DIST, params=None, n_params=0, theta=th3, tdim=3, L=2, val=out):
        return lib.bocf_loo_utility(h, group, flags, mode, kind, dp(params), n_params, dp(theta), tdim, L, dp(val))
    # not fitted
    ctx = _ffi.Context(0)
    bad(lib.bocf_loo(ctx.handle, BOTH, None, None, None, None), "bocf_loo", "model not fitted")
    bad(util(ctx.handle), "bocf_loo_utility", "model not fitted")
    # a host-given posterior
    post = _ffi.f64(np.ones((m, 4)))
    _ffi.check(lib.bocf_set_posterior(ctx.handle, m, 4, 5, dp(post), dp(post), dp(_ffi.f64(np.ones((m, 5))))), "bocf_set_posterior")
    bad(lib.bocf_loo(ctx.handle, BOTH, None, None, None, None), "bocf_loo", "host-given posterior")
    bad(util(ctx.handle), "bocf_loo_utility", "host-given posterior")
    # a fused inference leaves no factor
    X, Y = _ffi.f64(ref["X"]), _ffi.f64(ref["Y"])
    var, ls, nz = _ffi.f64(ref["var"]), _ffi.f64(ref["ls"]), _ffi.f64(ref["noise"])
    jit, lml = np.zeros(m), np.zeros(m)
    dv, dl, dn = np.zeros(m), np.zeros((m, 3)), np.zeros(m)
    assert lib.bocf_infer(ctx.handle, dp(X), dp(Y), N, 3, m, _ffi.KERN_SE, dp(var), dp(ls), dp(nz), 5, dp(jit), dp(lml), dp(dv), dp(dl), dp(dn)) == 0
    bad(lib.bocf_loo(ctx.handle, BOTH, None, None, None, None), "bocf_loo", "model not fitted")
    bad(util(ctx.handle), "bocf_loo_utility", "model not fitted")
    # ... and the same context is usable afterwards
    assert lib.bocf_fit(ctx.handle, dp(X), dp(Y), N, 3, m, _ffi.KERN_SE, dp(var), dp(ls), dp(nz), 5, dp(jit), dp(lml)) == 0
    h = ctx.handle
    bad(lib.bocf_loo(h, 4, None, None, None, None), "bocf_loo", "unknown flags")
    bad(util(h, flags=8), "bocf_loo_utility", "unknown flags")
    bad(util(h, group=-1), "bocf_loo_utility", "group out of range")
    bad(util(h, group=1), "bocf_loo_utility", "group out of range")
    bad(util(h, mode=3), "bocf_loo_utility", "unknown mode")
    bad(util(h, kind=6), "bocf_loo_utility", "unknown utility kind")
    bad(util(h, kind=-1), "bocf_loo_utility", "unknown utility kind")
    bad(util(h, theta=th2, tdim=2), "bocf_loo_utility", "theta_dim must equal m")
    bad(util(h, theta=None), "bocf_loo_utility", "theta must be")
    bad(util(h, L=0), "bocf_loo_utility", "L out of range")
    bad(util(h, L=33), "bocf_loo_utility", "L out of range")
    bad(util(h, kind=_ffi.UTIL_LINEAR), "bocf_loo_utility", "no closed-form expectation")
    bad(util(h, kind=_ffi.UTIL_ROSENBROCK), "bocf_loo_utility", "rosenbrock utility needs even m")
    bad(util(h, n_params=2), "bocf_loo_utility", "bad utility parameters")
    bad(util(h, mode=_ffi.EU_MC, kind=_ffi.UTIL_NEG_EXP_COS), "bocf_loo_utility", "neg_exp_cos needs m weights")
    bad(util(h, mode=_ffi.EU_CLOSED, kind=_ffi.UTIL_PROGRAM), "bocf_loo_utility", "no closed-form expectation")
    bad(util(h, mode=_ffi.EU_MC, kind=_ffi.UTIL_PROGRAM), "bocf_loo_utility", "no utility program is resident")
    bad(util(h, mode=_ffi.EU_MC), "bocf_loo_utility", "no Monte-Carlo samples set")
    Z = _ffi.f64(np.zeros((1, 5, m)))
    _ffi.check(lib.bocf_set_eu_samples(h, dp(Z), 1, 5), "bocf_set_eu_samples")
    bad(util(h, mode=_ffi.EU_MC), "bocf_loo_utility", "fewer Monte-Carlo sample blocks")
    bad(util(h, val=None), "bocf_loo_utility", "null val_out")
    assert util(h) == 0 and lib.bocf_loo(h, BOTH, None, None, None, None) == 0
    ctx.close()


# ---- bocf_loo_utility against the restatement ---------------------------------------------------------------------------------------
def _eu_tol(scale, S, m):
    return 64.0 * np.finfo(float).eps * (S + 8 * m) * scale


def _mc_scale(func, thetas, mean, var, Z):
    """The largest |U(theta_l, mean + sd o z)| over parameters, samples and points."""
    sd = np.sqrt(var)
    return max(np.abs(func(th, mean + sd * z[:, None])).max() for l, th in enumerate(thetas) for z in Z[l])


def _utility_case():
    ref = LR.reference(65, 3, MIX3, SEED)
    model = _ref_model(ref, MIX3)
    rng = np.random.RandomState(31)
    return ref, model, rng.normal(size=(2, 3)), rng.normal(size=(2, 65, 3))   # L = 2 parameters, S = 65 normals each


def _loo_utility(model, flags, mode, kind, thetas, params=None):
    thetas, params = _ffi.f64(thetas), None if params is None else _ffi.f64(params)
    out = np.empty((thetas.shape[0], model._X.shape[0]))
    _ffi.check(_ffi.load().bocf_loo_utility(model._context().handle, model._current_h, flags, mode, kind, _ffi.dptr(params),
                                            0 if params is None else params.size, _ffi.dptr(thetas), thetas.shape[1], thetas.shape[0],
                                            _ffi.dptr(out)), "bocf_loo_utility")
    return out


@pytest.mark.parametrize("flags", [BOTH, NOISELESS], ids=["noise", "noiseless"])
def test_loo_utility_closed_mean_and_monte_carlo_against_the_restatement(flags):
    ref, model, thetas, Z = _utility_case()
    mean, var = _device(model, flags)[:2]
    m, S = 3, Z.shape[1]
    got = _loo_utility(model, flags, _ffi.EU_MEAN, _ffi.UTIL_LINEAR, thetas)
    want = LR.loo_expected_utility("mean", "linear", thetas, mean, var)
    assert np.abs(got - want).max() <= _eu_tol(np.abs(thetas).max() * np.abs(mean).max() * m, 1, m)
    for kind in ("neg_sq_dist", "neg_sum_exp"):
        got = _loo_utility(model, flags, _ffi.EU_CLOSED, UTIL[kind], thetas)
        want = LR.loo_expected_utility("closed", kind, thetas, mean, var)
        assert np.abs(got - want).max() <= _eu_tol(np.abs(want).max(), 1, m), kind
    model.set_eu_samples(Z)
    c = np.array([0.7, 1.1, 0.4])
    for kind, params in (("neg_sq_dist", None), ("neg_sum_exp", None), ("neg_exp_cos", c)):
        got = _loo_utility(model, flags, _ffi.EU_MC, UTIL[kind], thetas, params)
        want = LR.loo_expected_utility("mc", kind, thetas, mean, var, Z, params)
        scale = _mc_scale(lambda t, y: O.utility_eval(kind, t, y, params), thetas, mean, var, Z)
        print("loo utility mc %s: max |device - restatement| %.2e (scale %.2e)" % (kind, np.abs(got - want).max(), scale))
        assert np.abs(got - want).max() <= _eu_tol(scale, S, m), kind
    # the closed form is the limit of the Monte-Carlo mean: a coarse check that the two modes speak of the same quantity
    closed = _loo_utility(model, flags, _ffi.EU_CLOSED, _ffi.UTIL_NEG_SQ_DIST, thetas)
    mc = _loo_utility(model, flags, _ffi.EU_MC, _ffi.UTIL_NEG_SQ_DIST, thetas)
    assert np.abs(mc - closed).max() <= 1.0


def test_loo_utility_program_against_the_restatement_and_the_compiled_in_kind():
    ref, model, thetas, Z = _utility_case()

    def neg_sq_dist(t, y):
        return -np.sum(np.square((y.transpose() - t).transpose()), axis=0)
    U = B.Utility(func=neg_sq_dist, parameter_dist=B.ParameterDistribution(support=thetas, prob_dist=np.full(2, 0.5)), device="program")
    assert U.device_kind(3) == _ffi.UTIL_PROGRAM
    model.set_utility_program(U.program_blob)
    model.set_eu_samples(Z)
    mean, var = _device(model, BOTH)[:2]
    got = _loo_utility(model, BOTH, _ffi.EU_MC, _ffi.UTIL_PROGRAM, thetas)
    want = LR.loo_expected_utility("mc", None, thetas, mean, var, Z, func=neg_sq_dist)
    tol = _eu_tol(_mc_scale(neg_sq_dist, thetas, mean, var, Z), Z.shape[1], 3)
    assert np.abs(got - want).max() <= tol
    compiled = _loo_utility(model, BOTH, _ffi.EU_MC, _ffi.UTIL_NEG_SQ_DIST, thetas)
    assert np.abs(got - compiled).max() <= tol
    # the program takes no parameters, and must be the one for this m and theta_dim
    lib, h = _ffi.load(), model._context().handle
    one = _ffi.f64([1.0])
    assert lib.bocf_loo_utility(h, 0, BOTH, _ffi.EU_MC, _ffi.UTIL_PROGRAM, _ffi.dptr(one), 1, _ffi.dptr(_ffi.f64(thetas)), 3, 2, _ffi.dptr(got)) < 0
    assert b"bocf_loo_utility" in lib.bocf_last_error()
    assert lib.bocf_loo_utility(h, 0, BOTH, _ffi.EU_MC, _ffi.UTIL_PROGRAM, None, 0, _ffi.dptr(_ffi.f64(thetas[:, :2])), 2, 2, _ffi.dptr(got)) < 0
    assert b"bocf_loo_utility" in lib.bocf_last_error()


# ---- the model class, end to end ----------------------------------------------------------------------------------------------------
def test_loo_utility_and_select_kernels_end_to_end_on_matern32_data():
    X, Y, var, ls, noise = LR.matern_problem()
    d, m = X.shape[1], len(Y)
    lists = [[KERN[k](d, variance=var, lengthscale=ls, ARD=True) for _ in range(m)] for k in LR.FAMILIES]
    model = B.multi_outputGP(m, kernel=lists[0], noise_var=[noise] * m, fixed_hyps=True)
    model.updateModel(X, [y[:, None] for y in Y])
    resident = model.loo()
    loo, lml = model.loo_compare(lists)
    want_loo, want_lml = LR.oracle_tables(X, Y, var, ls, noise)
    np.testing.assert_allclose(loo, want_loo, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(lml, want_lml, rtol=1e-8, atol=1e-8)
    for criterion in ("loo", "lml"):
        picked = model.select_kernels(lists, criterion=criterion)
        assert [type(k).__name__ for k in picked] == ["Matern32"] * m
        assert picked[0] is lists[3][0] and picked[1] is lists[3][1]
    # the comparison ran on a context of its own: the resident model answers as before, bit for bit
    for a, b in zip(resident, model.loo()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(model.loo_log_likelihood(), want_loo[0], rtol=1e-8)
    # the summary of the chosen family, against the oracle formula
    best = B.multi_outputGP(m, kernel=picked, noise_var=[noise] * m, fixed_hyps=True)
    best.updateModel(X, [y[:, None] for y in Y])
    fits = [O.GPFit("matern32", X, y, var, ls, noise) for y in Y]
    f = [LR.loo_formula_fit(fit, y) for fit, y in zip(fits, Y)]
    s = best.loo_summary()
    want = B.multi_outputGP.loo_summary_of(Y, np.stack([a[0] for a in f]), np.stack([a[1] for a in f]), np.stack([a[3] for a in f]))
    for key in want:
        np.testing.assert_allclose(s[key], want[key], rtol=1e-8, atol=1e-10, err_msg=key)
    assert np.all(s["coverage"] >= 0.85) and np.all(np.abs(s["z_var"] - 1.0) < 0.6)          # data from the model's own prior: calibrated
    # the cross-validated composite prediction: closed form for neg_sq_dist, observed values from the host callable
    thetas = np.array([[0.2, -0.1], [1.0, 0.5], [-0.4, 0.3]])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=thetas, prob_dist=np.full(3, 1.0 / 3)), device="neg_sq_dist")
    predicted, observed = best.loo_utility(U)
    assert predicted.shape == observed.shape == (3, X.shape[0])
    mean, varn = np.stack([a[0] for a in f]), np.stack([a[1] for a in f])
    np.testing.assert_allclose(predicted, LR.loo_expected_utility("closed", "neg_sq_dist", thetas, mean, varn), rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(observed, np.stack([O.utility_eval("neg_sq_dist", th, Y) for th in thetas]), rtol=1e-13)
    p0, _ = best.loo_utility(U, noiseless=True)
    np.testing.assert_allclose(p0 - predicted, m * noise, rtol=1e-6)                         # -sum var: the noise of m outputs less
    # a Monte-Carlo utility draws its normals from np.random (or takes Z); a linear one takes the mean form
    V = B.Utility(parameter_dist=B.ParameterDistribution(support=np.zeros((1, 1)), prob_dist=np.ones(1)), device="neg_exp_cos", device_params=[0.5, 1.5])
    Z = np.random.RandomState(3).normal(size=(1, 30, m))
    pm, om = best.loo_utility(V, Z=Z)
    np.testing.assert_allclose(pm, LR.loo_expected_utility("mc", "neg_exp_cos", np.zeros((1, 1)), mean, varn, Z, np.array([0.5, 1.5])), rtol=1e-7, atol=1e-8)
    lin = B.Utility(func=lambda t, y: np.dot(t, y), parameter_dist=B.ParameterDistribution(support=thetas, prob_dist=np.full(3, 1.0 / 3)), linear=True)
    pl, ol = best.loo_utility(lin)
    np.testing.assert_allclose(pl, thetas.dot(mean), rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(ol, thetas.dot(Y), rtol=1e-13)
