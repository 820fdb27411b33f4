"""The number of outputs per hyper-sample m = 1 ... 16 through every kernel that takes it as a template argument (acq.hip:
acq_mc_m_kernel<M>, acq_mc_grad_kernel<MC>; eu.hip: eu_kernel<MC>; kg.hip: kg_kernel<MODE, TAB, M>; pending.hip: pending_acq_kernel<TAB, M>
and its gradient kernel; cacq.hip: the two constrained kernels -- M = 1 ... 8 and the run-time instantiation for 9 ... 16) and through the
kernels that loop to a run-time m over double y[BOCF_MAX_M] (acq_linear_kernel and its gradient twin, best_so_far_kernel, the selection
kernels of thompson.hip and paths.hip, the util_prog.hip interpreters), each against the oracle (oracle.cpu_ref) or the NumPy restatements
tests/kg_ref.py, pending_ref.py, constrained_ref.py, paths_ref.py on the problems of tests/outputs_problem.py: one kernel family per
output, utility parameters placed so that the compared values are not zeros.  tests/test_output_counts_cpu.py shows on the oracle alone
that every output moves every one of these comparisons beyond its gate.

Every tolerance is the project's own, taken from the test named in tests/outputs_problem.py; the one factor that is not copied (on the
path-utility gates, for the utilities the project's test does not gate) is derived there, from the reference alone.  Every figure -- the largest error per check
and per m, and its share of the allowance -- is printed before its assertion: run with -s to keep them as the record.
Run on the MI355X box: python -m pytest tests/test_gpu_output_counts.py -m gpu -s"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_ref as CR  # noqa: E402
import outputs_problem as P  # noqa: E402
import paths_ref as PTH  # noqa: E402
import pending_ref as PR  # noqa: E402

from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MS = P.MS
SENTINEL = -7.25


@pytest.fixture(scope="module")
def B():
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


def _util(B, kind):
    F = B._ffi
    return {"linear": F.UTIL_LINEAR, "neg_sq_dist": F.UTIL_NEG_SQ_DIST, "neg_sum_exp": F.UTIL_NEG_SUM_EXP, "neg_exp_cos": F.UTIL_NEG_EXP_COS,
            "rosenbrock": F.UTIL_ROSENBROCK}[kind]


def _kernels(B, p):
    cls = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
    return [cls[k](P.D, variance=p["var"][j], lengthscale=p["ls"][j], ARD=True) for j, k in enumerate(p["kinds"])]


def _fixed_model(B, p):
    model = B.multi_outputGP(len(p["kinds"]), kernel=_kernels(B, p), noise_var=list(p["nz"]), fixed_hyps=True)
    model.updateModel(p["X"], [y[:, None] for y in p["Y"]])
    return model


def _hyper_model(B, p, H):
    """_hyper_model of tests/test_gpu_kg.py: H hyper-samples resident on the device, sample h with the variances x (1 + 0.1 h) and the
    lengthscales x (1 - 0.05 h) (outputs_problem.hyper_lookaheads gives the references)."""
    F = B._ffi
    kid = {"rbf": F.KERN_RBF, "se": F.KERN_SE, "matern52": F.KERN_MATERN52, "matern32": F.KERN_MATERN32}
    m = len(p["kinds"])
    model = B.multi_outputGP(m, fixed_hyps=False, n_samples=H)
    model._X, model._Y = np.ascontiguousarray(p["X"]), [y[:, None].copy() for y in p["Y"]]
    model._kernel_ids = [kid[k] for k in p["kinds"]]
    model._instances = [[(p["var"][j] * (1 + 0.1 * h), p["ls"][j] * (1 - 0.05 * h), p["nz"][j]) for j in range(m)] for h in range(H)]
    model._fit()
    return model


def _close(m, what, got, want, rtol, atol):
    """np.testing.assert_allclose, the largest error and the largest error / allowance printed first."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (m, what, got.shape, want.shape)
    err = np.abs(got - want)
    print("m %2d %-44s max |delta| %.3g, of its allowance %.3g (largest |value| %.3g)"
          % (m, what, err.max(), np.max(err / (atol + rtol * np.abs(want))), np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg="m = %d: %s" % (m, what))


def _per_coordinate(m, what, got, want, rtol, atol):
    _close(m, what, got, want, rtol, atol)
    for q in range(want.shape[-1]):
        np.testing.assert_allclose(got[..., q], want[..., q], rtol=rtol, atol=atol, err_msg="m = %d: %s, coordinate %d" % (m, what, q))


# ---- fit and predict -----------------------------------------------------------------------------------------------------------------
def _check_fit_and_predict(m, model, p, ref, n_grad=(7, 40)):
    """test_random_shapes (through tests/dims_problem.py): log-marginal, mean, variance, mean at the evaluated points, input gradients."""
    Xc = p["Xc"]
    assert np.all(np.asarray(model.jitter) == 0.0)
    _close(m, "log-marginal", model.log_marginal, [o.log_marginal for o in ref.output], 1e-9, 1e-9)
    mean, var = model.predict(Xc)
    rm, rv = ref.predict(Xc)
    _close(m, "mean, %d candidates" % len(Xc), mean, rm, P.MEAN_RTOL, P.MEAN_ATOL)
    _close(m, "variance, %d candidates" % len(Xc), var, rv, 0.0, P.VAR_GATE * max(p["var"]))
    _close(m, "mean at evaluated points", model.posterior_mean_at_evaluated_points(), ref.posterior_mean_at_evaluated_points(), 1e-6, 1e-7)
    for n in n_grad:                                     # 40 candidates take the tile path, 7 the small path
        _per_coordinate(m, "d mean / dx, %d candidates" % n, model.posterior_mean_gradient(Xc[:n]), ref.posterior_mean_gradient(Xc[:n]), 1e-5, 1e-6)
        _per_coordinate(m, "d variance / dx, %d candidates" % n, model.posterior_variance_gradient(Xc[:n]), ref.posterior_variance_gradient(Xc[:n]),
                        1e-4, 1e-7)


@pytest.mark.parametrize("m", MS)
def test_fit_and_predict(B, m):
    p, _, ref = P.oracle(m)
    _check_fit_and_predict(m, _fixed_model(B, p), p, ref)


@pytest.mark.parametrize("m", [9, 16])
def test_fit_and_predict_three_panels(B, m):
    """N = 300: three 128-row panels, the team schedule with m outputs per launch."""
    p, _, ref = P.oracle(m, 300)
    _check_fit_and_predict(m, _fixed_model(B, p), p, ref)


# ---- closed-form acquisitions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_closed_form_acquisitions(B, m):
    """maEI and maPI, value and gradient (acq_linear_kernel, acq_linear_grad_kernel; best_so_far_kernel through them: the oracle's
    ma_marginal_best_so_far); gates of test_fixed_hyps_every_dimension."""
    F = B._ffi
    p, post = P.problem(m), P.posterior(m)
    model = _fixed_model(B, p)
    thetas, _ = P.support(m, "linear")
    for name, kind in (("EI", F.ACQ_EI), ("PI", F.ACQ_PI)):
        want = P.ma_values(post, thetas, P.PROB, name)
        print("m %2d ma%s: share of candidates above 1e3 x atol %.2f" % (m, name, P.share(want, P.ACQ_VALUE[1])))
        _close(m, "ma%s" % name, model.acq_linear(p["Xc"], kind, thetas, P.PROB), want, *P.ACQ_VALUE)
        a, da = model.acq_linear_grad(p["Xc"][:P.NGRAD], kind, thetas, P.PROB)
        wa, wda = P.ma_grad(post, thetas, P.PROB, name)
        _close(m, "ma%s, gradient entry" % name, a, wa, *P.ACQ_VALUE)
        _per_coordinate(m, "d ma%s / dx" % name, da, wda, *P.ACQ_GRAD)


# ---- Monte-Carlo acquisitions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_monte_carlo_acquisitions(B, m):
    """uEI_noiseless and uPI values (acq_mc_m_kernel<M>; gate of test_mc_acquisition_every_output_count) and acq_mc_grad value and gradient
    (acq_mc_grad_kernel<MC>; gates of test_fixed_hyps_every_dimension) with every device utility."""
    F = B._ffi
    p, post = P.problem(m), P.posterior(m)
    model = _fixed_model(B, p)
    Xc, W = p["Xc"], p["W"]
    for kind in P.utilities(m):
        thetas, params = P.support(m, kind)
        u = (_util(B, kind), params, thetas, P.PROB)
        for name, acq in (("EI", F.ACQ_EI), ("PI", F.ACQ_PI)):
            want = P.mc_values(post, W, kind, thetas, P.PROB, params, name)
            print("m %2d u%s %s: share of candidates above 1e3 x atol %.2f" % (m, name, kind, P.share(want, P.MC_VALUE[1])))
            _close(m, "u%s, %s" % (name, kind), model.acq_mc(Xc, acq, *u, W=W), want, *P.MC_VALUE)
        a, da = model.acq_mc_grad(Xc[:P.NGRAD], *u, W=W)
        wa, wda = R.mc_acq_with_gradient(post["mean"][:, :P.NGRAD], post["sigma"][:, :P.NGRAD], post["dmean"], post["dvar"], post["mu_eval"], W,
                                         kind, thetas, P.PROB, params)
        _close(m, "uEI with gradient, %s" % kind, a, wa[:, 0], *P.ACQ_VALUE)
        _per_coordinate(m, "d uEI / dx, %s" % kind, da, wda, *P.ACQ_GRAD)


# ---- expected utility ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_expected_utility(B, m):
    """bocf_expected_utility (eu_kernel<MC>), the three modes, value and gradient, candidate i with parameter row i mod 2; gate of
    test_expected_utility_matches_oracle_fixed_hyps."""
    p, post = P.problem(m), P.posterior(m)
    model = _fixed_model(B, p)
    X = p["Xc"][:P.NGRAD]
    rows = p["rows"][:P.NGRAD]
    for mode, kind in P.eu_cases(m):
        thetas, params = P.support(m, kind)
        v, g = model.expected_utility(X, mode, kind, thetas, rows, Z=p["Zeu"], n_hyps=1, grad=True, util_params=params)
        wv, wg = P.expected_utility(post, mode, kind, thetas, rows, p["Zeu"], params, n=P.NGRAD)
        _close(m, "expected utility, %s %s" % (mode, kind), v, wv, P.EU_RTOL, P.EU_ATOL_SCALE * np.abs(wv).max())
        _per_coordinate(m, "d expected utility / dx, %s %s" % (mode, kind), g, wg, P.EU_RTOL, P.EU_ATOL_SCALE * np.abs(wg).max())
        vall = model.expected_utility(p["Xc"], mode, kind, thetas, p["rows"], Z=p["Zeu"], n_hyps=1, util_params=params)
        wall = P.expected_utility(post, mode, kind, thetas, p["rows"], p["Zeu"], params)[0]
        _close(m, "expected utility, %d candidates, %s %s" % (P.C, mode, kind), vall, wall, P.EU_RTOL, P.EU_ATOL_SCALE * np.abs(wall).max())


# ---- knowledge gradient ----------------------------------------------------------------------------------------------------------------
def _check_kg(B, m, model, las, p, mode, kind, A=None, tag=""):
    """Gates and near-tie rule of test_kg_values and test_kg_gradients."""
    thetas, params = P.support(m, kind)
    A = p["A"] if A is None else A
    ref = P.kg_reference(las, p, mode, kind, thetas, params, A=A)
    refg = P.kg_reference(las, p, mode, kind, thetas, params, grad=True, n=P.NGRAD, A=A)
    model.set_reference_points(A)
    u = (mode, _util(B, kind), params, thetas, P.PROB, p["Zf"])
    kg = model.acq_kg(p["Xc"], *u, W=p["W"])
    assert np.all(np.isfinite(kg))
    _close(m, "KG%s, %s %s" % (tag, mode, kind), kg, ref["kg"], P.KG_RTOL, P.KG_ATOL_SCALE * ref["vscale"])
    kgg, dkg = model.acq_kg(p["Xc"][:P.NGRAD], *u, W=p["W"], grad=True)
    np.testing.assert_array_equal(kgg, kg[:P.NGRAD])    # the value of the gradient entry: the same bits (test_kg_gradients)
    keep = refg["gap"] >= P.KG_TIE * np.max(np.abs(refg["kg"]))
    print("m %2d KG gradient%s, %s %s: %d of %d candidates near-tied" % (m, tag, mode, kind, np.sum(~keep), P.NGRAD))
    assert np.mean(~keep) <= P.LEFT_OUT
    _per_coordinate(m, "d KG / dx%s, %s %s" % (tag, mode, kind), dkg[keep], refg["dkg"][keep], P.KG_RTOL, P.KG_ATOL_SCALE * np.abs(refg["dkg"]).max())


@pytest.mark.parametrize("m", MS)
def test_knowledge_gradient(B, m):
    """bocf_acq_kg (kg_kernel<MODE, TAB, M>, kg_partials_kernel), the three modes with the utilities each admits, value and gradient."""
    p, la, _ = P.oracle(m)
    model = _fixed_model(B, p)
    for mode, kind in P.kg_cases(m):
        _check_kg(B, m, model, [la], p, mode, kind)


@pytest.mark.parametrize("m,na", P.KG_LIMIT_CASES)
def test_knowledge_gradient_table_limit(B, m, na):
    """Either side of the LDS-table limit as kg.hip computes it (kg_table_bytes; closed mode, neg_sq_dist with theta_dim = m, L = 2, Sf = 4:
    8 (2 m na + 4 m + 2 m + 4 + 16) bytes).  m = 16: 65 440 bytes at na = 252 (the tables in LDS), 65 696 at na = 253 (past 65 536: the tables
    in memory, kg_kernel<MODE, false, 0>); m = 8: 65 440 at na = 507, 65 568 at na = 508 (kg_kernel<MODE, false, 8>: the memory variant of a
    templated m)."""
    lds = P.kg_table_bytes(m, na) <= P.TABLE_LIMIT
    assert lds == (na in (252, 507)) and P.kg_table_bytes(16, 252) == 65440 and P.kg_table_bytes(8, 508) == 65568
    p, la, _ = P.oracle(m)
    _check_kg(B, m, _fixed_model(B, p), [la], p, "closed", "neg_sq_dist", A=P.kg_limit_points(na), tag=" na %d" % na)


# ---- pending points --------------------------------------------------------------------------------------------------------------------
def _check_pending(B, m, model, inp, ref, refg, tag=""):
    """Gates and near-threshold rule of test_values_against_the_restatement / test_gradients_against_the_restatement (test_gpu_pending.py)."""
    kind = inp["kind"]
    model.set_hyperparameters(0)
    model.set_pending_points(inp["P"], inp["Zp"], W=inp["W"])
    u = (_util(B, kind), inp["params"], inp["thetas"], inp["prob"])
    got = model.acq_pending(inp["Xc"], *u, W=inp["W"])
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    print("m %2d pending%s %s: share of candidates above 1e3 x atol %.2f" % (m, tag, kind, P.share(ref["alpha"], P.PEND_ATOL_SCALE * ref["scale"])))
    np.testing.assert_allclose(model.last_pending_jitter, ref["tau"], rtol=1e-6)
    _close(m, "pending%s, %s" % (tag, kind), got, ref["alpha"], P.PEND_RTOL, P.PEND_ATOL_SCALE * ref["scale"])
    model.set_hyperparameters(0)
    gotg, dgot = model.acq_pending(inp["Xc"][:P.NGRAD], *u, W=inp["W"], grad=True)
    np.testing.assert_array_equal(gotg, got[:P.NGRAD])
    keep = refg["gap"] >= P.PEND_NEAR * refg["scale"]
    print("m %2d pending gradient%s %s: %d of %d candidates near a threshold" % (m, tag, kind, np.sum(~keep), P.NGRAD))
    assert np.mean(~keep) <= P.LEFT_OUT
    _per_coordinate(m, "d pending / dx%s, %s" % (tag, kind), dgot[keep], refg["dalpha"][keep], P.PEND_RTOL, P.PEND_ATOL_SCALE * np.abs(refg["dalpha"]).max())


@pytest.mark.parametrize("m", MS)
def test_pending_points(B, m):
    """bocf_acq_pending (pending_acq_kernel<TAB, M> and its gradient kernel), value and gradient, every device utility."""
    p = P.problem(m)
    model = _fixed_model(B, p)
    for kind in P.utilities(m):
        _check_pending(B, m, model, *P.pending_case(m, kind))


@pytest.mark.parametrize("m,r", P.PENDING_LIMIT_CASES)
def test_pending_table_limit(B, m, r):
    """Either side of the LDS-table limit as pending.hip computes it (pending_table_bytes; S = 65, L = 2, neg_sq_dist with theta_dim = m:
    8 (m r S + m S + L S + L m + L + 16) bytes).  m = 16: 59 680 bytes at r = 6 (the tables in LDS), 68 000 at r = 7 (past 65 536: the tables
    in memory, the run-time instantiation); m = 8: 63 712 at r = 14, 67 872 at r = 15 (pending_acq_kernel<false, 8> and its gradient kernel)."""
    lds = P.pending_table_bytes(m, r) <= P.TABLE_LIMIT
    assert lds == (r in (6, 14)) and P.pending_table_bytes(16, 7) == 68000 and P.pending_table_bytes(8, 14) == 63712
    p, la, _ = P.oracle(m)
    inp = P.pending_limit_inputs(m, r)
    ref, refg = PR.case_reference(inp, [la]), PR.case_reference(inp, [la], grad=True, n=P.NGRAD)
    _check_pending(B, m, _fixed_model(B, p), inp, ref, refg, tag=" r %d" % r)


# ---- constrained ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_constrained(B, m):
    """bocf_acq_mc_constrained (the two constrained kernels) and bocf_feasible_best, every device utility; gates of test_gpu_constrained.py."""
    p = P.problem(m)
    model = _fixed_model(B, p)
    for kind in P.utilities(m):
        thetas, params = P.support(m, kind)
        (A, b, eta), ref, refg = P.constrained_case(m, kind)
        model.set_output_constraints(B.OutputConstraints(A, b, eta))
        u = (_util(B, kind), params, thetas)
        got = model.acq_mc_constrained(p["Xc"], *u, P.PROB, W=p["W"])
        best, nf = model.feasible_best(*u)
        print("m %2d constrained %s: share of candidates above 1e3 x atol %.2f, %d of %d evaluated points feasible"
              % (m, kind, P.share(ref["alpha"], P.CON_VALUE[1]), nf, P.N))
        assert nf == ref["n_feasible"] and np.all(np.isfinite(got)) and np.all(got >= 0)
        _close(m, "feasible best, %s" % kind, best, ref["best"], *P.CON_BEST)
        _close(m, "constrained, %s" % kind, got, ref["alpha"], *P.CON_VALUE)
        gotg, dgot = model.acq_mc_constrained(p["Xc"][:P.NGRAD], *u, P.PROB, W=p["W"], grad=True)
        _close(m, "constrained, gradient entry, %s" % kind, gotg, refg["alpha"], *P.CON_VALUE)
        g = refg["dalpha"]
        _per_coordinate(m, "d constrained / dx, %s" % kind, dgot, g, P.CON_GRAD_RTOL, P.CON_GRAD_ATOL * max(1.0, np.abs(g).max()))


# ---- Thompson and pathwise selection --------------------------------------------------------------------------------------------------
def _check_selection(m, what, idx, val, u, k):
    """Path by path: the values are the k largest utilities of the samples the device ranked (rtol and atol 1e-13, as
    test_thompson_select_against_numpy); the indices are k different candidates that reproduce those values in the restatement (as
    test_selection_after_path_values: no tie exclusion needed); the index set is the restatement's wherever its k-th and (k + 1)-th
    values are clearly apart (the rule and margin of test_kg_values: more than 1e-4 of the k-th)."""
    order = np.lexsort((np.arange(len(u)), -u))
    np.testing.assert_allclose(val, u[order[:k]], *P.SELECT_VALUE, err_msg="m = %d: %s" % (m, what))
    assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < len(u), (m, what, idx)
    np.testing.assert_allclose(u[idx], val, *P.SELECT_VALUE, err_msg="m = %d: %s, indices" % (m, what))
    vk, vk1 = u[order[k - 1]], u[order[k]]
    if vk - vk1 > 1e-4 * abs(vk):
        assert set(idx.tolist()) == set(order[:k].tolist()), (m, what)
        return 1
    return 0


@pytest.mark.parametrize("m", MS)
def test_thompson_and_pathwise_selection(B, m):
    """bocf_thompson_select on joint posterior samples (thompson_topk) and on path values (pathwise_topk), each against U of the samples the
    device ranked, as test_gpu_thompson.py; the path values themselves and bocf_path_utility, value and gradient, against
    tests/paths_ref.py with the gates of test_gpu_paths.py (outputs_problem.path_utility_amp)."""
    p = P.problem(m)
    model = _fixed_model(B, p)
    Xc, Sp, k = p["Xc"], P.S_PATHS, P.K_SELECT
    rng = np.random.RandomState(300 + m)
    groups = np.zeros(Sp, dtype=int)
    np.random.seed(P.path_seed(m))
    model.draw_paths(Sp, P.F_PATHS)
    paths = P.paths(m)
    Fp, Gp = paths.values(Xc), paths.gradients(Xc[:P.NGRAD])
    Fd = model.path_values(Xc)
    vgate = P.PATH_VALUE_SCALE * p["var"].max()
    _close(m, "path values", Fd, Fp, 0.0, vgate)
    Z = {0: rng.normal(size=(m, P.C, Sp))}
    compared = 0
    for kind in P.UTILS:
        th, params = P.path_thetas(m, kind)                # one parameter row per path; rosenbrock at an odd m too
        U = B.Utility(parameter_dist=B.ParameterDistribution(support=th, prob_dist=np.full(Sp, 1.0 / Sp)), device=kind, device_params=params)
        idx, val = model.thompson_topk(Xc, th, groups, Z, U, k)
        Fs = model.posterior_samples_f(Xc, Z=Z[0])
        for s in range(Sp):
            compared += _check_selection(m, "thompson_topk %s path %d" % (kind, s), idx[s], val[s], R.utility_eval(kind, th[s], Fs[:, :, s], params), k)
        idx, val = model.pathwise_topk(Xc, th, model._path_groups(Sp), U, k)
        for s in range(Sp):
            compared += _check_selection(m, "pathwise_topk %s path %d" % (kind, s), idx[s], val[s], R.utility_eval(kind, th[s], Fd[:, :, s], params), k)
        v, g = model.path_utility(Xc[:P.NGRAD], P.path_rows(), th, U, grad=True)
        wv, wg, amp = P.path_utility_from(Fp, Gp, kind, th, params)
        _close(m, "path utility, %s" % kind, v, wv, 0.0, vgate * amp)
        _per_coordinate(m, "d path utility / dx, %s" % kind, g, wg, 0.0, vgate / p["ls"].min() * amp)
    print("m %2d selections compared by index set: %d of %d" % (m, compared, 2 * Sp * len(P.UTILS)))
    assert compared >= Sp * len(P.utilities(m))


# ---- traced utility program ----------------------------------------------------------------------------------------------------------------
def _neg_sq_dist(t, y):
    return -np.sum(np.square((y.transpose() - t).transpose()), axis=0)


@pytest.mark.parametrize("m", MS)
def test_traced_program(B, m):
    """The traced program of neg_sq_dist through acq_mc and acq_mc_grad (the util_prog.hip interpreters) against the compiled-in kind;
    gates of _check_ei_pi_grad (tests/test_gpu_utility_program.py)."""
    F = B._ffi
    p = P.problem(m)
    model = _fixed_model(B, p)
    thetas, _ = P.support(m, "neg_sq_dist")
    U = B.Utility(func=_neg_sq_dist, parameter_dist=B.ParameterDistribution(support=thetas, prob_dist=P.PROB), device="program")
    assert U.device_kind(m) == F.UTIL_PROGRAM
    u_ref, u_prog = (F.UTIL_NEG_SQ_DIST, None, thetas, P.PROB), (F.UTIL_PROGRAM, None, thetas, P.PROB)
    _close(m, "uEI, program", model.acq_mc(p["Xc"], F.ACQ_EI, *u_prog, W=p["W"], program=U.program_blob), model.acq_mc(p["Xc"], F.ACQ_EI, *u_ref, W=p["W"]),
           1e-5, 1e-9)
    a, r = model.acq_mc(p["Xc"], F.ACQ_PI, *u_prog, W=p["W"], program=U.program_blob), model.acq_mc(p["Xc"], F.ACQ_PI, *u_ref, W=p["W"])
    print("m %2d uPI, program: share differing %.4f, max difference %.3g" % (m, np.mean(np.abs(a - r) > 1e-12), np.abs(a - r).max()))
    assert np.mean(np.abs(a - r) > 1e-12) <= 0.01 and np.abs(a - r).max() <= 1.0 / P.S + 1e-12
    (a, da), (r, dr) = model.acq_mc_grad(p["Xc"][:P.NGRAD], *u_prog, W=p["W"], program=U.program_blob), model.acq_mc_grad(p["Xc"][:P.NGRAD], *u_ref, W=p["W"])
    assert np.abs(dr).max() > 0
    _close(m, "uEI with gradient, program", a, r, 1e-5, 1e-9)
    _per_coordinate(m, "d uEI / dx, program", da, dr, 1e-4, 1e-8)


# ---- hyper-samples --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [8, 9, 16])
def test_two_hyper_samples(B, m):
    """H = 2: 16, 18 and 32 outputs in the context, each group within the limit; acq_mc, acq_mc_grad, expected utility, KG, pending and
    constrained against the mean (expected utility: the sum) over the per-sample references.  The Monte-Carlo acquisitions take the
    best-so-far of the hyper-sample current on entry (0 here), KG each sample's own."""
    F = B._ffi
    H = 2
    p = P.problem(m)
    las = P.hyper_lookaheads(m, H)
    posts = [P.posterior_of(la, p["Xc"]) for la in las]
    model = _hyper_model(B, p, H)
    Xc, W, Xg = p["Xc"], p["W"], p["Xc"][:P.NGRAD]
    kind = "neg_sq_dist"
    thetas, params = P.support(m, kind)
    u = (_util(B, kind), params, thetas, P.PROB)
    own = [dict(q, mu_eval=posts[0]["mu_eval"]) for q in posts]            # the incumbent of hyper-sample 0 for every h
    model.set_hyperparameters(0)
    _close(m, "H 2: uEI, %s" % kind, model.acq_mc(Xc, F.ACQ_EI, *u, W=W), np.mean([P.mc_values(q, W, kind, thetas, P.PROB, params) for q in own], 0),
           *P.MC_VALUE)
    model.set_hyperparameters(0)
    a, da = model.acq_mc_grad(Xg, *u, W=W)
    rs = [R.mc_acq_with_gradient(q["mean"][:, :P.NGRAD], q["sigma"][:, :P.NGRAD], q["dmean"], q["dvar"], q["mu_eval"], W, kind, thetas, P.PROB, params)
          for q in own]
    _close(m, "H 2: uEI with gradient", a, np.mean([r[0][:, 0] for r in rs], 0), *P.ACQ_VALUE)
    _per_coordinate(m, "H 2: d uEI / dx", da, np.mean([r[1] for r in rs], 0), *P.ACQ_GRAD)
    rows = p["rows"][:P.NGRAD]
    for mode in ("closed", "mc"):
        v, g = model.expected_utility(Xg, mode, kind, thetas, rows, Z=p["Zeu"], n_hyps=H, grad=True, util_params=params)
        es = [P.expected_utility(q, mode, kind, thetas, rows, p["Zeu"], params, n=P.NGRAD) for q in posts]
        wv, wg = np.sum([e[0] for e in es], 0), np.sum([e[1] for e in es], 0)
        _close(m, "H 2: expected utility, %s" % mode, v, wv, P.EU_RTOL, P.EU_ATOL_SCALE * np.abs(wv).max())
        _per_coordinate(m, "H 2: d expected utility / dx, %s" % mode, g, wg, P.EU_RTOL, P.EU_ATOL_SCALE * np.abs(wg).max())
    _check_kg(B, m, model, las, p, "closed", kind, tag=" H 2")
    _check_kg(B, m, model, las, p, "mc", kind, tag=" H 2")
    inp = dict(P.pending_inputs(m, kind, 10), H=H)
    _check_pending(B, m, model, inp, PR.case_reference(inp, las), PR.case_reference(inp, las, grad=True, n=P.NGRAD), tag=" H 2")
    (A, b, eta), _, _ = P.constrained_case(m, kind)
    cu = (W, thetas, P.PROB, kind, params, A, b, eta)
    mts = [q["mu_eval"] for q in posts]
    ref = CR.constrained_hyper([q["mean"] for q in posts], [q["var"] for q in posts], mts, *cu, best_group=0)
    refg = CR.constrained_hyper([q["mean"][:, :P.NGRAD] for q in posts], [q["var"][:, :P.NGRAD] for q in posts], mts, *cu,
                                dmeans=[q["dmean"] for q in posts], dvars=[q["dvar"] for q in posts], best_group=0)
    model.set_output_constraints(B.OutputConstraints(A, b, eta))
    model.set_hyperparameters(0)
    _close(m, "H 2: constrained", model.acq_mc_constrained(Xc, *u, W=W), ref["alpha"], *P.CON_VALUE)
    model.set_hyperparameters(0)
    g = refg["dalpha"]
    _per_coordinate(m, "H 2: d constrained / dx", model.acq_mc_constrained(Xg, *u, W=W, grad=True)[1], g, P.CON_GRAD_RTOL,
                    P.CON_GRAD_ATOL * max(1.0, np.abs(g).max()))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _rosenbrock(a, y):
    h = y.shape[0] // 2
    return -(np.sum((a[0] - y[:h]) ** 2, axis=0) + 100.0 * np.sum(y[h:2 * h] ** 2, axis=0))


@pytest.mark.parametrize("m", [1, 9, 15])
def test_rosenbrock_at_odd_output_counts_is_refused(B, m):
    """Every entry point that states it: bocf_acq_mc and bocf_acq_mc_grad, bocf_expected_utility, bocf_acq_kg, bocf_acq_pending, the
    constrained pair, and the recognition of a Python callable (Utility.device_kind)."""
    F = B._ffi
    p = P.problem(m)
    model = _fixed_model(B, p)
    th = np.array([[0.3], [0.5]])
    u = (F.UTIL_ROSENBROCK, None, th, P.PROB)
    X = p["Xc"][:8]
    err = F.BocfHipError
    with pytest.raises(err, match="bocf_acq_mc.*rosenbrock utility needs theta_dim >= 1 and even m"):
        model.acq_mc(X, F.ACQ_EI, *u, W=p["W"])
    with pytest.raises(err, match="bocf_acq_mc_grad.*rosenbrock utility needs theta_dim >= 1 and even m"):
        model.acq_mc_grad(X, *u, W=p["W"])
    for mode in ("closed", "mc"):
        with pytest.raises(err, match="bocf_expected_utility.*rosenbrock utility needs even m"):
            model.expected_utility(X, mode, "rosenbrock", th, np.zeros(8, dtype=int), Z=p["Zeu"], n_hyps=1)
        model.set_reference_points(p["A"])
        with pytest.raises(err, match="bocf_acq_kg.*rosenbrock utility needs even m"):
            model.acq_kg(X, mode, F.UTIL_ROSENBROCK, None, th, P.PROB, p["Zf"], W=p["W"])
    inp = P.pending_inputs(m, "neg_sq_dist")
    model.set_pending_points(inp["P"], inp["Zp"], W=p["W"])
    with pytest.raises(err, match="bocf_acq_pending.*rosenbrock utility needs even m"):
        model.acq_pending(X, *u, W=p["W"])
    model.set_output_constraints(B.OutputConstraints(np.ones((1, m)), [0.0], 0.05))
    with pytest.raises(err, match="bocf_acq_mc_constrained.*rosenbrock utility needs even m"):
        model.acq_mc_constrained(X, *u, W=p["W"])
    with pytest.raises(err, match="bocf_feasible_best.*rosenbrock utility needs even m"):
        model.feasible_best(F.UTIL_ROSENBROCK, None, th)
    U = B.Utility(func=_rosenbrock, parameter_dist=B.ParameterDistribution(support=th, prob_dist=P.PROB))
    try:
        kind = U.device_kind(m)
    except NotImplementedError:
        kind = None
    assert kind != F.UTIL_ROSENBROCK
    if m > 1:                                            # (at m = 1 the callable is the constant 0; the same callable is recognised at the even count next to m)
        assert kind is None
        assert B.Utility(func=_rosenbrock, parameter_dist=B.ParameterDistribution(support=th, prob_dist=P.PROB)).device_kind(m - 1) == F.UTIL_ROSENBROCK
    # the model serves the next call as if nothing had happened
    thetas, params = P.support(m, "neg_sq_dist")
    _close(m, "uEI after the refusals", model.acq_mc(p["Xc"], F.ACQ_EI, F.UTIL_NEG_SQ_DIST, None, thetas, P.PROB, W=p["W"]),
           P.mc_values(P.posterior(m), p["W"], "neg_sq_dist", thetas, P.PROB), *P.MC_VALUE)


def test_seventeen_outputs_fit_and_every_utility_entry_point_refuses(B):
    """A 17-output model fits and predicts against the oracle; every entry point that evaluates a device utility returns a negative status
    whose message names it, before any launch, and leaves its output buffers alone.  What refuses is group_size in capi.hip,
    `m > BOCF_MAX_M` in capi_kg.hip and capi_pending.hip, and `per > BOCF_MAX_M` in capi_thompson.hip and capi_paths.hip: the last two
    after posterior samples and paths were staged for the 17 outputs (bocf_posterior_samples, bocf_set_paths and bocf_path_values index
    the outputs by workgroup row and hold no [BOCF_MAX_M] array), so that nothing but that guard stands before thompson_util_kernel and
    path_chain_kernel.  Five entry points are refused by an earlier check of the same block because their prerequisite setter already
    refuses 17 outputs, which makes their own output-count check unreachable: bocf_acq_mc, bocf_acq_mc_grad and bocf_set_pending_points
    (bocf_set_mc_samples refuses: no normals can be resident), bocf_acq_mc_constrained and bocf_feasible_best
    (bocf_set_output_constraints refuses: no constraints can be resident)."""
    F = B._ffi
    m, n = 17, 8
    rng = np.random.RandomState(17)
    X = 0.7 * rng.uniform(size=(P.N, P.D))
    Y = [0.3 * np.sin(X.dot(rng.uniform(1.0, 3.0, size=P.D)) + j) for j in range(m)]
    p = dict(kinds=P.kinds(m), X=X, Y=Y, var=rng.uniform(0.8, 1.6, size=m), ls=rng.uniform(0.4, 0.7, size=(m, P.D)) * np.sqrt(P.D),
             nz=np.full(m, P.NOISE), Xc=rng.uniform(size=(P.C, P.D)))
    ref = R.MultiOutputGPRef(p["kinds"], p["var"], list(p["ls"]), list(p["nz"]))
    ref.updateModel(X, [y[:, None] for y in Y])
    model = _fixed_model(B, p)
    _check_fit_and_predict(m, model, p, ref)
    lib, h, dp = F.load(), model._context().handle, F.dptr
    model._set_candidates(p["Xc"][:n])
    th, prob, W = F.f64(rng.normal(size=(2, m))), F.f64(P.PROB), F.f64(rng.normal(size=(P.S, m)))
    th1 = F.f64(np.zeros((2, 1)))
    Zf, Zp, Xp = F.f64(rng.normal(size=(P.SF, m))), F.f64(rng.normal(size=(P.S, m, P.RP))), F.f64(rng.uniform(size=(P.RP, P.D)))
    rows = np.zeros(n, dtype=np.int32)
    rows_p = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    nf = ctypes.c_longlong(-7)

    group_size = b"too many outputs per hyper-sample"
    too_many = b"more outputs per hyper-sample than the device utilities take (16)"

    def refused(name, rc, *outs, why=None):
        msg = lib.bocf_last_error()
        print("m 17 %-28s status %d: %s" % (name, rc, msg.decode()))
        assert rc < 0 and name.encode() in msg, (name, rc, msg)
        assert why is None or why in msg, (name, msg)
        for o in outs:
            assert np.all(o == SENTINEL), name

    def out(*shape):
        return np.full(shape, SENTINEL)

    a, da = out(n), out(n, P.D)
    refused("bocf_acq_linear", lib.bocf_acq_linear(h, F.ACQ_EI, dp(th), dp(prob), 2, dp(a)), a, why=group_size)
    refused("bocf_acq_linear_grad", lib.bocf_acq_linear_grad(h, F.ACQ_EI, dp(th), dp(prob), 2, dp(a), dp(da)), a, da, why=group_size)
    refused("bocf_set_mc_samples", lib.bocf_set_mc_samples(h, dp(W), P.S), why=group_size)
    # (no normals can be resident -- the setter above refuses --, so the two Monte-Carlo entry points stop at "no Monte-Carlo samples set",
    # before the group_size check they share with the setter; likewise bocf_set_pending_points below)
    refused("bocf_acq_mc", lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_NEG_SQ_DIST, None, 0, dp(th), m, dp(prob), 2, dp(a)), a)
    refused("bocf_acq_mc_grad", lib.bocf_acq_mc_grad(h, F.UTIL_NEG_SQ_DIST, None, 0, dp(th), m, dp(prob), 2, dp(a), dp(da)), a, da)
    refused("bocf_set_eu_samples", lib.bocf_set_eu_samples(h, dp(F.f64(rng.normal(size=(2, P.S, m)))), 2, P.S), why=group_size)
    for mode in (F.EU_MEAN, F.EU_CLOSED, F.EU_MC):
        refused("bocf_expected_utility", lib.bocf_expected_utility(h, mode, F.UTIL_NEG_SUM_EXP, None, 0, dp(th1), 1, 2, rows_p, 1, dp(a), dp(da)), a, da, why=group_size)
    model.set_reference_points(rng.uniform(size=(P.NA, P.D)))                  # (staging needs no utility: it serves 17 outputs)
    model._set_candidates(p["Xc"][:n])
    for mode in (F.EU_MEAN, F.EU_CLOSED, F.EU_MC):
        refused("bocf_acq_kg", lib.bocf_acq_kg(h, mode, F.UTIL_NEG_SUM_EXP, None, 0, dp(th1), 1, dp(prob), 2, dp(Zf), P.SF, dp(a), dp(da)), a, da, why=too_many)
    jit = out(m)
    refused("bocf_set_pending_points", lib.bocf_set_pending_points(h, dp(Xp), P.RP, dp(Zp), P.S, 5, dp(jit)), jit)
    refused("bocf_acq_pending", lib.bocf_acq_pending(h, F.UTIL_NEG_SUM_EXP, None, 0, dp(th1), 1, dp(prob), 2, dp(a), dp(da)), a, da, why=too_many)
    A, b, eta = F.f64(rng.normal(size=(2, m))), F.f64(np.zeros(2)), F.f64(np.full(2, 0.05))
    refused("bocf_set_output_constraints", lib.bocf_set_output_constraints(h, dp(A), dp(b), dp(eta), 2, m))
    # (no constraints can be resident -- the setter above refuses --, so the constrained pair stops at "no output constraints resident",
    # before its own `m > BOCF_MAX_M`)
    refused("bocf_acq_mc_constrained", lib.bocf_acq_mc_constrained(h, F.UTIL_NEG_SUM_EXP, None, 0, dp(th1), 1, dp(prob), 2, dp(a), dp(da)), a, da)
    best = out(2)
    refused("bocf_feasible_best", lib.bocf_feasible_best(h, F.UTIL_NEG_SUM_EXP, None, 0, dp(th1), 1, 2, dp(best), ctypes.byref(nf)), best)
    assert nf.value == -7
    # the selection entry points, with their prerequisites resident: joint samples, then paths (both serve 17 outputs, checked here)
    Xn, Sp = p["Xc"][:n], 2
    Fs = model.posterior_samples_f(Xn, Z=rng.normal(size=(m, n, Sp)))
    assert Fs.shape == (m, n, Sp) and np.all(np.isfinite(Fs))
    thp = F.f64(np.zeros((Sp, 1)))
    idx, val = np.full((Sp, 4), -7, dtype=np.int64), out(Sp, 4)
    select = lambda: lib.bocf_thompson_select(h, F.UTIL_NEG_SUM_EXP, None, 0, dp(thp), 1, 4, idx.ctypes.data_as(F._c_ll_p), dp(val))  # noqa: E731
    refused("bocf_thompson_select", select(), val, why=too_many)
    assert np.all(idx == -7)
    np.random.seed(17)
    model.draw_paths(Sp, 16)
    paths = PTH.Paths(ref, [y[:, None] for y in Y], *PTH.draw(p["kinds"], P.N, P.D, 16, Sp, np.random.RandomState(17)))
    _close(m, "path values", model.path_values(Xn), paths.values(Xn), 0.0, P.PATH_VALUE_SCALE * p["var"].max())
    refused("bocf_thompson_select", select(), val, why=too_many)                 # (the path values are the resident samples now)
    assert np.all(idx == -7)
    refused("bocf_path_utility", lib.bocf_path_utility(h, F.UTIL_NEG_SUM_EXP, None, 0, dp(thp), 1, Sp, rows_p, dp(a), dp(da)), a, da, why=too_many)
    # the context serves the model as before
    mean, _ = model.predict(p["Xc"])
    _close(m, "mean after the refusals", mean, ref.predict(p["Xc"])[0], P.MEAN_RTOL, P.MEAN_ATOL)
