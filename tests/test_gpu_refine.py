"""GPU checks of the device-resident anchor refinement (bocf_refine_acq).

The device loop against the host loop: lbfgsb_batched driving model.acq_linear_grad / model.acq_mc_grad on the same model and the same
starts, with the tolerances of tests/test_optimizer_cpu.py (X to 1e-6, F to rtol 1e-10 / atol 1e-12, per-row iteration and evaluation
counts equal when maxfun or maxiter cuts the run, iterations within 3 otherwise).  The state machine alone (refine_advance_kernel on the polynomial
of refine_poly.h through a probes-build hook) equals the CPU driver bit for bit.  Every figure is printed before its assertion: run
with -s to keep them.  Nothing here waits on the device (no polling kernel, no cross-workgroup dependency), so as in the other GPU tests
no per-test time limit is set beyond the runner's.
Run on the MI355X box: python -m pytest tests/test_gpu_refine.py -m gpu"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dims_problem as P  # noqa: E402
import refine_cases as C  # noqa: E402

from bocf_amd import _ffi  # noqa: E402
from bocf_amd import acquisition_optimizer as AO  # noqa: E402
from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

D, M, S = 3, 3, 128
BOUNDS = [(0.0, 1.0)] * D
WHO = b"bocf_refine_acq"


@pytest.fixture(scope="module")
def B():
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


@functools.lru_cache(maxsize=None)
def _problem(N):
    return R.synthetic_problem(N, D, M, 8, S, 4242)      # the problem of test_acquisition_optimizer_vs_reference_flow (N = 40 there)


_models = {}


def _model(B, N):
    if N not in _models:
        p = _problem(N)
        kern = [B.kern.RBF(D, variance=p["variances"][j], lengthscale=p["lengthscales"][j], ARD=True) for j in range(M)]
        model = B.multi_outputGP(M, kernel=kern, noise_var=list(p["noise"]), fixed_hyps=True)
        model.updateModel(p["X"], p["Y"])
        _models[N] = model
    return _models[N]


def _neg_sq_dist(t, y):
    return -np.sum(np.square((y.transpose() - t).transpose()), axis=0)


@functools.lru_cache(maxsize=None)
def _program():
    from bocf_amd.utility import ParameterDistribution, Utility
    U = Utility(func=_neg_sq_dist, parameter_dist=ParameterDistribution(support=np.array([[1.2, -1.0, 1.1]]), prob_dist=np.ones(1)), device="program")
    assert U.device_kind(M) == _ffi.UTIL_PROGRAM
    return U.program_blob


def _form(name, N):
    """Keyword arguments of multi_outputGP.refine_acq that describe the objective."""
    linear = dict(thetas=np.array([[1.0 / 3, 1.0 / 3, 1.0 / 3], [0.5, 0.2, 0.3]]), prob=np.array([0.4, 0.6]))
    mc = dict(form=_ffi.REFINE_MC, thetas=np.array([[1.2, -1.0, 1.1], [0.9, -0.6, 0.8]]), prob=np.array([0.7, 0.3]), W=_problem(N)["W"])
    if name == "EI":
        return dict(form=_ffi.REFINE_LINEAR, kind=_ffi.ACQ_EI, **linear)
    if name == "PI":
        return dict(form=_ffi.REFINE_LINEAR, kind=_ffi.ACQ_PI, **linear)
    if name == "mc":
        return dict(util_kind=_ffi.UTIL_NEG_SQ_DIST, **mc)
    return dict(util_kind=_ffi.UTIL_PROGRAM, program=_program(), **dict(mc, thetas=mc["thetas"][:1], prob=np.ones(1)))


def _host_f_df(model, form):
    """What acquisition_function_withGradients hands the host loop: (-acq, -d acq / dX) of the rows it is given."""
    def f_df(Z):
        if form["form"] == _ffi.REFINE_LINEAR:
            a, g = model.acq_linear_grad(Z, form["kind"], form["thetas"], form["prob"])
        else:
            a, g = model.acq_mc_grad(Z, form["util_kind"], form.get("util_params"), form["thetas"], form["prob"], W=form["W"], program=form.get("program"))
        return -a, -g
    return f_df


def _starts(f_df, A, d=D, seed=11, near=None):
    """The A best of 400 uniform points under the objective, as the optimiser picks its anchors: where the acquisition is not flat.
    near (n, d): the A points with the largest gradient among those and the rows of `near` moved by N(0, 0.02^2) instead -- the
    probability of improvement is 0 or 1 to rounding almost everywhere (every uniform start would stop where it is) and changes next to
    the evaluated points."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(400, d))
    if near is not None:
        X = np.vstack([X, np.clip(near + 0.02 * rng.normal(size=near.shape), 0.0, 1.0)])
    f, g = f_df(X)
    return X[np.argsort(f if near is None else -np.abs(g).max(1), kind="stable")[:A]]


def _device(model, X0, bounds, form, **kw):
    X, F, info = model.refine_acq(X0, bounds, **dict(form, **kw))
    return dict(X=X, F=F, iterations=info["iterations"], evaluations=info["evaluations"], reasons=[_ffi.REFINE_REASONS.index(r) for r in info["reasons"]],
                passes=info["passes"], host_syncs=info["host_syncs"])


def _compare_loops(model, form, X0, bounds, settings, what):
    f_df = _host_f_df(model, form)
    for kw in settings:
        ref = C.host_reference(f_df, X0, bounds, loop=AO.lbfgsb_batched, **kw)
        got = _device(model, X0, bounds, form, **kw)
        C.compare(got, ref, C.CUT(kw), "%s %s:" % (what, kw))
        lo, hi = np.array(bounds).T
        assert np.all(got["X"] >= lo) and np.all(got["X"] <= hi)
    return ref


# ---- device loop against host loop
@pytest.mark.parametrize("form", ["EI", "PI", "mc", "program"])
@pytest.mark.parametrize("N", [40, 130])
def test_device_loop_equals_host_loop(B, N, form):
    model = _model(B, N)
    fm = _form(form, N)
    X0 = _starts(_host_f_df(model, fm), 16, near=_problem(N)["X"] if form == "PI" else None)
    ref = _compare_loops(model, fm, X0, BOUNDS, C.SETTINGS, "N %d %s A 16" % (N, form))
    # the comparison is of runs, not of zeros: some start was not stationary (the probability of improvement is a step at this noise
    # level: one iteration reaches its plateau, so one is all that can be asked of it)
    assert ref["iterations"].max() >= (1 if form == "PI" else 3)


@pytest.mark.parametrize("form", ["EI", "mc"])
@pytest.mark.parametrize("A", [1, 17, 64])
def test_row_counts_around_the_small_path_and_at_the_cap(B, A, form):
    """A = 1 and 16: both loops send every point through the n <= 16 path of the predict pass.  A = 17 and 64: the host loop evaluates
    the running rows only, so once 16 or fewer are left it goes through that path, where a whole-batch posterior is the GEMM path's; on
    the same 16 points the two paths differ by 1.3e-12 (Monte-Carlo form) to 1.2e-7 (EI, values near 1e-9) relative in the acquisition,
    and three iterations carry that to 1.19e-10 relative in F, beyond the rtol of 1e-10 (measured on an MI355X with a device loop that
    predicted the whole batch only).  So for A > 16 the device loop predicts twice per pass -- the whole batch, and the first 16 running
    rows gathered -- and reads the gathered columns once no more than 16 rows run (refine_compact_kernel)."""
    model = _model(B, 130)
    fm = _form(form, 130)
    X0 = _starts(_host_f_df(model, fm), A)
    _compare_loops(model, fm, X0, BOUNDS, C.SETTINGS, "N 130 %s A %d" % (form, A))


@pytest.mark.parametrize("form", ["EI", "mc"])
@pytest.mark.parametrize("A", [17, 64])
def test_row_counts_above_the_small_path_with_one_predict_path(B, A, form):
    """With the n <= 16 path switched off (option small_path, speed only) both loops evaluate every point through the same kernels
    whatever the row count: the device loop then IS the host loop, bit for bit."""
    model = _model(B, 130)
    fm = _form(form, 130)
    f_df = _host_f_df(model, fm)
    X0 = _starts(f_df, A)
    model.set_option("small_path", 0)
    try:
        for kw in C.SETTINGS:
            ref = C.host_reference(f_df, X0, BOUNDS, loop=AO.lbfgsb_batched, **kw)
            got = _device(model, X0, BOUNDS, fm, **kw)
            assert np.array_equal(got["X"], ref["X"]) and np.array_equal(got["F"], ref["F"]), kw
            assert np.array_equal(got["iterations"], ref["iterations"]) and np.array_equal(got["evaluations"], ref["evaluations"]), kw
    finally:
        model.set_option("small_path", 1)


@pytest.mark.parametrize("form", ["EI", "mc"])
@pytest.mark.parametrize("d", [1, 32])
def test_input_dimensions_1_and_32(B, d, form):
    N, Cn, noise = 200, 518, 1e-4
    p = P.problem(d, N, Cn, noise)
    model = P.mixed_model(B, p)
    inp = P.acquisition_inputs(d, N, Cn, noise)            # supports at which the oracle's gradient at Xc[:7] is non-zero in every coordinate
    if form == "EI":
        fm = dict(form=_ffi.REFINE_LINEAR, kind=_ffi.ACQ_EI, thetas=inp["ma"][0], prob=P.ACQ_PROB)
    else:
        fm = dict(form=_ffi.REFINE_MC, util_kind=_ffi.UTIL_NEG_SQ_DIST, thetas=inp["mc"][0], prob=P.ACQ_PROB, W=p["W"])
    _compare_loops(model, fm, p["Xc"][:P.N_ACQ], [(0.0, 1.0)] * d, C.SETTINGS, "d %d %s" % (d, form))


# ---- two hyper-samples, on the C ABI (a fixed-hyper-parameter model holds one)
def _raw_refine(lib, h, d, form, kind, util_kind, params, thetas, prob, X0, lo, hi, poll_every=8, **kw):
    s = dict(C.DEFAULTS, **kw)
    X0 = _ffi.f64(np.atleast_2d(X0))
    A = X0.shape[0] if X0.size else 0
    th = None if thetas is None else _ffi.f64(np.atleast_2d(thetas))
    par, pr = None if params is None else _ffi.f64(params), None if prob is None else _ffi.f64(prob)
    X, F = np.empty((max(A, 1), d)), np.empty(max(A, 1))
    it, nf, why = (np.zeros(max(A, 1), dtype=np.int32) for _ in range(3))
    counters = (ctypes.c_longlong * 2)()
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    rc = lib.bocf_refine_acq(h, form, kind, util_kind, _ffi.dptr(par), 0 if par is None else par.size, _ffi.dptr(th), 0 if th is None else th.shape[1],
                             _ffi.dptr(pr), 1 if th is None else th.shape[0], _ffi.dptr(X0), A, _ffi.dptr(_ffi.f64(lo)), _ffi.dptr(_ffi.f64(hi)),
                             s["maxiter"], s["m"], s["factr"], s["pgtol"], s["max_ls"], s["c1"], -1 if s["maxfun"] is None else s["maxfun"], poll_every,
                             _ffi.dptr(X), _ffi.dptr(F), ip(it), ip(nf), ip(why), counters)
    return rc, dict(X=X, F=F, iterations=it.astype(int), evaluations=nf.astype(int), reasons=why.astype(int), passes=int(counters[0]),
                    host_syncs=int(counters[1]))


def test_two_hyper_samples():
    H, N = 2, 40
    p = _problem(N)
    rng = np.random.RandomState(5)
    var = 0.8 + 0.4 * rng.uniform(size=H * M)
    ls = np.stack(p["lengthscales"] * H) * (0.9 + 0.2 * rng.uniform(size=(H * M, D)))
    lib, ctx, dp = _ffi.load(), _ffi.Context(0), _ffi.dptr
    h = ctx.handle
    ctx.set_option("hyper_samples", H)
    Y = np.tile(np.stack([y[:, 0] for y in p["Y"]]), (H, 1))
    _ffi.check(lib.bocf_fit(h, dp(_ffi.f64(p["X"])), dp(_ffi.f64(Y)), N, D, H * M, _ffi.KERN_RBF, dp(_ffi.f64(var)), dp(_ffi.f64(ls)),
                            dp(np.full(H * M, 1e-6)), 5, None, None), "bocf_fit")
    ctx.set_option("best_group", 1)                        # (uEI_noiseless: the incumbent of the hyper-sample current on entry)
    _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(p["W"])), S), "bocf_set_mc_samples")
    thetas, prob = _ffi.f64([[1.2, -1.0, 1.1], [0.9, -0.6, 0.8]]), _ffi.f64([0.7, 0.3])

    def f_df(Z):
        Z = _ffi.f64(Z)
        a, g = np.empty(len(Z)), np.empty(Z.shape)
        _ffi.check(lib.bocf_set_candidates(h, dp(Z), len(Z)), "bocf_set_candidates")
        _ffi.check(lib.bocf_acq_mc_grad(h, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(thetas), M, dp(prob), 2, dp(a), dp(g)), "bocf_acq_mc_grad")
        return -a, -g
    X0 = _starts(f_df, 16)
    for kw in C.SETTINGS:
        ref = C.host_reference(f_df, X0, BOUNDS, loop=AO.lbfgsb_batched, **kw)
        rc, got = _raw_refine(lib, h, D, _ffi.REFINE_MC, 0, _ffi.UTIL_NEG_SQ_DIST, None, thetas, prob, X0, [0.0] * D, [1.0] * D, **kw)
        assert rc == 0, lib.bocf_last_error()
        C.compare(got, ref, C.CUT(kw), "H 2 mc %s:" % (kw,))
    ctx.close()


# ---- the state machine on the device alone
def test_state_machine_on_the_device_equals_the_cpu_driver_bit_for_bit(tmp_path_factory):
    if not os.path.exists(C.CLANG):
        pytest.skip("no clang++ next to hipcc")
    driver = C.build_driver(tmp_path_factory.mktemp("refine_bits"))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    with _ffi.probes_library() as lib:
        for d in (1, 6, 32):
            for boxed in (True, False):
                X0, bounds = C.poly_problem(d, boxed)
                lo, hi = (_ffi.f64(v) for v in np.array(bounds).T)
                for kw in C.SETTINGS + [dict(m=1), dict(maxiter=0)]:
                    s = dict(C.DEFAULTS, **kw)
                    cpu = C.run_driver(driver, "poly", X0, bounds, **kw)
                    A = len(X0)
                    X, F = np.empty((A, d)), np.empty(A)
                    it, nf, why = (np.zeros(A, dtype=np.int32) for _ in range(3))
                    rc = lib.bocf_refine_probe_poly(_ffi.dptr(_ffi.f64(X0)), A, d, _ffi.dptr(lo), _ffi.dptr(hi), s["maxiter"], s["m"], s["factr"], s["pgtol"],
                                                    s["max_ls"], s["c1"], -1 if s["maxfun"] is None else s["maxfun"], cpu["passes"] + 2,
                                                    _ffi.dptr(X), _ffi.dptr(F), ip(it), ip(nf), ip(why))
                    assert rc == 0, lib.bocf_last_error()
                    what = "d %d boxed %s %s" % (d, boxed, kw)
                    print("%s: %d passes, bits differ in %d of %d doubles" % (what, cpu["passes"], int(np.sum(X.view(np.int64) != cpu["X"].view(np.int64)))
                                                                             + int(np.sum(F.view(np.int64) != cpu["F"].view(np.int64))), X.size + F.size))
                    assert np.array_equal(X.view(np.int64), cpu["X"].view(np.int64)), what
                    assert np.array_equal(F.view(np.int64), cpu["F"].view(np.int64)), what
                    assert np.array_equal(it, cpu["iterations"]) and np.array_equal(nf, cpu["evaluations"]) and np.array_equal(why, cpu["reasons"]), what
                    if not C.CUT(kw) and d > 1:
                        assert cpu["iterations"].max() >= 3, what


# ---- poll_every, maxiter = 0
def test_poll_every_changes_nothing_but_the_synchronisations(B):
    model = _model(B, 130)
    fm = _form("mc", 130)
    X0 = _starts(_host_f_df(model, fm), 16)
    runs = {q: _device(model, X0, BOUNDS, fm, poll_every=q) for q in (1, 5, 1000)}
    for q, r in runs.items():
        print("poll_every %d: %d passes, %d host synchronisations, %d evaluations" % (q, r["passes"], r["host_syncs"], r["evaluations"].sum()))
        assert r["host_syncs"] <= r["passes"] // q + 2
        for key in ("X", "F"):
            assert np.array_equal(r[key].view(np.int64), runs[1][key].view(np.int64)), (q, key)
        for key in ("iterations", "evaluations", "reasons"):
            assert np.array_equal(r[key], runs[1][key]), (q, key)
    assert runs[1]["passes"] == runs[1]["evaluations"].max()          # polled after every pass: stopped with the last row


def test_maxiter_zero_returns_the_clamped_starts(B):
    model = _model(B, 40)
    fm = _form("EI", 40)
    X0 = np.random.RandomState(2).uniform(-0.2, 1.2, size=(5, D))
    got = _device(model, X0, BOUNDS, fm, maxiter=0)
    Xc = np.clip(X0, 0.0, 1.0)
    assert np.array_equal(got["X"], Xc) and got["passes"] == 1
    assert np.all(got["evaluations"] == 1) and np.all(got["iterations"] == 0) and np.all(np.array(got["reasons"]) == C.MAXITER)
    np.testing.assert_allclose(got["F"], _host_f_df(model, fm)(Xc)[0], rtol=1e-10, atol=1e-12)


# ---- through the plug-in surface
@pytest.mark.parametrize("which", ["maEI", "uEI"])
def test_optimize_with_the_device_refinement(B, which):
    p = _problem(40)
    model = _model(B, 40)
    space = AO.Design_space(bounds=BOUNDS)
    out = {}
    for refine in ("host", "device"):
        opt = AO.AcquisitionOptimizer(space, n_starting=400, n_anchor=16, **({} if refine == "host" else {"refine": "device"}))
        if which == "maEI":
            U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.full((1, M), 1.0 / M), prob_dist=np.ones(1)), linear=True)
            acq = B.maEI(model, space, optimizer=opt, utility=U)
        else:
            U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[1.2, -1.0, 1.1]]), prob_dist=np.ones(1)), device="neg_sq_dist")
            acq = B.uEI_noiseless(model, space, optimizer=opt, utility=U)
            acq.W_samples = p["W"]
        assert opt.refine == refine
        np.random.seed(11)
        x_min, fx_min = acq.optimize(x_baseline=p["Xc"][:2])
        out[refine] = (x_min, fx_min, opt.last_info)
    (xh, fh, ih), (xd, fd, idv) = out["host"], out["device"]
    fh, fd = (float(np.asarray(v).reshape(-1)[0]) for v in (fh, fd))
    print("%s: |dx| %.3g, rel |df| %.3g; host %d passes / %d points, device %d passes / %d points / %d synchronisations"
          % (which, np.abs(xh - xd).max(), abs(fh - fd) / abs(fh), ih["f_df_calls"], ih["points_evaluated"], idv["f_df_calls"],
             idv["points_evaluated"], idv["host_syncs"]))
    np.testing.assert_allclose(xd, xh, rtol=0, atol=1e-6)
    np.testing.assert_allclose(fd, fh, rtol=1e-9)
    assert np.array_equal(idv["anchor_points"], ih["anchor_points"]) and np.array_equal(idv["anchor_points_values"], ih["anchor_points_values"])
    assert idv["anchor_points"].shape == (18, D)            # 16 anchors and the two x_baseline rows
    assert set(ih) | {"host_syncs"} <= set(idv)
    assert np.shape(xd) == (1, D)


# ---- state
def test_context_state_after_the_call(B):
    p = _problem(40)
    model, fresh = _model(B, 40), None
    fm = _form("mc", 40)
    X0 = _starts(_host_f_df(model, fm), 4)
    model.acq_mc(p["Xc"], _ffi.ACQ_EI, fm["util_kind"], None, fm["thetas"], fm["prob"], W=fm["W"])
    assert len(model.select_topk(3)[0]) == 3               # an acquisition vector is resident ...
    _device(model, X0, BOUNDS, fm, maxiter=2)
    with pytest.raises(_ffi.BocfHipError, match="no acquisition vector"):
        model.select_topk(3)                               # ... and gone after the refinement
    assert model._resident.candidates is None
    kern = [B.kern.RBF(D, variance=p["variances"][j], lengthscale=p["lengthscales"][j], ARD=True) for j in range(M)]
    fresh = B.multi_outputGP(M, kernel=kern, noise_var=list(p["noise"]), fixed_hyps=True)
    fresh.updateModel(p["X"], p["Y"])
    Xn = np.random.RandomState(9).uniform(size=(33, D))
    args = (_ffi.ACQ_EI, fm["util_kind"], None, fm["thetas"], fm["prob"])
    assert np.array_equal(model.acq_mc(Xn, *args, W=fm["W"]), fresh.acq_mc(Xn, *args, W=fm["W"]))
    assert np.array_equal(model.select_topk(5)[0], fresh.select_topk(5)[0])


# ---- refusals
def test_refusals_name_the_entry_point_and_leave_the_context_usable(B):
    lib = _ffi.load()
    p = _problem(40)
    X0 = p["Xc"][:4]
    lo, hi = [0.0] * D, [1.0] * D
    th, pr = np.array([[1.2, -1.0, 1.1]]), np.ones(1)

    def bad(rc_and_out, text):
        assert rc_and_out[0] < 0
        msg = lib.bocf_last_error()
        assert WHO in msg and text.encode() in msg, msg

    ctx = _ffi.Context(0)
    bad(_raw_refine(lib, ctx.handle, D, _ffi.REFINE_MC, 0, _ffi.UTIL_NEG_SQ_DIST, None, th, pr, X0, lo, hi), "not fitted")
    mean, var, mt = np.zeros((M, 4)), np.ones((M, 4)), np.zeros((M, 6))
    _ffi.check(lib.bocf_set_posterior(ctx.handle, M, 4, 6, _ffi.dptr(mean), _ffi.dptr(var), _ffi.dptr(mt)), "bocf_set_posterior")
    bad(_raw_refine(lib, ctx.handle, 1, _ffi.REFINE_LINEAR, _ffi.ACQ_EI, 0, None, th, pr, X0[:, :1], lo[:1], hi[:1]), "host-given posterior")
    ctx.close()

    kern = [B.kern.RBF(D, variance=p["variances"][j], lengthscale=p["lengthscales"][j], ARD=True) for j in range(M)]
    model = B.multi_outputGP(M, kernel=kern, noise_var=list(p["noise"]), fixed_hyps=True)
    model.updateModel(p["X"], p["Y"])
    h = model._context().handle
    mc = lambda **kw: _raw_refine(lib, h, D, **dict(dict(form=_ffi.REFINE_MC, kind=0, util_kind=_ffi.UTIL_NEG_SQ_DIST, params=None, thetas=th, prob=pr,
                                                         X0=X0, lo=lo, hi=hi), **kw))
    bad(mc(), "no Monte-Carlo samples")                    # MC without samples
    model.set_mc_samples(p["W"])
    bad(mc(X0=np.empty((0, D))), "A out of range")
    bad(mc(X0=np.tile(X0, (17, 1))[:65]), "A out of range")
    bad(mc(lo=[0.0, 0.7, 0.0], hi=[1.0, 0.2, 1.0]), "lo > hi")
    bad(mc(poll_every=0), "poll_every")
    bad(mc(form=2), "unknown form")
    bad(mc(form=_ffi.REFINE_LINEAR, kind=7), "unknown acquisition kind")
    bad(mc(util_kind=_ffi.UTIL_PROGRAM), "no utility program is resident")
    from bocf_amd.utility import ParameterDistribution, Utility
    U = Utility(func=lambda t, y: -np.sum(np.square(y - t[0]), axis=0), device="program",
                parameter_dist=ParameterDistribution(support=np.array([[0.3]]), prob_dist=np.ones(1)))
    U.device_kind(2)                                       # traced for two outputs: the wrong width for this model
    model.set_utility_program(U.program_blob)
    bad(mc(util_kind=_ffi.UTIL_PROGRAM, thetas=np.array([[0.3]])), "was built for m = 2 outputs")
    with pytest.raises(ValueError, match="output_dim"):   # the linear form reads L rows of output_dim doubles: a narrower theta never gets there
        model.refine_acq(X0, BOUNDS, form=_ffi.REFINE_LINEAR, kind=_ffi.ACQ_EI, thetas=np.ones((1, M - 1)), prob=pr)
    # the context is as it was: the same call with good arguments runs, and equals the host loop
    rc, got = mc(maxiter=3)
    assert rc == 0, lib.bocf_last_error()
    fm = dict(form=_ffi.REFINE_MC, util_kind=_ffi.UTIL_NEG_SQ_DIST, thetas=th, prob=pr, W=p["W"])
    C.compare(got, C.host_reference(_host_f_df(model, fm), X0, BOUNDS, loop=AO.lbfgsb_batched, maxiter=3), True, "after the refusals:")
