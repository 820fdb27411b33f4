"""Pathwise posterior samples on the device (bocf_set_paths, bocf_path_values, bocf_path_utility) against the NumPy restatement
tests/paths_ref.py built from the oracle's factors; selection through bocf_thompson_select; lifetime; refusals;
CompositePathwiseThompsonBatch driving CBO end to end.

The value gate is 1e-10 max sigma_f^2 absolute -- the gate of test_posterior_covariance_against_the_oracle at this conditioning (noise
1e-2, lengthscales 0.4 (0.8 ... 1.2)) -- about 500 times the restatement's own error against long double (tests/test_paths_cpu.py) and
about 1e8 times below any indexing mistake: no value is excluded from a comparison.  The candidate tile of path_values_kernel is 64 rows
per workgroup in four 16-row wave tiles, its contraction step 32 rows in instructions of 4."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paths_ref as PR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
_c_int_p = ctypes.POINTER(ctypes.c_int)


def _data(kinds, N, d, seed, ls=0.4):
    rng = np.random.RandomState(seed)
    m = len(kinds)
    X = rng.uniform(size=(N, d))
    Y = [np.sin(3 * X[:, :1] + j) + 0.3 * X[:, -1:] * (j + 1) for j in range(m)]
    var = 0.5 + rng.uniform(size=m)
    lss = [ls * (0.8 + 0.4 * rng.uniform(size=d)) for _ in range(m)]
    return X, Y, var, lss


def _setup(kinds, N, d, seed, ls=0.4, noise=1e-2):
    X, Y, var, lss = _data(kinds, N, d, seed, ls)
    m = len(kinds)
    model = B.multi_outputGP(m, kernel=[KINDS[kinds[j]](d, variance=var[j], lengthscale=lss[j], ARD=True) for j in range(m)],
                             noise_var=[noise] * m, fixed_hyps=True)
    model.updateModel(X, Y)
    ref = R.MultiOutputGPRef(list(kinds), var, lss, [noise] * m)
    ref.updateModel(X, Y)
    return model, ref, var, lss, X, Y


def _stage(handle, draws, group=-1):
    om, ph, w, E = [_ffi.f64(a) for a in draws]
    _ffi.check(_ffi.load().bocf_set_paths(handle, group, _ffi.dptr(om), _ffi.dptr(ph), _ffi.dptr(w), _ffi.dptr(E), om.shape[1], w.shape[2]), "bocf_set_paths")


def _values(handle, M, C, S, group=-1):
    out = np.empty((M, C, S))
    _ffi.check(_ffi.load().bocf_path_values(handle, group, _ffi.dptr(out)), "bocf_path_values")
    return out


def _case(kinds=("rbf", "matern32", "se"), N=200, C=129, S=7, F=130, d=3):
    """One sweep point: the device values of S paths at C candidates against the restatement."""
    model, ref, var, lss, X, Y = _setup(kinds, N, d, 11 + N + d)
    draws = PR.draw(kinds, N, d, F, S, np.random.RandomState(1000 * S + F))
    Xc = np.random.RandomState(C + 7 * d).uniform(size=(C, d))
    h = model._context().handle
    _stage(h, draws)
    model._set_candidates(Xc)
    got = _values(h, len(kinds), C, S)
    want = PR.Paths(ref, Y, *draws).values(Xc)
    err = float(np.max(np.abs(got - want)))
    print("paths", kinds, "N", N, "C", C, "S", S, "F", F, "d", d, "max error", err, "gate", 1e-10 * var.max())
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10 * var.max())


# ---- 1. values against the restatement: one axis at a time around N = 200, C = 129, S = 7, F = 130, d = 3
@pytest.mark.parametrize("N", [1, 127, 128, 129, 300])
def test_values_sweep_N(N):
    _case(N=N)


@pytest.mark.parametrize("C", [1, 15, 16, 17, 63, 64, 65, 513])
def test_values_sweep_C(C):
    _case(C=C)


@pytest.mark.parametrize("S", [1, 15, 16, 17, 33, 64])
def test_values_sweep_S(S):
    _case(S=S)


@pytest.mark.parametrize("F", [1, 3, 4, 5, 130])
def test_values_sweep_F(F):
    _case(F=F)


@pytest.mark.parametrize("d", [1, 8, 9, 32])
def test_values_sweep_d(d):
    _case(d=d)


@pytest.mark.parametrize("kinds", [("rbf",), ("se",), ("matern52",), ("matern32",), ("rbf", "matern32", "se")])
def test_values_sweep_kernels(kinds):
    _case(kinds=kinds)


def _raw_fit(ctx, X, Y, H, var, ls, noise):
    lib = _ffi.load()
    N, d = X.shape
    ctx.set_option("hyper_samples", H)
    _ffi.check(lib.bocf_fit(ctx.handle, _ffi.dptr(_ffi.f64(X)), _ffi.dptr(_ffi.f64(Y)), N, d, Y.shape[0], _ffi.KERN_RBF, _ffi.dptr(_ffi.f64(var)),
                            _ffi.dptr(_ffi.f64(ls)), _ffi.dptr(_ffi.f64(noise)), 5, None, None), "bocf_fit")


def _two_hyper_samples(N=200, d=3, m=2, H=2, seed=4):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    Yg = [np.sin(3 * X[:, :1] + j) + 0.3 * X[:, -1:] * (j + 1) for j in range(m)]
    var = 0.5 + rng.uniform(size=H * m)
    ls = 0.4 * (0.8 + 0.4 * rng.uniform(size=(H * m, d)))
    ctx = _ffi.Context(0)
    _raw_fit(ctx, X, np.tile(np.stack([y[:, 0] for y in Yg]), (H, 1)), H, var, ls, np.full(H * m, 1e-2))
    refs = []
    for g in range(H):
        r = R.MultiOutputGPRef("rbf", var[g * m:(g + 1) * m], list(ls[g * m:(g + 1) * m]), [1e-2] * m)
        r.updateModel(X, Yg)
        refs.append(r)
    return ctx, refs, X, Yg, var


def test_two_hyper_samples_and_groups():
    """group 0, 1 and -1: the same values bit for bit, each group against the restatement with that hyper-sample's hyper-parameters."""
    N, d, m, H, C, S, F = 200, 3, 2, 2, 129, 7, 130
    ctx, refs, X, Yg, var = _two_hyper_samples(N, d, m, H)
    lib = _ffi.load()
    draws = [PR.draw(("rbf",) * m, N, d, F, S, np.random.RandomState(40 + g)) for g in range(H)]
    Xc = np.random.RandomState(3).uniform(size=(C, d))
    _ffi.check(lib.bocf_set_candidates(ctx.handle, _ffi.dptr(_ffi.f64(Xc)), C), "bocf_set_candidates")
    _stage(ctx.handle, [np.concatenate([draws[g][i] for g in range(H)]) for i in range(4)], -1)
    allv = _values(ctx.handle, H * m, C, S, -1)
    for g in range(H):
        want = PR.Paths(refs[g], Yg, *draws[g]).values(Xc)
        np.testing.assert_allclose(allv[g * m:(g + 1) * m], want, rtol=0, atol=1e-10 * var.max())
    for g in range(H):
        _stage(ctx.handle, draws[g], g)
        np.testing.assert_array_equal(_values(ctx.handle, m, C, S, g), allv[g * m:(g + 1) * m])
    np.testing.assert_array_equal(_values(ctx.handle, H * m, C, S, -1), allv)


# ---- 2. batch invariance
def test_a_candidate_value_does_not_depend_on_its_batch():
    kinds = ("rbf", "matern52")
    model, ref, var, lss, X, Y = _setup(kinds, 200, 3, 5)
    draws = PR.draw(kinds, 200, 3, 130, 7, np.random.RandomState(9))
    Xc = np.random.RandomState(10).uniform(size=(513, 3))
    h = model._context().handle
    _stage(h, draws)
    model._set_candidates(Xc)
    whole = _values(h, 2, 513, 7)
    model._set_candidates(Xc[:256])
    first = _values(h, 2, 256, 7)
    model._set_candidates(Xc[256:])
    second = _values(h, 2, 257, 7)
    np.testing.assert_array_equal(first, whole[:, :256])
    np.testing.assert_array_equal(second, whole[:, 256:])
    model._set_candidates(Xc[101:])                                # (a cut inside a workgroup's and a wave's tile: every candidate changes its lane)
    np.testing.assert_array_equal(_values(h, 2, 412, 7), whole[:, 101:])


# ---- 3. selection
def _abs15(t, y):
    return -np.sum(np.abs((np.asarray(y).T - t).T) ** 1.5, axis=0)


@pytest.mark.parametrize("name", ["neg_sq_dist", "linear", "program"])
def test_selection_after_path_values(name):
    """bocf_thompson_select ranks the path values unchanged: its values are the restatement's k largest utilities (1e-9 relative) and its
    indices reproduce those values in the restatement -- a form that needs no tie exclusions."""
    kinds = ("rbf", "matern32", "se")
    m, C, S, k = 3, 300, 6, 9
    model, ref, var, lss, X, Y = _setup(kinds, 120, 2, 8)
    draws = PR.draw(kinds, 120, 2, 130, S, np.random.RandomState(3))
    Xc = np.random.RandomState(6).uniform(size=(C, 2))
    th = np.random.RandomState(8).normal(size=(S, m))
    h = model._context().handle
    _stage(h, draws)
    model._set_candidates(Xc)
    if name == "program":
        U = B.Utility(func=_abs15, parameter_dist=B.ParameterDistribution(support=th, prob_dist=np.full(S, 1.0 / S)), device="program")
        kind = U.device_kind(m)
        model.set_utility_program(U.program_blob)
        host = lambda t, y: _abs15(t, y)
    else:
        kind = {"neg_sq_dist": _ffi.UTIL_NEG_SQ_DIST, "linear": _ffi.UTIL_LINEAR}[name]
        host = lambda t, y: R.utility_eval(name, t, y)
    _ffi.check(_ffi.load().bocf_path_values(h, -1, None), "bocf_path_values")
    idx, val = np.empty((S, k), dtype=np.int64), np.empty((S, k))
    _ffi.check(_ffi.load().bocf_thompson_select(h, kind, None, 0, _ffi.dptr(_ffi.f64(th)), m, k, idx.ctypes.data_as(_ffi._c_ll_p), _ffi.dptr(val)),
               "bocf_thompson_select")
    F = PR.Paths(ref, Y, *draws).values(Xc)
    for s in range(S):
        u = host(th[s], F[:, :, s])
        np.testing.assert_allclose(val[s], np.sort(u)[::-1][:k], rtol=1e-9, atol=0)
        assert len(set(idx[s].tolist())) == k and idx[s].min() >= 0 and idx[s].max() < C
        np.testing.assert_allclose(u[idx[s]], val[s], rtol=1e-9, atol=0)


# ---- 4. bocf_path_utility
def _path_utility(handle, kind, th, P, rows, C, d, grad=True, params=None):
    val, g = np.empty(C), (np.empty((C, d)) if grad else None)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    pa = None if params is None else _ffi.f64(params)
    rc = _ffi.load().bocf_path_utility(handle, kind, _ffi.dptr(pa), 0 if pa is None else pa.size, _ffi.dptr(_ffi.f64(th)), th.shape[1], P,
                                       rows.ctypes.data_as(_c_int_p), _ffi.dptr(val), _ffi.dptr(g))
    return rc, val, g


@pytest.mark.parametrize("C", [1, 16, 17, 200])
def test_path_utility_value_and_gradient(C):
    """Rows with mixed path indices across two hyper-samples; linear with theta = e_j isolates df_j/dx, neg_sq_dist mixes the outputs.
    Gradient gate 1e-10 max sigma_f^2 / min l: the derivative carries 1 / l."""
    N, d, m, H, S, F = 200, 3, 2, 2, 5, 130
    ctx, refs, X, Yg, var = _two_hyper_samples(N, d, m, H)
    lib = _ffi.load()
    draws = [PR.draw(("rbf",) * m, N, d, F, S, np.random.RandomState(50 + g)) for g in range(H)]
    for g in range(H):
        _stage(ctx.handle, draws[g], g)
    rng = np.random.RandomState(C)
    Xc = rng.uniform(size=(C, d))
    rows = rng.randint(0, H * S, size=C)
    rows[0] = H * S - 1
    _ffi.check(lib.bocf_set_candidates(ctx.handle, _ffi.dptr(_ffi.f64(Xc)), C), "bocf_set_candidates")
    paths = [PR.Paths(refs[g], Yg, *draws[g]) for g in range(H)]
    minl = min(float(np.min(o.lengthscale)) for r in refs for o in r.output)
    vtol, gtol = 1e-10 * var.max(), 1e-10 * var.max() / minl

    def want(util, th):
        v, g = np.empty(C), np.empty((C, d))
        for i in range(C):
            gi, s = divmod(int(rows[i]), S)
            vi, di = paths[gi].utility(Xc[i:i + 1], [s], {s: th[rows[i]]}, util, grad=True)
            v[i], g[i] = vi[0], di[0]
        return v, g
    for j in range(m):
        th = np.zeros((H * S, m))
        th[:, j] = 1.0
        rc, val, grad = _path_utility(ctx.handle, _ffi.UTIL_LINEAR, th, H * S, rows, C, d)
        assert rc == 0, lib.bocf_last_error()
        wv, wg = want("linear", th)
        print("path_utility linear e_%d C %d" % (j, C), np.max(np.abs(val - wv)), np.max(np.abs(grad - wg)), "gates", vtol, gtol)
        np.testing.assert_allclose(val, wv, rtol=0, atol=vtol)
        np.testing.assert_allclose(grad, wg, rtol=0, atol=gtol)
    th = rng.normal(size=(H * S, m))
    rc, val, grad = _path_utility(ctx.handle, _ffi.UTIL_NEG_SQ_DIST, th, H * S, rows, C, d)
    assert rc == 0, lib.bocf_last_error()
    wv, wg = want("neg_sq_dist", th)
    # U = -sum (y - theta)^2: dU/dy = -2 (y - theta) scales the error of y and of dy/dx by 2 |y - theta|, summed over the m outputs
    amp = 2.0 * m * max(1.0, float(np.max(np.abs(th))) + 3.0)
    np.testing.assert_allclose(val, wv, rtol=0, atol=vtol * amp)
    np.testing.assert_allclose(grad, wg, rtol=0, atol=gtol * amp)
    rc, val2, _ = _path_utility(ctx.handle, _ffi.UTIL_NEG_SQ_DIST, th, H * S, rows, C, d, grad=False)
    assert rc == 0
    np.testing.assert_array_equal(val2, val)


@pytest.mark.parametrize("kinds", [("rbf", "matern52"), ("se", "matern32")])
def test_path_utility_every_family(kinds):
    model, ref, var, lss, X, Y = _setup(kinds, 150, 3, 21)
    S, C, d, m = 4, 17, 3, 2
    draws = PR.draw(kinds, 150, d, 130, S, np.random.RandomState(2))
    h = model._context().handle
    _stage(h, draws)
    Xc = np.random.RandomState(4).uniform(size=(C, d))
    rows = np.arange(C) % S
    model._set_candidates(Xc)
    P = PR.Paths(ref, Y, *draws)
    minl = min(float(np.min(l)) for l in lss)
    for j in range(m):
        th = np.zeros((S, m))
        th[:, j] = 1.0
        rc, val, grad = _path_utility(h, _ffi.UTIL_LINEAR, th, S, rows, C, d)
        assert rc == 0, _ffi.load().bocf_last_error()
        wv, wg = P.utility(Xc, rows, th, "linear", grad=True)
        np.testing.assert_allclose(val, wv, rtol=0, atol=1e-10 * var.max())
        np.testing.assert_allclose(grad, wg, rtol=0, atol=1e-10 * var.max() / minl)
    # the traced program's value+gradient section through the same chain rule
    th = np.random.RandomState(5).normal(size=(S, m))
    U = B.Utility(func=_abs15, parameter_dist=B.ParameterDistribution(support=th, prob_dist=np.full(S, 1.0 / S)), device="program")
    kind = U.device_kind(m)                                        # (traces the callable: the blob exists from here on)
    model.set_utility_program(U.program_blob)
    rc, val, grad = _path_utility(h, kind, th, S, rows, C, d)
    assert rc == 0, _ffi.load().bocf_last_error()
    Fv, G = P.values(Xc), P.gradients(Xc)
    for i in range(C):
        y = Fv[:, i, rows[i]]
        dy = -1.5 * np.sign(y - th[rows[i]]) * np.abs(y - th[rows[i]]) ** 0.5
        np.testing.assert_allclose(val[i], _abs15(th[rows[i]], y), rtol=0, atol=1e-9)
        np.testing.assert_allclose(grad[i], dy.dot(G[:, i, rows[i], :]), rtol=0, atol=1e-8)


# ---- 5. lifetime
def test_lifetime():
    kinds = ("rbf", "matern52")
    N, d, S, F, C = 100, 2, 5, 130, 70
    X, Y, var, lss = _data(kinds, N + 1, d, 33)
    m = len(kinds)
    model = B.multi_outputGP(m, kernel=[KINDS[kinds[j]](d, variance=var[j], lengthscale=lss[j], ARD=True) for j in range(m)], noise_var=[1e-2] * m,
                             fixed_hyps=True)
    model.updateModel(X[:N], [y[:N] for y in Y])
    lib, h = _ffi.load(), model._context().handle
    draws = PR.draw(kinds, N, d, F, S, np.random.RandomState(1))
    Xc = np.random.RandomState(2).uniform(size=(C, d))
    # the acquisition vector and its selection before a path call are what they are after it
    thetas = np.random.RandomState(3).normal(size=(2, m))
    acq0 = model.acq_linear(Xc, _ffi.ACQ_EI, thetas, None)
    sel0 = model.select_topk(5)
    _stage(h, draws)
    v0 = _values(h, m, C, S)
    rc, _, _ = _path_utility(h, _ffi.UTIL_LINEAR, np.ones((S, m)), S, np.zeros(C, dtype=int), C, d)
    assert rc == 0
    sel1 = model.select_topk(5)
    np.testing.assert_array_equal(sel0[0], sel1[0])
    np.testing.assert_array_equal(sel0[1], sel1[1])
    np.testing.assert_array_equal(model.acq_linear(Xc, _ffi.ACQ_EI, thetas, None), acq0)
    # paths survive a candidate upload
    model._set_candidates(Xc[:10])
    np.testing.assert_array_equal(_values(h, m, 10, S), v0[:, :10])
    # ... and are dropped by new targets, an appended observation and a fit
    out = np.empty((m, 10, S))

    def gone():
        assert lib.bocf_path_values(h, -1, _ffi.dptr(out)) < 0
        assert b"bocf_path_values" in lib.bocf_last_error() and b"no paths are resident" in lib.bocf_last_error()
        rc, _, _ = _path_utility(h, _ffi.UTIL_LINEAR, np.ones((S, m)), S, np.zeros(10, dtype=int), 10, d)
        assert rc < 0 and b"no paths are resident" in lib.bocf_last_error()
    model.updateModel(X[:N], [y[:N] + 0.1 for y in Y])             # bocf_update_targets
    model._set_candidates(Xc[:10])
    gone()
    _stage(h, draws)
    model.updateModel(X, Y)                                        # bocf_append
    model._set_candidates(Xc[:10])
    gone()
    # re-staged after the append: the restatement on N + 1 points
    draws1 = PR.draw(kinds, N + 1, d, F, S, np.random.RandomState(4))
    _stage(h, draws1)
    ref = R.MultiOutputGPRef(list(kinds), var, lss, [1e-2] * m)
    ref.updateModel(X, Y)
    np.testing.assert_allclose(_values(h, m, 10, S), PR.Paths(ref, Y, *draws1).values(Xc[:10]), rtol=0, atol=1e-10 * var.max())
    model._fit()                                                   # bocf_fit
    model._set_candidates(Xc[:10])
    gone()
    assert model._resident.paths is None


# ---- 6. refusals
def test_refusals_name_the_entry_point_and_leave_the_context_usable():
    lib = _ffi.load()
    kinds = ("rbf",)
    model, ref, var, lss, X, Y = _setup(kinds, 60, 2, 1)
    h = model._context().handle
    S, F, C = 3, 20, 12
    draws = PR.draw(kinds, 60, 2, F, S, np.random.RandomState(0))
    om, ph, w, E = [_ffi.f64(a) for a in draws]
    Xc = np.random.RandomState(1).uniform(size=(C, 2))
    model._set_candidates(Xc)
    want = PR.Paths(ref, Y, *draws).values(Xc)

    def ok():
        _stage(h, draws)
        np.testing.assert_allclose(_values(h, 1, C, S), want, rtol=0, atol=1e-10 * var.max())
    big = np.zeros((1, 60, 65))
    assert lib.bocf_set_paths(h, -1, _ffi.dptr(om), _ffi.dptr(ph), _ffi.dptr(np.zeros((1, F, 65))), _ffi.dptr(big), F, 65) < 0      # S = 65
    assert b"bocf_set_paths" in lib.bocf_last_error()
    ok()
    assert lib.bocf_set_paths(h, -1, _ffi.dptr(om), _ffi.dptr(ph), _ffi.dptr(w), _ffi.dptr(E), 0, S) < 0                              # F = 0
    assert b"bocf_set_paths" in lib.bocf_last_error()
    ok()
    fresh = _ffi.Context(0)                                                                                                          # unfitted
    assert lib.bocf_set_paths(fresh.handle, -1, _ffi.dptr(om), _ffi.dptr(ph), _ffi.dptr(w), _ffi.dptr(E), F, S) < 0
    assert b"bocf_set_paths" in lib.bocf_last_error() and b"not fitted" in lib.bocf_last_error()
    assert lib.bocf_path_values(fresh.handle, -1, None) < 0
    assert b"bocf_path_values" in lib.bocf_last_error()
    ok()
    canned = _ffi.Context(0)                                                                                                         # bocf_set_posterior
    mean, vv, mt = np.zeros((1, 4)), np.ones((1, 4)), np.zeros((1, 3))
    _ffi.check(lib.bocf_set_posterior(canned.handle, 1, 4, 3, _ffi.dptr(mean), _ffi.dptr(vv), _ffi.dptr(mt)), "bocf_set_posterior")
    assert lib.bocf_set_paths(canned.handle, -1, _ffi.dptr(om), _ffi.dptr(ph), _ffi.dptr(w), _ffi.dptr(E), F, S) < 0
    assert b"bocf_set_paths" in lib.bocf_last_error() and b"host-given posterior" in lib.bocf_last_error()
    ok()
    th = np.ones((S, 1))
    rows = np.zeros(C, dtype=int)
    rows[5] = S                                                                                                                      # row_path out of range
    rc, _, _ = _path_utility(h, _ffi.UTIL_LINEAR, th, S, rows, C, 2)
    assert rc < 0 and b"bocf_path_utility" in lib.bocf_last_error() and b"row_path" in lib.bocf_last_error()
    rows[5] = -1
    rc, _, _ = _path_utility(h, _ffi.UTIL_LINEAR, th, S, rows, C, 2)
    assert rc < 0 and b"row_path" in lib.bocf_last_error()
    rows[5] = S - 1
    rc, _, _ = _path_utility(h, _ffi.UTIL_LINEAR, np.ones((S + 1, 1)), S + 1, rows, C, 2)                                             # P not the resident paths
    assert rc < 0 and b"bocf_path_utility" in lib.bocf_last_error() and b"P does not match" in lib.bocf_last_error()
    rc, val, grad = _path_utility(h, _ffi.UTIL_LINEAR, th, S, rows, C, 2)
    assert rc == 0
    np.testing.assert_allclose(val, want[0, np.arange(C), rows], rtol=0, atol=1e-10 * var.max())
    ok()
    _ffi.check(lib.bocf_set_paths(h, -1, None, None, None, None, F, 0), "bocf_set_paths")                                             # S = 0 drops
    assert lib.bocf_path_values(h, -1, None) < 0 and b"no paths are resident" in lib.bocf_last_error()
    ok()


# ---- 7. end to end
def test_cbo_with_pathwise_thompson_batches():
    np.random.seed(21)
    d, m, q = 2, 2, 4
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m,
                             fixed_hyps=True)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9]]), prob_dist=np.array([0.5, 0.5])),
                  device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=100, n_anchor=4)
    acq = B.uEI_noiseless(model, space, optimizer=opt, utility=U)
    X0 = np.random.uniform(size=(5, d))
    records = []

    class Recording(B.CompositePathwiseThompsonBatch):
        def compute_batch(self, *a, **kw):
            out = B.CompositePathwiseThompsonBatch.compute_batch(self, *a, **kw)
            records.append(self.last_refinement)
            return out
    ev = Recording(acq, q, n_candidates=2048, n_features=256)
    bo = B.CBO(model, space, objective, acq, ev, X0)
    bo.run_optimization(max_iter=3)
    assert bo.X.shape == (5 + 3 * q, d)
    assert np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)
    assert len(records) == 3
    for it in range(3):
        rows = bo.X[5 + q * it:5 + q * (it + 1)]
        assert len({tuple(r) for r in rows}) == q
        rec = records[it]
        for s in range(q - 1):
            if rec["kept"][s]:
                np.testing.assert_array_equal(rows[1 + s], rec["refined"][s])
                assert rec["refined_values"][s] >= rec["pick_values"][s]
            else:
                np.testing.assert_array_equal(rows[1 + s], rec["picks"][s])
