"""Incremental updates of the resident model -- bocf_append (bordered factor: two GEMVs + append_write_kernel) and bocf_update_targets --
against the NumPy oracle refitted from scratch and, where conditioning matters, against the long-double truth (oracle/truth.py).

Every later predict, gradient, acquisition, KG, pending and Thompson call of a BO run reads the state these two calls leave behind, so
the cases walk the places where it can go wrong without a refit noticing: the tile / grid boundaries of append_write_kernel (N = 129 ...
640, first and last row of a 128-tile, second block of the grid), the padding each factorization schedule leaves behind, buffers a larger
earlier fit wrote, the reduced-precision copies of R, the Ky^-1 an inference caches (C ABI), a chain of 127 bordered updates, target
edge cases, every refusal of bocf_append and the resident candidate / KG / pending state.

A refused append turns into a refit inside multi_outputGP.updateModel, so every test that means to exercise the append counts the
_fit calls (as test_gpu_parity.test_incremental_update does) and asserts the exact number.  The inputs are ones the oracle factorizes
with zero jitter (asserted on both sides).

Tolerances against the oracle are those of test_incremental_update: mean rtol 1e-6 / atol 1e-7, |dvar| <= 1e-9, log-marginal rtol 1e-9,
L rtol 1e-6 / atol 1e-9, input gradients rtol 1e-5 / atol 1e-6 and rtol 1e-4 / atol 1e-8, hyper-gradients rtol 1e-6 (lengthscales atol 1e-8).
They were set on a problem with cond(Ky) <= N sigma_f^2 / noise ~ 1e6; `problem` below keeps cond(Ky) in that range at noise 1e-6 too
by tying the lengthscales to the point spacing (every point keeps a handful of correlated neighbours, K stays far from low rank).
alpha (not looked at by test_incremental_update): rtol 1e-6 with the absolute floor 1e-6 max|alpha| -- both sides solve Ky alpha = yc in
fp64, normwise error eps cond(Ky) max|alpha| <= 2.2e-16 x 1e7 max|alpha|.
The log-marginal's rtol 1e-9 has no absolute floor, so the inputs are also ones whose log-marginal does not cancel (lml_cancellation,
asserted): its three terms are each ~ 1e2 .. 1e3 with roundings ~ 1e-8, which a sum that lands near zero would turn into any relative error."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_ref as K  # noqa: E402
import pending_ref as PR  # noqa: E402

from oracle import cpu_ref as R  # noqa: E402
from oracle import truth as T  # noqa: E402

pytestmark = pytest.mark.gpu

MIXED5 = ["matern52", "rbf", "matern32", "se", "rbf"]
TILE = 128


@pytest.fixture(scope="module")
def B():
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


# ---------------------------------------------------------------------------------------------------------------------------------
# problems, models, the oracle
def design(n, d, rng):
    """n points in the unit box; d = 1: a jittered grid in random order (no two points closer than 0.4 / n: uniform draws in one
    dimension have pairs ~ 1 / n^2 apart, which a noise of 1e-6 does not keep apart at the tolerances above)."""
    if d == 1:
        return ((rng.permutation(n) + 0.5 + 0.3 * rng.uniform(-1, 1, size=n)) / n)[:, None]
    return rng.uniform(size=(n, d))


def problem(n, d, m, noise, seed, C=40):
    """n observations of m smooth outputs, ARD lengthscales 1.5 (d = 1: 1.2) x the mean point spacing n^(-1/d) (+- 20 % per dimension
    and output), variances in [0.8, 1.25], C candidates in the box."""
    rng = np.random.RandomState(seed)
    X = design(n, d, rng)
    h = n ** (-1.0 / d)
    ls = [(1.2 if d == 1 else 1.5) * h * (1.0 + 0.2 * rng.uniform(-1, 1, size=d)) for _ in range(m)]
    variances = list(rng.uniform(0.8, 1.25, size=m))
    Y = []
    for _ in range(m):
        a, b = rng.normal(size=d), rng.normal(size=d)
        Y.append((np.sin(2 * np.pi * X.dot(a)) + 0.5 * np.cos(3 * X.dot(b)))[:, None])
    return dict(X=X, Y=Y, lengthscales=ls, variances=variances, noise=[float(noise)] * m, Xc=rng.uniform(size=(C, d)))


def kinds_of(kind, m):
    if kind == "mixed":
        assert m == len(MIXED5)
        return list(MIXED5)
    return [kind] * m


def device_model(B, kinds, p, n=None, options=()):
    """The device model of problem p (one kernel family per output); fitted on the first n observations when n is given."""
    d = p["X"].shape[1]
    cls = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
    kern = [cls[k](d, variance=p["variances"][j], lengthscale=p["lengthscales"][j], ARD=np.size(p["lengthscales"][j]) > 1)
            for j, k in enumerate(kinds)]
    model = B.multi_outputGP(len(kinds), kernel=kern, noise_var=list(p["noise"]), fixed_hyps=True)
    for name, value in options:
        model.set_option(name, value)
    if n is not None:
        model.updateModel(p["X"][:n], [y[:n] for y in p["Y"]])
    return model


def count_fits(model):
    """Counts the from-scratch fits from here on: a refused bocf_append becomes one."""
    calls = {"fit": 0}
    orig_fit = model._fit

    def counting_fit():
        calls["fit"] += 1
        orig_fit()
    model._fit = counting_fit
    return calls


def oracle(kinds, p, X, Ys):
    """The oracle fitted from scratch; no output may need jitter."""
    ref = R.MultiOutputGPRef(kinds, p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(X, Ys)
    assert all(o.jitter == 0 for o in ref.output), "the oracle needs jitter on these inputs: choose others"
    return ref


def lml_cancellation(ref):
    """Smallest |log-marginal| / (sum of the sizes of its three terms) over the outputs of an oracle fit.  The log-marginal is
    -(N/2) log 2 pi - sum log diag L - yc^T alpha / 2; each term carries its own fp64 rounding (~ eps cond(Ky) of its size), so a RELATIVE
    tolerance on their sum is a statement about the factorization only while the sum does not cancel."""
    out = []
    for o in ref.output:
        n = o.L.shape[0]
        terms = [0.5 * n * np.log(2 * np.pi), float(np.sum(np.log(np.diag(o.L))))]
        terms.append(-float(o.log_marginal) - terms[0] - terms[1])
        out.append(abs(float(o.log_marginal)) / sum(abs(t) for t in terms))
    return min(out)


def update(model, p, n, Ys=None):
    model.updateModel(p["X"][:n], [y[:n] for y in (p["Y"] if Ys is None else Ys)])


def check(model, ref, Xc, factor_outputs=None):
    """Everything a later call reads, against the oracle refitted from scratch, at the tolerances of test_incremental_update."""
    m = model.output_dim
    assert np.all(np.asarray(model.jitter) == 0)
    assert lml_cancellation(ref) > 0.05, "a log-marginal of these inputs cancels to < 5 % of its terms: rtol 1e-9 is not about the fit, choose others"
    rm, rv = ref.predict(Xc)
    assert Xc.shape[0] > 16
    for sl in (slice(None), slice(0, 5)):                  # > 16 candidates: the GEMM path; 5: the small MFMA path, which reads RT
        mean, var = model.predict(Xc[sl])
        np.testing.assert_allclose(mean, rm[:, sl], rtol=1e-6, atol=1e-7)
        assert np.abs(var - rv[:, sl]).max() <= 1e-9, np.abs(var - rv[:, sl]).max()
    dm, dv = model.posterior_mean_gradient(Xc[:5]), model.posterior_variance_gradient(Xc[:5])
    np.testing.assert_allclose(dm, ref.posterior_mean_gradient(Xc[:5]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dv, ref.posterior_variance_gradient(Xc[:5]), rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(model.posterior_mean_at_evaluated_points(), ref.posterior_mean_at_evaluated_points(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(model.log_marginal, [o.log_marginal for o in ref.output], rtol=1e-9)
    for j in sorted({0, m - 1} if factor_outputs is None else set(factor_outputs)):
        L, alpha = model.get_factor(j)
        np.testing.assert_allclose(L, ref.output[j].L, rtol=1e-6, atol=1e-9)
        ra = ref.output[j].alpha[:, 0]
        np.testing.assert_allclose(alpha, ra, rtol=1e-6, atol=1e-6 * np.abs(ra).max())
    dvh, dlh, dnh = model.log_likelihood_gradients()
    for j in range(m):
        rvh, rlh, rnh = ref.output[j].lml_gradients()
        np.testing.assert_allclose([dvh[j], dnh[j]], [rvh, rnh], rtol=1e-6)
        np.testing.assert_allclose(dlh[j], rlh, rtol=1e-6, atol=1e-8)


def check_n(model, kinds, p, n, Ys=None):
    Yn = [y[:n] for y in (p["Y"] if Ys is None else Ys)]
    check(model, oracle(kinds, p, p["X"][:n], Yn), p["Xc"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. tile and grid boundaries of the append against a from-scratch fit.  N: last row of the first tile's successor (129), last row of
# a tile (255, 383, 511: the append fills the padding), a full padding (256, 384, 640: no row left, the append is refused and the
# model refits exactly once), first row of a new tile + second block of the 256-wide grid (257, 385).  m, d, kernel family and noise
# cover {1, 5} x {1, 7}, the four families / one mixed list and {1e-4, 1e-6} over the table.
SINGLE = [
    (129, 1, 1, "rbf", 1e-4), (129, 5, 7, "mixed", 1e-6),
    (255, 5, 1, "matern32", 1e-6), (255, 1, 7, "matern52", 1e-4),
    (256, 1, 7, "rbf", 1e-6), (256, 5, 1, "matern52", 1e-4),
    (257, 5, 7, "matern32", 1e-4), (257, 1, 1, "matern52", 1e-6),
    (383, 1, 1, "matern32", 1e-6), (383, 5, 7, "rbf", 1e-4),
    (384, 5, 1, "mixed", 1e-4), (384, 1, 7, "matern32", 1e-6),
    (385, 1, 7, "rbf", 1e-4), (385, 5, 1, "rbf", 1e-6),
    (511, 5, 7, "matern52", 1e-6), (511, 1, 1, "rbf", 1e-4),
    (640, 1, 7, "matern52", 1e-4), (640, 5, 1, "mixed", 1e-6),
]


# seeds: base + 1000 k with the first k at which no log-marginal of the N + 1-point problem cancels (lml_cancellation; found on the CPU,
# asserted by check)
SEED_SHIFT = {(384, 5): 2000, (640, 5): 1000}


def seed_single(N, m):
    return 100 + N + m + SEED_SHIFT.get((N, m), 0)


@pytest.mark.parametrize("N,m,d,kind,noise", SINGLE, ids=["N%d-m%d-d%d-%s-%g" % c for c in SINGLE])
def test_append_at_tile_and_grid_boundaries(B, N, m, d, kind, noise):
    kinds = kinds_of(kind, m)
    p = problem(N + 1, d, m, noise, seed_single(N, m))
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    update(model, p, N + 1)
    assert calls["fit"] == (1 if N % TILE == 0 else 0)     # a full padding (Np = N) is the one refusal here
    check_n(model, kinds, p, N + 1)


RUNS = [(254, 5, 7, "mixed", 1e-4), (382, 1, 1, "rbf", 1e-6), (510, 5, 1, "matern52", 1e-6)]


@pytest.mark.parametrize("N,m,d,kind,noise", RUNS, ids=["N%d-m%d-d%d-%s-%g" % c for c in RUNS])
def test_append_run_fills_the_padding_then_refits(B, N, m, d, kind, noise):
    kinds = kinds_of(kind, m)
    p = problem(N + 3, d, m, noise, 200 + N)
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    for n in (N + 1, N + 2):                               # N + 2 is a multiple of 128: the last padding row
        update(model, p, n)
        assert calls["fit"] == 0
        check_n(model, kinds, p, n)
    update(model, p, N + 3)                                # no row left: refused, one refit
    assert calls["fit"] == 1
    check_n(model, kinds, p, N + 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the append reads R over all Np rows, so it depends on the padding the fit left behind: behind the launched schedule (team_fit = 0)
# and the default one (one team launch), and on a context whose earlier, larger fit wrote the rows the append now reads as padding
@pytest.mark.parametrize("N", [300, 1100])
@pytest.mark.parametrize("team_fit,schedule", [(0, 0), (-1, 3)], ids=["launched", "default"])
def test_append_behind_each_schedule(B, N, team_fit, schedule):
    m, d = 2, 3
    kinds = ["matern52", "rbf"]
    p = problem(N + 1, d, m, 1e-4, {300: 1600, 1100: 1400}[N])         # (seeds: as SEED_SHIFT)
    model = device_model(B, kinds, p, N, options=[("team_fit", team_fit)])
    assert model._context().stat("last_schedule") == schedule
    calls = count_fits(model)
    update(model, p, N + 1)
    assert calls["fit"] == 0
    assert model._context().stat("last_schedule") == schedule       # (no factorization since)
    check_n(model, kinds, p, N + 1)


@pytest.mark.parametrize("N_big,N_small", [(380, 260), (300, 140)], ids=["same-Np", "smaller-Np"])
def test_append_on_buffers_of_a_larger_earlier_fit(B, N_big, N_small):
    """Fit N_big, refit N_small < N_big with another history (380 -> 260: the same Np = 384, rows 260 .. 379 of every buffer held the
    first fit's numbers; 300 -> 140: a smaller Np inside the larger allocation), then append twice: nothing stale may leak."""
    m, d = 2, 4
    kinds = ["rbf", "matern32"]
    big = problem(N_big, d, m, 1e-4, 400 + N_big)
    p = problem(N_small + 2, d, m, 1e-4, 500 + N_small)
    for key in ("lengthscales", "variances"):              # same hyper-parameters: only the history changes
        p[key] = big[key]
    model = device_model(B, kinds, big, N_big)
    calls = count_fits(model)
    update(model, p, N_small)
    assert calls["fit"] == 1
    for n in (N_small + 1, N_small + 2):
        update(model, p, n)
        assert calls["fit"] == 1
        check_n(model, kinds, p, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the reduced-precision copies of R (options predict_f32, predict_i8) are rebuilt after an append.  The new observation sits ON a
# candidate with a target 5 away from the prior mean: were the copy of the N-point factor still in use, the answer would be the
# N-point posterior, which differs from the N + 1-point one by far more than the tolerance (asserted on the oracle).
# Tolerances: the option's own against fp64 (|dvar| <= 2e-5 for fp32, test_gpu_parity.test_predict_f32; 1e-9 max sigma_f^2 for int8,
# test_gpu_round4.test_int8_variance_contraction_against_fp64) plus the append's 1e-9 against the oracle; means do not go through the
# contraction (fp64 tolerances).
@pytest.mark.parametrize("option,kind,tol", [("predict_f32", "matern32", 2e-5), ("predict_i8", "rbf", 1e-9)])
def test_reduced_precision_copies_follow_an_append(B, option, kind, tol):
    N, m, d, C = 300, 2, 3, 64
    kinds = [kind] * m
    p = problem(N + 1, d, m, 1e-4, 600, C=C)
    tol = tol * max(1.0, max(p["variances"])) + 1e-9
    ref0 = oracle(kinds, p, p["X"][:N], [y[:N] for y in p["Y"]])
    p["X"][N] = p["Xc"][int(np.argmax(ref0.predict(p["Xc"])[1].min(0)))]       # the candidate the N-point model knows least about
    p["Y"] = [np.vstack([y[:N], [[float(y[:N].mean()) + 5.0]]]) for y in p["Y"]]
    ref1 = oracle(kinds, p, p["X"], p["Y"])
    (rm0, rv0), (rm1, rv1) = ref0.predict(p["Xc"]), ref1.predict(p["Xc"])
    assert np.abs(rv0 - rv1).max() > 1e3 * tol and np.abs(rm0 - rm1).max() > 1.0
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    v64 = model.predict(p["Xc"])[1]
    model.set_option(option, 1)
    mean0, var0 = model.predict(p["Xc"])                   # builds the copy of the N-point factor
    assert not np.array_equal(var0, v64), "the %s contraction did not run" % option
    np.testing.assert_allclose(mean0, rm0, rtol=1e-6, atol=1e-7)
    assert np.abs(var0 - rv0).max() <= tol
    update(model, p, N + 1)
    assert calls["fit"] == 0 and np.all(model.jitter == 0)
    mean1, var1 = model.predict(p["Xc"])
    np.testing.assert_allclose(mean1, rm1, rtol=1e-6, atol=1e-7)
    print("%s after an append: max |dvar| %.3e against the N + 1 oracle (bound %.3e), %.3e against the N-point one"
          % (option, np.abs(var1 - rv1).max(), tol, np.abs(var1 - rv0).max()))
    assert np.abs(var1 - rv1).max() <= tol
    fresh = device_model(B, kinds, p, options=[(option, 1)])
    update(fresh, p, N + 1)
    meanf, varf = fresh.predict(p["Xc"])
    np.testing.assert_allclose(mean1, meanf, rtol=1e-6, atol=1e-7)
    assert np.abs(var1 - varf).max() <= tol


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. Ky^-1 across an incremental update, at the C ABI on a raw context.  bocf_infer beyond one tile fits with "Ky^-1 wanted"; the
# one-team-launch schedule (2 .. 24 panels) leaves it in the T scratch for bocf_lml_gradients.  An append changes Ky: the cached
# inverse must be dropped.  New targets do not change Ky: it may stay.
def _abi_problem(B, kind, n):
    F = B._ffi
    p = problem(n, 3, 2, 1e-4, 700 + n)
    X = F.f64(p["X"])
    Y = F.f64(np.stack([y[:, 0] for y in p["Y"]]))
    return p, X, Y, F.f64(p["variances"]), F.f64(np.stack(p["lengthscales"])), F.f64(p["noise"])


def _abi_infer(B, ctx, kind, X, Y, var, ls, noise):
    """bocf_infer on the raw context: (lml, dvariance, dlengthscale, dnoise); zero jitter and the team-whole schedule asserted."""
    F = B._ffi
    kid = {"rbf": F.KERN_RBF, "matern52": F.KERN_MATERN52}[kind]
    m, N = Y.shape
    d = X.shape[1]
    jit, lml, dv, dl, dn = np.ones(m), np.zeros(m), np.zeros(m), np.zeros((m, d)), np.zeros(m)
    rc = F.load().bocf_infer(ctx.handle, F.dptr(X), F.dptr(Y), N, d, m, kid, F.dptr(var), F.dptr(ls), F.dptr(noise), 5, F.dptr(jit), F.dptr(lml),
                             F.dptr(dv), F.dptr(dl), F.dptr(dn))
    assert F.check(rc, "bocf_infer") == 0 and np.all(jit == 0)
    assert ctx.stat("last_schedule") == 3, "not the one-team-launch schedule: the case does not exercise the cached inverse"
    return lml, dv, dl, dn


def _abi_gradients(B, ctx, m, d):
    F = B._ffi
    dv, dl, dn = np.full(m, np.nan), np.full((m, d), np.nan), np.full(m, np.nan)
    F.check(F.load().bocf_lml_gradients(ctx.handle, F.dptr(dv), F.dptr(dl), F.dptr(dn)), "bocf_lml_gradients")
    return dv, dl, dn


def _check_hyper_gradients(kind, p, X, Y, got_lml, got):
    """Against the oracle on (X, Y), at the tolerances of test_hyper_gradients_multi_tile."""
    dv, dl, dn = got
    for j in range(Y.shape[0]):
        fit = R.GPFit(kind, X, Y[j][:, None], p["variances"][j], p["lengthscales"][j], p["noise"][j])
        assert fit.jitter == 0
        rv, rl, rn = fit.lml_gradients()
        print("output %d: d/dvariance %.9g (oracle %.9g)  d/dnoise %.9g (oracle %.9g)" % (j, dv[j], rv, dn[j], rn))
        np.testing.assert_allclose(got_lml[j], fit.log_marginal, rtol=1e-9)
        np.testing.assert_allclose(dv[j], rv, rtol=1e-6)
        np.testing.assert_allclose(dl[j], rl, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(dn[j], rn, rtol=1e-6)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("N", [200, 600, 640])
def test_cached_inverse_is_dropped_by_an_append(B, kind, N):
    """bocf_infer -> bocf_append -> bocf_lml_gradients == the oracle on N + 1 points.  N = 200: two panels; 600: five panels, the third
    block of the append's grid.  N = 640 = Np has no padding row: the append is refused (1), the N-point model and its cached inverse
    stay valid and the gradients are still those of N points.
    Fails without the invalidation in bocf_append: the gradients are taken with the inverse of the N-point matrix.  Recorded on the
    library of the commit before the fix (one MI355X), d/dvariance and d/dnoise of output 0 (the first one compared), device (oracle): N = 200 rbf 871.969 (872.215), 401582.7
    (398879.8); 200 matern52 51.5785 (51.5308), -1687.95 (-1743.05); 600 rbf -248.576 (-248.376), -623149 (-625387); 600 matern52
    -317.171 (-317.211), -14673.5 (-14697.3) -- relative errors 1e-4 .. 3e-2 against the rtol of 1e-6; N = 640 and the new-targets
    cases passed before and after."""
    F = B._ffi
    lib = F.load()
    ctx = F.Context(0)
    p, X, Y, var, ls, noise = _abi_problem(B, kind, N + 1)
    X0, Y0 = F.f64(X[:N]), F.f64(Y[:, :N])
    lml0, dv0, dl0, dn0 = _abi_infer(B, ctx, kind, X0, Y0, var, ls, noise)
    _check_hyper_gradients(kind, p, X0, Y0, lml0, (dv0, dl0, dn0))
    lml = np.full(2, np.nan)
    rc = lib.bocf_append(ctx.handle, F.dptr(F.f64(X[N])), F.dptr(Y), F.dptr(lml))
    if N % TILE == 0:
        assert rc == 1
        _check_hyper_gradients(kind, p, X0, Y0, lml0, _abi_gradients(B, ctx, 2, 3))
        return
    assert rc == 0
    assert ctx.stat("last_schedule") == 3
    _check_hyper_gradients(kind, p, X, Y, lml, _abi_gradients(B, ctx, 2, 3))


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
@pytest.mark.parametrize("N", [200, 640])
def test_cached_inverse_survives_new_targets(B, kind, N):
    """bocf_infer -> bocf_update_targets (scaled and shifted Y) -> bocf_lml_gradients == the oracle with the new Y: Ky^-1 does not
    depend on the targets, the cached inverse is kept where it is still valid."""
    F = B._ffi
    ctx = F.Context(0)
    p, X, Y, var, ls, noise = _abi_problem(B, kind, N)
    _abi_infer(B, ctx, kind, X, Y, var, ls, noise)
    Y2 = F.f64(Y * np.array([[1.5], [-0.7]]) + np.array([[-0.3], [2.0]]))
    lml = np.full(2, np.nan)
    assert F.load().bocf_update_targets(ctx.handle, F.dptr(Y2), F.dptr(lml)) == 0
    _check_hyper_gradients(kind, p, X, Y2, lml, _abi_gradients(B, ctx, 2, 3))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5, 6. against the long-double truth.  The gate is the one of test_gpu_round3: err_device <= max(1e-5 scale, 4 err_oracle), both
# errors against oracle/truth_ld.c; the oracle is the NumPy one refitted from scratch.  scale: means -> the largest |truth - c|, c = 0
# (round 3's rule) or, where the targets carry a large common offset, the target mean of the output (the device and the oracle both work
# on centred targets: adding the offset back costs one rounding, 1e6 eps = 2e-10; measured against |mean| ~ 1e6 the gate would allow an
# error of 10); raw variance -> the largest sigma_f^2; log-marginal -> the largest |truth|.
def gate_rows(tag, model, kinds, p, n, Ys=None, centre=None):
    """(all ok, printable rows) of the four gated quantities of `model` holding the first n observations."""
    Ys = [y[:n] for y in (p["Y"] if Ys is None else Ys)]
    X, Xc, m = p["X"][:n], p["Xc"], len(kinds)
    assert len(set(kinds)) == 1
    ref = oracle(kinds, p, X, Ys)
    tru = T.model_truth(kinds[0], X, Ys, p["variances"], p["lengthscales"], p["noise"], Xc)
    assert tru["raw_var"].min() > 1e-10                    # (the device clips there: above it the clipped variance IS the raw one)
    c = np.zeros((m, 1)) if centre is None else np.asarray(centre, dtype=float).reshape(m, 1)
    raw_orc = np.stack([o.raw_posterior_variance(Xc)[:, 0] for o in ref.output])
    quantities = [("mean", model.posterior_mean(Xc), ref.posterior_mean(Xc), tru["mean"], np.abs(tru["mean"] - c).max()),
                  ("raw variance", model.posterior_variance_noiseless(Xc), raw_orc, tru["raw_var"], max(p["variances"])),
                  ("mean at train", model.posterior_mean_at_evaluated_points(), ref.posterior_mean_at_evaluated_points(), tru["mu_train"],
                   np.abs(tru["mu_train"] - c).max()),
                  ("log-marginal", model.log_marginal, [o.log_marginal for o in ref.output], tru["lml"], np.abs(tru["lml"]).max())]
    ok_all, rows = True, []
    for name, dev, orc, tr, scale in quantities:
        ok, e_dev, e_orc, bound = T.gate(dev, orc, tr, scale)
        rows.append("%-28s %-14s device %.3e   oracle %.3e   bound %.3e%s" % (tag, name, e_dev, e_orc, bound, "" if ok else "   <-- FAILS"))
        ok_all &= ok
    return ok_all, rows


def test_chain_of_appends_against_the_truth(B):
    """N = 129 -> 256 one observation at a time: 127 bordered updates, no refit, at cond(Ky) ~ 1e8 (Matern-5/2, noise 1e-6, lengthscales
    0.9 sqrt(d)); gated at N = 192 and 256, a from-scratch device fit at the same N printed beside it so that drift is visible."""
    m, d = 2, 4
    kinds = ["matern52"] * m
    p = R.synthetic_problem(256, d, m, 60, 4, 5151, noise=1e-6)
    p["lengthscales"] = [1.8 * l for l in p["lengthscales"]]
    Ky = R.kern_K("matern52", p["X"], None, p["variances"][0], p["lengthscales"][0]) + (1e-6 + 1e-8) * np.eye(256)
    cond = np.linalg.cond(Ky)
    print("chain of appends: cond(Ky) = %.3e at N = 256" % cond)
    assert 3e7 < cond < 3e8
    model = device_model(B, kinds, p, 129)
    calls = count_fits(model)
    ok_all, rows = True, []
    for n in range(130, 257):
        update(model, p, n)
        if n in (192, 256):
            ok, r = gate_rows("N = %d, chained from 129" % n, model, kinds, p, n)
            ok2, r2 = gate_rows("N = %d, from scratch" % n, device_model(B, kinds, p, n), kinds, p, n)
            ok_all &= ok and ok2
            rows += r + r2
    print("max abs error against the long-double truth:\n  " + "\n  ".join(rows))
    assert calls["fit"] == 0 and np.all(model.jitter == 0)
    assert ok_all


def _targets_problem():
    return R.synthetic_problem(132, 3, 3, 40, 4, 6161, noise=1e-5)


@pytest.mark.parametrize("edge", ["offset", "scaled", "constant"])
def test_update_targets_edges_against_the_truth(B, edge):
    """bocf_update_targets with targets y + 1e6, 1e-6 y, and one output constant (its centred targets are zero: alpha = 0, the
    posterior mean is the constant)."""
    kinds = ["matern52"] * 3
    p = _targets_problem()
    N = 130
    Ys = {"offset": [y + 1e6 for y in p["Y"]], "scaled": [1e-6 * y for y in p["Y"]],
          "constant": [p["Y"][0], np.full_like(p["Y"][1], 0.7), p["Y"][2]]}[edge]
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    update(model, p, N, Ys)
    assert calls["fit"] == 0 and np.all(model.jitter == 0)
    ok, rows = gate_rows("targets: " + edge, model, kinds, p, N, Ys, centre=[float(y[:N].mean()) for y in Ys])
    print("max abs error against the long-double truth:\n  " + "\n  ".join(rows))
    assert ok


def test_targets_and_appends_interleaved(B):
    """targets -> append -> targets -> append on one model from N = 130, gated after every step, no refit."""
    kinds = ["matern52"] * 3
    p = _targets_problem()
    Ya = [1.5 * y - 0.3 for y in p["Y"]]
    Yb = [0.5 * y + 2.0 for y in p["Y"]]
    model = device_model(B, kinds, p, 130)
    calls = count_fits(model)
    ok_all, rows = True, []
    for step, (n, Ys) in enumerate([(130, Ya), (131, Ya), (131, Yb), (132, Yb)]):
        update(model, p, n, Ys)
        ok, r = gate_rows("step %d (N = %d)" % (step, n), model, kinds, p, n, Ys, centre=[float(y[:n].mean()) for y in Ys])
        ok_all &= ok
        rows += r
    print("max abs error against the long-double truth:\n  " + "\n  ".join(rows))
    assert calls["fit"] == 0 and np.all(model.jitter == 0)
    assert ok_all
    check(model, oracle(kinds, p, p["X"][:132], [y[:132] for y in Yb]), p["Xc"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the refusals of bocf_append and what follows them
def test_append_to_a_jittered_factor_refits(B, probes):
    """One output carries jitter (the diagonal-shift hook of the probes build, as test_gpu_round2.test_failed_outputs_are_reported_per_output):
    the append is refused, updateModel refits exactly once, and the result is that of a from-scratch model bit for bit."""
    rng = np.random.RandomState(4)
    N, d, m = 150, 2, 3
    X = rng.uniform(size=(N + 1, d))
    Y = [rng.normal(size=(N + 1, 1)) for _ in range(m)]
    Xc = rng.uniform(size=(40, d))
    ls = [[0.4, 0.4], [500.0, 500.0], [0.3, 0.5]]          # output 1: K numerically rank one
    noise = [1e-6, 0.0, 1e-6]

    def make():
        model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=np.array(l), ARD=True) for l in ls], noise_var=noise, fixed_hyps=True)
        model.set_option("test_diag_shift_1e12", 20000)     # diag(Ky) -= 2e-8: output 1 (noise 0, diag 1 + 1e-8) loses definiteness
        return model
    model = make()
    model.updateModel(X[:N], [y[:N] for y in Y])
    assert model.jitter[1] > 0 and model.jitter[0] == 0 and model.jitter[2] == 0
    calls = count_fits(model)
    model.updateModel(X, Y)
    assert calls["fit"] == 1
    scratch = make()
    scratch.incremental = False
    scratch.updateModel(X, Y)
    assert scratch.jitter[1] > 0
    np.testing.assert_array_equal(model.jitter, scratch.jitter)
    np.testing.assert_array_equal(model.log_marginal, scratch.log_marginal)
    for a, b in zip(model.predict(Xc), scratch.predict(Xc)):
        np.testing.assert_array_equal(a, b)


def test_incremental_calls_refuse_an_output_sharded_fit(B, probes):
    """At the ABI: behind an output-sharded fit (simulated ranks, a hook of the probes build) bocf_append returns 1 (the caller refits)
    and bocf_update_targets returns its error; the resident model is untouched."""
    F = B._ffi
    lib = F.load()
    ctx = F.Context(0)
    p = problem(151, 3, 4, 1e-4, 808)
    X, Y = F.f64(p["X"][:150]), F.f64(np.stack([y[:150, 0] for y in p["Y"]]))
    Y1 = F.f64(np.stack([y[:, 0] for y in p["Y"]]))
    var, ls, noise = F.f64(p["variances"]), F.f64(np.stack(p["lengthscales"])), F.f64(p["noise"])
    ctx.set_option("shard_fit_simulate", 2)
    ctx.set_option("shard_fit", 1)
    jit, lml = np.ones(4), np.zeros(4)
    assert lib.bocf_fit(ctx.handle, F.dptr(X), F.dptr(Y), 150, 3, 4, F.KERN_MATERN52, F.dptr(var), F.dptr(ls), F.dptr(noise), 5, F.dptr(jit), F.dptr(lml)) == 0
    assert np.all(jit == 0)
    Xc = F.f64(p["Xc"])

    def predict():
        mean, v = np.full((4, len(Xc)), np.nan), np.full((4, len(Xc)), np.nan)
        assert lib.bocf_set_candidates(ctx.handle, F.dptr(Xc), len(Xc)) == 0
        assert lib.bocf_predict(ctx.handle, F.ADD_NOISE | F.CLIP, F.dptr(mean), F.dptr(v)) == 0
        return mean, v
    before = predict()
    out = np.full(4, np.nan)
    assert lib.bocf_append(ctx.handle, F.dptr(F.f64(p["X"][150])), F.dptr(Y1), F.dptr(out)) == 1
    assert lib.bocf_update_targets(ctx.handle, F.dptr(F.f64(2.0 * Y)), F.dptr(out)) < 0
    msg = lib.bocf_last_error()
    assert b"bocf_update_targets" in msg and b"output-sharded" in msg, msg
    assert np.all(np.isnan(out))
    for a, b in zip(before, predict()):
        np.testing.assert_array_equal(a, b)
    ref = oracle(["matern52"] * 4, p, p["X"][:150], [y[:150] for y in p["Y"]])
    np.testing.assert_allclose(before[0], ref.predict(p["Xc"])[0], rtol=1e-6, atol=1e-7)


def _duplicate_problem():
    """A factor that fits with zero jitter (lengthscales of a third of the point spacing: K is close to sigma_f^2 I) at noise 0 and
    sigma_f^2 = 1e6, and an exact duplicate of observation 17 as the new point.  The bordered pivot is
    rho^2 = sigma_f^2 + 1e-8 - ||u||^2 = 1e-8 + (the latent posterior variance at a training point, <= 1e-8): 2e-8 at most, which is
    inside the rounding noise of ||u||^2 ~ sigma_f^2 = 1e6 -- append_write_kernel's threshold 32 eps (N + 1) sigma_f^2 = 9e-7 -- so
    the append must refuse: it cannot tell this pivot from zero."""
    rng = np.random.RandomState(77)
    N, d, m = 130, 3, 2
    X = rng.uniform(size=(N, d))
    X1 = np.vstack([X, X[17:18]])
    f = lambda Z: [np.sin(3 * Z.sum(1))[:, None], np.cos(2 * Z[:, :1]) + Z[:, 1:2]]
    ls = [np.full(d, 0.07), np.full(d, 0.06)]
    return N, d, m, X, f(X), X1, f(X1), [1e6, 1e6], ls, [0.0, 0.0], rng.uniform(size=(20, d))


def test_failed_pivot_at_the_abi_leaves_the_model_unfitted(B):
    F = B._ffi
    lib = F.load()
    ctx = F.Context(0)
    N, d, m, X, Ys, X1, Ys1, var, ls, noise, Xc = _duplicate_problem()
    Xd, Y = F.f64(X), F.f64(np.stack([y[:, 0] for y in Ys]))
    jit, lml = np.ones(m), np.zeros(m)
    rc = lib.bocf_fit(ctx.handle, F.dptr(Xd), F.dptr(Y), N, d, m, F.KERN_MATERN52, F.dptr(F.f64(var)), F.dptr(F.f64(np.stack(ls))), F.dptr(F.f64(noise)),
                      5, F.dptr(jit), F.dptr(lml))
    assert rc == 0 and np.all(jit == 0)
    Xcd = F.f64(Xc)
    assert lib.bocf_set_candidates(ctx.handle, F.dptr(Xcd), len(Xcd)) == 0
    mean, v = np.full((m, len(Xcd)), np.nan), np.full((m, len(Xcd)), np.nan)
    assert lib.bocf_predict(ctx.handle, F.ADD_NOISE | F.CLIP, F.dptr(mean), F.dptr(v)) == 0 and np.all(np.isfinite(mean))
    Y1 = F.f64(np.stack([y[:, 0] for y in Ys1]))
    out = np.full(m, np.nan)
    assert lib.bocf_append(ctx.handle, F.dptr(F.f64(X1[N])), F.dptr(Y1), F.dptr(out)) == 1
    assert np.all(np.isnan(out))
    # some outputs may already be extended: the context is un-fitted, and every reader says so instead of returning numbers
    mean[:], v[:] = np.nan, np.nan
    assert lib.bocf_predict(ctx.handle, F.ADD_NOISE | F.CLIP, F.dptr(mean), F.dptr(v)) < 0
    msg = lib.bocf_last_error()
    assert b"bocf_predict" in msg and b"not fitted" in msg, msg
    assert np.all(np.isnan(mean)) and np.all(np.isnan(v))
    dv, dl, dn = np.full(m, np.nan), np.full((m, d), np.nan), np.full(m, np.nan)
    assert lib.bocf_lml_gradients(ctx.handle, F.dptr(dv), F.dptr(dl), F.dptr(dn)) < 0
    msg = lib.bocf_last_error()
    assert b"bocf_lml_gradients" in msg and b"not fitted" in msg, msg
    assert np.all(np.isnan(dv)) and np.all(np.isnan(dl)) and np.all(np.isnan(dn))
    assert lib.bocf_set_candidates(ctx.handle, F.dptr(Xcd), len(Xcd)) < 0
    assert lib.bocf_update_targets(ctx.handle, F.dptr(Y), F.dptr(out)) < 0
    assert lib.bocf_append(ctx.handle, F.dptr(F.f64(X1[N])), F.dptr(Y1), F.dptr(out)) < 0


def test_failed_pivot_through_the_model_class_refits(B):
    N, d, m, X, Ys, X1, Ys1, var, ls, noise, Xc = _duplicate_problem()

    def make():
        return B.multi_outputGP(m, kernel=[B.kern.Matern52(d, variance=var[j], lengthscale=ls[j], ARD=True) for j in range(m)], noise_var=noise,
                                fixed_hyps=True)
    model = make()
    model.updateModel(X, Ys)
    assert np.all(model.jitter == 0)
    calls = count_fits(model)
    model.updateModel(X1, Ys1)
    assert calls["fit"] == 1
    scratch = make()
    scratch.incremental = False
    scratch.updateModel(X1, Ys1)
    np.testing.assert_array_equal(model.jitter, scratch.jitter)
    np.testing.assert_array_equal(model.log_marginal, scratch.log_marginal)
    for a, b in zip(model.predict(Xc), scratch.predict(Xc)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(model.posterior_mean_at_evaluated_points(), scratch.posterior_mean_at_evaluated_points())


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. what is resident beside the factor: the candidate batch, its acquisition vector, the reference set (uKG) and the pending points
def test_resident_state_across_an_append(B):
    """After a successful append nothing scores the old batch: the selection and the look-ahead acquisitions report their error, the
    Monte-Carlo acquisition sees an EMPTY batch (writes nothing, leaves no acquisition vector to select from).  Re-staged, uKG and
    uEI given pending points equal a fresh model of N + 1 points at the gates of test_gpu_kg / test_gpu_pending (rtol 1e-5, atol 1e-12
    x the size of the terms) and the restatements on N + 1 points."""
    F = B._ffi
    lib = F.load()
    N, d, C, na, r, S = 130, 3, 64, 8, 3, 16
    kinds = ["se", "matern52", "rbf"]
    m = len(kinds)
    p = problem(N + 1, d, m, 1e-4, 23, C=C)                # (lengthscales of the point spacing: the acquisitions are not all zero)
    X, Y, Xc = p["X"], [y[:, 0].copy() for y in p["Y"]], p["Xc"]
    var, ls, nz = np.array(p["variances"]), np.stack(p["lengthscales"]), np.array(p["noise"])
    X[N] = Xc[5]                                           # the new observation: on a candidate, 1 above the target mean
    for j in range(m):
        Y[j][N] = Y[j][:N].mean() + 1.0
    rng = np.random.RandomState(9)
    A, Zf = rng.uniform(size=(na, d)), rng.normal(size=(4, m))
    P, Zp, W = rng.uniform(size=(r, d)), rng.normal(size=(S, m, r)), rng.normal(size=(S, m))
    thetas, prob = rng.uniform(-0.5, 0.5, size=(2, m)), np.array([0.4, 0.6])
    cls = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}

    def make(n):
        model = B.multi_outputGP(m, kernel=[cls[k](d, variance=var[j], lengthscale=ls[j], ARD=True) for j, k in enumerate(kinds)],
                                 noise_var=list(nz), fixed_hyps=True)
        model.updateModel(X[:n], [y[:n, None] for y in Y])
        return model

    def evaluate(model):
        model.set_reference_points(A)
        kg = model.acq_kg(Xc, "closed", F.UTIL_NEG_SQ_DIST, None, thetas, prob, Zf)
        model.set_pending_points(P, Zp, W=W)
        return kg, model.acq_pending(Xc, F.UTIL_NEG_SQ_DIST, None, thetas, prob, W=W)
    model = make(N)
    h = model._context().handle
    kg0, al0 = evaluate(model)
    a0 = model.acq_mc(Xc, F.ACQ_EI, F.UTIL_NEG_SQ_DIST, None, thetas, prob, W=W)
    assert len(model.select_topk(4)[0]) == 4
    calls = count_fits(model)
    model.updateModel(X, [y[:, None] for y in Y])
    assert calls["fit"] == 0 and np.all(model.jitter == 0)
    # ---- no new set_candidates: nothing may score the 64 candidates of the N-point model
    with pytest.raises(F.BocfHipError, match="no acquisition vector"):
        model.select_topk(4)
    th, pr = F.f64(thetas), F.f64(prob)
    out = np.full(C, np.nan)
    rc = lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_NEG_SQ_DIST, None, 0, F.dptr(th), m, F.dptr(pr), 2, F.dptr(out))
    assert rc <= 0 and np.all(np.isnan(out))               # an error, or the empty batch: nothing written ...
    with pytest.raises(F.BocfHipError, match="no acquisition vector"):
        model.select_topk(4)                               # ... and nothing to select from
    assert lib.bocf_acq_kg(h, F.EU_CLOSED, F.UTIL_NEG_SQ_DIST, None, 0, F.dptr(th), m, F.dptr(pr), 2, F.dptr(F.f64(Zf)), 4, F.dptr(out), None) < 0
    assert b"bocf_acq_kg" in lib.bocf_last_error()
    assert lib.bocf_acq_pending(h, F.UTIL_NEG_SQ_DIST, None, 0, F.dptr(th), m, F.dptr(pr), 2, F.dptr(out), None) < 0
    assert b"bocf_acq_pending" in lib.bocf_last_error()
    # re-staged for the new model, still without candidates: the look-ahead acquisitions name what is missing
    model.set_reference_points(A)
    model.set_pending_points(P, Zp, W=W)
    assert lib.bocf_acq_kg(h, F.EU_CLOSED, F.UTIL_NEG_SQ_DIST, None, 0, F.dptr(th), m, F.dptr(pr), 2, F.dptr(F.f64(Zf)), 4, F.dptr(out), None) < 0
    msg = lib.bocf_last_error()
    assert b"bocf_acq_kg" in msg and b"no resident candidates" in msg, msg
    assert lib.bocf_acq_pending(h, F.UTIL_NEG_SQ_DIST, None, 0, F.dptr(th), m, F.dptr(pr), 2, F.dptr(out), None) < 0
    msg = lib.bocf_last_error()
    assert b"bocf_acq_pending" in msg and b"no resident candidates" in msg, msg
    assert np.all(np.isnan(out))
    # ---- re-staged and evaluated: the N + 1-point model
    kg1, al1 = evaluate(model)
    kgf, alf = evaluate(make(N + 1))
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    assert all(f.jitter == 0 for f in la.fits)
    rk = la.kg(Xc, A, Zf, thetas, prob, "closed", "neg_sq_dist")
    rp = PR.pending(la, Xc, P, Zp, W, thetas, prob, "neg_sq_dist")
    print("after an append: uKG max abs err %.3g (term size %.3g, moved by the new point %.3g); pending max abs err %.3g (scale %.3g, moved %.3g)"
          % (np.abs(kg1 - rk["kg"]).max(), rk["vscale"], np.abs(kg1 - kg0).max(), np.abs(al1 - rp["alpha"]).max(), rp["scale"], np.abs(al1 - al0).max()))
    # (the new point matters: values of the N-point model would show)
    assert np.abs(kg1 - kg0).max() > 30 * (1e-5 * np.abs(kg1).max() + 1e-12 * rk["vscale"])
    assert np.abs(al1 - al0).max() > 30 * (1e-5 * np.abs(al1).max() + 1e-12 * rp["scale"]) and np.mean(rp["alpha"] > 0) > 0.05
    np.testing.assert_allclose(kg1, kgf, rtol=1e-5, atol=1e-12 * rk["vscale"])
    np.testing.assert_allclose(kg1, rk["kg"], rtol=1e-5, atol=1e-12 * rk["vscale"])
    np.testing.assert_allclose(al1, alf, rtol=1e-5, atol=1e-12 * rp["scale"])
    np.testing.assert_allclose(al1, rp["alpha"], rtol=1e-5, atol=1e-12 * rp["scale"])
    a1 = model.acq_mc(Xc, F.ACQ_EI, F.UTIL_NEG_SQ_DIST, None, thetas, prob, W=W)
    assert a1.shape == a0.shape and len(model.select_topk(4)[0]) == 4
