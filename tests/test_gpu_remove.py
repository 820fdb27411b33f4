"""Removal of observations from the resident model -- bocf_remove (remove.hip: scan, block partial sums, rotation and store kernels),
multi_outputGP.remove_observations / updateModel with a deleted row, CBO(max_observations=...) -- against the NumPy oracle refitted from
scratch on the surviving points and, where conditioning matters, against the long-double truth (oracle/truth.py).

Helpers, problems and tolerances are those of tests/test_gpu_incremental.py (its header lists them): mean rtol 1e-6 / atol 1e-7,
|dvar| <= 1e-9, log-marginal rtol 1e-9, L rtol 1e-6 / atol 1e-9, alpha rtol 1e-6, input and hyper-gradients as there.  The inputs are ones
the oracle factorizes with zero jitter (asserted); tests/test_remove_cpu.py shows on the oracle alone that every removal of the boundary
cases moves the posterior at the candidates by more than these gates.  updateModel takes a deleted row on the resident factor only
under model.incremental_remove (remove_rows sets it; the default, a refit, is pinned in tests/test_remove_cpu.py).  A refused removal turns into a refit inside the model class, so
every case that means to exercise the kernels counts the _fit calls and asserts the exact number."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remove_ref as RR  # noqa: E402
import loo_ref as LR  # noqa: E402
import test_gpu_incremental as G  # noqa: E402
from test_gpu_incremental import B, device_model, oracle, check, count_fits, gate_rows  # noqa: E402,F401  (B: that module's fixture)

from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
TILE = 128


def remove_rows(model, p, rows, Ys=None):
    """updateModel with the observations `rows` of problem p (in this order), deleted rows taken on the resident factor."""
    model.incremental_remove = True
    model.updateModel(p["X"][rows], [y[rows] for y in (p["Y"] if Ys is None else Ys)])


def check_rows(model, kinds, p, rows, Ys=None):
    check(model, oracle(kinds, p, p["X"][rows], [y[rows] for y in (p["Y"] if Ys is None else Ys)]), p["Xc"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. tile and grid boundaries: every N with the first (all rotations) and the last (none) observation, every tile-edge k at N = 385
@pytest.mark.parametrize("N,k,m,d,kind,noise", RR.BOUNDARY, ids=["N%d-k%d-m%d-d%d-%s-%g" % c for c in RR.BOUNDARY])
def test_remove_at_tile_and_grid_boundaries(B, N, k, m, d, kind, noise):
    kinds = G.kinds_of(kind, m)
    p = RR.make_outlier(G.problem(N, d, m, noise, RR.boundary_seed(N, k, m)), k)
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    rows = [i for i in range(N) if i != k]
    if k % 2 == 0:
        remove_rows(model, p, rows)                        # through updateModel's row matching
    else:
        model.remove_observations([k])
    assert calls["fit"] == 0
    assert model._X.shape[0] == N - 1
    check_rows(model, kinds, p, rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the padding row a removal frees
def test_append_after_a_removal_at_a_full_padding(B):
    """N = 256 = Np: an append alone is refused (no padding row); after a removal it runs on the freed row."""
    N, m, d = 256, 2, 3
    kinds = ["matern52", "rbf"]
    p = G.problem(N + 1, d, m, 1e-4, 3911)                # (seeds: no log-marginal of the states checked cancels, found on the CPU, asserted by check)
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    rows = [i for i in range(N) if i != 100]
    model.remove_observations([100])
    assert calls["fit"] == 0
    check_rows(model, kinds, p, rows)
    rows.append(N)
    remove_rows(model, p, rows)                            # one new last row: bocf_append into the freed padding row
    assert calls["fit"] == 0
    check_rows(model, kinds, p, rows)


def test_remove_append_remove_append_at_one_tile(B):
    N, m, d = 128, 1, 2
    kinds = ["rbf"]
    p = G.problem(N + 2, d, m, 1e-4, 912)
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    rows = list(range(N))
    for drop, add in ((0, N), (64, N + 1)):
        rows.remove(drop)
        remove_rows(model, p, rows)
        rows.append(add)
        remove_rows(model, p, rows)
        assert calls["fit"] == 0
        check_rows(model, kinds, p, rows)


def test_window_of_256_slid_64_times(B):
    """Delete the first row and add a last one in ONE updateModel, 64 times at N = 256 = Np: no refit; checked after step 1 and at the end."""
    W, steps, m, d = 256, 64, 2, 3
    kinds = ["matern52", "matern32"]
    p = G.problem(W + steps, d, m, 1e-4, 3913)
    model = device_model(B, kinds, p, W)
    calls = count_fits(model)
    for s in range(1, steps + 1):
        rows = list(range(s, W + s))
        remove_rows(model, p, rows)
        if s in (1, steps):
            assert calls["fit"] == 0
            check_rows(model, kinds, p, rows)
    assert calls["fit"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the padding and scratch each factorization schedule leaves behind, buffers of a larger earlier fit, H m resident factorizations
@pytest.mark.parametrize("N", [300, 1100])
@pytest.mark.parametrize("team_fit,schedule", [(0, 0), (-1, 3)], ids=["launched", "default"])
def test_remove_behind_each_schedule(B, N, team_fit, schedule):
    m, d = 2, 3
    kinds = ["matern52", "rbf"]
    p = G.problem(N + 1, d, m, 1e-4, {300: 1600, 1100: 1400}[N])
    model = device_model(B, kinds, p, N + 1, options=[("team_fit", team_fit)])
    assert model._context().stat("last_schedule") == schedule
    calls = count_fits(model)
    model.remove_observations([N])                         # the last row first, then one in the first tile: the N - 1 points of rows
    model.remove_observations([5])
    assert calls["fit"] == 0
    assert model._context().stat("last_schedule") == schedule       # (no factorization since)
    check_rows(model, kinds, p, [i for i in range(N) if i != 5])


@pytest.mark.parametrize("N_big,N_small", [(380, 260), (300, 140)], ids=["same-Np", "smaller-Np"])
def test_remove_on_buffers_of_a_larger_earlier_fit(B, N_big, N_small):
    m, d = 2, 4
    kinds = ["rbf", "matern32"]
    big = G.problem(N_big, d, m, 1e-4, 400 + N_big)
    p = G.problem(N_small, d, m, 1e-4, 500 + N_small)
    for key in ("lengthscales", "variances"):
        p[key] = big[key]
    model = device_model(B, kinds, big, N_big)
    calls = count_fits(model)
    G.update(model, p, N_small)
    assert calls["fit"] == 1
    model.remove_observations([N_small - 1, 3, 130])       # from the highest index down, one bocf_remove each
    assert calls["fit"] == 1
    check_rows(model, kinds, p, [i for i in range(N_small) if i not in (3, 130, N_small - 1)])


def _abi_predict(F, lib, ctx, Xc, M):
    mean, v = np.full((M, len(Xc)), np.nan), np.full((M, len(Xc)), np.nan)
    assert lib.bocf_set_candidates(ctx.handle, F.dptr(Xc), len(Xc)) == 0
    assert lib.bocf_predict(ctx.handle, F.ADD_NOISE | F.CLIP, F.dptr(mean), F.dptr(v)) == 0
    return mean, v


def test_remove_with_two_hyper_sample_groups_at_the_abi(B):
    """hyper_samples = 2: M = H m = 4 resident factorizations with different hyper-parameters, one bocf_remove for all of them."""
    F = B._ffi
    lib = F.load()
    ctx = F.Context(0)
    N, d, m, H, k = 200, 3, 2, 2, 130
    p = G.problem(N, d, m, 1e-4, 914)
    var = F.f64(list(p["variances"]) + [1.3 * v for v in p["variances"]])
    ls = F.f64(np.stack(list(p["lengthscales"]) + [0.8 * l for l in p["lengthscales"]]))
    noise = F.f64([1e-4] * (H * m))
    X, Y = F.f64(p["X"]), F.f64(np.tile(np.stack([y[:, 0] for y in p["Y"]]), (H, 1)))
    ctx.set_option("hyper_samples", H)
    jit, lml = np.ones(H * m), np.zeros(H * m)
    assert lib.bocf_fit(ctx.handle, F.dptr(X), F.dptr(Y), N, d, H * m, F.KERN_MATERN52, F.dptr(var), F.dptr(ls), F.dptr(noise), 5, F.dptr(jit), F.dptr(lml)) == 0
    assert np.all(jit == 0)
    Y1 = F.f64(np.delete(Y, k, axis=1))
    out = np.full(H * m, np.nan)
    assert lib.bocf_remove(ctx.handle, k, F.dptr(Y1), F.dptr(out)) == 0
    Xc = F.f64(p["Xc"])
    mean, v = _abi_predict(F, lib, ctx, Xc, H * m)
    Xr, Yr = RR.without(p, k)
    for row in range(H * m):
        fit = R.GPFit("matern52", Xr, Yr[row % m], var[row], ls[row], noise[row])
        assert fit.jitter == 0
        rm, rv = fit.predict(p["Xc"])
        np.testing.assert_allclose(mean[row], rm[:, 0], rtol=1e-6, atol=1e-7)
        assert np.abs(v[row] - rv[:, 0]).max() <= 1e-9
        np.testing.assert_allclose(out[row], fit.log_marginal, rtol=1e-9)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. what is derived from the factor
@pytest.mark.parametrize("option,kind,tol", [("predict_f32", "matern32", 2e-5), ("predict_i8", "rbf", 1e-9)])
def test_reduced_precision_copies_follow_a_removal(B, option, kind, tol):
    """As test_reduced_precision_copies_follow_an_append: the copy of the N-point factor is built, the outlier on a candidate removed; the
    copy must be rebuilt (the N-point posterior differs by far more than the tolerance, asserted on the oracle)."""
    N, m, d, C, k = 300, 2, 3, 64, 77
    kinds = [kind] * m
    p = G.problem(N, d, m, 1e-4, 600, C=C)
    for y in p["Y"]:
        y[k] = float(y.mean()) + 5.0
    p["Xc"][0] = p["X"][k]
    tol = tol * max(1.0, max(p["variances"])) + 1e-9
    rows = [i for i in range(N) if i != k]
    ref0 = oracle(kinds, p, p["X"], p["Y"])
    ref1 = oracle(kinds, p, p["X"][rows], [y[rows] for y in p["Y"]])
    (rm0, rv0), (rm1, rv1) = ref0.predict(p["Xc"]), ref1.predict(p["Xc"])
    assert np.abs(rv0 - rv1).max() > 1e3 * tol and np.abs(rm0 - rm1).max() > 1.0
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    model.set_option(option, 1)
    mean0, var0 = model.predict(p["Xc"])                   # builds the copy of the N-point factor
    assert np.abs(var0 - rv0).max() <= tol
    model.remove_observations([k])
    assert calls["fit"] == 0 and np.all(model.jitter == 0)
    mean1, var1 = model.predict(p["Xc"])
    np.testing.assert_allclose(mean1, rm1, rtol=1e-6, atol=1e-7)
    print("%s after a removal: max |dvar| %.3e against the N - 1 oracle (bound %.3e), %.3e against the N-point one"
          % (option, np.abs(var1 - rv1).max(), tol, np.abs(var1 - rv0).max()))
    assert np.abs(var1 - rv1).max() <= tol
    fresh = device_model(B, kinds, p, options=[(option, 1)])
    remove_rows(fresh, p, rows)
    meanf, varf = fresh.predict(p["Xc"])
    np.testing.assert_allclose(mean1, meanf, rtol=1e-6, atol=1e-7)
    assert np.abs(var1 - varf).max() <= tol


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_cached_inverse_is_dropped_by_a_removal(B, kind):
    """bocf_infer (leaves Ky^-1 in the T scratch under the one-team-launch schedule) -> bocf_remove (uses that scratch) ->
    bocf_lml_gradients == the oracle on the N - 1 points."""
    F = B._ffi
    N, k = 600, 301
    p, X, Y, var, ls, noise = G._abi_problem(B, kind, N)
    ctx = F.Context(0)
    G._abi_infer(B, ctx, kind, X, Y, var, ls, noise)
    Y1 = F.f64(np.delete(Y, k, axis=1))
    lml = np.zeros(Y.shape[0])
    assert F.check(F.load().bocf_remove(ctx.handle, k, F.dptr(Y1), F.dptr(lml)), "bocf_remove") == 0
    got = G._abi_gradients(B, ctx, Y.shape[0], X.shape[1])
    G._check_hyper_gradients(kind, p, np.delete(X, k, axis=0), Y1, lml, got)
    ctx.close()


@pytest.mark.parametrize("N,d,kinds,k", [(128, 3, ("se", "matern52", "matern32"), 0), (129, 1, ("matern52",), 64)], ids=["129to128", "130to129"])
def test_loo_after_a_removal(B, N, d, kinds, k):
    """bocf_loo reads R and alpha: after a removal they are those of the N surviving points (tests/loo_ref.py, gates of tests/test_gpu_loo.py)."""
    import test_gpu_loo as TL
    ref = LR.reference(N, d, kinds, TL.SEED)
    rng = np.random.RandomState(5)
    X = np.insert(ref["X"], k, rng.uniform(size=d), axis=0)
    Y = np.insert(ref["Y"], k, 3.0, axis=1)
    model = TL._model(kinds, X, Y, ref["var"], ref["ls"], ref["noise"])
    assert np.all(model.jitter == 0)
    calls = count_fits(model)
    model.remove_observations([k])
    assert calls["fit"] == 0
    np.testing.assert_array_equal(model._X, ref["X"])
    TL._gate("removal to %d" % N, model, ref)


def test_resident_state_across_a_removal(B):
    """After a removal nothing scores the old batch, and the reference set and pending points are gone, exactly as after an append."""
    F = B._ffi
    lib = F.load()
    N, d, C, S = 131, 3, 64, 16
    kinds = ["se", "matern52", "rbf"]
    m = len(kinds)
    p = G.problem(N, d, m, 1e-4, 23, C=C)
    rng = np.random.RandomState(9)
    A, Zf = rng.uniform(size=(8, d)), rng.normal(size=(4, m))
    P, Zp, W = rng.uniform(size=(3, d)), rng.normal(size=(S, m, 3)), rng.normal(size=(S, m))
    thetas, prob = rng.uniform(-0.5, 0.5, size=(2, m)), np.array([0.4, 0.6])
    model = device_model(B, kinds, p, N)
    h = model._context().handle

    def evaluate(mdl):
        mdl.set_reference_points(A)
        kg = mdl.acq_kg(p["Xc"], "closed", F.UTIL_NEG_SQ_DIST, None, thetas, prob, Zf)
        mdl.set_pending_points(P, Zp, W=W)
        return kg, mdl.acq_pending(p["Xc"], F.UTIL_NEG_SQ_DIST, None, thetas, prob, W=W)
    evaluate(model)
    model.acq_mc(p["Xc"], F.ACQ_EI, F.UTIL_NEG_SQ_DIST, None, thetas, prob, W=W)
    assert len(model.select_topk(4)[0]) == 4
    calls = count_fits(model)
    model.remove_observations([50])
    assert calls["fit"] == 0
    with pytest.raises(F.BocfHipError, match="no acquisition vector"):
        model.select_topk(4)
    th, pr, out = F.f64(thetas), F.f64(prob), np.full(C, np.nan)
    # the candidate batch itself is gone (its workspaces were the removal's scratch): the Monte-Carlo acquisition sees an error or an
    # EMPTY batch -- nothing written, no acquisition vector left to select from
    rc = lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_NEG_SQ_DIST, None, 0, F.dptr(th), m, F.dptr(pr), 2, F.dptr(out))
    assert rc <= 0 and np.all(np.isnan(out))
    with pytest.raises(F.BocfHipError, match="no acquisition vector"):
        model.select_topk(4)
    assert lib.bocf_acq_kg(h, F.EU_CLOSED, F.UTIL_NEG_SQ_DIST, None, 0, F.dptr(th), m, F.dptr(pr), 2, F.dptr(F.f64(Zf)), 4, F.dptr(out), None) < 0
    assert b"bocf_acq_kg" in lib.bocf_last_error()
    assert lib.bocf_acq_pending(h, F.UTIL_NEG_SQ_DIST, None, 0, F.dptr(th), m, F.dptr(pr), 2, F.dptr(out), None) < 0
    assert b"bocf_acq_pending" in lib.bocf_last_error()
    assert np.all(np.isnan(out))
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
    kg1, al1 = evaluate(model)                             # re-staged and evaluated: the N - 1-point model
    rows = [i for i in range(N) if i != 50]
    fresh = device_model(B, kinds, p)
    remove_rows(fresh, p, rows)
    kgf, alf = evaluate(fresh)
    np.testing.assert_allclose(kg1, kgf, rtol=1e-5, atol=1e-12 * max(1.0, np.abs(kgf).max()))
    np.testing.assert_allclose(al1, alf, rtol=1e-5, atol=1e-12 * max(1.0, np.abs(alf).max()))


def test_sample_paths_are_dropped_by_a_removal():
    """As the append in test_gpu_paths.test_lifetime: staged paths are gone after a removal (both path entry points say so), and paths
    re-staged afterwards are those of the N - 1-point model (the restatement tests/paths_ref.py, that test's tolerance)."""
    import test_gpu_paths as TP
    Bm, F = TP.B, TP._ffi
    kinds = ("rbf", "matern52")
    N, d, S, nf, C, k = 101, 2, 5, 130, 10, 37
    X, Y, var, lss = TP._data(kinds, N, d, 33)
    m = len(kinds)
    model = Bm.multi_outputGP(m, kernel=[TP.KINDS[kinds[j]](d, variance=var[j], lengthscale=lss[j], ARD=True) for j in range(m)], noise_var=[1e-2] * m,
                              fixed_hyps=True)
    model.updateModel(X, Y)
    lib, h = F.load(), model._context().handle
    Xc = np.random.RandomState(2).uniform(size=(C, d))
    TP._stage(h, TP.PR.draw(kinds, N, d, nf, S, np.random.RandomState(1)))
    model._set_candidates(Xc)
    assert np.all(np.isfinite(TP._values(h, m, C, S)))
    calls = count_fits(model)
    model.remove_observations([k])
    assert calls["fit"] == 0 and model._resident.paths is None
    model._set_candidates(Xc)
    out = np.full((m, C, S), np.nan)
    assert lib.bocf_path_values(h, -1, F.dptr(out)) < 0
    assert b"bocf_path_values" in lib.bocf_last_error() and b"no paths are resident" in lib.bocf_last_error()
    rc, _, _ = TP._path_utility(h, F.UTIL_LINEAR, np.ones((S, m)), S, np.zeros(C, dtype=int), C, d)
    assert rc < 0 and b"no paths are resident" in lib.bocf_last_error()
    assert np.all(np.isnan(out))
    X1, Y1 = np.delete(X, k, axis=0), [np.delete(y, k, axis=0) for y in Y]
    draws1 = TP.PR.draw(kinds, N - 1, d, nf, S, np.random.RandomState(4))
    TP._stage(h, draws1)
    ref = R.MultiOutputGPRef(list(kinds), var, lss, [1e-2] * m)
    ref.updateModel(X1, Y1)
    np.testing.assert_allclose(TP._values(h, m, C, S), TP.PR.Paths(ref, Y1, *draws1).values(Xc), rtol=0, atol=1e-10 * var.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. a chain of removals, and removals between appends and new targets, against the long-double truth (gates of
# test_chain_of_appends_against_the_truth: oracle/truth.gate)
def test_chain_of_removals_against_the_truth(B):
    """N = 512 -> 385 one observation at a time: 127 removals, every third at index 0 (all rotations), no refit, Matern-5/2 at noise 1e-6;
    gated at the end, a from-scratch device fit of the same points printed beside it so that drift is visible."""
    m, d, N = 2, 4, 512
    kinds = ["matern52"] * m
    p = R.synthetic_problem(N, d, m, 60, 4, 5151, noise=1e-6)
    p["lengthscales"] = [1.8 * l for l in p["lengthscales"]]
    model = device_model(B, kinds, p, N)
    calls = count_fits(model)
    rows = list(range(N))
    rng = np.random.RandomState(12)
    for step in range(127):
        k = 0 if step % 3 == 0 else int(rng.randint(len(rows)))
        del rows[k]
        if step % 2:
            model.remove_observations([k])
        else:
            remove_rows(model, p, rows)
    assert calls["fit"] == 0 and np.all(model.jitter == 0) and len(rows) == 385
    q = dict(p, X=p["X"][rows], Y=[y[rows] for y in p["Y"]])
    Ky = R.kern_K("matern52", q["X"], None, q["variances"][0], q["lengthscales"][0]) + (1e-6 + 1e-8) * np.eye(385)
    print("chain of removals: cond(Ky) = %.3e at N = 385" % np.linalg.cond(Ky))
    ok, r = gate_rows("N = 385, chained from 512", model, kinds, q, 385)
    ok2, r2 = gate_rows("N = 385, from scratch", device_model(B, kinds, q, 385), kinds, q, 385)
    print("max abs error against the long-double truth:\n  " + "\n  ".join(r + r2))
    assert ok and ok2


def test_removals_appends_and_targets_interleaved(B):
    """remove -> new targets -> append -> remove -> append on one model from N = 130, gated after every step, no refit."""
    kinds = ["matern52"] * 3
    p = G._targets_problem()
    Ya = [1.5 * y - 0.3 for y in p["Y"]]
    model = device_model(B, kinds, p, 130)
    calls = count_fits(model)
    ok_all, out = True, []
    steps = [([i for i in range(130) if i != 0], p["Y"]), ([i for i in range(130) if i != 0], Ya),
             ([i for i in range(131) if i != 0], Ya), ([i for i in range(131) if i not in (0, 128)], Ya),
             ([i for i in range(132) if i not in (0, 128, 129)], p["Y"])]          # row 129 leaves, row 131 arrives, new targets
    for step, (rows, Ys) in enumerate(steps):
        remove_rows(model, p, rows, Ys)
        q = dict(p, X=p["X"][rows], Y=[y[rows] for y in Ys])
        ok, r = gate_rows("step %d (N = %d)" % (step, len(rows)), model, kinds, q, len(rows), centre=[float(y.mean()) for y in q["Y"]])
        ok_all &= ok
        out += r
    print("max abs error against the long-double truth:\n  " + "\n  ".join(out))
    assert calls["fit"] == 0 and np.all(model.jitter == 0)
    assert ok_all


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the refusals
def test_removal_from_a_jittered_factor_refits(B, probes):
    """One output carries jitter (the diagonal-shift hook of the probes build): bocf_remove returns 1 and leaves the model as it was;
    through the model class that is exactly one refit, equal to a from-scratch model bit for bit."""
    F = B._ffi
    rng = np.random.RandomState(4)
    N, d, m, k = 150, 2, 3, 40
    X = rng.uniform(size=(N, d))
    Y = [rng.normal(size=(N, 1)) for _ in range(m)]
    Xc = rng.uniform(size=(40, d))
    ls = [[0.4, 0.4], [500.0, 500.0], [0.3, 0.5]]          # output 1: K numerically rank one
    noise = [1e-6, 0.0, 1e-6]

    def make():
        model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=np.array(l), ARD=True) for l in ls], noise_var=noise, fixed_hyps=True)
        model.set_option("test_diag_shift_1e12", 20000)
        return model
    model = make()
    model.updateModel(X, Y)
    assert model.jitter[1] > 0 and model.jitter[0] == 0 and model.jitter[2] == 0
    lib, ctx, Xcd = F.load(), model._context(), F.f64(Xc)
    before = _abi_predict(F, lib, ctx, Xcd, m)             # (at the ABI: no host-side cache answers in the device's place)
    Y1 = F.f64(np.stack([np.delete(y[:, 0], k) for y in Y]))
    out = np.full(m, np.nan)
    assert lib.bocf_remove(ctx.handle, k, F.dptr(Y1), F.dptr(out)) == 1
    assert np.all(np.isnan(out))
    for a, b in zip(before, _abi_predict(F, lib, ctx, Xcd, m)):
        np.testing.assert_array_equal(a, b)                # nothing has been touched
    calls = count_fits(model)
    model.remove_observations([k])
    assert calls["fit"] == 1
    scratch = make()
    scratch.incremental = False
    scratch.updateModel(np.delete(X, k, axis=0), [np.delete(y, k, axis=0) for y in Y])
    np.testing.assert_array_equal(model.jitter, scratch.jitter)
    np.testing.assert_array_equal(model.log_marginal, scratch.log_marginal)
    for a, b in zip(model.predict(Xc), scratch.predict(Xc)):
        np.testing.assert_array_equal(a, b)


def test_removal_refuses_an_output_sharded_fit(B, probes):
    F = B._ffi
    lib = F.load()
    ctx = F.Context(0)
    p = G.problem(150, 3, 4, 1e-4, 808)
    X, Y = F.f64(p["X"]), F.f64(np.stack([y[:, 0] for y in p["Y"]]))
    var, ls, noise = F.f64(p["variances"]), F.f64(np.stack(p["lengthscales"])), F.f64(p["noise"])
    ctx.set_option("shard_fit_simulate", 2)
    ctx.set_option("shard_fit", 1)
    jit, lml = np.ones(4), np.zeros(4)
    assert lib.bocf_fit(ctx.handle, F.dptr(X), F.dptr(Y), 150, 3, 4, F.KERN_MATERN52, F.dptr(var), F.dptr(ls), F.dptr(noise), 5, F.dptr(jit), F.dptr(lml)) == 0
    Xc = F.f64(p["Xc"])
    before = _abi_predict(F, lib, ctx, Xc, 4)
    out = np.full(4, np.nan)
    assert lib.bocf_remove(ctx.handle, 10, F.dptr(F.f64(np.delete(Y, 10, axis=1))), F.dptr(out)) == 1
    assert np.all(np.isnan(out))
    for a, b in zip(before, _abi_predict(F, lib, ctx, Xc, 4)):
        np.testing.assert_array_equal(a, b)
    ctx.close()


@pytest.mark.parametrize("ask_the_device", [False, True], ids=["incremental-off", "bocf_remove-returns-1"])
def test_removal_from_an_output_sharded_fit_through_the_model_class_refits_once(B, probes, ask_the_device):
    """set_option("shard_fit") turns the incremental updates off, so remove_observations refits at once; with them forced back on
    bocf_remove is asked, returns 1, and the model refits.  Either way exactly one (sharded) refit, equal to a from-scratch model bit for bit."""
    N, k = 150, 20
    kinds = ["matern52"] * 4
    p = G.problem(N, 3, 4, 1e-4, 808)
    options = [("shard_fit_simulate", 2), ("shard_fit", 1)]
    model = device_model(B, kinds, p, N, options=options)
    assert model.incremental is False and np.all(model.jitter == 0)
    model.incremental = ask_the_device
    calls = count_fits(model)
    model.remove_observations([k])
    assert calls["fit"] == 1 and model._X.shape[0] == N - 1
    rows = [i for i in range(N) if i != k]
    scratch = device_model(B, kinds, p, options=options)
    scratch.updateModel(p["X"][rows], [y[rows] for y in p["Y"]])
    np.testing.assert_array_equal(model.log_marginal, scratch.log_marginal)
    for a, b in zip(model.predict(p["Xc"]), scratch.predict(p["Xc"])):
        np.testing.assert_array_equal(a, b)
    ref = oracle(kinds, p, p["X"][rows], [y[rows] for y in p["Y"]])
    np.testing.assert_allclose(model.predict(p["Xc"])[0], ref.predict(p["Xc"])[0], rtol=1e-6, atol=1e-7)


def test_invalid_removals_are_errors_with_a_message(B):
    F = B._ffi
    lib = F.load()
    ctx = F.Context(0)
    p = G.problem(20, 2, 1, 1e-4, 5)
    X, Y = F.f64(p["X"]), F.f64(p["Y"][0][:, 0][None, :])
    var, ls, noise = F.f64(p["variances"]), F.f64(np.stack(p["lengthscales"])), F.f64(p["noise"])
    out, jit = np.full(1, np.nan), np.ones(1)

    def bad(rc, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and b"bocf_remove" in msg and text in msg, (rc, msg)
    bad(lib.bocf_remove(ctx.handle, 0, F.dptr(Y), F.dptr(out)), b"not fitted")                     # an unfitted context
    bad(lib.bocf_remove(None, 0, F.dptr(Y), F.dptr(out)), b"not fitted")
    fit = lambda n: lib.bocf_fit(ctx.handle, F.dptr(X), F.dptr(Y), n, 2, 1, F.KERN_RBF, F.dptr(var), F.dptr(ls), F.dptr(noise), 5, F.dptr(jit), F.dptr(out))
    assert fit(20) == 0
    out[:] = np.nan
    Y1 = F.f64(Y[:, :19])
    bad(lib.bocf_remove(ctx.handle, -1, F.dptr(Y1), F.dptr(out)), b"index outside")
    bad(lib.bocf_remove(ctx.handle, 20, F.dptr(Y1), F.dptr(out)), b"index outside")
    bad(lib.bocf_remove(ctx.handle, 3, None, F.dptr(out)), b"null Y")
    assert np.all(np.isnan(out))
    assert lib.bocf_remove(ctx.handle, 19, F.dptr(Y1), F.dptr(out)) == 0 and np.isfinite(out[0])  # (the context was left usable)
    assert fit(1) == 0
    bad(lib.bocf_remove(ctx.handle, 0, F.dptr(Y1), F.dptr(out)), b"only observation")             # N = 1
    mean, v = F.f64(np.zeros((1, 4))), F.f64(np.ones((1, 4)))
    assert lib.bocf_set_posterior(ctx.handle, 1, 4, 3, F.dptr(mean), F.dptr(v), F.dptr(F.f64(np.zeros((1, 3))))) == 0
    bad(lib.bocf_remove(ctx.handle, 0, F.dptr(Y1), F.dptr(out)), b"not fitted")                    # a canned posterior
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the sliding window of the BO loop
def _bo(B, seed, **window):
    np.random.seed(seed)
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m, fixed_hyps=True)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9]]), prob_dist=np.array([0.5, 0.5])), device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=100, n_anchor=4)
    acq = B.uEI_noiseless(model, space, optimizer=opt, utility=U)
    X0 = np.random.uniform(size=(12, d))
    objective = B.MultiObjective(f, noise_var=[1e-4] * m)
    return B.CBO(model, space, objective, acq, B.Sequential(acq), X0, **window), model


def test_cbo_sliding_window(B):
    bo, model = _bo(B, 7, max_observations=12)
    calls = count_fits(model)
    sizes = []
    orig = model.updateModel

    def recording(X, Y):
        sizes.append(np.atleast_2d(X).shape[0])
        orig(X, Y)
    model.updateModel = recording
    bo.run_optimization(max_iter=5)
    assert calls["fit"] == 1                               # the first fit; every later update is a removal and an append, or new targets
    assert max(sizes) == 12 and bo.X.shape == (12, 2) and all(y.shape == (12, 1) for y in bo.Y)
    assert bo.num_acquisitions == 5
    fresh = B.multi_outputGP(2, kernel=[B.kern.RBF(2, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(2)], noise_var=[1e-4] * 2, fixed_hyps=True)
    fresh.updateModel(bo.X, bo.Y)
    Xc = np.random.RandomState(3).uniform(size=(40, 2))
    (m1, v1), (m0, v0) = model.predict(Xc), fresh.predict(Xc)
    np.testing.assert_allclose(m1, m0, rtol=1e-6, atol=1e-7)
    assert np.abs(v1 - v0).max() <= 1e-9
    np.testing.assert_allclose(model.log_marginal, fresh.log_marginal, rtol=1e-9)


def test_cbo_forget_callable_and_default(B):
    """forget as a callable names the row that leaves; max_observations=None (and a window never reached) leave the loop as it is."""
    bo, model = _bo(B, 8, max_observations=12, forget=lambda X, Y: int(np.argmin(Y[0][:, 0])))
    calls = count_fits(model)
    first = None

    def spy(X, Y, pick=bo.forget):
        nonlocal first
        k = pick(X, Y)
        first = (X[k].copy(), X.shape[0]) if first is None else first
        return k
    bo.forget = spy
    bo.run_optimization(max_iter=2)
    assert calls["fit"] == 1 and bo.X.shape == (12, 2)
    assert first[1] == 13 and not np.any(np.all(bo.X == first[0], axis=1))
    runs = []
    for window in ({}, {"max_observations": None}, {"max_observations": 1000}):
        bo, model = _bo(B, 9, **window)
        bo.run_optimization(max_iter=2)
        runs.append((bo.X.copy(), [y.copy() for y in bo.Y]))
    for X, Y in runs[1:]:
        np.testing.assert_array_equal(X, runs[0][0])
        for a, b in zip(Y, runs[0][1]):
            np.testing.assert_array_equal(a, b)
    for bad in (0, 1):                                     # (the loop measures the distance of the last two evaluations)
        with pytest.raises(ValueError):
            _bo(B, 9, max_observations=bad)
    with pytest.raises(ValueError):
        _bo(B, 9, max_observations=5, forget="newest")
