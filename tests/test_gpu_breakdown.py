"""GPU: pivot breakdown at every panel position under every Cholesky schedule.  The device's fit is optimistic -- the diagonal-block kernel
records the first bad pivot and carries on with a unit pivot, the inverse and the alpha solve are enqueued before the host knows, garbage
flows through row solves, trailing updates, the early inverse and the dependency counters, and the next rung rebuilds K into the same
buffers.  On the problems of tests/breakdown_problem.py (breakdown at ONE known pivot k by a margin no summation order can move;
tests/test_breakdown_cpu.py shows that on the oracle alone) this file pins: the reported position is LAPACK's k + 1 for k on every strip,
16-block, panel and hybrid-split edge; per output; at every rung of jitchol's ladder; and a failed attempt leaves NOTHING behind -- no
counted time-out, an un-fitted context, and a next fit that is bit for bit a fresh context's.
Run on the MI355X box: python -m pytest tests -m gpu"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breakdown_problem as P  # noqa: E402

from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KID = {"rbf": 0, "se": 1, "matern52": 2, "matern32": 3}
CLIP = 2


@pytest.fixture(scope="module")
def B():
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


# name -> (N, options, expected last_schedule (None: the factorization runs in the shard helper's context), warm, inference, outputs).
# warm: a clean fit first -- the reserved-CU chain is never a context's first factorization, and the 25-panel cases follow
# test_hybrid_time_out_is_redone_launched; the cold ones break down in the context's very first factorization.
CONFIGS = {
    "fit128": (128, (), 0, False, False, 1),                                                # one panel: the launched path
    "fused128": (128, (), None, False, True, 1),                                            # the fused inference launch
    "launched": (300, (("team_fit", 0),), 0, False, False, 1),
    "reserved": (300, (("team_fit", 0), ("lookahead", 2)), 2, True, False, 1),
    "team": (300, (), 3, False, False, 1),
    "team_kinv": (300, (), 3, False, True, 1),                                              # bocf_infer: the team launch that also forms Ky^-1
    "sharded": (300, (("shard_fit_simulate", 2), ("shard_fit", 1)), None, False, False, 2),
    "pairs": (600, (("aggregate", 2), ("lookahead", 0)), 0, False, False, 1),               # launched, two panels per trailing update
    "hybrid": (3100, (), 5, True, False, 2),
    "groups": (3100, (("team_fit", 1), ("team_hybrid", 0), ("team_panels", 5)), 4, True, False, 2),
    "launched25": (3100, (("team_fit", 0),), 0, True, False, 2),                            # launched, G = 2, early inverse
}
POSITION_CASES = [(name, k) for name in CONFIGS for k in P.POSITIONS[CONFIGS[name][0]]]
LADDER_K = {128: 64, 300: 129, 600: 256, 3100: 2048}


class _Result(object):
    def __init__(self, rc, info, jit, lml, grads):
        self.rc, self.info, self.jit, self.lml, self.grads = rc, info, jit, lml, grads


def _candidates(p):
    return np.random.RandomState(9200 + p.N).uniform(size=(64, p.d))


def _context(B, name, shift=0):
    ctx = B._ffi.Context(0)
    for key, value in CONFIGS[name][1]:
        ctx.set_option(key, value)
    ctx.set_option("test_diag_shift_1e12", shift)
    return ctx


def _expected_schedule(ctx, name):
    want = CONFIGS[name][2]
    return 0 if want == 2 and not ctx.stat("cu_masks_ok") else want


def _run(B, ctx, name, p, clean, tries, noise=None):
    """bocf_fit / bocf_infer of problem p on the raw context, at its inputs with the repeated point or (clean) at the duplicate-free
    ones: (rc, per-output info, jitter, log-marginal, gradients)."""
    F, lib = B._ffi, B._ffi.load()
    infer, m = CONFIGS[name][4], max(p.m, CONFIGS[name][5])
    var, ls = F.f64(np.resize(p.variance, m)), F.f64(np.resize(p.lengthscale, (m, p.d)))
    nz = F.f64(np.resize(p.noise if noise is None else noise, m))
    Xh, Y = F.f64(p.X_clean if clean else p.X), F.f64((p.Y_clean if clean else p.Y)[:m])
    jit, lml = np.full(m, np.nan), np.full(m, np.nan)
    grads = None
    if infer:
        grads = (np.zeros(m), np.zeros((m, p.d)), np.zeros(m))
        rc = lib.bocf_infer(ctx.handle, F.dptr(Xh), F.dptr(Y), p.N, p.d, m, KID[p.kind], F.dptr(var), F.dptr(ls), F.dptr(nz), tries, F.dptr(jit), F.dptr(lml),
                            F.dptr(grads[0]), F.dptr(grads[1]), F.dptr(grads[2]))
    else:
        rc = lib.bocf_fit(ctx.handle, F.dptr(Xh), F.dptr(Y), p.N, p.d, m, KID[p.kind], F.dptr(var), F.dptr(ls), F.dptr(nz), tries, F.dptr(jit), F.dptr(lml))
    F.check(rc, "bocf_infer" if infer else "bocf_fit")
    info = (ctypes.c_int * m)()
    F.check(lib.bocf_last_fit_info(ctx.handle, info, m), "bocf_last_fit_info")
    return _Result(rc, list(info), jit, lml, grads)


def _factor(B, ctx, N, j, want_L=True):
    L, a = np.empty((N, N)) if want_L else None, np.empty(N)
    B._ffi.check(B._ffi.load().bocf_get_factor(ctx.handle, j, B._ffi.dptr(L), B._ffi.dptr(a)), "bocf_get_factor")
    return L, a


def _predict(B, ctx, p, m):
    F, lib = B._ffi, B._ffi.load()
    Xc = F.f64(_candidates(p))
    F.check(lib.bocf_set_candidates(ctx.handle, F.dptr(Xc), Xc.shape[0]), "bocf_set_candidates")
    mean, var = np.empty((m, Xc.shape[0])), np.empty((m, Xc.shape[0]))
    F.check(lib.bocf_predict(ctx.handle, CLIP, F.dptr(mean), F.dptr(var)), "bocf_predict")
    return mean, var


def _snapshot(B, ctx, name, p, res):
    """Everything a successful fit leaves that the host can read: log-marginal, jitter, an inference's gradients, the factor and alpha
    of every output (an output-sharded fit keeps no upper factor: alpha and a prediction instead; the fused inference leaves no model)."""
    N, m = p.N, len(res.info)
    out = [res.lml.copy(), res.jit.copy()] + ([g.copy() for g in res.grads] if res.grads else [])
    if name == "fused128":
        return out
    sharded = name == "sharded"
    for j in range(m):
        out.extend(a for a in _factor(B, ctx, N, j, want_L=not sharded) if a is not None)
    if sharded:
        out.extend(_predict(B, ctx, p, m))
    return out


_fresh = {}


def _fresh_clean_fit(B, name, p):
    """The clean fit (duplicate-free X, no shift) of a context that never saw a failure, under the configuration's options and warm-up:
    computed once per configuration (the clean problem does not depend on k), read-only."""
    if name not in _fresh:
        ctx = _context(B, name)
        if CONFIGS[name][3]:
            assert _run(B, ctx, name, p, True, 0).rc == 0
        res = _run(B, ctx, name, p, True, 0)
        assert res.rc == 0 and not any(res.info) and not res.jit.any()
        _fresh[name] = (_snapshot(B, ctx, name, p, res), ctx.stat("last_schedule"))
        ctx.close()
    return _fresh[name]


def _check_failed(B, ctx, name, res, info):
    """After a failing fit: LAPACK's position for every output, rc the first failing output's; no time-out counted (two of them would
    switch the gated schedules off for the context's lifetime); jitchol's message; the context is not fitted."""
    lib = B._ffi.load()
    assert res.info == info and res.rc == next(v for v in info if v), (res.rc, res.info, info)
    assert ctx.stat("sched_timeouts") == 0
    if _expected_schedule(ctx, name) is not None:
        assert ctx.stat("last_schedule") == _expected_schedule(ctx, name)
    assert "not positive definite" in lib.bocf_last_error().decode()
    assert lib.bocf_predict(ctx.handle, CLIP, None, None) < 0 and "not fitted" in lib.bocf_last_error().decode()


def _check_clean_fit_equals_fresh(B, ctx, name, p):
    """The same context, no shift, the duplicate-free X: bit for bit what a context that never failed computes."""
    ctx.set_option("test_diag_shift_1e12", 0)
    res = _run(B, ctx, name, p, True, 0)
    assert res.rc == 0 and not any(res.info) and not res.jit.any()
    want, schedule = _fresh_clean_fit(B, name, p)
    assert ctx.stat("last_schedule") == schedule and ctx.stat("sched_timeouts") == 0
    got = _snapshot(B, ctx, name, p, res)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------
# Cases 1-4: the position under every schedule, and what the failed attempt leaves behind.
@pytest.mark.parametrize("name,k", POSITION_CASES)
def test_breakdown_position_and_the_fit_after_it(B, probes, name, k):
    N, _, _, warm, _, m = CONFIGS[name]
    p = P.single(N, k)
    ctx = _context(B, name)
    if warm:
        assert _run(B, ctx, name, p, True, 0).rc == 0
    ctx.set_option("test_diag_shift_1e12", P.SHIFT_OPTION)
    res = _run(B, ctx, name, p, False, 0)
    _check_failed(B, ctx, name, res, [k + 1] * m)
    _check_clean_fit_equals_fresh(B, ctx, name, p)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# Case 6: jitchol's ladder per schedule.  max_jitter_tries counts RETRIES (as GPy's maxtries): the unjittered attempt and the rungs 1e-6,
# 1e-5, 1e-4 break down at the same k (pivot -6.0e-4, -5.98e-4, -5.8e-4, -4.0e-4), the fourth retry (1 - DELTA) 1e-3 factorizes (+1.4e-3).
def _big_reference(k):
    """The oracle's posterior of the N = 3100 problem at the effective noise jitter - shift (what the jittered device fit factorizes)."""
    key = ("big", k)
    if key not in _fresh:
        p = P.single(3100, k)
        ref = R.MultiOutputGPRef(p.kind, p.variance, list(p.lengthscale), list(p.jitter - P.SHIFT))
        ref.updateModel(p.X, [p.Y[j][:, None] for j in range(2)])
        _fresh[key] = ref.predict_noiseless(_candidates(p))
    return _fresh[key]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_ladder_per_schedule(B, probes, name):
    N, _, _, warm, infer, m = CONFIGS[name]
    k = LADDER_K[N]
    p = P.single(N, k)
    ctx = _context(B, name)
    if warm:
        assert _run(B, ctx, name, p, True, 0).rc == 0
    ctx.set_option("test_diag_shift_1e12", P.SHIFT_OPTION)
    for tries in range(P.TRIES_NEEDED):
        res = _run(B, ctx, name, p, False, tries)
        _check_failed(B, ctx, name, res, [k + 1] * m)
    res = _run(B, ctx, name, p, False, P.TRIES_NEEDED)
    assert res.rc == 0 and res.info == [0] * m and ctx.stat("sched_timeouts") == 0
    if _expected_schedule(ctx, name) is not None:
        assert ctx.stat("last_schedule") == _expected_schedule(ctx, name)
    np.testing.assert_allclose(res.jit, np.resize(p.jitter, m), rtol=1e-12, atol=0)
    if infer:
        # log-marginal and gradients against the oracle at the effective noise (gates of test_team_inference_equals_launched_inference)
        for j in range(m):
            fit = R.GPFit(p.kind, p.X, p.Y[j], 1.0, p.lengthscale[0], p.jitter[0] - P.SHIFT)
            np.testing.assert_allclose(res.lml[j], fit.log_marginal, rtol=1e-9)
            dv, dl, dn = fit.lml_gradients()
            np.testing.assert_allclose(res.grads[0][j], dv, rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(res.grads[1][j], dl, rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(res.grads[2][j], dn, rtol=1e-6, atol=1e-4 * abs(dn))
    if name == "fused128":
        pass                                                # (no model left behind)
    elif N <= P.KEEP_KY and name != "sharded":
        for j in range(m):
            L = _factor(B, ctx, N, j)[0]
            np.testing.assert_allclose(L.dot(L.T), p.Ky + p.jitter[0] * np.eye(N), rtol=0, atol=1e-10)
    else:
        # the predict gates of _against_oracle (test_gpu_round4.py), noiseless on both sides (the device's noise is 0, the oracle's the rung)
        mean, var = _predict(B, ctx, p, m)
        if N <= P.KEEP_KY:
            ref = R.MultiOutputGPRef(p.kind, np.ones(m), [p.lengthscale[0]] * m, [p.jitter[0] - P.SHIFT] * m)
            ref.updateModel(p.X, [p.Y[j][:, None] for j in range(m)])
            rm, rv = ref.predict_noiseless(_candidates(p))
        else:
            rm, rv = _big_reference(k)
        np.testing.assert_allclose(mean, rm, rtol=1e-5, atol=1e-6)
        assert np.abs(var - rv).max() <= 1e-5 * 1.0 + 1e-10
    _check_clean_fit_equals_fresh(B, ctx, name, p)
    ctx.close()


def test_ladder_through_the_model(B, probes):
    """multi_outputGP (five retries, fixed): model.jitter is the oracle's rung; when no rung survives LinAlgError names the output; the
    model fits again afterwards, bit for bit as a new model does."""
    N, k = 300, 129
    p = P.single(N, k)
    assert p.reference_gives_up_at_exhaust is True

    def model(X, shift):
        mod = B.multi_outputGP(1, kernel=[B.kern.Matern52(p.d, variance=1.0, lengthscale=p.lengthscale[0], ARD=True)], noise_var=[0.0], fixed_hyps=True)
        mod.incremental = False
        mod.set_option("test_diag_shift_1e12", shift)
        return mod

    Y = [p.Y[0][:, None]]
    mod = model(p.X, P.SHIFT_OPTION)
    mod.updateModel(p.X, Y)
    assert mod.jitter[0] == pytest.approx(p.jitter[0], rel=1e-12) and mod._context().stat("last_schedule") == 3
    L = mod.get_factor(0)[0]
    np.testing.assert_allclose(L.dot(L.T), p.Ky + p.jitter[0] * np.eye(N), rtol=0, atol=1e-10)
    mod.set_option("test_diag_shift_1e12", P.SHIFT_EXHAUST_OPTION)
    with pytest.raises(np.linalg.LinAlgError) as err:
        mod.updateModel(p.X, Y)
        mod.predict(_candidates(p))
    assert err.value.outputs == [0] and mod._context().stat("sched_timeouts") == 0
    mod.set_option("test_diag_shift_1e12", 0)
    mod.updateModel(p.X_clean, Y)
    fresh = model(p.X_clean, 0)
    fresh.updateModel(p.X_clean, Y)
    assert mod.jitter[0] == 0.0
    for a, b in zip(mod.get_factor(0) + mod.predict(_candidates(p)), fresh.get_factor(0) + fresh.predict(_candidates(p))):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------
# Case 5: per-output positions (the ARD construction): output 0 healthy, output 1 breaks at k1, output 2 at k2 < k1 in another panel.
PER_OUTPUT_CONFIGS = {"launched": 300, "team": 300, "hybrid": 3100}


@pytest.mark.parametrize("name", list(PER_OUTPUT_CONFIGS))
def test_per_output_positions_and_the_healthy_neighbour(B, probes, name):
    N, warm = PER_OUTPUT_CONFIGS[name], CONFIGS[name][3]
    p = P.per_output(N)
    factors = []
    for noise in (None, p.healthy_noise):                   # the problem; then the same with every output healthy
        ctx = _context(B, name)
        if warm:
            assert _run(B, ctx, name, p, True, 0, noise=p.healthy_noise).rc == 0
        ctx.set_option("test_diag_shift_1e12", P.SHIFT_OPTION)
        if noise is None:
            res = _run(B, ctx, name, p, False, 0)
            _check_failed(B, ctx, name, res, p.info)            # rc = the first failing OUTPUT's info (k1 + 1), not the smallest position
            assert res.rc == p.rc
        res = _run(B, ctx, name, p, False, P.TRIES_NEEDED, noise=noise)
        assert res.rc == 0 and res.info == [0, 0, 0] and ctx.stat("sched_timeouts") == 0
        assert ctx.stat("last_schedule") == _expected_schedule(ctx, name)
        if noise is None:
            assert res.jit[0] == 0.0
            np.testing.assert_allclose(res.jit[1:], p.jitter[1:], rtol=1e-12, atol=0)
            if N <= P.KEEP_KY:
                for j in range(3):
                    L = _factor(B, ctx, N, j)[0]
                    np.testing.assert_allclose(L.dot(L.T), p.Ky[j] + p.jitter[j] * np.eye(N), rtol=0, atol=1e-10)
        else:
            assert not res.jit.any()
        factors.append(_factor(B, ctx, N, 0))
        ctx.close()
    # the output that never failed: untouched by its neighbours' three failed rungs
    np.testing.assert_array_equal(factors[0][0], factors[1][0])
    np.testing.assert_array_equal(factors[0][1], factors[1][1])
