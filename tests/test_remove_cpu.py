"""Removal of an observation from the resident factor, on the CPU: the NumPy statement of the algorithm (tests/remove_ref.py) against the
oracle refitted on the N - 1 remaining points, the proof on the oracle alone that every removal the device test makes changes the
posterior by more than that test's gates, and the row matching of multi_outputGP.updateModel.

Gates: U and R = U^-1 at the L gate of tests/test_gpu_incremental.py (rtol 1e-6 / atol 1e-9) -- every step is an orthogonal
transformation, so the update itself adds ~ eps N to a factor whose own uncertainty is eps cond(Ky) <= 2.2e-16 x 1e7."""
import os
import sys

import numpy as np
import pytest
from scipy.linalg import solve_triangular

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remove_ref as RR  # noqa: E402
import test_gpu_incremental as G  # noqa: E402  (its problems and helpers; none of its tests is collected from here)

from oracle import cpu_ref as R  # noqa: E402
from bocf_amd.multi_outputGP import match_removed_row  # noqa: E402


def factor(kind, p, X, Y, j=0):
    fit = R.GPFit(kind, X, Y, p["variances"][j], p["lengthscales"][j], p["noise"][j])
    assert fit.jitter == 0
    U = np.ascontiguousarray(fit.L.T)
    return U, solve_triangular(U, np.eye(U.shape[0]), lower=False)


def assert_factor(Un, Rn, U_ref, R_ref):
    n = U_ref.shape[0]
    assert Un.shape == (n, n) and Rn.shape == (n, n)
    assert np.all(np.diag(Un) > 0) and np.all(np.diag(Rn) > 0)
    assert not np.any(np.tril(Un, -1)) and not np.any(np.tril(Rn, -1))             # exact zeros, not 1e-16 residue
    np.testing.assert_allclose(Un, U_ref, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(Rn, R_ref, rtol=1e-6, atol=1e-9)


CASES = [(N, k) for N in (2, 129, 300) for k in sorted({0, 1, 127, 128, N - 2, N - 1}) if 0 <= k < N]


@pytest.mark.parametrize("N,k", CASES, ids=["N%d-k%d" % c for c in CASES])
def test_restatement_against_the_oracle_refitted(N, k):
    p = G.problem(N, 3, 1, 1e-6, 40 + N)
    U, Rm = factor("matern52", p, p["X"], p["Y"][0])
    Xr, Yr = RR.without(p, k)
    U_ref, R_ref = factor("matern52", p, Xr, Yr[0])
    Un, Rn, last = RR.remove(U, Rm, k)
    assert last <= 1e-12 * np.abs(U).max()                 # the row that is dropped
    assert_factor(Un, Rn, U_ref, R_ref)
    Up, Rp = RR.remove_prefix(U, Rm, k)                    # the form the kernels evaluate
    assert_factor(Up, Rp, U_ref, R_ref)
    np.testing.assert_allclose(Up, Un, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(Rp, Rn, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("form", ["rotations", "prefix"])
def test_chain_of_127_removals(form):
    """N = 300 -> 173, every third removal at index 0 (all rotations), the others random; compared with a refit at the end and on the way."""
    N = 300
    p = G.problem(N, 3, 1, 1e-6, 41)
    X, Y = p["X"], p["Y"][0]
    U, Rm = factor("matern52", p, X, Y)
    rng = np.random.RandomState(3)
    for step in range(127):
        k = 0 if step % 3 == 0 else int(rng.randint(U.shape[0]))
        X, Y = np.delete(X, k, axis=0), np.delete(Y, k, axis=0)
        U, Rm = RR.remove(U, Rm, k)[:2] if form == "rotations" else RR.remove_prefix(U, Rm, k)
        if step in (63, 126):
            U_ref, R_ref = factor("matern52", p, X, Y)
            err_u = np.abs(U - U_ref).max() / np.abs(U_ref).max()
            err_r = np.abs(Rm - R_ref).max() / np.abs(R_ref).max()
            print("after %d removals (%s): U %.2e, R %.2e relative to a refit" % (step + 1, form, err_u, err_r))
            assert_factor(U, Rm, U_ref, R_ref)
            np.testing.assert_allclose(Rm.dot(U), np.eye(U.shape[0]), atol=1e-9)
    assert U.shape[0] == N - 127


@pytest.mark.parametrize("N,k,m,d,kind,noise", RR.BOUNDARY, ids=["N%d-k%d-m%d-d%d-%s-%g" % c for c in RR.BOUNDARY])
def test_every_removal_of_the_device_test_matters(N, k, m, d, kind, noise):
    """The N-point and the (N - 1)-point oracle differ at the candidates by more than the device test's mean and variance gates (rtol 1e-6 /
    atol 1e-7 and 1e-9): a removal that silently did nothing could not pass there.  The N - 1 points factorize with zero jitter and their
    log-marginals do not cancel (what tests/test_gpu_remove.py relies on)."""
    kinds = G.kinds_of(kind, m)
    p = RR.make_outlier(G.problem(N, d, m, noise, RR.boundary_seed(N, k, m)), k)
    full = G.oracle(kinds, p, p["X"], p["Y"])
    Xr, Yr = RR.without(p, k)
    less = G.oracle(kinds, p, Xr, Yr)
    assert G.lml_cancellation(less) > 0.05
    (m0, v0), (m1, v1) = full.predict(p["Xc"]), less.predict(p["Xc"])
    for j in range(m):                                     # every output, so that one left behind would show
        assert np.max(np.abs(m0[j] - m1[j]) - (1e-7 + 1e-6 * np.abs(m1[j]))) > 0
        assert np.abs(v0[j] - v1[j]).max() > 1e-9
    assert not np.allclose([o.log_marginal for o in full.output], [o.log_marginal for o in less.output], rtol=1e-9)


# ---- the row matching of updateModel
def _X(n=7, d=3, seed=0):
    return np.random.RandomState(seed).uniform(size=(n, d))


@pytest.mark.parametrize("k", [0, 3, 6])
def test_match_one_row_deleted(k):
    X = _X()
    assert match_removed_row(X, np.delete(X, k, axis=0)) == (k, False)


@pytest.mark.parametrize("k", [0, 3, 6])
def test_match_delete_plus_append(k):
    X = _X()
    new = np.vstack([np.delete(X, k, axis=0), [[0.5, 0.25, 0.125]]])
    assert match_removed_row(X, new) == (k, True)


def test_match_duplicates_give_a_consistent_index():
    X = _X()
    X[4] = X[3]
    X[5] = X[3]
    for k in (3, 4, 5):
        after = np.delete(X, k, axis=0)
        hit = match_removed_row(X, after)
        assert hit is not None and hit[1] is False and hit[0] in (3, 4, 5)
        np.testing.assert_array_equal(np.delete(X, hit[0], axis=0), after)
        hit = match_removed_row(X, np.vstack([after, X[:1] + 1.0]))
        assert hit is not None and hit[1] is True
        np.testing.assert_array_equal(np.delete(X, hit[0], axis=0), after)


def test_match_refuses_every_other_change():
    X = _X()
    assert match_removed_row(X, np.delete(X, [1, 4], axis=0)) is None              # two rows deleted
    assert match_removed_row(X, np.vstack([np.delete(X, [1, 4], axis=0), X[:1] + 1.0])) is None
    changed = X.copy()
    changed[2, 1] += 1e-9
    assert match_removed_row(X, changed) is None                                   # a changed row, same shape
    assert match_removed_row(X, np.delete(changed, 5, axis=0)) is None             # a changed row and a deleted one
    assert match_removed_row(X, np.vstack([X, X[:1]])) is None                     # an append (updateModel's own case)
    assert match_removed_row(X, np.vstack([X, X[:2]])) is None
    assert match_removed_row(X, X[:, :2]) is None                                  # another input dimension
    assert match_removed_row(X[:1], X[:0]) is None                                 # the only observation
    perm = X[::-1].copy()
    assert match_removed_row(X, perm) is None


def test_match_a_changed_last_row_is_a_removal_and_an_append():
    """Replacing the last row IS deleting it and appending another: the one change of a row the matcher describes."""
    X = _X()
    changed = X.copy()
    changed[-1] += 0.5
    assert match_removed_row(X, changed) == (6, True)


# ---- the library calls of a removal, entry for entry (the recording stand-in of tests/test_model_calls_cpu.py: no library, no GPU)
def _calls(monkeypatch, steps, returns=None):
    import bocf_amd as B
    from bocf_amd import _ffi
    import test_model_calls_cpu as MC
    lib = MC.RecordingLibrary()
    lib.returns.update(returns or {})
    monkeypatch.setattr(_ffi, "load", lambda: lib)
    rng = np.random.RandomState(0)
    X, Y = rng.uniform(size=(9, 3)), [rng.normal(size=(9, 1)) for _ in range(2)]
    model = B.multi_outputGP(2, fixed_hyps=True, noise_var=[1e-4] * 2)
    model.updateModel(X[:8], [y[:8] for y in Y])
    del lib.calls[:]
    steps(model, X, Y)
    return [[c[0], c[2]] if c[0] == "bocf_remove" else c[:1] for c in lib.calls if c[0] in ("bocf_fit", "bocf_remove", "bocf_append", "bocf_update_targets")]


def test_update_model_with_a_deleted_row_refits_unless_asked(monkeypatch):
    rows = [0, 1, 2, 4, 5, 6, 7]

    def deleted(model, X, Y):
        model.updateModel(X[rows], [y[rows] for y in Y])
    assert _calls(monkeypatch, deleted) == [["bocf_fit"]]                          # the default: as it always was

    def asked(model, X, Y):
        model.incremental_remove = True
        model.updateModel(X[rows], [y[rows] for y in Y])
        model.updateModel(X[rows[1:] + [8]], [y[rows[1:] + [8]] for y in Y])       # the window slides: row 0 leaves, row 8 arrives
    assert _calls(monkeypatch, asked) == [["bocf_remove", 3], ["bocf_remove", 0], ["bocf_append"]]


def test_refused_removals_and_appends_become_one_refit(monkeypatch):
    rows = [0, 1, 2, 4, 5, 6, 7]

    def slide(model, X, Y):
        model.incremental_remove = True
        model.updateModel(X[rows + [8]], [y[rows + [8]] for y in Y])
    assert _calls(monkeypatch, slide, {"bocf_remove": [1]}) == [["bocf_remove", 3], ["bocf_fit"]]
    assert _calls(monkeypatch, slide, {"bocf_append": [1]}) == [["bocf_remove", 3], ["bocf_append"], ["bocf_fit"]]

    def explicit(model, X, Y):
        model.remove_observations([1, 6])
        assert model._X.shape == (6, 3) and all(y.shape == (6, 1) for y in model._Y)
    assert _calls(monkeypatch, explicit) == [["bocf_remove", 6], ["bocf_remove", 1]]                      # from the highest index down
    assert _calls(monkeypatch, explicit, {"bocf_remove": [0, 1]}) == [["bocf_remove", 6], ["bocf_remove", 1], ["bocf_fit"]]
