"""Pathwise posterior samples, CPU side: the NumPy restatement (tests/paths_ref.py) against what the method promises -- the identity at
the training inputs, the exact mean, the closed-form variance given the features, its own finite differences and its long-double twin --
the public surface, and CompositePathwiseThompsonBatch's draw order on a stand-in model that evaluates the restatement."""
import os
import sys

import numpy as np
import pytest
from scipy.linalg import cho_solve

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paths_ref as PR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from bocf_amd.acquisition_optimizer import samples_multidimensional_uniform  # noqa: E402
from bocf_amd.cbo import distinct_picks  # noqa: E402
from oracle import cpu_ref as R  # noqa: E402

ENTRY_POINTS = ["bocf_set_paths", "bocf_path_values", "bocf_path_utility"]


def _problem(kinds, N, d, seed, ls=0.4, noise=1e-2):
    """The model of the GPU tests (tests/test_gpu_paths.py _setup) on the oracle alone."""
    rng = np.random.RandomState(seed)
    m = len(kinds)
    X = rng.uniform(size=(N, d))
    Y = [np.sin(3 * X[:, :1] + j) + 0.3 * X[:, -1:] * (j + 1) for j in range(m)]
    var = 0.5 + rng.uniform(size=m)
    lss = [ls * (0.8 + 0.4 * rng.uniform(size=d)) for _ in range(m)]
    ref = R.MultiOutputGPRef(list(kinds), var, lss, [noise] * m)
    ref.updateModel(X, Y)
    return ref, X, Y, var, lss


@pytest.mark.parametrize("kind", ["rbf", "se", "matern52", "matern32"])
@pytest.mark.parametrize("N", [40, 300])
def test_identity_at_the_training_inputs(kind, N):
    """f_s(X_i) = Y_i - sqrt(nug) E_is - nug v_is (measured here 9e-15 ... 1.2e-13 for N = 40 ... 300)."""
    ref, X, Y, var, lss = _problem((kind,), N, 3, 3 + N)
    draws = PR.draw((kind,), N, 3, 130, 7, np.random.RandomState(N))
    P = PR.Paths(ref, Y, *draws)
    o = ref.output[0]
    nug = PR.nugget(o)
    want = Y[0] - np.sqrt(nug) * draws[3][0] - nug * P.v[0]
    err = np.max(np.abs(P.values(X)[0] - want))
    print("identity", kind, N, err)
    assert err <= 1e-10


@pytest.mark.parametrize("kind", ["rbf", "matern52", "matern32"])
def test_mean_and_variance_given_the_features(kind):
    """S = 4096 paths, F = 2048, N = 40, d = 2.  Given (omega, b) the path mean IS the posterior mean: within 5 standard errors
    (measured z <= 2.2 at these seeds).  The sample variance against the closed form |phi(x) - Phi(X)^T Ky^-1 k(X, x)|^2 + nug |Ky^-1 k(X, x)|^2: the
    relative standard error of a variance estimate from S Gaussian draws is sqrt(2 / S), the gate 5 of them = 0.11 (measured <= 0.06)."""
    N, d, F, S = 40, 2, 2048, 4096
    ref, X, Y, var, lss = _problem((kind,), N, d, 17)
    draws = PR.draw((kind,), N, d, F, S, np.random.RandomState(5))
    P = PR.Paths(ref, Y, *draws)
    Xq = np.random.RandomState(6).uniform(size=(25, d))
    f = P.values(Xq)[0]                                         # (n, S)
    o = ref.output[0]
    mu = o.posterior_mean(Xq)[:, 0]
    se = f.std(axis=1, ddof=1) / np.sqrt(S)
    z = np.abs(f.mean(axis=1) - mu) / se
    print("mean z", kind, z.max())
    assert z.max() <= 5.0
    nug = PR.nugget(o)
    A = cho_solve((o.L, True), R.kern_K(o.kind, o.X, Xq, o.variance, o.lengthscale))        # (N, n)
    resid = PR.features(o, draws[0][0], draws[1][0], Xq) - A.T.dot(PR.features(o, draws[0][0], draws[1][0], o.X))   # (n, F)
    closed = np.sum(resid ** 2, axis=1) + nug * np.sum(A ** 2, axis=0)
    dev = np.abs(f.var(axis=1, ddof=1) / closed - 1.0)
    print("variance deviation", kind, dev.max())
    assert dev.max() <= 5.0 * np.sqrt(2.0 / S)


@pytest.mark.parametrize("kinds", [("rbf", "matern52"), ("se", "matern32")])
def test_gradient_against_central_differences(kinds):
    """The restatement's analytic gradient against central differences of its own values: step 1e-6, values O(1) with third derivatives
    O(1 / l^3) ~ 30, so truncation ~ 5e-12 and rounding ~ 1e-16 / 1e-6 = 1e-10 times the cancellation in f (|v| ~ 1e2): gate 1e-6."""
    d = 3
    ref, X, Y, var, lss = _problem(kinds, 60, d, 8)
    draws = PR.draw(kinds, 60, d, 130, 4, np.random.RandomState(2))
    P = PR.Paths(ref, Y, *draws)
    Xq = np.random.RandomState(3).uniform(size=(6, d))
    G = P.gradients(Xq)
    h = 1e-6
    for q in range(d):
        e = np.zeros(d)
        e[q] = h
        fd = (P.values(Xq + e) - P.values(Xq - e)) / (2 * h)
        np.testing.assert_allclose(G[..., q], fd, rtol=0, atol=1e-6)
    # and through a utility: neg_sq_dist on mixed paths
    th = np.random.RandomState(4).normal(size=(4, 2))
    rows = np.array([0, 3, 1, 1, 2, 0])
    u, du = P.utility(Xq, rows, th, "neg_sq_dist", grad=True)
    for q in range(d):
        e = np.zeros(d)
        e[q] = h
        fd = (P.utility(Xq + e, rows, th, "neg_sq_dist") - P.utility(Xq - e, rows, th, "neg_sq_dist")) / (2 * h)
        np.testing.assert_allclose(du[:, q], fd, rtol=0, atol=1e-5)


def test_restatement_against_its_long_double_twin():
    """At the GPU tests' conditioning (noise 1e-2, lengthscales 0.4 (0.8 ... 1.2), N = 300, F = 130, S = 64) the fp64 restatement is within
    1e-12 of the long-double one (measured 2.2e-13): about 500 times below the GPU tests' gate."""
    kinds = ("rbf", "matern52", "matern32")
    ref, X, Y, var, lss = _problem(kinds, 300, 3, 11)
    draws = PR.draw(kinds, 300, 3, 130, 64, np.random.RandomState(1))
    Xq = np.random.RandomState(2).uniform(size=(40, 3))
    f = PR.Paths(ref, Y, *draws).values(Xq)
    ld = PR.values_ld(ref, Y, *draws, Xq)
    err = float(np.max(np.abs(f - ld)))
    print("fp64 restatement vs long double", err)
    assert err <= 1e-12


def test_public_surface():
    for name in ENTRY_POINTS:
        assert name in _ffi.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bocf_hip.h")).read()
    for name in ENTRY_POINTS:
        assert "int %s(" % name in header
    for name in ("draw_paths", "path_values", "path_utility", "pathwise_topk"):
        assert callable(getattr(B.multi_outputGP, name))
    assert "paths" in B.multi_outputGP(1, fixed_hyps=True)._resident.__slots__
    assert B.CompositePathwiseThompsonBatch is not None
    with pytest.raises(ValueError):
        B.CompositePathwiseThompsonBatch(None, 0)
    with pytest.raises(ValueError):
        B.CompositePathwiseThompsonBatch(None, 65)


def test_the_host_record_of_the_paths_is_forgotten_with_the_posterior():
    """`paths` of _Resident goes where the library drops the paths: a new fit, new data, pickling; not with a candidate upload."""
    import pickle
    model = B.multi_outputGP(1, fixed_hyps=True)
    model._resident.paths = {"serial": 0}
    model._resident.forget("candidates")
    assert model._resident.paths is not None
    assert pickle.loads(pickle.dumps(model))._resident.paths is None
    import inspect
    src = inspect.getsource(sys.modules[B.multi_outputGP.__module__])
    for fn in ("def updateModel", "def _refactorized", "def _fit"):
        body = src[src.index(fn):]
        body = body[:body.index("\n    def ", 10)]
        assert '"paths"' in body, fn


# ---- the evaluator's draw order on a stand-in model ----------------------------------------------------------------------------------
class _StandIn(object):
    """What CompositePathwiseThompsonBatch asks of a model, answered by the restatement; draw_paths draws in the documented order."""
    output_dim = 2
    kinds = ("rbf", "matern52")

    def __init__(self):
        self.ref, self.X, self.Y, _, _ = _problem(self.kinds, 30, 2, 5)
        self.paths = None
        self.utility_calls = 0

    def number_of_hyps_samples(self):
        return 10

    def draw_paths(self, n_paths, n_features=1024):
        self.paths = PR.Paths(self.ref, self.Y, *PR.draw(self.kinds, 30, 2, n_features, n_paths))

    def pathwise_topk(self, X, thetas, path_groups, utility, k):
        F = self.paths.values(X)
        idx = np.stack([np.lexsort((np.arange(X.shape[0]), -R.utility_eval("neg_sq_dist", thetas[s], F[:, :, s])))[:k] for s in range(len(thetas))])
        return idx, None

    def path_utility(self, X, row_path, thetas, utility, grad=False):
        self.utility_calls += 1
        return self.paths.utility(X, row_path, thetas, "neg_sq_dist", grad=grad)


class _Acq(object):
    def __init__(self, model, space, utility):
        self.model, self.space, self.utility = model, space, utility

    def optimize(self, x_baseline=None):
        return np.array([[0.5, 0.5]]), 0.0


def _stand_in_batch(refine, seed=31, q=4, C=200, F=64):
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9], [0.3, 0.3]]), prob_dist=np.full(3, 1.0 / 3)),
                  device="neg_sq_dist")
    model = _StandIn()
    ev = B.CompositePathwiseThompsonBatch(_Acq(model, space, U), q, n_candidates=C, n_features=F, refine=refine)
    np.random.seed(seed)
    return ev, model, space, U, ev.compute_batch()


def test_evaluator_draw_order():
    """design, then theta, then the paths' draws (per output z, chi2 for Matern, b, w, E): replayed by hand from the same seed."""
    q, C, F = 4, 200, 64
    ev, model, space, U, batch = _stand_in_batch(False, q=q, C=C, F=F)
    np.random.seed(31)
    Xc = samples_multidimensional_uniform([(0.0, 1.0), (0.0, 1.0)], C)
    thetas = np.asarray(U.parameter_dist.sample(q - 1), dtype=float).reshape(q - 1, -1)
    paths = PR.Paths(model.ref, model.Y, *PR.draw(model.kinds, 30, 2, F, q - 1))
    Fv = paths.values(Xc)
    idx = np.stack([np.lexsort((np.arange(C), -R.utility_eval("neg_sq_dist", thetas[s], Fv[:, :, s])))[:q] for s in range(q - 1)])
    np.testing.assert_array_equal(batch, np.vstack(([[0.5, 0.5]], Xc[distinct_picks(idx)])))


def test_evaluator_refinement_keeps_what_is_not_worse():
    ev, model, space, U, batch = _stand_in_batch(True)
    rec = ev.last_refinement
    assert batch.shape == (4, 2) and np.all(batch >= 0.0) and np.all(batch <= 1.0)
    assert model.utility_calls >= 3
    for s in range(3):
        want = rec["refined"][s] if rec["kept"][s] else rec["picks"][s]
        np.testing.assert_array_equal(batch[1 + s], want)
        if rec["kept"][s]:
            assert rec["refined_values"][s] >= rec["pick_values"][s]
    assert np.any(rec["refined_values"] > rec["pick_values"])       # the refinement does move a pick of a 200-point design uphill
