"""CompositeThompsonBatch and the CBO loop's batch handling on the CPU: a fake model stands in for the device (model.thompson_topk)."""
import numpy as np
import pytest

import bocf_amd
from bocf_amd.acquisition_optimizer import samples_multidimensional_uniform
from bocf_amd.cbo import CBO, CompositeThompsonBatch, Sequential, distinct_picks


class FakeDist(object):
    def __init__(self, dim):
        self.dim = dim
        self.use_full_support = False

    def sample(self, n):
        return np.random.uniform(size=(n, self.dim))


class FakeUtility(object):
    def __init__(self, dim):
        self.parameter_dist = FakeDist(dim)


class FakeModel(object):
    """Records the thompson_topk calls; path s ranks the candidates by the fixed order `ranking[s]` (or candidate s, s + 1, ...)."""

    def __init__(self, m=2, n_hyps=1, ranking=None):
        self.output_dim, self.n_hyps, self.ranking, self.calls = m, n_hyps, ranking, []

    def number_of_hyps_samples(self):
        return self.n_hyps

    def thompson_topk(self, X, thetas, path_groups, Z, utility, k):
        self.calls.append(dict(X=X.copy(), thetas=np.array(thetas), groups=np.array(path_groups), Z={h: z.copy() for h, z in Z.items()}, k=k))
        P = len(path_groups)
        if self.ranking is not None:
            idx = np.asarray(self.ranking)[:, :k]
        else:
            idx = (np.arange(P)[:, None] + np.arange(k)[None, :]) % X.shape[0]
        return idx, -np.arange(k, dtype=float)[None, :].repeat(P, 0)


class FakeAcq(object):
    def __init__(self, model, bounds, m=2):
        self.model, self.space, self.utility = model, bounds, FakeUtility(m)
        self.optimize_calls = []

    def optimize(self, duplicate_manager=None, x_baseline=None):
        self.optimize_calls.append(x_baseline)
        return np.full((1, len(self.space)), 0.5), np.zeros((1, 1))


BOUNDS = [(0.0, 1.0), (-2.0, 3.0), (5.0, 6.0)]


def test_rng_order_of_compute_batch():
    model = FakeModel(m=2, n_hyps=3)
    acq = FakeAcq(model, BOUNDS)
    ev = CompositeThompsonBatch(acq, 6, n_candidates=50)
    np.random.seed(7)
    X = ev.compute_batch(x_baseline=np.zeros((1, 3)))
    # the same draws, replayed in the documented order
    np.random.seed(7)
    Xc = samples_multidimensional_uniform(BOUNDS, 50)
    th = np.random.uniform(size=(5, 2))
    groups = np.arange(5) % 3
    Z = {h: np.random.normal(size=(2, 50, int(np.sum(groups == h)))) for h in range(3)}
    after = np.random.uniform()
    call = model.calls[0]
    np.testing.assert_array_equal(call["X"], Xc)
    np.testing.assert_array_equal(call["thetas"], th)
    np.testing.assert_array_equal(call["groups"], groups)
    assert sorted(call["Z"]) == [0, 1, 2]
    for h in range(3):
        np.testing.assert_array_equal(call["Z"][h], Z[h])
    assert call["k"] == 6
    np.random.seed(7)
    samples_multidimensional_uniform(BOUNDS, 50); np.random.uniform(size=(5, 2))
    for h in range(3):
        np.random.normal(size=(2, 50, int(np.sum(groups == h))))
    assert np.random.uniform() == after
    assert X.shape == (6, 3)
    np.testing.assert_array_equal(X[0], np.full(3, 0.5))
    np.testing.assert_array_equal(X[1:], Xc[np.arange(5)])


def test_batch_size_one_is_sequential():
    model = FakeModel()
    acq = FakeAcq(model, BOUNDS)
    np.random.seed(3)
    x = CompositeThompsonBatch(acq, 1).compute_batch(x_baseline=np.ones((1, 3)))
    state = np.random.get_state()[1].copy()
    np.random.seed(3)
    y = Sequential(acq).compute_batch(x_baseline=np.ones((1, 3)))
    np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(state, np.random.get_state()[1])       # nothing more was drawn
    assert model.calls == []
    assert len(acq.optimize_calls) == 2 and np.all(acq.optimize_calls[0] == 1.0)


def test_paths_sharing_an_argmax_take_distinct_candidates():
    ranking = [[4, 1, 2, 3], [4, 2, 1, 3], [2, 4, 1, 0]]
    model = FakeModel(ranking=ranking)
    acq = FakeAcq(model, BOUNDS)
    np.random.seed(0)
    X = CompositeThompsonBatch(acq, 4, n_candidates=8).compute_batch()
    Xc = model.calls[0]["X"]
    np.testing.assert_array_equal(X[1:], Xc[[4, 2, 1]])
    np.testing.assert_array_equal(distinct_picks(ranking), [4, 2, 1])
    with pytest.raises(RuntimeError):
        distinct_picks([[1, 2], [2, 1], [1, 2]])


@pytest.mark.parametrize("n_hyps,q", [(1, 5), (4, 11), (25, 16)])
def test_path_to_hyper_sample_mapping(n_hyps, q):
    model = FakeModel(n_hyps=n_hyps)
    np.random.seed(1)
    CompositeThompsonBatch(FakeAcq(model, BOUNDS), q, n_candidates=64).compute_batch()
    call = model.calls[0]
    n_h = min(10, n_hyps)
    np.testing.assert_array_equal(call["groups"], np.arange(q - 1) % n_h)
    used = sorted(set((np.arange(q - 1) % n_h).tolist()))
    assert sorted(call["Z"]) == used
    for h in used:
        assert call["Z"][h].shape == (2, 64, int(np.sum(np.arange(q - 1) % n_h == h)))


def test_batch_size_bounds():
    acq = FakeAcq(FakeModel(), BOUNDS)
    with pytest.raises(ValueError):
        CompositeThompsonBatch(acq, 0)
    with pytest.raises(ValueError):
        CompositeThompsonBatch(acq, 9, n_candidates=8)
    assert bocf_amd.CompositeThompsonBatch is CompositeThompsonBatch


class _Space(object):
    def round_optimum(self, x):
        return np.atleast_2d(x)


class _Batch(object):
    def __init__(self, rows):
        self.rows = rows

    def compute_batch(self, duplicate_manager=None, context_manager=None, x_baseline=None):
        return self.rows


def _loop(rows, X_init):
    bo = CBO.__new__(CBO)
    bo.space, bo.evaluator, bo.suggested_sample, bo.X = _Space(), _Batch(rows), X_init, X_init
    bo.compute_next_evaluations = lambda: rows
    seen = {}

    class _Acq(object):
        def update_Z_samples(self):
            pass

    bo.acquisition = _Acq()
    bo.evaluate_objective = lambda: seen.setdefault("x", bo.suggested_sample.copy())
    bo.num_acquisitions, bo.model_update_interval = 0, 1
    bo._update_model = lambda: None

    class _Model(object):
        def get_model_parameters_names(self):
            pass

        def get_model_parameters(self):
            pass

    bo.model, bo.full_parameter_support, bo.verbosity = _Model(), True, False
    bo._current_max_value = lambda: 0.0
    bo.historical_optimal_values, bo.historical_time, bo.time_zero = [], [], 0.0
    bo._one_iteration(False)
    return bo, seen["x"]


def test_one_iteration_accepts_a_batch_after_a_differently_sized_X_init():
    X_init = np.random.RandomState(0).uniform(size=(5, 3))
    rows = np.random.RandomState(1).uniform(size=(4, 3))
    bo, x = _loop(rows, X_init)
    np.testing.assert_array_equal(x, rows)                # not a repeat: used as it is
    assert bo.X.shape == (9, 3)


def test_one_iteration_perturbs_a_repeated_batch_and_keeps_the_single_row_broadcast():
    rows = np.random.RandomState(1).uniform(size=(4, 3))
    np.random.seed(5)
    _, x = _loop(rows, rows.copy())
    assert x.shape == rows.shape and not np.all(x == rows)
    # q = 1: a row equal to every row of X_init (broadcast) counts as repeated, exactly as before
    one = np.array([[0.2, 0.3, 0.4]])
    _, x1 = _loop(one, np.repeat(one, 3, axis=0))
    assert not np.all(x1 == one)
    _, x2 = _loop(one, np.vstack((one, one + 1)))
    np.testing.assert_array_equal(x2, one)
