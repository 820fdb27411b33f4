"""The library calls the host side makes, entry for entry: which bocf_* function, with which scalars, in which order -- and which
uploads are NOT repeated because the host knows the buffer is resident (W, Z, the utility program, the reference set, the candidates,
the all-hyper-sample query caches).  `_ffi.load` is replaced by a recording stand-in, so no library and no GPU is needed.

The expected trace, tests/golden/model_calls.json, was recorded with this module (`python tests/test_model_calls_cpu.py`) against the
commit BEFORE the residency record / utility table refactor (the third scenario: against the commit before the model's acquisition
tails were folded into _run_acq / _select_paths); it also holds one np.random.random() drawn after each scenario, which
pins the number and the order of the global-RNG draws.  The stand-in leaves output arrays uninitialised: no scenario branches on a
returned value.  Record again only when a change is MEANT to alter the calls."""
import json
import numbers
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "model_calls.json")
N, D, M, C, L, S = 12, 3, 2, 5, 3, 4


class RecordingLibrary(object):
    """Every bocf_* attribute appends [name, arg, ...] to `calls` and returns 0 (or the next value queued for it in `returns`)."""

    def __init__(self):
        self.calls, self.returns = [], {}

    def mark(self, text):
        self.calls.append(["#", text])

    def __getattr__(self, name):
        if not name.startswith("bocf_"):
            raise AttributeError(name)

        def call(*args):
            rec = [name]
            for a in args:
                if a is None:
                    rec.append(None)
                elif isinstance(a, numbers.Integral):
                    rec.append(int(a))
                elif isinstance(a, numbers.Real):
                    rec.append(float(a))
                elif isinstance(a, bytes):
                    rec.append(len(a) if name == "bocf_set_utility_program" else a.decode())
                else:
                    rec.append("p")
            self.calls.append(rec)
            if name == "bocf_create":
                args[1]._obj.value = 1
            if name == "bocf_last_error":
                return b""
            queued = self.returns.get(name)
            return queued.pop(0) if queued else 0
        return call


def _space():
    return B.Design_space([{"name": "x%d" % q, "type": "continuous", "domain": (0.0, 1.0)} for q in range(D)])


def _dist(support, prob=None):
    support = np.asarray(support, dtype=float)
    return B.ParameterDistribution(support=support, prob_dist=np.full(len(support), 1.0 / len(support)) if prob is None else np.asarray(prob))


def abs15(t, y):
    return -np.sum(np.abs((np.asarray(y).T - t).T) ** 1.5, axis=0)


def _data(rng):
    return rng.uniform(size=(N, D)), [rng.normal(size=(N, 1)) for _ in range(M)]


def scenario_fixed(lib):
    rng = np.random.RandomState(0)
    np.random.seed(1)
    X, Y = _data(rng)
    Xc = rng.uniform(size=(C, D))
    support, prob = rng.uniform(size=(L, M)), np.array([0.2, 0.3, 0.5])
    wide = rng.uniform(size=(24, M))                          # >= 20 rows: not "full support", thetas are sampled
    model = B.multi_outputGP(M, fixed_hyps=True, noise_var=[1e-4] * M)
    lib.mark("updateModel")
    model.updateModel(X, Y)
    U = B.Utility(parameter_dist=_dist(support, prob), device="neg_sq_dist")
    lib.mark("uEI value twice, gradient, top-k")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq._compute_acq(Xc)
    acq._compute_acq(Xc)
    acq._compute_acq_withGradients(Xc[:1])
    model.select_topk(3)
    acq.select_anchors(2)
    lib.mark("append one row")
    X = np.vstack([X, rng.uniform(size=(1, D))])
    Y = [np.vstack([y, rng.normal(size=(1, 1))]) for y in Y]
    model.updateModel(X, Y)
    acq._compute_acq(Xc)
    lib.mark("same X, new Y")
    Y = [y + 0.1 for y in Y]
    model.updateModel(X, Y)
    acq._compute_acq_withGradients(Xc[:1])
    lib.mark("append refused by the device: refit")
    lib.returns["bocf_append"] = [1]
    X = np.vstack([X, rng.uniform(size=(1, D))])
    Y = [np.vstack([y, rng.normal(size=(1, 1))]) for y in Y]
    model.updateModel(X, Y)
    acq._compute_acq(Xc)
    lib.mark("expected utility")
    rows = np.arange(C) % L
    Z = rng.normal(size=(L, S, M))
    for mode in ("mean", "closed", "mc"):
        for grad in (False, True):
            model.expected_utility(Xc, mode, U, support, rows, Z=Z if mode == "mc" else None, grad=grad)
    model.expected_utility(None, _ffi.EU_CLOSED, "neg_sum_exp", np.zeros((L, 1)), rows)
    model.expected_utility(Xc[:2], "closed", _ffi.UTIL_ROSENBROCK, support[:, :1], rows[:2], n_hyps=3, grad=True, util_params=None)
    lib.mark("closed-form acquisitions")
    U_lin = B.Utility(func=lambda t, y: np.dot(t, y), parameter_dist=_dist(support, prob), linear=True)
    ei = B.maEI(model, None, utility=U_lin)
    ei._compute_acq(Xc)
    ei._compute_acq_withGradients(Xc[:1])
    pi = B.maPI(model, None, utility=B.Utility(func=lambda t, y: np.dot(t, y), parameter_dist=_dist(wide), linear=True))
    pi._compute_acq(Xc)                                       # draws 10 thetas
    pi._compute_acq_withGradients(Xc[:1])                     # draws 3
    lib.mark("Monte-Carlo acquisitions, sampled thetas, a utility that does not read theta")
    U_exp = B.Utility(parameter_dist=_dist(wide), device="neg_sum_exp")
    mc = B.uEI_noiseless(model, None, utility=U_exp)          # W (25, m), then ten thetas
    mc._compute_acq(Xc)
    mc._compute_acq_withGradients(Xc[:1])                     # one fresh theta
    B.uPI(model, None, utility=B.Utility(parameter_dist=_dist(support, prob), device="neg_exp_cos", device_params=np.ones(M)))._compute_acq(Xc)
    lib.mark("the resident entry points of the benchmark")
    n = model._set_candidates(Xc)
    model.set_mc_samples(acq.W_samples)
    model._acq_mc_resident(_ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, n, fetch=False)
    model._acq_mc_resident(_ffi.ACQ_PI, _ffi.UTIL_NEG_SUM_EXP, None, None, None, n)
    model.acq_mc(None, _ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, support, None)
    lib.mark("knowledge gradient")
    kg = B.uKG(model, _space(), utility=U, n_fantasies=S, n_ref_points=4)
    kg._compute_acq(Xc)                                       # draws the reference points
    kg._compute_acq_withGradients(Xc[:1])                     # same fit: nothing drawn, nothing staged
    model.updateModel(X, [y - 0.1 for y in Y])
    kg._compute_acq(Xc)                                       # new fit serial: drawn and staged again
    kg.set_reference_points(rng.uniform(size=(3, D)))
    kg._compute_acq(Xc)
    kg._compute_acq_withGradients(Xc[:1])
    kg_mc = B.uKG(model, _space(), utility=B.Utility(parameter_dist=_dist(wide), device="neg_exp_cos", device_params=np.ones(M)),
                  n_fantasies=S, n_ref_points=1)
    kg_mc._compute_acq(Xc)
    B.uKG(model, _space(), utility=U_lin, n_fantasies=S, n_ref_points=2)._compute_acq_withGradients(Xc[:1])
    lib.mark("utility program")
    U_prog = B.Utility(func=abs15, parameter_dist=_dist(support, prob), device="program")
    prog = B.uEI_noiseless(model, None, utility=U_prog)
    prog._compute_acq(Xc)
    prog._compute_acq(Xc)
    prog._compute_acq_withGradients(Xc[:1])
    model.expected_utility(Xc, "mc", U_prog, support, rows, Z=Z)
    lib.mark("Thompson")
    groups = [0, 1, 0]
    Zt = {0: rng.normal(size=(M, C, 2)), 1: rng.normal(size=(M, C, 1))}
    model.thompson_topk(Xc, support, groups, Zt, U, 2)
    model.thompson_topk(Xc, support, groups, Zt, U_prog, 2)
    model.posterior_samples_f(Xc, size=2)                     # draws (m, n, 2) normals
    lib.mark("predictions")
    model.predict(Xc, full_cov=True)
    model.predict(Xc)
    model.predict_noiseless(Xc)
    model.posterior_mean(Xc)
    model.posterior_variance_noiseless(Xc)
    model.posterior_mean_gradient(Xc)
    model.posterior_mean_at_evaluated_points()
    model.posterior_covariance_between_points(Xc, Xc[:2])
    model.get_factor(1)
    model.log_likelihood_gradients()
    lib.mark("look-ahead")
    model.partial_precomputation_for_covariance(Xc[:2])
    model.posterior_covariance_between_points_partially_precomputed(Xc, Xc[:2])
    model.partial_precomputation_for_variance_conditioned_on_next_point(Xc[:1])
    model.posterior_variance_conditioned_on_next_point(Xc)
    model.posterior_variance_gradient_conditioned_on_next_point(Xc)
    model.posterior_covariance_gradient(Xc, Xc[1:2])
    model.partial_precomputation_for_covariance_gradient(Xc[1:2])
    model.posterior_covariance_gradient_partially_precomputed(Xc, Xc[1:2])
    model.set_reference_points(Xc[:2])
    model.set_reference_points(Xc[:2])
    model.acq_kg(Xc, "closed", _ffi.UTIL_NEG_SQ_DIST, None, support, prob, rng.normal(size=(S, M)), fetch=False)
    lib.mark("a fit the device gives up on")
    lib.returns["bocf_fit"] = [2]
    try:
        model.updateModel(X[:-1], [y[:-1] for y in Y])
        raise AssertionError("LinAlgError expected")
    except np.linalg.LinAlgError:
        pass
    acq._compute_acq(Xc)
    lib.mark("pickle")
    clone = pickle.loads(pickle.dumps(model))
    clone.posterior_mean(Xc)
    acq.model = clone
    acq._compute_acq(Xc)


def scenario_hyper_samples(lib):
    from bocf_amd import hyper
    rng = np.random.RandomState(2)
    np.random.seed(3)
    H = 2
    X, Y = _data(rng)
    Xc = rng.uniform(size=(C, D))
    support, prob = rng.uniform(size=(L, M)), np.array([0.5, 0.25, 0.25])
    model = B.multi_outputGP(M, fixed_hyps=False, n_samples=H)
    model._X, model._Y = np.ascontiguousarray(X), [y.copy() for y in Y]
    model._kernel_ids = [_ffi.KERN_SE, _ffi.KERN_MATERN52]
    model._instances = [[(1.0 + 0.1 * h, np.full(D, 0.5 - 0.05 * h), 1e-4) for _ in range(M)] for h in range(H)]
    lib.mark("fit")
    model._fit()
    lib.mark("the same query per hyper-sample")
    for query in (model.posterior_mean, model.predict, model.posterior_variance_gradient):
        for h in range(H):                                    # h = 1 is a slice of the pass that answered h = 0: no device call
            model.set_hyperparameters(h)
            query(Xc)
    model.posterior_mean(Xc)                                  # the last query was another one: the device answers again
    model.predict(Xc, full_cov=True)
    model.posterior_mean_at_evaluated_points()
    lib.mark("acquisitions")
    U = B.Utility(parameter_dist=_dist(support, prob), device="neg_sq_dist")
    W = rng.normal(size=(S, M))
    model.set_hyperparameters(1)
    model.acq_mc(Xc, _ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W, n_hyps=1)
    model.acq_mc(Xc, _ffi.ACQ_PI, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W, n_hyps=5, fetch=False)
    acq = B.uEI_noiseless(model, None, utility=U)
    acq._compute_acq(Xc)
    acq._compute_acq_withGradients(Xc[:1])
    B.maEI(model, None, utility=B.Utility(func=lambda t, y: np.dot(t, y), parameter_dist=_dist(support, prob), linear=True))._compute_acq(Xc)
    model.expected_utility(Xc, "closed", U, support, np.arange(C) % L, n_hyps=2, grad=True)
    kg = B.uKG(model, _space(), utility=U, n_fantasies=S, n_ref_points=3)
    kg._compute_acq(Xc)
    model.set_hyperparameters(0)
    model.posterior_covariance_gradient(Xc, Xc[:1])
    groups = [0, 1, 1]
    model.thompson_topk(Xc, support, groups, {0: rng.normal(size=(M, C, 1)), 1: rng.normal(size=(M, C, 2))}, U, 2)
    lib.mark("an inference and a device chain: the fit and every upload are forgotten")
    model._create_sampler_state()
    model._infer([(1.2, np.full(D, 0.4), 0.02)] * M)
    acq._compute_acq(Xc)
    outs = model._sampler_outputs
    draws = hyper.LockstepSampler.draw(outs, 3, rng=np.random.RandomState(4))
    model._device_hmc(outs, [dr[1] for dr in draws], [dr[2] for dr in draws], 2, 0.05, True)
    acq._compute_acq(Xc)
    model.posterior_mean(Xc)


def scenario_batches_constraints_paths(lib):
    """The pending-point, constrained and pathwise entry points, once with fixed hyper-parameters and once with H = 2 hyper-samples."""
    from bocf_amd.constraints import OutputConstraints
    rng = np.random.RandomState(5)
    np.random.seed(6)
    H = 2
    X, Y = _data(rng)
    Xc = rng.uniform(size=(C, D))
    support, prob = rng.uniform(size=(L, M)), np.array([0.25, 0.25, 0.5])
    fixed = B.multi_outputGP(M, fixed_hyps=True, noise_var=[1e-4] * M)
    lib.mark("fixed hyper-parameters: updateModel")
    fixed.updateModel(X, Y)
    sampled = B.multi_outputGP(M, fixed_hyps=False, n_samples=H)
    sampled._X, sampled._Y = np.ascontiguousarray(X), [y.copy() for y in Y]
    sampled._kernel_ids = [_ffi.KERN_MATERN32, _ffi.KERN_SE]
    sampled._instances = [[(1.0 + 0.1 * h, np.full(D, 0.5 - 0.05 * h), 1e-4) for _ in range(M)] for h in range(H)]
    lib.mark("H = 2: fit")
    sampled._fit()
    U = B.Utility(parameter_dist=_dist(support, prob), device="neg_sq_dist")
    U_prog = B.Utility(func=abs15, parameter_dist=_dist(support, prob), device="program")
    cons = OutputConstraints([[1.0, -1.0], [0.5, 0.25]], [0.1, 0.2], eta=[1e-2, 1e-3])
    for name, model in (("fixed", fixed), ("H = 2", sampled)):
        W, W2 = rng.normal(size=(S, M)), rng.normal(size=(S, M))
        P, Zp = rng.uniform(size=(2, D)), rng.normal(size=(S, M, 2))
        lib.mark(name + ": pending points")
        if model is sampled:
            model.set_hyperparameters(1)
        model.set_mc_samples(W)
        model.set_pending_points(P, Zp)
        model.set_pending_points(P, Zp)                       # resident: no call
        model.set_pending_points(P[:1], Zp[:, :, :1], W=W2)   # W first, then the new set
        model.pending_samples()
        model.acq_pending(Xc, _ffi.UTIL_NEG_SQ_DIST, None, support, prob)
        model.acq_pending(Xc[:1], _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W2, n_hyps=1, grad=True)
        model.acq_pending(Xc, _ffi.UTIL_NEG_EXP_COS, np.ones(M), support, None, W=W, fetch=False)
        lib.mark(name + ": output constraints")
        model.set_output_constraints(cons)
        model.set_output_constraints(cons)                    # resident: no call
        model.feasible_best(_ffi.UTIL_NEG_SQ_DIST, None, support)
        model.acq_mc_constrained(Xc, _ffi.UTIL_NEG_SQ_DIST, None, support, prob)
        model.acq_mc_constrained(Xc[:2], _ffi.UTIL_NEG_SUM_EXP, None, support[:, :1], None, W=W2, n_hyps=2, grad=True)
        model.acq_mc_constrained(Xc, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, fetch=False)
        model.set_output_constraints(None)
        try:
            model.acq_mc_constrained(Xc, _ffi.UTIL_NEG_SQ_DIST, None, support, prob)
            raise AssertionError("RuntimeError expected")
        except RuntimeError:
            pass
        lib.mark(name + ": paths")
        n_paths = 3
        thetas = rng.uniform(size=(n_paths, M))
        model.draw_paths(n_paths, n_features=4)
        model.path_values(Xc)
        model.path_utility(Xc, np.arange(C) % n_paths, thetas, U, grad=True)
        model.path_utility(Xc[:2], [2, 0], thetas, U_prog)
        model.pathwise_topk(Xc, thetas, model._path_groups(n_paths), U, 2)
        model.pathwise_topk(Xc, thetas, model._path_groups(n_paths), U_prog, 2)
        lib.mark(name + ": Monte-Carlo gradient with a utility program")
        model.acq_mc_grad(Xc[:1], _ffi.UTIL_PROGRAM, None, support, prob, W=W, program=U_prog.program_blob)
        model.acq_mc_grad(Xc[:2], _ffi.UTIL_PROGRAM, None, support, prob, n_hyps=1, program=U_prog.program_blob)
        lib.mark(name + ": a new fit forgets the pending points and the paths")
        model.updateModel(X, [y + 0.05 for y in Y]) if model is fixed else model._fit()
        for call in (model.pending_samples, lambda: model.acq_pending(Xc, _ffi.UTIL_NEG_SQ_DIST, None, support, prob),
                     lambda: model.path_values(Xc)):
            try:
                call()
                raise AssertionError("RuntimeError expected")
            except RuntimeError:
                pass


SCENARIOS = (("fixed", scenario_fixed), ("hyper_samples", scenario_hyper_samples),
             ("batches_constraints_paths", scenario_batches_constraints_paths))


def run(scenario, monkeypatch=None):
    lib = RecordingLibrary()
    if monkeypatch is None:
        _ffi.load = lambda: lib
    else:
        monkeypatch.setattr(_ffi, "load", lambda: lib)
    scenario(lib)
    return json.loads(json.dumps({"calls": lib.calls, "random": np.random.random()}))


def _check(name, scenario, monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = run(scenario, monkeypatch)
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, "call %d: %r, recorded %r (after %r)" % (i, g, w, got["calls"][max(0, i - 3):i])
    assert len(got["calls"]) == len(want["calls"]), (got["calls"][len(want["calls"]):], want["calls"][len(got["calls"]):])
    assert got["random"] == want["random"]


def test_calls_with_fixed_hyperparameters(monkeypatch):
    _check("fixed", scenario_fixed, monkeypatch)


def test_calls_with_hyper_samples(monkeypatch):
    _check("hyper_samples", scenario_hyper_samples, monkeypatch)


def test_calls_of_batches_constraints_and_paths(monkeypatch):
    _check("batches_constraints_paths", scenario_batches_constraints_paths, monkeypatch)


if __name__ == "__main__":
    out = {name: run(scenario) for name, scenario in SCENARIOS}
    target = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(target, "w") as f:
        f.write("{\n" + ",\n".join('"%s": {"random": %r, "calls": [\n%s\n]}' % (
            name, out[name]["random"], ",\n".join(json.dumps(c) for c in out[name]["calls"])) for name in out) + "\n}\n")
    print("recorded", {name: len(out[name]["calls"]) for name in out}, "->", target)
