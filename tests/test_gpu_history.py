"""No entry point's result depends on the context's call history.

One bocf_ctx carries some twenty feature families and almost every one keeps state between calls (csrc/bocf_ctx.h: parameter and
best-so-far caches, the validity flags of the reduced-precision copies of R, the Ky^-1 an inference leaves, capacities that only grow,
resident W / Z / program / constraints / reference / pending / Thompson / path sets, scratch that families share by contract); the model
class mirrors it in _Resident.  The acquisition kernels use fixed reduction orders, so the property needs no tolerance:

    a call's result on a context with any history equals, BIT FOR BIT, the same call on a context that has only seen the same model changes.

The calls are the catalogue of tests/history_calls.py (self-contained, two variants that differ in every size).  A STATE is a list of
model changes on one context; expected(state, call, variant) builds a new model on a new context, replays the changes and nothing else,
runs that one call and is cached for the session -- the only reference here.  A recording proxy around the loaded library checks on that
new context that the call reached every entry point it declares.

  A  every ordered pair (c1, c2) of calls on one long-lived model per problem: c2 after c1 equals expected;
  B  a seeded walk of about 80 steps on one context, one step in five a model change (append, new targets, removal, refit, raw
     inference, and switches of the problem that move N, Np, d and m down and up), with the options that never change a number mixed in
     (chunk, swizzle, prefetch1, workspace_mb; small_path for more than 16 candidates -- SMALL_PATH below says what holds for fewer);
  C  at the end of each walk the busy model against the independent restatements (oracle/cpu_ref.py, tests/loo_ref.py) at those suites'
     tolerances -- the busy and the new context could be wrong in the same way.

EXCEPTIONS (calls compared with their restatement instead of bit for bit, each with the sentence of the contract that allows it): none.

Run on the MI355X box:  python -m pytest tests/test_gpu_history.py -m gpu"""
import collections
import os
import pickle
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import history_calls as H  # noqa: E402
import loo_ref as LR  # noqa: E402

from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CALL_NAMES = list(H.CALLS)
EXCEPTIONS = {}               # call name -> (sentence of include/bocf_hip.h or csrc/bocf_ctx.h that allows a difference, restatement); at most two

# ---------------------------------------------------------------------------------------------------------------------------------
# problems: at most 3 panels of 128 rows, where every Cholesky schedule gives the same bits (tests/test_gpu_round4.py: up to 8)
#            N    d  kernel family per output          seed
PROBLEMS = {
    "P1": (130, 3, ("matern52", "rbf"), 11),                     # mixed families, two panels
    "P1s": (90, 4, ("matern32", "matern32"), 15),                # as many outputs as P1: the switch that stays on the same model object
    "P2": (70, 5, ("matern32", "matern32", "matern32"), 12),     # one panel, one family
    "P3": (260, 2, ("se",), 13),                                 # three panels, one output
}
SPARE = 6                     # observations beyond N that the appends of a walk draw on
P4 = dict(N=40, d=2, m=2, H=3, seed=14)                        # the learning-mode model
TARGETS = {0: (1.0, 0.0), 1: (1.5, -0.3), 2: (-0.7, 2.0)}      # versions of the targets: scale, shift


@pytest.fixture(scope="module")
def B():
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


_data = {}


def data(name):
    """The observations of a problem (N + SPARE of them) and its hyper-parameters: smooth outputs, ARD lengthscales of 1.5 x the mean point
    spacing (cond(Ky) ~ 1e6 at noise 1e-4, as in tests/test_gpu_incremental.py: the tolerances of part C were set there)."""
    if name not in _data:
        N, d, kinds, seed = PROBLEMS[name]
        rng = np.random.RandomState(seed)
        n, m = N + SPARE, len(kinds)
        X = rng.uniform(size=(n, d))
        h = N ** (-1.0 / d)
        ls = [1.5 * h * (1.0 + 0.2 * rng.uniform(-1, 1, size=d)) for _ in range(m)]
        var = list(rng.uniform(0.8, 1.25, size=m))
        Y = []
        for _ in range(m):
            a, b = rng.normal(size=d), rng.normal(size=d)
            Y.append(np.sin(2 * np.pi * X.dot(a)) + 0.5 * np.cos(3 * X.dot(b)))
        _data[name] = dict(X=X, Y=np.stack(Y), kinds=list(kinds), lengthscales=ls, variances=var, noise=[1e-4] * m, N=N, d=d, m=m)
    return _data[name]


def _kernels(B, p):
    cls = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
    return [cls[k](p["d"], variance=p["variances"][j], lengthscale=p["lengthscales"][j], ARD=True) for j, k in enumerate(p["kinds"])]


# ---------------------------------------------------------------------------------------------------------------------------------
# the recording proxy
class Recorder(object):
    """Stands in for the loaded library: every bocf_* function called through it is noted in `seen`."""

    def __init__(self, lib):
        self._lib, self.seen = lib, set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("bocf_"):
            return fn

        def noted(*args):
            self.seen.add(name)
            return fn(*args)
        return noted


@pytest.fixture(scope="module", autouse=True)
def recorder(B):
    F = B._ffi
    real = F.load()
    rec = Recorder(real)
    F._libs["product"] = rec
    try:
        yield rec
    finally:
        F._libs["product"] = real
        _expected.clear()
        _busy.clear()


# ---------------------------------------------------------------------------------------------------------------------------------
# model changes.  A change is a tuple; a state is a tuple of changes, replayed by Sim on any model.
#   ("fit", problem, n)   the first n observations of `problem` -- on the same model object when the output count allows it, else on a
#                         new model object that takes over the context
#   ("append",)           one more observation (bocf_append, or a refit where it is refused)
#   ("targets", k)        version k of the targets on the same inputs (bocf_update_targets)
#   ("remove", i)         remove_observations([i]) (bocf_remove)
#   ("refit",)            the same data with incremental = False (bocf_fit)
#   ("infer",)            a raw bocf_infer with the model's hyper-parameters: it refactorizes, may leave Ky^-1 behind, and (N <= 128) leaves
#                         no factor; then the fit the model class runs at its next use
#   ("learn",)            the learning-mode model, updated once: its pickle twin
class Sim(object):
    def __init__(self, B):
        self.B, self.model, self.problem, self.rows, self.version, self.next = B, None, None, [], 0, 0

    def _switch(self, name):
        B, p = self.B, data(name)
        old = self.model
        if old is not None and old.output_dim == p["m"]:
            old.kernel, old.noise_var = _kernels(B, p), list(p["noise"])        # the same model object, the same context
        else:
            self.model = B.multi_outputGP(p["m"], kernel=_kernels(B, p), noise_var=list(p["noise"]), fixed_hyps=True)
            if old is not None:
                self.model._ctx, old._ctx = old._ctx, None                     # a new model object on the context with all its history
        self.problem = name

    def _update(self):
        p = data(self.problem)
        a, b = TARGETS[self.version]
        self.model.updateModel(p["X"][self.rows], [(a * y[self.rows] + b)[:, None] for y in p["Y"]])

    def current(self):
        """(X, Y (m, N)) the model holds."""
        p = data(self.problem)
        a, b = TARGETS[self.version]
        return p["X"][self.rows], a * p["Y"][:, self.rows] + b

    def apply(self, change):
        """Applies one change; returns the numbers the change itself produces (log-marginals; a raw inference: and its gradients)."""
        kind = change[0]
        if kind == "learn":
            self.model, self.problem = pickle.loads(learned(self.B)[1]), "P4"
            return ()
        if kind == "fit":
            self._switch(change[1])
            self.rows, self.version, self.next = list(range(change[2])), 0, change[2]
            self._update()
        elif kind == "append":
            assert self.next < data(self.problem)["N"] + SPARE
            self.rows.append(self.next)
            self.next += 1
            self._update()
        elif kind == "targets":
            self.version = change[1]
            self._update()
        elif kind == "remove":
            del self.rows[change[1]]
            self.model.remove_observations([change[1]])
        elif kind == "refit":
            self.model.incremental = False
            try:
                self._update()
            finally:
                self.model.incremental = True
        elif kind == "infer":
            return self._infer()
        else:
            raise ValueError(change)
        X, _ = self.current()
        assert np.array_equal(self.model._X, X)
        return (np.array(self.model.log_marginal),)

    def _infer(self):
        F, model = self.B._ffi, self.model
        kids, var, ls, noise = model._hyper_arrays()
        X, Y = self.current()
        X, Y = F.f64(X), F.f64(Y)
        M, (N, d) = var.size, X.shape
        jit, lml, dv, dl, dn = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros((M, d)), np.zeros(M)
        kid = model._send_kernel_ids(kids)
        rc = F.load().bocf_infer(model._context().handle, F.dptr(X), F.dptr(Y), N, d, M, kid, F.dptr(var), F.dptr(ls), F.dptr(noise), 5, F.dptr(jit),
                                 F.dptr(lml), F.dptr(dv), F.dptr(dl), F.dptr(dn))
        model._refactorized(rc, "bocf_infer", M)               # what the model class does after its own inferences: the next use fits again
        # ... and that fit is part of the change: left to the next call, the busy model (fitted by its next call) would answer a removal
        # with bocf_remove where the replay (no call in between) refits -- the same model up to rounding, not bit for bit
        model._ensure_fitted()
        return jit, lml, dv, dl, dn, np.array(model.log_marginal)


_learned = []


def learned(B):
    """(the learning-mode model right after its update, its pickle taken at that moment): the shortest sampler settings an existing learning
    test uses (tests/test_gpu_round3.py).  The pickle holds the same hyper-samples and no context, which is what __getstate__ is for."""
    if not _learned:
        rng = np.random.RandomState(P4["seed"])
        X = rng.uniform(size=(P4["N"], P4["d"]))
        Y = [np.sin(3 * X[:, :1] + j) + 0.1 * rng.normal(size=(P4["N"], 1)) for j in range(P4["m"])]
        model = B.multi_outputGP(P4["m"], fixed_hyps=False, n_samples=P4["H"])
        model.n_burnin, model.subsample_interval, model.leapfrog_steps, model.step_size, model.max_iters = 2, 1, 3, 0.02, 4
        np.random.seed(P4["seed"])
        model.updateModel(X, Y)
        assert model._H == P4["H"]
        _learned.extend([model, pickle.dumps(model)])
    return _learned


# the states of part A: one per problem, each behind a different last change
STATES = {
    "P1": (("fit", "P1", 129), ("append",)),
    "P2": (("fit", "P2", 70),),
    "P3": (("fit", "P3", 260), ("targets", 1)),
    "P4": (("learn",),),
}


def shape_of(model):
    return model._X.shape[1], model.output_dim


# ---------------------------------------------------------------------------------------------------------------------------------
# expected values
_expected = {}
_fresh_seconds = []


def replay(B, state):
    sim, out = Sim(B), ()
    for change in state:
        out = sim.apply(change)
    return sim, out


def reads_small_path(name):
    """Does the call evaluate 16 or fewer candidates in one predict pass (its own batch, or the gathered running rows of a refinement)?"""
    return any(s in H.CALLS[name].sizes for s in ("Cs", "A"))


def expected(B, rec, state, name, variant, shared=False, small_path=1):
    """The call on a new model with a new context that has seen the state's model changes and nothing else; cached per session.
    small_path = 0: with that option set on the new context as well (SMALL_PATH below)."""
    key = (state, name, variant, shared, small_path)
    if key not in _expected:
        t0 = time.perf_counter()
        sim, _ = replay(B, state)
        call = H.CALLS[name]
        inp = call.inputs(variant, *shape_of(sim.model), shared=shared)
        if not small_path:
            sim.model.set_option("small_path", 0)
        rec.seen.clear()
        out = call.run(sim.model, inp)
        missed = set(call.entries) - rec.seen
        assert not missed, "%s (%s) did not reach %s" % (name, variant, sorted(missed))
        for a in out:
            a.setflags(write=False)
        _expected[key] = out
        _fresh_seconds.append(time.perf_counter() - t0)
    return _expected[key]


def expected_change(B, state):
    """What the state's last change returns on a new context that has seen the changes alone."""
    key = (state, None, None, None, None)
    if key not in _expected:
        _expected[key] = tuple(np.array(a) for a in replay(B, state)[1])
    return _expected[key]


def first_difference(got, want):
    """None when the tuples of arrays agree bit for bit (NaN-safe), else a description of the first difference."""
    if len(got) != len(want):
        return "%d arrays, expected %d" % (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            return "array %d: shape %s dtype %s, expected %s %s" % (k, g.shape, g.dtype, w.shape, w.dtype)
        if g.tobytes() == w.tobytes():
            continue
        bits = np.uint64 if g.dtype.itemsize == 8 else np.uint32
        bad = np.flatnonzero(g.reshape(-1).view(bits) != w.reshape(-1).view(bits))
        i = int(bad[0])
        return "array %d of shape %s differs in %d of %d entries, first at flat index %d %s: got %r, expected %r" % (
            k, g.shape, bad.size, g.size, i, np.unravel_index(i, g.shape), g.reshape(-1)[i], w.reshape(-1)[i])
    return None


def recheck(B, rec, state, pair, shared, small_path):
    """Runs just the calls of `pair` on a new context behind the state: does the pair alone reproduce the mismatch?"""
    sim, _ = replay(B, state)
    if not small_path:
        sim.model.set_option("small_path", 0)
    out = None
    for name, variant in pair:
        out = H.CALLS[name].run(sim.model, H.CALLS[name].inputs(variant, *shape_of(sim.model), shared=shared))
    diff = first_difference(out, expected(B, rec, state, *pair[-1], shared=shared, small_path=small_path))
    return "the pair alone on a new context REPRODUCES it (%s)" % diff if diff else "the pair alone on a new context does NOT reproduce it: longer history is needed"


def run_checked(B, rec, sim, state, name, variant, trail, before=None, shared=False, small_path=1):
    call = H.CALLS[name]
    small_path = small_path if reads_small_path(name) else 1
    got = call.run(sim.model, call.inputs(variant, *shape_of(sim.model), shared=shared))
    trail.append("%s(%s%s)" % (name, variant, ", shared inputs" if shared else ""))
    diff = first_difference(got, expected(B, rec, state, name, variant, shared, small_path))
    if diff:
        pair = ([before] if before else []) + [(name, variant)]
        raise AssertionError("%s (variant %s, %s inputs)%s on the busy context differs from the same call on a new one.\n  %s\n  state: %s\n  last calls: %s\n  %s" % (
            name, variant, "shared" if shared else "its own", " after %s (variant %s)" % before if before else "", diff, state, " -> ".join(trail),
            recheck(B, rec, state, pair, shared, small_path)))
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# A. every ordered pair
_busy = {}


def busy_model(B, problem):
    """The one long-lived model of a problem (the learning-mode model: the very object whose context ran the optimiser and the chains)."""
    if problem not in _busy:
        if problem == "P4":
            sim = Sim(B)
            sim.model, sim.problem = learned(B)[0], "P4"
        else:
            sim, _ = replay(B, STATES[problem])
        _busy[problem] = (sim, collections.deque(maxlen=10))
    return _busy[problem]


@pytest.mark.parametrize("c1", CALL_NAMES)
@pytest.mark.parametrize("inputs", ["own", "shared"])
@pytest.mark.parametrize("problem", list(STATES))
def test_every_ordered_pair_of_calls(B, recorder, problem, inputs, c1):
    """inputs = "own": every call with the arrays drawn for it alone.  "shared": the twin catalogue in which calls of different families hand
    over the same candidates, samples, parameters and point sets (Call.inputs), so that c2 finds c1's uploads and caches matching."""
    shared = inputs == "shared"
    state = STATES[problem]
    sim, trail = busy_model(B, problem)
    i1, n = CALL_NAMES.index(c1), len(CALL_NAMES)
    for i2, c2 in enumerate(CALL_NAMES):
        pair = i1 * n + i2
        v1, v2 = H.VARIANTS[pair % 2], H.VARIANTS[(pair // 2) % 2]
        run_checked(B, recorder, sim, state, c1, v1, trail, shared=shared)       # (itself the second call of the pair (c2 before, c1): checked as well)
        run_checked(B, recorder, sim, state, c2, v2, trail, before=(c1, v1), shared=shared)


def test_the_expected_values_are_not_degenerate(B, recorder):
    """A catalogue of all-zero acquisitions would compare equal whatever the kernels did: on every problem every call returns finite
    numbers, and in at least one variant its first array holds more than one value (an improvement over a hard-to-beat incumbent is
    exactly zero over a small batch with few samples: the share of non-zero entries of every variant is printed)."""
    for problem, state in STATES.items():
        for name in CALL_NAMES:
            varied = []
            for variant in H.VARIANTS:
                out = expected(B, recorder, state, name, variant)
                floats = [a for a in out if a.dtype.kind == "f"]
                assert floats, name
                for a in floats:
                    assert np.isfinite(a).sum() > 0, (problem, name, variant)
                values = np.concatenate([a.reshape(-1) for a in floats])
                varied.append(np.unique(values[np.isfinite(values)]).size > 1)
                print("%s %s(%s): non-zero share of each array %s" % (problem, name, variant, ["%.2f" % np.mean(a != 0) for a in floats]))
            assert any(varied), (problem, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# named regression cases: the minimal (state, c1, c2) of every dependence on history these tests have found
def test_regression_precision_option_behind_the_hyper_sample_query_cache(B, recorder):
    """State P4 (several hyper-samples resident); c1 = predict(X); c2 = predict(X) under predict_f32 / predict_i8, the SAME X.
    With several hyper-samples the model class answers a repeated posterior query from the host copy of the first one (cbo.py walks the
    hyper-samples with one query each); the copy's key held X, the flags and the fit, not the options that choose the arithmetic of the
    variance contraction -- so c2 returned c1's fp64 variances.  (The catalogue cannot see it: its calls draw their own X.)"""
    X = H.CALLS["predict_tile"].inputs("b", P4["d"], P4["m"])["X"]
    busy = pickle.loads(learned(B)[1])
    busy.set_hyperparameters(1)
    plain = busy.predict(X)
    for option in ("predict_f32", "predict_i8"):
        new = pickle.loads(learned(B)[1])
        new.set_hyperparameters(1)
        want = H._with_option(new, option, lambda: new.predict(X))
        got = H._with_option(busy, option, lambda: busy.predict(X))
        assert first_difference(want, plain), "%s does not change the variances here: the case shows nothing" % option
        diff = first_difference(got, want)
        assert not diff, "predict under %s after a plain predict of the same X: %s" % (option, diff)
        diff = first_difference(busy.predict(X), plain)
        assert not diff, "plain predict after one under %s: %s" % (option, diff)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. the seeded walk, C. the anchor
WALK = [("append",), ("targets", 1), ("infer",), ("remove", 7), ("fit", "P1s", 90), ("append",), ("fit", "P2", 70), ("infer",), ("targets", 2),
        ("fit", "P3", 260), ("append",), ("remove", 100), ("refit",), ("fit", "P1", 130), ("targets", 1), ("append",)]
STEPS = 80
# the options that never change a number (include/bocf_hip.h: "speed only", "results do not depend on the chunking", "both give bit-identical
# sums"), value for value; the first of each list is the default.  workspace_mb = 4: the largest workspace a catalogue call asks for is the
# joint gradient's 6 x 128 x (2 x 128 + 128 + 120 x 2) x 8 bytes = 3.7 MiB on the learning-mode model, 3.0 MiB on the problems of the walk
OPTIONS = {"chunk": (65536, 128), "small_path": (1, 0), "swizzle": (-1, 0, 258), "prefetch1": (0, 1), "workspace_mb": (24576, 4)}
# SMALL_PATH.  The four others are set on the busy model alone.  small_path is one of them for every call of more than 16 candidates, which it
# cannot reach.  For 16 or fewer the library's contract is that the GEMV-shaped path and the tile path agree "to round-off"
# (tests/test_gpu_parity.py: "<= 16 candidates take the GEMV-shaped path: same values to round-off"; DESIGN.md section 4: "a row's value can
# differ in its last bits with the size of the batch it came in") -- the option does change bits there, by design (seed 101 met it: a
# three-row refinement under small_path = 0 moved by 3e-15).  For those calls (reads_small_path) the option's value counts as part of the call:
# the new context of the reference gets the same value, the comparison stays bit for bit, and everything else the busy context carries is
# still history.


def _anchor(B, sim):
    """C: the busy model at the end of a walk against the restatements on the data it holds."""
    p, model = data(sim.problem), sim.model
    X, Y = sim.current()
    d, m = shape_of(model)
    ref = R.MultiOutputGPRef(p["kinds"], p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(X, [y[:, None] for y in Y])
    assert all(o.jitter == 0 for o in ref.output) and np.all(np.asarray(model.jitter) == 0)
    # predict: the tolerances of tests/test_gpu_incremental.py (mean rtol 1e-6 / atol 1e-7, |dvar| <= 1e-9)
    Xc = H.CALLS["predict_tile"].inputs("b", d, m)["X"]
    mean, var = model.predict(Xc)
    rm, rv = ref.predict(Xc)
    np.testing.assert_allclose(mean, rm, rtol=1e-6, atol=1e-7)
    assert np.abs(var - rv).max() <= 1e-9, np.abs(var - rv).max()
    # uEI: the tolerance of tests/test_gpu_parity.py against batch_uEI (rtol 1e-5, atol 1e-10)
    i = H.CALLS["acq_mc_ei"].inputs("b", d, m)
    a = H.CALLS["acq_mc_ei"].run(model, i)[0]
    r = R.batch_uEI(ref, i["X"], i["W"], "neg_sq_dist", i["thetas"], i["prob"], "EI")[0].reshape(-1)
    assert np.mean(r > 0) > 0.05, "the anchor's acquisition is zero almost everywhere: it anchors nothing"
    np.testing.assert_allclose(a, r, rtol=1e-5, atol=1e-10)
    # leave-one-out: the gate of tests/test_gpu_loo.py -- distances to the long-double brute force within 100 x those of the oracle formula
    mean, var, lpd = model.loo()
    var0 = model.loo(noiseless=True)[1]
    for j, kind in enumerate(p["kinds"]):
        nz = p["noise"][j]
        truth = LR.loo_brute(kind, X, Y[j], p["variances"][j], p["lengthscales"][j], nz, 1e-8, np.longdouble)
        fit = R.GPFit(kind, X, Y[j][:, None], p["variances"][j], p["lengthscales"][j], nz)
        floor = LR.distances(LR.loo_formula_fit(fit, Y[j]), truth, nz)
        want0 = np.maximum(truth[2], np.longdouble(1e-10))
        dev = (mean[j], var[j], var0[j], lpd[j])
        dist = LR.distances(dev, (truth[0], truth[1], want0, truth[3]), nz)
        dist0 = LR.distances(dev, (truth[0], truth[1], want0, truth[3]), nz, with_noise=False)[1]
        print("anchor, leave-one-out of output %d: floor %s, device %s, noiseless variance %.1e" % (j, ["%.1e" % v for v in floor], ["%.1e" % v for v in dist], dist0))
        for k in range(3):
            assert dist[k] <= LR.gate(floor[k]), (j, k, dist[k], floor[k])
        assert dist0 <= LR.gate(floor[1]), (j, dist0, floor[1])


@pytest.mark.parametrize("seed", [101, 202, 303])
def test_seeded_walk_with_model_changes(B, recorder, seed):
    print("walk seed %d" % seed)
    rng = np.random.RandomState(seed)
    state = STATES["P1"]
    sim, _ = replay(B, state)
    trail = collections.deque(maxlen=10)
    options = {name: values[0] for name, values in OPTIONS.items()}
    try:
        for name in CALL_NAMES:                                # the context has used every family, at the larger sizes, before anything changes
            run_checked(B, recorder, sim, state, name, "b", trail)
        at = set(rng.choice(np.arange(2, STEPS), size=len(WALK), replace=False).tolist())
        changes = list(WALK)
        for step in range(STEPS):
            if rng.uniform() < 0.2:                            # an option that changes no number, on the busy model only
                name = sorted(OPTIONS)[rng.randint(len(OPTIONS))]
                options[name] = OPTIONS[name][rng.randint(len(OPTIONS[name]))]
                sim.model.set_option(name, options[name])
                trail.append("%s=%d" % (name, options[name]))
            if step in at:
                change = changes.pop(0)
                got = sim.apply(change)
                state = state + (change,)
                trail.append(repr(change))
                diff = first_difference(got, expected_change(B, state))
                assert not diff, "the model change %r on the busy context differs from the same change on a new one.\n  %s\n  state: %s\n  last calls: %s" % (
                    change, diff, state, " -> ".join(trail))
            else:
                name, variant = CALL_NAMES[rng.randint(len(CALL_NAMES))], H.VARIANTS[rng.randint(2)]
                run_checked(B, recorder, sim, state, name, variant, trail, shared=bool(rng.randint(2)), small_path=options["small_path"])
        assert not changes and sim.problem == "P1"
        _anchor(B, sim)
    finally:
        print("options at the end: %s; %d new contexts so far, %.3f s each on average (the slowest %.3f s)" % (
            options, len(_fresh_seconds), np.mean(_fresh_seconds), np.max(_fresh_seconds)))
