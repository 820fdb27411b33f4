"""The catalogue of the call-history tests (tests/test_history_cpu.py, tests/test_gpu_history.py).  TEST INFRASTRUCTURE ONLY; imports
without a device.

A CALL is a named function run(model, inputs) -> tuple of ndarrays over the model methods the other suites use.  It is self-contained:
every array it depends on -- X, W, Z, Zf, Zp, thetas, prob, the program blob, the constraints, the hyper-sample -- is an explicit
argument taken from `inputs`, nothing is left to what an earlier call made resident (no None for X, W or Z, no draw from the host's
global random stream).  So its contract is free of the context's history: on a context with any history it must return, bit for bit,
what it returns on a context that has only seen the same model changes.

Every call exists in two VARIANTS, "a" and "b", which differ in every size the call declares (SIZES): a walk over calls in random
variants grows and shrinks every buffer.  The inputs come from a generator seeded by (call name, variant, d, m) and nothing else.

Each call declares the C entry points it must reach (`entries`, checked by a recording proxy on a new context) and the options it
toggles (`options`; set and reset inside the call)."""
import contextlib
import functools
import zlib

import numpy as np

import bocf_amd as B
from bocf_amd import _ffi as F

VARIANTS = ("a", "b")

# every size a call can declare: name -> (variant a, variant b)
SIZES = {
    "C": (37, 150),      # candidates: below / above one 128-column tile, neither a multiple of anything
    "Cs": (3, 16),       # candidates on the small path (<= 16)
    "S": (25, 70),       # Monte-Carlo samples (of W, of Z per parameter, of the pending / joint normals, of a joint posterior draw)
    "L": (1, 3),         # utility parameters
    "na": (3, 130),      # reference points: below / above one 128-column tile
    "r": (2, 7),         # pending points
    "q": (2, 4),         # points per joint batch
    "B": (9, 30),        # joint batches (B q = 18 / 120 points: the gradient form takes at most 128)
    "Sf": (4, 16),       # fantasy normals of the knowledge gradient
    "F": (64, 130),      # random Fourier features per path
    "P": (2, 6),         # Thompson paths
    "k": (5, 33),        # selection size
    "A": (3, 20),        # rows of a refinement: the small path / more than 16 rows (predicted twice per pass)
    "K": (1, 3),         # linear output constraints
}
# the documented limits of the entry points (include/bocf_hip.h) that bound a size
LIMITS = {"S": 256, "L": 32, "na": 1024, "r": 15, "q": 8, "Sf": 256, "F": 16384, "P": 64, "k": 64, "A": 64, "K": 8, "Cs": 16}
JOINT_GRAD_POINTS = 128

# the candidates' box: wider than the unit box of the observations, so that part of every batch lies where the posterior is uncertain and the
# improvement acquisitions are not zero throughout
BOX = (-0.3, 1.3)
KIND = F.UTIL_NEG_SQ_DIST     # the composite utility of the Monte-Carlo calls: -|y - theta|^2, theta_dim = m, any m, has a closed form


def size(name, variant):
    return SIZES[name][VARIANTS.index(variant)]


def _seed(*key):
    return zlib.crc32("|".join(str(k) for k in key).encode()) & 0x7FFFFFFF


@contextlib.contextmanager
def seeded_global_stream(seed):
    """draw_paths draws its frequencies from the host's global stream: seeded here from the call's inputs, and put back afterwards, so the
    call neither reads nor leaves any host random state."""
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        yield
    finally:
        np.random.set_state(state)


def _neg_sq_dist(t, y):
    return -np.sum(np.square((y.transpose() - t).transpose()), axis=0)


@functools.lru_cache(maxsize=None)
def program_blob(m):
    """The traced utility program of -|y - theta|^2 for m outputs (traced on the host; no device)."""
    U = B.Utility(func=_neg_sq_dist, parameter_dist=B.ParameterDistribution(support=np.zeros((1, m)), prob_dist=np.ones(1)), device="program")
    assert U.device_kind(m) == F.UTIL_PROGRAM
    return U.program_blob


def _utility(thetas):
    n = len(thetas)
    return B.Utility(parameter_dist=B.ParameterDistribution(support=thetas, prob_dist=np.full(n, 1.0 / n)), device="neg_sq_dist")


class Call(object):
    def __init__(self, name, fn, sizes, entries, options):
        self.name, self.fn, self.sizes, self.entries, self.options = name, fn, tuple(sizes), tuple(entries), tuple(options)

    def sizes_of(self, variant):
        return {s: size(s, variant) for s in self.sizes}

    def inputs(self, variant, d, m, shared=False):
        """The call's inputs for a model with d input dimensions and m outputs: a dict of arrays and ints, a function of
        (name, variant, d, m) alone.  shared=True: the twin in which every array a resident set or a device-side cache is made from (SHARED)
        is a function of its role and shape alone, so calls of different families hand over the SAME candidates, samples, parameters,
        reference and pending points -- the uploads that are skipped for identical content and the best-so-far cache are then hit across
        calls, which inputs of the call's own never do.  Treat the dict as read-only."""
        return _inputs(self.name, self.sizes, variant, int(d), int(m), bool(shared))

    def run(self, model, inp):
        model.set_hyperparameters(inp["h"] % model._H)         # (the acquisitions leave the model on the last hyper-sample they averaged)
        out = self.fn(model, inp)
        return tuple(np.asarray(a) for a in out)


SHARED = ("x1", "X", "W", "thetas", "prob", "rows", "Zeu", "A", "Zf", "P", "Zp", "Zq", "thetasP", "cA")


def _draw(rng, field, shape, hi):
    if field == "X":
        return rng.uniform(BOX[0], BOX[1], size=shape)
    if field in ("x1", "A", "P"):
        return rng.uniform(size=shape)
    if field in ("thetas", "thetasP"):
        return rng.uniform(-0.5, 0.5, size=shape)
    if field == "prob":
        p = rng.uniform(0.5, 1.5, size=shape)
        return p / p.sum()
    if field in ("rows", "row_path"):
        return rng.randint(0, hi, size=shape)
    if field == "c":
        return rng.uniform(0.5, 1.5, size=shape)
    return rng.normal(size=shape)                                   # W, Zeu, Zf, Zp, Zq, Zpath, Zs, cA


@functools.lru_cache(maxsize=None)
def _inputs(name, sizes, variant, d, m, shared=False):
    own = np.random.RandomState(_seed(name, variant, d, m))
    n = {s: size(s, variant) for s in sizes}
    rows = n.get("C") or n.get("Cs") or n.get("A") or (n["B"] * n["q"] if "B" in n else 0)
    S, L = n.get("S"), n.get("L")
    want = [("x1", (1, d), None)]                                    # (field, shape, exclusive upper bound of an index array), in drawing order
    if rows:
        want.append(("X", (rows, d), None))
    if S:
        want.append(("W", (S, m), None))
    if L:
        want += [("thetas", (L, m), None), ("prob", (L,), None), ("rows", (rows,), L)]
        if S:
            want.append(("Zeu", (L, S, m), None))
    if "na" in n:
        want.append(("A", (n["na"], d), None))
    if "Sf" in n:
        want.append(("Zf", (n["Sf"], m), None))
    if "r" in n:
        want += [("P", (n["r"], d), None), ("Zp", (S, m, n["r"]), None)]
    if "q" in n:
        want.append(("Zq", (S, m, n["q"]), None))
    if "P" in n:                                                    # Zpath: the joint-posterior normals of path s, (m, C)
        want += [("thetasP", (n["P"], m), None), ("Zpath", (n["P"], m, rows), None), ("row_path", (rows,), n["P"])]
    if S and rows and not L:
        want.append(("Zs", (m, rows, S), None))
    if "K" in n:
        want.append(("cA", (n["K"], m), None))
    if L and not rows:                                              # loo_utility: the weights of neg_exp_cos
        want.append(("c", (m,), None))
    i = {"n": n, "h": 0 if variant == "a" else 2, "j": 0 if variant == "a" else m - 1, "seed": _seed("stream", name, variant, d, m),
         "bounds": [BOX] * d}
    for field, shape, hi in want:
        rng = np.random.RandomState(_seed("shared", field, shape, hi)) if shared and field in SHARED else own
        i[field] = _draw(rng, field, shape, hi)
    if "K" in n:
        i["cb"], i["ceta"] = np.full(n["K"], 0.8), 0.1
    for v in i.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return i


CALLS = {}


def call(name, sizes=(), entries=(), options=()):
    def deco(fn):
        assert name not in CALLS
        CALLS[name] = Call(name, fn, sizes, entries, options)
        return fn
    return deco


def _with_option(model, name, fn):
    model.set_option(name, 1)
    try:
        return fn()
    finally:
        model.set_option(name, 0)


# ---- predict ------------------------------------------------------------------------------------------------------------------------
@call("posterior_mean", ("C",), ("bocf_set_candidates", "bocf_predict"))
def _posterior_mean(model, i):
    return (model.posterior_mean(i["X"]),)


def _both_predicts(model, i):
    return model.predict(i["X"]) + model.predict_noiseless(i["X"])


call("predict_tile", ("C",), ("bocf_set_candidates", "bocf_predict"))(_both_predicts)
call("predict_small", ("Cs",), ("bocf_set_candidates", "bocf_predict"))(_both_predicts)


@call("predict_full_cov", ("C",), ("bocf_predict", "bocf_predict_cov_column"))
def _predict_full_cov(model, i):
    return model.predict(i["X"], full_cov=True)


@call("predict_f32", ("C",), ("bocf_set_option", "bocf_predict"), options=("predict_f32",))
def _predict_f32(model, i):
    return _with_option(model, "predict_f32", lambda: model.predict(i["X"]))


@call("predict_i8", ("C",), ("bocf_set_option", "bocf_predict"), options=("predict_i8",))
def _predict_i8(model, i):
    return _with_option(model, "predict_i8", lambda: model.predict(i["X"]))


def _gradients(model, i):
    return model.posterior_mean_gradient(i["X"]), model.posterior_variance_gradient(i["X"])


call("gradients_small", ("Cs",), ("bocf_set_candidates", "bocf_predict_gradients"))(_gradients)
call("gradients_tile", ("C",), ("bocf_set_candidates", "bocf_predict_gradients"))(_gradients)


@call("mean_at_train", (), ("bocf_mean_at_train",))
def _mean_at_train(model, i):
    return (model.posterior_mean_at_evaluated_points(),)


# ---- improvement acquisitions -------------------------------------------------------------------------------------------------------
@call("acq_linear_ei", ("C", "L"), ("bocf_acq_linear",))
def _acq_linear_ei(model, i):
    return (model.acq_linear(i["X"], F.ACQ_EI, i["thetas"], i["prob"]),)


@call("acq_linear_pi", ("C", "L"), ("bocf_acq_linear",))
def _acq_linear_pi(model, i):
    return (model.acq_linear(i["X"], F.ACQ_PI, i["thetas"], i["prob"]),)


@call("acq_linear_grad", ("C", "L"), ("bocf_acq_linear_grad",))
def _acq_linear_grad(model, i):
    return model.acq_linear_grad(i["X"], F.ACQ_EI, i["thetas"], i["prob"])


@call("acq_mc_ei", ("C", "S", "L"), ("bocf_set_mc_samples", "bocf_acq_mc"))
def _acq_mc_ei(model, i):
    return (model.acq_mc(i["X"], F.ACQ_EI, KIND, None, i["thetas"], i["prob"], W=i["W"]),)


@call("acq_mc_pi", ("C", "S", "L"), ("bocf_set_mc_samples", "bocf_acq_mc"))
def _acq_mc_pi(model, i):
    return (model.acq_mc(i["X"], F.ACQ_PI, KIND, None, i["thetas"], i["prob"], W=i["W"]),)


@call("acq_mc_program", ("C", "S", "L"), ("bocf_set_utility_program", "bocf_set_mc_samples", "bocf_acq_mc"))
def _acq_mc_program(model, i):
    blob = program_blob(model.output_dim)
    model.set_utility_program(blob)
    return (model.acq_mc(i["X"], F.ACQ_EI, F.UTIL_PROGRAM, None, i["thetas"], i["prob"], W=i["W"], program=blob),)


@call("acq_mc_grad", ("C", "S", "L"), ("bocf_set_mc_samples", "bocf_acq_mc_grad"))
def _acq_mc_grad(model, i):
    return model.acq_mc_grad(i["X"], KIND, None, i["thetas"], i["prob"], W=i["W"])


@call("acq_mc_topk", ("C", "S", "L", "k"), ("bocf_acq_mc", "bocf_select_topk"))
def _acq_mc_topk(model, i):
    a = model.acq_mc(i["X"], F.ACQ_EI, KIND, None, i["thetas"], i["prob"], W=i["W"])
    return (a,) + model.select_topk(i["n"]["k"])


# ---- look-ahead -----------------------------------------------------------------------------------------------------------------------
def _kg(mode, grad):
    def run(model, i):
        model.set_reference_points(i["A"])
        samples = {"W": i["W"]} if mode == "mc" else {}        # (the closed form reads no Monte-Carlo samples)
        out = model.acq_kg(i["X"], mode, KIND, None, i["thetas"], i["prob"], i["Zf"], grad=grad, **samples)
        return out if grad else (out,)
    return run


call("kg_closed", ("C", "L", "na", "Sf"), ("bocf_set_ref_points", "bocf_acq_kg"))(_kg("closed", False))
call("kg_closed_grad", ("C", "L", "na", "Sf"), ("bocf_set_ref_points", "bocf_acq_kg"))(_kg("closed", True))
call("kg_mc", ("C", "S", "L", "na", "Sf"), ("bocf_set_ref_points", "bocf_set_mc_samples", "bocf_acq_kg"))(_kg("mc", False))
call("kg_mc_grad", ("C", "S", "L", "na", "Sf"), ("bocf_set_ref_points", "bocf_set_mc_samples", "bocf_acq_kg"))(_kg("mc", True))


@call("cov_precomputed", ("C", "na"), ("bocf_set_ref_points", "bocf_cov_to_ref"))
def _cov_precomputed(model, i):
    model.partial_precomputation_for_covariance(i["A"])
    return (model.posterior_covariance_between_points_partially_precomputed(i["X"], i["A"]),)


@call("conditioned_variance", ("C",), ("bocf_set_ref_points", "bocf_conditioned_variance"))
def _conditioned_variance(model, i):
    model.partial_precomputation_for_variance_conditioned_on_next_point(i["x1"])
    return model.posterior_variance_conditioned_on_next_point(i["X"]), model.posterior_variance_gradient_conditioned_on_next_point(i["X"])


@call("covariance_gradient", ("C",), ("bocf_set_ref_points", "bocf_cov_to_ref"))
def _covariance_gradient(model, i):
    return (model.posterior_covariance_gradient(i["X"], i["x1"]),)


@call("posterior_cov", ("C", "na"), ("bocf_posterior_cov",))
def _posterior_cov(model, i):
    return (model.posterior_covariance_between_points(i["X"], i["A"]),)


# ---- pending points -------------------------------------------------------------------------------------------------------------------
@call("pending", ("C", "S", "L", "r"), ("bocf_set_mc_samples", "bocf_set_pending_points", "bocf_acq_pending", "bocf_get_pending_samples"))
def _pending(model, i):
    model.set_pending_points(i["P"], i["Zp"], W=i["W"])
    a = model.acq_pending(i["X"], KIND, None, i["thetas"], i["prob"], W=i["W"])
    return a, model.pending_samples()


@call("pending_grad", ("C", "S", "L", "r"), ("bocf_set_mc_samples", "bocf_set_pending_points", "bocf_acq_pending"))
def _pending_grad(model, i):
    model.set_pending_points(i["P"], i["Zp"], W=i["W"])
    return model.acq_pending(i["X"], KIND, None, i["thetas"], i["prob"], W=i["W"], grad=True)


# ---- joint q-point expected improvement ----------------------------------------------------------------------------------------------
@call("joint", ("B", "q", "S", "L"), ("bocf_acq_joint",))
def _joint(model, i):
    a = model.acq_joint(i["X"], i["n"]["q"], KIND, None, i["thetas"], i["prob"], i["Zq"])
    return a, model.last_joint_floored


@call("joint_grad", ("B", "q", "S", "L"), ("bocf_acq_joint",))
def _joint_grad(model, i):
    return model.acq_joint(i["X"], i["n"]["q"], KIND, None, i["thetas"], i["prob"], i["Zq"], grad=True)


# ---- constrained ----------------------------------------------------------------------------------------------------------------------
def _constraints(i):
    return B.OutputConstraints(i["cA"], i["cb"], i["ceta"])


def _constrained_mc(grad):
    def run(model, i):
        model.set_output_constraints(_constraints(i))
        out = model.acq_mc_constrained(i["X"], KIND, None, i["thetas"], i["prob"], W=i["W"], grad=grad)
        best, nf = model.feasible_best(KIND, None, i["thetas"])
        return (out if grad else (out,)) + (best, np.array([nf]))
    return run


_CMC = ("bocf_set_output_constraints", "bocf_set_mc_samples", "bocf_acq_mc_constrained", "bocf_feasible_best")
call("constrained_mc", ("C", "S", "L", "K"), _CMC)(_constrained_mc(False))
call("constrained_mc_grad", ("C", "S", "L", "K"), _CMC)(_constrained_mc(True))


@call("constrained_eu", ("C", "S", "L", "K"), ("bocf_set_output_constraints", "bocf_set_eu_samples", "bocf_train_utility_range",
                                             "bocf_expected_utility_constrained"))
def _constrained_eu(model, i):
    model.set_output_constraints(_constraints(i))
    lo, hi = model.train_utility_range(KIND, None, i["thetas"])
    return (lo, hi) + model.expected_utility_constrained(i["X"], KIND, i["thetas"], i["rows"], lo, i["Zeu"], grad=True)


# ---- recommendation -------------------------------------------------------------------------------------------------------------------
@call("eu_mean", ("C", "L"), ("bocf_expected_utility",))
def _eu_mean(model, i):
    return (model.expected_utility(i["X"], "mean", F.UTIL_LINEAR, i["thetas"], i["rows"]),)


@call("eu_closed", ("C", "L"), ("bocf_expected_utility",))
def _eu_closed(model, i):
    return (model.expected_utility(i["X"], "closed", KIND, i["thetas"], i["rows"]),)


@call("eu_mc", ("C", "S", "L"), ("bocf_set_eu_samples", "bocf_expected_utility"))
def _eu_mc(model, i):
    return (model.expected_utility(i["X"], "mc", KIND, i["thetas"], i["rows"], Z=i["Zeu"]),)


@call("eu_mc_grad", ("C", "S", "L"), ("bocf_set_eu_samples", "bocf_expected_utility"))
def _eu_mc_grad(model, i):
    return model.expected_utility(i["X"], "mc", KIND, i["thetas"], i["rows"], Z=i["Zeu"], grad=True)


# ---- risk and log ---------------------------------------------------------------------------------------------------------------------
@call("risk_quantile", ("C", "S", "L"), ("bocf_set_mc_samples", "bocf_acq_risk"))
def _risk_quantile(model, i):
    return (model.acq_risk(i["X"], F.RISK_QUANTILE, i["n"]["S"] // 4, KIND, None, i["thetas"], i["prob"], W=i["W"]),)


@call("risk_tail_mean", ("C", "S", "L"), ("bocf_set_mc_samples", "bocf_acq_risk"))
def _risk_tail_mean(model, i):
    return model.acq_risk(i["X"], F.RISK_LOWER_TAIL, i["n"]["S"] // 4, KIND, None, i["thetas"], i["prob"], W=i["W"], grad=True)


@call("linear_ucb", ("C", "L"), ("bocf_acq_linear_ucb",))
def _linear_ucb(model, i):
    return model.acq_linear_ucb(i["X"], 1.7, i["thetas"], i["prob"], grad=True)


@call("log_linear", ("C", "L"), ("bocf_acq_log_linear",))
def _log_linear(model, i):
    return model.acq_log_linear(i["X"], i["thetas"], i["prob"], grad=True)


@call("log_mc", ("C", "S", "L"), ("bocf_set_mc_samples", "bocf_acq_log_mc"))
def _log_mc(model, i):
    return model.acq_log_mc(i["X"], KIND, None, i["thetas"], i["prob"], 0.05, W=i["W"], grad=True)


# ---- samples --------------------------------------------------------------------------------------------------------------------------
@call("posterior_samples", ("C", "S"), ("bocf_set_candidates", "bocf_posterior_samples"))
def _posterior_samples(model, i):
    return model.posterior_samples_f(i["X"], Z=i["Zs"]), model.last_sample_jitter


def _path_groups(model, n):
    """Hyper-sample of path s, as draw_paths assigns it."""
    return np.arange(n) % min(10, model._H)


@call("thompson_topk", ("C", "P", "k"), ("bocf_set_candidates", "bocf_posterior_samples", "bocf_thompson_select"))
def _thompson_topk(model, i):
    groups = _path_groups(model, i["n"]["P"])
    Z = {int(h): np.stack([i["Zpath"][s] for s in np.flatnonzero(groups == h)], axis=2) for h in set(groups.tolist())}
    return model.thompson_topk(i["X"], i["thetasP"], groups, Z, _utility(i["thetasP"]), i["n"]["k"])


@call("paths", ("C", "P", "F", "k"), ("bocf_set_paths", "bocf_path_values", "bocf_path_utility", "bocf_thompson_select"))
def _paths(model, i):
    U = _utility(i["thetasP"])
    with seeded_global_stream(i["seed"]):
        model.draw_paths(i["n"]["P"], i["n"]["F"])
    values = model.path_values(i["X"])
    u, du = model.path_utility(i["X"], i["row_path"], i["thetasP"], U, grad=True)
    idx, val = model.pathwise_topk(i["X"], i["thetasP"], model._path_groups(i["n"]["P"]), U, i["n"]["k"])
    return values, u, du, idx, val


# ---- refinement -----------------------------------------------------------------------------------------------------------------------
def _refined(out):
    X, Fv, info = out
    return X, Fv, info["iterations"], info["evaluations"]


@call("refine_linear", ("A", "L"), ("bocf_refine_acq",))
def _refine_linear(model, i):
    return _refined(model.refine_acq(i["X"], i["bounds"], F.REFINE_LINEAR, kind=F.ACQ_EI, thetas=i["thetas"], prob=i["prob"], maxiter=5))


@call("refine_mc", ("A", "S", "L"), ("bocf_set_mc_samples", "bocf_refine_acq"))
def _refine_mc(model, i):
    return _refined(model.refine_acq(i["X"], i["bounds"], F.REFINE_MC, util_kind=KIND, thetas=i["thetas"], prob=i["prob"], W=i["W"], maxiter=5))


# ---- diagnostics ----------------------------------------------------------------------------------------------------------------------
@call("loo", (), ("bocf_loo",))
def _loo(model, i):
    return model.loo() + (model.loo_log_likelihood(),)


@call("loo_utility", ("L", "S"), ("bocf_set_eu_samples", "bocf_loo_utility"))
def _loo_utility(model, i):
    closed = model.loo_utility(_utility(i["thetas"]), Z=i["Zeu"])[0]      # (Z is read only if this m has no closed form)
    L = i["n"]["L"]
    V = B.Utility(parameter_dist=B.ParameterDistribution(support=np.zeros((L, 1)), prob_dist=np.full(L, 1.0 / L)), device="neg_exp_cos",
                  device_params=i["c"])
    return closed, model.loo_utility(V, Z=i["Zeu"])[0]


@call("lml_gradients", (), ("bocf_lml_gradients",))
def _lml_gradients(model, i):
    return model.log_likelihood_gradients()


@call("factor", (), ("bocf_get_factor", "bocf_get_train_kernel"))
def _factor(model, i):
    return model.get_factor(i["j"]) + (model.get_train_kernel(i["j"]),)


# ---- the entry points of include/bocf_hip.h that no call reaches, each with its reason ---------------------------------------------------
_MODEL_CHANGE = "acts as a model change: part of a state's replay in tests/test_gpu_history.py, on the busy and on the new context alike"
_MULTI_RANK = "multi-rank selection: needs a communicator or a peer's packed buffer (tests/test_00_gpu_rccl.py, tests/test_gpu_select.py)"
_PLUMBING = "returns no number of the model"
EXCLUDED = {
    "bocf_version": _PLUMBING,
    "bocf_last_error": _PLUMBING,
    "bocf_create": _PLUMBING + ": every new context of the reference goes through it",
    "bocf_destroy": _PLUMBING,
    "bocf_sync": _PLUMBING,
    "bocf_option_count": "the option table, readable without a context",
    "bocf_option_info": "the option table, readable without a context",
    "bocf_option_check": "the option table, readable without a context",
    "bocf_profile_read": "profiling: event times, no result",
    "bocf_profile_phase": "profiling: event times, no result",
    "bocf_get_stat": "diagnostic counters; none of them changes a result",
    "bocf_comm_unique_id": _MULTI_RANK,
    "bocf_comm_init": _MULTI_RANK,
    "bocf_comm_destroy": _MULTI_RANK,
    "bocf_comm_info": _MULTI_RANK,
    "bocf_global_topk": _MULTI_RANK,
    "bocf_topk_packed": _MULTI_RANK,
    "bocf_merge_packed": _MULTI_RANK,
    "bocf_fit": _MODEL_CHANGE,
    "bocf_set_kernel_ids": _MODEL_CHANGE + " (consumed by the next fit)",
    "bocf_update_targets": _MODEL_CHANGE,
    "bocf_append": _MODEL_CHANGE,
    "bocf_remove": _MODEL_CHANGE,
    "bocf_infer": _MODEL_CHANGE,
    "bocf_hmc": _MODEL_CHANGE + " (the update of the learning-mode model)",
    "bocf_hmc_streamed": _MODEL_CHANGE + " (the update of a learning-mode model beyond the fused kernel; tests/test_gpu_round3.py)",
    "bocf_last_fit_info": "read only after a failed factorization, which no state of these tests has",
    "bocf_set_posterior": "replaces the model by a host-given posterior (a test hook of the acquisition kernels): no fitted state to keep",
    "bocf_lbfgsb_batched": "host arithmetic without a context: it has no call history",
    "bocf_check_utility_program": "host-only check without a context: it has no call history",
}
