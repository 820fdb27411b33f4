"""The recommendation step of the BOCF loop (cbo.py:61-84,121-235): for every utility parameter theta_l of one
_current_max_value, the argument of the maximum of the posterior expected utility

    x_l = argmax_x  sum_{h < n_hyps} E_n[ U(theta_l, f(x)) ]

found as GeneralOptimizer('lbfgs').optimize finds it (GPyOpt/optimization/general_optimizer.py:53-94): 200 random starts
scored by the objective, the best 24 refined with L-BFGS-B (factr=1e6, maxiter=500), the best optimum taken unless the
best anchor's own value is lower.  The reference solves the L problems one after the other, every objective call a Python
loop over hyper-samples, points and Monte-Carlo samples.  Here the L problems advance TOGETHER: all L x 200 starts are scored
in one device call, all L x 24 anchors are refined by one batched L-BFGS whose every step is one device call
(bocf_expected_utility: each row carries its own parameter index), and the optima are re-evaluated in one more call.

Random numbers are drawn exactly as the reference draws them, all before any device work: for each parameter in order,
first its Monte-Carlo normals Z (np.random.normal(size=(50, m)), cbo.py:200; Monte-Carlo branch only), then its random
design (one np.random.uniform per input dimension, random_design.py:67-77).  The reference evaluates the objective at
x_l between two parameters; the CBO loop here evaluates it after all L problems are solved, so the objective must not use
np.random (MultiObjective.evaluate does not; evaluate_w_noise, which does, is not called here).

The objective of the inner problems takes one of three forms (cbo.py:124-233): the posterior mean theta . mu when the
utility is linear, the closed-form expectation psi when an ExpectationUtility is given, Monte-Carlo otherwise.  A psi that
is the closed form of the utility's device kind, or a device utility in the Monte-Carlo branch, runs on the device; any
other callable runs the reference's loops on the host over the model's public per-hyper-sample methods.
"""
import warnings

import numpy as np

from . import _ffi
from .acquisition_optimizer import _bounds_of, lbfgsb_batched, samples_multidimensional_uniform
from .utility import device_utility, expectation_mode

N_Z_SAMPLES = 50                  # cbo.py:200


def branch_of(utility, expectation_utility=None):
    """Which form the reference's _current_marginal_argmax takes (cbo.py:124, 159, 190)."""
    if utility.linear:
        return "mean"
    if expectation_utility is not None:
        return "closed"
    return "mc"


def draw_inputs(space, branch, n_parameters, m, n_starting=200, always_Z=False):
    """The random numbers of one _current_max_value after its parameter draw, in the reference's order: per parameter, Z (50, m)
    (Monte-Carlo branch only; with always_Z -- the constrained step, which has the Monte-Carlo form only -- in every branch) then the
    (n_starting, d) random design.  Returns (Z (L, 50, m) or None, designs (L, n_starting, d))."""
    bounds = _bounds_of(space)
    Zs, designs = [], []
    for _ in range(n_parameters):
        if branch == "mc" or always_Z:
            Zs.append(np.random.normal(size=(N_Z_SAMPLES, m)))
        designs.append(samples_multidimensional_uniform(bounds, n_starting))
    return (np.stack(Zs) if Zs else None), np.stack(designs)


def closed_form(kind, theta, mu, var):
    """psi(theta, mu, var) = E[U(theta, y)], y ~ N(mu, diag(var)), and its gradient [dpsi/dmu; dpsi/dvar] (2m,) for the device
    utilities that have one (the psi / psi_gradient of the reference's experiment scripts)."""
    theta = np.atleast_1d(np.asarray(theta, dtype=float)).reshape(-1)
    mu, var = np.asarray(mu, dtype=float).reshape(-1), np.asarray(var, dtype=float).reshape(-1)
    m = mu.size
    if kind == "neg_sq_dist":
        t = mu - theta
        return -np.sum(t * t) - np.sum(var), np.concatenate((-2.0 * t, -np.ones(m)))
    if kind == "neg_sum_exp":
        e = np.exp(mu + 0.5 * var)
        return -np.sum(e), np.concatenate((-e, -0.5 * e))
    if kind == "rosenbrock":
        h, a = m // 2, theta[0]
        v = -np.sum((a - mu[:h]) ** 2 + 100.0 * mu[h:2 * h] ** 2 + var[:h] + 100.0 * var[h:2 * h])
        return v, np.concatenate((2.0 * (a - mu[:h]), -200.0 * mu[h:2 * h], -np.ones(h), -100.0 * np.ones(h)))
    raise ValueError("no closed-form expectation for utility %r" % (kind,))


def recognise_expectation_utility(expectation_utility, utility, m, theta=None):
    """Name of the device utility whose closed-form expectation `expectation_utility` (psi, psi_gradient) computes, or None.
    Like Utility._recognise: psi and its gradient are probed at fixed points drawn from a private RNG (the global np.random
    stream is not touched) and compared with the closed form of the utility's own device kind."""
    try:
        kind = utility.device_kind(m)
    except NotImplementedError:
        return None
    if expectation_mode(kind, m) != _ffi.EU_CLOSED:
        return None
    kind = device_utility(kind).name
    if theta is None:
        support = getattr(utility.parameter_dist, "support", None)
        if support is None or len(support) == 0:
            return None
        theta = support[0]
    theta = np.asarray(theta, dtype=float)
    rng = np.random.RandomState(20180103)
    try:
        for _ in range(4):
            mu, var = rng.uniform(-1.0, 1.0, size=m), rng.uniform(0.01, 1.0, size=m)
            v = float(np.squeeze(expectation_utility.func(theta, mu, var)))
            g = np.asarray(expectation_utility.gradient(theta, mu, var), dtype=float).reshape(-1)
            cv, cg = closed_form(kind, theta, mu, var)
            if g.shape != cg.shape or not np.isfinite(v) or not np.all(np.isfinite(g)):
                return None
            if abs(v - cv) > 1e-9 * (1.0 + abs(cv)) or np.any(np.abs(g - cg) > 1e-9 * (1.0 + np.abs(cg))):
                return None
    except Exception:
        return None
    return kind


def device_evaluator(model, branch, utility, parameters, Z=None, n_hyps=None, kind=None):
    """ev(X, rows, grad) -> (v (n,), dv/dX (n, d) or None): sum_h E_h[U(theta_{rows[i]}, f(X_i))] from bocf_expected_utility."""
    thetas = np.asarray(parameters, dtype=float).reshape(len(parameters), -1)
    if kind is None and branch != "mean":
        kind = device_utility(utility.device_kind(model.output_dim)).name

    def ev(X, rows, grad=False):
        # (a utility program travels with its Utility: the model stages the blob)
        out = model.expected_utility(X, branch, (utility if kind == "program" else kind) if branch != "mean" else None, thetas, rows, Z=Z,
                                     n_hyps=n_hyps, grad=grad, util_params=utility.device_params)
        return out if grad else (out, None)
    return ev


def host_evaluator(model, branch, utility, parameters, expectation_utility=None, Z=None, n_hyps=None):
    """The same callable as `device_evaluator`, computed by the reference's loops (cbo.py:124-231) with the user's callables over
    the model's public per-hyper-sample methods (set_hyperparameters(h), posterior_mean / predict_noiseless and the gradients):
    the path for a utility or psi outside the device's closed set."""
    n_h = min(10, model.number_of_hyps_samples()) if n_hyps is None else int(n_hyps)
    m = model.output_dim

    def ev(X, rows, grad=False):
        X = np.atleast_2d(X)
        rows = np.asarray(rows).reshape(-1)
        n, d = X.shape
        val, dval = np.zeros(n), np.zeros((n, d))
        for l in np.unique(rows):
            sel = np.flatnonzero(rows == l)
            Xl, theta = X[sel], parameters[l]
            for h in range(n_h):
                model.set_hyperparameters(h)
                if branch == "mean":
                    mu = model.posterior_mean(Xl)
                    val[sel] += np.reshape(theta * mu if m == 1 else np.matmul(theta, mu), (len(sel),))
                    if grad:
                        dmu = model.posterior_mean_gradient(Xl)
                        dval[sel] += np.reshape(theta * dmu if m == 1 else np.tensordot(theta, dmu, axes=1), (len(sel), d))
                    continue
                mean, var = model.predict_noiseless(Xl)
                if grad:
                    dmean, dvar = model.posterior_mean_gradient(Xl), model.posterior_variance_gradient(Xl)
                if branch == "closed":
                    for i, r in enumerate(sel):
                        val[r] += float(np.squeeze(expectation_utility.func(theta, mean[:, i], var[:, i])))
                        if grad:
                            g = np.asarray(expectation_utility.gradient(theta, mean[:, i], var[:, i]), dtype=float)
                            dval[r] += np.matmul(g, np.concatenate((dmean, dvar))[:, i])
                    continue
                std = np.sqrt(var)
                for i, r in enumerate(sel):
                    if grad:
                        dstd = dvar[:, i, :] / (2.0 * std[:, i])[:, None]
                    for z in Z[l]:
                        y = mean[:, i] + z * std[:, i]
                        val[r] += float(np.squeeze(utility.eval_func(theta, y)))
                        if grad:
                            dval[r] += np.matmul(np.asarray(utility.eval_gradient(theta, y), dtype=float), dmean[:, i, :] + (dstd.T * z).T)
        return val, (dval if grad else None)
    return ev


def optimize_batched(evaluator, designs, bounds, n_anchor=24, info=None):
    """GeneralOptimizer.optimize (general_optimizer.py:53-94) for L problems at once.  designs (L, P, d): the random starts of every
    problem; evaluator(X, rows, grad) returns the quantity to MAXIMISE for parameter rows[i] (the reference minimises its
    negative).  Returns (x (L, d), value (L,): the maximised quantity at x)."""
    designs = np.asarray(designs, dtype=float)
    L, P, d = designs.shape
    scores = -evaluator(designs.reshape(L * P, d), np.repeat(np.arange(L), P), False)[0]
    scores = np.asarray(scores, dtype=float).reshape(L, P)
    k = min(P, n_anchor)
    # anchor_points_generator.py:59-61 as ObjectiveAnchorPointsGenerator restates it: lowest scores first, ties to the lowest index
    idx = np.stack([np.argsort(scores[l], kind="stable")[:k] for l in range(L)])
    anchors = np.concatenate([designs[l][idx[l]] for l in range(L)])
    anchor_values = np.stack([scores[l][idx[l]] for l in range(L)])
    arow = np.repeat(np.arange(L), k)

    def f_df(X, rows):
        v, g = evaluator(X, arow[rows], True)
        return -np.asarray(v), -np.asarray(g)
    lb_info = {}
    Xopt, _ = lbfgsb_batched(f_df, anchors, bounds, maxiter=500, factr=1e6, info=lb_info, with_rows=True)
    fx = -np.asarray(evaluator(Xopt, arow, False)[0], dtype=float).reshape(L, k)     # optimizer.py:464, one batch
    x_best, f_best = np.empty((L, d)), np.empty(L)
    for l in range(L):
        b = int(np.argmin(fx[l]))                        # min(optimized_points, key=fx): first of equal minima
        x_best[l], f_best[l] = Xopt[l * k + b], fx[l, b]
        if anchor_values[l, 0] < f_best[l]:             # general_optimizer.py:89-93
            x_best[l], f_best[l] = anchors[l * k], anchor_values[l, 0]
    if info is not None:
        info.update(anchors=anchors.reshape(L, k, d), anchor_values=anchor_values, optimized_points=Xopt.reshape(L, k, d), optimized_values=fx,
                    **lb_info)
    return x_best, -f_best


def constrained_device_evaluator(model, utility, parameters, Z, u_infeasible, n_hyps=None):
    """ev(X, rows, grad) -> (G (n,), dG/dX (n, d) or None) from bocf_expected_utility_constrained (the constraints are resident on the
    model), and ev.pof(X, rows) -> the smoothed probability of feasibility (n,).  The utility's compiled-in device kind in every branch
    (the linear kind for a linear utility); a utility without one raises NotImplementedError: this path has no host loop."""
    m = model.output_dim
    kind = _ffi.UTIL_LINEAR if utility.linear else utility.device_kind(m)
    if kind == _ffi.UTIL_PROGRAM:
        raise NotImplementedError("the constrained recommendation step takes the compiled-in device utilities only, not a utility program")
    thetas = np.asarray(parameters, dtype=float).reshape(len(parameters), -1)

    def ev(X, rows, grad=False):
        out = model.expected_utility_constrained(X, kind, thetas, rows, u_infeasible, Z, n_hyps=n_hyps, grad=grad, util_params=utility.device_params)
        return (out[0], out[2]) if grad else (out[0], None)
    ev.pof = lambda X, rows: model.expected_utility_constrained(X, kind, thetas, rows, u_infeasible, Z, n_hyps=n_hyps,
                                                                util_params=utility.device_params)[1]
    return ev


def current_marginal_argmaxes(model, space, utility, parameters, expectation_utility=None, n_hyps=None, n_starting=200, n_anchor=24,
                              evaluator=None, info=None, constraints=None, infeasible_utility=None):
    """x_l = argmax_x sum_{h < n_hyps} E_n[U(theta_l, f(x))] for every row theta_l of `parameters`, all in one batch (what
    cbo.py:121-235 computes for one parameter).  Draws Z and the random designs first (see the module docstring), then
    scores, refines and selects on the device.  n_hyps defaults to min(10, model.number_of_hyps_samples()) (cbo.py:52).
    `evaluator(parameters, Z)`, if given, builds the objective in place of the model's: it returns a callable ev(X, rows, grad) ->
    (sum_h E_h[U(theta_{rows[i]}, f(X_i))] (n,), its gradient (n, d) or None) -- e.g. a CPU restatement; Z is None outside the
    Monte-Carlo branch.  By default the device evaluates it, or the host loops when the utility / psi is outside the device's
    closed set.  Returns (x (L, d), values (L,)); `info`, if a dict, receives Z, the designs, the anchors and the L-BFGS counters.

    constraints: an OutputConstraints makes the step feasibility-aware: the objective becomes the constrained
    expected utility  sum_h sum_s [u0_l + phi(y_s) (U(theta_l, y_s) - u0_l)], an infeasible outcome worth u0_l = infeasible_utility (a
    scalar or (L,); default: the min of U(theta_l, mu(X_i)) over the training points, model.train_utility_range).  The constraints are
    staged on the model (free when already resident).  There is no mean or closed form once phi multiplies the utility: every branch
    takes the Monte-Carlo form, so Z is drawn in every branch, in the Monte-Carlo branch's order -- the draws from np.random differ from
    the unconstrained call's only then.  `evaluator(parameters, Z, constraints, u_infeasible)` then takes two more arguments, and its
    callable may carry ev.pof(X, rows).  `info` additionally receives pof (L,) at the returned points and u_infeasible (L,)."""
    parameters = np.asarray(parameters, dtype=float)
    if parameters.ndim == 1:
        parameters = parameters[:, None]
    L, m = len(parameters), model.output_dim
    n_h = min(10, model.number_of_hyps_samples()) if n_hyps is None else int(n_hyps)
    branch = branch_of(utility, expectation_utility)
    if constraints is None:
        if infeasible_utility is not None:
            raise ValueError("infeasible_utility is the worth of an outcome that violates `constraints`: give them")
        Z, designs = draw_inputs(space, branch, L, m, n_starting)
        ev = make_evaluator(model, branch, utility, parameters, expectation_utility, Z, n_h) if evaluator is None else evaluator(parameters, Z)
        if info is not None:
            info.update(Z=Z, designs=designs, branch=branch)
        return optimize_batched(ev, designs, _bounds_of(space), n_anchor, info)
    Z, designs = draw_inputs(space, branch, L, m, n_starting, always_Z=True)
    if evaluator is None:
        model.set_output_constraints(constraints)
    if infeasible_utility is None:
        kind = _ffi.UTIL_LINEAR if utility.linear else utility.device_kind(m)
        u0 = np.asarray(model.train_utility_range(kind, utility.device_params, parameters)[0], dtype=float)
    else:
        u0 = np.array(np.broadcast_to(np.asarray(infeasible_utility, dtype=float), (L,)))
    if not np.all(np.isfinite(u0)):
        raise ValueError("infeasible_utility must be finite")
    ev = constrained_device_evaluator(model, utility, parameters, Z, u0, n_h) if evaluator is None else evaluator(parameters, Z, constraints, u0)
    if info is not None:
        info.update(Z=Z, designs=designs, branch=branch)
    X, values = optimize_batched(ev, designs, _bounds_of(space), n_anchor, info)
    if info is not None:
        info.update(u_infeasible=u0, pof=np.asarray(ev.pof(X, np.arange(L)), dtype=float) if hasattr(ev, "pof") else None)
    return X, values


def make_evaluator(model, branch, utility, parameters, expectation_utility=None, Z=None, n_hyps=None):
    """The device evaluator when the form is on the device (a linear utility; a device utility in the Monte-Carlo branch; a psi
    recognised as the closed form of the utility's device kind), else the host loops (with a warning)."""
    if branch == "mean":
        return device_evaluator(model, branch, utility, parameters, Z, n_hyps)
    if branch == "closed":
        kind = recognise_expectation_utility(expectation_utility, utility, model.output_dim, parameters[0])
    else:
        try:
            kind = device_utility(utility.device_kind(model.output_dim)).name
        except NotImplementedError:
            kind = None
    if kind is not None:
        return device_evaluator(model, branch, utility, parameters, Z, n_hyps, kind=kind)
    warnings.warn("bocf_amd: the %s is a Python callable outside the device's closed set: the recommendation step evaluates it on the "
                  "HOST, point by point (the posterior still comes from the GPU)"
                  % ("expectation utility" if branch == "closed" else "utility"), RuntimeWarning, stacklevel=3)
    return host_evaluator(model, branch, utility, parameters, expectation_utility, Z, n_hyps)
