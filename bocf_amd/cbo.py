"""The BOCF loop with the reference's surface (cbo.py:19-420: CBO) plus the evaluator it is driven by
(GPyOpt/core/evaluators/sequential.py: Sequential).

    bo = bocf_amd.CBO(model, space, objective, acquisition, bocf_amd.Sequential(acquisition), X_init, expectation_utility=psi)
    bo.run_optimization(max_iter, results_file="results.txt")

Every iteration does what the reference does, in the same order and with the same draws from np.random: the acquisition is
optimised from the current recommendation (x_baseline = current_argmax), a repeated suggestion is perturbed, the objective is
evaluated with noise, the model is updated, and the recommendation step (_current_max_value) solves one argmax problem per
utility parameter -- here all of them in one batch on the device (bocf_amd.recommend) -- and records
sum_l p_l U(theta_l, f(x_l)) in historical_optimal_values.  Elapsed times use time.perf_counter (the reference's time.clock no
longer exists in Python 3).  Plotting, context variables, a non-constant cost and the convergence-assessment helpers are not
provided: they raise NotImplementedError.
"""
import time

import numpy as np

from .acquisition_optimizer import ContextManager, _bounds_of, lbfgsb_batched, samples_multidimensional_uniform
from .recommend import current_marginal_argmaxes


class Sequential(object):
    """GPyOpt/core/evaluators/sequential.py: one suggestion per iteration, from acquisition.optimize."""

    def __init__(self, acquisition, batch_size=1):
        self.acquisition = acquisition
        self.batch_size = batch_size

    def compute_batch(self, duplicate_manager=None, context_manager=None, x_baseline=None):
        x, _ = self.acquisition.optimize(duplicate_manager=duplicate_manager, x_baseline=x_baseline)
        return x


class CompositeThompsonBatch(object):
    """q suggestions per iteration by Thompson sampling on the composite objective.  The first point is acquisition.optimize's, as in
    Sequential (batch_size = 1 is Sequential).  Each of the q - 1 others is the argmax over a random candidate design of
    U(theta_s, f_s(c)), with f_s a joint posterior sample of all outputs on the design and theta_s a draw of the utility parameter.
    Draws from np.random, in this order: the design (samples_multidimensional_uniform, one np.random.uniform per dimension), theta for
    all paths (utility.parameter_dist.sample(q - 1)), then the normals Z (m, n_candidates, paths of h) of every hyper-sample h used, in
    increasing h.  Path s uses hyper-sample s mod min(10, number_of_hyps_samples()).  Path s takes its best candidate not taken by an
    earlier path of the batch (model.thompson_topk gives each path its top q).  (GPyOpt's ThompsonBatch samples each output's marginal
    and assumes a single-output model; this is a different method, hence the different name.)"""

    def __init__(self, acquisition, batch_size, n_candidates=4096):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        if int(batch_size) > int(n_candidates) or int(batch_size) > 64:
            raise ValueError("batch_size must be <= min(n_candidates, 64)")
        self.acquisition = acquisition
        self.batch_size = int(batch_size)
        self.n_candidates = int(n_candidates)

    def compute_batch(self, duplicate_manager=None, context_manager=None, x_baseline=None):
        x0, _ = self.acquisition.optimize(x_baseline=x_baseline)
        x0 = np.atleast_2d(x0)
        q = self.batch_size
        if q == 1:
            return x0
        model, utility = self.acquisition.model, self.acquisition.utility
        P = q - 1
        Xc = samples_multidimensional_uniform(_bounds_of(self.acquisition.space), self.n_candidates)
        thetas = np.asarray(utility.parameter_dist.sample(P), dtype=float).reshape(P, -1)
        n_h = min(10, model.number_of_hyps_samples())
        groups = np.arange(P) % n_h
        Z = {h: np.random.normal(size=(model.output_dim, self.n_candidates, int(np.sum(groups == h)))) for h in sorted(set(groups.tolist()))}
        idx, _ = model.thompson_topk(Xc, thetas, groups, Z, utility, q)
        return np.vstack((x0, Xc[distinct_picks(idx)]))


class CompositePathwiseThompsonBatch(object):
    """q suggestions per iteration by Thompson sampling on the composite objective with sample paths that are FUNCTIONS of x
    (model.draw_paths: Matheron's rule with random Fourier features).  The first point is acquisition.optimize's, as in Sequential
    (batch_size = 1 is Sequential).  Each of the q - 1 others is a path's argmax of U(theta_s, f_s(.)): the paths score a random design of
    n_candidates points (no candidate covariance is formed, so the design is as large as any acquisition's), path s takes its best
    candidate not taken by an earlier path (model.pathwise_topk gives each path its top q), and with `refine` all picks are refined at
    once by the batched L-BFGS-B inside the space's bounds on the paths' own value and gradient (model.path_utility, one device call per
    step).  A refined point is kept only where its path utility is not lower than its pick's and it does not repeat an earlier point of
    the batch; `last_refinement` records picks, refined points and both utilities.
    Draws from np.random, in this order: the design (samples_multidimensional_uniform, one np.random.uniform per dimension), theta for
    all paths (utility.parameter_dist.sample(q - 1)), then model.draw_paths(q - 1, n_features): per hyper-sample used, in increasing h,
    per output the frequencies z (F, d), chi2 (F,) for the Matern kernels only, the phases b (F,), the weights w (F, paths of h) and the
    noise draws E (N, paths of h).  Path s uses hyper-sample s mod min(10, number_of_hyps_samples()).
    Given the frequencies a path's mean is the posterior mean exactly; its variance is that of the feature approximation."""

    def __init__(self, acquisition, batch_size, n_candidates=65536, n_features=1024, refine=True):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        if int(batch_size) > int(n_candidates) or int(batch_size) > 64:
            raise ValueError("batch_size must be <= min(n_candidates, 64)")
        if int(n_features) < 1:
            raise ValueError("n_features must be >= 1")
        self.acquisition = acquisition
        self.batch_size = int(batch_size)
        self.n_candidates = int(n_candidates)
        self.n_features = int(n_features)
        self.refine = bool(refine)
        self.last_refinement = None

    def compute_batch(self, duplicate_manager=None, context_manager=None, x_baseline=None):
        x0, _ = self.acquisition.optimize(x_baseline=x_baseline)
        x0 = np.atleast_2d(x0)
        q = self.batch_size
        if q == 1:
            return x0
        model, utility = self.acquisition.model, self.acquisition.utility
        P = q - 1
        bounds = _bounds_of(self.acquisition.space)
        Xc = samples_multidimensional_uniform(bounds, self.n_candidates)
        thetas = np.asarray(utility.parameter_dist.sample(P), dtype=float).reshape(P, -1)
        groups = np.arange(P) % min(10, model.number_of_hyps_samples())
        model.draw_paths(P, self.n_features)
        idx, _ = model.pathwise_topk(Xc, thetas, groups, utility, q)
        picks = Xc[distinct_picks(idx)]
        if not self.refine:
            return np.vstack((x0, picks))
        paths = np.arange(P)
        u_pick = np.asarray(model.path_utility(picks, paths, thetas, utility), dtype=float)

        def f_df(X, rows):
            v, g = model.path_utility(X, paths[rows], thetas, utility, grad=True)
            return -np.asarray(v), -np.asarray(g)
        refined, _ = lbfgsb_batched(f_df, picks, bounds, with_rows=True)
        u_ref = np.asarray(model.path_utility(refined, paths, thetas, utility), dtype=float)
        batch, kept = [x0[0]], np.zeros(P, dtype=bool)
        for s in range(P):
            kept[s] = bool(u_ref[s] >= u_pick[s]) and not any(np.array_equal(refined[s], b) for b in batch)
            batch.append(refined[s] if kept[s] else picks[s])
        self.last_refinement = {"picks": picks, "pick_values": u_pick, "refined": refined, "refined_values": u_ref, "kept": kept}
        return np.vstack(batch)


class CompositeGreedyBatch(object):
    """q <= 16 suggestions per iteration by greedily maximising the joint Monte-Carlo expected improvement of the composite utility
    (q-uEI): point k maximises alpha(x | p_1 .. p_{k-1}) = qEI({p_1 .. p_{k-1}, x}) - qEI({p_1 .. p_{k-1}}) with the earlier points
    pending.  `acquisition` is a bocf_amd.uEI_pending.  The first point is acquisition.optimize's with no pending point, as in Sequential
    (batch_size = 1 is Sequential).  Draws from np.random, in this order: whatever the optimisation of point 1 draws, then ONE
    np.random.normal(size=(S, m, q - 1)) for the whole batch (S = len(acquisition.W_samples)), then whatever the optimisations of points
    2 .. q draw.  Step k uses the pending points found so far and the leading k - 1 columns of that array: the joint sample at the
    pending points is mu(P) + L z with L the lower Cholesky factor of Sigma(P, P) + tau I, whose leading block does not change when a
    point is appended, so the samples at the earlier pending points stay fixed across the steps of a batch (up to the jitter tau, 1e-8
    of the mean variance of the pending points, which is recomputed per step).  The pending points are cleared at the end, also when a
    step raises."""

    def __init__(self, acquisition, batch_size):
        if not 1 <= int(batch_size) <= 16:
            raise ValueError("batch_size must be in 1 .. 16")
        if not hasattr(acquisition, "set_pending_points"):
            raise TypeError("CompositeGreedyBatch needs an acquisition with set_pending_points (bocf_amd.uEI_pending)")
        self.acquisition = acquisition
        self.batch_size = int(batch_size)

    def compute_batch(self, duplicate_manager=None, context_manager=None, x_baseline=None):
        acq, q = self.acquisition, self.batch_size
        acq.set_pending_points(None)
        try:
            x, _ = acq.optimize(duplicate_manager=duplicate_manager, x_baseline=x_baseline)
            X = np.atleast_2d(x)
            if q == 1:
                return X
            S, m = acq.W_samples.shape
            Z = np.random.normal(size=(S, m, q - 1))
            for k in range(1, q):
                acq.set_pending_points(X, np.ascontiguousarray(Z[:, :, :k]))
                x, _ = acq.optimize(duplicate_manager=duplicate_manager, x_baseline=x_baseline)
                X = np.vstack((X, np.atleast_2d(x)))
            return X
        finally:
            acq.set_pending_points(None)


class CompositeJointBatch(object):
    """q <= 8 suggestions per iteration by maximising the joint Monte-Carlo expected improvement of the composite utility (q-uEI) over all
    q points together.  `acquisition` is a bocf_amd.uEI_joint with q = batch_size.  compute_batch draws n_starting random batches, scores
    them in one device call, keeps the n_anchor best as anchors, adds the batch of `warm_start` (any evaluator whose compute_batch returns
    (q, d), e.g. a CompositeGreedyBatch) as one more anchor, refines all anchors together on -alpha with the batched L-BFGS-B inside the
    bounds (lbfgsb_batched, which has no limit on the q * d dimensions; its arc search only accepts decreases of -alpha), scores the
    refined batches again and returns the best as (q, d).  `last_info` records anchors, their values, the refined batches and theirs.
    Draws from np.random, in this order: the starting design (samples_multidimensional_uniform over the bounds tiled q times: one
    np.random.uniform per coordinate of a batch, q * d calls), then whatever warm_start.compute_batch draws, then -- only without full
    support of the utility parameter -- one parameter per gradient call of the refinement."""

    def __init__(self, acquisition, batch_size, n_starting=256, n_anchor=16, warm_start=None):
        if not 1 <= int(batch_size) <= 8:
            raise ValueError("batch_size must be in 1 .. 8")
        if not hasattr(acquisition, "Z_samples") or getattr(acquisition, "q", None) != int(batch_size):
            raise TypeError("CompositeJointBatch needs a bocf_amd.uEI_joint acquisition with q = batch_size")
        if int(n_anchor) < 1 or int(n_starting) < int(n_anchor):
            raise ValueError("1 <= n_anchor <= n_starting")
        if warm_start is not None and not hasattr(warm_start, "compute_batch"):
            raise TypeError("warm_start must be a batch evaluator (compute_batch)")
        self.acquisition = acquisition
        self.batch_size = int(batch_size)
        self.n_starting, self.n_anchor = int(n_starting), int(n_anchor)
        self.warm_start = warm_start
        self.last_info = None

    def compute_batch(self, duplicate_manager=None, context_manager=None, x_baseline=None):
        acq, q = self.acquisition, self.batch_size
        bounds = _bounds_of(acq.space) * q
        starts = samples_multidimensional_uniform(bounds, self.n_starting)
        values = np.asarray(acq._compute_acq(starts), dtype=float).reshape(-1)
        anchors = starts[np.argsort(-values, kind="stable")[:self.n_anchor]]
        if self.warm_start is not None:
            warm = np.asarray(self.warm_start.compute_batch(duplicate_manager=duplicate_manager, context_manager=context_manager, x_baseline=x_baseline),
                              dtype=float)
            if warm.size != anchors.shape[1]:
                raise ValueError("warm_start returned %r, not (q, d) = (%d, %d)" % (warm.shape, q, anchors.shape[1] // q))
            anchors = np.vstack((anchors, warm.reshape(1, -1)))
        lo, hi = np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds])
        anchors = np.minimum(np.maximum(anchors, lo), hi)
        anchor_values = np.asarray(acq._compute_acq(anchors), dtype=float).reshape(-1)

        def f_df(X):
            f, g = acq.acquisition_function_withGradients(X)
            return np.asarray(f).reshape(-1), np.asarray(g)
        refined, _ = lbfgsb_batched(f_df, anchors, bounds)
        refined_values = np.asarray(acq._compute_acq(refined), dtype=float).reshape(-1)
        # the best of everything scored under the one set of parameters _compute_acq uses: a refined batch, or its start where the
        # gradient calls saw another parameter draw
        pool, pool_values = np.vstack((refined, anchors)), np.concatenate((refined_values, anchor_values))
        best = int(np.argmax(pool_values))
        self.last_info = {"anchors": anchors, "anchor_values": anchor_values, "refined": refined, "refined_values": refined_values,
                          "value": float(pool_values[best])}
        return pool[best].reshape(q, -1)


def distinct_picks(idx):
    """Row s of idx ranks path s's candidates; path s takes its first candidate that no earlier path took."""
    taken = []
    for row in np.asarray(idx):
        pick = next((int(i) for i in row if int(i) >= 0 and int(i) not in taken), None)
        if pick is None:
            raise RuntimeError("a Thompson path found no candidate left untaken in its top %d" % len(row))
        taken.append(pick)
    return np.asarray(taken, dtype=int)


class _ConstantCost(object):
    """GPyOpt's CostModel(None): every evaluation costs the same; nothing to update."""
    cost_type = "Constant cost"

    def update_cost_model(self, x, cost_x):
        pass


def _repeats(x, previous):
    """The suggestion repeats the previous batch: for one row, equal to it (broadcast against previous, as the reference compares);
    for q rows, the same shape and every entry equal."""
    x, previous = np.asarray(x), np.asarray(previous)
    if x.ndim == 2 and x.shape[0] == 1:
        return bool(np.all(x == previous))
    return x.shape == previous.shape and bool(np.all(x == previous))


def _zip(space, X):
    return space.zip_inputs(X) if hasattr(space, "zip_inputs") else X


def _unzip(space, X):
    return space.unzip_inputs(X) if hasattr(space, "unzip_inputs") else X


class CBO(object):
    """cbo.py:19-58.  model: a bocf_amd.multi_outputGP; space: a Design_space; objective: a MultiObjective (or anything with
    evaluate / evaluate_w_noise returning (list of m (n, 1) arrays, cost)); acquisition: a bocf_amd acquisition (its `utility` is
    the loop's utility); evaluator: Sequential(acquisition); X_init (n, d); expectation_utility: the closed-form E[U] (psi) of the
    recommendation step, or None (then the Monte-Carlo form, or the posterior mean for a linear utility).
    constraints: an OutputConstraints makes the recommendation step feasibility-aware (opt-in; NOT picked up from the acquisition): the
    recommended designs maximise the constrained expected utility (recommend.current_marginal_argmaxes), an infeasible outcome worth
    infeasible_utility (a scalar or one value per utility parameter; default: the lowest utility of the posterior mean at the training
    points), and a recommendation whose TRUE outputs violate constraints.feasible is scored with that worth in
    historical_optimal_values.  last_recommendation carries pof, the smoothed probability of feasibility at the recommended points.
    max_observations: a sliding window -- once the data exceed it the loop forgets one observation per acquisition before the model update
    (forget="oldest": index 0; or a callable forget(X, Y) -> index); at least 2; None (default) keeps every observation.  A window sets
    model.incremental_remove = True ON THE MODEL PASSED IN, so that its updateModel takes the delete-and-add update on the resident factor."""

    def __init__(self, model, space, objective, acquisition, evaluator, X_init, Y_init=None, cost=None, normalize_Y=False,
                 model_update_interval=1, expectation_utility=None, constraints=None, infeasible_utility=None, max_observations=None,
                 forget="oldest"):
        if cost is not None:
            raise NotImplementedError("only a constant evaluation cost is supported (cost=None)")
        self.model = model
        self.space = space
        self.objective = objective
        self.acquisition = acquisition
        self.utility = acquisition.utility
        self.expectation_utility = expectation_utility
        if constraints is None and infeasible_utility is not None:
            raise ValueError("infeasible_utility is the worth of an outcome that violates `constraints`: give them")
        self.constraints, self.infeasible_utility = constraints, infeasible_utility
        self.evaluator = evaluator
        self.X = X_init
        self.Y = Y_init
        self.normalize_Y = normalize_Y
        self.cost = _ConstantCost()
        self.model_update_interval = model_update_interval
        if max_observations is not None and int(max_observations) < 2:
            raise ValueError("max_observations must be at least 2 (or None: keep every observation)")
        if forget != "oldest" and not callable(forget):
            raise ValueError("forget is 'oldest' or a callable forget(X, Y) -> index")
        self.max_observations = None if max_observations is None else int(max_observations)
        self.forget = forget
        if self.max_observations is not None and hasattr(model, "incremental_remove"):
            model.incremental_remove = True      # the window's delete-and-add update runs on the resident factor
        self.historical_optimal_values = []
        self.historical_time = []
        self.n_attributes = self.model.output_dim
        self.n_hyps_samples = min(10, self.model.number_of_hyps_samples())
        self.n_parameter_samples = 10
        self.full_parameter_support = self.utility.parameter_dist.use_full_support
        self.n_starting, self.n_anchor = 200, 24        # GeneralOptimizer.optimize's defaults (general_optimizer.py:53)
        self.context = None
        self.current_argmax = np.atleast_2d(X_init[0, :])
        self.last_recommendation = {}
        self.verbosity = False

    # ---- recommendation step -------------------------------------------------------------------------------------------------
    def _recommend(self, parameters):
        """argmax_x sum_h E_n[U(theta_l, f(x))] for every parameter row, in one batch; current_argmax becomes the last one."""
        info = {}
        X, _ = current_marginal_argmaxes(self.model, self.space, self.utility, parameters, self.expectation_utility,
                                         n_hyps=self.n_hyps_samples, n_starting=self.n_starting, n_anchor=self.n_anchor, info=info,
                                         **self._constraint_arguments())
        self.last_recommendation = info
        self.current_argmax = np.atleast_2d(X[-1])
        return X

    def _constraint_arguments(self):
        """The two keywords of current_marginal_argmaxes; none without constraints, so that call is the one it always was."""
        return {} if self.constraints is None else {"constraints": self.constraints, "infeasible_utility": self.infeasible_utility}

    def _marginal_value(self, parameter, x, u_infeasible=None):
        """U(theta, f(x)) with the true (noiseless) objective at one recommended point; with constraints, u_infeasible when the true
        outputs there fail constraints.feasible."""
        fx = np.reshape(self.objective.evaluate(np.atleast_2d(x))[0], (self.n_attributes,))
        if self.constraints is not None and u_infeasible is not None and not bool(self.constraints.feasible(fx)):
            return u_infeasible
        return self.utility.eval_func(parameter, fx)

    def _parameters_of_this_step(self):
        """(parameters, weights): the full support with its probabilities, or n_parameter_samples draws of parameter_dist.sample
        (the first draw of the step) with None -- a plain mean."""
        dist = self.utility.parameter_dist
        if self.full_parameter_support:
            return dist.support, dist.prob_dist
        return dist.sample(self.n_parameter_samples), None

    def _score(self, parameters, weights):
        """sum_l w_l U(theta_l, f(x_l)) over the batched recommendations (a plain mean without weights), in parameter order."""
        X = self._recommend(parameters)
        u0 = self.last_recommendation.get("u_infeasible") if self.constraints is not None else None
        terms = [self._marginal_value(parameters[l], X[l], None if u0 is None else u0[l]) for l in range(len(parameters))]
        total = 0
        for l, t in enumerate(terms):
            total = total + (t * weights[l] if weights is not None else t)
        if weights is None:
            total = total / len(parameters)
        if self.verbosity:
            print("recommended value %s" % (np.squeeze(total),))
        return np.squeeze(total)

    def _current_max_value(self):
        """E_n[U(f(x_l))] over the utility parameters of this step (cbo.py:61-84)."""
        return self._score(*self._parameters_of_this_step())

    def _current_max_value_parallel(self):
        """cbo.py:101-111 spreads the sampled parameters over a process pool; here they go through the same batched path, after the
        same parameter draw."""
        return self._score(self.utility.parameter_dist.sample(self.n_parameter_samples), None)

    def _current_marginal_max_value(self, parameter):
        x = self._current_marginal_argmax(parameter)
        u0 = self.last_recommendation.get("u_infeasible") if self.constraints is not None else None
        return self._marginal_value(parameter, x, None if u0 is None else u0[0])

    def _current_marginal_argmax(self, parameter):
        """argmax_x sum_h E_n[U(theta, f(x))] for one parameter (the batched path with L = 1); sets current_argmax."""
        return np.atleast_2d(self._recommend(np.atleast_2d(np.asarray(parameter, dtype=float)))[0])

    def _current_max_value_and_var(self):
        raise NotImplementedError("_current_max_value_and_var (cbo.py:87-98) is not provided")

    def convergence_assesment(self, *a, **kw):
        raise NotImplementedError("the convergence assessment (cbo.py:423-460) plots; plotting is not provided")

    def one_step_assesment(self, *a, **kw):
        raise NotImplementedError("the one-step assessment (cbo.py:463-495) plots; plotting is not provided")

    def integrated_plot(self, *a, **kw):
        raise NotImplementedError("plotting is not provided")

    plot_acquisition = plot_convergence = integrated_plot

    def model_check(self):
        """Leave-one-out check of the surrogate the loop currently rests on (model.loo_summary(): per output the log pseudo-likelihood,
        the rmse and the calibration of the standardised residuals).  On request only: run_optimization never calls it."""
        return self.model.loo_summary()

    # ---- the loop ------------------------------------------------------------------------------------------------------------
    def run_optimization(self, max_iter=1, parallel=False, plot=False, results_file=None, max_time=np.inf, eps=1e-8, context=None,
                         verbosity=False):
        """Run max_iter acquisitions (or until max_time seconds have passed; None for either means no limit on it, both None
        means no acquisition).  Per iteration: suggestion from x_baseline = current_argmax (perturbed if it repeats the previous
        one), noisy evaluation, model update every model_update_interval acquisitions, recommendation step; then the results file."""
        if self.objective is None:
            raise ValueError("run_optimization needs an objective")
        if plot:
            raise NotImplementedError("plotting is not provided (plot=False)")
        if context:
            raise NotImplementedError("context variables are not provided (context=None)")
        self.verbosity, self.results_file, self.context, self.eps = verbosity, results_file, context, eps
        no_limit = max_iter is None and max_time is None
        self.max_iter = 0 if no_limit else (np.inf if max_iter is None else max_iter)
        self.max_time = np.inf if (no_limit or max_time is None) else max_time
        if self.Y is None and self.X is not None:
            self.Y = self.objective.evaluate(self.X)[0]
        self.model.updateModel(self.X, self.Y)
        self.time_zero = time.perf_counter()
        self.cum_time, self.num_acquisitions = 0, 0
        self.suggested_sample, self.Y_new = self.X, self.Y
        while self.num_acquisitions < self.max_iter and self.cum_time < self.max_time:
            self._one_iteration(parallel)
        if results_file is not None:
            self.save_results(results_file)

    def _one_iteration(self, parallel):
        previous = self.suggested_sample
        x = self.compute_next_evaluations()
        self.suggested_sample = self._perturb(x) if _repeats(x, previous) else x
        try:
            # the reference calls update_Z_samples() without its required argument: the TypeError is swallowed, nothing is drawn
            self.acquisition.update_Z_samples()
        except Exception:
            pass
        self.X = np.vstack((self.X, self.suggested_sample))
        self.evaluate_objective()
        self._forget_observations()
        if self.num_acquisitions % self.model_update_interval == 0:
            self._update_model()
        self.model.get_model_parameters_names()
        self.model.get_model_parameters()
        use_parallel = parallel and not self.full_parameter_support
        value = self._current_max_value_parallel() if use_parallel else self._current_max_value()
        self.historical_optimal_values.append(value)
        self.cum_time = time.perf_counter() - self.time_zero
        self.historical_time.append(self.cum_time)
        self.num_acquisitions += 1
        if self.verbosity:
            print("iteration %d: x = %s, recommended value %s, %.2f s" % (self.num_acquisitions, self.suggested_sample, value, self.cum_time))

    def evaluate_objective(self):
        """Noisy observation at the suggestion, appended to every output's column."""
        self.Y_new, cost = self.objective.evaluate_w_noise(self.suggested_sample)
        self.cost.update_cost_model(self.suggested_sample, cost)
        self.Y = [np.vstack((old, new)) for old, new in zip(self.Y, self.Y_new)]

    def _forget_observations(self):
        """Sliding window (max_observations): while the data exceed it, one observation leaves -- index 0 (forget="oldest") or the one
        the callable forget(X, Y) names.  With one suggestion per acquisition that is one row per iteration, which the model update
        that follows takes as a removal and an append on the resident factor, O(N^2), instead of a refit."""
        if getattr(self, "max_observations", None) is None:        # (a loop object built without __init__ has no window either)
            return
        while self.X.shape[0] > self.max_observations:
            k = 0 if self.forget == "oldest" else int(self.forget(self.X, self.Y))
            if not -self.X.shape[0] <= k < self.X.shape[0]:
                raise IndexError("forget returned %d for %d observations" % (k, self.X.shape[0]))
            self.X = np.delete(self.X, k, axis=0)
            self.Y = [np.delete(y, k, axis=0) for y in self.Y]

    def _distance_last_evaluations(self):
        return float(np.linalg.norm(self.X[-1] - self.X[-2]))

    def _perturb(self, x):
        """x moved by N(0, 0.01^2) noise per coordinate (rounded to the space), redrawn until it differs from x."""
        while True:
            moved = self.space.round_optimum(x + np.random.normal(size=x.shape, scale=1e-2))
            if not np.all(moved == x):
                return moved

    def compute_next_evaluations(self, pending_zipped_X=None, ignored_zipped_X=None):
        """The next suggestion: update the model (with learned hyper-parameters this re-runs the sampler, as the reference does),
        then optimise the acquisition starting from x_baseline = current_argmax."""
        if self.Y is None and self.X is not None:
            self.Y = self.objective.evaluate(self.X)[0]
        self.model.updateModel(self.X, self.Y)
        self.acquisition.optimizer.context_manager = ContextManager(self.space, self.context)
        return _zip(self.space, self.evaluator.compute_batch(duplicate_manager=None, x_baseline=self.current_argmax))

    def _update_model(self):
        self.model.updateModel(_unzip(self.space, self.X), list(self.Y))

    def get_evaluations(self):
        return self.X.copy(), [y.copy() for y in self.Y]

    def save_results(self, filename):
        """Two columns per iteration: the recommended value and the elapsed seconds."""
        np.savetxt(filename, np.column_stack((np.atleast_1d(self.historical_optimal_values), np.atleast_1d(self.historical_time))))
