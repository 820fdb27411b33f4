"""Acquisition plug-ins with the reference's class surface (GPyOpt/acquisitions/base.py:5-74,
maEI.py, maPI.py, EI.py, PI.py, uEI_noiseless.py, uPI.py) whose `_compute_acq` runs on the
MI355X: predict (K* build, N^2 C contraction) + acquisition in one device pass per call.

The host keeps exactly the reference's RNG touchpoints (W_samples drawn with np.random.normal
at construction, theta sampled with np.random.choice) so seeded trajectories line up.
There is no CPU fallback: the model must be a bocf_amd.multi_outputGP.
"""
import warnings

import numpy as np

from . import _ffi
from .utility import COMPILED_IN, device_thetas, inner_expectation


def constant_cost_withGradients(x):
    """GPyOpt/core/task/cost.py:76-80."""
    return np.ones(x.shape[0])[:, None], np.zeros(x.shape)


class AcquisitionBase(object):
    """GPyOpt/acquisitions/base.py:5-74 (fork: acquisition_function returns -acq, cost and
    constraint weighting commented out)."""

    analytical_gradient_prediction = False

    def __init__(self, model, space, optimizer, cost_withGradients=None):
        self.model = model
        self.space = space
        self.optimizer = optimizer
        self.analytical_gradient_acq = self.analytical_gradient_prediction and self.model.analytical_gradient_prediction
        if cost_withGradients is None:
            self.cost_withGradients = constant_cost_withGradients
        else:
            self.cost_withGradients = cost_withGradients

    @staticmethod
    def fromDict(model, space, optimizer, cost_withGradients, config):
        raise NotImplementedError()

    def acquisition_function(self, x):
        f_acqu = self._compute_acq(x)
        return -f_acqu

    def acquisition_function_withGradients(self, x):
        f_acqu, df_acqu = self._compute_acq_withGradients(x)
        return -f_acqu, -df_acqu

    def optimize(self, duplicate_manager=None, x_baseline=None):
        if not self.analytical_gradient_acq:
            out = self.optimizer.optimize(f=self.acquisition_function, duplicate_manager=duplicate_manager, x_baseline=x_baseline)
        else:
            out = self.optimizer.optimize(f=self.acquisition_function, f_df=self.acquisition_function_withGradients,
                                          duplicate_manager=duplicate_manager, x_baseline=x_baseline)
        return out

    def _compute_acq(self, x):
        raise NotImplementedError('')

    def _compute_acq_withGradients(self, x):
        raise NotImplementedError('')

    # -- shared by the subclasses
    _model_entry = "acq_linear"   # the model method that tells a bocf_amd.multi_outputGP from anything else

    def _device_model(self):
        if not hasattr(self.model, self._model_entry):
            raise TypeError("bocf_amd acquisitions need a bocf_amd.multi_outputGP model (no CPU fallback)")
        return self.model

    def _compiled_in_kind(self, who, why):
        """The compiled-in device kind of the utility, for the acquisitions with an entry point of their own: they have no host loop and
        take no utility program, so anything else is NotImplementedError -- `who` needs one because `why`."""
        try:
            kind = self.utility.device_kind(self.model.output_dim)
        except NotImplementedError:
            kind = None
        if kind is None or kind == _ffi.UTIL_PROGRAM:
            raise NotImplementedError("%s needs a utility with a compiled-in device kind (Utility(..., device=...): %s): %s"
                                      % (who, ", ".join(COMPILED_IN), why))
        return kind

    # -- the device-resident refinement (AcquisitionOptimizer(..., refine="device"))
    _device_refine = False        # True on the classes the device loop covers

    def device_refine_objective(self):
        """The objective of acquisition_function_withGradients as keyword arguments of multi_outputGP.refine_acq, or
        NotImplementedError with the reason: an explicit refine="device" never falls back."""
        if not type(self)._device_refine:
            raise NotImplementedError("refine='device' does not cover %s (covered: maEI, maPI, EI, PI, uEI_noiseless); use refine='host'"
                                      % type(self).__name__)
        if not self.use_full_support:
            raise NotImplementedError("refine='device' needs a utility-parameter distribution with full support: without it the host path "
                                      "draws fresh theta from np.random on every gradient call, which a device loop cannot reproduce; "
                                      "use refine='host'")
        if not hasattr(self.model, "refine_acq"):
            raise TypeError("bocf_amd acquisitions need a bocf_amd.multi_outputGP model (no CPU fallback)")
        return self._device_refine_kwargs()

    def _init_composite(self, cost_withGradients):
        """Constructor tail of the composite-utility acquisitions (uEI_noiseless.py:25-38): W_samples, then -- without full
        support -- ten utility parameters, in this order from np.random."""
        if cost_withGradients is not None:
            print('LBC acquisition does now make sense with cost. Cost set to constant.')
        self.cost_withGradients = constant_cost_withGradients
        self.n_attributes = self.model.output_dim
        self.W_samples = np.random.normal(size=(25, self.n_attributes))          # uEI_noiseless.py:31
        self.n_hyps_samples = min(10, self.model.number_of_hyps_samples())
        self.use_full_support = self.utility.parameter_dist.use_full_support
        if self.use_full_support:
            self.utility_params_samples = self.utility.parameter_dist.support
            self.utility_prob_dist = np.atleast_1d(self.utility.parameter_dist.prob_dist)
        else:
            self.utility_params_samples = self.utility.parameter_dist.sample(10)  # uEI_noiseless.py:38
            self.utility_prob_dist = None

    def select_anchors(self, num_anchor=16):
        """Indices (into the last evaluated batch) of the `num_anchor` best candidates, computed on
        the device: np.argsort(acquisition_function(X).flatten())[:num_anchor] of
        anchor_points_generator.py:59-61."""
        return self._device_model().select_topk(num_anchor)[0]


class _ClosedForm(AcquisitionBase):
    """maEI.py:9-163 / maPI.py:9-158: closed-form EI / PI of a linear utility theta.f(x),
    averaged over the utility-parameter distribution."""
    analytical_gradient_prediction = True
    _kind = _ffi.ACQ_EI
    _n_theta_samples = 3          # maEI.py:46; maPI.py:46 draws 10
    _device_refine = True

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None):
        self.optimizer = optimizer
        self.utility = utility
        super(_ClosedForm, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        if cost_withGradients is not None:
            print('LBC acquisition does now make sense with cost. Cost set to constant.')
        self.cost_withGradients = constant_cost_withGradients
        self.use_full_support = self.utility.parameter_dist.use_full_support
        self.n_hyps_samples = min(10, self.model.number_of_hyps_samples())

    def _parameters(self, n_theta_samples):
        """(thetas (L, m), weights (L,) or None): the support and its weights, or n_theta_samples freshly drawn thetas."""
        if self.use_full_support:
            self.utility_params_samples = self.utility.parameter_dist.support
            self.utility_param_dist = np.atleast_1d(self.utility.parameter_dist.prob_dist)
            prob = self.utility_param_dist
        else:
            self.utility_params_samples = self.utility.parameter_dist.sample(n_theta_samples)
            prob = None
        return np.asarray(self.utility_params_samples, dtype=float).reshape(len(self.utility_params_samples), -1), prob

    def _evaluate(self, X, n_theta_samples, entry):
        """(X (n, d), what model.`entry` returns for it) with the parameters of _parameters(n_theta_samples)."""
        thetas, prob = self._parameters(n_theta_samples)
        X = np.atleast_2d(X)
        # the h-loop of maEI.py:85-98 runs on the device (with fixed hyper-parameters its identical passes are one pass)
        return X, getattr(self._device_model(), entry)(X, self._kind, thetas, prob, n_hyps=self.n_hyps_samples)

    def _compute_acq(self, X):
        X, acqX = self._evaluate(X, self._n_theta_samples, "acq_linear")
        return np.reshape(acqX, (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        """maEI.py:57-78 / maPI.py:56-76: value and d/dX; not-full-support draws 3 thetas (both classes)."""
        X, (acqX, dacq_dX) = self._evaluate(X, 3, "acq_linear_grad")
        return np.reshape(acqX, (X.shape[0], 1)), np.reshape(dacq_dX, X.shape)

    def _device_refine_kwargs(self):
        support = self.utility.parameter_dist.support
        thetas = np.asarray(support, dtype=float).reshape(len(support), -1)
        return dict(form=_ffi.REFINE_LINEAR, kind=self._kind, thetas=thetas, prob=np.atleast_1d(self.utility.parameter_dist.prob_dist),
                    n_hyps=self.n_hyps_samples)


class maEI(_ClosedForm):
    _kind = _ffi.ACQ_EI
    _n_theta_samples = 3


class maPI(_ClosedForm):
    _kind = _ffi.ACQ_PI
    _n_theta_samples = 10

    def __init__(self, *a, **kw):
        super(maPI, self).__init__(*a, **kw)
        self.jitter = 1e-6


class EI(maEI):
    """EI.py: single-output specialisation (n_hyps_samples = 1, :35)."""

    def __init__(self, *a, **kw):
        super(EI, self).__init__(*a, **kw)
        self.n_hyps_samples = 1


class PI(maPI):
    """PI.py: single-output specialisation.  Unlike EI.py:35 it keeps n_hyps_samples = min(10, number_of_hyps_samples())
    (PI.py:34): the h-loop averages over the hyper-samples and leaves the model on the last one."""


class _MonteCarlo(AcquisitionBase):
    """uEI_noiseless.py:9-175 / uPI.py:9-125: Monte-Carlo EI / PI of a composite utility
    U(theta, f(x)) with common random numbers W."""
    _kind = _ffi.ACQ_EI

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None):
        self.optimizer = optimizer
        self.utility = utility
        super(_MonteCarlo, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        self._init_composite(cost_withGradients)

    def _compute_acq(self, X, parallel=True):
        """`parallel` is accepted for signature compatibility: the reference's pathos variant
        (uEI_noiseless.py:85-116) computes the same numbers one candidate at a time."""
        X = np.atleast_2d(X)
        model = self._device_model()
        kind = self._device_kind_or_none()
        if kind is None:
            return self._host_utility_acq(X)
        prob = self.utility_prob_dist if self.use_full_support else None
        thetas = device_thetas(kind, self.utility_params_samples)
        acqX = model.acq_mc(X, self._kind, kind, self.utility.device_params, thetas, prob, W=self.W_samples, n_hyps=self.n_hyps_samples,
                            program=self.utility.program_blob if kind == _ffi.UTIL_PROGRAM else None)
        return np.reshape(acqX, (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        """uEI_noiseless.py:118-136: full support -> the support and its weights; otherwise ONE freshly
        sampled theta per call (parameter_dist.sample(1), a global-RNG touchpoint)."""
        if not type(self).analytical_gradient_prediction:
            raise NotImplementedError('')
        X = np.atleast_2d(X)
        if self.use_full_support:
            samples2, prob = self.utility.parameter_dist.support, self.utility_prob_dist
        else:
            samples2, prob = self.utility.parameter_dist.sample(1), None
        kind = self._device_kind_or_none()
        if kind is None:
            return self._host_utility_acq_with_gradients(X, samples2, prob)
        acqX, dacq_dX = self._device_model().acq_mc_grad(X, kind, self.utility.device_params, device_thetas(kind, samples2), prob,
                                                         W=self.W_samples, n_hyps=self.n_hyps_samples,
                                                         program=self.utility.program_blob if kind == _ffi.UTIL_PROGRAM else None)
        return np.reshape(acqX, (X.shape[0], 1)), np.reshape(dacq_dX, X.shape)

    # ---- utilities outside the device's closed set (utility.py:37-41 accepts ANY callable): the posterior still comes from
    # the device (K*, the N^2 C contraction, gradients -- all the O(N^2) work), only U itself is evaluated on the host with the
    # user's func / dfunc ("closed enum + host fallback for anything else"); nothing here is test infrastructure.
    def _device_kind_or_none(self):
        try:
            return self.utility.device_kind(self.model.output_dim)
        except NotImplementedError:
            if not getattr(self, "_warned_host_utility", False):
                warnings.warn("bocf_amd: the utility is a Python callable outside the device's closed set (%s): the posterior "
                              "(mean, variance, gradients) is computed on the GPU, the Monte-Carlo loop over U runs on the HOST -- "
                              "orders of magnitude slower than a device utility (Utility(..., device=...); device='program' traces this "
                              "callable and runs it on the GPU)"
                              % ", ".join(sorted(COMPILED_IN)), RuntimeWarning,
                              stacklevel=3)
                self._warned_host_utility = True
            return None

    def _eval_user_utility(self, f, theta, y):
        """f(theta, y) for y (m, n): one vectorised call when the callable broadcasts over candidates the way the reference
        itself uses it on the (m, N) evaluated points (uEI_noiseless.py:76), else candidate by candidate.  Returns (n,) -- or
        (m, n) for a gradient."""
        n = y.shape[1]
        if getattr(self, "_user_vectorised", None) is not False:
            try:
                out = np.asarray(f(theta, y), dtype=float)
                if out.shape in ((n,), (1, n), (y.shape[0], n)):
                    if getattr(self, "_user_vectorised", None) is None:        # check the broadcast once against single columns
                        k = min(n, 3)
                        one = np.stack([np.asarray(f(theta, y[:, i]), dtype=float).reshape(-1) for i in range(k)], -1)
                        ok = np.allclose(one.reshape(-1, k), out.reshape(-1, n)[:, :k], rtol=1e-12, atol=1e-300)
                        self._user_vectorised = bool(ok)
                    if self._user_vectorised:
                        return out.reshape(-1, n) if out.ndim == 2 and out.shape[0] == y.shape[0] and out.shape[0] > 1 else out.reshape(n)
            except Exception:
                self._user_vectorised = False
        cols = [np.asarray(f(theta, y[:, i]), dtype=float).reshape(-1) for i in range(n)]
        out = np.stack(cols, -1)
        return out[0] if out.shape[0] == 1 else out

    def _host_utility_acq(self, X):
        """uEI_noiseless.py:63-83 / uPI.py:66-86 with the user's callable: best-so-far from the hyper-sample current on entry
        (:66), then per hyper-sample the device posterior and the host Monte-Carlo sum."""
        model = self._device_model()
        thetas = list(self.utility_params_samples)
        prob = self.utility_prob_dist if self.use_full_support else None
        n, L = X.shape[0], len(thetas)
        marg = np.zeros((n, L))
        f_eval = model.posterior_mean_at_evaluated_points()
        best = [float(np.max(self._eval_user_utility(self.utility.eval_func, th, f_eval))) for th in thetas]
        pi = self._kind == _ffi.ACQ_PI
        W = np.asarray(self.W_samples, dtype=float)
        for h in range(self.n_hyps_samples):
            model.set_hyperparameters(h)
            mu = model.posterior_mean(X)
            sigma = np.sqrt(model.posterior_variance(X))
            for l, th in enumerate(thetas):
                for w in W:
                    val = self._eval_user_utility(self.utility.eval_func, th, mu + sigma * w[:, None])
                    if pi:
                        marg[:, l] += (val - (best[l] + 1e-6)) > 0.0          # uPI.py:83
                    else:
                        marg[:, l] += np.maximum(val - best[l], 0.0)          # uEI_noiseless.py:80
        marg /= (self.n_hyps_samples * W.shape[0])
        acq = marg.dot(np.atleast_1d(prob)) if prob is not None else marg.sum(1) / L
        return acq.reshape(n, 1)

    def _host_utility_acq_with_gradients(self, X, thetas, prob):
        """uEI_noiseless.py:138-170 with the user's func and dfunc (device posterior + gradients, host Monte-Carlo loop)."""
        if self.utility.dfunc is None:
            raise TypeError("the utility has no dfunc: the gradient of the acquisition cannot be computed (utility.py:44-48)")
        model = self._device_model()
        thetas = list(thetas)
        n, d, L = X.shape[0], X.shape[1], len(thetas)
        marg, dmarg = np.zeros((n, L)), np.zeros((n, d, L))
        f_eval = model.posterior_mean_at_evaluated_points()
        best = [float(np.max(self._eval_user_utility(self.utility.eval_func, th, f_eval))) for th in thetas]
        W = np.asarray(self.W_samples, dtype=float)
        for h in range(self.n_hyps_samples):
            model.set_hyperparameters(h)
            mu = model.posterior_mean(X)
            sigma = np.sqrt(model.posterior_variance(X))
            dmu = model.posterior_mean_gradient(X)                            # (m, n, d)
            dvar = model.posterior_variance_gradient(X)
            for l, th in enumerate(thetas):
                for w in W:
                    a = mu + sigma * w[:, None]
                    val = self._eval_user_utility(self.utility.eval_func, th, a)
                    marg[:, l] += np.maximum(val - best[l], 0.0)
                    imp = val > best[l]
                    if imp.any():
                        g = np.asarray(self._eval_user_utility(self.utility.eval_gradient, th, a[:, imp]), dtype=float).reshape(mu.shape[0], -1)
                        b = dmu[:, imp, :] + (0.5 * w[:, None] / sigma[:, imp])[:, :, None] * dvar[:, imp, :]
                        dmarg[imp, :, l] += np.einsum("ji,jiq->iq", g, b)
        marg /= (self.n_hyps_samples * W.shape[0])
        dmarg /= (self.n_hyps_samples * W.shape[0])
        if prob is not None:
            acq, dacq = marg.dot(np.atleast_1d(prob)), np.tensordot(dmarg, np.atleast_1d(prob), 1)
        else:
            acq, dacq = marg.sum(1) / L, dmarg.sum(2) / L
        return acq.reshape(n, 1), dacq.reshape(n, d)

    def update_Z_samples(self, n_samples):
        """uEI_noiseless.py:172-175.  `n_samples` is REQUIRED as in the reference: cbo.py:299-302 calls
        update_Z_samples() without it inside a try/except, so in a cbo run the TypeError is swallowed, W_samples is
        never redrawn and np.random is not consumed -- a seeded cbo-style trajectory relies on exactly that."""
        print('Update utility parameter W and Z samples')
        self.W_samples = np.random.normal(size=self.W_samples.shape)


class uEI_noiseless(_MonteCarlo):
    analytical_gradient_prediction = True
    _kind = _ffi.ACQ_EI
    _device_refine = True

    def _device_refine_kwargs(self):
        try:
            kind = self.utility.device_kind(self.model.output_dim)
        except NotImplementedError:
            raise NotImplementedError("refine='device' needs a device utility (Utility(..., device=...), device='program' included): this "
                                      "utility is a host callable, whose Monte-Carlo loop runs on the host; use refine='host'")
        return dict(form=_ffi.REFINE_MC, util_kind=kind, util_params=self.utility.device_params,
                    thetas=device_thetas(kind, self.utility.parameter_dist.support), prob=self.utility_prob_dist, W=self.W_samples,
                    n_hyps=self.n_hyps_samples, program=self.utility.program_blob if kind == _ffi.UTIL_PROGRAM else None)


class uEI_pending(uEI_noiseless):
    """uEI_noiseless conditioned on the pending points of a batch under construction: with P = (p_1 .. p_r), r <= 15, set,

        alpha(x | P) = sum_l p_l (1/S) sum_s max( U(theta_l, y_s(x)) - max(best_l, max_i U(theta_l, F_s(p_i))), 0 ),

    where (F_s, y_s(x)) is a joint posterior sample at (P, x): F_s from the normals Z (S, m, r) of set_pending_points, y_s(x) correlated
    with it through Sigma(P, x) and closed with W_samples[s] -- so alpha(x | P) = qEI(P u {x}) - qEI(P) for these normals, the increment a
    greedy batch maximises (CompositeGreedyBatch).  Everything runs on the device (bocf_acq_pending).  Unlike the parent it uses the latent,
    noiseless variance.  With no pending points (None or an empty P) the class IS its parent: the same calls, the same numbers.

    Parameter conventions are the parent's: _compute_acq uses utility_params_samples (the support with its weights, or the ten parameters
    drawn at construction), _compute_acq_withGradients the support or ONE freshly drawn parameter per call.  The pending points are staged
    again whenever the model's fit serial changes.  A utility without a compiled-in device kind raises NotImplementedError."""
    _model_entry = "acq_pending"
    _device_refine = False        # (its objective has an entry point of its own: outside the device-resident refinement)

    def __init__(self, *a, **kw):
        super(uEI_pending, self).__init__(*a, **kw)
        self.pending_points = None
        self.pending_Z = None
        self._staged_serial = None

    def set_pending_points(self, P, Z=None):
        """P (r, d), 1 <= r <= 15, and the joint normals Z (S, m, r), S = len(W_samples); Z = None draws np.random.normal(size=(S, m, r)).
        P = None or an empty P clears the pending set: the parent's behaviour, exactly."""
        if P is None or np.size(P) == 0:
            self.pending_points = self.pending_Z = self._staged_serial = None
            return
        P = np.array(np.atleast_2d(P), dtype=float)
        if not 1 <= P.shape[0] <= 15:
            raise ValueError("1 .. 15 pending points")
        S, m = self.W_samples.shape
        Z = np.random.normal(size=(S, m, P.shape[0])) if Z is None else np.array(Z, dtype=float)
        if Z.shape != (S, m, P.shape[0]):
            raise ValueError("Z must be (len(W_samples), output_dim, r) = %r" % ((S, m, P.shape[0]),))
        self.pending_points, self.pending_Z, self._staged_serial = P, Z, None

    def _pending_kind(self):
        return self._compiled_in_kind("uEI_pending", "the conditioning on pending points runs on the device, there is no host loop and no utility program")

    def _stage(self):
        model = self._device_model()
        model._ensure_fitted()
        self._staged_serial = model._fit_serial
        model.set_pending_points(self.pending_points, self.pending_Z, W=self.W_samples)     # (free when this set is the resident one)

    def _compute_acq(self, X, parallel=True):
        if self.pending_points is None:
            return super(uEI_pending, self)._compute_acq(X, parallel)
        X = np.atleast_2d(X)
        kind = self._pending_kind()
        self._stage()
        prob = self.utility_prob_dist if self.use_full_support else None
        acqX = self._device_model().acq_pending(X, kind, self.utility.device_params, device_thetas(kind, self.utility_params_samples), prob,
                                                W=self.W_samples, n_hyps=self.n_hyps_samples)
        return np.reshape(acqX, (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        if self.pending_points is None:
            return super(uEI_pending, self)._compute_acq_withGradients(X)
        X = np.atleast_2d(X)
        if self.use_full_support:
            samples2, prob = self.utility.parameter_dist.support, self.utility_prob_dist
        else:
            samples2, prob = self.utility.parameter_dist.sample(1), None
        kind = self._pending_kind()
        self._stage()
        acqX, dacq_dX = self._device_model().acq_pending(X, kind, self.utility.device_params, device_thetas(kind, samples2), prob,
                                                         W=self.W_samples, n_hyps=self.n_hyps_samples, grad=True)
        return np.reshape(acqX, (X.shape[0], 1)), np.reshape(dacq_dX, X.shape)


class uEI_joint(AcquisitionBase):
    """Joint Monte-Carlo expected improvement of the composite utility at a whole batch of q points (q-uEI), 1 <= q <= 8: a row of X is a
    batch, its q points side by side (length q * d), and

        alpha(X) = sum_l p_l (1/S) sum_s max( max_k U(theta_l, y_s(x_k)) - best_l, 0 ),

    y_s a joint posterior sample at the q points made from Z_samples[s] (S, m, q) through the Cholesky factor of the latent, noiseless
    covariance -- the quantity CompositeGreedyBatch maximises one point at a time and the Thompson evaluators approximate.  Value and
    gradient run on the device (bocf_acq_joint; the gradient follows the envelope rule with Z, theta and the incumbent fixed), so two
    batches are compared under common random numbers and all q points can be improved together (CompositeJointBatch).  best_l is the
    best-so-far of uEI_noiseless.

    Random numbers, all in the constructor and in this order: W_samples (25, m) and -- without full support -- ten utility parameters, as
    every composite acquisition draws them, then Z_samples = np.random.normal(size=(n_samples, m, q)).  update_Z_samples(n) redraws
    Z_samples alone.  Parameter conventions are uEI_noiseless's: _compute_acq uses utility_params_samples, _compute_acq_withGradients the
    support or ONE freshly drawn parameter per call.  The gradient form holds 128 points on the device: more batches than 128 // q are
    worked off in groups.  Only compiled-in device utilities are accepted: anything else raises NotImplementedError."""
    analytical_gradient_prediction = True
    _model_entry = "acq_joint"
    _device_refine = False        # (its objective has an entry point of its own: outside the device-resident refinement)

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None, q=2, n_samples=64):
        if not 1 <= int(q) <= 8:
            raise ValueError("q must be in 1 .. 8")
        if not 1 <= int(n_samples) <= 256:
            raise ValueError("n_samples must be in 1 .. 256")
        self.optimizer = optimizer
        self.utility = utility
        self.q = int(q)
        super(uEI_joint, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        self._init_composite(cost_withGradients)
        self.Z_samples = np.random.normal(size=(int(n_samples), self.model.output_dim, self.q))

    def update_Z_samples(self, n_samples):
        n_samples = int(n_samples)
        if not 1 <= n_samples <= 256:
            raise ValueError("n_samples must be in 1 .. 256")
        self.Z_samples = np.random.normal(size=(n_samples, self.model.output_dim, self.q))

    def _joint_kind(self):
        return self._compiled_in_kind("uEI_joint", "the joint samples and their maximum over the batch run on the device, there is no host loop and no utility program")

    def _batches(self, X):
        X = np.atleast_2d(np.asarray(X, dtype=float))
        if X.shape[1] % self.q:
            raise ValueError("a row holds q = %d points side by side: its length must be a multiple of q" % self.q)
        return X

    def _compute_acq(self, X):
        X = self._batches(X)
        kind = self._joint_kind()
        prob = self.utility_prob_dist if self.use_full_support else None
        acqX = self._device_model().acq_joint(X, self.q, kind, self.utility.device_params, device_thetas(kind, self.utility_params_samples), prob,
                                              self.Z_samples, n_hyps=self.n_hyps_samples)
        return np.reshape(acqX, (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        X = self._batches(X)
        if self.use_full_support:
            samples2, prob = self.utility.parameter_dist.support, self.utility_prob_dist
        else:
            samples2, prob = self.utility.parameter_dist.sample(1), None
        kind = self._joint_kind()
        thetas = device_thetas(kind, samples2)
        model, step = self._device_model(), max(1, 128 // self.q)
        acqX, dacq = np.empty((X.shape[0], 1)), np.empty(X.shape)
        entry_h = getattr(model, "_current_h", None)          # a call leaves the model on the last hyper-sample: every group starts from the same one
        for i in range(0, X.shape[0], step):
            if i and entry_h is not None:
                model.set_hyperparameters(entry_h)
            a, g = model.acq_joint(X[i:i + step], self.q, kind, self.utility.device_params, thetas, prob, self.Z_samples, n_hyps=self.n_hyps_samples,
                                   grad=True)
            acqX[i:i + step, 0] = a
            dacq[i:i + step] = np.reshape(g, (len(a), -1))
        return acqX, dacq


class uEI_constrained(uEI_noiseless):
    """uEI_noiseless under linear constraints on the outputs (constraints.OutputConstraints):

        alpha(x) = sum_l p_l (1/S) sum_s I_ls(x) phi(y_s(x)),   phi(y) = prod_k s(-(A y - b)_k / eta_k),

    s the logistic function, y_s(x) = mu(x) + sigma(x) o W_s the parent's samples, I_ls the improvement over the best FEASIBLE training
    point (hard test on the posterior mean), or 1 when no training point is feasible -- the acquisition is then the smoothed probability
    of feasibility.  The constraints read the same outputs as the utility, so they are applied sample by sample on the device
    (bocf_acq_mc_constrained); value and gradient are those of the same smooth function.

    Parameter conventions and np.random touchpoints are the parent's.  There is no host fallback: a utility without a compiled-in device
    kind raises NotImplementedError."""
    _model_entry = "acq_mc_constrained"
    _device_refine = False        # (its objective has an entry point of its own: outside the device-resident refinement)

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None, constraints=None):
        super(uEI_constrained, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients, utility=utility)
        if constraints is None or not hasattr(constraints, "feasible"):
            raise TypeError("uEI_constrained needs constraints=OutputConstraints(A, b, eta)")
        if constraints.m != self.model.output_dim:
            raise ValueError("the constraints are on %d outputs, the model has %d" % (constraints.m, self.model.output_dim))
        self.constraints = constraints

    def _constrained_kind(self):
        return self._compiled_in_kind("uEI_constrained", "the constraints are applied inside the device's Monte-Carlo sum, there is no host loop and no utility program")

    def _evaluate(self, X, samples, prob, grad):
        kind = self._constrained_kind()
        model = self._device_model()
        model.set_output_constraints(self.constraints)       # (free when this set is the resident one)
        return model.acq_mc_constrained(X, kind, self.utility.device_params, device_thetas(kind, samples), prob, W=self.W_samples,
                                        n_hyps=self.n_hyps_samples, grad=grad)

    def _compute_acq(self, X, parallel=True):
        X = np.atleast_2d(X)
        prob = self.utility_prob_dist if self.use_full_support else None
        return np.reshape(self._evaluate(X, self.utility_params_samples, prob, False), (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        X = np.atleast_2d(X)
        if self.use_full_support:
            samples2, prob = self.utility.parameter_dist.support, self.utility_prob_dist
        else:
            samples2, prob = self.utility.parameter_dist.sample(1), None
        acqX, dacq_dX = self._evaluate(X, samples2, prob, True)
        return np.reshape(acqX, (X.shape[0], 1)), np.reshape(dacq_dX, X.shape)


def risk_rank(level, n_samples):
    """The integer rank the device takes for a level in [0, 1] and S samples: min(S - 1, floor(level * S)), computed here, once, in double
    precision (the C ABI takes only the integer, so no floating floor is computed twice)."""
    level, S = float(level), int(n_samples)
    if not 0.0 <= level <= 1.0:
        raise ValueError("level must be in [0, 1]")
    if S < 1:
        raise ValueError("no samples")
    return min(S - 1, int(np.floor(level * S)))


class _Risk(_MonteCarlo):
    """Order statistics of the Monte-Carlo samples of the composite utility: with u_s = U(theta_l, mu(x) + sigma(x) o W_s),
    the parent's samples, in ascending order (ties by sample index, a NaN as -inf) and k = risk_rank(level, S),

        alpha(x) = sum_l p_l rho_l(x),   rho = u_(k) (uUCB) | mean of u_(0) .. u_(k) (uCVaR, lower) | mean of u_(k) .. u_(S-1) (uCVaR, upper),

    averaged over the hyper-samples, on the device (bocf_acq_risk); the gradient is pathwise over the selected samples.  There is no
    incumbent, so the acquisition is informative where uEI is flat (early in a run, or with no feasible training point).

    Parameter conventions and np.random touchpoints are uEI_noiseless's: _compute_acq uses utility_params_samples (the support with its
    weights, or the ten parameters drawn at construction), _compute_acq_withGradients the support or ONE freshly drawn parameter per call.
    There is no host fallback and no utility program: a utility without a compiled-in device kind raises NotImplementedError."""
    analytical_gradient_prediction = True
    _model_entry = "acq_risk"
    _device_refine = False        # (its objective has an entry point of its own: outside the device-resident refinement)
    _risk_kind = _ffi.RISK_QUANTILE

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None, level=0.9):
        super(_Risk, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients, utility=utility)
        risk_rank(level, len(self.W_samples))               # (validates the level)
        self.level = float(level)

    @property
    def rank(self):
        """k for the current W_samples."""
        return risk_rank(self.level, len(self.W_samples))

    def _risk_device_kind(self):
        return self._compiled_in_kind(type(self).__name__, "the samples are ranked on the device, there is no host loop and no utility program")

    def _evaluate(self, X, samples, prob, grad):
        kind = self._risk_device_kind()
        if len(self.W_samples) > _ffi.RISK_MAX_SAMPLES:
            raise ValueError("at most %d Monte-Carlo samples (W_samples)" % _ffi.RISK_MAX_SAMPLES)
        return self._device_model().acq_risk(X, self._risk_kind, self.rank, kind, self.utility.device_params, device_thetas(kind, samples), prob,
                                             W=self.W_samples, n_hyps=self.n_hyps_samples, grad=grad)

    def _compute_acq(self, X, parallel=True):
        X = np.atleast_2d(X)
        prob = self.utility_prob_dist if self.use_full_support else None
        return np.reshape(self._evaluate(X, self.utility_params_samples, prob, False), (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        X = np.atleast_2d(X)
        if self.use_full_support:
            samples2, prob = self.utility.parameter_dist.support, self.utility_prob_dist
        else:
            samples2, prob = self.utility.parameter_dist.sample(1), None
        acqX, dacq_dX = self._evaluate(X, samples2, prob, True)
        return np.reshape(acqX, (X.shape[0], 1)), np.reshape(dacq_dX, X.shape)


class uUCB(_Risk):
    """Upper confidence bound of the composite utility: the `level` quantile of its Monte-Carlo samples, u_(k) with
    k = min(S - 1, floor(level * S)) -- an exact order statistic, no interpolation.  See _Risk."""
    _risk_kind = _ffi.RISK_QUANTILE


class uCVaR(_Risk):
    """Tail mean of the composite utility's Monte-Carlo samples with k = min(S - 1, floor(level * S)): tail="lower" is the mean of the
    k + 1 worst samples u_(0) .. u_(k) (the conditional value at risk at `level`: a point that is good even when things go badly),
    tail="upper" the mean of the S - k best, u_(k) .. u_(S-1).  See _Risk."""

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None, level=0.1, tail="lower"):
        if tail not in ("lower", "upper"):
            raise ValueError("tail must be 'lower' or 'upper'")
        super(uCVaR, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients, utility=utility, level=level)
        self.tail = tail
        self._risk_kind = _ffi.RISK_LOWER_TAIL if tail == "lower" else _ffi.RISK_UPPER_TAIL


class maUCB(_ClosedForm):
    """Confidence bound of a linear utility theta . f(x) in closed form (GP-UCB; GPyOpt's AcquisitionLCB with the sign of a maximiser):

        alpha(x) = sum_l p_l [ theta_l . mu(x) + exploration_weight * sqrt(sum_j theta_lj^2 var_j(x)) ],

    averaged over the hyper-samples, value and gradient on the device (bocf_acq_linear_ucb).  Needs a linear utility.  The utility
    parameters are maEI's: the support with its weights, or three freshly drawn ones per call."""
    _model_entry = "acq_linear_ucb"
    _device_refine = False        # (its objective has an entry point of its own: outside the device-resident refinement)

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None, exploration_weight=2):
        super(maUCB, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients, utility=utility)
        if not np.isfinite(exploration_weight):
            raise ValueError("exploration_weight must be finite")
        self.exploration_weight = float(exploration_weight)

    def _ucb(self, X, grad):
        if not getattr(self.utility, "linear", False) and getattr(self.utility, "device", None) != "linear":
            raise NotImplementedError("%s is the closed form of a LINEAR utility (Utility(..., linear=True) or Utility(..., device='linear')); "
                                      "for any other compiled-in utility use uUCB" % type(self).__name__)
        thetas, prob = self._parameters(3)
        X = np.atleast_2d(X)
        return X, self._device_model().acq_linear_ucb(X, self.exploration_weight, thetas, prob, n_hyps=self.n_hyps_samples, grad=grad)

    def _compute_acq(self, X):
        X, acqX = self._ucb(X, False)
        return np.reshape(acqX, (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        X, (acqX, dacq_dX) = self._ucb(X, True)
        return np.reshape(acqX, (X.shape[0], 1)), np.reshape(dacq_dX, X.shape)


class UCB(maUCB):
    """Single-output specialisation of maUCB (n_hyps_samples = 1, as EI)."""

    def __init__(self, *a, **kw):
        super(UCB, self).__init__(*a, **kw)
        self.n_hyps_samples = 1


class maLogEI(_ClosedForm):
    """log of maEI in closed form (Ament et al. 2023): with z = (theta_l . mu - best_l) / sigma_l,

        log alpha(x) = LSE over hyper-samples h and parameters l of [ log p_l - log H + log sigma_l + log h(z) ],   h(z) = phi(z) + z Phi(z),

    value and gradient on the device (bocf_acq_log_linear), log h accurate for every finite z.  It has maEI's maximisers, but where the
    incumbent is hard to beat -- maEI and its gradient are then exactly zero -- it stays finite with a useful gradient, so the anchor
    selection and the refinement do not work on a plateau.  Constructor, utility parameters and np.random touchpoints are maEI's: the
    support with its weights, or three freshly drawn parameters per call."""
    _model_entry = "acq_log_linear"
    _device_refine = False        # (its objective has an entry point of its own: outside the device-resident refinement)
    _n_theta_samples = 3

    def _log_ei(self, X, grad):
        thetas, prob = self._parameters(3 if grad else self._n_theta_samples)
        X = np.atleast_2d(X)
        return X, self._device_model().acq_log_linear(X, thetas, prob, n_hyps=self.n_hyps_samples, grad=grad)

    def _compute_acq(self, X):
        X, acqX = self._log_ei(X, False)
        return np.reshape(acqX, (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        X, (acqX, dacq_dX) = self._log_ei(X, True)
        return np.reshape(acqX, (X.shape[0], 1)), np.reshape(dacq_dX, X.shape)


class LogEI(maLogEI):
    """Single-output specialisation of maLogEI (n_hyps_samples = 1, as EI)."""

    def __init__(self, *a, **kw):
        super(LogEI, self).__init__(*a, **kw)
        self.n_hyps_samples = 1


class uLogEI(_MonteCarlo):
    """log of a smooth surrogate of uEI_noiseless (Ament et al. 2023): with the parent's samples
    y_s = mu(x) + sigma(x) o W_s and t = (U(theta_l, y_s) - best_l) / tau,

        log alpha_tau(x) = LSE over hyper-samples h, parameters l and samples s of [ log p_l - log(H S) + log tau + log psi(t) ],
        psi(t) = softplus(t) + 0.1 / (1 + t^2),

    value and pathwise gradient on the device (bocf_acq_log_mc).  psi replaces the hinge max(t, 0) by a monotone function with a fat tail,
    so a candidate none of whose samples improves still has a finite value and a non-zero gradient.  `tau` is in the UNITS OF THE UTILITY:
    0 < exp(log alpha_tau) - uEI <= tau (ln 2 + 0.1), so choose it small against the improvements that matter (the default 1e-6 suits
    utilities of order one).  Constructor draws, parameter conventions and np.random touchpoints are uEI_noiseless's.  Compiled-in utilities
    and utility programs (Utility(..., device="program")); there is no host fallback: a host callable raises NotImplementedError."""
    analytical_gradient_prediction = True
    _model_entry = "acq_log_mc"
    _device_refine = False        # (its objective has an entry point of its own: outside the device-resident refinement)

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None, tau=1e-6):
        super(uLogEI, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients, utility=utility)
        if not (np.isfinite(tau) and tau > 0):
            raise ValueError("tau must be finite and > 0 (it is in the units of the utility)")
        self.tau = float(tau)

    def _evaluate(self, X, samples, prob, grad):
        try:
            kind = self.utility.device_kind(self.model.output_dim)
        except NotImplementedError:
            raise NotImplementedError("uLogEI needs a device utility (Utility(..., device=...): %s, or device='program' to trace a callable): the "
                                      "log-sum-exp over the samples runs on the device, there is no host loop" % ", ".join(COMPILED_IN))
        return self._device_model().acq_log_mc(X, kind, self.utility.device_params, device_thetas(kind, samples), prob, self.tau, W=self.W_samples,
                                               n_hyps=self.n_hyps_samples, grad=grad,
                                               program=self.utility.program_blob if kind == _ffi.UTIL_PROGRAM else None)

    def _compute_acq(self, X, parallel=True):
        X = np.atleast_2d(X)
        prob = self.utility_prob_dist if self.use_full_support else None
        return np.reshape(self._evaluate(X, self.utility_params_samples, prob, False), (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        X = np.atleast_2d(X)
        if self.use_full_support:
            samples2, prob = self.utility.parameter_dist.support, self.utility_prob_dist
        else:
            samples2, prob = self.utility.parameter_dist.sample(1), None
        acqX, dacq_dX = self._evaluate(X, samples2, prob, True)
        return np.reshape(acqX, (X.shape[0], 1)), np.reshape(dacq_dX, X.shape)


class uPI(_MonteCarlo):
    analytical_gradient_prediction = False
    _kind = _ffi.ACQ_PI

    def __init__(self, *a, **kw):
        super(uPI, self).__init__(*a, **kw)
        self.jitter = 1e-6


class uKG(AcquisitionBase):
    """Discrete composite knowledge gradient: the one-step look-ahead value of x against a set A of reference points,

        KG(x) = sum_l p_l [ (1/Sf) sum_s max_a v(a; x, z_s, theta_l)  -  max_a v0(a; theta_l) ],

    v the posterior expected utility at a after a fantasy observation at x with normals z_s, v0 the current one (the reference's
    experiment scripts import such acquisitions, test_1a.py:7-8: uKG_SGA / uKG_cf, over the look-ahead helpers of its
    multi_outputGP, multi_outputGP.py:203-281,309-330).  Everything runs on the device (bocf_acq_kg); the gradient follows the
    envelope rule.  With a finite number of fantasies KG can be slightly negative; it is not clamped.

    Random numbers, all in the constructor and in this order: Z_samples (n_fantasies, m) and W_samples (25, m) with
    np.random.normal, then -- without full support -- ten utility parameters (parameter_dist.sample(10)).  The reference points
    are those of set_reference_points(A); if none are set they are drawn once per model update, at the first evaluation after it:
    n_ref_points - 1 uniform points in the space's bounds (one np.random.uniform per input dimension) plus the training input with
    the best current expected utility.  They are staged again whenever the model's fit serial changes.

    The inner expectation follows the recommendation step (recommend.py): the posterior mean for a linear utility, the closed form
    when the utility's device kind has one, Monte-Carlo over W_samples otherwise.  A utility without a device kind raises
    NotImplementedError."""
    analytical_gradient_prediction = True
    _model_entry = "acq_kg"

    def __init__(self, model, space, optimizer=None, cost_withGradients=None, utility=None, n_fantasies=16, n_ref_points=64):
        self.optimizer = optimizer
        self.utility = utility
        super(uKG, self).__init__(model, space, optimizer, cost_withGradients=cost_withGradients)
        if not 1 <= int(n_fantasies) <= 256:
            raise ValueError("n_fantasies must be in 1 .. 256")
        if not 1 <= int(n_ref_points) <= 1024:
            raise ValueError("n_ref_points must be in 1 .. 1024")
        self.n_fantasies, self.n_ref_points = int(n_fantasies), int(n_ref_points)
        self.Z_samples = np.random.normal(size=(self.n_fantasies, self.model.output_dim))
        self._init_composite(cost_withGradients)
        self.reference_points = None          # the set in use
        self._user_reference_points = None
        self._staged_serial = None

    # ---- what the device evaluates
    def _mode_and_kind(self):
        """(mode, device utility kind) as the recommendation step chooses its form (utility.inner_expectation)."""
        try:
            mode, kind = inner_expectation(self.utility, self.model.output_dim)
        except NotImplementedError:
            raise NotImplementedError("uKG needs a utility with a device kind (Utility(..., device=...): %s): the look-ahead runs on the "
                                      "device, there is no host loop for a Python callable" % ", ".join(COMPILED_IN))
        if kind == _ffi.UTIL_PROGRAM:
            raise NotImplementedError("uKG does not take a utility program (Utility(..., device='program')): the knowledge gradient runs the "
                                      "compiled-in utilities only (%s)" % ", ".join(COMPILED_IN))
        return mode, kind

    # ---- reference points
    def set_reference_points(self, A):
        """Use A (na, d), 1 <= na <= 1024, as the discretisation from now on (None: back to drawn sets)."""
        self._user_reference_points = None if A is None else np.array(np.atleast_2d(A), dtype=float)
        self._staged_serial = None

    def _draw_reference_points(self, mode, kind):
        from .acquisition_optimizer import _bounds_of, samples_multidimensional_uniform
        model = self._device_model()
        pts = []
        if self.n_ref_points > 1:
            pts.append(np.atleast_2d(samples_multidimensional_uniform(_bounds_of(self.space), self.n_ref_points - 1)))
        # the training input with the best current expected utility  sum_l p_l E[U(theta_l, f(x))]
        Xt = np.atleast_2d(model.get_evaluated_points())
        thetas = device_thetas(kind, self.utility_params_samples)
        L, n = thetas.shape[0], Xt.shape[0]
        Z = np.broadcast_to(self.W_samples, (L,) + self.W_samples.shape) if mode == _ffi.EU_MC else None
        v = model.expected_utility(np.tile(Xt, (L, 1)), mode, kind, thetas, np.repeat(np.arange(L), n), Z=Z, n_hyps=self.n_hyps_samples,
                                   util_params=self.utility.device_params)
        p = self.utility_prob_dist if self.utility_prob_dist is not None else np.full(L, 1.0 / L)
        pts.append(Xt[int(np.argmax(np.asarray(p).dot(np.asarray(v).reshape(L, n))))][None, :])
        return np.concatenate(pts)

    def _stage(self, mode, kind):
        model = self._device_model()
        model._ensure_fitted()
        serial = model._fit_serial
        if self._staged_serial != serial:
            self.reference_points = self._user_reference_points if self._user_reference_points is not None else self._draw_reference_points(mode, kind)
            self._staged_serial = serial
        model.set_reference_points(self.reference_points)     # (free when this set is the resident one)

    def _evaluate(self, X, grad):
        X = np.atleast_2d(X)
        mode, kind = self._mode_and_kind()
        self._stage(mode, kind)
        prob = self.utility_prob_dist if self.use_full_support else None
        thetas = device_thetas(kind, self.utility_params_samples)
        out = self._device_model().acq_kg(X, mode, kind, self.utility.device_params, thetas, prob, self.Z_samples,
                                         W=self.W_samples if mode == _ffi.EU_MC else None, n_hyps=self.n_hyps_samples, grad=grad)
        return X, out

    def _compute_acq(self, X):
        X, acq = self._evaluate(X, False)
        return np.reshape(acq, (X.shape[0], 1))

    def _compute_acq_withGradients(self, X):
        X, (acq, dacq) = self._evaluate(X, True)
        return np.reshape(acq, (X.shape[0], 1)), np.reshape(dacq, X.shape)
