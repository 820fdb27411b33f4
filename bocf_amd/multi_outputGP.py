"""MI355X-backed drop-in for the reference's `multi_outputGP` (multi_outputGP.py:9-349), both with fixed
hyper-parameters (GPModelFixedHyps, GPyOpt/models/gpmodel_fixed_hyps.py:9-120) and with learned ones (GPModel,
GPyOpt/models/gpmodel.py:9-230: optimise + HMC per update, n_samples hyper-samples resident on the device).

Same constructor, attributes and method set; every number is produced by libbocf_hip.so
(no CPU fallback).  The m independent GPs are fitted and evaluated together on the device:
results are stacked as (m, n) float64 arrays exactly like the reference.
"""
import ctypes

import numpy as np

from . import _ffi
from .hyper import OutputHyper
from .kern import SE, kernel_spec
from .utility import device_utility


class _Resident(object):
    """THE record of what the host believes is resident on the device -- a new resident buffer is a field here, and the events that
    invalidate it name it in their forget() call; nowhere else.  None = unknown / not resident.
    candidates: their count; W, Z, reference, pending: key of the uploaded set_mc_samples / set_eu_samples / set_reference_points /
    set_pending_points arrays; paths: the record of draw_paths (fit serial, device group and device order of every path); program: the utility program blob; query, gradient: (key, arrays) of the last all-hyper-sample posterior query, served per h as
    slices; constraints: key of the set_output_constraints set (it does not depend on the fit: no model change forgets it, only pickling
    -- a new context -- does)."""
    __slots__ = ("candidates", "W", "Z", "program", "reference", "pending", "paths", "query", "gradient", "constraints")

    def __init__(self):
        self.forget()

    def forget(self, *names):
        """Forget the named fields, or everything."""
        for name in names or self.__slots__:
            setattr(self, name, None)


class _GPView(object):
    """What `output[j].model` exposes in the reference (GPRegression): the data."""

    def __init__(self, parent, j):
        self._p, self._j = parent, j

    @property
    def X(self):
        return self._p._X

    @property
    def Y(self):
        return self._p._Y[self._j]


class _OutputView(object):
    """Per-output facade with the GPModelFixedHyps method set (gpmodel_fixed_hyps.py:61-120);
    each call evaluates all outputs on the device and returns row j as an (n, 1) column."""
    analytical_gradient_prediction = True

    def __init__(self, parent, j):
        self._p, self._j = parent, j
        self.model = _GPView(parent, j)

    def _col(self, a):
        return a[self._j][:, None].copy()

    def predict(self, X, full_cov=False):
        m, v = self._p.predict(X, full_cov)
        return self._col(m), self._col(v)

    def predict_noiseless(self, X, full_cov=False):
        m, v = self._p.predict_noiseless(X, full_cov)
        return self._col(m), self._col(v)

    def posterior_mean(self, X):
        return self._col(self._p.posterior_mean(np.atleast_2d(X)))

    def posterior_variance(self, X):
        return self._col(self._p.posterior_variance(np.atleast_2d(X)))

    def posterior_variance_noiseless(self, X):
        return self._col(self._p.posterior_variance_noiseless(np.atleast_2d(X)))

    def posterior_mean_gradient(self, X):     # gpmodel_fixed_hyps.py:187-192 -> (n, d)
        return self._p.posterior_mean_gradient(np.atleast_2d(X))[self._j].copy()

    def posterior_variance_gradient(self, X):
        return self._p.posterior_variance_gradient(np.atleast_2d(X))[self._j].copy()

    def set_hyperparameters(self, i):
        pass

    def get_fmin(self):                       # gpmodel_fixed_hyps.py:181-185
        return self._p.predict(self._p._X)[0][self._j].min()


def match_removed_row(prevX, X):
    """How X follows from prevX by deleting ONE row: (k, False) when X is prevX without row k, (k, True) when X is prevX without row k
    plus one new last row, None for every other change (the caller refits).  With duplicate rows several k describe the same X: the
    smallest is returned.  Pure NumPy: no device, no model state."""
    prevX, X = np.asarray(prevX), np.asarray(X)
    if prevX.ndim != 2 or X.ndim != 2 or prevX.shape[1] != X.shape[1] or prevX.shape[0] < 2:
        return None
    n = prevX.shape[0]
    if X.shape[0] == n - 1:
        kept, appended = X, False
    elif X.shape[0] == n:
        kept, appended = X[:-1], True
    else:
        return None
    differs = np.flatnonzero(np.any(prevX[:-1] != kept, axis=1))
    k = int(differs[0]) if differs.size else n - 1
    if not np.array_equal(prevX[k + 1:], kept[k:]):
        return None
    return k, appended


class multi_outputGP(object):
    """
    General class for handling a multi-output Gaussian process (drop-in for multi_outputGP.py:9).

    :param output_dim: number of outputs.
    :param kernel: list of kernels (bocf_amd.kern.* or duck-typed GPy kernels).  None entries: fixed_hyps ->
        SE(variance=2, lengthscale=0.3) (gpmodel_fixed_hyps.py:50); otherwise SE(variance=1, ARD=ARD[j]) (gpmodel.py:58).
    :param noise_var: list of noise variances.  None entries: fixed_hyps -> 1e-10 (gpmodel_fixed_hyps.py:56); otherwise
        0.01 Var(Y) as the starting value of a free noise (gpmodel.py:64).
    :param exact_feval: list of bools; with learning, True fixes the noise at 1e-6 (gpmodel.py:71-72).
    :param ARD: list of bools (default all True, multi_outputGP.py:44-47); used for default kernels when learning.
    :param n_samples: number of hyper-parameter samples (number_of_hyps_samples()).
    :param fixed_hyps: True -> GPModelFixedHyps semantics (one set of hyper-parameters, set_hyperparameters a no-op).
        False (the reference's default) -> GPModel semantics: every updateModel optimises the hyper-parameters, runs
        HMC and keeps n_samples draws (gpmodel.py:102-128); all inferences run on the device, the m outputs in
        lockstep (bocf_amd/hyper.py).  The sampler settings are the attributes n_burnin, subsample_interval,
        step_size, leapfrog_steps, max_iters (GPModel's defaults, gpmodel.py:32).
    :param device: HIP device index (default: LOCAL_RANK or 0).
    """
    analytical_gradient_prediction = True

    def __init__(self, output_dim, kernel=None, noise_var=None, exact_feval=None, n_samples=10, ARD=None, fixed_hyps=False,
                 device=None, reference_instance_kernels=False):
        self.output_dim = output_dim
        # fixed_hyps=False with a USER kernel: the reference learns the hyper-parameters with that kernel but builds its n_samples
        # prediction instances as SE whatever it was (gpmodel.py:57-61 resets self.kernel to None, :80-84 then takes the SE branch) and
        # writes the HMC samples into them (:121-126).  False (default): the instances keep the family that was learned.  True: the
        # reference's behaviour, bit for bit in the family it predicts with.
        self.reference_instance_kernels = bool(reference_instance_kernels)
        self.kernel = [None] * output_dim if kernel is None else list(kernel)
        self.noise_var = [None] * output_dim if noise_var is None else list(noise_var)
        self.exact_feval = [False] * output_dim if exact_feval is None else exact_feval
        self.n_samples = n_samples
        self.ARD = [True] * output_dim if ARD is None else ARD
        self.fixed_hyps = fixed_hyps
        if device is None:
            import os
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = device
        self._ctx = None
        self._X = None
        self._Y = None
        self._fitted = False
        self._resident = _Resident()
        self._fit_key = None
        self._cov_points = self._next_point = self._grad_point = None
        self.incremental = True       # O(N^2) updateModel when only targets change or one observation is appended
        # ... and, on request, when one row of X was deleted (with or without one new last row): bocf_remove (+ bocf_append).  Off by default:
        # an updateModel with fewer rows is a refit, as it always was (the jitter ladder and the schedule start afresh);
        # remove_observations needs no switch, CBO(max_observations=...) sets it on its model
        self.incremental_remove = False
        # ---- hyper-parameter learning (fixed_hyps=False): GPModel's sampler settings (gpmodel.py:32)
        self.n_burnin, self.subsample_interval, self.step_size, self.leapfrog_steps, self.max_iters = 100, 10, 1e-1, 20, 200
        # a leapfrog trajectory whose Ky stops factorizing: "raise" = the reference (LinAlgError out of jitchol propagates out of
        # updateModel, GPy/util/linalg.py:71 <- gpmodel.py:117-118); "reject" = drop that proposal for that output and carry on
        self.hmc_on_failure = "raise"
        self.device_hmc_streamed = True         # N > 128 (or d > 16): the stream-resident chain (bocf_hmc_streamed); False = lockstep host loop
        self.device_hmc = True                  # N <= 128, d <= 16: the whole HMC chain in one device launch (bocf_hmc); False = lockstep host loop
        self._H = 1 if fixed_hyps else int(n_samples)     # hyper-samples resident on the device
        self._current_h = 0                                # set_hyperparameters(h)
        self.sample_jitter_tries = 10                      # rungs of the jitter ladder of the joint posterior samples
        self.last_sample_jitter = None                     # the jitter per output of the last posterior_samples_f / thompson_topk draw
        self.last_pending_jitter = None                    # the jitter per output of the last set_pending_points
        self.last_joint_floored = None                     # floored pivots per batch of the last acq_joint
        self._sampler_outputs = None                       # per output: parameter state of GPModel.model
        self._Ymat = None                                  # (m, N) targets, cached for the inferences of one update
        self._ibuf = None                                  # argument block of bocf_infer (arrays + ctypes pointers)
        self._fit_serial = 0
        self._instances = None                             # [h][j] -> (variance, lengthscale (d,), noise): GPModel.model_instances
        self._kernel_ids = None
        self.hmc_samples = None
        self.last_update_info = {}
        self.jitter = None
        self.log_marginal = None
        self.output = [_OutputView(self, j) for j in range(output_dim)]

    # ---- device handle management (objects are pickled into pathos workers in the reference,
    # acquisition_optimizer.py:131-133: the handle is dropped and rebuilt lazily)
    def __getstate__(self):
        st = dict(self.__dict__)
        st["_ctx"] = None
        st["_fitted"] = False
        st["_resident"] = _Resident()
        st["_ibuf"] = None
        return st

    def _context(self):
        if self._ctx is None:
            self._ctx = _ffi.Context(self.device)
        return self._ctx

    def _ensure_fitted(self):
        if self._X is None:
            raise RuntimeError("updateModel has not been called")
        if not self._fitted:
            self._fit()

    def set_option(self, name, value):
        self._context().set_option(name, value)
        # the host copies of the last all-hyper-sample queries were made under the old options (predict_f32 / predict_i8 choose the
        # arithmetic of the variances): the next query goes to the device
        self._resident.forget("query", "gradient")
        if name in ("shard_fit", "shard_fit_simulate") and value:
            # an output-sharded fit exchanges the inverse factors only: the O(N^2) incremental updates need the upper factor,
            # which stays on its owner, so every updateModel is a (sharded) refit
            self.incremental = False

    # ---- fit ---------------------------------------------------------------------------------
    def updateModel(self, X_all, Y_all):
        """Updates the model with new observations (multi_outputGP.py:97-102): X_all (N, d),
        Y_all list of m arrays (N, 1)."""
        X = _ffi.f64(np.atleast_2d(X_all))
        Y = [np.asarray(y, dtype=np.float64).reshape(-1) for y in Y_all]
        if len(Y) != self.output_dim or any(y.shape[0] != X.shape[0] for y in Y):
            raise ValueError("Y_all must hold output_dim arrays of N observations")
        prevX = self._X
        self._resident.forget("candidates", "reference", "pending", "paths")      # every model change drops the device's reference set, pending points and paths
        self._X, self._Y = X.copy(), [y[:, None].copy() for y in Y]
        self._Ymat = None
        self._ibuf = None
        if not self.fixed_hyps:
            return self._update_hyper_samples()
        if self.incremental and self._fitted and prevX is not None and self._hyper_key() == self._fit_key:
            # cbo.py adds one observation per iteration (cbo.py:363,419) and the reference refits from scratch
            # (GP.set_XY, gp.py:191-227); with the factor resident on the device the two common cases are O(N^2)
            Ymat = _ffi.f64(np.stack(Y, 0))
            lib, ctx = _ffi.load(), self._context()
            lml = np.zeros(self.output_dim)
            if X.shape == prevX.shape and np.array_equal(X, prevX):
                _ffi.check(lib.bocf_update_targets(ctx.handle, _ffi.dptr(Ymat), _ffi.dptr(lml)), "bocf_update_targets")
                self.log_marginal = lml
                self._fit_serial += 1
                return
            if X.shape[0] == prevX.shape[0] + 1 and X.shape[1] == prevX.shape[1] and np.array_equal(X[:-1], prevX):
                xnew = _ffi.f64(X[-1])
                rc = _ffi.check(lib.bocf_append(ctx.handle, _ffi.dptr(xnew), _ffi.dptr(Ymat), _ffi.dptr(lml)), "bocf_append")
                if rc == 0:
                    self.log_marginal = lml
                    self._fit_serial += 1
                    return
            elif self.incremental_remove:
                # one row deleted (an outlier dropped, a sliding window), possibly with one new last row: O(N^2) as well
                hit = match_removed_row(prevX, X)
                if hit is not None and self._remove_then_append(hit[0], X, Y, Ymat, hit[1], lml):
                    self.log_marginal = lml
                    self._fit_serial += 1
                    return
        self._fit()

    def _remove_then_append(self, k, X, Y, Ymat, appended, lml):
        """bocf_remove of row k of the resident inputs, then (appended) bocf_append of X's last row.  False: the device asked for a refit."""
        lib, ctx = _ffi.load(), self._context()
        Yrem = Ymat if not appended else _ffi.f64(np.stack([y[:-1] for y in Y], 0))      # the targets of the rows that stay
        if _ffi.check(lib.bocf_remove(ctx.handle, int(k), _ffi.dptr(Yrem), _ffi.dptr(lml)), "bocf_remove") != 0:
            return False
        if not appended:
            return True
        xnew = _ffi.f64(X[-1])
        rc = _ffi.check(lib.bocf_append(ctx.handle, _ffi.dptr(xnew), _ffi.dptr(Ymat), _ffi.dptr(lml)), "bocf_append")
        if rc != 0:
            self._fitted = False                 # the device holds the model without row k and without the new row: refit
        return rc == 0

    def remove_observations(self, indices):
        """Removes the observations `indices` (rows of the training inputs) from the model: from the highest index down, one bocf_remove
        each -- O(N^2) per row on the resident factor -- or one refit of what remains when the device refuses (a jittered factor, an
        output-sharded fit) or no fixed-hyper-parameter fit is resident."""
        if self._X is None:
            raise RuntimeError("updateModel has not been called")
        N = self._X.shape[0]
        idx = sorted({int(i) + (N if int(i) < 0 else 0) for i in np.atleast_1d(indices)}, reverse=True)
        if not idx:
            return
        if idx[0] >= N or idx[-1] < 0:
            raise IndexError("observation index out of range")
        if len(idx) >= N:
            raise ValueError("at least one observation must remain")
        self._resident.forget("candidates", "reference", "pending", "paths")      # as every model change (updateModel)
        self._Ymat = None
        self._ibuf = None
        if not self.fixed_hyps:
            self._X, self._Y = np.delete(self._X, idx, axis=0), [np.delete(y, idx, axis=0) for y in self._Y]
            return self._update_hyper_samples()
        resident = self.incremental and self._fitted and self._hyper_key() == self._fit_key
        lib, ctx = _ffi.load(), self._context()
        lml = np.zeros(self.output_dim)
        for k in idx:
            self._X, self._Y = _ffi.f64(np.delete(self._X, k, axis=0)), [np.delete(y, k, axis=0) for y in self._Y]
            if resident:
                Ymat = _ffi.f64(np.stack([y[:, 0] for y in self._Y], 0))
                try:
                    resident = _ffi.check(lib.bocf_remove(ctx.handle, k, _ffi.dptr(Ymat), _ffi.dptr(lml)), "bocf_remove") == 0
                except Exception:
                    self._fitted = False         # the host arrays are ahead of the device model: the next use refits
                    raise
        if not resident:
            return self._fit()
        self.log_marginal = lml
        self._fit_serial += 1

    def _hyper_key(self):
        kids, var, ls, noise = self._hyper_arrays()
        return (tuple(kids), var.tobytes(), ls.tobytes(), noise.tobytes())

    def _hyper_arrays(self):
        """(kernel ids (M), variance (M,), lengthscale (M, d), noise (M,)) of the M = H * m factorizations resident on the
        device, hyper-sample-major (H = 1 with fixed hyper-parameters).  The outputs may use different kernel families (the
        reference takes a kernel list, multi_outputGP.py:44-47): the ids go to the device with bocf_set_kernel_ids."""
        d = self._X.shape[1]
        if not self.fixed_hyps:
            if self._instances is None:
                raise RuntimeError("updateModel has not been called")
            flat = [inst for group in self._instances for inst in group]
            inst_ids = [_ffi.KERN_SE] * self.output_dim if self.reference_instance_kernels else list(self._kernel_ids)      # gpmodel.py:80-84
            return (inst_ids * len(self._instances), _ffi.f64([v for v, _, _ in flat]), _ffi.f64([l for _, l, _ in flat]),
                    _ffi.f64([n for _, _, n in flat]))
        kids, var, ls = [], [], []
        for j in range(self.output_dim):
            k = self.kernel[j] if self.kernel[j] is not None else SE(d, variance=2., lengthscale=0.3)
            kj, vj, lj = kernel_spec(k, d)
            kids.append(int(kj))
            var.append(vj)
            ls.append(lj)
        noise = [1e-10 if nv is None else float(nv) for nv in self.noise_var]
        return kids, _ffi.f64(var), _ffi.f64(ls), _ffi.f64(noise)

    def _send_kernel_ids(self, kids):
        """Outputs of different kernel families: hand the id list to the device for the NEXT fit / inference / chain (it is consumed by
        that call); returns the scalar kernel id argument of that call."""
        kids = [int(k) for k in kids]
        if len(set(kids)) > 1:
            arr = (ctypes.c_int * len(kids))(*kids)
            _ffi.check(_ffi.load().bocf_set_kernel_ids(self._context().handle, arr, len(kids)), "bocf_set_kernel_ids")
        return kids[0]

    def _device_fit(self, kids, var, ls, noise, groups):
        """One bocf_fit over var.size factorizations (`groups` copies of the m targets); returns (jitter, lml)."""
        lib, ctx = _ffi.load(), self._context()
        kid = self._send_kernel_ids(kids)
        N, d = self._X.shape
        M = var.size
        Y = _ffi.f64(np.tile(np.stack([y[:, 0] for y in self._Y], 0), (groups, 1)))
        jit, lml = np.zeros(M), np.zeros(M)
        rc = lib.bocf_fit(ctx.handle, _ffi.dptr(self._X), _ffi.dptr(Y), N, d, M, kid, _ffi.dptr(var), _ffi.dptr(ls), _ffi.dptr(noise), 5,
                          _ffi.dptr(jit), _ffi.dptr(lml))
        self._refactorized(rc, "bocf_fit", M)
        return jit, lml

    def _refactorized(self, rc, what, M=None):
        """After every library call that factorizes anew (bocf_fit, bocf_infer, the HMC chains): the fit and the uploads that live with
        it are gone.  With M, a positive return raises jitchol's error for the outputs that failed."""
        _ffi.check(rc, what)
        self._fitted = False
        self._resident.forget("W", "Z", "program", "candidates", "paths")
        if M is not None and rc > 0:   # jitchol gave up (GPy/util/linalg.py:71) for the outputs whose last rung still has a bad pivot
            err = np.linalg.LinAlgError("not positive definite, even with jitter.")
            err.outputs = self._failed_outputs(M)
            raise err

    def _failed_outputs(self, M):
        """Outputs whose factorization failed in the last bocf_fit / bocf_infer (the library's own per-output info)."""
        info = (ctypes.c_int * M)()
        _ffi.check(_ffi.load().bocf_last_fit_info(self._context().handle, info, M), "bocf_last_fit_info")
        return [j for j in range(M) if info[j] != 0]

    def _fit(self):
        kids, var, ls, noise = self._hyper_arrays()
        self._context().set_option("hyper_samples", self._H)
        self.jitter, self.log_marginal = self._device_fit(kids, var, ls, noise, self._H)
        self._fit_key = self._hyper_key()
        self._fitted = True
        self._fit_serial += 1
        self._resident.forget("query", "gradient", "paths")

    # ---- hyper-parameter learning: GPModel._create_model / updateModel (gpmodel.py:50-128) ------------------------
    def _create_sampler_state(self):
        d = self._X.shape[1]
        self._sampler_outputs, self._instance_noise, kids = [], [], []
        for j in range(self.output_dim):
            k = self.kernel[j]
            if k is None:
                k = SE(d, variance=1., ARD=bool(self.ARD[j]))                        # gpmodel.py:58
            # (with a user kernel the reference builds its model_instances from SE all the same, gpmodel.py:80-84 -- a
            #  slip: self.kernel was reset to None at :61; here the instances keep the user's kernel family unless
            #  reference_instance_kernels=True asks for the reference's behaviour)
            kj, vj, lj = kernel_spec(k, d)
            kids.append(int(kj))
            ard = bool(getattr(k, "ARD", np.asarray(k.lengthscale).size > 1))
            if self.exact_feval[j]:
                noise, fixed = 1e-6, True                                            # gpmodel.py:71-72
            elif self.noise_var[j] is not None:
                noise, fixed = float(self.noise_var[j]), True                        # :73-74
            else:
                noise, fixed = float(np.var(self._Y[j])) * 0.01, False               # :64, :75-76
            self._sampler_outputs.append(OutputHyper(vj, lj if ard else lj[:1], noise, fixed))
            self._instance_noise.append(noise)
        self._kernel_ids = kids

    def _infer_buffers(self):
        """Argument block of bocf_infer, built once per data set: thousands of inferences reuse the same arrays and
        ctypes pointers."""
        N, d = self._X.shape
        m = self.output_dim
        key = (id(self._X), N, d, m)
        b = self._ibuf
        if b is None or b["key"] != key:
            if self._Ymat is None:
                self._Ymat = _ffi.f64(np.stack([y[:, 0] for y in self._Y], 0))
            hyp = np.zeros((m, d + 2))                     # [variance, lengthscale (d), noise] per output, one validity check
            arr = dict(var=np.zeros(m), ls=np.zeros((m, d)), noise=np.zeros(m), jit=np.zeros(m), lml=np.zeros(m), dv=np.zeros(m),
                       dl=np.zeros((m, d)), dn=np.zeros(m))
            b = dict(key=key, hyp=hyp, X=self._X, Y=self._Ymat, **arr)
            b["args"] = (_ffi.dptr(self._X), _ffi.dptr(self._Ymat), N, d, m, self._kernel_ids[0], _ffi.dptr(arr["var"]), _ffi.dptr(arr["ls"]),
                         _ffi.dptr(arr["noise"]), 5, _ffi.dptr(arr["jit"]), _ffi.dptr(arr["lml"]), _ffi.dptr(arr["dv"]), _ffi.dptr(arr["dl"]),
                         _ffi.dptr(arr["dn"]))
            self._ibuf = b
        return b

    def _infer(self, params):
        """One batched device inference for the m sampler models: log-marginals and their hyper-gradients."""
        b = self._infer_buffers()
        var, ls, noise, hyp = b["var"], b["ls"], b["noise"], b["hyp"]
        for j, (v, l, nz) in enumerate(params):
            var[j] = v
            ls[j] = l
            noise[j] = nz
        hyp[:, 0] = var
        hyp[:, 1:-1] = ls
        hyp[:, -1] = noise + 1.0                           # noise may be 0: shift it into the "> 0" test
        with np.errstate(invalid="ignore"):
            if not (np.isfinite(hyp).all() and (hyp[:, :-1] > 0).all() and (noise >= 0).all()):
                ok = np.isfinite(hyp).all(axis=1) & (hyp[:, :-1] > 0).all(axis=1) & (noise >= 0)
                err = np.linalg.LinAlgError("hyper-parameters left the positive domain")
                err.outputs = [int(j) for j in np.flatnonzero(~ok)]
                raise err
        self._send_kernel_ids(self._kernel_ids)             # (no-op unless the outputs differ in kernel family)
        rc = _ffi.load().bocf_infer(self._context().handle, *b["args"])
        self._refactorized(rc, "bocf_infer", self.output_dim)
        return b["lml"].copy(), b["dv"].copy(), b["dl"].copy(), b["dn"].copy()

    def _update_hyper_samples(self):
        from .hyper import LockstepSampler
        if self._sampler_outputs is None:
            self._create_sampler_state()
        outs, d = self._sampler_outputs, self._X.shape[1]
        sampler = LockstepSampler(outs, self._infer, d, device_hmc=self._device_hmc if self.device_hmc else None)
        ctx = self._context()
        sampler.evaluate()                       # first inference uploads X, Y; the thousands that follow reuse them
        ctx.set_option("reuse_data", 1)
        ctx.set_option("skip_mu_train", 1)
        try:
            opt_info, n_opt, num_samples, chains = self._optimize_and_sample(sampler, outs)
        finally:
            ctx.set_option("reuse_data", 0)
            ctx.set_option("skip_mu_train", 0)
        self.hmc_samples = [ch[self.n_burnin::self.subsample_interval] for ch in chains]                              # :119
        self._instances = []
        for h in range(self.n_samples):                                               # :121-126
            group = []
            for j, o in enumerate(outs):
                theta = o.param_array.copy()
                theta[-1] = self._instance_noise[j]        # a fixed noise keeps its constrained value in the instances
                theta[~o.fixed] = self.hmc_samples[j][h]
                ls = theta[1:-1]
                group.append((theta[0], np.full(d, ls[0]) if ls.size == 1 else ls.copy(), theta[-1]))
            self._instances.append(group)
        self.last_update_info = dict(optimizer_inferences=n_opt, hmc_inferences=sampler.n_inferences - n_opt,
                                     optimizer_iterations=opt_info["iterations"], accepted=sampler.accepted.copy(), num_samples=num_samples)
        self._fit()
        self._current_h = 0                                                           # :128

    def _device_hmc(self, outs, momenta, uniforms, hmc_iters, stepsize, raise_on_failure):
        """The chain of every output on the device (hmc.py:30-69): ONE launch for models with N <= 128, d <= 16 (bocf_hmc), the
        stream-resident chain beyond that (bocf_hmc_streamed: one inference's launches per leapfrog step, no host round trip).
        Returns (chains, accepted, diverged, n_inferences, status, draws_done); draws_done < len(uniforms[0]) means the streamed chain
        met a factorization that needs jitchol's ladder in that draw -- the caller runs it on the host and calls again for the rest.
        None when the model is outside what the device chains serve (outputs with different parameter counts)."""
        N, d = self._X.shape
        m = len(outs)
        sizes = {o.param_array.size for o in outs}
        if len(sizes) != 1:
            return None
        P = sizes.pop()
        nls = P - 2
        if nls not in (1, d):
            return None
        fused = N <= 128 and d <= 16
        if not fused and not self.device_hmc_streamed:
            return None
        ns = len(uniforms[0])
        theta = _ffi.f64(np.stack([o.param_array for o in outs]))
        fixed = np.ascontiguousarray(np.stack([o.fixed for o in outs]).astype(np.int32))
        mom = np.zeros((m, ns, P))
        for j in range(m):
            pf = int(np.sum(~outs[j].fixed))
            mom[j, :, :pf] = np.asarray(momenta[j], dtype=float).reshape(ns, pf)
        uni = _ffi.f64(np.stack([np.asarray(u, dtype=float) for u in uniforms]))
        if self._Ymat is None:
            self._Ymat = _ffi.f64(np.stack([y[:, 0] for y in self._Y], 0))
        chains = np.zeros((m, ns, P))
        acc, div, status = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
        ninf = ctypes.c_longlong(0)
        done = ctypes.c_int(ns)
        ip = ctypes.POINTER(ctypes.c_int)
        pr = outs[0].prior
        lib, ctx = _ffi.load(), self._context()
        kid = self._send_kernel_ids(self._kernel_ids)
        if fused:
            rc = lib.bocf_hmc(ctx.handle, _ffi.dptr(self._X), _ffi.dptr(self._Ymat), N, d, m, kid, _ffi.dptr(theta), nls,
                              fixed.ctypes.data_as(ip), pr.a, pr.b, _ffi.dptr(mom), _ffi.dptr(uni), ns, int(hmc_iters), float(stepsize), 5,
                              1 if raise_on_failure else 0, _ffi.dptr(chains), acc.ctypes.data_as(ip), div.ctypes.data_as(ip),
                              status.ctypes.data_as(ip), ctypes.byref(ninf))
            self._refactorized(rc, "bocf_hmc")
        else:
            rc = lib.bocf_hmc_streamed(ctx.handle, _ffi.dptr(self._X), _ffi.dptr(self._Ymat), N, d, m, kid, _ffi.dptr(theta), nls,
                                       fixed.ctypes.data_as(ip), pr.a, pr.b, _ffi.dptr(mom), _ffi.dptr(uni), ns, int(hmc_iters), float(stepsize),
                                       _ffi.dptr(chains), acc.ctypes.data_as(ip), div.ctypes.data_as(ip), ctypes.byref(done), ctypes.byref(ninf))
            self._refactorized(rc, "bocf_hmc_streamed")
        for j, o in enumerate(outs):
            o.param_array[:] = theta[j]
        out_chains = [chains[j, :, :int(np.sum(~outs[j].fixed))].copy() for j in range(m)]
        return out_chains, acc.astype(int), div.astype(int), ninf.value, status, int(done.value)

    def _optimize_and_sample(self, sampler, outs):
        from .hyper import LockstepSampler
        opt_info = sampler.optimize(self.max_iters)                                   # gpmodel.py:115
        n_opt = sampler.n_inferences
        num_samples = self.n_burnin + self.n_samples * self.subsample_interval
        draws = LockstepSampler.draw(outs, num_samples)
        for o, (eps, _, _) in zip(outs, draws):
            o.param_array[:] = o.param_array * (1. + eps * 0.01)                      # :116 (raw write: a fixed noise moves too)
        chains = sampler.hmc([dr[1] for dr in draws], [dr[2] for dr in draws], self.leapfrog_steps, self.step_size,
                             on_failure=self.hmc_on_failure)                          # :117-118
        return opt_info, n_opt, num_samples, chains

    def number_of_hyps_samples(self):
        return self.n_samples

    def set_hyperparameters(self, n):
        """gpmodel_fixed_hyps.py:76-77: no-op with fixed hyper-parameters; gpmodel.py:137-138: select hyper-sample n --
        every posterior query below answers for that sample (all n_samples factorizations stay on the device)."""
        if not self.fixed_hyps:
            if not 0 <= int(n) < self._H:
                raise IndexError("hyper-sample %r out of range (n_samples = %d)" % (n, self._H))
            self._current_h = int(n)

    def _rows(self):
        """Rows of the device's (H * m, ...) results that belong to the current hyper-sample."""
        return slice(self._current_h * self.output_dim, (self._current_h + 1) * self.output_dim)

    def get_evaluated_points(self):
        return np.copy(self._X)

    # ---- predictions ---------------------------------------------------------------------------
    def _set_candidates(self, X):
        self._ensure_fitted()
        X = _ffi.f64(X)
        if X.ndim != 2 or X.shape[1] != self._X.shape[1]:
            raise ValueError("candidates must be (n, %d)" % self._X.shape[1])
        self._resident.forget("candidates")
        _ffi.check(_ffi.load().bocf_set_candidates(self._context().handle, _ffi.dptr(X), X.shape[0]), "bocf_set_candidates")
        self._resident.candidates = X.shape[0]
        return X.shape[0]

    def _all_hyper_samples(self, slot, key, X, run):
        """A posterior query at X: `run(n)` makes the device call for the n staged candidates and returns its (H * m, n, ...) arrays.
        cbo.py walks the hyper-samples with set_hyperparameters(h) + a posterior query per h (cbo.py:162-166,176-178): the device
        answers for all H at once, so the queries after the first are slices of the same pass, kept in self._resident.`slot`."""
        if self._H == 1:
            return run(self._set_candidates(X))
        self._ensure_fitted()
        key = key + (np.shape(X), hash(np.ascontiguousarray(X, dtype=np.float64).tobytes()), self._fit_serial)
        hit = getattr(self._resident, slot)
        if hit is None or hit[0] != key:
            hit = (key, run(self._set_candidates(X)))
            setattr(self._resident, slot, hit)
        rows = self._rows()
        return tuple(None if a is None else a[rows].copy() for a in hit[1])

    def _predict(self, X, flags, want_var=True):
        def run(n):
            M = self.output_dim * self._H
            mean = np.empty((M, n))
            var = np.empty((M, n)) if want_var else None
            if n:
                _ffi.check(_ffi.load().bocf_predict(self._context().handle, flags, _ffi.dptr(mean), _ffi.dptr(var)), "bocf_predict")
            return mean, var
        return self._all_hyper_samples("query", ("p", flags, want_var), X, run)

    def predict(self, X, full_cov=False):
        """Posterior means and variances at X, likelihood noise included, clipped at 1e-10
        (multi_outputGP.py:138-149 -> gpmodel_fixed_hyps.py:79-87).  Returns ((m, n), (m, n))."""
        if full_cov:
            # each output's model returns its n x n covariance and the wrapper keeps column 0 of it (multi_outputGP.py:146-148):
            # row j = the covariances of every point with the FIRST one, noise on entry 0, every entry clipped at 1e-10
            X = np.atleast_2d(X)
            mean, _ = self._predict(X, 0, want_var=False)
            M = self.output_dim * self._H
            cov = np.empty((M, X.shape[0]))
            if self._set_candidates(X):         # (the mean may have come from the hyper-sample cache without touching the device)
                _ffi.check(_ffi.load().bocf_predict_cov_column(self._context().handle, _ffi.ADD_NOISE | _ffi.CLIP, _ffi.dptr(cov)),
                           "bocf_predict_cov_column")
            return mean, cov[self._rows()].copy()
        return self._predict(np.atleast_2d(X), _ffi.ADD_NOISE | _ffi.CLIP)

    def predict_noiseless(self, X, full_cov=False):
        """multi_outputGP.py:151-162 -> gpmodel_fixed_hyps.py:89-97 / gpmodel.py:151-159 (full_cov is accepted and never looked at)."""
        return self._predict(np.atleast_2d(X), _ffi.CLIP)

    def posterior_mean(self, X):
        """multi_outputGP.py:165-173."""
        return self._predict(X, 0, want_var=False)[0]

    def posterior_variance(self, X):
        """Noise included, clipped (multi_outputGP.py:183-191 -> gpmodel_fixed_hyps.py:106-112)."""
        return self._predict(X, _ffi.ADD_NOISE | _ffi.CLIP)[1]

    def posterior_variance_noiseless(self, X):
        """multi_outputGP.py:194-200."""
        return self._predict(X, _ffi.CLIP)[1]

    def posterior_mean_at_evaluated_points(self):
        """multi_outputGP.py:176-180; cached on the device at fit time."""
        self._ensure_fitted()
        out = np.empty((self.output_dim * self._H, self._X.shape[0]))
        _ffi.check(_ffi.load().bocf_mean_at_train(self._context().handle, _ffi.dptr(out)), "bocf_mean_at_train")
        return out[self._rows()].copy() if self._H > 1 else out

    def _gradients(self, X):
        def run(n):
            shape = (self.output_dim * self._H, n, self._X.shape[1])
            dmean, dvar = np.empty(shape), np.empty(shape)
            if n:
                _ffi.check(_ffi.load().bocf_predict_gradients(self._context().handle, _ffi.dptr(dmean), _ffi.dptr(dvar)), "bocf_predict_gradients")
            return dmean, dvar
        return self._all_hyper_samples("gradient", ("g",), np.atleast_2d(X), run)

    def posterior_mean_gradient(self, X):
        """d mu / dX, (m, n, d)  (multi_outputGP.py:284-294 -> gp.py:438-461)."""
        return self._gradients(X)[0]

    def posterior_variance_gradient(self, X):
        """d var / dX, (m, n, d)  (multi_outputGP.py:297-306 -> gp.py:464-490)."""
        return self._gradients(X)[1]

    # ---- look-ahead posterior (multi_outputGP.py:203-281,309-330 -> GPy/core/gp.py:493-627): covariance against a staged point set,
    # variance conditioned on a next point, gradients of the posterior covariance -- what the knowledge-gradient acquisitions are built
    # from (bocf_amd.uKG).  All act on the current hyper-sample, like posterior_covariance_between_points.  The device keeps ONE resident
    # reference set; the set a method needs is staged when it differs from the resident one (keyed like set_mc_samples), so the three
    # "partial precomputations" can be interleaved freely.  Two deliberate differences from the reference's array shapes: the
    # covariance-gradient methods are defined for every kernel family (the reference's only work for its SE kernel), and they take ONE
    # point x2 (1, d) -- the only case in which the reference's (m, n, d) result is defined.
    def _off_path(self, *a, **kw):
        raise NotImplementedError("not part of the accelerated path: cbo.py and the maEI/maPI/uEI_noiseless/uPI/EI/PI acquisitions never "
                                  "call it (SURVEY.md section 8b)")

    def _points(self, X, what):
        if self._X is None:
            raise RuntimeError("updateModel has not been called")
        X = _ffi.f64(np.atleast_2d(X))
        if X.ndim != 2 or X.shape[1] != self._X.shape[1]:
            raise ValueError("%s must be (n, %d)" % (what, self._X.shape[1]))
        return X

    def set_reference_points(self, A):
        """Stage the reference set A (na, d), 1 <= na <= 1024, on the device for ALL hyper-samples (bocf_set_ref_points): V_A, Ky^-1 K(X, A),
        mu(A), sigma^2(A).  It stays resident until it is replaced or the model changes; re-sending the resident set is free."""
        self._ensure_fitted()
        A = self._points(A, "the reference points")
        key = (A.shape, hash(A.tobytes()), self._fit_serial)
        if key == self._resident.reference:
            return
        self._resident.forget("reference")
        _ffi.check(_ffi.load().bocf_set_ref_points(self._context().handle, _ffi.dptr(A), A.shape[0]), "bocf_set_ref_points")
        self._resident.reference = key

    def _staged(self, name, what):
        P = getattr(self, name, None)
        if P is None:
            raise RuntimeError("%s has not been called" % what)
        return P

    def partial_precomputation_for_covariance(self, X):
        """multi_outputGP.py:203-210 -> gp.py:547-561: X (n2, d) becomes the precomputed point set."""
        self._cov_points = self._points(X, "X").copy()
        self.set_reference_points(self._cov_points)

    def posterior_covariance_between_points_partially_precomputed(self, X1, X2):
        """Noiseless, unclipped posterior covariance between X1 (n1, d) and the precomputed set X2, (m, n1, n2)
        (multi_outputGP.py:269-281 -> gp.py:564-573).  X2 must be the set given to partial_precomputation_for_covariance."""
        X2 = self._points(X2, "X2")
        P = self._staged("_cov_points", "partial_precomputation_for_covariance")
        if X2.shape != P.shape or not np.array_equal(X2, P):
            raise ValueError("X2 is not the point set given to partial_precomputation_for_covariance")
        return self._cov_to_ref(X1, P, grad=False)[0]

    def _cov_to_ref(self, X, A, grad):
        """(Sigma(X, A) (m, n, na), d Sigma(X_i, a) / d X_i (m, n, na, d) or None) for the current hyper-sample."""
        self._ensure_fitted()
        X = self._points(X, "X")
        self.set_reference_points(A)
        n = self._set_candidates(X)
        na, d = A.shape
        cov = np.empty((self.output_dim, n, na))
        dcov = np.empty((self.output_dim, n, na, d)) if grad else None
        if n:
            _ffi.check(_ffi.load().bocf_cov_to_ref(self._context().handle, self._group(), _ffi.dptr(cov), _ffi.dptr(dcov)), "bocf_cov_to_ref")
        return cov, dcov

    def partial_precomputation_for_variance_conditioned_on_next_point(self, next_point):
        """multi_outputGP.py:223-230 -> gp.py:493-511: stages the next point (1, d)."""
        P = self._points(next_point, "next_point")
        if P.shape[0] != 1:
            raise ValueError("next_point must be one point (1, d)")
        self._next_point = P.copy()

    def _conditioned(self, X, grad):
        self._ensure_fitted()
        P = self._staged("_next_point", "partial_precomputation_for_variance_conditioned_on_next_point")
        X = self._points(X, "X")
        self.set_reference_points(P)
        n = self._set_candidates(X)
        var = np.empty((self.output_dim, n))
        dvar = np.empty((self.output_dim, n, X.shape[1])) if grad else None
        if n:
            _ffi.check(_ffi.load().bocf_conditioned_variance(self._context().handle, self._group(), 0, _ffi.dptr(var), _ffi.dptr(dvar)),
                       "bocf_conditioned_variance")
        return var, dvar

    def posterior_variance_conditioned_on_next_point(self, X):
        """Variance at X (n, d) once the staged next point has been observed, (m, n): sigma^2(X) - Sigma(X, x)^2 / (max(sigma^2(x), 0) +
        noise + 1e-8 + jitter), raw -- no clip, no noise (multi_outputGP.py:233-242 -> gp.py:514-544, which factorizes the bordered Ky)."""
        return self._conditioned(X, False)[0]

    def posterior_variance_gradient_conditioned_on_next_point(self, X):
        """Its gradient in X, (m, n, d) (multi_outputGP.py:245-254)."""
        return self._conditioned(X, True)[1]

    def posterior_covariance_gradient(self, X, x2):
        """d Sigma(X_i, x2) / d X_i for ONE point x2 (1, d), (m, n, d) (multi_outputGP.py:309-318 -> gp.py:586-610)."""
        P = self._points(x2, "x2")
        if P.shape[0] != 1:
            raise ValueError("x2 must be one point (1, d)")
        return self._cov_to_ref(X, P, grad=True)[1][:, :, 0, :].copy()

    def partial_precomputation_for_covariance_gradient(self, x):
        """multi_outputGP.py:213-220 -> gp.py:613-618: stages the point x (1, d) of the next method."""
        P = self._points(x, "x")
        if P.shape[0] != 1:
            raise ValueError("x must be one point (1, d)")
        self._grad_point = P.copy()

    def posterior_covariance_gradient_partially_precomputed(self, X, x2):
        """As posterior_covariance_gradient, for the point staged by partial_precomputation_for_covariance_gradient
        (multi_outputGP.py:321-330 -> gp.py:621-627)."""
        P = self._staged("_grad_point", "partial_precomputation_for_covariance_gradient")
        x2 = self._points(x2, "x2")
        if x2.shape != P.shape or not np.array_equal(x2, P):
            raise ValueError("x2 is not the point given to partial_precomputation_for_covariance_gradient")
        return self._cov_to_ref(X, P, grad=True)[1][:, :, 0, :].copy()

    def acq_kg(self, X, mode, util_kind, util_params, thetas, prob, Zf, W=None, n_hyps=None, grad=False, fetch=True):
        """Discrete composite knowledge gradient of the batch X (n, d) against the resident reference set (bocf_acq_kg): `mode` "mean",
        "closed" or "mc" (or the _ffi.EU_* value) is the inner expectation, Zf (Sf, m) the fantasy normals, W (S, m) the common random
        numbers of the "mc" mode.  Returns KG (n,), or (KG (n,), dKG/dX (n, d)) with grad=True.  The values stay on the device for
        select_topk (fetch=False returns None)."""
        mode = _ffi.eu_mode(mode)
        self._begin_acq(n_hyps, True)
        self._resident_for_fit("reference", "no reference points resident for this fit: call set_reference_points")
        if mode == _ffi.EU_MC and W is None:
            raise ValueError("the Monte-Carlo mode needs W (S, output_dim)")

        def fantasies():
            Z = _ffi.f64(np.atleast_2d(Zf))
            if Z.shape[1] != self.output_dim:
                raise ValueError("Zf must be (Sf, output_dim)")
            return _ffi.dptr(Z), Z.shape[0]
        return self._run_acq("bocf_acq_kg", (mode, int(util_kind)), X, util_params, thetas, prob, W if mode == _ffi.EU_MC else None, grad, fetch,
                             tail=fantasies)

    # ---- pending points of a greedy batch -------------------------------------------------------------------------------------
    def set_pending_points(self, P, Zp, W=None):
        """Stage the pending points P (r, d), 1 <= r <= 15, of a batch under construction for ALL hyper-samples (bocf_set_pending_points)
        with the joint normals Zp (S, output_dim, r): the device keeps Q = (Sigma(P, P) + tau I)^-1 and the joint samples at P.  S must be
        the number of resident Monte-Carlo samples (W (S, output_dim) is uploaded first when given).  The set stays resident until it is
        replaced or the model changes -- the reference set of set_reference_points is not touched; re-sending the resident set is free.
        The jitter tau per output is kept in last_pending_jitter."""
        self._ensure_fitted()
        if W is not None:
            self.set_mc_samples(W)
        P = self._points(P, "the pending points")
        Zp = _ffi.f64(Zp)
        if Zp.ndim != 3 or Zp.shape[1:] != (self.output_dim, P.shape[0]):
            raise ValueError("Zp must be (S, output_dim, r)")
        key = (P.shape, hash(P.tobytes()), Zp.shape, hash(Zp.tobytes()), self._fit_serial)
        if key == self._resident.pending:
            return
        self._resident.forget("pending")
        jit = np.empty(self.output_dim * self._H)
        rc = _ffi.check(_ffi.load().bocf_set_pending_points(self._context().handle, _ffi.dptr(P), P.shape[0], _ffi.dptr(Zp), Zp.shape[0],
                                                            self.sample_jitter_tries, _ffi.dptr(jit)), "bocf_set_pending_points")
        self.last_pending_jitter = jit
        if rc > 0:
            raise np.linalg.LinAlgError("covariance of the pending points of output %d not positive definite, even with jitter %g" % (rc - 1, jit[rc - 1]))
        self._resident.pending = key

    def pending_samples(self):
        """The joint samples F at the resident pending points, (H * output_dim, r, S) (bocf_get_pending_samples)."""
        key = self._resident_for_fit("pending", "no pending points resident for this fit: call set_pending_points")
        (r, _), (S, _, _) = key[0], key[2]
        F = np.empty((self.output_dim * self._H, r, S))
        _ffi.check(_ffi.load().bocf_get_pending_samples(self._context().handle, _ffi.dptr(F)), "bocf_get_pending_samples")
        return F

    def acq_pending(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, grad=False, fetch=True):
        """Monte-Carlo expected improvement of the batch X (n, d) conditioned on the resident pending points (bocf_acq_pending):
        alpha(x | P) = qEI(P u {x}) - qEI(P) for the staged normals; W (S, output_dim) are the common random numbers of the Monte-Carlo
        acquisitions.  The best-so-far is that of acq_mc: the hyper-sample current on entry.  Returns alpha (n,), or
        (alpha (n,), d alpha / dX (n, d)) with grad=True.  The values stay on the device for select_topk (fetch=False returns None)."""
        self._begin_acq(n_hyps, False)
        self._resident_for_fit("pending", "no pending points resident for this fit: call set_pending_points")
        return self._run_acq("bocf_acq_pending", (int(util_kind),), X, util_params, thetas, prob, W, grad, fetch)

    # ---- joint q-point expected improvement ------------------------------------------------------------------------------------------
    def acq_joint(self, X, q, util_kind, util_params, thetas, prob, Z, n_hyps=None, best=None, grad=False):
        """Joint Monte-Carlo expected improvement of the composite utility at B batches of q points, 1 <= q <= 8 (bocf_acq_joint): X is
        (B, q, d), (B, q * d) or (B * q, d), Z (S, output_dim, q), S <= 256, the normals common to all batches and hyper-samples.  best:
        None = the best-so-far of acq_mc (the hyper-sample current on entry), or the incumbents (L,) or (hyper-samples averaged, L).
        Returns alpha (B,), or (alpha (B,), d alpha / dX (B, q, d)) with grad=True (B * q <= 128 then).  The number of floored pivots
        of every batch is kept in last_joint_floored (B,); the values stay on the device for select_topk, which then ranks batches."""
        q = int(q)
        if not 1 <= q <= 8:
            raise ValueError("q must be in 1 .. 8")
        Z = _ffi.f64(Z)
        if Z.ndim != 3 or Z.shape[1:] != (self.output_dim, q) or not 1 <= Z.shape[0] <= 256:
            raise ValueError("Z must be (1 <= S <= 256, output_dim, q)")
        if self._X is None:
            raise RuntimeError("no model yet: call updateModel first")
        d = self._X.shape[1]
        X = _ffi.f64(X)
        if X.size == 0 or X.size % (q * d):
            raise ValueError("X must hold whole batches of q points: (B, q, %d), (B, q * %d) or (B * q, %d)" % (d, d, d))
        X = X.reshape(-1, d)
        B = X.shape[0] // q
        if grad and X.shape[0] > 128:
            raise ValueError("the gradient form takes at most 128 points (B * q <= 128)")
        self._begin_acq(n_hyps, False)
        util = self._utility_args(util_params, thetas, prob)
        if best is not None:
            n_h = 1 if self.fixed_hyps else (self._H if n_hyps is None else max(1, min(int(n_hyps), self._H)))
            best = _ffi.f64(best)
            if best.shape not in ((util[5],), (n_h, util[5])):
                raise ValueError("best must be (L,) or (hyper-samples averaged, L) = (%d, %d)" % (n_h, util[5]))
            best = _ffi.f64(np.broadcast_to(best, (n_h, util[5])))
        self._set_candidates(X)
        acq = np.empty(B)
        dacq = np.empty((B, q, d)) if grad else None
        floored = np.zeros(B, dtype=np.int32)
        _ffi.check(_ffi.load().bocf_acq_joint(self._context().handle, q, _ffi.dptr(Z), Z.shape[0], int(util_kind), *util, _ffi.dptr(best), _ffi.dptr(acq),
                                              _ffi.dptr(dacq), floored.ctypes.data_as(ctypes.POINTER(ctypes.c_int))), "bocf_acq_joint")
        self.last_joint_floored = floored.astype(int)
        return (acq, dacq) if grad else acq

    # ---- linear output constraints and the constrained Monte-Carlo acquisition ---------------------------------------------------
    def set_output_constraints(self, constraints):
        """Stage an OutputConstraints (A y - b <= 0, temperatures eta) on the device (bocf_set_output_constraints); None drops the resident
        set.  The set stays resident until it is replaced: it does not depend on the fit, so updateModel leaves it; re-sending the resident
        set is free."""
        self._ensure_fitted()
        lib, h = _ffi.load(), self._context().handle
        if constraints is None:
            _ffi.check(lib.bocf_set_output_constraints(h, None, None, None, 0, self.output_dim), "bocf_set_output_constraints")
            self._resident.forget("constraints")
            return
        if constraints.m != self.output_dim:
            raise ValueError("the constraints are on %d outputs, the model has %d" % (constraints.m, self.output_dim))
        key = constraints.key()
        if key == self._resident.constraints:
            return
        self._resident.forget("constraints")
        _ffi.check(lib.bocf_set_output_constraints(h, _ffi.dptr(constraints.A), _ffi.dptr(constraints.b), _ffi.dptr(constraints.eta), constraints.K,
                                                   constraints.m), "bocf_set_output_constraints")
        self._resident.constraints = key

    def _constraints_resident(self):
        if self._resident.constraints is None:
            raise RuntimeError("no output constraints resident: call set_output_constraints")

    def feasible_best(self, util_kind, util_params, thetas):
        """(best (L,), n_feasible): per utility parameter the best U(theta_l, mu(X_i)) over the training points whose posterior mean passes
        the HARD test A mu - b <= 0 of the resident constraints (-inf when none does), and how many pass (bocf_feasible_best); the
        posterior mean is that of the current hyper-sample."""
        self._ensure_fitted()
        self._constraints_resident()
        if not self.fixed_hyps:
            self._context().set_option("best_group", self._current_h)
        params, n_params, th, tdim, _, L = self._utility_args(util_params, thetas, None)
        best, nf = np.empty(L), ctypes.c_longlong()
        _ffi.check(_ffi.load().bocf_feasible_best(self._context().handle, int(util_kind), params, n_params, th, tdim, L, _ffi.dptr(best), ctypes.byref(nf)),
                   "bocf_feasible_best")
        return best, int(nf.value)

    def acq_mc_constrained(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, grad=False, fetch=True):
        """Constrained Monte-Carlo expected improvement of the batch X (n, d) (bocf_acq_mc_constrained): every sample of the uEI sum is
        weighed by the smoothed feasibility of the resident constraints, the incumbent is the best FEASIBLE training point of the
        hyper-sample current on entry (none feasible: the smoothed probability of feasibility).  Conventions of acq_mc: W (S, output_dim)
        are the common random numbers.  Returns alpha (n,), or (alpha (n,), d alpha / dX (n, d)) with grad=True.  The values stay on the
        device for select_topk (fetch=False returns None)."""
        self._begin_acq(n_hyps, False)
        self._constraints_resident()
        return self._run_acq("bocf_acq_mc_constrained", (int(util_kind),), X, util_params, thetas, prob, W, grad, fetch)

    # ---- quantile / tail-mean acquisitions of the composite utility and the closed-form confidence bound -------
    def acq_risk(self, X, kind, rank, util_kind, util_params, thetas, prob, W=None, n_hyps=None, grad=False, fetch=True):
        """Order statistic of the Monte-Carlo samples of the composite utility over the batch X (n, d) (bocf_acq_risk): with the samples
        u_s = U(theta_l, mu + sigma o W_s) in ascending order (ties by sample index, NaN as -inf), `kind` _ffi.RISK_QUANTILE is u_(rank),
        _ffi.RISK_UPPER_TAIL the mean of u_(rank) .. u_(S-1), _ffi.RISK_LOWER_TAIL the mean of u_(0) .. u_(rank); 0 <= rank <= S - 1 is an
        integer (the caller turns a level into it), S <= 4096.  Conventions of acq_mc: W (S, output_dim) are the common random numbers;
        there is no incumbent.  Returns alpha (n,), or (alpha (n,), d alpha / dX (n, d)) with grad=True (pathwise over the selected
        samples).  The values stay on the device for select_topk (fetch=False returns None)."""
        self._begin_acq(n_hyps, False)
        return self._run_acq("bocf_acq_risk", (int(kind), int(rank), int(util_kind)), X, util_params, thetas, prob, W, grad, fetch)

    def acq_linear_ucb(self, X, kappa, thetas, prob, n_hyps=None, grad=False, fetch=True):
        """Closed-form confidence bound of theta . f over the batch X (n, d) (bocf_acq_linear_ucb):
        sum_l p_l [theta_l . mu + kappa sqrt(sum_j theta_lj^2 var_j)], averaged over the hyper-samples; thetas (L, output_dim).  Returns
        alpha (n,), or (alpha (n,), d alpha / dX (n, d)) with grad=True.  The values stay on the device for select_topk."""
        self._begin_acq(n_hyps, False)
        thetas = _ffi.f64(np.atleast_2d(thetas))
        if thetas.shape[1] != self.output_dim:
            raise ValueError("theta must have output_dim entries")
        prob = None if prob is None else _ffi.f64(np.atleast_1d(prob))
        return self._call_acq("bocf_acq_linear_ucb", lambda: (float(kappa), _ffi.dptr(thetas), _ffi.dptr(prob), thetas.shape[0]), X, None, grad, fetch)

    # ---- log-space expected improvement --------------------------------------------------------------------------
    def acq_log_linear(self, X, thetas, prob, n_hyps=None, grad=False, fetch=True):
        """log EI of theta . f over the batch X (n, d) in closed form (bocf_acq_log_linear): the log-sum-exp over the hyper-samples and
        the parameters of log p_l - log H + log sigma + log h(z), h(z) = phi(z) + z Phi(z), with acq_linear's posterior and incumbents
        (each hyper-sample's own); thetas (L, output_dim).  Finite and with a useful gradient where acq_linear returns an exact 0.
        Returns log alpha (n,), or (log alpha (n,), d log alpha / dX (n, d)) with grad=True.  The values stay on the device for
        select_topk (fetch=False returns None)."""
        self._begin_acq(n_hyps, True)
        thetas = _ffi.f64(np.atleast_2d(thetas))
        if thetas.shape[1] != self.output_dim:
            raise ValueError("theta must have output_dim entries")
        prob = None if prob is None else _ffi.f64(np.atleast_1d(prob))
        return self._call_acq("bocf_acq_log_linear", lambda: (_ffi.dptr(thetas), _ffi.dptr(prob), thetas.shape[0]), X, None, grad, fetch)

    def acq_log_mc(self, X, util_kind, util_params, thetas, prob, tau, W=None, n_hyps=None, grad=False, program=None, fetch=True):
        """Log of the smooth surrogate of the Monte-Carlo EI of a device utility over the batch X (n, d) (bocf_acq_log_mc): the
        log-sum-exp over hyper-samples, parameters and samples of log p_l - log(H S) + log tau + log psi((U - best_l) / tau),
        psi(t) = softplus(t) + 0.1 / (1 + t^2), with acq_mc's posterior, samples W (S, output_dim) and incumbents (the hyper-sample
        current on entry).  `tau` > 0 is in the units of the utility: exp(result) exceeds acq_mc's EI by at most tau (ln 2 + 0.1).
        `program`: the blob for utility kind UTIL_PROGRAM.  Returns log alpha (n,), or (log alpha (n,), d log alpha / dX (n, d)) with
        grad=True (pathwise).  The values stay on the device for select_topk (fetch=False returns None)."""
        self._begin_acq(n_hyps, False)
        if util_kind == _ffi.UTIL_PROGRAM:
            self.set_utility_program(program)
        return self._run_acq("bocf_acq_log_mc", (float(tau), int(util_kind)), X, util_params, thetas, prob, W, grad, fetch)

    # ---- joint posterior and composite Thompson sampling ------------------------------------------------------------------------
    def _group(self):
        """Device group of the current hyper-sample (bocf_posterior_cov / bocf_posterior_samples)."""
        return self._current_h if self._H > 1 else 0

    def posterior_covariance_between_points(self, X1, X2):
        """Noiseless, unclipped posterior covariance between X1 (n1, d) and X2 (n2, d) for the current hyper-sample
        (multi_outputGP.py:257-266 -> gp.py:576-583 -> posterior.py:104-125): k(X1, X2) - k(X1, X) Ky^-1 k(X, X2).  Returns (m, n1, n2)."""
        self._ensure_fitted()
        X1, X2 = _ffi.f64(np.atleast_2d(X1)), _ffi.f64(np.atleast_2d(X2))
        d = self._X.shape[1]
        if X1.shape[1] != d or X2.shape[1] != d:
            raise ValueError("X1 and X2 must be (n, %d)" % d)
        out = np.empty((self.output_dim, X1.shape[0], X2.shape[0]))
        _ffi.check(_ffi.load().bocf_posterior_cov(self._context().handle, _ffi.dptr(X1), X1.shape[0], _ffi.dptr(X2), X2.shape[0], self._group(),
                                                  _ffi.dptr(out)), "bocf_posterior_cov")
        return out

    def _posterior_samples(self, group, Z, keep_out=True):
        """Joint samples at the resident candidates for device group `group` from Z (M_g, C, S); returns (samples or None, jitter (M_g,))."""
        Z = _ffi.f64(Z)
        M = Z.shape[0]
        out = np.empty(Z.shape) if keep_out else None
        jit = np.empty(M)
        rc = _ffi.load().bocf_posterior_samples(self._context().handle, int(group), _ffi.dptr(Z), Z.shape[2], self.sample_jitter_tries,
                                                _ffi.dptr(out), _ffi.dptr(jit))
        _ffi.check(rc, "bocf_posterior_samples")
        self.last_sample_jitter = jit
        if rc > 0:
            raise np.linalg.LinAlgError("posterior covariance of output %d not positive definite, even with jitter %g" % (rc - 1, jit[rc - 1]))
        return out, jit

    def posterior_samples_f(self, X, size=10, Z=None):
        """Joint samples of the latent outputs at X (n, d) for the current hyper-sample, GPy's fsim layout (gp.py:794-828): (m, n, size).
        f = mu + L Z with L the Cholesky factor of the noiseless posterior covariance + jitter I (jitter ladder from 1e-8 mean(diag),
        the jitter used is kept in last_sample_jitter).  Z defaults to np.random.normal(size=(m, n, size)).  GPy draws with
        np.random.multivariate_normal, which factors by SVD: seeded draws differ from GPy's, with the same distribution."""
        self._ensure_fitted()
        X = np.atleast_2d(X)
        if Z is None:
            Z = np.random.normal(size=(self.output_dim, X.shape[0], int(size)))
        Z = _ffi.f64(Z)
        if Z.shape[:2] != (self.output_dim, X.shape[0]):
            raise ValueError("Z must be (output_dim, n, size)")
        self._set_candidates(X)
        return self._posterior_samples(self._group(), Z)[0]

    def thompson_topk(self, X, thetas, path_groups, Z, utility, k):
        """Composite Thompson sampling on the candidate set X (C, d): path s draws a joint sample f_s of all outputs from hyper-sample
        path_groups[s] with the normals of Z[h] (dict: hyper-sample -> (m, C, paths of h in path order)) and ranks the candidates by
        U(thetas[s], f_s(c)).  One device sampling call per hyper-sample used, one selection call.  Returns (idx (P, k), val (P, k)) in
        path order, value descending, ties to the lowest index."""
        self._ensure_fitted()
        thetas = _ffi.f64(np.asarray(thetas, dtype=float).reshape(len(path_groups), -1))
        path_groups = np.asarray(path_groups, dtype=int)
        P = path_groups.size
        dev = path_groups if self._H > 1 else np.zeros(P, dtype=int)
        kind, params = self._device_utility(utility)
        self._set_candidates(X)
        order = []
        for g in sorted(set(dev.tolist())):
            hs = sorted(set(path_groups[dev == g].tolist()))          # (fixed hyper-parameters: the draws of every h feed group 0)
            Zg = np.concatenate([Z[h] for h in hs], axis=2)
            self._posterior_samples(g, Zg, keep_out=False)
            order += [s for h in hs for s in np.flatnonzero(path_groups == h)]
        return self._select_paths(kind, params, thetas, np.asarray(order, dtype=int), k)

    def _select_paths(self, kind, params, thetas, order, k):
        """One bocf_thompson_select over the resident samples (the device's path p is path order[p]); arguments and result in path order."""
        P = order.size
        pa, n_pa, th, tdim, _, _ = self._utility_args(params, thetas[order], None)
        idx = np.empty((P, k), dtype=np.int64)
        val = np.empty((P, k))
        _ffi.check(_ffi.load().bocf_thompson_select(self._context().handle, kind, pa, n_pa, th, tdim, int(k), idx.ctypes.data_as(_ffi._c_ll_p),
                                                    _ffi.dptr(val)), "bocf_thompson_select")
        out_idx, out_val = np.empty_like(idx), np.empty_like(val)
        out_idx[order], out_val[order] = idx, val
        return out_idx, out_val

    # ---- pathwise posterior samples: Thompson paths as functions --------------------------------------------------------------
    def _path_groups(self, n_paths):
        """Hyper-sample of path s: s mod min(10, number_of_hyps_samples()) (the acquisitions' hyper-sample count)."""
        return np.arange(int(n_paths)) % min(10, self.number_of_hyps_samples())

    def draw_paths(self, n_paths, n_features=1024):
        """Draw and stage n_paths posterior sample paths f_s(.) of all outputs (Matheron's rule with n_features random Fourier features per
        output, bocf_set_paths); path s belongs to hyper-sample s mod min(10, number_of_hyps_samples()).  A path is a function: it stays
        resident through every candidate upload and is dropped with the posterior (updateModel, refits).  Given the frequencies the
        path mean is the posterior mean exactly; the path variance is that of the feature approximation of the prior.
        np.random draw order: per device hyper-sample used, in increasing h (one, holding every path, with fixed hyper-parameters): per
        output j: z = normal(F, d); for the Matern kernels only chi2 = chisquare(2 nu, F) (omega = z / sqrt(chi2 / (2 nu)), nu = 5/2 or 3/2);
        b = uniform(0, 2 pi, F); w = normal(F, S_h); E = normal(N, S_h), with S_h the number of paths of h."""
        self._ensure_fitted()
        n_paths, F = int(n_paths), int(n_features)
        if n_paths < 1 or F < 1:
            raise ValueError("n_paths and n_features must be >= 1")
        groups = self._path_groups(n_paths)
        dev = groups if self._H > 1 else np.zeros(n_paths, dtype=int)
        kids = self._hyper_arrays()[0]
        N, d = self._X.shape
        m = self.output_dim
        lib, ctx = _ffi.load(), self._context()
        self._resident.forget("paths")
        _ffi.check(lib.bocf_set_paths(ctx.handle, -1, None, None, None, None, F, 0), "bocf_set_paths")     # (the paths of an earlier draw are gone)
        order, counts = [], {}
        for g in sorted(set(dev.tolist())):
            mine = np.flatnonzero(dev == g)
            S = mine.size
            om, ph, w, E = np.empty((m, F, d)), np.empty((m, F)), np.empty((m, F, S)), np.empty((m, N, S))
            for j in range(m):
                z = np.random.normal(size=(F, d))
                nu = {_ffi.KERN_MATERN52: 2.5, _ffi.KERN_MATERN32: 1.5}.get(int(kids[g * m + j]))
                if nu is not None:
                    z = z / np.sqrt(np.random.chisquare(2.0 * nu, size=F) / (2.0 * nu))[:, None]
                om[j] = z
                ph[j] = np.random.uniform(0.0, 2.0 * np.pi, size=F)
                w[j] = np.random.normal(size=(F, S))
                E[j] = np.random.normal(size=(N, S))
            _ffi.check(lib.bocf_set_paths(ctx.handle, int(g), _ffi.dptr(om), _ffi.dptr(ph), _ffi.dptr(w), _ffi.dptr(E), F, S), "bocf_set_paths")
            order += mine.tolist()
            counts[int(g)] = S
        self._resident.paths = {"serial": self._fit_serial, "n": n_paths, "features": F, "groups": groups, "order": np.asarray(order, dtype=int),
                                "counts": counts}

    def _paths(self):
        rec = self._resident.paths
        if rec is None or rec["serial"] != self._fit_serial:
            raise RuntimeError("no paths resident for this fit: call draw_paths")
        return rec

    def _path_values(self, rec, keep_out):
        """One bocf_path_values call per hyper-sample with paths, at the resident candidates; (m, n, P) in path order, or None."""
        n = self._resident.candidates
        out = np.empty((self.output_dim, n, rec["n"])) if keep_out else None
        at = 0
        for g in sorted(rec["counts"]):
            S = rec["counts"][g]
            blk = np.empty((self.output_dim, n, S)) if keep_out else None
            _ffi.check(_ffi.load().bocf_path_values(self._context().handle, g, _ffi.dptr(blk)), "bocf_path_values")
            if keep_out:
                out[:, :, rec["order"][at:at + S]] = blk
            at += S
        return out

    def path_values(self, X):
        """The resident paths at X (n, d): (m, n, n_paths), [j, i, s] = f_js(X_i) (target mean included)."""
        rec = self._paths()
        self._set_candidates(np.atleast_2d(X))
        return self._path_values(rec, True)

    def path_utility(self, X, row_path, thetas, utility, grad=False):
        """u_i = U(thetas[row_path[i]], f_{., row_path[i]}(X_i)) for the rows of X (n, d), each on ONE resident path (bocf_path_utility);
        thetas (n_paths, theta_dim), one row per path.  Returns u (n,), or (u (n,), du/dX (n, d)) with grad=True."""
        rec = self._paths()
        thetas = _ffi.f64(np.asarray(thetas, dtype=float).reshape(rec["n"], -1))
        rows = np.asarray(row_path, dtype=int).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= rec["n"]):
            raise IndexError("row_path out of range (0 .. n_paths - 1)")
        kind, params = self._device_utility(utility)
        n = self._set_candidates(np.atleast_2d(X))
        if n != rows.size:
            raise ValueError("row_path must hold one path index per row of X")
        inv = np.empty(rec["n"], dtype=int)
        inv[rec["order"]] = np.arange(rec["n"])                 # path s -> the device's path number
        dev_rows = np.ascontiguousarray(inv[rows], dtype=np.int32)
        pa, n_pa, th, tdim, _, _ = self._utility_args(params, thetas[rec["order"]], None)
        val = np.empty(n)
        dval = np.empty((n, self._X.shape[1])) if grad else None
        if n:
            _ffi.check(_ffi.load().bocf_path_utility(self._context().handle, kind, pa, n_pa, th, tdim, rec["n"],
                                                     dev_rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _ffi.dptr(val), _ffi.dptr(dval)),
                       "bocf_path_utility")
        return (val, dval) if grad else val

    def pathwise_topk(self, X, thetas, path_groups, utility, k):
        """The twin of thompson_topk on the resident paths of draw_paths: path s (of hyper-sample path_groups[s], which must be the
        hyper-sample it was drawn for) ranks the candidate set X (C, d) by U(thetas[s], f_s(c)).  One value call per hyper-sample used,
        one selection call; no C x C covariance, so C is not capped by it.  Returns (idx (P, k), val (P, k)) in path order, value
        descending, ties to the lowest index."""
        rec = self._paths()
        path_groups = np.asarray(path_groups, dtype=int)
        if path_groups.shape != rec["groups"].shape or np.any(path_groups != rec["groups"]):
            raise ValueError("path_groups are not the hyper-samples the resident paths were drawn for (draw_paths)")
        P = rec["n"]
        thetas = _ffi.f64(np.asarray(thetas, dtype=float).reshape(P, -1))
        kind, params = self._device_utility(utility)
        self._set_candidates(X)
        self._path_values(rec, False)
        return self._select_paths(kind, params, thetas, rec["order"], k)

    def set_hyperparameters2(self, hyperparameters):
        """multi_outputGP.py:118-120: per-output hyper-sample indices; the device keeps hyper-samples aligned across
        outputs (sample h of every output forms model h), so only a common index is supported."""
        idx = {int(h) for h in hyperparameters}
        if len(idx) != 1:
            raise NotImplementedError("per-output hyper-sample indices must be equal on the device path")
        self.set_hyperparameters(idx.pop())

    def get_hyperparameters_samples(self, n_samples=1):
        """multi_outputGP.py:123-128 -> gpmodel.py: the retained HMC draws, [sample][output] -> unfixed parameters."""
        if self.fixed_hyps or self.hmc_samples is None:
            return [[None] * self.output_dim for _ in range(n_samples)]
        return [[self.hmc_samples[j][i].copy() for j in range(self.output_dim)] for i in range(min(n_samples, self._H))]

    # ---- inspection ----------------------------------------------------------------------------
    def get_factor(self, j):
        """(L lower (N, N), alpha (N,)) of output j -- Posterior.woodbury_chol / woodbury_vector."""
        self._ensure_fitted()
        N = self._X.shape[0]
        L, a = np.empty((N, N)), np.empty(N)
        _ffi.check(_ffi.load().bocf_get_factor(self._context().handle, self._current_h * self.output_dim + j, _ffi.dptr(L), _ffi.dptr(a)),
                   "bocf_get_factor")
        return L, a

    def log_likelihood(self):
        """Log marginal likelihood per output (GP.log_likelihood, gp.py:262-266), (m,)."""
        self._ensure_fitted()
        return self.log_marginal[self._rows()].copy()

    def log_likelihood_gradients(self):
        """d log-marginal / d (kernel variance (m,), lengthscales (m, d), noise variance (m,)) of the current fit --
        what GP.parameters_changed leaves in kern.variance.gradient / kern.lengthscale.gradient /
        likelihood.variance.gradient (gp.py:256-258), in raw (untransformed) parameters.  For an isotropic
        kernel sum the lengthscale gradients over d."""
        self._ensure_fitted()
        m, d = self.output_dim * self._H, self._X.shape[1]
        dv, dl, dn = np.empty(m), np.empty((m, d)), np.empty(m)
        _ffi.check(_ffi.load().bocf_lml_gradients(self._context().handle, _ffi.dptr(dv), _ffi.dptr(dl), _ffi.dptr(dn)), "bocf_lml_gradients")
        return dv[self._rows()], dl[self._rows()], dn[self._rows()]

    def get_train_kernel(self, j):
        self._ensure_fitted()
        N = self._X.shape[0]
        K = np.empty((N, N))
        _ffi.check(_ffi.load().bocf_get_train_kernel(self._context().handle, self._current_h * self.output_dim + j, _ffi.dptr(K)),
                   "bocf_get_train_kernel")
        return K

    def get_model_parameters(self):
        """multi_outputGP.py:333-339: per output [variance, lengthscale..., noise]."""
        _, var, ls, noise = self._hyper_arrays()
        r = self._rows()
        var, ls, noise = var[r], ls[r], noise[r]
        return [np.atleast_2d(np.concatenate(([var[j]], ls[j], [noise[j]]))) for j in range(self.output_dim)]

    def get_model_parameters_names(self):
        d = self._X.shape[1]
        names = ["variance"] + ["lengthscale_%d" % q for q in range(d)] + ["Gaussian_noise.variance"]
        return [list(names) for _ in range(self.output_dim)]

    # ---- fused acquisition entry points used by bocf_amd.acquisitions ---------------------------
    def _begin_acq(self, n_hyps, own_best):
        """The reference's h-loop (maEI.py:85-97, uEI_noiseless.py:71-82) runs inside the device call: tell it how many
        hyper-samples to average (n_hyps_samples = min(10, number_of_hyps_samples())) and whose best-so-far to use --
        each hyper-sample's own (maEI.py:88) or the one that is current on entry (uEI_noiseless.py:66) -- and leave the
        model on the loop's last hyper-sample as set_hyperparameters(h) does."""
        self._ensure_fitted()
        if self.fixed_hyps:
            return
        n_h = self._H if n_hyps is None else max(1, min(int(n_hyps), self._H))
        ctx = self._context()
        ctx.set_option("acq_hyper_samples", n_h)
        ctx.set_option("best_group", -1 if own_best else self._current_h)
        self._current_h = n_h - 1

    @staticmethod
    def _utility_args(util_params, thetas, prob):
        """The utility block of the library's argument lists, in their order: (params, n_util_params, thetas, theta_dim, prob, L) from
        util_params (any shape or None), thetas (L, theta_dim) (None: L = 1, theta_dim = 0) and the weights prob (L,) or None.  The
        pointers keep their arrays alive."""
        params = None if util_params is None else _ffi.f64(np.atleast_1d(util_params))
        th = None if thetas is None else _ffi.f64(np.atleast_2d(thetas))
        L, tdim = (1, 0) if th is None else th.shape
        prob = None if prob is None else _ffi.f64(np.atleast_1d(prob))
        return _ffi.dptr(params), 0 if params is None else params.size, _ffi.dptr(th), tdim, _ffi.dptr(prob), L

    def _run_acq(self, name, head, X, util_params, thetas, prob, W, grad, fetch, tail=None):
        """The tail the acquisition entry points share: W (S, output_dim) goes up when given, X (n, d) becomes the resident candidates,
        then `name`(handle, *head, the utility block, *tail(), acq, dacq) runs unless n = 0 (`tail` checks and returns the arguments
        behind the block).  Returns acq (n,) (None with fetch=False), or (acq, dacq (n, d)) with grad=True."""
        def middle():
            extra = tail() if tail else ()
            return (*head, *self._utility_args(util_params, thetas, prob), *extra)
        return self._call_acq(name, middle, X, W, grad, fetch)

    def _call_acq(self, name, middle, X, W, grad, fetch):
        """W (S, output_dim) goes up when given, X (n, d) becomes the resident candidates, then `name`(handle, *middle(), acq, dacq) runs
        unless n = 0.  Returns acq (n,) (None with fetch=False), or (acq, dacq (n, d)) with grad=True."""
        if W is not None:
            self.set_mc_samples(W)
        n = self._set_candidates(np.atleast_2d(X))
        args = middle()
        acq = np.empty(n) if fetch else None
        dacq = np.empty((n, self._X.shape[1])) if grad else None
        if n:
            _ffi.check(getattr(_ffi.load(), name)(self._context().handle, *args, _ffi.dptr(acq), _ffi.dptr(dacq)), name)
        return (acq, dacq) if grad else acq

    REFINE_POLL_EVERY = 8      # passes between two reads of the running-rows word (the sweep is in DESIGN.md section 19)

    def refine_acq(self, X0, bounds, form, kind=_ffi.ACQ_EI, util_kind=_ffi.UTIL_LINEAR, util_params=None, thetas=None, prob=None, W=None,
                   n_hyps=None, program=None, maxiter=500, m=10, factr=1e6, pgtol=1e-5, max_ls=20, c1=1e-4, maxfun=None, poll_every=None):
        """Refine the rows of X0 (A <= 64, d) inside the box `bounds` with the loop on the device (bocf_refine_acq): minimises -acq of
        form _ffi.REFINE_LINEAR (closed-form EI / PI `kind` of theta . f, as acq_linear_grad) or _ffi.REFINE_MC (Monte-Carlo EI of the
        utility block, as acq_mc_grad; W and a program go up as there) with the algorithm and settings of lbfgsb_batched.  Returns
        (X (A, d), F (A,) = -acq there, info): iterations, evaluations and reasons (names of _ffi.REFINE_REASONS) per row, passes,
        points_evaluated, host_syncs.  Afterwards no candidates and no acquisition vector are resident."""
        self._begin_acq(n_hyps, form == _ffi.REFINE_LINEAR)
        if form == _ffi.REFINE_MC:
            if util_kind == _ffi.UTIL_PROGRAM:
                self.set_utility_program(program)
            if W is not None:
                self.set_mc_samples(W)
        X0 = _ffi.f64(np.atleast_2d(X0))
        A, d = X0.shape
        if d != self._X.shape[1]:
            raise ValueError("starts must be (A, %d)" % self._X.shape[1])
        lo = _ffi.f64([b[0] for b in bounds])
        hi = _ffi.f64([b[1] for b in bounds])
        if lo.shape != (d,):
            raise ValueError("bounds must be %d (lo, hi) pairs" % d)
        if form == _ffi.REFINE_LINEAR and (thetas is None or np.atleast_2d(thetas).shape[1] != self.output_dim):
            raise ValueError("theta must have output_dim entries")     # (the library reads L rows of output_dim doubles)
        util = self._utility_args(util_params, thetas, prob)
        X, F = np.empty((A, d)), np.empty(A)
        iters, nfun, reason = (np.zeros(A, dtype=np.int32) for _ in range(3))
        counters = (ctypes.c_longlong * 2)()
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        self._resident.forget("candidates")                # the batch and its acquisition vector are the loop's from here on
        _ffi.check(_ffi.load().bocf_refine_acq(self._context().handle, int(form), int(kind), int(util_kind), *util, _ffi.dptr(X0), A, _ffi.dptr(lo),
                                               _ffi.dptr(hi), int(maxiter), int(m), float(factr), float(pgtol), int(max_ls), float(c1),
                                               -1 if maxfun is None else int(maxfun), int(self.REFINE_POLL_EVERY if poll_every is None else poll_every),
                                               _ffi.dptr(X), _ffi.dptr(F), ip(iters), ip(nfun), ip(reason), counters), "bocf_refine_acq")
        info = dict(iterations=iters.astype(int), evaluations=nfun.astype(int), reasons=[_ffi.REFINE_REASONS[r] for r in reason],
                    passes=int(counters[0]), f_df_calls=int(counters[0]), points_evaluated=int(nfun.sum()), host_syncs=int(counters[1]))
        return X, F, info

    def _device_utility(self, utility):
        """(kind, params) of a Utility for the device; a utility program is staged."""
        kind = utility.device_kind(self.output_dim)
        if kind == _ffi.UTIL_PROGRAM:
            self.set_utility_program(utility.program_blob)
        return kind, utility.device_params

    def _resident_for_fit(self, slot, message):
        """The key of the resident `slot`, which ends in the serial of the fit it was staged for: the current one, or RuntimeError."""
        key = getattr(self._resident, slot)
        if key is None or key[-1] != self._fit_serial:
            raise RuntimeError(message)
        return key

    def _acq_linear(self, X, kind, thetas, prob, n_hyps, grad):
        self._begin_acq(n_hyps, True)
        n = self._set_candidates(np.atleast_2d(X))
        thetas = _ffi.f64(np.atleast_2d(thetas))
        if thetas.shape[1] != self.output_dim:
            raise ValueError("theta must have output_dim entries")
        prob = None if prob is None else _ffi.f64(np.atleast_1d(prob))
        acq = np.empty(n)
        dacq = np.empty((n, self._X.shape[1])) if grad else None
        what = "bocf_acq_linear_grad" if grad else "bocf_acq_linear"
        out = (_ffi.dptr(acq), _ffi.dptr(dacq)) if grad else (_ffi.dptr(acq),)
        if n:
            _ffi.check(getattr(_ffi.load(), what)(self._context().handle, kind, _ffi.dptr(thetas), _ffi.dptr(prob), thetas.shape[0], *out), what)
        return (acq, dacq) if grad else acq

    def acq_linear(self, X, kind, thetas, prob, n_hyps=None):
        """Closed-form EI/PI of theta.f over the batch X on the device (bocf_acq_linear)."""
        return self._acq_linear(X, kind, thetas, prob, n_hyps, False)

    def acq_linear_grad(self, X, kind, thetas, prob, n_hyps=None):
        """(acq (n,), d acq/dX (n, d)) of the closed-form EI/PI (bocf_acq_linear_grad)."""
        return self._acq_linear(X, kind, thetas, prob, n_hyps, True)

    def set_utility_program(self, blob):
        """Stage a utility program (the blob of utility_program.Program.to_bytes(), Utility.program_blob) on the device for the calls
        with utility kind _ffi.UTIL_PROGRAM; it stays resident until another one is set.  Key-cached like set_mc_samples: an L-BFGS
        run sends the same program hundreds of times."""
        if blob is None:
            raise ValueError("utility kind 'program' needs the program blob (Utility(..., device='program').program_blob)")
        blob = bytes(blob)
        if blob == self._resident.program:
            return
        _ffi.check(_ffi.load().bocf_set_utility_program(self._context().handle, blob, len(blob)), "bocf_set_utility_program")
        self._resident.program = blob

    def acq_mc_grad(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, program=None):
        """(acq (n,), d acq/dX (n, d)) of the Monte-Carlo EI (bocf_acq_mc_grad); `program`: the blob for utility kind UTIL_PROGRAM."""
        self._begin_acq(n_hyps, False)
        if util_kind == _ffi.UTIL_PROGRAM:
            self.set_utility_program(program)
        return self._run_acq("bocf_acq_mc_grad", (util_kind,), X, util_params, thetas, prob, W, True, True)

    def set_mc_samples(self, W):
        self._ensure_fitted()
        W = _ffi.f64(np.atleast_2d(W))
        if W.shape[1] != self.output_dim:
            raise ValueError("W must be (S, output_dim)")
        key = (W.shape, hash(W.tobytes()))
        if key == self._resident.W:       # the same common random numbers are already resident (L-BFGS calls f_df hundreds of times)
            return
        _ffi.check(_ffi.load().bocf_set_mc_samples(self._context().handle, _ffi.dptr(W), W.shape[0]), "bocf_set_mc_samples")
        self._resident.W = key

    def acq_mc(self, X, kind, util_kind, util_params, thetas, prob, W=None, fetch=True, n_hyps=None, program=None):
        """Monte-Carlo EI/PI of a device utility over the batch X (bocf_acq_mc); `program`: the blob for utility kind UTIL_PROGRAM."""
        self._begin_acq(n_hyps, False)
        if util_kind == _ffi.UTIL_PROGRAM:
            self.set_utility_program(program)
        if W is not None:
            self.set_mc_samples(W)
        n = self._set_candidates(np.atleast_2d(X)) if X is not None else None
        return self._acq_mc_resident(kind, util_kind, util_params, thetas, prob, n, fetch)

    def _acq_mc_resident(self, kind, util_kind, util_params, thetas, prob, n, fetch=True):
        util = self._utility_args(util_params, thetas, prob)
        acq = np.empty(n) if (fetch and n is not None) else None
        if n is None or n > 0:
            _ffi.check(_ffi.load().bocf_acq_mc(self._context().handle, kind, util_kind, *util, _ffi.dptr(acq)), "bocf_acq_mc")
        return acq

    def set_eu_samples(self, Z):
        """Upload the Monte-Carlo normals of the recommendation step, Z (L, S, output_dim): block l is the np.random.normal(size=(S, m))
        the reference draws for parameter l (cbo.py:200).  Key-cached like set_mc_samples: an L-BFGS run re-sends the same Z."""
        self._ensure_fitted()
        Z = _ffi.f64(Z)
        if Z.ndim == 2:
            Z = Z[None]
        if Z.ndim != 3 or Z.shape[2] != self.output_dim:
            raise ValueError("Z must be (L, S, output_dim)")
        key = (Z.shape, hash(Z.tobytes()))
        if key == self._resident.Z:
            return
        _ffi.check(_ffi.load().bocf_set_eu_samples(self._context().handle, _ffi.dptr(Z), Z.shape[0], Z.shape[1]), "bocf_set_eu_samples")
        self._resident.Z = key

    def expected_utility(self, X, mode, utility, thetas, row_param, Z=None, n_hyps=None, grad=False, util_params=None):
        """Posterior expected utility of the recommendation step (cbo.py:121-235) on the device, all utility parameters in one call:
        row i of X takes parameter thetas[row_param[i]] and gets

            v_i = sum_{h < n_hyps} E_h[ U(theta, f(X_i)) ]      (a sum, not a mean: cbo.py:160)

        under the noiseless posterior (predict_noiseless).  `mode`: "mean" (theta . mu, utility.linear), "closed" (the closed-form
        expectation of the device utility) or "mc" (sum over the S normals Z[row_param[i]] of U(theta, mu + sigma o Z_s)); or the
        _ffi.EU_* value.  `utility`: a Utility with a device kind, a device utility name or its _ffi.UTIL_* value (ignored in "mean"
        mode); `util_params` overrides utility.device_params.  Z (L, S, m) is needed in "mc" mode (cached on the device).
        X = None evaluates the candidates already resident (the last batch of any device call); row_param must then hold exactly
        one index per resident candidate (ValueError otherwise).
        n_hyps: hyper-samples to sum (default min(10, number_of_hyps_samples())); more than are resident is an IndexError; with fixed
        hyper-parameters the one resident sample counts n_hyps times, as the reference's identical passes do.  thetas must be 2-D.  Leaves the model on hyper-sample n_hyps - 1, as the
        reference's set_hyperparameters(h) loop does.  Returns v (n,), or (v (n,), dv/dX (n, d)) with grad=True."""
        mode = _ffi.eu_mode(mode)
        self._ensure_fitted()
        if hasattr(utility, "device_kind"):
            kind = 0 if mode == _ffi.EU_MEAN else utility.device_kind(self.output_dim)
            if util_params is None:
                util_params = utility.device_params
            if kind == _ffi.UTIL_PROGRAM and mode == _ffi.EU_MC:
                self.set_utility_program(utility.program_blob)
        elif isinstance(utility, str):
            kind = device_utility(utility).kind
        else:
            kind = 0 if utility is None else int(utility)
        n_h = min(10, self.number_of_hyps_samples()) if n_hyps is None else int(n_hyps)
        if n_h < 1:
            raise ValueError("n_hyps must be >= 1")
        if not self.fixed_hyps and n_h > self._H:
            # the reference's set_hyperparameters(h) loop would fail on h >= H: no silent clamping
            raise IndexError("n_hyps = %d exceeds the %d resident hyper-samples" % (n_h, self._H))
        th = _ffi.f64(thetas)
        if th.ndim != 2:
            raise ValueError("thetas must be 2-D (L, theta_dim); write L scalar parameters as an (L, 1) array")
        rows = np.ascontiguousarray(np.asarray(row_param).reshape(-1), dtype=np.int32)
        if mode == _ffi.EU_MC:
            if Z is None:
                raise ValueError("the Monte-Carlo mode needs Z (L, S, output_dim)")
            self.set_eu_samples(Z)
        if X is not None:
            n = self._set_candidates(np.atleast_2d(X))
            if n != rows.size:
                raise ValueError("row_param must hold one parameter index per row of X")
        elif self._resident.candidates is None or self._resident.candidates != rows.size:
            # the library reads row_param and writes the outputs for every RESIDENT candidate: the sizes must agree
            raise ValueError("X = None evaluates the resident candidates (%s): row_param must hold one index per candidate, it holds %d"
                             % ("none known" if self._resident.candidates is None else self._resident.candidates, rows.size))
        n = rows.size
        params, n_params, th, tdim, _, L = self._utility_args(util_params, th, None)
        val = np.empty(n)
        dval = np.empty((n, self._X.shape[1])) if grad else None
        if n:
            _ffi.check(_ffi.load().bocf_expected_utility(self._context().handle, mode, kind, params, n_params, th, tdim, L,
                                                         rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n_h, _ffi.dptr(val), _ffi.dptr(dval)),
                       "bocf_expected_utility")
        if not self.fixed_hyps:
            self._current_h = min(n_h, self._H) - 1
        return (val, dval) if grad else val

    # ---- feasibility-aware recommendation: the constrained expected utility -----------------------------------
    def _device_kind(self, utility):
        """(kind, device params or None) of a Utility with a device kind, a device utility name or its _ffi.UTIL_* value."""
        if hasattr(utility, "device_kind"):
            return utility.device_kind(self.output_dim), utility.device_params
        if isinstance(utility, str):
            return device_utility(utility).kind, None
        return int(utility), None

    def train_utility_range(self, kind, util_params, thetas):
        """(min (L,), max (L,)) of U(theta_l, mu(X_i)) over all training points (bocf_train_utility_range); the posterior mean is that of
        the current hyper-sample.  `kind`: as `utility` in expected_utility_constrained.  The min is the recommendation step's default
        worth of an infeasible outcome."""
        self._ensure_fitted()
        if not self.fixed_hyps:
            self._context().set_option("best_group", self._current_h)
        kind, own = self._device_kind(kind)
        params, n_params, th, tdim, _, L = self._utility_args(own if util_params is None else util_params, thetas, None)
        lo, hi = np.empty(L), np.empty(L)
        _ffi.check(_ffi.load().bocf_train_utility_range(self._context().handle, kind, params, n_params, th, tdim, L, _ffi.dptr(lo), _ffi.dptr(hi)),
                   "bocf_train_utility_range")
        return lo, hi

    def expected_utility_constrained(self, X, utility, thetas, row_param, u_infeasible, Z, n_hyps=None, grad=False, util_params=None):
        """The constrained expected utility of the recommendation step on the device (bocf_expected_utility_constrained), all utility
        parameters in one call: row i of X takes parameter thetas[row_param[i]], its normals Z[row_param[i]] and the worth
        u_infeasible[row_param[i]] of an infeasible outcome, and gets

            v_i   = sum_{h < n_hyps} sum_s [ u0 + phi(y_s) (U(theta, y_s) - u0) ],   y_s = mu_h + sigma_h o Z_s      (a sum, as expected_utility's)
            pof_i = mean over h and s of phi(y_s)                                     (smoothed probability of feasibility)

        under the noiseless posterior, phi from the resident constraints (set_output_constraints).  `utility`: a Utility with a compiled-in
        device kind, a device utility name or its _ffi.UTIL_* value (a utility program is refused); u_infeasible: a scalar or (L,); Z
        (L, S, m).  X = None, n_hyps and the hyper-sample the model is left on: as in expected_utility.  Returns (v (n,), pof (n,)), or
        (v, pof, dv/dX (n, d)) with grad=True; pof has no gradient."""
        self._ensure_fitted()
        self._constraints_resident()
        kind, own = self._device_kind(utility)
        if util_params is None:
            util_params = own
        n_h = min(10, self.number_of_hyps_samples()) if n_hyps is None else int(n_hyps)
        if n_h < 1:
            raise ValueError("n_hyps must be >= 1")
        if not self.fixed_hyps and n_h > self._H:
            raise IndexError("n_hyps = %d exceeds the %d resident hyper-samples" % (n_h, self._H))
        th = _ffi.f64(thetas)
        if th.ndim != 2:
            raise ValueError("thetas must be 2-D (L, theta_dim); write L scalar parameters as an (L, 1) array")
        u0 = _ffi.f64(np.broadcast_to(np.asarray(u_infeasible, dtype=float), (th.shape[0],)))
        rows = np.ascontiguousarray(np.asarray(row_param).reshape(-1), dtype=np.int32)
        if Z is None:
            raise ValueError("the constrained expected utility needs Z (L, S, output_dim)")
        self.set_eu_samples(Z)
        if X is not None:
            n = self._set_candidates(np.atleast_2d(X))
            if n != rows.size:
                raise ValueError("row_param must hold one parameter index per row of X")
        elif self._resident.candidates is None or self._resident.candidates != rows.size:
            raise ValueError("X = None evaluates the resident candidates (%s): row_param must hold one index per candidate, it holds %d"
                             % ("none known" if self._resident.candidates is None else self._resident.candidates, rows.size))
        n = rows.size
        params, n_params, th, tdim, _, L = self._utility_args(util_params, th, None)
        val, pof = np.empty(n), np.empty(n)
        dval = np.empty((n, self._X.shape[1])) if grad else None
        if n:
            _ffi.check(_ffi.load().bocf_expected_utility_constrained(self._context().handle, kind, params, n_params, th, tdim, L, _ffi.dptr(u0),
                                                                     rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n_h, _ffi.dptr(val),
                                                                     _ffi.dptr(pof), _ffi.dptr(dval)), "bocf_expected_utility_constrained")
        if not self.fixed_hyps:
            self._current_h = min(n_h, self._H) - 1
        return (val, pof, dval) if grad else (val, pof)

    # ---- leave-one-out cross-validation of the resident model ------------------------------------------------
    def _loo(self, flags, mean=False, var=False, lpd=False, total=False):
        """One bocf_loo over all H * m factorizations; only the arrays asked for are transferred (None for the others)."""
        self._ensure_fitted()
        M, N = self.output_dim * self._H, self._X.shape[0]
        out = [np.empty((M, N)) if want else None for want in (mean, var, lpd)] + [np.empty(M) if total else None]
        _ffi.check(_ffi.load().bocf_loo(self._context().handle, flags, *[_ffi.dptr(a) for a in out]), "bocf_loo")
        return out

    def _loo_rows(self, a, all_hyper_samples):
        if all_hyper_samples:
            return a.reshape((self._H, self.output_dim) + a.shape[1:])
        return a[self._rows()].copy()

    def loo(self, noiseless=False, all_hyper_samples=False):
        """Leave-one-out predictions at the training points from the resident factor (ExactGaussianInference.LOO,
        exact_gaussian_inference.py:67-79, and the predictive moments its densities are made of): (mean, var, lpd), each (m, N) -- point i
        predicted by the model of the other N - 1 points, hyper-parameters and the targets' centre held.  The variance includes the
        likelihood noise unless `noiseless` and is clipped at 1e-10 (as predict / predict_noiseless); lpd is the log density of y_i under
        the prediction with noise, whatever `noiseless`.  The current hyper-sample answers; all_hyper_samples=True gives (H, m, N) each."""
        flags = _ffi.CLIP | (0 if noiseless else _ffi.ADD_NOISE)
        mean, var, lpd, _ = self._loo(flags, mean=True, var=True, lpd=True)
        return tuple(self._loo_rows(a, all_hyper_samples) for a in (mean, var, lpd))

    def loo_log_likelihood(self, all_hyper_samples=False):
        """Leave-one-out log pseudo-likelihood sum_i lpd_i per output: (m,), or (H, m).  Only the sums leave the device."""
        return self._loo_rows(self._loo(_ffi.ADD_NOISE | _ffi.CLIP, total=True)[3], all_hyper_samples)

    @staticmethod
    def loo_summary_of(Y, mean, var, lpd):
        """The summary of leave-one-out results Y, mean, var (with noise), lpd, each (m, N): per output the pseudo-likelihood `lpd`, the
        `rmse` of the mean, mean `z_mean` and variance `z_var` of the standardised residuals z = (y - mean) / sqrt(var), and the share
        `coverage` of |z| <= 1.96 (0.95 for a calibrated model)."""
        Y, mean, var, lpd = (np.asarray(a, dtype=float) for a in (Y, mean, var, lpd))
        z = (Y - mean) / np.sqrt(var)
        return {"lpd": lpd.sum(1), "rmse": np.sqrt(np.mean((Y - mean) ** 2, 1)), "z_mean": z.mean(1), "z_var": z.var(1),
                "coverage": np.mean(np.abs(z) <= 1.96, 1)}

    def loo_summary(self):
        """loo_summary_of the current hyper-sample's leave-one-out predictions: a dict of (m,) arrays."""
        mean, var, lpd = self.loo()
        return self.loo_summary_of(np.stack([y[:, 0] for y in self._Y], 0), mean, var, lpd)

    def loo_utility(self, utility, parameters=None, noiseless=False, Z=None, n_samples=50):
        """The cross-validated composite prediction: (predicted (L, N), observed (L, N)) with predicted[l, i] = E[U(theta_l, y)] under the
        leave-one-out prediction of training point i (bocf_loo_utility, current hyper-sample; with the likelihood noise unless
        `noiseless`) and observed[l, i] = U(theta_l, y_i) from the utility's host callable.  `parameters` (L, theta_dim) defaults to the
        support of utility.parameter_dist.  The expectation takes the form the recommendation step takes for this utility: the mean for a
        linear one, the closed form where the device has one, else the mean over the normals Z (L, S, m) (default: n_samples draws per
        parameter from np.random.normal).  A utility outside the device set raises NotImplementedError: there is no host fallback."""
        from .utility import device_thetas, inner_expectation
        m = self.output_dim
        mode, kind = inner_expectation(utility, m)           # (raises before anything touches the device)
        self._ensure_fitted()
        N = self._X.shape[0]
        if parameters is None:
            parameters = getattr(utility.parameter_dist, "support", None)
            if parameters is None:
                raise ValueError("the utility's parameter distribution has no support: give `parameters`")
        parameters = np.asarray(parameters, dtype=float).reshape(len(parameters), -1)
        L = parameters.shape[0]
        if kind == _ffi.UTIL_PROGRAM:
            self.set_utility_program(utility.program_blob)
        if mode == _ffi.EU_MC:
            self.set_eu_samples(np.random.normal(size=(L, int(n_samples), m)) if Z is None else Z)
        params, n_params, th, tdim, _, _ = self._utility_args(utility.device_params, device_thetas(kind, parameters), None)
        predicted = np.empty((L, N))
        flags = _ffi.CLIP | (0 if noiseless else _ffi.ADD_NOISE)
        _ffi.check(_ffi.load().bocf_loo_utility(self._context().handle, self._current_h, flags, mode, kind, params, n_params, th, tdim, L,
                                                _ffi.dptr(predicted)), "bocf_loo_utility")
        Y = np.stack([y[:, 0] for y in self._Y], 0)
        observed = np.array([[float(np.squeeze(utility.func(parameters[l], Y[:, i]))) for i in range(N)] for l in range(L)])
        return predicted, observed

    def loo_compare(self, kernel_lists):
        """Score F candidate kernel lists (each one kernel per output, hyper-parameters as given) on the current data: the (F, m) tables
        (leave-one-out log pseudo-likelihood, log marginal likelihood).  The F x m models are fitted as F groups of m outputs in ONE
        bocf_fit on a context of their own -- the resident model is not touched.  Fixed hyper-parameters only (ValueError otherwise:
        learned ones would have to be re-learned per family)."""
        if not self.fixed_hyps:
            raise ValueError("loo_compare / select_kernels compare kernels at fixed hyper-parameters (fixed_hyps=True)")
        if self._X is None:
            raise RuntimeError("updateModel has not been called")
        kernel_lists = [list(kl) for kl in kernel_lists]
        F, m = len(kernel_lists), self.output_dim
        if F < 1 or any(len(kl) != m for kl in kernel_lists):
            raise ValueError("kernel_lists must hold lists of output_dim kernels")
        N, d = self._X.shape
        specs = [kernel_spec(k, d) for kl in kernel_lists for k in kl]
        kids = [int(s[0]) for s in specs]
        var, ls = _ffi.f64([s[1] for s in specs]), _ffi.f64([s[2] for s in specs])
        noise = _ffi.f64(np.tile([1e-10 if nv is None else float(nv) for nv in self.noise_var], F))
        Y = _ffi.f64(np.tile(np.stack([y[:, 0] for y in self._Y], 0), (F, 1)))
        lib, ctx = _ffi.load(), _ffi.Context(self.device)
        try:
            ctx.set_option("hyper_samples", F)
            if len(set(kids)) > 1:
                _ffi.check(lib.bocf_set_kernel_ids(ctx.handle, (ctypes.c_int * len(kids))(*kids), len(kids)), "bocf_set_kernel_ids")
            jit, lml, loo = np.zeros(F * m), np.zeros(F * m), np.zeros(F * m)
            rc = _ffi.check(lib.bocf_fit(ctx.handle, _ffi.dptr(self._X), _ffi.dptr(Y), N, d, F * m, kids[0], _ffi.dptr(var), _ffi.dptr(ls),
                                         _ffi.dptr(noise), 5, _ffi.dptr(jit), _ffi.dptr(lml)), "bocf_fit")
            if rc > 0:
                raise np.linalg.LinAlgError("not positive definite, even with jitter.")
            _ffi.check(lib.bocf_loo(ctx.handle, _ffi.ADD_NOISE | _ffi.CLIP, None, None, None, _ffi.dptr(loo)), "bocf_loo")
        finally:
            ctx.close()
        return loo.reshape(F, m), lml.reshape(F, m)

    def select_kernels(self, kernel_lists, criterion="loo"):
        """Per output the kernel of the candidate list that scores best in loo_compare's table -- criterion "loo" (log pseudo-likelihood)
        or "lml" (log marginal likelihood); ties to the earlier list.  Returns a kernel list to build a model from."""
        if criterion not in ("loo", "lml"):
            raise ValueError("criterion must be 'loo' or 'lml'")
        kernel_lists = [list(kl) for kl in kernel_lists]
        table = self.loo_compare(kernel_lists)[0 if criterion == "loo" else 1]
        best = np.argmax(np.asarray(table), axis=0)
        return [kernel_lists[int(best[j])][j] for j in range(self.output_dim)]

    def select_topk(self, k):
        """(indices, values) of the k best candidates of the last acquisition call -- the
        np.argsort(-acq)[:k] of anchor_points_generator.py:61, ties to the lowest index.  A NaN
        value ranks as -inf (after every number, tied with -inf by index) and is reported as -inf.
        With fewer than k candidates, all of them are returned."""
        idx = np.empty(k, dtype=np.int64)
        val = np.empty(k)
        _ffi.check(_ffi.load().bocf_select_topk(self._context().handle, k, idx.ctypes.data_as(_ffi._c_ll_p), _ffi.dptr(val)),
                   "bocf_select_topk")
        keep = idx >= 0
        return idx[keep], val[keep]
