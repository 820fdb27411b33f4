"""The problem the input-dimension sweep shares (tests/test_input_dims_cpu.py, tests/test_gpu_input_dims.py): one seeded three-output
problem per input dimension d, one kernel family per output, the oracle's fit of it (computed once per shape, never modified), and the
gates the sweep applies -- the project's own, named after the tests they come from.  Test infrastructure only: nothing under bocf_amd/
imports it."""
import functools

import numpy as np

from oracle import cpu_ref as R

KINDS = ["rbf", "matern52", "matern32"]                 # one output per kernel template argument KID (rbf and se share KID 0)

# test_random_shapes: mean rtol / atol, variance |delta| <= 1e-8 max(sigma_f^2) (sigma_f^2 = 1 here)
MEAN_RTOL, MEAN_ATOL, VAR_GATE = 1e-6, 1e-7, 1e-8


def problem(d, N, C, noise):
    """ARD lengthscales 0.5 sqrt(d) (1 +- 0.2), distinct per coordinate and per output: the median off-diagonal of K stays near 0.7 for
    every d, so a high dimension does not degenerate into a diagonal matrix."""
    return R.synthetic_problem(N, d, 3, C, 8, 8800 + d, noise)


def fit_oracle(p, lengthscales=None):
    ref = R.MultiOutputGPRef(KINDS, p["variances"], p["lengthscales"] if lengthscales is None else lengthscales, p["noise"])
    ref.updateModel(p["X"], p["Y"])
    return ref


@functools.lru_cache(maxsize=None)
def oracle(d, N, C, noise):
    """(problem, fitted oracle) of a small shape, shared by every test that asks for it: read-only."""
    p = problem(d, N, C, noise)
    return p, fit_oracle(p)


def mixed_model(B, p):
    """The device model of a problem: fixed hyper-parameters, KINDS[j] for output j (as _mixed_model of test_gpu_round3.py)."""
    d = p["X"].shape[1]
    cls = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
    kern = [cls[k](d, variance=p["variances"][j], lengthscale=p["lengthscales"][j], ARD=True) for j, k in enumerate(KINDS)]
    model = B.multi_outputGP(len(KINDS), kernel=kern, noise_var=list(p["noise"]), fixed_hyps=True)
    model.updateModel(p["X"], p["Y"])
    return model


def predict_once(ref, Xc):
    """MultiOutputGPRef.predict (mean, variance + noise, clipped) from ONE cross-kernel evaluation per output instead of its two: the same
    formulas (GPFit.raw_posterior_mean / raw_posterior_variance), for the loops that refit many times."""
    from scipy.linalg import lapack
    mean, var = [], []
    for f in ref.output:
        Kx = R.kern_K(f.kind, f.X, Xc, f.variance, f.lengthscale)
        tmp = lapack.dtrtrs(np.asfortranarray(f.L), Kx, lower=1)[0]
        mean.append(Kx.T.dot(f.alpha)[:, 0] + f.ymean)
        var.append(np.clip(f.variance - np.square(tmp).sum(0) + f.noise_var, 1e-10, np.inf))
    return np.stack(mean), np.stack(var)


N_ACQ = 7                                             # the acquisition gradients are checked at Xc[:7] (small path)
ACQ_PROB = np.array([0.4, 0.6])


def acquisition_reference(d, N, C, noise):
    """What the acquisition checks share, from the oracle alone: its posterior at Xc[:7] and at the evaluated points."""
    p, ref = oracle(d, N, C, noise)
    X7 = p["Xc"][:N_ACQ]
    mean, var = ref.predict(X7)
    return dict(mean=mean, var=var, dmean=ref.posterior_mean_gradient(X7), dvar=ref.posterior_variance_gradient(X7),
                mu_eval=ref.posterior_mean_at_evaluated_points())


@functools.lru_cache(maxsize=None)
def acquisition_inputs(d, N, C, noise):
    """Two support points for maEI (linear utility) and two for uEI_noiseless (neg_sq_dist) at which the ORACLE's acquisition gradient is
    non-zero in every coordinate, with its acquisition value and gradient.

    With 200 evaluated points an improvement over the best of them is rare: random supports leave expected improvement and its gradient
    at zero for most d, and a comparison of zeros checks nothing.  So the supports are placed from the oracle's own posterior at two of the
    seven candidates (i, k) -- for the linear utility the direction from the centre of the evaluated means to the candidate's mean or its
    opposite, then signed unit vectors, then seeded normal draws; for the distance utility the candidate's mean itself, or that mean moved
    by +-0.05 -- and the first support, in that fixed order, whose oracle gradient exceeds 1e-4 (10^4 x the absolute tolerance of the comparison) in every coordinate is taken.  The device never enters the
    choice.  Returns dict(ma=(support, acq, dacq), mc=(support, acq, dacq))."""
    import itertools
    r = acquisition_reference(d, N, C, noise)
    p = problem(d, N, C, noise)
    mu, centre = r["mean"], r["mu_eval"].mean(1)
    sigma = np.sqrt(r["var"])

    def ok(a, da):
        return a.max() >= 1e-6 and np.abs(da).max(0).min() >= 1e-4

    pairs = list(itertools.combinations(range(N_ACQ), 2))
    unit, rng = np.eye(len(KINDS)), np.random.RandomState(8800 + d)
    linear = ([s * np.stack([mu[:, i] - centre, mu[:, k] - centre]) for i, k in pairs for s in (1.0, -1.0)]
              + [np.stack([s * unit[a], t * unit[b]]) for a in range(3) for b in range(3) for s in (1.0, -1.0) for t in (1.0, -1.0)]
              + [rng.normal(size=(2, len(KINDS))) for _ in range(60)])
    distance = [np.stack([mu[:, i] + off, mu[:, k] - off]) for i, k in pairs for off in (0.0, 0.05)]
    out = {}
    for th in linear:
        a, da = R.ma_acq_with_gradient(r["mean"], r["var"], r["dmean"], r["dvar"], r["mu_eval"], th, ACQ_PROB, "EI")
        if ok(a, da):
            out["ma"] = (th, a, da)
            break
    for th in distance:
        a, da = R.mc_acq_with_gradient(mu, sigma, r["dmean"], r["dvar"], r["mu_eval"], p["W"], "neg_sq_dist", th, ACQ_PROB)
        if ok(a, da):
            out["mc"] = (th, a, da)
            break
    if len(out) == 2:
        return out
    raise AssertionError("d = %d: no support gives a non-zero acquisition gradient in every coordinate (%s found)" % (d, sorted(out)))


def mean_excess(got, want):
    """How far |got - want| lies beyond the mean gate, largest over the entries (<= 0: within the gate everywhere)."""
    return float(np.max(np.abs(got - want) - (MEAN_ATOL + MEAN_RTOL * np.abs(want))))
