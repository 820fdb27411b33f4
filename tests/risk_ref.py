"""NumPy restatement of the quantile / tail-mean acquisitions of the composite utility and of the closed-form confidence bound (DESIGN.md
section 22, include/bocf_hip.h), over posterior arrays -- mean, var (m, n), their input gradients (m, n, d) -- and oracle.cpu_ref
(utility_eval, utility_grad).  Test infrastructure only: nothing under bocf_amd/ imports it.

    u_s      = U(theta_l, mu + sigma o W_s)             NaN -> -inf (in rank and in value)
    order    : stable argsort of u (value ascending, then sample index ascending; -0.0 == +0.0 as numbers)
    u_(k)    = the sample with k samples before it, s*(k) its index
    rho      = u_(k) | mean u_(k) .. u_(S-1) (S - k terms, math.fsum) | mean u_(0) .. u_(k) (k + 1 terms, math.fsum)
    alpha(x) = (1/H) sum_h sum_l p_l rho_hl(x)
    d rho/dx_q = (1/|T|) sum_{s in T} sum_j dU/dy_j(y_s) (dmu_j/dx_q + W_sj / (2 sigma_j) dvar_j/dx_q)
"""
import math

import numpy as np

from oracle import cpu_ref as R

QUANTILE, UPPER_TAIL, LOWER_TAIL = 0, 1, 2


def order(u):
    """(u with NaN -> -inf, the stable ascending order of its last axis).  np.argsort(kind="stable") compares doubles as numbers, so -0.0 and
    +0.0 tie and the index decides, as the definition says."""
    u = np.where(np.isnan(u), -np.inf, np.asarray(u, dtype=float))
    return u, np.argsort(u, axis=-1, kind="stable")


def members(S, kind, k):
    """Positions in the order that make up the selected set T."""
    if kind == QUANTILE:
        return np.arange(k, k + 1)
    return np.arange(k, S) if kind == UPPER_TAIL else np.arange(0, k + 1)


def tail_mean(v):
    """Exactly rounded sum over the count; inf - inf is NaN (math.fsum raises there)."""
    v = [float(x) for x in v]
    if any(math.isinf(x) for x in v):
        with np.errstate(invalid="ignore"):
            s = float(np.sum(np.array(v)[np.isinf(v)]))      # +inf, -inf, or NaN when both are present
    else:
        s = math.fsum(v)
    return s / len(v)


def statistic(u, kind, k):
    """rho of one sample vector u (S,), the indices T of its selected set (ascending in the order), and the smaller gap between u_(k) and
    its two neighbours in the order (inf where it has none)."""
    u, o = order(u)
    S = u.shape[0]
    assert 0 <= k < S
    T = o[members(S, kind, k)]
    rho = u[o[k]] if kind == QUANTILE else tail_mean(u[T])
    su = u[o]
    with np.errstate(invalid="ignore"):
        lo = su[k] - su[k - 1] if k > 0 else np.inf
        hi = su[k + 1] - su[k] if k < S - 1 else np.inf
    gap = np.nanmin([lo, hi]) if not (np.isnan(lo) and np.isnan(hi)) else 0.0
    return rho, T, gap


def risk(mean, var, W, thetas, prob, util, params, kind, k, dmean=None, dvar=None):
    """alpha of the n candidates of one hyper-sample.  Returns a dict: alpha (n,), gap (n, L) (see statistic), scale (n,) = max_s |u_s| over
    the finite samples of every theta, and with dmean / dvar the gradient dalpha (n, d)."""
    mean, var, W = np.asarray(mean, dtype=float), np.asarray(var, dtype=float), np.atleast_2d(W)
    thetas = np.atleast_2d(thetas)
    m, n = mean.shape
    S, L = W.shape[0], thetas.shape[0]
    p = np.full(L, 1.0 / L) if prob is None else np.asarray(prob, dtype=float)
    sg = np.sqrt(var)
    with np.errstate(invalid="ignore", over="ignore"):
        y = mean[:, None, :] + sg[:, None, :] * W.T[:, :, None]              # (m, S, n)
    grad = dmean is not None
    alpha, gap, scale = np.zeros(n), np.zeros((n, L)), np.zeros(n)
    dalpha = np.zeros((n, dmean.shape[2])) if grad else None
    for l, th in enumerate(thetas):
        with np.errstate(invalid="ignore", over="ignore"):
            U = R.utility_eval(util, th, y.reshape(m, S * n), params).reshape(S, n)
        for i in range(n):
            rho, T, gap[i, l] = statistic(U[:, i], kind, k)
            alpha[i] += p[l] * rho
            fin = np.abs(U[:, i][np.isfinite(U[:, i])])
            scale[i] = max(scale[i], fin.max() if fin.size else 0.0)
            if grad:
                g = np.zeros(dmean.shape[2])
                for s in T:
                    dU = R.utility_grad(util, th, y[:, s, i], params)
                    g += dU.dot(dmean[:, i, :]) + (dU * W[s] / (2.0 * sg[:, i])).dot(dvar[:, i, :])
                dalpha[i] += p[l] * g / len(T)
    out = dict(alpha=alpha, gap=gap, scale=scale)
    if grad:
        out["dalpha"] = dalpha
    return out


def risk_hyper(means, variances, W, thetas, prob, util, params, kind, k, dmeans=None, dvars=None):
    """The mean over the hyper-samples h of risk(means[h], ...); gap is the smallest, scale the largest over them."""
    rs = [risk(means[h], variances[h], W, thetas, prob, util, params, kind, k, None if dmeans is None else dmeans[h],
               None if dvars is None else dvars[h]) for h in range(len(means))]
    out = dict(alpha=np.mean([r["alpha"] for r in rs], 0), gap=np.min([r["gap"] for r in rs], 0), scale=np.max([r["scale"] for r in rs], 0))
    if dmeans is not None:
        out["dalpha"] = np.mean([r["dalpha"] for r in rs], 0)
    return out


def linear_ucb(mean, var, thetas, prob, kappa, dmean=None, dvar=None):
    """sum_l p_l [theta_l . mu + kappa sqrt(sum_j theta_lj^2 var_j)] (n,), and with dmean / dvar its input gradient (n, d)."""
    thetas = np.atleast_2d(thetas)
    L = thetas.shape[0]
    p = np.full(L, 1.0 / L) if prob is None else np.asarray(prob, dtype=float)
    mu = thetas.dot(mean)                                                     # (L, n)
    sig = np.sqrt((thetas ** 2).dot(var))
    val = p.dot(mu + kappa * sig)
    if dmean is None:
        return val
    dmu = np.einsum("lj,jnq->lnq", thetas, dmean)
    dv = np.einsum("lj,jnq->lnq", thetas ** 2, dvar)
    return val, np.einsum("l,lnq->nq", p, dmu + kappa * dv / (2.0 * sig[:, :, None]))


def rank_of(level, S):
    """min(S - 1, floor(level * S)): the rank the Python classes hand to the device."""
    return min(S - 1, int(math.floor(level * S)))
