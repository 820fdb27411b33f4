"""NumPy restatement of the constrained Monte-Carlo expected improvement (include/bocf_hip.h), over posterior arrays
-- mean, var (m, n), their input gradients (m, n, d), the train mean (m, N) -- and oracle.cpu_ref (utility_eval, utility_grad).  Test
infrastructure only: nothing under bocf_amd/ imports it.

    c_k(y)   = sum_j A_kj y_j - b_k                  feasible <=> c_k(y) <= 0 for every k
    s(t)     = 1 / (1 + exp(-t))                     with exp of a non-positive argument on both branches
    phi(y)   = prod_k s(-c_k(y) / eta_k)             k in index order
    y_s(x)   = mu(x) + sigma(x) o W_s
    F        = { i : c_k(mu(X_i)) <= 0 for every k } (hard), best_l = max_{i in F} U(theta_l, mu(X_i))
    I_ls     = max(U(theta_l, y_s) - best_l, 0) if F is not empty, 1 if it is
    alpha(x) = sum_l p_l (1/S) sum_s I_ls phi(y_s)
    dT/dy_j  = [F not empty] 1{U > best_l} dU/dy_j phi - T_ls sum_k (1 - s_k) A_kj / eta_k,  T = I phi
    d alpha/dx_q = sum_j A_j dmu_j/dx_q + B_j dsigma^2_j/dx_q,  A_j = sum_l p_l/S sum_s dT/dy_j,  B_j = sum_l p_l/S sum_s dT/dy_j W_sj / (2 sigma_j)
"""
import numpy as np

from oracle import cpu_ref as R


def sigmoid(t):
    """(s(t), 1 - s(t)), each from e = exp(-|t|)."""
    t = np.asarray(t, dtype=float)
    e = np.exp(-np.abs(t))
    hi, lo = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(t >= 0, hi, lo), np.where(t >= 0, lo, hi)


def constraint_values(A, b, y):
    """c (K, ...) = A y - b for y (m, ...)."""
    A, b = np.atleast_2d(A), np.atleast_1d(b)
    return np.tensordot(A, y, axes=(1, 0)) - b.reshape((-1,) + (1,) * (y.ndim - 1))


def feasible_best(mu_train, thetas, kind, params, A, b):
    """(best (L,), number of feasible training points): the hard test on the train mean (m, N); best = -inf when none passes."""
    feas = np.all(constraint_values(A, b, mu_train) <= 0.0, axis=0)
    thetas = np.atleast_2d(thetas)
    if not feas.any():
        return np.full(len(thetas), -np.inf), 0
    return np.array([np.max(R.utility_eval(kind, th, mu_train[:, feas], params)) for th in thetas]), int(feas.sum())


def constrained(mean, var, mu_train, W, thetas, prob, kind, params, A, b, eta, dmean=None, dvar=None, best=None, hard=False):
    """alpha of the n candidates of one hyper-sample.  best: (best (L,), n_feasible) to use instead of this train mean's (the incumbent of
    another hyper-sample); hard: the indicator of the feasible set in the place of phi (values only).  Returns a dict: alpha (n,),
    best, n_feasible, gap (n,) = the smallest |U - best_l| over (l, s) (inf with no incumbent), cmin (n,) = the smallest |c_k(y_s)|,
    phi_mean (n,) = mean_s phi, scale = the largest |U| met, and with dmean / dvar the gradient dalpha (n, d)."""
    mean, var, W = np.asarray(mean, dtype=float), np.asarray(var, dtype=float), np.atleast_2d(W)
    A, b, eta = np.atleast_2d(np.asarray(A, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float)), np.atleast_1d(np.asarray(eta, dtype=float))
    thetas = np.atleast_2d(thetas)
    m, n = mean.shape
    S, L, K = W.shape[0], thetas.shape[0], A.shape[0]
    p = np.full(L, 1.0 / L) if prob is None else np.asarray(prob, dtype=float)
    best, nf = feasible_best(mu_train, thetas, kind, params, A, b) if best is None else best
    sg = np.sqrt(var)
    y = mean[:, None, :] + sg[:, None, :] * W.T[:, :, None]              # (m, S, n)
    c = constraint_values(A, b, y)                                        # (K, S, n)
    sk, omsk = sigmoid(-c / eta[:, None, None])
    if hard:
        phi = np.all(c <= 0.0, axis=0).astype(float)
    else:
        phi = np.ones((S, n))
        for k in range(K):
            phi = phi * sk[k]
    grad = dmean is not None
    alpha, gap, scale = np.zeros(n), np.full(n, np.inf), 0.0
    dTdy = np.zeros((m, S, n))                                            # sum_l p_l dT_ls / dy_j
    q = np.einsum("ksn,kj->jsn", omsk / eta[:, None, None], A)            # sum_k (1 - s_k) A_kj / eta_k
    for l, th in enumerate(thetas):
        if nf > 0:
            U = R.utility_eval(kind, th, y.reshape(m, S * n), params).reshape(S, n)
            scale = max(scale, float(np.max(np.abs(U))), abs(float(best[l])))
            gap = np.minimum(gap, np.min(np.abs(U - best[l]), axis=0))
            I = np.maximum(U - best[l], 0.0)
        else:
            I = np.ones((S, n))
        T = I * phi
        alpha += p[l] / S * T.sum(0)
        if grad:
            dTdy -= p[l] * T[None] * q
            if nf > 0:
                for s, i in zip(*np.nonzero(U > best[l])):
                    dTdy[:, s, i] += p[l] * phi[s, i] * R.utility_grad(kind, th, y[:, s, i], params)
    out = dict(alpha=alpha, best=best, n_feasible=nf, gap=gap, cmin=np.min(np.abs(c), axis=(0, 1)), phi_mean=phi.mean(0), scale=scale)
    if grad:
        Aj = dTdy.sum(1) / S                                              # (m, n)
        Bj = (dTdy * W.T[:, :, None]).sum(1) / S / (2.0 * sg)
        out["dalpha"] = np.einsum("jn,jnq->nq", Aj, dmean) + np.einsum("jn,jnq->nq", Bj, dvar)
    return out


def constrained_hyper(means, variances, mu_trains, W, thetas, prob, kind, params, A, b, eta, dmeans=None, dvars=None, best_group=0, hard=False):
    """The mean over the hyper-samples h of constrained(means[h], ...), with the incumbent of hyper-sample best_group for all of them (the
    rule of the Monte-Carlo acquisitions: the hyper-sample current on entry), or each one's own with best_group = None."""
    rs = []
    for h in range(len(means)):
        g = h if best_group is None else best_group
        best = feasible_best(mu_trains[g], thetas, kind, params, A, b)
        rs.append(constrained(means[h], variances[h], mu_trains[h], W, thetas, prob, kind, params, A, b, eta,
                              None if dmeans is None else dmeans[h], None if dvars is None else dvars[h], best=best, hard=hard))
    out = dict(alpha=np.mean([r["alpha"] for r in rs], 0), gap=np.min([r["gap"] for r in rs], 0), cmin=np.min([r["cmin"] for r in rs], 0),
               scale=max(r["scale"] for r in rs), best=rs[0]["best"], n_feasible=rs[0]["n_feasible"], phi_mean=np.mean([r["phi_mean"] for r in rs], 0))
    if dmeans is not None:
        out["dalpha"] = np.mean([r["dalpha"] for r in rs], 0)
    return out


# ---- the posterior the device tests compare on: tests/kg_ref.LookAhead fits (oracle GPFit per output)
def posterior(la, X, grad=False):
    """(mean, var) (m, n) as the Monte-Carlo acquisitions read them -- variance with noise, clipped at 1e-10 -- and with grad their input
    gradients (m, n, d)."""
    X = np.atleast_2d(X)
    mean = np.stack([f.posterior_mean(X)[:, 0] for f in la.fits])
    var = np.stack([f.posterior_variance(X)[:, 0] for f in la.fits])
    if not grad:
        return mean, var
    return mean, var, np.stack([f.posterior_mean_gradient(X) for f in la.fits]), np.stack([f.posterior_variance_gradient(X) for f in la.fits])


def train_mean(la):
    return np.stack([f.posterior_mean(f.X)[:, 0] for f in la.fits])


def draw_constraints(rng, mu_train, K, eta, share=0.5):
    """K random linear constraints whose right-hand sides leave about `share` of the training means on the feasible side of each row."""
    m = mu_train.shape[0]
    A = rng.normal(size=(K, m))
    b = np.array([np.quantile(A[k].dot(mu_train), share ** (1.0 / K)) for k in range(K)])
    return A, b, np.full(K, float(eta))


def utility_inputs(rng, kind, m, L):
    """(thetas (L, theta_dim), prob, params) of a device utility, as the pending-point cases draw them."""
    if kind == "rosenbrock":
        thetas = rng.uniform(0.2, 1.0, size=(L, 1))
    elif kind in ("neg_sum_exp", "neg_exp_cos"):
        thetas = np.zeros((L, 1))
    else:
        thetas = rng.uniform(-0.5, 0.5, size=(L, m))
    params = rng.uniform(0.5, 1.0, size=m) if kind == "neg_exp_cos" else None
    return thetas, params
