"""NumPy restatement of the constrained expected utility of the recommendation step (include/bocf_hip.h), over
posterior arrays -- mean, var (m, n), their input gradients (m, n, d) -- with oracle.cpu_ref (utility_eval, utility_grad) and
tests/constrained_ref (sigmoid, constraint_values).  Test infrastructure only: nothing under bocf_amd/ imports it.

    phi(y)  = prod_k s(-c_k(y) / eta_k)              k in index order, c = A y - b
    y_s(x)  = mu(x) + sigma(x) o Z_s                 Z = the normals of the row's own parameter, block rows[i]
    T_s     = phi(y_s) (U(theta_l, y_s) - u0_l)
    G_l(x)  = sum_{h < n_hyps} sum_s [u0_l + T_s]    a SUM; one hyper-sample counts n_hyps times
    P(x)    = mean over the hyper-samples visited and s of phi(y_s)
    dT/dy_j = phi (dU/dy_j - (U - u0_l) q_j),  q_j = sum_k (1 - s_k) A_kj / eta_k
    dG/dx_q = sum_h sum_j A_j dmu_j/dx_q + B_j dsigma^2_j/dx_q,  A_j = sum_s dT/dy_j,  B_j = sum_s dT/dy_j Z_sj / (2 sigma_j)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_ref as CR  # noqa: E402

from oracle import cpu_ref as R  # noqa: E402


def constrained_eu(mean, var, Z, thetas, rows, u0, kind, params, A, b, eta, dmean=None, dvar=None, hard=False):
    """One hyper-sample.  mean, var (m, n); Z (L, S, m); thetas (L, theta_dim); rows (n,) in [0, L); u0 (L,).  hard: the indicator of the
    feasible set in the place of phi (values only).  Returns a dict: G (n,) = sum_s [u0 + T_s], phi_sum (n,) = sum_s phi, scale = the
    largest |U - u0| met, and with dmean / dvar the gradient dG (n, d)."""
    mean, var, Z = np.asarray(mean, dtype=float), np.asarray(var, dtype=float), np.asarray(Z, dtype=float)
    A, b, eta = np.atleast_2d(np.asarray(A, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float)), np.atleast_1d(np.asarray(eta, dtype=float))
    thetas, rows, u0 = np.atleast_2d(thetas), np.asarray(rows).reshape(-1), np.atleast_1d(np.asarray(u0, dtype=float))
    m, n = mean.shape
    S, K = Z.shape[1], A.shape[0]
    grad = dmean is not None
    G, phi_sum, scale = np.zeros(n), np.zeros(n), 0.0
    dG = np.zeros((n, dmean.shape[2])) if grad else None
    sg = np.sqrt(var)
    for l in np.unique(rows):
        sel = np.flatnonzero(rows == l)
        th, Zl = thetas[l], Z[l]                                              # Zl (S, m)
        y = mean[:, None, sel] + sg[:, None, sel] * Zl.T[:, :, None]          # (m, S, nl)
        c = CR.constraint_values(A, b, y)                                     # (K, S, nl)
        sk, omsk = CR.sigmoid(-c / eta[:, None, None])
        if hard:
            phi = np.all(c <= 0.0, axis=0).astype(float)
        else:
            phi = np.ones(c.shape[1:])
            for k in range(K):
                phi = phi * sk[k]
        U = np.asarray(R.utility_eval(kind, th, y.reshape(m, -1), params), dtype=float).reshape(S, len(sel))
        t = U - u0[l]
        scale = max(scale, float(np.max(np.abs(t))))
        G[sel] = np.sum(u0[l] + phi * t, axis=0)
        phi_sum[sel] = phi.sum(0)
        if grad:
            q = np.einsum("ksn,kj->jsn", omsk / eta[:, None, None], A)        # (m, S, nl)
            dU = np.empty_like(y)
            for s in range(S):
                for i in range(len(sel)):
                    dU[:, s, i] = R.utility_grad(kind, th, y[:, s, i], params)
            dT = phi[None] * (dU - t[None] * q)                               # (m, S, nl)
            Aj = dT.sum(1)                                                    # (m, nl)
            Bj = (dT * Zl.T[:, :, None]).sum(1) / (2.0 * sg[:, sel])
            dG[sel] = np.einsum("jn,jnq->nq", Aj, dmean[:, sel]) + np.einsum("jn,jnq->nq", Bj, dvar[:, sel])
    out = dict(G=G, phi_sum=phi_sum, scale=scale)
    if grad:
        out["dG"] = dG
    return out


def constrained_eu_hyper(means, variances, Z, thetas, rows, u0, kind, params, A, b, eta, n_hyps, dmeans=None, dvars=None, hard=False):
    """The sum over the first n_hyps hyper-samples of constrained_eu(means[h], ...); with ONE hyper-sample given it counts n_hyps times
    (bocf_expected_utility's rule for fixed hyper-parameters).  Returns G (n,), P (n,) = the mean of phi over the hyper-samples visited
    and the samples, scale, n_h = hyper-samples visited, and dG with the gradients."""
    H = len(means)
    n_h = 1 if H == 1 else int(n_hyps)
    assert n_h <= H
    rs = [constrained_eu(means[h], variances[h], Z, thetas, rows, u0, kind, params, A, b, eta,
                         None if dmeans is None else dmeans[h], None if dvars is None else dvars[h], hard=hard) for h in range(n_h)]
    mult = float(n_hyps) if H == 1 else 1.0
    S = np.asarray(Z).shape[1]
    out = dict(G=mult * np.sum([r["G"] for r in rs], 0), P=np.sum([r["phi_sum"] for r in rs], 0) / (n_h * S), scale=max(r["scale"] for r in rs), n_h=n_h)
    if dmeans is not None:
        out["dG"] = mult * np.sum([r["dG"] for r in rs], 0)
    return out


def plain_mc_eu(mean, var, Z, thetas, rows, kind, params):
    """sum_s U(theta_{rows[i]}, mu_i + sigma_i o Z_s): the Monte-Carlo expected utility of cbo.py:190-231 for one hyper-sample, written with
    the oracle's utilities one sample at a time."""
    mean, var = np.asarray(mean, dtype=float), np.asarray(var, dtype=float)
    sg = np.sqrt(var)
    out = np.zeros(mean.shape[1])
    for i, l in enumerate(np.asarray(rows).reshape(-1)):
        for z in np.asarray(Z)[l]:
            out[i] += float(R.utility_eval(kind, np.atleast_2d(thetas)[l], mean[:, i] + sg[:, i] * z, params))
    return out


# ---- the posterior the device tests compare on: tests/kg_ref.LookAhead fits (oracle GPFit per output)
def posterior_noiseless(la, X, grad=False):
    """(mean, var) (m, n) as bocf_expected_utility reads them -- predict_noiseless: no likelihood noise, clipped at 1e-10 -- and with grad
    their input gradients (m, n, d)."""
    X = np.atleast_2d(X)
    mean = np.stack([f.posterior_mean(X)[:, 0] for f in la.fits])
    var = np.stack([f.posterior_variance_noiseless(X)[:, 0] for f in la.fits])
    if not grad:
        return mean, var
    return mean, var, np.stack([f.posterior_mean_gradient(X) for f in la.fits]), np.stack([f.posterior_variance_gradient(X) for f in la.fits])


def restated_factory(ref, kind, n_h, params=None):
    """evaluator= of bocf_amd.current_marginal_argmaxes: the restatement on the noiseless posterior of `ref` (predict_noiseless,
    posterior_mean_gradient, posterior_variance_gradient: the oracle's MultiOutputGPRef, or a model with fixed hyper-parameters), the one
    hyper-sample counted n_h times.  Without constraints: the plain Monte-Carlo expected utility, as the same sums with phi = 1."""
    def factory(parameters, Z, constraints=None, u0=None):
        def both(X, rows, grad):
            X = np.atleast_2d(X)
            mean, var = ref.predict_noiseless(X)
            dm, dv = (ref.posterior_mean_gradient(X), ref.posterior_variance_gradient(X)) if grad else (None, None)
            if constraints is None:                                                # the plain expected utility: phi = 1 and q = 0 exactly
                A, b, eta, u = np.ones((1, ref.output_dim)), np.full(1, 1e30), np.ones(1), np.zeros(len(parameters))
            else:
                A, b, eta, u = constraints.A, constraints.b, constraints.eta, u0
            r = constrained_eu_hyper([mean], [var], Z, parameters, rows, u, kind, params, A, b, eta, n_h,
                                        None if dm is None else [dm], None if dv is None else [dv])
            return r["G"], r.get("dG"), r["P"]

        def ev(X, rows, grad=False):
            return both(X, rows, grad)[:2]
        ev.pof = lambda X, rows: both(X, rows, False)[2]
        return ev
    return factory
