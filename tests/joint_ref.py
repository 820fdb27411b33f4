"""NumPy restatement of the joint Monte-Carlo expected improvement of the composite utility at whole q-point batches (q-uEI), over
tests/kg_ref.LookAhead (mean, cov, cov_grad, var_grad), tests/pending_ref (mean_grad, best_so_far) and oracle.cpu_ref (utility_eval,
utility_grad).  Test infrastructure only: nothing under bocf_amd/ imports it.  It is the authority on what bocf_acq_joint computes.

Per output j of a batch X = (x_1 .. x_q): mu_j(X) (q,), Sigma_j = k_j(X, X) - V_X^T V_X symmetrised (latent, noiseless),
tau_j = 1e-8 max(mean diag Sigma_j, 1e-10) (rung 0 of pending_ref.ladder, no further rungs; a constant in the gradient) and C_j the lower
factor of Sigma_j + tau_j I by the row-wise Cholesky with a pivot floor (chol_floor): p_k = a_kk - sum_{i<k} C_ki^2, and where
not (p_k > 1e-10) p_k := 1e-10 and the pivot is floored -- a constant whose adjoint is dropped.  With the normals Z (S, m, q):

    y[s, j, k] = mu_jk + sum_{i <= k} C_j[k, i] Z[s, j, i],   u[l, s, k] = U(theta_l, y[s, :, k]),   k* = lowest index of max_k u
    alpha(X)   = sum_l p_l (1/S) sum_s max(u[l, s, k*] - best_l, 0)

Gradient (envelope rule; Z, theta, best fixed):  Ybar[s, j, k*] += p_l / S 1[u > best_l] dU/dy_j,  mubar_jk = sum_s Ybar[s, j, k],
Cbar_j[k, i] = sum_s Ybar[s, j, k] Z[s, j, i] (i <= k),  Sigmabar_j = chol_adjoint (symmetric convention d alpha = sum_ab Sigmabar_ab
dSigma_ab),  d alpha / dx_a = sum_j [ mubar_ja dmu_j(x_a)/dx + Sigmabar_j[a, a] dsigma^2_j(x_a)/dx + 2 sum_{b != a} Sigmabar_j[a, b]
d_1 Sigma_j(x_a, x_b) ],  d_1 holding x_b fixed (LookAhead.cov_grad)."""
import numpy as np

from oracle import cpu_ref as R

import pending_ref as PR

FLOOR = 1e-10


def jitter(Sigma):
    return 1e-8 * max(float(np.mean(np.diag(Sigma))), 1e-10)


def chol_floor(A, tau=0.0):
    """(C lower, floored (q,) bool) of A + tau I, row by row with the pivot floor."""
    q = len(A)
    C, floored = np.zeros((q, q)), np.zeros(q, dtype=bool)
    for k in range(q):
        for i in range(k):
            C[k, i] = (A[k, i] - C[k, :i].dot(C[i, :i])) / C[i, i]
        p = A[k, k] + tau - C[k, :k].dot(C[k, :k])
        if not p > FLOOR:
            p, floored[k] = FLOOR, True
        C[k, k] = np.sqrt(p)
    return C, floored


def chol_adjoint(C, floored, Cbar):
    """Sigmabar (q, q) symmetric with d alpha = sum_ab Sigmabar_ab dA_ab, from Cbar (lower triangle read): rows k = q - 1 .. 0, the pivot's
    adjoint first, then the off-diagonal numerators i = k - 1 .. 0."""
    q = len(C)
    G = np.tril(np.array(Cbar, dtype=float))
    for k in range(q - 1, -1, -1):
        pb = 0.0 if floored[k] else G[k, k] / (2.0 * C[k, k])
        G[k, k] = pb
        G[k, :k] -= 2.0 * pb * C[k, :k]
        for i in range(k - 1, -1, -1):
            nb = G[k, i] / C[i, i]
            G[i, i] -= nb * C[k, i]
            G[k, :i] -= nb * C[i, :i]
            G[i, :i] -= nb * C[k, :i]
            G[k, i] = nb
    low = np.tril(G, -1)
    return np.diag(np.diag(G)) + 0.5 * (low + low.T)


def batch_samples(mu, C, Z):
    """y (S, m, q) from mu (m, q), C (m, q, q) lower and Z (S, m, q)."""
    return mu[None, :, :] + np.einsum("jki,sji->sjk", C, Z)


def utilities(y, thetas, kind, params=None):
    """u (L, S, q) of y (S, m, q)."""
    S, m, q = y.shape
    flat = y.transpose(1, 0, 2).reshape(m, S * q)
    return np.stack([R.utility_eval(kind, th, flat, params).reshape(S, q) for th in np.atleast_2d(thetas)])


def value_from_moments(mu, Sigma, Z, thetas, prob, kind, params, best):
    """alpha of ONE batch from its mu (m, q) and Sigma (m, q, q); also what the gradient and the tests' filters need."""
    m, q = mu.shape
    S, Lt = Z.shape[0], len(np.atleast_2d(thetas))
    p = np.full(Lt, 1.0 / Lt) if prob is None else np.asarray(prob, dtype=float)
    C, floored, tau, cond = np.zeros((m, q, q)), np.zeros((m, q), dtype=bool), np.zeros(m), 0.0
    for j in range(m):
        Sj = 0.5 * (Sigma[j] + Sigma[j].T)
        tau[j] = jitter(Sj)
        C[j], floored[j] = chol_floor(Sj, tau[j])
        cond = max(cond, float(np.linalg.cond(Sj + tau[j] * np.eye(q))))
    y = batch_samples(mu, C, Z)
    u = utilities(y, thetas, kind, params)                       # (L, S, q)
    kstar = np.argmax(u, 2)                                      # numpy returns the first maximum
    top = np.max(u, 2)                                           # (L, S)
    imp = top - np.asarray(best, dtype=float)[:, None]
    alpha = float(np.sum(p[:, None] * np.maximum(imp, 0.0)) / S)
    margin = float(np.min(np.abs(imp)))
    if q > 1:
        margin = min(margin, float(np.min(top - np.sort(u, 2)[:, :, -2])))
    scale = max(float(np.max(np.abs(u))), float(np.max(np.abs(best))))
    return dict(alpha=alpha, C=C, floored=floored, tau=tau, cond=cond, y=y, u=u, kstar=kstar, imp=imp, margin=margin, scale=scale, p=p)


def joint(la, X, Z, thetas, prob, kind, params=None, best=None, grad=False):
    """alpha of every batch of X (B, q, d) under one LookAhead.  Returns a dict: alpha (B,), floored (B,) = floored pivots per batch,
    cond = max cond(Sigma_j + tau_j I), scale = the largest |U| met (and |best|), margin (B,) = the smallest distance to a kink over
    (l, s): the gap between the best and the second-best point and |u - best|; with grad dalpha (B, q, d)."""
    X, Z = np.asarray(X, dtype=float), np.asarray(Z, dtype=float)
    B, q, d = X.shape
    thetas = np.atleast_2d(thetas)
    if best is None:
        best = PR.best_so_far(la, thetas, kind, params)
    S = Z.shape[0]
    out = dict(alpha=np.zeros(B), floored=np.zeros(B, dtype=int), margin=np.zeros(B), cond=0.0, scale=0.0, best=np.asarray(best, dtype=float))
    if grad:
        out["dalpha"] = np.zeros((B, q, d))
    for b in range(B):
        mu, Sig = la.mean(X[b]), la.cov(X[b], X[b])
        v = value_from_moments(mu, Sig, Z, thetas, prob, kind, params, best)
        out["alpha"][b], out["floored"][b], out["margin"][b] = v["alpha"], int(v["floored"].sum()), v["margin"]
        out["cond"], out["scale"] = max(out["cond"], v["cond"]), max(out["scale"], v["scale"])
        if not grad:
            continue
        m = la.m
        Ybar = np.zeros((S, m, q))
        for l, th in enumerate(thetas):
            for s in np.flatnonzero(v["imp"][l] > 0.0):
                k = v["kstar"][l, s]
                Ybar[s, :, k] += v["p"][l] / S * R.utility_grad(kind, th, v["y"][s, :, k], params)
        mubar = Ybar.sum(0)                                       # (m, q)
        dmu, ds2, dcv = PR.mean_grad(la, X[b]), la.var_grad(X[b]), la.cov_grad(X[b], X[b])       # (m, q, d), (m, q, d), (m, q, q, d)
        for j in range(m):
            Cbar = np.einsum("sk,si->ki", Ybar[:, j, :], Z[:, j, :])
            Sb = chol_adjoint(v["C"][j], v["floored"][j], Cbar)
            for a in range(q):
                g = mubar[j, a] * dmu[j, a] + Sb[a, a] * ds2[j, a]
                for o in range(q):
                    if o != a:
                        g = g + 2.0 * Sb[a, o] * dcv[j, a, o]
                out["dalpha"][b, a] += g
    return out


def joint_hyper(las, X, Z, thetas, prob, kind, params=None, best=None, grad=False):
    """The restatement averaged over the hyper-samples `las`.  best: None = the best-so-far of hyper-sample 0 for all (the rule of the
    Monte-Carlo acquisitions: the hyper-sample current on entry), (L,) for all, or (H, L)."""
    thetas = np.atleast_2d(thetas)
    if best is None:
        best = PR.best_so_far(las[0], thetas, kind, params)
    best = np.broadcast_to(np.asarray(best, dtype=float), (len(las), len(thetas)))
    rs = [joint(la, X, Z, thetas, prob, kind, params, best=best[h], grad=grad) for h, la in enumerate(las)]
    out = dict(alpha=np.mean([r["alpha"] for r in rs], 0), floored=np.sum([r["floored"] for r in rs], 0), margin=np.min([r["margin"] for r in rs], 0),
               cond=max(r["cond"] for r in rs), scale=max(r["scale"] for r in rs), best=best)
    if grad:
        out["dalpha"] = np.mean([r["dalpha"] for r in rs], 0)
    return out


def median_best(las, X0, Z, thetas, kind, params=None):
    """(H, L): per hyper-sample and parameter the median over s of max_k u at the batch X0 (q, d) -- an incumbent that makes about half the
    samples of a typical batch improve."""
    thetas = np.atleast_2d(thetas)
    out = np.zeros((len(las), len(thetas)))
    for h, la in enumerate(las):
        v = value_from_moments(la.mean(X0), la.cov(X0, X0), Z, thetas, None, kind, params, np.zeros(len(thetas)))
        out[h] = np.median(np.max(v["u"], 2), 1)
    return out


# ---- the device test's cases (tests/test_gpu_joint.py), shared with the CPU checks of their caps (tests/test_joint_cpu.py)
MIXED = ["se", "matern52", "rbf", "matern32"]
#         N   d   m  q   S   L  H  B   utility        seed  best
# The seeds were searched on the CPU for the caps tests/test_joint_cpu.py checks (cond <= 1e4, at most 1/8 of the batches near a kink,
# alpha > 0 on at least 3/4).  With one sample the median incumbent IS the first batch's sample: that batch sits on its kink and is one
# of the sixteen; with an odd S the same holds for one sample of the first batch.
CASES = [(12, 1, 1, 1, 1, 1, 1, 16, "neg_sq_dist", 2, "median"),          # smallest m, q, d, S, L
         (40, 3, 3, 2, 64, 3, 1, 1, "neg_sum_exp", 2, "median"),          # one batch, one full wave of samples
         (130, 3, 3, 3, 65, 3, 2, 16, "neg_sq_dist", 3, "median"),        # past one wave, Np = 256, two hyper-samples, q no divisor of 128
         (40, 1, 3, 2, 64, 3, 1, 16, "neg_exp_cos", 1, "median"),         # d = 1
         (12, 3, 16, 8, 256, 1, 1, 4, "rosenbrock", 5, "median"),         # the limits of m, q and S together
         (12, 3, 2, 8, 96, 1, 1, 16, "neg_sq_dist", 20, None)]            # the default incumbent (launch_best_so_far), kinds se and matern52
# value only, across the chunk boundary at 128 points (N = 130, m = 2 under workspace_mb = 1: chunks of 128 points, 126 at q = 3)
CHUNK_CASES = [(130, 3, 2, 3, 64, 3, 1, 42, "neg_sq_dist", 1, "median"),
               (130, 3, 2, 3, 64, 3, 1, 43, "neg_sq_dist", 1, "median"),
               (130, 3, 2, 8, 64, 3, 1, 17, "neg_sq_dist", 7, "median")]


def case_id(c):
    return "N%d-d%d-m%d-q%d-S%d-L%d-H%d-B%d-%s" % c[:9]


def case_inputs(N, d, m, q, S, L, H, B, kind, seed, best):
    """Everything a case is made of, from its seed: the problem of kg_ref.problem (noise 1e-4) with one kernel family per output, the
    batches X (B, q, d), the normals Z (S, m, q), utility parameters."""
    import kg_ref as K
    kinds = [MIXED[j % 4] for j in range(m)]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, B * q, seed, noise=1e-4)
    rng = np.random.RandomState(7000 + seed)
    Z = rng.normal(size=(S, m, q))
    if kind == "rosenbrock":
        thetas = rng.uniform(0.2, 1.0, size=(L, 1))
    elif kind in ("neg_sum_exp", "neg_exp_cos"):
        thetas = np.zeros((L, 1))
    else:
        thetas = rng.uniform(-0.5, 0.5, size=(L, m))
    prob = None if L == 1 else rng.dirichlet(np.ones(L))
    params = rng.uniform(0.5, 1.0, size=m) if kind == "neg_exp_cos" else None
    return dict(kinds=kinds, X=X, Y=Y, var=var, ls=ls, nz=nz, Xb=Xc.reshape(B, q, d), Z=Z, thetas=thetas, prob=prob, params=params, kind=kind, H=H, q=q,
                best=best)


def case_reference(inp, las, grad=False, n=None):
    """(restatement, the incumbents handed to the device or None): best = "median" is median_best at the case's first batch."""
    best = median_best(las, inp["Xb"][0], inp["Z"], inp["thetas"], inp["kind"], inp["params"]) if inp["best"] == "median" else None
    Xb = inp["Xb"] if n is None else inp["Xb"][:n]
    return joint_hyper(las, Xb, inp["Z"], inp["thetas"], inp["prob"], inp["kind"], inp["params"], best=best, grad=grad), best
