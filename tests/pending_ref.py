"""NumPy restatement of the Monte-Carlo expected improvement of the composite utility conditioned on pending points, over
tests/kg_ref.LookAhead (mean, var_raw, cov, cov_grad, var_grad) and oracle.cpu_ref (utility_eval, utility_grad).  Test infrastructure
only: nothing under bocf_amd/ imports it.

Per output j, P = (p_1 .. p_r) pending, Sigma~_j = Sigma_j(P, P) + tau_j I (jitter ladder: 1e-8 max(mean diag, 1e-10), x 10 per rung):

    route "bordered" (the default): per candidate x the (r + 1) x (r + 1) matrix B_j = [[Sigma~_j, c_j], [c_j^T, sigma^2_j(x)]],
        c_j = Sigma_j(P, x), is factorized whole (numpy.linalg.cholesky); its last row (g_j^T, sqrt(v_j)) gives
        y_sj(x) = mu_j(x) + g_j^T Zp[s, j, :] + sqrt(v_j) W[s, j], its leading block the joint samples F_sj = mu_j(P) + L_j Zp[s, j, :].
        Where sigma^2_j(x) - g^T g is not above the 1e-10 clip the corner is set to g^T g + 1e-10 (what the clip means) and B factorized again.
        Gradient: dg = L^-1 dc, dv = dsigma^2 - 2 g^T dg.
    route "conditional": Q_j = Sigma~_j^-1, G_sj = L_j^-T Zp[s, j, :], v_j = max(sigma^2_j - c_j^T Q_j c_j, 1e-10),
        y_sj = mu_j(x) + c_j^T G_sj + sqrt(v_j) W[s, j];  dv = dsigma^2 - 2 (Q c)^T dc.

    T_ls = max(best_l, max_i U(theta_l, F_s[:, i])),   alpha(x | P) = sum_l p_l (1/S) sum_s max(U(theta_l, y_s(x)) - T_ls, 0)
    d alpha / dx = sum_l p_l / S sum_s 1[U > T_ls] sum_j dU/dy_j dy_sj/dx,   dy_sj/dx = dmu_j/dx + (.)^T dc_j/dx + W[s, j] dv_j/dx / (2 sqrt(v_j)),
    dv = 0 where the clip is active.  P, Zp and W are held fixed.
"""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import cpu_ref as R

CLIP = 1e-10


def ladder(Sigma, max_tries=10):
    """(tau, L lower) of the first rung at which Sigma + tau I factorizes; LinAlgError when none of max_tries rungs does."""
    tau = 1e-8 * max(float(np.mean(np.diag(Sigma))), 1e-10)
    for _ in range(max(1, int(max_tries))):
        try:
            return tau, np.linalg.cholesky(Sigma + tau * np.eye(len(Sigma)))
        except np.linalg.LinAlgError:
            tau *= 10.0
    raise np.linalg.LinAlgError("not positive definite, even with jitter.")


def best_so_far(la, thetas, kind, params=None):
    """best_l = max_i U(theta_l, mu(X_i)) over the training inputs: the best-so-far of the Monte-Carlo acquisitions."""
    mu = la.mean(la.fits[0].X)
    return np.array([np.max(R.utility_eval(kind, th, mu, params)) for th in np.atleast_2d(thetas)])


def mean_grad(la, Xc):
    return np.stack([f.posterior_mean_gradient(Xc) for f in la.fits])


def pending_state(la, P, Zp, max_tries=10):
    """What depends on the pending points only: dict(tau (m,), L, Q (m, r, r), F, G (S, m, r), cond = max_j cond(Sigma~_j), Sigma)."""
    P, Zp = np.atleast_2d(P), np.asarray(Zp, dtype=float)
    m, r = la.m, P.shape[0]
    Sig, muP = la.cov(P, P), la.mean(P)
    tau, L, Q = np.zeros(m), np.zeros((m, r, r)), np.zeros((m, r, r))
    F, G = np.zeros(Zp.shape), np.zeros(Zp.shape)
    cond = 0.0
    for j in range(m):
        S_j = 0.5 * (Sig[j] + Sig[j].T)
        tau[j], L[j] = ladder(S_j, max_tries)
        Q[j] = np.linalg.inv(S_j + tau[j] * np.eye(r))
        cond = max(cond, float(np.linalg.cond(S_j + tau[j] * np.eye(r))))
        F[:, j, :] = muP[j] + Zp[:, j, :].dot(L[j].T)
        G[:, j, :] = solve_triangular(L[j], Zp[:, j, :].T, lower=True, trans="T").T
    return dict(tau=tau, L=L, Q=Q, F=F, G=G, cond=cond, Sigma=Sig)


def thresholds(F, thetas, best, kind, params=None):
    """T (L, S) and the largest |U| met at the pending samples."""
    thetas = np.atleast_2d(thetas)
    S, m, r = F.shape
    T = np.empty((len(thetas), S))
    scale = 0.0
    for l, th in enumerate(thetas):
        u = R.utility_eval(kind, th, F.transpose(1, 0, 2).reshape(m, S * r), params).reshape(S, r)
        scale = max(scale, float(np.max(np.abs(u))), abs(float(best[l])))
        T[l] = np.maximum(best[l], u.max(1))
    return T, scale


def pending(la, Xc, P, Zp, W, thetas, prob, kind, params=None, best=None, grad=False, route="bordered", max_tries=10):
    """alpha(x | P) of every row of Xc.  Returns a dict: alpha (n,), scale = the largest |U| met, gap (n,) = min over (l, s) of
    |U - T_ls|, cond = max_j cond(Sigma~_j), F, T, tau, and with grad the gradient dalpha (n, d) and slope (n,) = the largest
    sum_q |dU(theta_l, y_s(x)) / dx_q| over (l, s): how far a step in x can move a sample's utility."""
    Xc, P = np.atleast_2d(Xc), np.atleast_2d(P)
    Zp, W = np.asarray(Zp, dtype=float), np.atleast_2d(W)
    thetas = np.atleast_2d(thetas)
    n, d = Xc.shape
    m, r, S, Lt = la.m, P.shape[0], W.shape[0], thetas.shape[0]
    p = np.full(Lt, 1.0 / Lt) if prob is None else np.asarray(prob, dtype=float)
    if best is None:
        best = best_so_far(la, thetas, kind, params)
    st = pending_state(la, P, Zp, max_tries)
    T, scale = thresholds(st["F"], thetas, best, kind, params)
    mu, s2 = la.mean(Xc), la.var_raw(Xc)                   # (m, n)
    c = la.cov(Xc, P)                                      # (m, n, r)
    if grad:
        dmu, ds2, dc = mean_grad(la, Xc), la.var_grad(Xc), la.cov_grad(Xc, P)       # (m, n, d), (m, n, d), (m, n, r, d)
    y = np.empty((S, m, n))
    dy = np.zeros((S, m, n, d)) if grad else None
    for j in range(m):
        Sj = 0.5 * (st["Sigma"][j] + st["Sigma"][j].T) + st["tau"][j] * np.eye(r)
        for i in range(n):
            cj = c[j, i]
            if route == "bordered":
                B = np.empty((r + 1, r + 1))
                B[:r, :r], B[:r, r], B[r, :r], B[r, r] = Sj, cj, cj, s2[j, i]
                clipped = False
                try:
                    LB = np.linalg.cholesky(B)
                    clipped = not LB[r, r] ** 2 > CLIP
                except np.linalg.LinAlgError:
                    clipped = True
                if clipped:
                    g = solve_triangular(st["L"][j], cj, lower=True)
                    B[r, r] = g.dot(g) + CLIP
                    LB = np.linalg.cholesky(B)
                lead, sv = LB[r, :r], LB[r, r]
                y[:, j, i] = mu[j, i] + Zp[:, j, :].dot(lead) + sv * W[:, j]
                if grad:
                    dlead = solve_triangular(LB[:r, :r], dc[j, i], lower=True)          # (r, d)
                    dv = np.zeros(d) if clipped else ds2[j, i] - 2.0 * lead.dot(dlead)
                    dy[:, j, i, :] = dmu[j, i] + Zp[:, j, :].dot(dlead) + np.outer(W[:, j], dv / (2.0 * sv))
            else:
                a = st["Q"][j].dot(cj)
                raw = s2[j, i] - cj.dot(a)
                v = max(raw, CLIP)
                y[:, j, i] = mu[j, i] + st["G"][:, j, :].dot(cj) + np.sqrt(v) * W[:, j]
                if grad:
                    dv = ds2[j, i] - 2.0 * a.dot(dc[j, i]) if raw > CLIP else np.zeros(d)
                    dy[:, j, i, :] = dmu[j, i] + st["G"][:, j, :].dot(dc[j, i]) + np.outer(W[:, j], dv / (2.0 * np.sqrt(v)))
    alpha, gap = np.zeros(n), np.full(n, np.inf)
    dalpha = np.zeros((n, d)) if grad else None
    slope = np.zeros(n)
    for l, th in enumerate(thetas):
        u = R.utility_eval(kind, th, y.transpose(1, 0, 2).reshape(m, S * n), params).reshape(S, n)
        scale = max(scale, float(np.max(np.abs(u))))
        diff = u - T[l][:, None]
        gap = np.minimum(gap, np.min(np.abs(diff), 0))
        alpha += p[l] / S * np.sum(np.maximum(diff, 0.0), 0)
        if grad:
            for s in range(S):
                for i in range(n):
                    du = R.utility_grad(kind, th, y[s, :, i], params).dot(dy[s, :, i, :])
                    slope[i] = max(slope[i], float(np.sum(np.abs(du))))
                    if diff[s, i] > 0.0:
                        dalpha[i] += p[l] / S * du
    out = dict(alpha=alpha, scale=scale, gap=gap, cond=st["cond"], F=st["F"], T=T, tau=st["tau"])
    if grad:
        out["dalpha"], out["slope"] = dalpha, slope
    return out


def qei(la, X, Z, thetas, prob, kind, params, best, diag):
    """Brute-force joint Monte-Carlo expected improvement of the point set X (q, d) with the joint normals Z (S, m, q):
    (1/S) sum_s sum_l p_l max(max_i U(theta_l, f_s(x_i)) - best_l, 0), f_s = mu(X) + chol(Sigma(X, X) + diag(diag_j)) Z_s; diag (m, q) is
    the jitter the conditional construction puts on the diagonal (tau_j on the pending points, nothing on the new one)."""
    X = np.atleast_2d(X)
    thetas = np.atleast_2d(thetas)
    q, m, S = X.shape[0], la.m, Z.shape[0]
    p = np.full(len(thetas), 1.0 / len(thetas)) if prob is None else np.asarray(prob, dtype=float)
    Sig, mu = la.cov(X, X), la.mean(X)
    f = np.empty((S, m, q))
    for j in range(m):
        Lj = np.linalg.cholesky(0.5 * (Sig[j] + Sig[j].T) + np.diag(diag[j]))
        f[:, j, :] = mu[j] + Z[:, j, :].dot(Lj.T)
    total = 0.0
    for l, th in enumerate(thetas):
        u = R.utility_eval(kind, th, f.transpose(1, 0, 2).reshape(m, S * q), params).reshape(S, q)
        total += p[l] / S * np.sum(np.maximum(u.max(1) - best[l], 0.0))
    return total


# ---- the device test's cases (tests/test_gpu_pending.py), shared with the CPU checks of their seeds (tests/test_pending_cpu.py)
MIXED = ["se", "matern52", "rbf", "matern32"]
#          N    d  m   r   S   L  H  C
SHAPES = [(200, 2, 1, 1, 1, 1, 1, 1),            # smallest of everything
          (200, 6, 4, 7, 64, 3, 1, 5),           # partial workgroup
          (200, 6, 4, 15, 65, 3, 3, 130),        # past one wave of samples, past one 128-column pad, table in LDS
          (500, 3, 4, 9, 256, 1, 1, 40),         # table > 64 KiB: the memory path
          (200, 4, 10, 3, 32, 2, 1, 9)]          # the runtime-m instantiation
UTILS = ["neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock"]
# Seeds, per shape in the order of UTILS.  The best-so-far comes from N observations, so most candidates of a random design improve on
# nothing; the seeds were searched on the CPU (tests/test_pending_cpu.py checks them) for cond(Sigma~) <= 1e4, at most 5 % of the candidates
# near a threshold, and a share of candidates with alpha > 0 as large as sixty seeds offered (for C = 1: that candidate).
SEEDS = [(249, 121, 197), (15, 3, 7, 19), (54, 49, 34, 41), (96, 106, 19, 157), (14, 57, 12, 12)]
CASES = [shape + (kind, SEEDS[i][k]) for i, shape in enumerate(SHAPES) for k, kind in enumerate(UTILS) if not (kind == "rosenbrock" and shape[2] % 2)]


def case_inputs(N, d, m, r, S, L, H, C, kind, seed):
    """Everything a case is made of, from its seed: the problem of kg_ref.problem with one kernel family per output, pending points,
    normals, utility parameters."""
    import kg_ref as K
    kinds = [MIXED[j % 4] for j in range(m)]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, seed, noise=1e-4)
    rng = np.random.RandomState(5000 + seed)
    P = rng.uniform(size=(r, d))
    Zp, W = rng.normal(size=(S, m, r)), rng.normal(size=(S, m))
    if kind == "rosenbrock":
        thetas = rng.uniform(0.2, 1.0, size=(L, 1))
    elif kind in ("neg_sum_exp", "neg_exp_cos"):
        thetas = np.zeros((L, 1))
    else:
        thetas = rng.uniform(-0.5, 0.5, size=(L, m))
    prob = None if L == 1 else rng.dirichlet(np.ones(L))
    params = rng.uniform(0.5, 1.0, size=m) if kind == "neg_exp_cos" else None
    return dict(kinds=kinds, X=X, Y=Y, var=var, ls=ls, nz=nz, Xc=Xc, P=P, Zp=Zp, W=W, thetas=thetas, prob=prob, params=params, kind=kind, H=H)


def case_lookaheads(inp):
    """One LookAhead per hyper-sample: sample h scales the variances by 1 + 0.1 h and the lengthscales by 1 - 0.05 h."""
    import kg_ref as K
    return [K.LookAhead.fit(inp["kinds"], inp["X"], inp["Y"], inp["var"] * (1 + 0.1 * h), inp["ls"] * (1 - 0.05 * h), inp["nz"])
            for h in range(inp["H"])]


def case_reference(inp, las, grad=False, route="bordered", n=None):
    """The restatement averaged over the hyper-samples, the best-so-far from hyper-sample 0 (the rule of the Monte-Carlo acquisitions:
    the hyper-sample current on entry).  n: only the first n candidates."""
    best = best_so_far(las[0], inp["thetas"], inp["kind"], inp["params"])
    Xc = inp["Xc"] if n is None else inp["Xc"][:n]
    rs = [pending(la, Xc, inp["P"], inp["Zp"], inp["W"], inp["thetas"], inp["prob"], inp["kind"], inp["params"], best=best, grad=grad, route=route)
          for la in las]
    out = dict(alpha=np.mean([r["alpha"] for r in rs], 0), gap=np.min([r["gap"] for r in rs], 0), scale=max(r["scale"] for r in rs),
               cond=max(r["cond"] for r in rs), F=np.concatenate([r["F"] for r in rs], 1), tau=np.concatenate([r["tau"] for r in rs]), best=best)
    if grad:
        out["dalpha"] = np.mean([r["dalpha"] for r in rs], 0)
    return out
