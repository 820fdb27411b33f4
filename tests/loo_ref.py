"""NumPy restatement of the leave-one-out cross-validation of the resident model (include/bocf_hip.h) on the
oracle's kernels and fits (oracle.cpu_ref.kern_K, GPFit).  TEST INFRASTRUCTURE ONLY.

Definitions (one output): Ky = K + (noise + shift) I with shift = 1e-8 + jitter, yc = y - mean(y) -- the centre and the hyper-parameters
are held when a point is left out, as ExactGaussianInference.LOO holds them (exact_gaussian_inference.py:67-79 works from the
existing posterior) --, and for training point i

    mu[i]   = mean(y) + k_i^T Ky_-i^-1 yc_-i
    s2[i]   = Ky_ii - k_i^T Ky_-i^-1 k_i              (the predictive variance with noise AND shift: 1 / (Ky^-1)_ii)
    var[i]  = s2[i] - shift  (with the likelihood noise),  s2[i] - shift - noise  (without)
    lpd[i]  = -0.5 log 2 pi - 0.5 log s2[i] - 0.5 (y_i - mu[i])^2 / s2[i]

loo_brute factorizes the N matrices Ky_-i explicitly (N = 1: the prior); loo_formula takes the same numbers from one factor of Ky.
"""
import functools

import numpy as np
import scipy.linalg

from oracle import cpu_ref as O

LOG_2PI = np.log(2.0 * np.pi)
FAMILIES = ("se", "rbf", "matern52", "matern32")


def train_matrix(kind, X, variance, lengthscale, noise, shift=1e-8):
    """The fit's own Ky (fp64, the oracle's kernel)."""
    Ky = O.kern_K(kind, np.atleast_2d(X), None, variance, lengthscale).copy()
    Ky[np.diag_indices_from(Ky)] += noise + shift
    return Ky


def _finish(y, ymean, s2, resid, noise, shift):
    """(mean, var with noise, var without, lpd) from s2 and resid = y - mu, in the dtype of s2."""
    half = s2.dtype.type(0.5)
    lpd = -half * s2.dtype.type(LOG_2PI) - half * np.log(s2) - half * resid * resid / s2
    return y - resid, s2 - shift, s2 - shift - noise, lpd


def _brute_f64(Ky, y, ymean):
    N = len(y)
    yc = y - ymean
    s2, resid = np.empty(N), np.empty(N)
    for i in range(N):
        keep = np.arange(N) != i
        if N == 1:
            s2[i], resid[i] = Ky[i, i], yc[i]
            continue
        L = np.linalg.cholesky(Ky[np.ix_(keep, keep)])
        v = scipy.linalg.solve_triangular(L, Ky[keep, i], lower=True)
        t = scipy.linalg.solve_triangular(L, yc[keep], lower=True)
        s2[i] = Ky[i, i] - v.dot(v)
        resid[i] = yc[i] - v.dot(t)
    return s2, resid


def _eliminate(T, steps):
    """`steps` columns of the hand-written right-looking Cholesky on the symmetric matrix T, in place: step k forms the factor's column k
    (below the pivot) and takes its outer product off the trailing block, which is then the Schur complement."""
    for k in range(steps):
        col = T[k + 1:, k] / np.sqrt(T[k, k])
        T[k + 1:, k + 1:] -= np.outer(col, col)


def _brute_ld(Ky, y, ymean):
    """Long double.  For point i the matrix [[Ky_-i, k_i, yc_-i], [k_i^T, Ky_ii, yc_i], [yc_-i^T, yc_i, 0]] takes the N - 1 elimination
    steps of the Cholesky factorization of Ky_-i; the two bordering rows are carried along (the forward substitutions), so the 2 x 2 block
    that is left holds s2[i] = Ky_ii - k_i^T Ky_-i^-1 k_i and y_i - mu[i] = yc_i - k_i^T Ky_-i^-1 yc_-i.  The elimination steps of the
    columns before i are the same numbers for every later i (a Cholesky factor's leading rows depend on the leading block only): they
    are taken once, on the bordered full matrix, instead of once per i -- the arithmetic of each factorization is unchanged."""
    ld = np.longdouble
    N = len(y)
    yc = y.astype(ld) - ld(ymean)
    A = np.zeros((N + 1, N + 1), dtype=ld)
    A[:N, :N] = Ky.astype(ld)
    A[:N, N] = A[N, :N] = yc
    s2, resid = np.empty(N, dtype=ld), np.empty(N, dtype=ld)
    for i in range(N):
        n = N + 1 - i                                      # trailing block: points i .. N - 1 and the target row
        perm = list(range(1, n - 1)) + [0, n - 1]          # point i behind the points that stay
        T = A[i:, i:][np.ix_(perm, perm)].copy()
        _eliminate(T, n - 2)
        s2[i], resid[i] = T[n - 2, n - 2], T[n - 2, n - 1]
        _eliminate(A[i:, i:], 1)                           # column i of the full matrix: shared by every later point
    return s2, resid


def loo_brute(kind, X, y, variance, lengthscale, noise, shift=1e-8, dtype=np.float64):
    """Brute force: (mean, var with noise, var without noise, lpd), each (N,), in `dtype` (np.float64: LAPACK per left-out point;
    np.longdouble: the hand-written Cholesky -- the truth).  The kernel matrix is the oracle's fp64 one in both."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ymean = y.mean()
    Ky = train_matrix(kind, X, variance, lengthscale, noise, shift)
    if dtype == np.float64:
        s2, resid = _brute_f64(Ky, y, ymean)
        return _finish(y, ymean, s2, resid, noise, shift)
    s2, resid = _brute_ld(Ky, y, ymean)
    return _finish(y.astype(np.longdouble), ymean, s2, resid, np.longdouble(noise), np.longdouble(shift))


def loo_formula(L, alpha, y, noise, shift=1e-8):
    """From one factor Ky = L L^T (lower) and alpha = Ky^-1 yc: c_i = (Ky^-1)_ii = sum_k (L^-1)[k][i]^2, mu = y - alpha / c,
    s2 = 1 / c.  Returns (mean, var with noise, var without noise, lpd)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    Linv = scipy.linalg.solve_triangular(L, np.eye(len(y)), lower=True)
    c = np.sum(Linv * Linv, axis=0)
    return y - alpha / c, 1.0 / c - shift, 1.0 / c - shift - noise, lpd_gpy(c, alpha)


def lpd_gpy(c, alpha):
    """exact_gaussian_inference.py:73-79 to the letter: neg_log_marginal_LOO = 0.5 log 2 pi - 0.5 log(diag Ky^-1) + 0.5 alpha^2 /
    diag Ky^-1, returned negated."""
    return -(0.5 * np.log(2 * np.pi) - 0.5 * np.log(c) + 0.5 * alpha ** 2 / c)


def loo_formula_fit(fit, y):
    """loo_formula on an oracle fit (cpu_ref.GPFit) of the targets y: its factor, its alpha, its jitter."""
    return loo_formula(fit.L, fit.alpha[:, 0], y, fit.noise_var, 1e-8 + fit.jitter)


def distances(got, want, noise, with_noise=True):
    """(mean: absolute, variance: relative to the with-noise variance, lpd: relative to 1 + |lpd|) between two (mean, var with noise,
    var without, lpd) tuples, in long double; the variance compared is the one `with_noise` selects."""
    g = [np.asarray(a, dtype=np.longdouble) for a in got]
    w = [np.asarray(a, dtype=np.longdouble) for a in want]
    k = 1 if with_noise else 2
    return (float(np.max(np.abs(g[0] - w[0]))), float(np.max(np.abs(g[k] - w[k]) / w[1])),
            float(np.max(np.abs(g[3] - w[3]) / (1 + np.abs(w[3])))))


# ---- one case: data, the oracle fits, the long-double truth and the floor, computed once and shared ----------------------------------
def problem(N, d, kinds, seed, lengthscale=0.4, noise=1e-3):
    rng = np.random.RandomState(seed)
    m = len(kinds)
    X = rng.uniform(0.0, 1.0, size=(N, d))
    Y = np.stack([np.sin(3.0 * X.sum(1) + j) + 0.5 * np.cos(5.0 * X[:, 0] * (j + 1)) + 0.05 * rng.normal(size=N) for j in range(m)], 0)
    var = 0.8 + 0.4 * np.arange(m)
    ls = np.stack([lengthscale * (1.0 + 0.25 * j) * (1.0 + 0.1 * np.arange(d)) for j in range(m)], 0)
    nz = noise * (1.0 + np.arange(m))
    return X, Y, var, ls, nz


@functools.lru_cache(maxsize=None)
def reference(N, d, kinds, seed, lengthscale=0.4, noise=1e-3, jitter=0.0):
    """For the problem of these arguments: per output the truth (long-double brute force), the oracle formula's results and the floor
    e_ref = their distances (mean, variance, lpd) -- made from references only.  Returns a dict; treat it as read-only."""
    X, Y, var, ls, nz = problem(N, d, kinds, seed, lengthscale, noise)
    truth, formula, floors = [], [], []
    for j, kind in enumerate(kinds):
        shift = 1e-8 + jitter
        t = loo_brute(kind, X, Y[j], var[j], ls[j], nz[j], shift, np.longdouble)
        Ky = train_matrix(kind, X, var[j], ls[j], nz[j], shift)
        L = np.linalg.cholesky(Ky)
        yc = Y[j] - Y[j].mean()
        alpha = scipy.linalg.cho_solve((L, True), yc)
        f = loo_formula(L, alpha, Y[j], nz[j], shift)
        truth.append(t)
        formula.append(f)
        floors.append(distances(f, t, nz[j]))
    return {"X": X, "Y": Y, "var": var, "ls": ls, "noise": nz, "truth": truth, "formula": formula, "floor": np.array(floors)}


def matern_problem(seed=2, N=40, d=2, m=2, lengthscale=0.3, noise=1e-2):
    """Data drawn from a Matern-3/2 prior (variance 1, this lengthscale) plus noise, for the kernel-selection tests: (X, Y (m, N),
    variance, lengthscale (d,), noise).  Seed 2 is one for which the oracle alone picks matern32 for both outputs under both criteria,
    with a margin above 3 nats (tests/test_loo_cpu.py checks that)."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    K = O.kern_K("matern32", X, None, 1.0, np.full(d, lengthscale))
    K[np.diag_indices_from(K)] += 1e-10
    C = np.linalg.cholesky(K)
    Y = np.stack([C.dot(rng.normal(size=N)) + np.sqrt(noise) * rng.normal(size=N) for _ in range(m)], 0)
    return X, Y, 1.0, np.full(d, lengthscale), noise


def oracle_tables(X, Y, variance, lengthscale, noise, families=FAMILIES):
    """(F, m) tables (leave-one-out log pseudo-likelihood, log marginal likelihood) of the oracle's fits, one family per row."""
    loo, lml = np.empty((len(families), len(Y))), np.empty((len(families), len(Y)))
    for f, kind in enumerate(families):
        for j, y in enumerate(Y):
            fit = O.GPFit(kind, X, y, variance, lengthscale, noise)
            loo[f, j], lml[f, j] = loo_formula_fit(fit, y)[3].sum(), fit.log_marginal
    return loo, lml


def gate(e_ref):
    """The bound of a device distance whose floor is e_ref: 100 e_ref, never tighter than 1e-13."""
    return max(100.0 * e_ref, 1e-13)


# ---- expected utility over the leave-one-out posteriors -----------------------------------------------------------------------------
def closed_form(kind, theta, mu, var):
    """E[U(theta, y)], y ~ N(mu, diag var), mu / var (m, n): the closed forms of include/bocf_hip.h (BOCF_EU_CLOSED)."""
    if kind == "neg_sq_dist":
        return -np.sum((mu.T - theta).T ** 2, axis=0) - var.sum(0)
    if kind == "neg_sum_exp":
        return -np.sum(np.exp(mu + 0.5 * var), axis=0)
    if kind == "rosenbrock":
        h = mu.shape[0] // 2
        return -(np.sum((theta[0] - mu[:h]) ** 2 + var[:h], axis=0) + 100.0 * np.sum(mu[h:2 * h] ** 2 + var[h:2 * h], axis=0))
    raise ValueError(kind)


def loo_expected_utility(mode, kind, thetas, mean, var, Z=None, params=None, func=None):
    """(L, N): E[U(theta_l, y)] under y ~ N(mean[:, i], diag var[:, i]).  mode "mean": theta . mean; "closed": closed_form; "mc": the
    MEAN over the S normals Z[l] (S, m) of U(theta_l, mean + sqrt(var) o z) through cpu_ref.utility_eval (or `func(theta, y)` for a
    utility program)."""
    thetas = np.atleast_2d(thetas)
    out = np.empty((thetas.shape[0], mean.shape[1]))
    for l, th in enumerate(thetas):
        if mode == "mean":
            out[l] = th.dot(mean)
        elif mode == "closed":
            out[l] = closed_form(kind, th, mean, var)
        else:
            sd = np.sqrt(var)
            acc = np.zeros(mean.shape[1])
            for z in Z[l]:
                y = mean + sd * z[:, None]
                acc += func(th, y) if func is not None else O.utility_eval(kind, th, y, params)
            out[l] = acc / len(Z[l])
    return out
