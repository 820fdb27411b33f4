"""NumPy restatement of the pathwise posterior samples, built on oracle.cpu_ref, and a long-double twin with its own
Cholesky solve.  Per output j and path s, with x~ = x / l_j:

    phi_f(x) = sqrt(2 s2 / F) cos(omega_f . x~ + b_f)
    g_s(x)   = sum_f phi_f(x) w_fs
    v_s      = Ky^-1 (yc - g_s(X) - sqrt(nug) E[:, s]),   nug = noise + 1e-8 + jitter
    f_s(x)   = ybar + g_s(x) + sum_i k(x, X_i) v_s[i]
"""
import numpy as np
from scipy.linalg import cho_solve

from oracle import cpu_ref as R

NU = {"matern52": 2.5, "matern32": 1.5}


def draw(kinds, N, d, F, S, rng=np.random):
    """The draws of one hyper-sample in multi_outputGP.draw_paths' order: per output z (F, d), chi2 (F,) for the Matern kinds only,
    b (F,), w (F, S), E (N, S).  Returns omega (m, F, d), phase (m, F), w (m, F, S), E (m, N, S)."""
    m = len(kinds)
    om, ph, w, E = np.empty((m, F, d)), np.empty((m, F)), np.empty((m, F, S)), np.empty((m, N, S))
    for j, kind in enumerate(kinds):
        z = rng.normal(size=(F, d))
        if kind in NU:
            z = z / np.sqrt(rng.chisquare(2.0 * NU[kind], size=F) / (2.0 * NU[kind]))[:, None]
        om[j] = z
        ph[j] = rng.uniform(0.0, 2.0 * np.pi, size=F)
        w[j] = rng.normal(size=(F, S))
        E[j] = rng.normal(size=(N, S))
    return om, ph, w, E


def features(o, omega, phase, Xq):
    """Phi (n, F) of one output (an oracle GPFit)."""
    F = omega.shape[0]
    return np.sqrt(2.0 * o.variance / F) * np.cos((Xq / o.lengthscale).dot(omega.T) + phase)


def nugget(o):
    return o.noise_var + 1e-8 + o.jitter


class Paths(object):
    """S paths of every output of an oracle MultiOutputGPRef from the draws (omega, phase, w, E); Y: the list of (N, 1) targets."""

    def __init__(self, ref, Y, omega, phase, w, E):
        self.ref, self.omega, self.phase, self.w, self.E = ref, omega, phase, w, E
        self.v = []
        for j, o in enumerate(ref.output):
            yc = np.asarray(Y[j], dtype=float).reshape(-1, 1) - o.ymean
            rhs = yc - features(o, omega[j], phase[j], o.X).dot(w[j]) - np.sqrt(nugget(o)) * E[j]
            self.v.append(cho_solve((o.L, True), rhs))

    def values(self, Xq):
        """(m, n, S)"""
        Xq = np.atleast_2d(Xq)
        out = []
        for j, o in enumerate(self.ref.output):
            Kx = R.kern_K(o.kind, Xq, o.X, o.variance, o.lengthscale)
            out.append(o.ymean + features(o, self.omega[j], self.phase[j], Xq).dot(self.w[j]) + Kx.dot(self.v[j]))
        return np.stack(out)

    def gradients(self, Xq, paths=None):
        """(m, n, S', d): d f_js(x_i) / dx for the paths listed (all by default)."""
        Xq = np.atleast_2d(Xq)
        n, d = Xq.shape
        S = self.w[0].shape[1]
        paths = range(S) if paths is None else paths
        out = np.empty((len(self.ref.output), n, len(paths), d))
        for j, o in enumerate(self.ref.output):
            F = self.omega[j].shape[0]
            arg = (Xq / o.lengthscale).dot(self.omega[j].T) + self.phase[j]
            dphi = -np.sqrt(2.0 * o.variance / F) * np.sin(arg)                      # (n, F)
            for a, s in enumerate(paths):
                gk = R.kern_gradients_X(o.kind, np.tile(self.v[j][:, s], (n, 1)), Xq, o.X, o.variance, o.lengthscale)
                gf = (dphi * self.w[j][:, s]).dot(self.omega[j]) / o.lengthscale
                out[j, :, a, :] = gk + gf
        return out

    def utility(self, X, row_path, thetas, util, params=None, grad=False):
        """u_i = U(thetas[row_path[i]], f_{., row_path[i]}(X_i)) and its input gradient (n, d)."""
        X = np.atleast_2d(X)
        n, d = X.shape
        F = self.values(X)
        val, dval = np.empty(n), np.empty((n, d))
        for i in range(n):
            s = int(row_path[i])
            y = F[:, i, s]
            val[i] = R.utility_eval(util, thetas[s], y, params)
            if grad:
                g = self.gradients(X[i:i + 1], [s])[:, 0, 0, :]                       # (m, d)
                dval[i] = np.asarray(R.utility_grad(util, thetas[s], y, params)).dot(g)
        return (val, dval) if grad else val


# ---- long-double twin --------------------------------------------------------------------------------------------------------------
LD = np.longdouble


def _kern_ld(kind, X1, X2, variance, ls):
    D = (X1[:, None, :] - X2[None, :, :]) / ls
    r2 = np.sum(D * D, axis=2)
    if kind in ("rbf", "se"):
        return variance * np.exp(-r2 / LD(2))
    r = np.sqrt(r2)
    if kind == "matern52":
        s5 = np.sqrt(LD(5))
        return variance * (1 + s5 * r + LD(5) / LD(3) * r2) * np.exp(-s5 * r)
    s3 = np.sqrt(LD(3))
    return variance * (1 + s3 * r) * np.exp(-s3 * r)


def _chol_ld(A):
    n = A.shape[0]
    L = np.zeros_like(A)
    for k in range(n):
        L[k, k] = np.sqrt(A[k, k] - np.dot(L[k, :k], L[k, :k]))
        if k + 1 < n:
            L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k].dot(L[k, :k])) / L[k, k]
    return L


def _solve_ld(L, B):
    n = L.shape[0]
    Y = np.zeros_like(B)
    for k in range(n):
        Y[k] = (B[k] - L[k, :k].dot(Y[:k])) / L[k, k]
    Xs = np.zeros_like(B)
    for k in range(n - 1, -1, -1):
        Xs[k] = (Y[k] - L[k + 1:, k].dot(Xs[k + 1:])) / L[k, k]
    return Xs


def values_ld(ref, Y, omega, phase, w, E, Xq):
    """Paths.values in long double throughout (kernel, features, Cholesky factor and solve of its own); returns (m, n, S) long double."""
    Xq = np.atleast_2d(Xq).astype(LD)
    out = []
    for j, o in enumerate(ref.output):
        X, ls, var = o.X.astype(LD), o.lengthscale.astype(LD), LD(o.variance)
        N, F = X.shape[0], omega[j].shape[0]
        nug = LD(o.noise_var) + LD(1e-8) + LD(o.jitter)
        y = np.asarray(Y[j], dtype=float).reshape(-1, 1).astype(LD)
        ybar = LD(o.ymean)
        amp = np.sqrt(LD(2) * var / LD(F))
        om, ph, wj, Ej = omega[j].astype(LD), phase[j].astype(LD), w[j].astype(LD), E[j].astype(LD)
        phi = lambda Z: amp * np.cos((Z / ls).dot(om.T) + ph)
        Ky = _kern_ld(o.kind, X, X, var, ls) + nug * np.eye(N, dtype=LD)
        rhs = (y - ybar) - phi(X).dot(wj) - np.sqrt(nug) * Ej
        v = _solve_ld(_chol_ld(Ky), rhs)
        out.append(ybar + phi(Xq).dot(wj) + _kern_ld(o.kind, Xq, X, var, ls).dot(v))
    return np.stack(out)
