"""NumPy statement of the removal of one observation from a Cholesky factor and its inverse, shared by
tests/test_remove_cpu.py and tests/test_gpu_remove.py.

U is upper triangular with Ky = U^T U, R = U^-1.  Row k of R fixes every plane rotation; `remove` applies them one after the other as the
derivation states them, `remove_prefix` is the form the device kernels evaluate (the carry of the chain as a prefix dot product with r).
Both return (U', R') of the N - 1 remaining observations with exact zeros below the diagonal."""
import numpy as np


def rotations(r, k):
    """t (prefix norms of r[k:]), c, s of the N - 1 - k plane rotations: t_k = r[k], t_{j+1} = hypot(t_j, r[j+1]), c_j = r[j+1] / t_{j+1},
    s_j = t_j / t_{j+1}.  c and s are indexed by j (entries in front of k unused)."""
    N = r.shape[0]
    t, c, s = np.zeros(N), np.zeros(N), np.zeros(N)
    t[k] = r[k]
    for j in range(k, N - 1):
        t[j + 1] = np.hypot(t[j], r[j + 1])
        c[j], s[j] = r[j + 1] / t[j + 1], t[j] / t[j + 1]
    return t, c, s


def remove(U, R, k):
    """Scan, reflections, dropped row / column.  U, R: (N, N) upper triangular."""
    N = U.shape[0]
    assert N >= 2 and 0 <= k < N
    r = R[k].copy()
    assert r[k] > 0 and not np.any(r[:k])
    _, c, s = rotations(r, k)
    Un = np.delete(U, k, axis=1)                           # (N, N - 1)
    Rn = np.delete(R, k, axis=0)                           # (N - 1, N)
    for j in range(k, N - 1):
        a, b = Un[j].copy(), Un[j + 1].copy()
        Un[j], Un[j + 1] = s[j] * b - c[j] * a, s[j] * a + c[j] * b
        a, b = Rn[:, j].copy(), Rn[:, j + 1].copy()
        Rn[:, j], Rn[:, j + 1] = s[j] * b - c[j] * a, s[j] * a + c[j] * b
    last_row = np.abs(Un[N - 1]).max() if N > 1 else 0.0   # zero up to rounding: dropped
    Un, Rn = np.triu(Un[:N - 1]), np.triu(Rn[:, :N - 1])   # zero by construction below the diagonal
    return Un, Rn, last_row


def remove_prefix(U, R, k):
    """The same update as the kernels evaluate it: with x a column of U (by row) or a row of R (by column),
    out[j] = x[j] (j < k), out[j] = s_j x[j+1] - (c_j / t_j) sum_{q = k .. j} r[q] x[q] (k <= j <= N - 2); R' takes its diagonal from 1 / diag U'."""
    N = U.shape[0]
    r = R[k].copy()
    t = np.zeros(N)
    t[k:] = np.sqrt(np.cumsum(r[k:] ** 2))
    s, g = np.zeros(N), np.zeros(N)
    s[k:N - 1] = t[k:N - 1] / t[k + 1:]
    g[k:N - 1] = r[k + 1:] / (t[k + 1:] * t[k:N - 1])

    def columns(M):                                        # recurrence down the rows of every column of M (N, n)
        acc = np.cumsum(r[:, None] * M, axis=0)            # r is zero in front of k
        out = M[:N - 1].copy()
        out[k:] = s[k:N - 1, None] * M[k + 1:] - g[k:N - 1, None] * acc[k:N - 1]
        return out
    Un = np.triu(columns(np.delete(U, k, axis=1)))
    Rn = np.triu(columns(np.delete(R, k, axis=0).T).T, 1)
    Rn[np.arange(N - 1), np.arange(N - 1)] = 1.0 / np.diag(Un)
    return Un, Rn


# The cases of the removal's boundary test on the device (tests/test_gpu_remove.py) -- N, removed index k, outputs m, input dimension d,
# kernel family (or "mixed": five families), noise -- kept here so that tests/test_remove_cpu.py can show on the oracle alone that each
# removal changes the posterior by more than the gates.  Every N with k = 0 and k = N - 1; every tile-edge k at N = 385.
BOUNDARY = [
    (2, 0, 1, 1, "rbf", 1e-6), (2, 1, 5, 6, "mixed", 1e-2),
    (128, 0, 5, 1, "mixed", 1e-6), (128, 127, 1, 6, "matern52", 1e-2),
    (129, 0, 1, 6, "matern32", 1e-6), (129, 128, 5, 1, "mixed", 1e-2),
    (256, 0, 1, 1, "matern52", 1e-2), (256, 255, 5, 6, "mixed", 1e-6),
    (257, 0, 5, 6, "mixed", 1e-2), (257, 256, 1, 1, "rbf", 1e-6),
    (385, 0, 1, 6, "rbf", 1e-6), (385, 384, 5, 1, "mixed", 1e-2),
    (385, 127, 1, 1, "matern32", 1e-2), (385, 128, 5, 6, "mixed", 1e-6), (385, 129, 1, 6, "se", 1e-2), (385, 383, 1, 1, "matern52", 1e-6),
    (640, 0, 5, 6, "mixed", 1e-6), (640, 639, 1, 1, "rbf", 1e-2),
]
# seeds: 300 + N + m + 1000 s with the first s at which the oracle factorizes the N - 1 remaining points with zero jitter and no
# log-marginal cancels (test_gpu_incremental.lml_cancellation); found on the CPU, asserted by the tests
SEED_SHIFT = {(128, 0, 5): 5}


def boundary_seed(N, k, m):
    return 300 + N + m + 1000 * SEED_SHIFT.get((N, k, m), 0)


def without(p, k, n=None):
    """(X, Ys) of the first n observations of problem p with row k deleted."""
    X = p["X"] if n is None else p["X"][:n]
    Ys = [y if n is None else y[:n] for y in p["Y"]]
    return np.delete(X, k, axis=0), [np.delete(y, k, axis=0) for y in Ys]


def make_outlier(p, k):
    """Observation k of problem p becomes one worth removing: its targets move by 1 and the first candidate sits on it, so that the
    posterior with and without it differs at the candidates by far more than any gate (asserted in tests/test_remove_cpu.py)."""
    p["Y"] = [y.copy() for y in p["Y"]]
    for y in p["Y"]:
        y[k] += 1.0
    p["Xc"] = p["Xc"].copy()
    p["Xc"][0] = p["X"][k]
    return p
