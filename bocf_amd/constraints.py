"""Linear constraints on the outputs of a composite problem: the simulator's outputs also decide whether a design is admissible (a stress,
a temperature, a budget computed by the same run).  OutputConstraints holds  A y - b <= 0  with a smoothing temperature per row; the
constrained acquisition (acquisitions.uEI_constrained) weighs every Monte-Carlo sample with them on the device."""
import numpy as np

MAX_CONSTRAINTS = 8


class OutputConstraints(object):
    """K linear constraints on the m outputs: y is feasible when  A y - b <= 0  in every row.

    :param A: (K, m), 1 <= K <= 8, every entry finite.
    :param b: (K,), every entry finite.
    :param eta: scalar or (K,): temperature of the logistic smoothing  s(-(A y - b)_k / eta_k)  the acquisition applies per sample;
        > 0 and finite.  eta -> 0 recovers the indicator of the feasible set.
    """

    def __init__(self, A, b, eta=1e-3):
        A = np.array(A, dtype=float)
        if A.ndim == 1:
            A = A[None, :]
        b = np.atleast_1d(np.array(b, dtype=float))
        if A.ndim != 2 or A.shape[1] < 1:
            raise ValueError("A must be (K, m)")
        K = A.shape[0]
        if not 1 <= K <= MAX_CONSTRAINTS:
            raise ValueError("1 .. %d constraints, got %d" % (MAX_CONSTRAINTS, K))
        if b.shape != (K,):
            raise ValueError("b must be (K,) = (%d,)" % K)
        eta = np.array(eta, dtype=float)
        if eta.ndim == 0:
            eta = np.full(K, float(eta))
        if eta.shape != (K,):
            raise ValueError("eta must be a scalar or (K,) = (%d,)" % K)
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
            raise ValueError("A and b must be finite")
        if not (np.all(np.isfinite(eta)) and np.all(eta > 0)):
            raise ValueError("eta must be finite and > 0")
        self.A, self.b, self.eta = np.ascontiguousarray(A), np.ascontiguousarray(b), np.ascontiguousarray(eta)

    @property
    def K(self):
        return self.A.shape[0]

    @property
    def m(self):
        return self.A.shape[1]

    @classmethod
    def bounds(cls, lower, upper, eta=1e-3):
        """Per-output boxes  lower_j <= y_j <= upper_j.  None or infinite entries add no row; lower / upper may be None altogether."""
        if lower is None and upper is None:
            raise ValueError("no bound given")
        m = len(lower) if lower is not None else len(upper)
        lower = [None] * m if lower is None else list(lower)
        upper = [None] * m if upper is None else list(upper)
        if len(lower) != m or len(upper) != m:
            raise ValueError("lower and upper must have one entry per output")
        rows, rhs = [], []
        for j in range(m):
            lo, hi = lower[j], upper[j]
            if hi is not None and np.isnan(hi) or lo is not None and np.isnan(lo):
                raise ValueError("a bound is NaN")
            if hi is not None and np.isfinite(hi):              # y_j - hi <= 0
                e = np.zeros(m)
                e[j] = 1.0
                rows.append(e)
                rhs.append(float(hi))
            if lo is not None and np.isfinite(lo):              # -y_j + lo <= 0
                e = np.zeros(m)
                e[j] = -1.0
                rows.append(e)
                rhs.append(-float(lo))
        if not rows:
            raise ValueError("every bound is None or infinite: no constraint")
        return cls(np.array(rows), np.array(rhs), eta)

    def values(self, Y):
        """c (K, n) = A Y - b for Y (m, n) (or (m,) -> (K,))."""
        Y = np.asarray(Y, dtype=float)
        if Y.shape[0] != self.m:
            raise ValueError("Y must have %d rows (one per output)" % self.m)
        return self.A.dot(Y) - (self.b if Y.ndim == 1 else self.b[:, None])

    def feasible(self, Y):
        """The hard test on Y (m, n): a boolean (n,), True where every constraint holds (a scalar bool for Y (m,))."""
        return np.all(self.values(Y) <= 0.0, axis=0)

    def key(self):
        return (self.A.shape, self.A.tobytes(), self.b.tobytes(), self.eta.tobytes())
