"""The problems the pivot-breakdown tests share (tests/test_breakdown_cpu.py, tests/test_gpu_breakdown.py): matrices Ky that lose positive
definiteness at ONE known pivot k, whatever the summation order of the factorization, with everything the tests expect of them taken
from the oracle alone (LAPACK's info, jitchol's rung, the reference pivots).  Test infrastructure only: nothing under bocf_amd/ imports it.

The construction: X uniform in [0, 1]^d with short lengthscales (K far from singular), one repeated point X[k] = X[i] (i < k), noise 0
and the probes build's diagonal shift 1e-8 + DELTA, so that Ky = K - DELTA I.  In exact arithmetic pivot k is then ~ -2 DELTA while every
earlier pivot stays near its unshifted value; jitchol's rungs (1 - DELTA) 1e-6 10^r lift pivot k by twice the rung, so the rungs 1e-6, 1e-5
and 1e-4 fail at the same k and 1e-3 succeeds: the unjittered attempt and THREE retries return k + 1, the FOURTH retry factorizes
(max_jitter_tries counts retries, as jitchol's maxtries does: TRIES_NEEDED = 4).  Every problem asserts its preconditions on the
reference pivots before it is handed out: a problem whose breakdown position could depend on rounding is refused here, not by the device."""
import functools
import types

import numpy as np
from scipy.linalg import lapack, solve_triangular

from oracle import cpu_ref as R

DELTA = 3e-4
SHIFT = 1e-8 + DELTA                                    # what option test_diag_shift_1e12 takes off diag(Ky): Ky = K + noise I - DELTA I
SHIFT_OPTION = int(round(SHIFT * 1e12))
TRIES_NEEDED = 4                                        # retries of the ladder until pivot k is positive (asserted per problem)
# a shift no rung of the model layer's five survives (pivot k ~ -2 (DELTA_EXHAUST - 1e-2)): jitchol raises, positions are not compared
DELTA_EXHAUST = 2e-2
SHIFT_EXHAUST_OPTION = int(round((1e-8 + DELTA_EXHAUST) * 1e12))
HEALTHY_NOISE = 1e-2

# shape -> input dimension, lengthscale, kernel family, outputs (the N = 128, d = 3 trial was too dense: an early pivot of 2.6e-5)
# (... and so is N = 600 at d = 4: an early pivot of 6e-3; one more dimension thins it out)
SHAPES = {128: (4, 0.15, "matern52", 1), 300: (4, 0.15, "matern52", 1), 600: (5, 0.15, "se", 1), 3100: (6, 0.12, "rbf", 2)}
# the breakdown positions per shape: strip (k mod 4), 16-block and last-row edges of the diagonal-block kernel at one panel; first row,
# both sides of every panel edge and the last (ragged) row at three panels; at 25 panels the launched / team-group part, the two sides
# of the hybrid split (block row 16) and the last row of the tail's ragged last panel
POSITIONS = {128: (1, 3, 4, 15, 16, 17, 63, 64, 127), 300: (1, 127, 128, 129, 255, 256, 299), 600: (1, 127, 128, 129, 255, 256, 599),
             3100: (200, 2047, 2048, 3099)}
# (k1, k2) of the per-output problems: output 1 breaks at k1, output 2 at k2 < k1 -- different panels, and at 25 panels the tail / the first part
ARD_POSITIONS = {300: (270, 133), 3100: (2500, 1000)}
ARD_SHAPES = {300: (5, 0.15), 3100: (7, 0.12)}          # one coordinate of a breaking output is switched off (lengthscale 1e6): d - 1 remain
KEEP_KY = 600                                           # the reference matrices are kept up to this size (77 MB each at N = 3100)


def shifted_Ky(kind, X, variance, lengthscale, noise, shift=SHIFT):
    """What the device factorizes under the diagonal shift: K + (noise + 1e-8 - shift) I."""
    Ky = R.kern_K(kind, X, None, variance, lengthscale)
    Ky[np.diag_indices_from(Ky)] += noise + 1e-8 - shift
    return Ky


def reference_pivots(Ky, k, jitter=0.0):
    """The pivots 0 .. k - 1 of Ky + jitter I and its pivot k, from LAPACK's factor of the leading k x k block (which must be positive
    definite) and the Schur complement of entry (k, k)."""
    if k == 0:
        return np.zeros(0), Ky[0, 0] + jitter
    A = Ky[:k, :k].copy()
    A[np.diag_indices_from(A)] += jitter
    L = np.linalg.cholesky(A)
    v = solve_triangular(L, Ky[:k, k], lower=True)
    return np.diag(L) ** 2, Ky[k, k] + jitter - v.dot(v)


def lapack_info(Ky):
    return int(lapack.dpotrf(np.ascontiguousarray(Ky), lower=1)[1])


def check_breaks_at(Ky, k):
    """The preconditions, from the reference alone: every pivot before k >= 100 DELTA, pivot k <= -DELTA, LAPACK reports k + 1; jitchol
    stops at the rung TRIES_NEEDED retries reach, where pivot k >= DELTA.  Returns (jitter of that rung, the figures)."""
    before, piv = reference_pivots(Ky, k)
    assert before.size == 0 or before.min() >= 100 * DELTA, (k, before.min())
    assert piv <= -DELTA, (k, piv)
    assert lapack_info(Ky) == k + 1, (k, lapack_info(Ky))
    jitter = R.jitchol(Ky)[1]
    assert abs(jitter / (np.diag(Ky).mean() * 1e-6 * 10.0 ** (TRIES_NEEDED - 1)) - 1.0) < 1e-14, jitter
    before_j, piv_j = reference_pivots(Ky, k, jitter)
    assert piv_j >= DELTA and (before_j.size == 0 or before_j.min() >= 100 * DELTA), (k, piv_j)
    # ... and the rung before it still breaks at k, by the same margin
    before_f, piv_f = reference_pivots(Ky, k, jitter / 10)
    assert piv_f <= -DELTA and (before_f.size == 0 or before_f.min() >= 100 * DELTA), (k, piv_f)
    return jitter, dict(min_before=float(before.min()) if before.size else np.inf, pivot=float(piv), pivot_at_rung=float(piv_j), pivot_below_rung=float(piv_f))


def check_healthy(Ky):
    """No pivot anywhere near zero (a repeated point under noise 1e-2 has the pivot 2 (1e-2 - DELTA) = 65 DELTA; rounding moves a pivot
    by ~1e-13): no attempt at such a matrix fails, whatever the summation order."""
    assert lapack_info(Ky) == 0
    assert (np.diag(np.linalg.cholesky(Ky)) ** 2).min() >= 10 * DELTA


def _targets(X, m):
    """Smooth targets of the inputs (a repeated point repeats its target: alpha stays moderate on the jittered rung)."""
    return np.stack([np.sin(3.0 * X.sum(1) + j) for j in range(m)])


def _base(N, d, seed):
    return np.random.RandomState(seed).uniform(size=(N, d))


@functools.lru_cache(maxsize=None)
def single(N, k):
    """Every output breaks at pivot k (the outputs share the hyper-parameters and differ in their targets; two rows of targets are
    handed out whatever m, for the callers that fit the problem with two outputs).  Read-only."""
    d, ls, kind, m = SHAPES[N]
    X_clean = _base(N, d, 9100 + N)
    X = X_clean.copy()
    X[k] = X[k // 2]
    Ky = shifted_Ky(kind, X, 1.0, ls, 0.0)
    jitter, figures = check_breaks_at(Ky, k)
    check_healthy(shifted_Ky(kind, X_clean, 1.0, ls, 0.0, shift=0.0))
    # the exhausted ladder of the model layer: no positions compared, only that the reference gives up as well
    exhausted = None
    if N <= KEEP_KY:
        try:
            R.jitchol(shifted_Ky(kind, X, 1.0, ls, 0.0, shift=1e-8 + DELTA_EXHAUST))
            exhausted = False
        except Exception as e:                          # noqa: BLE001  (scipy's LinAlgError)
            exhausted = "even with jitter" in str(e)
    return types.SimpleNamespace(
        N=N, d=d, m=m, k=k, kind=kind, X=X, X_clean=X_clean, Y=_targets(X, max(m, 2)), Y_clean=_targets(X_clean, max(m, 2)), variance=np.ones(m), lengthscale=np.full((m, d), ls),
        noise=np.zeros(m), info=[k + 1] * m, rc=k + 1, jitter=np.full(m, jitter), figures=figures, reference_gives_up_at_exhaust=exhausted,
        Ky=Ky if N <= KEEP_KY else None)


@functools.lru_cache(maxsize=None)
def per_output(N):
    """Three ARD outputs over two near-pairs: (i1, k1) differ only in coordinate 0, (i2, k2) only in coordinate 1, by 0.1.  An output
    sees a pair as a repeated point only where its lengthscale in that coordinate is 1e6 (kernel value 1 - O(1e-14)): output 0 (noise
    1e-2) never breaks, output 1 breaks at k1, output 2 at k2 < k1.  `healthy_noise` makes every output healthy (noise 1e-2)."""
    d, ls = ARD_SHAPES[N]
    k1, k2 = ARD_POSITIONS[N]
    X_clean = _base(N, d, 9300 + N)
    X = X_clean.copy()
    for k, q in ((k1, 0), (k2, 1)):
        X[k] = X[k // 2]
        X[k, q] += 0.1 if X[k, q] < 0.9 else -0.1
    lengthscale = np.full((3, d), ls)
    lengthscale[1, 0] = 1e6
    lengthscale[2, 1] = 1e6
    noise = np.array([HEALTHY_NOISE, 0.0, 0.0])
    jitter, figures, Kys = np.zeros(3), [None] * 3, [None] * 3
    for j, k in ((1, k1), (2, k2)):
        Ky = shifted_Ky("rbf", X, 1.0, lengthscale[j], 0.0)
        jitter[j], figures[j] = check_breaks_at(Ky, k)
        Kys[j] = Ky if N <= KEEP_KY else None
    Ky0 = shifted_Ky("rbf", X, 1.0, lengthscale[0], HEALTHY_NOISE)
    check_healthy(Ky0)
    Kys[0] = Ky0 if N <= KEEP_KY else None
    return types.SimpleNamespace(
        N=N, d=d, m=3, k=(None, k1, k2), kind="rbf", X=X, X_clean=X_clean, Y=_targets(X, 3), Y_clean=_targets(X_clean, 3), variance=np.ones(3), lengthscale=lengthscale,
        noise=noise, healthy_noise=np.full(3, HEALTHY_NOISE), info=[0, k1 + 1, k2 + 1], rc=k1 + 1, jitter=jitter, figures=figures, Ky=Kys)

