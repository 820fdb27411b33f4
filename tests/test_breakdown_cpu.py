"""The breakdown cases of tests/test_gpu_breakdown.py can tell a wrong position from a right one: on the oracle alone, every problem the
GPU file lists breaks down at exactly the pivot it names (LAPACK's info is k + 1, by a margin of DELTA against pivots of >= 100 DELTA
before it), jitchol climbs to the rung the GPU file expects, and that rung is the FOURTH retry -- GPy's maxtries and the library's
max_jitter_tries both count retries, so three of them still return k + 1.  No GPU needed.

Not among the cases: a non-finite input row.  X[r] = NaN leaves the diagonal of K finite (a stationary kernel's diagonal is the variance,
here as on the device) and makes row and column r NaN; the LAPACK behind scipy (OpenBLAS: `ajj <= 0`, no isnan) then reports info = 0
for r = 0, 1 and 129 at N = 300 and returns a factor full of NaN, and a LAPACK that did test for NaN would name pivot 1, not 0, for
r = 0.  With no reference position to compare against, the device's answer for such a row is not pinned here."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg
from scipy.linalg import lapack

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breakdown_problem as P  # noqa: E402

from oracle import cpu_ref as R  # noqa: E402

CASES = [(N, k) for N in sorted(P.POSITIONS) for k in P.POSITIONS[N]]


@pytest.mark.parametrize("N,k", CASES)
def test_every_case_breaks_down_at_its_pivot_only(N, k):
    """The builder's own asserts (reference pivots before k >= 100 DELTA, pivot k <= -DELTA, >= DELTA at the succeeding rung and
    <= -DELTA at the rung below it, the duplicate-free X healthy) and what it hands out.  Measured: pivot k is -6.0009e-4 .. -6.0012e-4
    in every case, +1.3987e-3 .. 1.3990e-3 at the fourth rung; the smallest earlier pivot is 0.106 (N = 3100, k = 3099)."""
    p = P.single(N, k)
    f = p.figures
    print("N %d k %d: min pivot before %.4g, pivot k %.6g, at the rung %.6g, one rung below %.6g" % (N, k, f["min_before"], f["pivot"], f["pivot_at_rung"],
                                                                                                       f["pivot_below_rung"]))
    assert p.info == [k + 1] * p.m and p.rc == k + 1
    assert f["min_before"] >= 100 * P.DELTA and f["pivot"] <= -P.DELTA and f["pivot_at_rung"] >= P.DELTA and f["pivot_below_rung"] <= -P.DELTA
    assert p.jitter[0] == pytest.approx((1.0 - P.DELTA) * 1e-3, rel=1e-12)
    assert np.array_equal(p.X[k], p.X[k // 2]) and np.array_equal(np.delete(p.X, k, 0), np.delete(p.X_clean, k, 0))


@pytest.mark.parametrize("N,k", [c for c in CASES if c[0] <= P.KEEP_KY])
def test_lapack_reports_the_position_in_both_forms_and_jitchol_the_rung(N, k):
    """dpotrf, lower and upper (the device factorizes the upper form), reports info == k + 1 and numpy raises; jitchol with three retries
    gives up, with four it returns the rung (1 - DELTA) 1e-3 -- the device's max_jitter_tries 0 .. 3 must return k + 1, 4 must succeed."""
    Ky = P.single(N, k).Ky
    for lower in (0, 1):
        assert lapack.dpotrf(Ky, lower=lower)[1] == k + 1
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(Ky)
    with pytest.raises(scipy.linalg.LinAlgError):
        R.jitchol(Ky, maxtries=P.TRIES_NEEDED - 1)
    L, jitter = R.jitchol(Ky, maxtries=P.TRIES_NEEDED)
    assert jitter == pytest.approx((1.0 - P.DELTA) * 1e-3, rel=1e-12)
    np.testing.assert_allclose(L.dot(L.T), Ky + jitter * np.eye(N), rtol=0, atol=1e-12)
    assert P.single(N, k).reference_gives_up_at_exhaust is True          # the shift of the model-layer test: all five rungs fail


@pytest.mark.parametrize("N", sorted(P.ARD_POSITIONS))
def test_per_output_positions(N):
    """The ARD construction: output 0 never breaks, output 1 breaks at k1, output 2 at k2 < k1 (preconditions per output inside the
    builder); the first failing OUTPUT's info is k1 + 1, which is not the smallest position."""
    p = P.per_output(N)
    k1, k2 = P.ARD_POSITIONS[N]
    assert k2 < k1 and k1 // 128 != k2 // 128
    assert p.info == [0, k1 + 1, k2 + 1] and p.rc == k1 + 1 and p.rc != min(v for v in p.info if v)
    assert p.jitter[0] == 0.0 and p.jitter[1] == pytest.approx((1.0 - P.DELTA) * 1e-3, rel=1e-12) and p.jitter[2] == p.jitter[1]
    for j in (1, 2):
        print("N %d output %d: %s" % (N, j, p.figures[j]))
    if N <= P.KEEP_KY:
        assert [P.lapack_info(Ky) for Ky in p.Ky] == p.info
        # the pair an output does NOT see as a repeated point is an ordinary pair to it: kernel value exp(-0.5 (0.1 / 0.15)^2) = 0.80
        assert 0.75 < p.Ky[1][k2, k2 // 2] < 0.85 and 0.75 < p.Ky[2][k1, k1 // 2] < 0.85
        assert 1.0 - p.Ky[1][k1, k1 // 2] < 1e-13 and 1.0 - p.Ky[2][k2, k2 // 2] < 1e-13
        # with every output healthy (noise 1e-2) nothing breaks
        for j in range(3):
            P.check_healthy(P.shifted_Ky("rbf", p.X, 1.0, p.lengthscale[j], P.HEALTHY_NOISE))


def test_positions_cover_the_edges_the_kernels_have():
    """One panel: both sides of a strip (k mod 4) and of a 16-block, the last row.  Several panels: both sides of every panel edge, the
    last ragged row; at 25 panels both sides of the hybrid split (the largest power of two below 25 is 16: row 2048)."""
    one = P.POSITIONS[128]
    assert {3, 4} <= set(one) and {15, 16, 17} <= set(one) and {63, 64} <= set(one) and 127 in one
    for N in (300, 600):
        ks = P.POSITIONS[N]
        assert {127, 128, 129, 255, 256} <= set(ks) and N - 1 in ks and N % 128 != 0
    big = P.POSITIONS[3100]
    assert {2047, 2048} <= set(big) and 3099 in big and min(big) < 2048 - 128 and -(-3100 // 128) == 25
