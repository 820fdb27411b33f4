"""The batch acquisition step after the tile queue of the variance contraction and the full-tile loop of the cross kernel:
means, variances and uEI values must not depend on the tiling of the contraction (256-row tiles worked through as a queue by
one workgroup per compute unit / 128-row tiles, one workgroup each), on the chunking of the candidates, or on which call of
a sequence computed them (the queue's counters are left re-armed by every launch), bit for bit; and a candidate's K* column
and mean must not depend on whether its workgroup took the cross kernel's full-tile loop or the guarded one.
Run on the MI355X box:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu

D, S, CMAX = 8, 64, 16384
KERNELS = {"rbf": "RBF", "matern52": "Matern52"}


@pytest.fixture(scope="module")
def B():
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


_cache = {}


def _setup(B, kind, N, m):
    """One fitted model, its acquisition and the oracle's variances of the first 256 candidates per (kernel, N, m): the three
    candidate counts of a case are prefixes of the same batch."""
    key = (kind, N, m)
    if key not in _cache:
        _cache.clear()                                   # (one resident model at a time)
        p = R.synthetic_problem(N, D, m, CMAX, S, 4100 + N + m, noise=1e-5)
        cls = getattr(B.kern, KERNELS[kind])
        kern = [cls(D, variance=p["variances"][j], lengthscale=p["lengthscales"][j], ARD=True) for j in range(m)]
        model = B.multi_outputGP(m, kernel=kern, noise_var=list(p["noise"]), fixed_hyps=True)
        model.updateModel(p["X"], p["Y"])
        theta = np.array([[0.2 * (j + 1) for j in range(m)]])
        U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=np.ones(1)), device="neg_sq_dist")
        acq = B.uEI_noiseless(model, None, utility=U)
        acq.W_samples = p["W"]
        ref = R.MultiOutputGPRef(kind, p["variances"], p["lengthscales"], p["noise"])
        ref.updateModel(p["X"], p["Y"])
        _cache[key] = (p, model, acq, ref.predict(p["Xc"][:256])[1])
    return _cache[key]


def _step(model, acq, Xc):
    mean, var = model.predict(Xc)
    return mean, var, acq._compute_acq(Xc)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("mean", "variance", "uEI")):
        assert g.shape == w.shape
        assert g.tobytes() == w.tobytes(), "%s differs (%s): max |diff| %.3e" % (name, what, np.abs(g - w).max())


# 5000: ragged last column tile; 2304: the padded N is no multiple of 256, so the launcher falls back to 128-row tiles
@pytest.mark.parametrize("C", [2048, 5000, 16384])
@pytest.mark.parametrize("m", [1, 4])
@pytest.mark.parametrize("N", [1024, 2304, 4096])
@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_step_is_bit_identical_across_tilings_chunks_and_calls(B, kind, N, m, C):
    p, model, acq, ref_var = _setup(B, kind, N, m)
    Xc = p["Xc"][:C]
    model.set_option("swizzle", -1)
    model.set_option("chunk", 65536)
    first = _step(model, acq, Xc)
    _same(_step(model, acq, Xc), first, "second of two consecutive calls")
    try:
        model.set_option("swizzle", 0)
        _same(_step(model, acq, Xc), first, "swizzle = 0")
        model.set_option("swizzle", -1)
        model.set_option("chunk", 2048)
        _same(_step(model, acq, Xc), first, "chunk = 2048")
    finally:
        model.set_option("swizzle", -1)
        model.set_option("chunk", 65536)
    _same(_step(model, acq, Xc), first, "default tiling again, after the other tilings")
    assert np.isfinite(first[2]).all() and first[1].min() >= 1e-10
    # the tolerances of tests/test_gpu_parity.py::test_variance_gemm_tilings_are_bit_identical for the same quantity
    np.testing.assert_allclose(first[1][:, :256], ref_var, rtol=1e-4, atol=1e-8)


# The cross kernel's full-tile loop (workgroups whose 512 columns all exist, row blocks entirely below N) against its guarded loop:
# the same candidates evaluated in a batch that fills their workgroup and in one that leaves it ragged; N = 1000 also has a ragged
# last row block, N = 1024 none.
@pytest.mark.parametrize("N", [1000, 1024])
@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_cross_kernel_full_and_guarded_loops_agree(B, kind, N):
    p, model, acq, _ = _setup(B, kind, N, 2)
    full = _step(model, acq, p["Xc"][:2560])             # workgroups 0..4 full
    for n in (2559, 2049):                               # workgroup 4 ragged: columns 2048.. take the guarded loop
        part = _step(model, acq, p["Xc"][:n])
        _same(part, tuple(x[:, :n] if i < 2 else x[:n] for i, x in enumerate(full)), "first %d of 2560 candidates" % n)
