"""The top-k selection on the device against np.argsort(-acq, kind="stable")[:k] (value descending, ties to the lowest index).

Part 1: every launch form of launch_topk (bocf_amd/csrc/acq.hip) -- the single block, topk_wave_kernel<1|2|4|8|16> and
topk_stream_kernel<256> in stage 1, the stage-2 merge of the block winners at every slot count -- at the boundaries of C and k,
on vectors built to catch tie-break, block-boundary and tail mistakes.  A chosen vector reaches the device without a test hook:
a host-given posterior (m = 1, train mean 0, so the best-so-far is 0) and the closed-form EI with theta = 1 turn (mean, var)
into the acquisition vector, which is then the reference's input.  EI is increasing in the mean at var = 1; var = 0 with a
negative mean gives an exact 0; mean = +inf gives +inf; mean = NaN gives NaN.

Part 2: the device half of the multi-rank arg-max (pack_topk_kernel, unpack_topk_kernel and the merge) at G simulated ranks on
one GPU: rank r's slice goes through bocf_topk_packed into a device buffer, the host takes the element-wise max of the G
buffers (what all-reduce(MAX) computes), and bocf_merge_packed merges it.

torch is not imported here: test_00_gpu_rccl.py must be the first in the pytest process to open the GPU."""
import ctypes

import numpy as np
import pytest

from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 16, 17, 33, 64)
# every row of launch_topk's table, each at its boundary (C <= 256: one block; then wave<1> up to 16384, <2>, <4>, <8>, <16>, stream)
SIZES = (1, 15, 16, 17, 256, 257, 4097, 16384, 16385, 32769, 65536, 65537, 131072, 131073, 262144, 262145, 600013)
PATTERNS = ("distinct", "equal", "sparse", "runs", "best_first", "best_last", "inf_nan")


def _blocks(C):
    """Stage-1 block count and block size of launch_topk (topk_num_blocks)."""
    nb = min(64, max(1, -(-C // 256)))
    return nb, -(-C // nb)


def _stage1_kernel(C):
    nb, per = _blocks(C)
    if nb > 1 and per > 4096:
        return "topk_stream_kernel<256>"
    return "topk_wave_kernel<%d>" % min(e for e in (1, 2, 4, 8, 16) if 256 * e >= per)


def test_sizes_reach_every_stage1_form():
    forms = set(_stage1_kernel(C) for C in SIZES)
    assert forms == {"topk_wave_kernel<1>", "topk_wave_kernel<2>", "topk_wave_kernel<4>", "topk_wave_kernel<8>", "topk_wave_kernel<16>",
                     "topk_stream_kernel<256>"}


@pytest.fixture(scope="module")
def F():
    from bocf_amd import _ffi
    _ffi.load()                    # fail loudly if the HIP library is missing
    return _ffi


@pytest.fixture(scope="module")
def dev(F):
    d = _Canned(F)
    yield d
    d.ctx.close()


@pytest.fixture(scope="module")
def hip(F):
    lib = ctypes.CDLL("libamdhip64.so.7")       # the runtime libbocf_hip.so has loaded (same soname: the same handle)
    lib.hipMalloc.restype = ctypes.c_int
    lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    lib.hipMemcpy.restype = ctypes.c_int
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipFree.restype = ctypes.c_int
    lib.hipFree.argtypes = [ctypes.c_void_p]
    lib.hipDeviceSynchronize.restype = ctypes.c_int
    lib.hipDeviceSynchronize.argtypes = []
    return lib


class _Canned(object):
    """One context driven through the C ABI: a host-given posterior, the closed-form EI, the selections."""

    def __init__(self, F):
        self.F, self.lib = F, F.load()
        self.ctx = F.Context(0)

    def acq(self, mean, var):
        F = self.F
        mean, var = F.f64(mean)[None, :], F.f64(var)[None, :]
        C = mean.shape[1]
        zero = np.zeros((1, 1))
        F.check(self.lib.bocf_set_posterior(self.ctx.handle, 1, C, 1, F.dptr(mean), F.dptr(var), F.dptr(zero)), "bocf_set_posterior")
        th, pr, out = np.ones((1, 1)), np.ones(1), np.empty(C)
        F.check(self.lib.bocf_acq_linear(self.ctx.handle, F.ACQ_EI, F.dptr(th), F.dptr(pr), 1, F.dptr(out)), "bocf_acq_linear")
        return out

    def select(self, k):
        idx, val = np.empty(k, dtype=np.int64), np.empty(k)
        self.F.check(self.lib.bocf_select_topk(self.ctx.handle, k, idx.ctypes.data_as(self.F._c_ll_p), self.F.dptr(val)), "bocf_select_topk")
        return idx, val

    def global_topk(self, k, lo):
        idx, val = np.empty(k, dtype=np.int64), np.empty(k)
        self.F.check(self.lib.bocf_global_topk(self.ctx.handle, k, lo, idx.ctypes.data_as(self.F._c_ll_p), self.F.dptr(val)), "bocf_global_topk")
        return idx, val

    def topk_packed(self, k, lo, world, rank, buf):
        self.F.check(self.lib.bocf_topk_packed(self.ctx.handle, k, lo, world, rank, buf.ptr), "bocf_topk_packed")

    def merge_packed(self, k, world, buf):
        idx, val = np.empty(k, dtype=np.int64), np.empty(k)
        self.F.check(self.lib.bocf_merge_packed(self.ctx.handle, k, world, buf.ptr, idx.ctypes.data_as(self.F._c_ll_p), self.F.dptr(val)),
                     "bocf_merge_packed")
        return idx, val


class _DeviceBuf(object):
    """n doubles of device memory (hipMalloc), freed on exit."""

    def __init__(self, hip, n):
        self.hip, self.n, self.ptr = hip, n, ctypes.c_void_p()
        _hip_check(hip.hipMalloc(ctypes.byref(self.ptr), 8 * n), "hipMalloc")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _hip_check(self.hip.hipFree(self.ptr), "hipFree")

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.n
        _hip_check(self.hip.hipMemcpy(self.ptr, a.ctypes.data, 8 * self.n, 1), "hipMemcpy H2D")      # hipMemcpyHostToDevice
        _hip_check(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def download(self):
        out = np.empty(self.n)
        _hip_check(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
        _hip_check(self.hip.hipMemcpy(out.ctypes.data, self.ptr, 8 * self.n, 2), "hipMemcpy D2H")    # hipMemcpyDeviceToHost
        return out


def _hip_check(rc, what):
    assert rc == 0, "%s returned hipError %d" % (what, rc)


# ---------------------------------------------------------------------------------------------
# the vectors: (mean, var) per candidate; EI(mean, var = 1) at best-so-far 0 is strictly increasing in the mean

def _sparse_positions(C):
    """The positives of the mostly-zero vector: the first block (wave and slot edges), three block boundaries, the last (ragged)
    block.  Few enough that k = 17 ... 64 also takes zeros."""
    nb, per = _blocks(C)
    pos = [0, 1, 63, 64, 255, 256]
    for b in sorted({1, nb // 2, nb - 1}):
        if b >= 1:
            pos += [b * per - 1, b * per]
    last = (nb - 1) * per
    pos += [last, last + 63, last + 64, C - 2, C - 1]
    return np.array(sorted({p for p in pos if 0 <= p < C}), dtype=np.int64)


def _run_starts(C):
    """Where runs of equal values straddle a boundary: the stage-1 block boundaries, or the wave boundaries of the single block."""
    nb, per = _blocks(C)
    if nb > 1:
        return [b * per for b in range(1, nb)]
    return list(range(64, C, 64))


def _vector(pattern, C, seed):
    rng = np.random.RandomState(seed)
    var = np.ones(C)
    if pattern == "distinct":
        mean = rng.permutation(np.linspace(-3.0, 3.0, C))
    elif pattern == "equal":
        mean = np.full(C, 0.25)
    elif pattern == "sparse":
        mean, var = np.full(C, -1.0), np.zeros(C)                 # EI = 0 exactly
        pos = _sparse_positions(C)
        mean[pos] = rng.choice([0.5, 1.0, 1.5], size=pos.size)    # ties among the positives too
        var[pos] = 1.0
    elif pattern == "runs":
        mean = rng.permutation(np.linspace(-3.0, 0.0, C))
        for j, b in enumerate(_run_starts(C)):
            mean[max(0, b - 12):b + 12] = 1.0 if j % 2 == 0 else 0.5
    elif pattern in ("best_first", "best_last"):
        mean = rng.permutation(np.linspace(-3.0, 2.0, C))
        mean[0 if pattern == "best_first" else C - 1] = 3.0
    elif pattern == "inf_nan":
        mean = rng.permutation(np.linspace(-3.0, 3.0, C))
        nb, per = _blocks(C)
        mean[[C // 2, C - 1, min(per, C - 1)]] = np.inf
        mean[[0, C // 3, per - 1]] = np.nan
    else:
        raise ValueError(pattern)
    return mean, var


def _assert_elementwise(mean, var, acq):
    """Equal (mean, var) inputs give equal acquisition bits (the ties the selection tests rely on are real ties)."""
    order = np.lexsort((var, mean))
    m, v, a = mean[order], var[order], acq[order].view(np.uint64)
    same = (m[1:] == m[:-1]) & (v[1:] == v[:-1])
    np.testing.assert_array_equal(a[1:][same], a[:-1][same])


def _check_pattern(pattern, C, acq):
    if pattern == "distinct":
        assert np.unique(acq).size == C
    elif pattern == "equal":
        assert np.all(acq.view(np.uint64) == acq.view(np.uint64)[0])
    elif pattern == "sparse":
        pos = _sparse_positions(C)
        assert np.all(acq[pos] > 0.0)
        assert np.count_nonzero(acq) == pos.size
    elif pattern in ("best_first", "best_last"):
        i = 0 if pattern == "best_first" else C - 1
        assert np.all(acq[i] > np.delete(acq, i))
    elif pattern == "inf_nan" and C >= 4:
        assert np.isnan(acq).any() and np.isposinf(acq).any()


def _expected(acq, order, k):
    """(indices, values) the C ABI must return: the stable argsort `order` of -acq, then (-1, -inf) for k > C.  A NaN candidate
    ranks as -inf (after every number, by index among the NaN: np.argsort's order, as the vector holds no -inf) and is reported
    as -inf."""
    n = min(k, acq.size)
    idx = np.full(k, -1, dtype=np.int64)
    val = np.full(k, -np.inf)
    idx[:n] = order[:n]
    val[:n] = np.where(np.isnan(acq[idx[:n]]), -np.inf, acq[idx[:n]])
    return idx, val


def _assert_same(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": indices")
    np.testing.assert_array_equal(got[1].view(np.uint64), want[1].view(np.uint64), err_msg=what + ": value bits")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("C", SIZES)
def test_select_topk_every_launch_form(dev, C, pattern):
    mean, var = _vector(pattern, C, seed=C % 1000 + 7 * PATTERNS.index(pattern))
    acq = dev.acq(mean, var)
    _assert_elementwise(mean, var, acq)
    _check_pattern(pattern, C, acq)
    order = R.select_anchors(acq, C)[0]
    ks = sorted(set(KS) | ({C, C + 1} if C < 64 else set()))
    for k in ks:
        want = _expected(acq, order, k)
        what = "%s C=%d k=%d (%s)" % (pattern, C, k, _stage1_kernel(C))
        got = dev.select(k)
        _assert_same(got, want, what)
        _assert_same(dev.select(k), got, what + " repeated")
        # no communicator: pack -> unpack -> merge on one rank; the global indices are lo + the local ones
        _assert_same(dev.global_topk(k, 0), got, what + " global_topk lo=0")
        lo = 1 << 40
        _assert_same(dev.global_topk(k, lo), (np.where(got[0] >= 0, got[0] + lo, -1), got[1]), what + " global_topk lo=2^40")


# ---------------------------------------------------------------------------------------------
# the multi-rank arg-max, device half, G ranks emulated on one context

def _sharded_vector(C, G, seed):
    """Distinct values, 30 % exact zeros, equal pairs straddling every shard boundary, the top value tied at 5, 2050, 4000."""
    from bocf_amd.distributed import shard_bounds
    rng = np.random.RandomState(seed)
    mean, var = rng.permutation(np.linspace(-3.0, 1.0, C)), np.ones(C)
    z = rng.rand(C) < 0.3
    mean[z], var[z] = -1.0, 0.0
    for r in range(1, G):
        lo = shard_bounds(C, G, r)[0]
        mean[[lo - 1, lo]], var[[lo - 1, lo]] = 1.5, 1.0
    top = [i for i in (5, 2050, 4000) if i < C]
    mean[top], var[top] = 2.0, 1.0
    return mean, var


@pytest.mark.parametrize("C,G,k", [
    (300001, 2, 16),         # shards of 150001: stage 1 in topk_wave_kernel<16>
    (100003, 3, 16),         # 33334 / 33335: topk_wave_kernel<4>
    (100003, 8, 16),         # 12500 / 12501: topk_wave_kernel<1>
    (600000, 8, 64),         # 75000: topk_wave_kernel<8>, stage 2 over 64 x 64 winners
    (325007, 65, 64),        # 65 x 64 = 4160 gathered winners: the merge takes topk_stream_kernel
    (3001, 65, 64),          # 46 / 47 candidates per shard < k: -1 slots packed and skipped
])
def test_device_pack_merge_emulated_ranks(dev, hip, C, G, k):
    from bocf_amd.distributed import pack_local_topk, shard_bounds
    mean, var = _sharded_vector(C, G, seed=G)
    whole = dev.acq(mean, var)
    want = _expected(whole, R.select_anchors(whole, k)[0], k)
    assert np.all(want[0] >= 0)
    n = 2 * G * k
    packs = []
    with _DeviceBuf(hip, n) as buf:
        for r in range(G):
            lo, hi = shard_bounds(C, G, r)
            a = dev.acq(mean[lo:hi], var[lo:hi])
            np.testing.assert_array_equal(a.view(np.uint64), whole[lo:hi].view(np.uint64))   # element-wise: the slice's bits
            li = R.select_anchors(a, k)[0]
            host = pack_local_topk(li, a[li], lo, k, G, r)
            dev.topk_packed(k, lo, G, r, buf)
            p = buf.download()
            np.testing.assert_array_equal(p.view(np.uint64), host.view(np.uint64), err_msg="pack of rank %d / %d" % (r, G))
            packs.append(p)
        buf.upload(np.max(np.stack(packs), axis=0))                # what all-reduce(MAX) computes
        got = dev.merge_packed(k, G, buf)
    _assert_same(got, want, "merge of %d ranks, C=%d k=%d" % (G, C, k))
    if C >= 4001:
        assert got[0][:3].tolist() == [5, 2050, 4000]


# ---------------------------------------------------------------------------------------------
# the same selection through the classes: multi_outputGP.select_topk drops the (-1, -inf) tail, select_anchors returns indices

@pytest.mark.parametrize("C,k", [(20, 33), (70001, 17), (300007, 64)])
def test_model_select_topk_and_anchors(F, C, k):
    import bocf_amd as B
    p = R.synthetic_problem(24, 2, 1, 4096, 1, 11)
    model = B.multi_outputGP(1, kernel=[B.kern.RBF(2, variance=1.0, lengthscale=p["lengthscales"][0], ARD=True)], noise_var=p["noise"],
                             fixed_hyps=True)
    model.updateModel(p["X"], p["Y"])
    rows = np.random.RandomState(C).randint(0, 8 if C < 64 else 4096, size=C)          # repeated candidates: ties
    Xc = p["Xc"][rows]
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.ones((1, 1)), prob_dist=np.ones(1)), linear=True)
    acq = B.maEI(model, None, utility=U)
    a = acq._compute_acq(Xc)[:, 0]
    want = R.select_anchors(a, k)[0]
    np.testing.assert_array_equal(acq.select_anchors(k), want)
    idx, val = model.select_topk(k)
    np.testing.assert_array_equal(idx, want)
    assert idx.size == min(k, C)
    np.testing.assert_array_equal(val.view(np.uint64), a[want].view(np.uint64))
