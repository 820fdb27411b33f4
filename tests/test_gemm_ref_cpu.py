"""No GPU: the NumPy reference of the matrix-product launchers (tests/gemm_ref.py) checked against itself, and the conditions under which
the integer-mode GPU tests (tests/test_gpu_gemm_kernels.py) may demand exact equality, on the very inputs those tests use."""
import ctypes

import numpy as np
import pytest

import gemm_ref as G

INT_CASES = sorted(G.CASES)
TRI_CASES = [n for n in INT_CASES if G.CASES[n][0] in ("f64", "f32", "i8") and ("contract" in n or "-V-" in n or "-W-" in n or "merge" in n or "kinv" in n)]


def test_every_triangular_form_is_covered():
    for n in INT_CASES:
        kind, d, _ = G.case(n)
        if kind != "t128":
            assert (d.tri is not None) == (n in TRI_CASES), n
    assert len(TRI_CASES) >= 60


@pytest.mark.parametrize("name", TRI_CASES)
def test_tile_rule_equals_dense_product_for_triangular_operands(name):
    """What makes the triangular contraction ranges legal: with A truly triangular the per-tile ranges give the plain dense product.  Every NaN
    of A lies strictly on the zero side of its diagonal (the part no tile may read), every other element of that side is zero, and every
    element on the other side is non-zero."""
    kind, d, _ = G.case(name)
    for z in range(d.batch):
        A = G.view2(d.A, d.offA + G.batch_offsets(d, z)[0], d.K, d.lda, d.M)
        k, r = np.arange(d.K)[:, None], np.arange(d.M)[None, :]
        zero_side = k > r if d.tri == "upper" else k < r
        unread = np.isnan(A)
        if kind == "i8":                                # the finite poison of the int8 operand stands where the others have NaN
            assert not unread.any()
            unread = G.view2(d.poison, d.offA + G.batch_offsets(d, z)[0], d.K, d.lda, d.M)
            assert unread.any() == (d.M > 128) and (A[unread] != 0.0).all()
            assert np.array_equal(unread, np.broadcast_to(k >= 128 * (r // 128 + 1), A.shape))
        assert zero_side[unread].all(), "poison on the non-zero side of the triangle"
        assert (A[zero_side & ~unread] == 0.0).all()
        live = ~zero_side & ~unread
        if not (kind == "i8" and "zero-column" in name):
            assert (A[live] != 0.0).all() and live.any(axis=0).all()
    assert G.dense_equals_tile_rule(d) == 0


@pytest.mark.parametrize("name", INT_CASES)
def test_integer_mode_is_exact_in_the_accumulator(name):
    """sum |a| |b| per output element, and the total of the squares per (row tile, column), stay below 2^53 (fp64 kernels) / 2^24 (fp32 kernels:
    products, the K-term sums, the squares and their sums are all formed in float): every partial sum in every order is then an integer the
    accumulator holds exactly, so the GPU test may assert array_equal."""
    kind, d, ref = G.case(name)
    limit = 2.0 ** 24 if kind == "f32" else 2.0 ** 53
    assert 0 < ref.absprod < limit
    if kind in ("f64", "f32") and d.epilogue == 1:
        assert 0 < ref.abssq < limit
    if kind in ("f64", "t128"):
        assert d.alpha in (-1.0, 0.0, 1.0) and d.beta in (-1.0, 0.0, 1.0)
    # the expected buffers hold integers (and the untouched fill) only
    exp = ref.C if getattr(ref, "S", None) is None else ref.S
    mask = ref.maskC if getattr(ref, "S", None) is None else ref.maskS
    assert mask.any() and not np.isnan(exp[mask]).any() and (exp[mask] == np.rint(exp[mask])).all()
    if mask.size > mask.sum():
        assert np.isnan(exp[~mask]).all()               # everything the call must not write is the sentinel


def test_every_product_route_has_a_case():
    """The routing conditions of the three launchers, restated on the descriptors: every branch is taken by at least one case.  This is a
    checklist, not a derivation: nothing ties it to launch_gemm_f64 (gemm_f64.hip), launch_gemm_f32_sumsq or launch_var_i8, so it has to be
    edited together with them -- a launcher whose conditions change without this copy leaves a route uncovered while the test still passes."""
    routes = set()
    for name in sorted(G.CASES):
        kind, d, _ = G.case(name)
        if kind == "f64":
            x3 = d.M % 256 == 0 and d.kb == 128 and d.krt == 128 and d.kct == 0 and d.kbeg_rt == 0 and d.kbeg_ct == 0 and d.K >= d.M
            if d.epilogue == 1 and d.swizzle >= 256 and not d.prefetch1 and d.M % 256 == 0 and d.batch1 == 0:
                routes.add("two-buffer-%d" % d.swizzle if d.swizzle != 258 else ("x3-queue" if d.use_queue else "x3") if x3 else "k128-sumsq")
            elif d.epilogue == 1:
                routes.add("k128-sumsq-pf1" if d.prefetch1 else ("k128-sumsq-fallback" if d.swizzle >= 256 else "k128-sumsq"))
            elif d.epilogue == 0 and not d.no_x3 and not d.has_cin and x3 and d.M >= 512 and not d.upper_only and d.rt_desc and not d.ct_desc:
                routes.add("x3-store-batch1" if d.batch1 else "x3-store")
            elif d.epilogue == 3:
                routes.add("upper-linear")
            else:
                routes.add("k128-store-swizzle2" if d.swizzle == 2 else "k128-store")
        elif kind == "f32":
            routes.add("f32-x3" if (not d.tile128 and d.M % 256 == 0 and d.Ncols >= 2048 and d.K >= d.M) else "f32-k128")
        elif kind == "i8":
            routes.add("i8-xcd" if d.i8_group < 1 else "i8-banded")
            routes.add("i8-nrt%d" % (d.M // 128))
    assert routes == {"two-buffer-256", "two-buffer-257", "x3", "x3-queue", "k128-sumsq", "k128-sumsq-pf1", "k128-sumsq-fallback", "x3-store", "x3-store-batch1",
                      "upper-linear", "k128-store", "k128-store-swizzle2", "f32-x3", "f32-k128", "i8-xcd", "i8-banded", "i8-nrt1", "i8-nrt2", "i8-nrt3"}, routes


def _digits(x, e, n=6):
    """the radix-254 digits slice_operand_kernel cuts x 2^-e 127 into"""
    x = np.ldexp(x, -e) * 127.0
    out = []
    for _ in range(n):
        dg = np.rint(x)
        out.append(int(dg))
        x = (x - dg) * 254.0
    return out, x


def test_int8_operands_have_three_digits_and_exact_products():
    """Entries in {-3 ... 3} under the exponents the test uses (per column of A: 1 for a maximum of 1, 2 for 2 or 3; B: 2) have at most three non-zero
    digits and no remainder: no dropped digit group i + j >= 6 is non-zero, and the int32 digit products over K <= 384 cannot overflow."""
    for e in (1, 2):
        for v in range(-3, 4):
            if abs(v) < 2 ** e:
                dg, rem = _digits(float(v), e)
                assert rem == 0.0 and all(abs(x) <= 127 for x in dg) and not any(dg[3:]), (v, e, dg)
    for name in INT_CASES:
        kind, d, _ = G.case(name)
        if kind != "i8":
            continue
        assert (d.eB == 2).all()
        vals = np.concatenate([d.A[~np.isnan(d.A) & ~d.poison], d.B[~np.isnan(d.B)]])
        assert set(np.unique(vals)) <= set(float(v) for v in range(-3, 4))
        assert d.K * 127 * 127 * 6 < 2 ** 31
        eA = G.ref_i8_exponents(d)
        ok = set((1, 2)) | ({int(G.ZERO_EXPO)} if "zero-column" in name else set())
        assert set(np.unique(eA)) <= ok


def test_sentinel_and_fill_patterns():
    assert np.isnan(G.SENTINEL) and G.bits(np.array([G.SENTINEL]))[0] == 0x7FF8DEAD0000BEEF
    assert int(G.ZERO_EXPO) == -2139062144


def test_reference_arithmetic_is_wider_than_fp64():
    a = np.array([[1.0], [2.0 ** -60]])
    out = G._extended_matmul(a, np.ones((2, 1)))
    assert out.dtype == np.longdouble
    if np.finfo(np.longdouble).nmant >= 63:
        assert out[0, 0] != 1.0                         # 1 + 2^-60 survives


def test_probe_entries_refuse_operands_outside_their_buffers(probes):
    """The entries check every extent on the host BEFORE anything is launched (so this needs no GPU): a buffer one element short of what the
    kernels of that launcher can touch is an error, not a launch."""
    from bocf_amd import _ffi
    kind, d, _ = G.case("contract_f64-k128-M128-N128")
    desc = _ffi.ProbeGemmF64()
    for f, _t in desc._fields_:
        if f in d.__dict__ and not isinstance(d.__dict__[f], np.ndarray) and d.__dict__[f] is not None:
            setattr(desc, f, d.__dict__[f])
    A, B, S = d.A.copy(), d.B.copy(), d.S.copy()
    desc.A, desc.B, desc.sumsq = _ffi.dptr(A), _ffi.dptr(B), _ffi.dptr(S)
    for short in ("lenA", "lenB", "lenS"):
        desc.lenA, desc.lenB, desc.lenS = A.size, B.size, S.size
        setattr(desc, short, getattr(desc, short) - 1)
        assert probes.bocf_probe_gemm_f64(ctypes.byref(desc)) < 0
        assert b"ends at element" in probes.bocf_last_error()
    desc.lenA, desc.lenB, desc.lenS = A.size, B.size, S.size
    desc.M = 100
    assert probes.bocf_probe_gemm_f64(ctypes.byref(desc)) < 0 and b"multiples" in probes.bocf_last_error()
    t = _ffi.ProbeTile128()
    assert probes.bocf_probe_tile128(ctypes.byref(t)) < 0
    assert probes.bocf_probe_gemm_f32(ctypes.byref(_ffi.ProbeGemmF32())) < 0
    assert probes.bocf_probe_var_i8(ctypes.byref(_ffi.ProbeVarI8())) < 0
