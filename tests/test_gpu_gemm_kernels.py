"""The matrix-product kernels run directly, on operands of the test's choosing, against the NumPy statement of their launchers' contract
(tests/gemm_ref.py), through the probes-only entries of csrc/capi_probe.hip.

Integer mode is the main gate: small integer operands, alpha, beta in {-1, 0, 1} -- every partial sum in every order is exact in the
accumulator (the condition is asserted on the CPU, tests/test_gemm_ref_cpu.py) -- so the result must EQUAL the int64 reference: a dropped,
doubled or misplaced k-tile or output tile is an exact mismatch, and the failure names the first wrong (batch, rt, ct) and element.  Everything
of A and B outside every tile's contraction range is NaN (int8: a finite non-zero poison in A, because the digit cut does not preserve NaN, and
none in B, all of whose rows the heaviest tile reads; fp32 cases on the 256-row kernel: zero up to the row pair's length); everything of C and of the sums the call must not write is a NaN with a payload
that has to survive bit for bit (lower tiles under upper_only, the margin between Ncols and ldc, the rows and columns around a sub-matrix
with a non-zero origin, the gaps between batch slots).  Real mode (one or two shapes per kernel) compares normal random operands with a
few columns scaled by 2^+-20 against extended precision with the standard a-priori bound, and prints the largest error / bound with -s.

Which case reaches which kernel (the routing is inside the launchers; their own conditions in brackets):

launch_gemm_f64
  gemm_tn_f64_kernel<1, 2> (128-row, sums of squares, two tiles ahead)   contract_f64-k128-*            [epilogue 1, swizzle 0]
                                                                         contract_f64-x3-fallback-M384  [swizzle 258 but M % 256 != 0 -> swizzle = 0]
  gemm_tn_f64_kernel<1, 1> (one tile ahead)                              contract_f64-k128-prefetch1-*  [prefetch1]
  gemm_tn_f64_sumsq256x3_kernel<0> (three buffers, 256 rows)             contract_f64-x3-M{256,512,768} [swizzle 258, M % 256 == 0, kb = krt = 128, K >= M, no counters]
  gemm_tn_f64_sumsq256x3_kernel<0, 1> (tile queue)                       contract_f64-queue-*           [the same with tile_ctr and ncu > 0; grid = min(tiles, ncu)]
  gemm_tn_f64_sumsq256_kernel<0, 2, 2> / <0, 2, 0> (two buffers)         contract_f64-two-buffer-swizzle256 / 257   [probes build, swizzle != 258]
  gemm_tn_f64_sumsq256x3_kernel<1> (store form)                          predict_gradients-V-x3store-M{512,768}, capi_chol-merge_second-M{512,768}-*-no_x3_0
                                                                         [epilogue 0, no Cin, M % 256 == 0, M >= 512, kb = krt = 128, rt_desc, !no_x3]
  gemm_tn_f64_kernel<0, 1, 8> (128-row, 8 waves, store)                  predict_gradients-V-k128-* [M < 512], no_x3-switch-V-k128, merge_second-*-no_x3_1,
                                                                         merge_second-M256 [M < 512], capi_kg-W-*, merge_first-* [kbeg_rt != 0], trsm, syrk, row_update
  gemm_tn_f64_kernel<3, 1, 8> (upper-only linear grid)                   capi_chol-trailing-*, capi_fit-kinv-*   [epilogue 3]
  batch orders: blockIdx.z (most cases), swizzle 2 row-tile-major with batch1 (merge_first / merge_second), the store form's own 1-D order.
launch_gemm_f32_sumsq
  gemm_tn_f32_sumsq_kernel (128-row)          contract_f32-tile128-* [tile128], contract_f32-k128-small-N [Ncols < 2048], contract_f32-k128-odd-M384 [M % 256 != 0]
  gemm_tn_f32_sumsq256x3_kernel (256-row)     contract_f32-x3-M{256,512}-N2048 [!tile128, M % 256 == 0, Ncols >= 2048, K >= M]
launch_var_i8 (+ launch_col_exponents, launch_slice_operand)
  var_i8_kernel, XCD-blocked grid             contract_i8-*-group0   [group < 1]
  var_i8_kernel, banded grid                  contract_i8-*-group1 / group2 [group >= 1, clipped to the number of pairs]
  Np 128: one unpaired tile; 256: one pair; 384: a pair and the unpaired middle tile.
launch_tile128
  tile128_kernel                              capi_chol-tile128-* (ntiles 1 and 3, K 128 and 384, beta 0 in place and beta 1)
"""
import ctypes

import numpy as np
import pytest

import gemm_ref as G

pytestmark = pytest.mark.gpu


def _fill(desc, d):
    for f, _t in desc._fields_:
        v = d.__dict__.get(f)
        if v is not None and not isinstance(v, np.ndarray) and f != "ctr":
            setattr(desc, f, v)


def _buf(a):
    """(pointer, length, the copy the pointer refers to) of a host buffer; an absent buffer is a null pointer of length 0"""
    if a is None:
        return None, 0, np.zeros(0)
    c = a.copy()
    return c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), c.size, c


def run(lib, kind, d, **over):
    """Run one descriptor through its entry on copies of its buffers; returns the buffers as they came back."""
    from bocf_amd import _ffi
    out = G.SimpleNamespace()
    if kind == "f64":
        desc = _ffi.ProbeGemmF64()
        _fill(desc, d)
        (desc.A, desc.lenA, out.A), (desc.B, desc.lenB, out.B) = _buf(d.A), _buf(d.B)
        (desc.C, desc.lenC, out.C), (desc.sumsq, desc.lenS, out.S) = _buf(d.C), _buf(d.S)
        fn = lib.bocf_probe_gemm_f64
    elif kind == "f32":
        desc = _ffi.ProbeGemmF32()
        _fill(desc, d)
        (desc.A, desc.lenA, out.A), (desc.B, desc.lenB, out.B), (desc.sumsq, desc.lenS, out.S) = _buf(d.A), _buf(d.B), _buf(d.S)
        fn = lib.bocf_probe_gemm_f32
    elif kind == "i8":
        desc = _ffi.ProbeVarI8()
        _fill(desc, d)
        desc.Np, desc.ncols, desc.m = d.M, d.Ncols, d.batch
        (desc.A, desc.lenA, out.A), (desc.B, desc.lenB, out.B), (desc.sumsq, desc.lenS, out.S) = _buf(d.A), _buf(d.B), _buf(d.S)
        out.eA, out.eB = np.full((d.batch, d.M), 12345, dtype=np.int32), d.eB.copy()
        desc.eA, desc.eB = out.eA.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), out.eB.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        fn = lib.bocf_probe_var_i8
    else:
        desc = _ffi.ProbeTile128()
        _fill(desc, d)
        (desc.A, desc.lenA, out.A), (desc.B, desc.lenB, out.B), (desc.C, desc.lenC, out.C) = _buf(d.A), _buf(d.B), _buf(d.C)
        fn = lib.bocf_probe_tile128
    for k, v in over.items():
        setattr(desc, k, v)
    rc = fn(ctypes.byref(desc))
    assert rc == 0, lib.bocf_last_error().decode("utf-8", "replace")
    if kind == "f64":
        out.ctr = (desc.ctr[0], desc.ctr[1])
    return out


def result_of(kind, d, ref, out):
    """(got, input, expected, mask, bound, name) of the buffer the call writes"""
    if kind in ("f32", "i8") or (kind == "f64" and d.epilogue == 1):
        return out.S, d.S, ref.S, ref.maskS, ref.boundS, "S"
    return out.C, d.C, ref.C, ref.maskC, ref.boundC, "C"


def check_untouched(kind, d, out, got, inp, mask):
    """the sentinel (and everything else the call must not write) survives bit for bit; the operands come back unchanged (the fp64 and
    tile128 entries copy A and B back; the fp32 and int8 kernels see converted copies, so there is nothing to compare for them)"""
    assert np.array_equal(G.bits(got)[~mask], G.bits(inp)[~mask]), "a store outside the tiles of the call: %d elements changed" % int(
        (G.bits(got)[~mask] != G.bits(inp)[~mask]).sum())
    if kind in ("f64", "t128"):
        assert np.array_equal(G.bits(out.A), G.bits(d.A)), "A was written"
        if d.B is not None:
            assert np.array_equal(G.bits(out.B), G.bits(d.B)), "B was written"


def describe(kind, d, got, exp, mask, what):
    if kind == "t128":
        bad = np.flatnonzero(mask & ~(got == exp))
        return "%d elements differ, first at flat index %d: %r, expected %r" % (len(bad), bad[0], got[bad[0]], float(exp[bad[0]]))
    return G.first_mismatch(d, got, exp, mask, what)


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_integer_operands_give_the_exact_product(probes, name):
    kind, d, ref = G.case(name)
    out = run(probes, kind, d, repeat=1)
    got, inp, exp, mask, _, what = result_of(kind, d, ref, out)
    check_untouched(kind, d, out, got, inp, mask)
    e64 = exp.astype(np.float64)                            # (integers below 2^53: exact)
    if kind == "i8":
        # exact digit products; only the fp64 recombination, the squares and the 128-row sum round (below about 160 ulp)
        ok = np.abs(got[mask] - e64[mask]) <= 1e-12 * np.abs(e64[mask])
        assert ok.all(), describe(kind, d, np.where(np.isclose(got, e64, rtol=1e-12, atol=0.0), e64, got), e64, mask, what)
        assert np.array_equal(out.eA, G.ref_i8_exponents(d)), "column exponents"
        assert np.array_equal(out.eB, d.eB)
        if "zero-column" in name:
            assert out.eA[0, 5] == G.ZERO_EXPO
    else:
        assert np.array_equal(got[mask], e64[mask]), describe(kind, d, got, e64, mask, what)
    if kind == "f64" and d.use_queue:
        # the same launch twice on the same counters: the second finds them as the first left them, gives the same bits, and both read back zero
        assert out.ctr == (0, 0)
        again = run(probes, kind, d, repeat=2)
        assert again.ctr == (0, 0), "the tile-queue counters are not back at zero after the launch: %r" % (again.ctr,)
        assert np.array_equal(G.bits(again.S), G.bits(out.S)), describe(kind, d, again.S, e64, mask, what)


@pytest.mark.parametrize("name", sorted(G.REAL_CASES))
def test_real_operands_stay_inside_the_a_priori_bound(probes, name):
    """|C - C_ref| <= gamma_K |alpha| |A|^T |B| + u |C_ref| elementwise (gamma_{K+2} over the terms with Cin where C is read), the bound propagated
    through (v + e)^2 plus gamma_129 sum v^2 for the sums of squares, u = 2^-24 and the input rounding for the fp32 kernels, the digit truncation
    for int8 (tests/gemm_ref.py states each).  The bound is the standard one, not a measured tolerance; the observed ratio is printed."""
    kind, d, ref = G.case(name)
    out = run(probes, kind, d, repeat=1)
    got, inp, exp, mask, bound, what = result_of(kind, d, ref, out)
    check_untouched(kind, d, out, got, inp, mask)
    assert not np.isnan(got[mask]).any(), "NaN in the result: something outside a contraction range was multiplied"
    err = np.abs(got[mask].astype(np.longdouble) - exp[mask]).astype(np.float64)
    b = bound[mask]
    assert (b > 0).all()
    ratio = float((err / b).max())
    print("\n%-52s largest error / bound = %.3g   (largest relative error %.3g)" % (name, ratio, float((err / np.maximum(np.abs(exp[mask]).astype(np.float64), 1e-300)).max())))
    assert ratio <= 1.0, "error %.3g of the bound at flat index %d of the written elements" % (ratio, int(np.argmax(err / b)))
    if kind == "i8":
        assert np.array_equal(out.eA, G.ref_i8_exponents(d)), "column exponents"
