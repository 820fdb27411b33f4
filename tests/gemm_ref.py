"""NumPy statement of the contract of the four matrix-product launchers (csrc/bocf_internal.h) and the operands the kernel tests run
them on.  Shared by tests/test_gemm_ref_cpu.py (no GPU: the reference against itself, the exactness conditions) and
tests/test_gpu_gemm_kernels.py (the kernels against the reference, through the probes-only entries of csrc/capi_probe.hip).

The contract, in plain loops over tiles (`ref_gemm`):
  * the tile at row rt, column ct contracts k in [kbeg_rt rt + kbeg_ct ct, min(K, kb + krt rt + kct ct));
  * C = beta Cin + alpha A^T B (A, B k-major, C row-major); without Cin, C = alpha A^T B;
  * upper_only leaves the tiles with ct < rt alone;
  * epilogue 1 writes, per 128-row tile, the column sums of squares as [batch][rt][Ncols] and never touches C;
  * batch z reads its operands at z stride, or with batch1 > 0 at (z % batch1) stride + (z / batch1) stride2.
The fp32 and int8 launchers are the sums-of-squares form with row tile rt ending at k = 128 (rt + 1); launch_tile128 is ntiles plain tiles
side by side.

Arithmetic: int64 in integer mode; in real mode np.longdouble where it carries 64 bits (x86), else mpmath or fractions.

Operands (`make_*`): every buffer starts as NaN (operands) or as the sentinel (C, sums); then only what a tile's contraction range
addresses is filled with values -- a triangular A with non-zero entries on and above its diagonal and zeros below it inside the range --
so a kernel that multiplies anything outside its range returns NaN and one that stores outside its tiles breaks the sentinel.  Two
exceptions, each stated at its maker: int8 operands pass through the digit cut, which does not preserve NaN, so A is poisoned with finite
non-zero values there (and B, every row of which the heaviest tile reads, has none); the 256-row fp32 kernel reads a row pair to the lower
half's length, so A is zero, not NaN, up to there in the cases the launcher sends to that kernel."""
import functools
from types import SimpleNamespace

import numpy as np

TILE = 128
SENTINEL = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]      # a NaN with a payload: compared bit for bit
ZERO_EXPO = np.array([0x80808080], dtype=np.uint32).view(np.int32)[0]               # the memset pattern an all-zero column keeps
U64 = 2.0 ** -53
U32 = 2.0 ** -24


def gamma(n, u):
    return n * u / (1.0 - n * u)


def view2(buf, origin, rows, ld, width):
    """rows x width window with leading dimension ld at `origin` of a flat buffer (writes go through)."""
    assert origin >= 0 and origin + (rows - 1) * ld + width <= buf.size, "window outside its buffer"
    return np.lib.stride_tricks.as_strided(buf[origin:], shape=(rows, width), strides=(ld * buf.itemsize, buf.itemsize))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact / extended arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def _extended_matmul(At, Bt):
    """At^T Bt (k x r, k x c) in extended precision, returned as longdouble (>= 64 bits where the platform has them)."""
    if np.finfo(np.longdouble).nmant >= 63:
        return At.astype(np.longdouble).T @ Bt.astype(np.longdouble)
    try:                                                # 53-bit long double: multi-precision, rounded once at the end
        import mpmath
        mpmath.mp.prec = 128
        out = mpmath.matrix(At.T.tolist()) * mpmath.matrix(Bt.tolist())
        return np.array([[float(out[i, j]) for j in range(out.cols)] for i in range(out.rows)], dtype=np.longdouble)
    except ImportError:
        from fractions import Fraction
        fa, fb = [[Fraction(x) for x in row] for row in At.T.tolist()], [[Fraction(x) for x in col] for col in Bt.T.tolist()]
        return np.array([[float(sum(x * y for x, y in zip(r, c))) for c in fb] for r in fa], dtype=np.longdouble)


def tile_product(At, Bt, integer):
    """(A^T B, |A|^T |B|) of one tile's contraction range."""
    if At.shape[0] == 0:
        z = np.zeros((At.shape[1], Bt.shape[1]), dtype=np.int64 if integer else np.longdouble)
        return z, np.zeros(z.shape)
    if integer:
        assert not np.isnan(At).any() and not np.isnan(Bt).any(), "NaN inside a contraction range"
        ai, bi = At.astype(np.int64), Bt.astype(np.int64)
        assert np.array_equal(ai, At) and np.array_equal(bi, Bt), "integer mode needs integer operands"
        return ai.T @ bi, np.abs(At).T @ np.abs(Bt)       # (the magnitudes in fp64: exact below 2^53, and at least 2^53 when they are not)
    return _extended_matmul(At, Bt), (np.abs(At).T @ np.abs(Bt)) * (1.0 + 1e-12)


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_gemm_f64
# ---------------------------------------------------------------------------------------------------------------------------------
_F64_DEFAULTS = dict(offA=0, offB=0, offC=0, offS=0, lda=0, strideA=0, strideA2=0, ldb=0, strideB=0, strideB2=0, ldc=0, strideC=0, strideC2=0,
                     strideSumsq=0, alpha=1.0, beta=0.0, M=0, Ncols=0, K=0, kb=0, krt=0, kct=0, kbeg_rt=0, kbeg_ct=0, batch1=0, upper_only=0,
                     rt_desc=0, ct_desc=0, swizzle=0, prefetch1=0, stagger=0, no_x3=0, vprobe=0, batch=1, epilogue=0, has_cin=0, b_alias_c=0,
                     use_queue=0, ncu=0, repeat=1, ctile=TILE, poison=None, A=None, B=None, C=None, S=None, integer=True, tri=None)


def gemm_desc(**kw):
    d = dict(_F64_DEFAULTS)
    assert set(kw) <= set(d), set(kw) - set(d)
    d.update(kw)
    return SimpleNamespace(**d)


def batch_offsets(d, z):
    if d.batch1 > 0:
        z1, z2 = z % d.batch1, z // d.batch1
        return z1 * d.strideA + z2 * d.strideA2, z1 * d.strideB + z2 * d.strideB2, z1 * d.strideC + z2 * d.strideC2
    return z * d.strideA, z * d.strideB, z * d.strideC


def gemm_tiles(d):
    """(z, rt, ct, kbeg, kend) of every tile the call computes."""
    for z in range(d.batch):
        for rt in range(d.M // TILE):
            for ct in range(d.Ncols // d.ctile):
                if d.upper_only and ct < rt:
                    continue
                yield z, rt, ct, d.kbeg_rt * rt + d.kbeg_ct * ct, min(d.K, d.kb + d.krt * rt + d.kct * ct)


def ref_gemm(d):
    """What launch_gemm_f64 must leave behind: dict with the expected C and sums buffers (copies of the inputs with every element the call
    writes replaced), the masks of the written elements, and in real mode the elementwise error bounds."""
    integer = d.integer
    Bbuf = d.C if d.b_alias_c else d.B
    store = d.epilogue != 1
    out = SimpleNamespace(C=None if d.C is None else d.C.astype(np.longdouble), S=None if d.S is None else d.S.astype(np.longdouble),
                          maskC=None if d.C is None else np.zeros(d.C.size, bool), maskS=None if d.S is None else np.zeros(d.S.size, bool),
                          boundC=None if d.C is None else np.zeros(d.C.size), boundS=None if d.S is None else np.zeros(d.S.size),
                          absprod=0.0, abssq=0.0)
    for z, rt, ct, kbeg, kend in gemm_tiles(d):
        oA, oB, oC = batch_offsets(d, z)
        At = view2(d.A, d.offA + oA, d.K, d.lda, d.M)[kbeg:max(kbeg, kend), rt * TILE:(rt + 1) * TILE]
        Bt = view2(Bbuf, d.offB + oB, d.K, d.ldb, d.Ncols)[kbeg:max(kbeg, kend), ct * d.ctile:(ct + 1) * d.ctile]
        acc, mag = tile_product(At, Bt, integer)
        klen = max(kend - kbeg, 1)
        out.absprod = max(out.absprod, float(mag.max()))
        if store:
            rows, cols = slice(rt * TILE, (rt + 1) * TILE), slice(ct * TILE, (ct + 1) * TILE)
            alpha, beta = (int(d.alpha), int(d.beta)) if integer else (np.longdouble(d.alpha), np.longdouble(d.beta))
            val = alpha * acc
            bound = gamma(klen, U64) * abs(d.alpha) * mag
            if d.has_cin:
                cin = view2(d.C, d.offC + oC, d.M, d.ldc, d.Ncols)[rows, cols]
                assert not np.isnan(cin).any(), "Cin holds the sentinel inside a tile"
                val = val + beta * (cin.astype(np.int64) if integer else cin.astype(np.longdouble))
                # alpha acc, beta cin and their sum each round once more than the stored product does
                bound = gamma(klen + 2, U64) * (abs(d.alpha) * mag + abs(d.beta) * np.abs(cin))
            bound = bound + U64 * np.abs(val).astype(np.float64)
            view2(out.C, d.offC + oC, d.M, d.ldc, d.Ncols)[rows, cols] = val
            view2(out.maskC, d.offC + oC, d.M, d.ldc, d.Ncols)[rows, cols] = True
            view2(out.boundC, d.offC + oC, d.M, d.ldc, d.Ncols)[rows, cols] = bound
        else:
            o = d.offS + z * d.strideSumsq + rt * d.Ncols + ct * d.ctile
            if integer:
                sq = (acc * acc).sum(axis=0)
                out.abssq = max(out.abssq, float(sq.max()))
                out.S[o:o + d.ctile] = sq
            else:
                out.S[o:o + d.ctile] = (acc * acc).sum(axis=0)
                out.boundS[o:o + d.ctile] = sumsq_bound(acc, gamma(klen, U64) * mag, U64)
            out.maskS[o:o + d.ctile] = True
    return out


def sumsq_bound(v, dv, u):
    """|sum (v + e)^2 - sum v^2| for |e| <= dv elementwise, plus the rounding of the 128 squares and 128 additions (fused or not)."""
    v = np.abs(v).astype(np.float64)
    return (2.0 * v * dv + dv * dv).sum(axis=0) + gamma(129, u) * ((v + dv) ** 2).sum(axis=0)


def nan_fill_operands(d, rng, tri=None, entries_a=(-3, -2, -1, 1, 2, 3), entries_b=(-3, -2, -1, 0, 1, 2, 3), real=False, zero_rows=None):
    """A and B of a launch_gemm_f64 descriptor: NaN everywhere, values only where some computed tile's contraction range addresses them.
    tri = 'upper': A[k][r] non-zero for k <= r, zero for k > r (inside a range); 'lower': non-zero for k >= r; None: dense (non-zero).
    zero_rows (fp32 256-row tiles): callable rt -> first k that may stay NaN; below it the part under the diagonal is zero, not NaN."""
    assert d.A.size and np.isnan(d.A).all() and (d.b_alias_c or np.isnan(d.B).all())
    Bbuf = d.C if d.b_alias_c else d.B
    nrt, nct = d.M // TILE, d.Ncols // d.ctile
    for z in range(d.batch):
        oA, oB, _ = batch_offsets(d, z)
        useA, useB = np.zeros((d.K, nrt), bool), np.zeros((d.K, nct), bool)
        for zz, rt, ct, kbeg, kend in gemm_tiles(d):
            if zz == z:
                useA[kbeg:kend, rt] = True
                useB[kbeg:kend, ct] = True
        if zero_rows is not None:
            for rt in range(nrt):
                useA[:min(d.K, zero_rows(rt)), rt] = True
        k = np.arange(d.K)[:, None]
        va = rng.standard_normal((d.K, d.M)) if real else rng.choice(entries_a, size=(d.K, d.M)).astype(np.float64)
        vb = rng.standard_normal((d.K, d.Ncols)) if real else rng.choice(entries_b, size=(d.K, d.Ncols)).astype(np.float64)
        if real:                                        # magnitudes that differ across a tile
            for c, e in ((1, 20), (d.M - 3, -20), (d.M // 2 + 5, 20)):
                va[:, c] *= 2.0 ** e
            for c, e in ((0, -20), (d.Ncols - 2, 20), (77, 20)):
                vb[:, c] *= 2.0 ** e
        r = np.arange(d.M)[None, :]
        if tri == "upper":
            va[k > r] = 0.0
        elif tri == "lower":
            va[k < r] = 0.0
        va[~np.repeat(useA, TILE, axis=1)] = np.nan
        vb[~np.repeat(useB, d.ctile, axis=1)] = np.nan
        view2(d.A, d.offA + oA, d.K, d.lda, d.M)[:] = va
        view2(Bbuf, d.offB + oB, d.K, d.ldb, d.Ncols)[:] = vb


def dense_equals_tile_rule(d):
    """Triangular forms: the tile rule's result equals the plain dense product of the same matrices (NaN = the zero the kernel never reads).
    Returns the largest absolute difference over all computed tiles (integer mode: 0 exactly)."""
    worst = 0
    Bbuf = d.C if d.b_alias_c else d.B
    for z in range(d.batch):
        oA, oB, _ = batch_offsets(d, z)
        A = np.nan_to_num(view2(d.A, d.offA + oA, d.K, d.lda, d.M), nan=0.0)
        if d.poison is not None:                        # (int8: the finite poison stands where the other kinds have NaN)
            A = np.where(view2(d.poison, d.offA + oA, d.K, d.lda, d.M), 0.0, A)
        A = A.astype(np.int64)
        B = np.nan_to_num(view2(Bbuf, d.offB + oB, d.K, d.ldb, d.Ncols), nan=0.0).astype(np.int64)
        dense = A.T @ B
        for zz, rt, ct, kbeg, kend in gemm_tiles(d):
            if zz != z:
                continue
            ruled = A[kbeg:max(kbeg, kend), rt * TILE:(rt + 1) * TILE].T @ B[kbeg:max(kbeg, kend), ct * d.ctile:(ct + 1) * d.ctile]
            worst = max(worst, int(np.abs(dense[rt * TILE:(rt + 1) * TILE, ct * d.ctile:(ct + 1) * d.ctile] - ruled).max()))
    return worst


def first_mismatch(d, got, exp, mask, what):
    """Name the first wrong tile and element of a flat result buffer (`what` = 'C' or 'S')."""
    for z, rt, ct, kbeg, kend in gemm_tiles(d):
        if what == "C":
            o = d.offC + batch_offsets(d, z)[2]
            g = view2(got, o, d.M, d.ldc, d.Ncols)[rt * TILE:(rt + 1) * TILE, ct * d.ctile:(ct + 1) * d.ctile]
            e = view2(exp, o, d.M, d.ldc, d.Ncols)[rt * TILE:(rt + 1) * TILE, ct * d.ctile:(ct + 1) * d.ctile]
        else:
            o = d.offS + z * d.strideSumsq + rt * d.Ncols + ct * d.ctile
            g, e = got[o:o + d.ctile][None, :], exp[o:o + d.ctile][None, :]
        bad = np.argwhere(~(g == e))
        if bad.size:
            r, c = bad[0]
            return "first wrong tile (batch %d, rt %d, ct %d) k in [%d, %d): element (%d, %d) is %r, expected %r; %d of %d elements of the tile differ" % (
                z, rt, ct, kbeg, kend, r, c, float(g[r, c]), float(e[r, c]), len(bad), g.size)
    m = np.argwhere(bits(got)[~mask] != bits(exp)[~mask])
    return "%d elements outside the written tiles changed (first at flat index %d of the unwritten ones)" % (len(m), m[0][0] if len(m) else -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the argument forms the callers build (field values copied from the call sites)
# ---------------------------------------------------------------------------------------------------------------------------------
def _alloc(n, fill=np.nan):
    return np.full(int(n), fill, dtype=np.float64)


def _place(rows, width, pad):
    """(ld, origin, elements) of a rows x width matrix: tight, or inside a larger allocation (ld > width, rows and columns around it)."""
    if not pad:
        return width, 0, rows * width
    ld = width + 2 * TILE
    return ld, 3 * ld + TILE, (rows + 5) * ld


def make_f64(form, M, Ncols, K=None, batch=1, batch1=0, pad=False, real=False, seed=0, **over):
    """One launch_gemm_f64 descriptor with operands.  `form` names the caller:
      variance        capi.hip contract_f64 (sums of squares; swizzle / prefetch1 / use_queue / ncu through **over)
      v_store         capi.hip predict_gradients (first), capi_thompson.hip:53: V = R^T K* stored
      w_store         capi.hip predict_gradients (second), capi_kg.hip:41: W = R V, kbeg_rt = 128
      trsm            capi_chol.hip:37 in-place panel solve
      syrk            capi_chol.hip:67 trailing update of block rows (M rows of an Ncols-wide trailing matrix)
      trailing        capi_chol.hip:234 trailing update behind g = K / 128 block rows (epilogue 3)
      row_update      capi_chol.hip:261
      merge_first     capi_chol.hip:475 (batch1 = m, swizzle 2)
      merge_second    capi_chol.hip:487 (batch1 = m, swizzle 2; no_x3 through **over)
      kinv            capi_fit.hip:656 Ky^-1 = R R^T on upper tiles, kbeg_ct = 128"""
    rng = np.random.default_rng(seed)
    K = M if K is None else K
    d = gemm_desc(M=M, Ncols=Ncols, K=K, batch=batch, integer=not real)
    tri = None
    if form == "variance":
        d.kb = d.krt = TILE; d.rt_desc = 1; d.epilogue = 1; tri = "upper"
    elif form == "v_store":
        d.kb = d.krt = TILE; d.rt_desc = 1; d.alpha = 1.0; tri = "upper"
    elif form == "w_store":
        d.kb = K; d.kbeg_rt = TILE; d.alpha = 1.0; tri = "lower"
    elif form == "trsm":
        assert M == TILE and K == TILE
        d.kb = TILE; d.alpha = 1.0; d.beta = 0.0; d.b_alias_c = 1
    elif form == "syrk":
        assert K == TILE
        d.kb = TILE; d.upper_only = 1; d.alpha = -1.0; d.beta = 1.0; d.has_cin = 1
    elif form == "trailing":
        assert M == Ncols
        d.kb = K; d.upper_only = 1; d.alpha = -1.0; d.beta = 1.0; d.has_cin = 1; d.epilogue = 3
    elif form == "row_update":
        assert M == TILE
        d.kb = K; d.alpha = -1.0; d.beta = 1.0; d.has_cin = 1
    elif form == "merge_first":
        d.kb = K; d.kbeg_rt = TILE; d.alpha = 1.0; d.batch1 = batch1; d.swizzle = 2; tri = "lower"
    elif form == "merge_second":
        d.kb = d.krt = TILE; d.rt_desc = 1; d.alpha = -1.0; d.batch1 = batch1; d.swizzle = 2; tri = "upper"
    elif form == "kinv":
        assert M == Ncols == K
        d.kb = K; d.kbeg_ct = TILE; d.upper_only = 1; d.alpha = 1.0; d.epilogue = 3; tri = "lower"
    else:
        raise ValueError(form)
    d.tri = tri
    d.__dict__.update(over)
    # allocations: full K rows of each operand, as the callers have them
    d.lda, d.offA, nA = _place(K, M, pad)
    d.ldb, d.offB, nB = _place(K, Ncols, pad)
    d.ldc, d.offC, nC = _place(M, Ncols, pad)
    if form == "trsm":
        d.lda, d.offA, nA = TILE, (TILE * TILE if pad else 0), TILE * TILE * (3 if pad else 1)        # E_p: tile p of a stack of 128 x 128 blocks
        d.ldb, d.offB, nB = d.ldc, d.offC, 0
    if batch1 > 0:                                      # two-level: batch1 square allocations, the outer index steps along the diagonal of each
        outer = (batch + batch1 - 1) // batch1
        big = max(K, M, Ncols)
        dstep = big + TILE
        ld = (outer - 1) * dstep + big + (2 * TILE if pad else 0)
        rows = (outer - 1) * dstep + big + (5 if pad else 0)
        d.lda = d.ldb = d.ldc = ld
        d.offA = d.offB = d.offC = 3 * ld + TILE if pad else 0
        d.strideA = d.strideB = d.strideC = rows * ld
        d.strideA2 = d.strideB2 = d.strideC2 = dstep * (ld + 1)
        nA = nB = nC = rows * ld * batch1
    else:
        d.strideA, d.strideB, d.strideC = nA, nB, nC
        nA, nB, nC = nA * batch, nB * batch, nC * batch
    d.A = _alloc(nA)
    d.B = None if d.b_alias_c else _alloc(nB)
    if d.epilogue == 1:
        nrt = M // TILE
        d.strideSumsq = nrt * Ncols + (TILE if pad else 0)
        d.offS = 64 if pad else 0
        d.S = _alloc(d.offS + batch * d.strideSumsq + (64 if pad else 0), SENTINEL)
    else:
        d.C = _alloc(nC, np.nan if d.b_alias_c else SENTINEL)
    nan_fill_operands(d, rng, tri=tri, real=real)
    if d.b_alias_c:                                     # everything of C that is not the panel: sentinel
        keep = np.zeros(d.C.size, bool)
        for z in range(batch):
            view2(keep, d.offB + batch_offsets(d, z)[1], d.K, d.ldb, d.Ncols)[:] = True
        d.C[~keep] = SENTINEL
    if d.has_cin:
        for z in range(batch):
            for zz, rt, ct, _, _ in gemm_tiles(d):
                if zz == z:
                    cin = rng.standard_normal((TILE, TILE)) if real else rng.integers(-9, 10, size=(TILE, TILE)).astype(np.float64)
                    if real:                            # magnitudes that differ across the tile, as in the operands
                        cin[:, 3] *= 2.0 ** 20
                        cin[:, TILE - 5] *= 2.0 ** -20
                    view2(d.C, d.offC + batch_offsets(d, z)[2], d.M, d.ldc, d.Ncols)[rt * TILE:(rt + 1) * TILE, ct * d.ctile:(ct + 1) * d.ctile] = cin
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_gemm_f32_sumsq, launch_var_i8: sums of squares of V = A^T B, A upper triangular, row tile rt ends at k = 128 (rt + 1)
# ---------------------------------------------------------------------------------------------------------------------------------
def make_f32(M, Ncols, batch=1, tile128=0, pad=False, real=False, seed=0):
    """capi.hip contract_f32.  The 256-row kernel cannot skip the zero blocks of the diagonal range (gemm_f32.hip): it runs both halves of a
    row pair to the lower half's length, so where the launcher's own condition picks that kernel everything below the diagonal of row tile
    rt up to k = 256 (rt / 2 + 1) is the ZERO the triangular operand has there, and only what lies beyond is NaN.  The cases the launcher
    sends to the 128-row kernel get NaN from k = 128 (rt + 1) on, like the fp64 ones."""
    rng = np.random.default_rng(seed)
    d = gemm_desc(M=M, Ncols=Ncols, K=M, batch=batch, integer=not real, kb=TILE, krt=TILE, rt_desc=1, epilogue=1, tri="upper")
    d.tile128 = tile128
    d.lda, d.offA, nA = _place(M, M, pad)
    d.ldb, d.offB, nB = _place(M, Ncols, pad)
    if pad:                                             # 16-byte vectors of floats: origins in multiples of 4 elements (they are)
        assert d.offA % 4 == 0 and d.offB % 4 == 0
    d.strideA, d.strideB = nA, nB
    d.A, d.B = _alloc(nA * batch), _alloc(nB * batch)
    d.strideSumsq = (M // TILE) * Ncols + (TILE if pad else 0)
    d.offS = 64 if pad else 0
    d.S = _alloc(d.offS + batch * d.strideSumsq + (64 if pad else 0), SENTINEL)
    rows256 = not tile128 and M % (2 * TILE) == 0 and Ncols >= 2048        # launch_gemm_f32_sumsq's condition (K = M)
    nan_fill_operands(d, rng, tri="upper", entries_a=(-1, 1), entries_b=(-1, 0, 1), real=real,
                      zero_rows=(lambda rt: 2 * TILE * (rt // 2 + 1)) if rows256 else None)
    return d


def ref_f32(d):
    """Expected sums buffer of the fp32 launcher (exact / extended arithmetic on the fp64 operands), mask, and the real-mode bound:
    both operands round to float on the way in (1 + u)^2, the K-term float accumulation, then squares and sums in float."""
    out = ref_gemm(d)
    if not d.integer:
        out.boundS[:] = 0.0
        for z, rt, ct, kbeg, kend in gemm_tiles(d):
            oA, oB, _ = batch_offsets(d, z)
            At = view2(d.A, d.offA + oA, d.K, d.lda, d.M)[kbeg:kend, rt * TILE:(rt + 1) * TILE]
            Bt = view2(d.B, d.offB + oB, d.K, d.ldb, d.Ncols)[kbeg:kend, ct * d.ctile:(ct + 1) * d.ctile]
            acc, mag = tile_product(At, Bt, False)
            dv = ((1.0 + U32) ** 2 * (1.0 + gamma(kend - kbeg, U32)) - 1.0) * mag
            o = d.offS + z * d.strideSumsq + rt * d.Ncols + ct * d.ctile
            out.boundS[o:o + d.ctile] = sumsq_bound(acc, dv, U32)
    return out


def make_i8(Np, ncols, m=1, pad=False, real=False, seed=0, zero_col=None, i8_group=0):
    """capi.hip prepare_i8 / contract_i8: A = m matrices Np x Np (leading dimension Np), B = m matrices Np x ncols."""
    rng = np.random.default_rng(seed)
    d = gemm_desc(M=Np, Ncols=ncols, K=Np, batch=m, integer=not real, kb=TILE, krt=TILE, rt_desc=1, epilogue=1, tri="upper", ctile=64)
    d.i8_group = i8_group
    d.lda, d.offA = Np, 0
    d.strideA = Np * Np + (TILE if pad else 0)
    d.A = _alloc(m * d.strideA)
    d.poison = np.zeros(d.A.size, bool)
    d.ldb = ncols + (64 if pad else 0)
    d.offB = 2 * d.ldb + 16 if pad else 0
    d.strideB = (Np + 4) * d.ldb if pad else Np * d.ldb
    d.B = _alloc(m * d.strideB)
    nrt = Np // TILE
    d.strideSumsq = nrt * ncols + (64 if pad else 0)
    d.offS = 32 if pad else 0
    d.S = _alloc(d.offS + m * d.strideSumsq + (32 if pad else 0), SENTINEL)
    k, r = np.arange(Np)[:, None], np.arange(Np)[None, :]
    for z in range(m):
        va = rng.standard_normal((Np, Np)) if real else rng.choice((-3, -2, -1, 1, 2, 3), size=(Np, Np)).astype(np.float64)
        vb = rng.standard_normal((Np, ncols)) if real else rng.integers(-3, 4, size=(Np, ncols)).astype(np.float64)
        if real:
            va[:, 1] *= 2.0 ** 20
            va[:, Np - 3] *= 2.0 ** -20
        va[k > r] = 0.0
        if zero_col is not None:
            va[:, zero_col] = 0.0
        # beyond row tile rt's range k < 128 (rt + 1): NaN would not survive the digit cut (slice_operand_kernel turns it into an arbitrary
        # digit, 0 on this hardware), so the poison is a finite non-zero value of the column's own size -- a pair that runs a chunk too far
        # is an exact mismatch.  (launch_col_exponents reads k <= r only: the exponents do not see it.)
        beyond = np.broadcast_to(k >= TILE * (r // TILE + 1), va.shape)
        diag = np.diagonal(va).copy()
        va[beyond] = np.broadcast_to(np.where(diag != 0.0, diag, 1.0)[None, :], va.shape)[beyond]
        view2(d.A, z * d.strideA, Np, Np, Np)[:] = va
        view2(d.poison, z * d.strideA, Np, Np, Np)[:] = beyond
        view2(d.B, d.offB + z * d.strideB, Np, d.ldb, ncols)[:] = vb
    # one exponent per matrix of B: 2^e >= every |entry| (integer mode: entries up to 3 -> 2)
    d.eB = np.array([2 if not real else int(np.floor(np.log2(np.nanmax(np.abs(view2(d.B, d.offB + z * d.strideB, Np, d.ldb, ncols)))))) + 1 for z in range(m)],
                    dtype=np.int32)
    return d


def ref_i8_exponents(d):
    """e[j][r] = ilogb(max_{k <= r} |A[k][r]|) + 1; an all-zero column keeps the fill."""
    Np = d.M
    out = np.full((d.batch, Np), ZERO_EXPO, dtype=np.int32)
    for z in range(d.batch):
        A = np.nan_to_num(view2(d.A, z * d.strideA, Np, Np, Np), nan=0.0)
        mx = np.abs(np.triu(A)).max(axis=0)
        nz = mx > 0
        out[z, nz] = np.frexp(mx[nz])[1]                  # frexp exponent = ilogb + 1
    return out


def ref_i8(d):
    """Expected sums; real mode: the bound of the fp64 sums of squares (gamma_K |A|^T |B| per element of V, propagated through the squares,
    plus gamma_129 sum v^2) with the digit truncation of 254^-6 of the two column scales per term (header of gemm_i8.hip) added to it."""
    out = ref_gemm(d)
    if not d.integer:
        eA = ref_i8_exponents(d)
        out.boundS[:] = 0.0
        for z, rt, ct, kbeg, kend in gemm_tiles(d):
            At = view2(d.A, z * d.strideA, d.K, d.lda, d.M)[kbeg:kend, rt * TILE:(rt + 1) * TILE]
            Bt = view2(d.B, d.offB + z * d.strideB, d.K, d.ldb, d.Ncols)[kbeg:kend, ct * d.ctile:(ct + 1) * d.ctile]
            acc, mag = tile_product(At, Bt, False)
            scale = np.ldexp(1.0, eA[z, rt * TILE:(rt + 1) * TILE].astype(np.int64) + int(d.eB[z]))[:, None]
            dv = gamma(kend - kbeg, U64) * mag + (kend - kbeg) * 254.0 ** -6 * scale
            o = d.offS + z * d.strideSumsq + rt * d.Ncols + ct * d.ctile
            out.boundS[o:o + d.ctile] = sumsq_bound(acc, dv, U64)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_tile128
# ---------------------------------------------------------------------------------------------------------------------------------
def make_tile128(form, ntiles, K, m=1, pad=False, real=False, seed=0):
    """The launch_tile128 forms of capi_chol.hip:
      row_solve   :54 / :165 / :171  U[p][p+1 ...] = E_p^T A[p][p+1 ...] in place (alpha 1, beta 0, K = 128, B aliases C)
      s1          :166 / :174        trailing tile(s) -= panel^T panel (alpha -1, beta 1, K = 128)
      row_update  :269               block row -= rows^T rows (alpha -1, beta 1, K = 128 q)"""
    rng = np.random.default_rng(seed)
    d = SimpleNamespace(form=form, ntiles=ntiles, K=K, m=m, integer=not real, repeat=1, b_alias_c=0)
    W = ntiles * TILE
    if form == "row_solve":
        assert K == TILE
        d.alpha, d.beta, d.b_alias_c = 1.0, 0.0, 1
    elif form in ("s1", "row_update"):
        d.alpha, d.beta = -1.0, 1.0
    else:
        raise ValueError(form)
    d.lda, d.offA, nA = _place(K, TILE, pad)
    d.ldb, d.offB, nB = _place(K, W, pad)
    d.ldc, d.offC, nC = _place(TILE, W, pad)
    if form == "row_solve":
        d.lda, d.offA, nA = TILE, (TILE * TILE if pad else 0), TILE * TILE * (3 if pad else 1)
        d.ldb, d.offB, nB = d.ldc, d.offC, 0
    d.strideA, d.strideB, d.strideC = nA, (nC if d.b_alias_c else nB), nC
    d.A, d.B, d.C = _alloc(nA * m), (None if d.b_alias_c else _alloc(nB * m)), _alloc(nC * m, SENTINEL)
    def draw(shape):
        if not real:
            return rng.integers(-3, 4, size=shape).astype(np.float64)
        v = rng.standard_normal(shape)                  # a few columns scaled by 2^+-20: magnitudes differ across a tile
        for c, e in ((1, 20), (shape[1] - 3, -20), (shape[1] // 2 + 5, 20)):
            v[:, c] *= 2.0 ** e
        return v

    for z in range(m):
        view2(d.A, d.offA + z * d.strideA, K, d.lda, TILE)[:] = draw((K, TILE))
        if d.b_alias_c:
            view2(d.C, d.offC + z * d.strideC, TILE, d.ldc, W)[:] = draw((TILE, W))
        else:
            view2(d.B, d.offB + z * d.strideB, K, d.ldb, W)[:] = draw((K, W))
            view2(d.C, d.offC + z * d.strideC, TILE, d.ldc, W)[:] = draw((TILE, W))
    return d


def ref_tile128(d):
    out = SimpleNamespace(C=d.C.astype(np.longdouble), maskC=np.zeros(d.C.size, bool), boundC=np.zeros(d.C.size), absprod=0.0)
    W = d.ntiles * TILE
    for z in range(d.m):
        A = view2(d.A, d.offA + z * d.strideA, d.K, d.lda, TILE)
        B = view2(d.C if d.b_alias_c else d.B, d.offB + z * d.strideB, d.K, d.ldb, W)
        cin = view2(d.C, d.offC + z * d.strideC, TILE, d.ldc, W)
        for t in range(d.ntiles):
            cols = slice(t * TILE, (t + 1) * TILE)
            acc, mag = tile_product(A, B[:, cols], d.integer)
            out.absprod = max(out.absprod, float(mag.max()))
            if d.integer:
                val = int(d.alpha) * acc + (int(d.beta) * cin[:, cols].astype(np.int64) if d.beta != 0.0 else 0)
            else:
                val = np.longdouble(d.alpha) * acc + (np.longdouble(d.beta) * cin[:, cols].astype(np.longdouble) if d.beta != 0.0 else 0)
            bound = gamma(d.K + 2, U64) * (abs(d.alpha) * mag + (abs(d.beta) * np.abs(cin[:, cols]) if d.beta != 0.0 else 0.0)) + U64 * np.abs(val).astype(np.float64)
            view2(out.C, d.offC + z * d.strideC, TILE, d.ldc, W)[:, cols] = val
            view2(out.maskC, d.offC + z * d.strideC, TILE, d.ldc, W)[:, cols] = True
            view2(out.boundC, d.offC + z * d.strideC, TILE, d.ldc, W)[:, cols] = bound
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_gemm_kernels.py (and of the CPU-side checks on the same inputs): name -> (kind, builder)
# ---------------------------------------------------------------------------------------------------------------------------------
def _f64(form, *a, **kw):
    return "f64", functools.partial(make_f64, form, *a, **kw)


CASES = {}


def _add(name, kind_builder):
    assert name not in CASES, name
    CASES[name] = kind_builder


# capi.hip contract_f64: sums of squares.  128-row kernel (swizzle 0: two tiles ahead; prefetch1: one), M, Ncols in {128, 384}
for M, N in ((128, 128), (128, 384), (384, 128), (384, 384)):
    _add("contract_f64-k128-M%d-N%d" % (M, N), _f64("variance", M, N, batch=3 if (M, N) == (384, 128) else 1, pad=(M, N) == (384, 384)))
_add("contract_f64-k128-prefetch1-M384-N384", _f64("variance", 384, 384, prefetch1=1, batch=3, pad=True))
# swizzle 258: the three-buffer 256-row kernel, M in {256, 512, 768}; M = 384 falls back to the 128-row kernel
for M, N in ((256, 128), (256, 384), (512, 128), (512, 384), (768, 128), (768, 384)):
    _add("contract_f64-x3-M%d-N%d" % (M, N), _f64("variance", M, N, swizzle=258, batch=3 if (M, N) == (512, 128) else 1, pad=(M, N) == (768, 384)))
_add("contract_f64-x3-fallback-M384-N384", _f64("variance", 384, 384, swizzle=258))
# the tile queue: tiles = (M / 256) nct batch
_add("contract_f64-queue-ncu1-8tiles", _f64("variance", 512, 256, swizzle=258, batch=2, use_queue=1, ncu=1, repeat=2, pad=True))
_add("contract_f64-queue-ncu3-7tiles", _f64("variance", 256, 128, swizzle=258, batch=7, use_queue=1, ncu=3, repeat=2))
_add("contract_f64-queue-ncu3-8tiles", _f64("variance", 512, 256, swizzle=258, batch=2, use_queue=1, ncu=3, repeat=2))
_add("contract_f64-queue-ncu-equals-tiles", _f64("variance", 768, 384, swizzle=258, batch=1, use_queue=1, ncu=9, repeat=2))
_add("contract_f64-queue-ncu-above-tiles", _f64("variance", 512, 384, swizzle=258, batch=1, use_queue=1, ncu=64, repeat=2))
# probes-only correct variants of the same contraction: the two-buffer 256-row kernel
for sw in (256, 257):
    _add("contract_f64-two-buffer-swizzle%d-M512-N384" % sw, _f64("variance", 512, 384, swizzle=sw, batch=3, pad=True))
    _add("contract_f64-two-buffer-swizzle%d-M256-N128" % sw, _f64("variance", 256, 128, swizzle=sw))
# V = R^T K* stored (capi.hip predict_gradients, capi_thompson.hip:53): 128-row 8-wave kernel below 512 rows, store form of the three-buffer kernel from 512
for M, N in ((128, 384), (256, 128), (384, 384)):
    _add("predict_gradients-V-k128-M%d-N%d" % (M, N), _f64("v_store", M, N, batch=3 if M == 256 else 1, pad=M == 384))
for M, N in ((512, 128), (512, 384), (768, 384)):
    _add("predict_gradients-V-x3store-M%d-N%d" % (M, N), _f64("v_store", M, N, batch=3 if (M, N) == (512, 128) else 1, pad=M == 768))
# the no_x3 switch (no caller of this form sets it): an M >= 512 V-store kept on the 128-row kernel
_add("no_x3-switch-V-k128-M512-N128", _f64("v_store", 512, 128, no_x3=1))
# W = R V with kbeg_rt = 128 (predict_gradients second product, capi_kg.hip:41)
for M, N in ((128, 128), (384, 384), (512, 128)):
    _add("capi_kg-W-M%d-N%d" % (M, N), _f64("w_store", M, N, batch=3 if M == 384 else 1, pad=M == 384))
# the factorization
for W in (128, 384):
    _add("capi_chol-trsm-W%d" % W, _f64("trsm", 128, W, batch=3 if W == 384 else 1, pad=W == 384))
for rows, W in ((1, 128), (1, 384), (2, 384), (3, 384)):
    _add("capi_chol-syrk-rows%d-W%d" % (rows, W), _f64("syrk", rows * 128, W, K=128, batch=3 if rows == 2 else 1, pad=rows == 2))
for g, nct in ((1, 1), (1, 2), (2, 3), (4, 5), (2, 2), (4, 3)):
    _add("capi_chol-trailing-g%d-nct%d" % (g, nct), _f64("trailing", nct * 128, nct * 128, K=g * 128, batch=3 if nct == 2 else 1, pad=nct == 3))
for q, W in ((1, 128), (2, 384), (3, 384)):
    _add("capi_chol-row_update-q%d-W%d" % (q, W), _f64("row_update", 128, W, K=q * 128, batch=3 if q == 2 else 1, pad=q == 2))
# the inverse merges: batch1 = m with two values of the outer index
for b1n, m, count in ((1, 1, 2), (2, 2, 2), (3, 2, 1)):
    _add("capi_chol-merge_first-b%d-m%d-count%d" % (b1n, m, count), _f64("merge_first", b1n * 128, (b1n % 3 + 1) * 128, batch=m * count, batch1=m, pad=b1n == 2))
    _add("capi_chol-merge_second-b%d-m%d-count%d" % (b1n, m, count), _f64("merge_second", b1n * 128, (b1n % 3 + 1) * 128, batch=m * count, batch1=m, pad=b1n == 2, no_x3=1))
for M, m, count, nx in ((512, 1, 2, 0), (512, 2, 2, 1), (768, 2, 1, 0), (256, 1, 2, 0)):
    _add("capi_chol-merge_second-M%d-m%d-count%d-no_x3_%d" % (M, m, count, nx), _f64("merge_second", M, 128 if M != 768 else 384, batch=m * count, batch1=m, no_x3=nx, pad=M == 512 and m == 1))
# Ky^-1 = R R^T on upper tiles (capi_fit.hip:656)
for nct in (1, 2, 3, 5):
    _add("capi_fit-kinv-nct%d" % nct, _f64("kinv", nct * 128, nct * 128, batch=3 if nct == 2 else 1, pad=nct == 3))
# fp32
_add("contract_f32-tile128-M384-N384", ("f32", functools.partial(make_f32, 384, 384, tile128=1, batch=3, pad=True)))
_add("contract_f32-tile128-M256-N2048", ("f32", functools.partial(make_f32, 256, 2048, tile128=1)))
_add("contract_f32-k128-small-N-M256-N384", ("f32", functools.partial(make_f32, 256, 384)))
_add("contract_f32-x3-M256-N2048", ("f32", functools.partial(make_f32, 256, 2048, batch=2)))
_add("contract_f32-x3-M512-N2048", ("f32", functools.partial(make_f32, 512, 2048, pad=True)))
_add("contract_f32-k128-odd-M384-N2048", ("f32", functools.partial(make_f32, 384, 2048)))
# int8
for Np in (128, 256, 384):
    for nc in (64, 192):
        for grp in (0, 1, 2):
            _add("contract_i8-Np%d-N%d-group%d" % (Np, nc, grp),
                 ("i8", functools.partial(make_i8, Np, nc, m=3 if (Np, nc) == (256, 64) else 1, pad=(Np, nc) == (384, 192), seed=grp, i8_group=grp)))
_add("contract_i8-zero-column-Np128-N64-group0", ("i8", functools.partial(make_i8, 128, 64, zero_col=5)))
# launch_tile128
for nt in (1, 3):
    _add("capi_chol-tile128-row_solve-ntiles%d-K128" % nt, ("t128", functools.partial(make_tile128, "row_solve", nt, 128, m=3 if nt == 3 else 1, pad=nt == 3)))
    _add("capi_chol-tile128-s1-ntiles%d-K128" % nt, ("t128", functools.partial(make_tile128, "s1", nt, 128, m=2 if nt == 1 else 1, pad=nt == 1)))
    for K in (128, 384):
        _add("capi_chol-tile128-row_update-ntiles%d-K%d" % (nt, K), ("t128", functools.partial(make_tile128, "row_update", nt, K, m=2 if K == 384 else 1, pad=K == 384 and nt == 3)))

# real mode: one or two shapes per kernel
REAL_CASES = {
    "real-contract_f64-k128-M384-N384": _f64("variance", 384, 384, real=True, pad=True),
    "real-contract_f64-x3-M768-N384": _f64("variance", 768, 384, swizzle=258, real=True),
    "real-contract_f64-queue-M512-N256": _f64("variance", 512, 256, swizzle=258, batch=2, use_queue=1, ncu=3, real=True),
    "real-contract_f64-two-buffer-M512-N128": _f64("variance", 512, 128, swizzle=256, real=True),
    "real-predict_gradients-V-k128-M384-N128": _f64("v_store", 384, 128, real=True),
    "real-predict_gradients-V-x3store-M768-N128": _f64("v_store", 768, 128, real=True, pad=True),
    "real-capi_kg-W-M384-N128": _f64("w_store", 384, 128, real=True),
    "real-capi_chol-trailing-g2-nct3": _f64("trailing", 384, 384, K=256, real=True, pad=True),
    "real-capi_chol-row_update-q3-W384": _f64("row_update", 128, 384, K=384, real=True),
    "real-contract_f32-tile128-M384-N384": ("f32", functools.partial(make_f32, 384, 384, tile128=1, real=True)),
    "real-contract_f32-x3-M256-N2048": ("f32", functools.partial(make_f32, 256, 2048, real=True)),
    "real-contract_i8-Np384-N192": ("i8", functools.partial(make_i8, 384, 192, real=True, pad=True)),
    "real-contract_i8-Np256-N64": ("i8", functools.partial(make_i8, 256, 64, real=True, m=2)),
    "real-capi_chol-tile128-row_update-ntiles3-K384": ("t128", functools.partial(make_tile128, "row_update", 3, 384, real=True, pad=True)),
    "real-capi_chol-tile128-row_solve-ntiles3-K128": ("t128", functools.partial(make_tile128, "row_solve", 3, 128, real=True)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(kind, descriptor, reference) of a case: built once, shared by every test that needs it, never modified (tests copy the buffers)."""
    kind, build = (CASES.get(name) or REAL_CASES[name])
    d = build()
    ref = {"f64": ref_gemm, "f32": ref_f32, "i8": ref_i8, "t128": ref_tile128}[kind](d)
    return kind, d, ref
