"""CPU-only checks of the predict planner (bocf_amd/csrc/predict_plan.h): plan_predict decides how one predict pass runs before anything is
enqueued -- the contraction kind, the chunking, the variance-GEMM tiling and the bytes of every workspace buffer.  A table of decisions, the
workspace cap, and the byte counts against a restatement of the sizing rules over a sweep.  The header is driven through
tests/predict_plan_driver.cpp."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
MEAN, SMALL, F64, F32, I8 = range(5)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ next to hipcc")
    exe = str(tmp_path_factory.mktemp("predict_plan") / "predict_plan_driver")
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "predict_plan_driver.cpp"), "-o", exe])
    return exe


# config 2 (m = 4 outputs, d = 6, N = 1024, 8192 candidates) asking for variances; options at their defaults
BASE = dict(C=8192, N=1024, Np=1024, m=4, d=6, pred_cap=0, need_var=1, need_grad=0, chunk=65536, workspace_mb=24576, small_path=1,
            predict_f32=0, predict_i8=0, swizzle=-1)


def plans(driver, cases):
    lines = [" ".join("%s=%d" % kv for kv in dict(BASE, **case).items()) for case in cases]
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return [dict((k, int(v)) for k, v in (tok.split("=") for tok in line.split())) for line in out if line]


def plan(driver, **case):
    return plans(driver, [case])[0]


# (inputs and options, expected fields of the plan)
TABLE = [
    # config 2: the fp64 GEMM in 256-row tiles, all 8192 candidates in one pass
    (dict(), dict(kind=F64, tiling=258, passes=1, chunkpad=8192, mean_with_var=1)),
    (dict(C=1024), dict(kind=F64, tiling=0, passes=1)),
    (dict(C=2048), dict(kind=F64, tiling=258)),
    (dict(chunk=1024), dict(kind=F64, tiling=0, passes=8, chunkpad=1024)),
    (dict(swizzle=0), dict(kind=F64, tiling=0)),
    (dict(C=1024, swizzle=258), dict(kind=F64, tiling=258)),
    # <= 16 candidates: the small path, the fp64 GEMM without it; fp32 does not take them from the small path
    (dict(C=16), dict(kind=SMALL, chunkpad=128)),
    (dict(C=1), dict(kind=SMALL)),
    (dict(C=17), dict(kind=F64)),
    (dict(C=16, small_path=0), dict(kind=F64)),
    (dict(C=16, predict_f32=1), dict(kind=SMALL)),
    (dict(C=16, need_grad=1), dict(kind=SMALL)),
    # fp32 before int8; neither with gradients; int8 up to Np = 16384
    (dict(predict_f32=1), dict(kind=F32)),
    (dict(predict_f32=1, predict_i8=1), dict(kind=F32)),
    (dict(predict_i8=1), dict(kind=I8)),
    (dict(predict_f32=1, need_grad=1), dict(kind=F64)),
    (dict(predict_i8=1, need_grad=1), dict(kind=F64)),
    (dict(predict_i8=1, N=16384, Np=16384), dict(kind=I8)),
    (dict(predict_i8=1, N=16500, Np=16512), dict(kind=F64)),
    # means only: no variance finalisation, whatever the options
    (dict(need_var=0), dict(kind=MEAN, mean_with_var=0)),
    (dict(need_var=0, C=16, predict_f32=1, predict_i8=1), dict(kind=MEAN)),
]


def test_pinned_decisions(driver):
    got = plans(driver, [case for case, _ in TABLE])
    for (case, want), p in zip(TABLE, got):
        assert {k: p[k] for k in want} == want, (case, p)


def test_workspace_cap(driver):
    """The chunk is lowered so that K* of all outputs fits workspace_mb: a multiple of 128, at least 128, about half as many columns when the
    gradient path needs V as well."""
    for N, m, mb in ((1024, 4, 64), (4096, 4, 100), (4096, 8, 1000), (1024, 1, 24576)):
        v = plan(driver, C=1 << 20, N=N, Np=N, m=m, workspace_mb=mb)
        g = plan(driver, C=1 << 20, N=N, Np=N, m=m, workspace_mb=mb, need_grad=1)
        for p in (v, g):
            assert p["chunk"] % 128 == 0 and 128 <= p["chunk"] <= 65536, (N, m, mb, p)
        per_col = 8 * m * N
        if v["chunk"] < 65536:
            assert v["chunk"] * per_col <= mb << 20 < (v["chunk"] + 128) * per_col, (N, m, mb, v)
            assert abs(g["chunk"] - v["chunk"] / 2) <= 128, (N, m, mb, v["chunk"], g["chunk"])
    tiny = plan(driver, C=4096, N=16384, Np=16384, m=64, workspace_mb=1)
    assert tiny["chunk"] == 128 and tiny["passes"] == 32


def test_mean_only_has_no_kstar_workspace(driver):
    p = plan(driver, need_var=0)
    assert p["kstar"] == 0 and p["sumsq"] == 0 and p["vs"] == 0 and p["vbuf"] == 0 and p["ki8"] == 0 and p["r32"] == 0
    assert p["meanpart"] > 0 and p["mean"] > 0


def test_columns_of_the_results(driver):
    """mean / var / acq keep their columns when they already hold enough: the leading dimension never shrinks."""
    assert plan(driver, C=1000)["ld"] == 1024
    assert plan(driver, C=1000, pred_cap=8192)["ld"] == 8192
    assert plan(driver, C=1000, pred_cap=512)["ld"] == 1024


def rules(c):
    """The sizing rules of a predict pass restated: bytes of every buffer it grows (0: not touched)."""
    C, Np, m, d, need_var, need_grad = c["C"], c["Np"], c["m"], c["d"], c["need_var"], c["need_grad"]
    rup = lambda x: (x + 127) // 128 * 128
    nrt = Np // 128
    per_col = m * Np * 8.0 * (2.0 if need_grad else 1.0)
    fit_cols = max(int(c["workspace_mb"] * 1048576.0 / per_col) // 128 * 128, 128)
    chunk = min(c["chunk"], fit_cols)
    chunkpad = rup(C) if C < chunk else chunk
    ld = rup(C) if c["pred_cap"] < C else c["pred_cap"]
    small = C <= 16 and c["small_path"]
    f32 = c["predict_f32"] and need_var and not need_grad and not small
    i8 = c["predict_i8"] and need_var and not need_grad and not small and not f32 and Np <= 16384
    i8b = lambda n: m * 6 * (Np // 64) * (n // 16) * 1024
    b = dict(mean=8 * m * ld, var=8 * m * ld, acq=8 * ld, meanpart=8 * 2 * m * nrt * max(chunkpad, Np))
    b["kstar"] = 8 * m * Np * chunkpad if need_var else 0
    b["sumsq"] = 8 * m * (Np // 16 if C <= 16 else nrt) * chunkpad if need_var else 0
    b["vs"] = b["ws"] = 8 * m * Np * 16 if small and need_var else 0
    b["vbuf"] = 8 * m * Np * chunkpad if need_grad and not small else 0
    b["dmean"] = b["dvar"] = 8 * m * ld * d if need_grad else 0
    b["dacq"] = 8 * ld * d if need_grad else 0
    b["r32"] = 4 * m * Np * Np if f32 else 0
    b["ki8"], b["ki8e"], b["ri8"], b["ri8e"] = (i8b(chunkpad), 4 * m, i8b(Np), 4 * m * Np) if i8 else (0, 0, 0, 0)
    return dict(b, chunk=chunk, chunkpad=chunkpad, ld=ld)


def test_bytes_over_a_sweep(driver):
    opts = (dict(), dict(small_path=0), dict(predict_f32=1), dict(predict_i8=1), dict(chunk=2048, workspace_mb=300))
    cases = [dict(C=C, N=Np - 5, Np=Np, m=m, need_var=v, need_grad=g, pred_cap=cap, **o)
             for C, Np, m, (v, g), o, cap in itertools.product((1, 16, 17, 1000, 8192, 70000), (128, 1024, 16512), (1, 4, 64),
                                                                ((1, 0), (0, 0), (1, 1)), opts, (0, 65536))]
    for case, p in zip(cases, plans(driver, cases)):
        want = rules(dict(BASE, **case))
        assert {k: p[k] for k in want} == want, case
