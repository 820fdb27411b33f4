"""Wall time of the leave-one-out pass (bocf_loo) at N = 1024 / 4096, d = 6, m = 4, H = 1 and 10 resident
hyper-samples, next to the bytes it must read: the upper triangles of the M = H m inverse factors (M N (N + 1) / 2 doubles; the kernel
starts every row at its 64-aligned column, which the second figure counts).

    python tools/loo_latency.py [--reps 20] [--out profiles/loo/latency.json]

Per configuration: the whole call with no output (results stay on the device), with the sums only, and with all three (M, N) arrays
copied back (wall clock, median), and the kernels' phase alone (device events, bocf_profile_phase "loo").  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bocf_amd as B                                               # noqa: E402
from bocf_amd import _ffi                                           # noqa: E402


def phase_ms(model, name):
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    _ffi.check(_ffi.load().bocf_profile_phase(model._context().handle, name.encode(), ctypes.byref(ms), ctypes.byref(n), 1), "bocf_profile_phase")
    return ms.value


def model_with_hyper_samples(N, d, m, H, seed=0):
    """H hyper-samples resident on the device without running the sampler: sample h scales the variances by 1 + 0.02 h and the
    lengthscales by 1 - 0.01 h."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] + 1e-3 * rng.normal(size=(N, 1)) for j in range(m)]
    model = B.multi_outputGP(m, fixed_hyps=False, n_samples=H)
    model._X, model._Y = np.ascontiguousarray(X), [y.copy() for y in Y]
    model._kernel_ids = [_ffi.KERN_SE] * m
    model._instances = [[(1.0 + 0.02 * h, np.full(d, 0.5 * (1 - 0.01 * h)), 1e-4) for _ in range(m)] for h in range(H)]
    model._fit()
    return model


def median_ms(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d, m = 6, 4
    lib, dp = _ffi.load(), _ffi.dptr
    rows = []
    for N in (1024, 4096):
        for H in (1, 10):
            model = model_with_hyper_samples(N, d, m, H)
            h, M = model._context().handle, m * H
            flags = _ffi.ADD_NOISE | _ffi.CLIP
            mean, var, lpd, tot = np.empty((M, N)), np.empty((M, N)), np.empty((M, N)), np.empty(M)
            row = dict(N=N, d=d, m=m, H=H, factorizations=M)
            row["upper_triangle_bytes"] = M * N * (N + 1) // 2 * 8
            row["bytes_from_aligned_row_starts"] = M * 8 * int(sum(N - (r & ~63) for r in range(N)))
            row["wall_ms_no_output"] = round(median_ms(lambda: _ffi.check(lib.bocf_loo(h, flags, None, None, None, None), "bocf_loo"), a.reps), 4)
            row["wall_ms_sums_only"] = round(median_ms(lambda: _ffi.check(lib.bocf_loo(h, flags, None, None, None, dp(tot)), "bocf_loo"), a.reps), 4)
            row["wall_ms_all_outputs"] = round(median_ms(lambda: _ffi.check(lib.bocf_loo(h, flags, dp(mean), dp(var), dp(lpd), dp(tot)), "bocf_loo"),
                                                         a.reps), 4)
            model.set_option("profile", 1)
            phase_ms(model, "loo")
            dev = []
            for _ in range(a.reps):
                _ffi.check(lib.bocf_loo(h, flags, None, None, None, None), "bocf_loo")
                dev.append(phase_ms(model, "loo"))
            row["kernel_ms"] = round(float(np.median(dev)), 4)
            row["kernel_GBps_of_read_bytes"] = round(row["bytes_from_aligned_row_starts"] / (row["kernel_ms"] * 1e-3) / 1e9, 1)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            model._ctx.close()
            model._ctx = None
    out = {"loo_latency": rows}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
