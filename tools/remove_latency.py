"""Wall time of the removal of one observation from the resident factor (bocf_remove) at N = 1024 / 4096, d = 6,
m = 4, next to a from-scratch bocf_fit of the same N - 1 points in the same process.

    python tools/remove_latency.py [--reps 7] [--out profiles/remove/latency.json]

Per N and removed index k = 0 (every rotation: the worst case), N / 2 and N - 1 (none): `reps` rounds of [fit N points (untimed) ->
bocf_remove(k) (timed) -> bocf_fit of the N - 1 survivors (timed)], wall clock around each call (both end with their one host
synchronisation), medians; and the device time of the removal's two phases (bocf_profile_phase "remove": the four factor kernels and the
input shift; "remove_alpha": the alpha solve, refinement and log-marginal that every target refresh runs).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bocf_amd import _ffi                                           # noqa: E402


def phase_ms(ctx, name):
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    _ffi.check(_ffi.load().bocf_profile_phase(ctx.handle, name.encode(), ctypes.byref(ms), ctypes.byref(n), 1), "bocf_profile_phase")
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d, m = 6, 4
    lib, dp = _ffi.load(), _ffi.dptr
    rows = []
    for N in (1024, 4096):
        rng = np.random.RandomState(N)
        X = _ffi.f64(rng.uniform(size=(N, d)))
        Y = _ffi.f64(np.stack([np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1) + 1e-3 * rng.normal(size=N) for j in range(m)]))
        var, ls, noise = _ffi.f64(np.ones(m)), _ffi.f64(np.full((m, d), 0.3)), _ffi.f64(np.full(m, 1e-4))
        jit, lml = np.zeros(m), np.zeros(m)
        ctx = _ffi.Context(0)

        def fit(Xf, Yf):
            rc = lib.bocf_fit(ctx.handle, dp(Xf), dp(Yf), Xf.shape[0], d, m, _ffi.KERN_MATERN52, dp(var), dp(ls), dp(noise), 5, dp(jit), dp(lml))
            _ffi.check(rc, "bocf_fit")
            assert rc == 0 and np.all(jit == 0), "the problem needs jitter: the removal would be refused"
        for k in (0, N // 2, N - 1):
            X1, Y1 = _ffi.f64(np.delete(X, k, axis=0)), _ffi.f64(np.delete(Y, k, axis=1))
            t_rm, t_fit, dev, dev_alpha = [], [], [], []
            for rep in range(a.reps + 1):                                  # (round 0 warms both paths up and is dropped)
                ctx.set_option("profile", 0)
                fit(X, Y)
                ctx.set_option("profile", 1)
                phase_ms(ctx, "remove"), phase_ms(ctx, "remove_alpha")
                t0 = time.perf_counter()
                rc = lib.bocf_remove(ctx.handle, k, dp(Y1), dp(lml))
                t1 = time.perf_counter()
                assert _ffi.check(rc, "bocf_remove") == 0
                lml_removed = lml.copy()
                dev.append(phase_ms(ctx, "remove"))
                dev_alpha.append(phase_ms(ctx, "remove_alpha"))
                ctx.set_option("profile", 0)
                t2 = time.perf_counter()
                fit(X1, Y1)
                t3 = time.perf_counter()
                assert np.allclose(lml_removed, lml, rtol=1e-8), (lml_removed, lml)      # the same model either way
                if rep:
                    t_rm.append(1e3 * (t1 - t0))
                    t_fit.append(1e3 * (t3 - t2))
            row = dict(N=N, d=d, m=m, k=k, reps=a.reps, remove_wall_ms=round(float(np.median(t_rm)), 4), refit_wall_ms=round(float(np.median(t_fit)), 4),
                       remove_factor_kernels_ms=round(float(np.median(dev[1:])), 4), remove_alpha_phase_ms=round(float(np.median(dev_alpha[1:])), 4),
                       remove_wall_ms_all=[round(t, 4) for t in t_rm], refit_wall_ms_all=[round(t, 4) for t in t_fit])
            row["refit_over_remove"] = round(row["refit_wall_ms"] / row["remove_wall_ms"], 2)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        ctx.close()
    out = {"remove_latency": rows}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
