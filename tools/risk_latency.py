"""Latency of the quantile / tail-mean acquisition next to bocf_acq_mc on the same shape, in the same process (m = 4, d = 6, fixed
hyper-parameters, L = 4 weighted parameters, S in {64, 256, 1024} samples, the three kinds at the rank of level 0.9) at (N, C) in
{(1024, 8192), (4096, 65536)}: one alpha call over the C candidates (wall clock, values left on the device; and the acquisition phase
alone -- device events, bocf_profile_phase "acq": the kernel) and value + gradient on 16 points, f_df(16) (wall clock).  The closed-form
confidence bound is timed next to bocf_acq_linear the same way.

    python tools/risk_latency.py [--reps 5] [--small]

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bocf_amd as B                                               # noqa: E402
from bocf_amd import _ffi                                          # noqa: E402
from bocf_amd.acquisitions import risk_rank                        # noqa: E402

KINDS = (("quantile", _ffi.RISK_QUANTILE), ("upper_tail", _ffi.RISK_UPPER_TAIL), ("lower_tail", _ffi.RISK_LOWER_TAIL))


def phase(model, name):
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    _ffi.check(_ffi.load().bocf_profile_phase(model._context().handle, name.encode(), ctypes.byref(ms), ctypes.byref(n), 1), "bocf_profile_phase")
    return ms.value


def med(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def timed(model, run, fdf, reps):
    """(wall ms of run, its acquisition phase in ms, wall ms of fdf), medians / means over reps after one warm-up each."""
    run()
    phase(model, "acq")
    wall = med(run, reps)
    acq_ms = phase(model, "acq") / reps
    fdf()
    return round(wall, 3), round(acq_ms, 4), round(med(fdf, max(reps, 5)), 3)


def case(N, C, reps, m=4, d=6, L=4):
    rng = np.random.RandomState(N + C)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.5, ARD=True) for _ in range(m)], noise_var=[1e-3] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    Xc = rng.uniform(size=(C, d))
    thetas, prob = rng.normal(size=(L, m)), np.full(L, 1.0 / L)
    kind = _ffi.UTIL_NEG_SQ_DIST
    out = {"N": N, "C": C, "m": m, "d": d, "L": L}
    model.set_option("profile", 1)
    X16 = Xc[:16]
    for S in (64, 256, 1024):
        W = rng.normal(size=(S, m))
        k = risk_rank(0.9, S)
        wall, acq_ms, fdf = timed(model, lambda: model.acq_mc(Xc, _ffi.ACQ_EI, kind, None, thetas, prob, W=W, fetch=False),
                                  lambda: model.acq_mc_grad(X16, kind, None, thetas, prob, W=W), reps)
        row = {"rank": k, "acq_mc": {"wall_ms": wall, "acq_phase_ms": acq_ms, "f_df_16_wall_ms": fdf}}
        for name, rk in KINDS:
            w, a, f = timed(model, lambda: model.acq_risk(Xc, rk, k, kind, None, thetas, prob, W=W, fetch=False),
                            lambda: model.acq_risk(X16, rk, k, kind, None, thetas, prob, W=W, grad=True), reps)
            row[name] = {"wall_ms": w, "acq_phase_ms": a, "f_df_16_wall_ms": f, "acq_phase_ratio_to_acq_mc": round(a / acq_ms, 3),
                         "wall_ratio_to_acq_mc": round(w / wall, 3), "f_df_16_ratio_to_acq_mc": round(f / fdf, 3)}
        out["S%d" % S] = row
    wall, acq_ms, fdf = timed(model, lambda: model.acq_linear(Xc, _ffi.ACQ_EI, thetas, prob), lambda: model.acq_linear_grad(X16, _ffi.ACQ_EI, thetas, prob), reps)
    w, a, f = timed(model, lambda: model.acq_linear_ucb(Xc, 2.0, thetas, prob), lambda: model.acq_linear_ucb(X16, 2.0, thetas, prob, grad=True), reps)
    out["linear"] = {"acq_linear": {"wall_ms": wall, "acq_phase_ms": acq_ms, "f_df_16_wall_ms": fdf},
                     "linear_ucb": {"wall_ms": w, "acq_phase_ms": a, "f_df_16_wall_ms": f, "acq_phase_ratio_to_acq_linear": round(a / acq_ms, 3),
                                    "wall_ratio_to_acq_linear": round(w / wall, 3)}}
    model.set_option("profile", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="only (N = 1024, C = 8192)")
    a = ap.parse_args()
    shapes = [(1024, 8192)] if a.small else [(1024, 8192), (4096, 65536)]
    print(json.dumps({"risk_latency": [case(N, C, a.reps) for N, C in shapes]}))


if __name__ == "__main__":
    main()
