"""Phases of one CompositeThompsonBatch.compute_batch (q = 16, m = 4, d = 6, fixed hyper-parameters) at C in {4096, 8192} candidates and
N in {1024, 4096} observations: covariance (cross kernel + V = R^T K + the Sigma kernel), factorization of Sigma, samples, selection
(device events, bocf_profile_phase) and the whole compute_batch (wall clock, acquisition optimisation included).  The covariance's
achieved fraction of the 78.6 TFLOP/s fp64 matrix peak counts m N^2 C flops for V and m N C^2 for the symmetric Sigma.

    python tools/thompson_latency.py [--reps 3]

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

PEAK = 78.6e12
PHASES = ("post_cov", "post_chol", "post_samples", "thompson_select")


def phase(model, name):
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    _ffi.check(_ffi.load().bocf_profile_phase(model._context().handle, name.encode(), ctypes.byref(ms), ctypes.byref(n), 1), "bocf_profile_phase")
    return ms.value


def case(N, C, reps, m=4, d=6, q=16):
    rng = np.random.RandomState(N + C)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.5, ARD=True) for _ in range(m)], noise_var=[1e-3] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=rng.normal(size=(4, m)), prob_dist=np.full(4, 0.25)), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, space, optimizer=B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=8), utility=U)
    ev = B.CompositeThompsonBatch(acq, q, n_candidates=C)
    model.set_option("profile", 1)
    np.random.seed(0)
    ev.compute_batch()                                             # warm-up: code objects, allocations
    for p in PHASES:
        phase(model, p)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ev.compute_batch()
        wall.append((time.perf_counter() - t0) * 1e3)
    ms = {p: phase(model, p) / reps for p in PHASES}
    flops = m * float(N) ** 2 * C + m * float(N) * C * C
    return {"N": N, "C": C, "m": m, "q": q, "cov_ms": round(ms["post_cov"], 3), "chol_ms": round(ms["post_chol"], 3),
            "samples_ms": round(ms["post_samples"], 3), "select_ms": round(ms["thompson_select"], 3),
            "compute_batch_ms": round(float(np.median(wall)), 2), "cov_gflop": round(flops / 1e9, 1),
            "cov_frac_fp64_peak": round(flops / (ms["post_cov"] * 1e-3) / PEAK, 3), "jitter_max": float(np.max(model.last_sample_jitter))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    out = [case(N, C, a.reps) for N in (1024, 4096) for C in (4096, 8192)]
    print(json.dumps({"thompson_latency": out}))


if __name__ == "__main__":
    main()
