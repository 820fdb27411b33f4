"""Pathwise Thompson sampling (m = 4, d = 6, q = 16, F = 1024 features, fixed hyper-parameters) at N in {1024, 4096} observations and
C in {8192, 65536} candidates: staging (bocf_set_paths), the value kernel (bocf_path_values), selection, the refinement's value-and-gradient
calls (device events, bocf_profile_phase) and a whole CompositePathwiseThompsonBatch.compute_batch (wall clock, acquisition optimisation
included).  Next to it, from the same process: the cross kernel's time for the same (N, C, m) -- the mean-only predict pass, the path
kernel's vector-ALU yardstick -- and CompositeThompsonBatch.compute_batch at C in {4096, 8192}.

    python tools/paths_latency.py [--reps 3]

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

PHASES = ("paths_stage", "path_values", "thompson_select", "path_utility", "cross")


def phase(model, name):
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    _ffi.check(_ffi.load().bocf_profile_phase(model._context().handle, name.encode(), ctypes.byref(ms), ctypes.byref(n), 1), "bocf_profile_phase")
    return ms.value, n.value


def problem(N, m=4, d=6):
    rng = np.random.RandomState(N)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.5, ARD=True) for _ in range(m)], noise_var=[1e-3] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=rng.normal(size=(4, m)), prob_dist=np.full(4, 0.25)), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, space, optimizer=B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=8), utility=U)
    model.set_option("profile", 1)
    return model, acq


def timed(ev, reps):
    np.random.seed(0)
    ev.compute_batch()                                             # warm-up: code objects, allocations
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ev.compute_batch()
        wall.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(wall)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    m, d, q, F = 4, 6, 16, 1024
    paths, joint = [], []
    for N in (1024, 4096):
        model, acq = problem(N, m, d)
        for C in (8192, 65536):
            ev = B.CompositePathwiseThompsonBatch(acq, q, n_candidates=C, n_features=F)
            np.random.seed(0)
            ev.compute_batch()
            for p in PHASES:
                phase(model, p)
            batch_ms = timed(ev, a.reps)
            ms = {p: phase(model, p) for p in PHASES}
            calls = a.reps + 1
            Xc = np.random.RandomState(C).uniform(size=(C, d))
            phase(model, "cross")
            model.posterior_mean(Xc)                                 # the cross kernel alone (means only) for the same (N, C, m)
            cross_ms = phase(model, "cross")[0]
            paths.append({"N": N, "C": C, "m": m, "q": q, "F": F, "S": q - 1,
                          "set_paths_ms": round(ms["paths_stage"][0] / calls, 3), "path_values_ms": round(ms["path_values"][0] / calls, 3),
                          "select_ms": round(ms["thompson_select"][0] / calls, 3),
                          "path_utility_ms_per_call": round(ms["path_utility"][0] / max(1, ms["path_utility"][1]), 4),
                          "path_utility_calls_per_batch": round(ms["path_utility"][1] / calls, 1),
                          "compute_batch_ms": batch_ms, "cross_kernel_ms": round(cross_ms, 3)})
        for C in (4096, 8192):
            joint.append({"N": N, "C": C, "m": m, "q": q, "compute_batch_ms": timed(B.CompositeThompsonBatch(acq, q, n_candidates=C), a.reps)})
    print(json.dumps({"paths_latency": paths, "composite_thompson_batch": joint}))


if __name__ == "__main__":
    main()
