"""Phases of the pending-point acquisition (m = 4, d = 6, fixed hyper-parameters, S = 256 samples, r = 7 pending points, L = 4 weighted
parameters) at (N, C) in {(1024, 8192), (4096, 65536)}: staging the pending points (bocf_set_pending_points, wall clock and its kg_ref
phase), one alpha(. | P) call split into V = R^T K(X, x) (kg_V), the covariances Sigma(x, P) with the raw variances (kg_cov) and the
threshold + value kernels (pending_kernel) -- device events, bocf_profile_phase --, value + gradient on 16 points (wall clock), a whole
q = 8 CompositeGreedyBatch.compute_batch (wall clock, the optimiser's defaults), and for scale the uEI step of the same process at the same
shape (wall clock of one acq_mc call + top-16).

    python tools/pending_latency.py [--reps 5] [--small]

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

PHASES = ("kg_ref", "kg_V", "kg_cov", "pending_kernel", "kg_grad")


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


def case(N, C, reps, m=4, d=6, r=7, L=4, S=256, q=8):
    rng = np.random.RandomState(N + C)
    np.random.seed(N + C)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.5, ARD=True) for _ in range(m)], noise_var=[1e-3] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    Xc, P = rng.uniform(size=(C, d)), rng.uniform(size=(r, d))
    thetas, prob = rng.normal(size=(L, m)), np.full(L, 1.0 / L)
    Zp, W = rng.normal(size=(S, m, r)), rng.normal(size=(S, m))
    out = {"N": N, "C": C, "m": m, "d": d, "r": r, "L": L, "S": S}
    model.set_option("profile", 1)
    kind = _ffi.UTIL_NEG_SQ_DIST

    def stage(k=[0]):
        k[0] += 1
        model.set_pending_points(P, Zp + 1e-9 * k[0], W=W)         # (another key every time: the device call is made)
    stage()                                                         # warm-up: code objects, allocations
    phase(model, "kg_ref")
    out["set_pending_points_wall_ms"] = round(med(stage, reps), 3)
    out["set_pending_points_device_ms"] = round(phase(model, "kg_ref") / reps, 3)
    run = lambda: model.acq_pending(Xc, kind, None, thetas, prob, W=W, fetch=False)            # noqa: E731
    run()
    for p in PHASES:
        phase(model, p)
    wall = med(run, reps)
    ms = {p: phase(model, p) / reps for p in PHASES}
    total = ms["kg_V"] + ms["kg_cov"] + ms["pending_kernel"]
    out["value"] = {"wall_ms": round(wall, 3), "V_ms": round(ms["kg_V"], 3), "cov_ms": round(ms["kg_cov"], 3),
                    "pending_kernel_ms": round(ms["pending_kernel"], 3), "pending_kernel_share": round(ms["pending_kernel"] / total, 3)}
    X16 = Xc[:16]
    fdf = lambda: model.acq_pending(X16, kind, None, thetas, prob, W=W, grad=True)             # noqa: E731
    fdf()
    out["f_df_16_wall_ms"] = round(med(fdf, max(reps, 5)), 3)
    model.set_option("profile", 0)

    def uei():
        model.acq_mc(Xc, _ffi.ACQ_EI, kind, None, thetas, prob, W=W, fetch=False)
        model.select_topk(16)
    uei()
    out["uEI_step_wall_ms"] = round(med(uei, reps), 3)
    # a whole greedy batch through the acquisition optimiser
    space = B.Design_space([{"name": "x", "type": "continuous", "domain": (0, 1), "dimensionality": d}])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=thetas, prob_dist=prob), device="neg_sq_dist")
    acq = B.uEI_pending(model, space, optimizer=B.AcquisitionOptimizer(space, optimizer="lbfgs"), utility=U)
    acq.W_samples = W
    batch = B.CompositeGreedyBatch(acq, q)
    t0 = time.perf_counter()
    Xq = batch.compute_batch()
    out["compute_batch_q%d_wall_ms" % q] = round((time.perf_counter() - t0) * 1e3, 1)
    assert Xq.shape == (q, d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="only (N = 1024, C = 8192)")
    a = ap.parse_args()
    shapes = [(1024, 8192)] if a.small else [(1024, 8192), (4096, 65536)]
    print(json.dumps({"pending_latency": [case(N, C, a.reps) for N, C in shapes]}))


if __name__ == "__main__":
    main()
