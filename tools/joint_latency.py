"""Latency of the joint q-point acquisition (m = 4, d = 6, fixed hyper-parameters, S = 256 normals, L = 4 weighted parameters, q = 8) at
N in {1024, 4096}: bocf_acq_joint's value on 512 batches and value + gradient on 16 batches, each as the wall clock of the synchronised
call (median) and split into its device-event phases (bocf_profile_phase: joint_V, joint_cov, joint_grad, joint_kernel); beside it
bocf_acq_pending's value + gradient on the same 128 points with 7 pending points; a whole CompositeJointBatch.compute_batch(q = 8) with
and without the greedy warm start against CompositeGreedyBatch(q = 8), alternating in one process; and, as a quality figure, the joint
alpha of each evaluator's batch under one common Z.

    python tools/joint_latency.py [--reps 5] [--small] [--batches 2]

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

PHASES = ("joint_V", "joint_cov", "joint_grad", "joint_kernel")


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


def phased(model, f, reps):
    f()                                                             # warm-up: code objects, allocations
    for p in PHASES:
        phase(model, p)
    wall = med(f, reps)
    out = {"wall_ms": round(wall, 3)}
    out.update({p + "_ms": round(phase(model, p) / reps, 3) for p in PHASES})
    return out


def case(N, reps, n_batches, m=4, d=6, L=4, S=256, q=8, r=7):
    rng = np.random.RandomState(N)
    np.random.seed(N)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.5, ARD=True) for _ in range(m)], noise_var=[1e-3] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    thetas, prob = rng.normal(size=(L, m)), np.full(L, 1.0 / L)
    Z, W, Zp = rng.normal(size=(S, m, q)), rng.normal(size=(S, m)), rng.normal(size=(S, m, r))
    Xv, Xg, P = rng.uniform(size=(512, q, d)), rng.uniform(size=(16, q, d)), rng.uniform(size=(r, d))
    kind = _ffi.UTIL_NEG_SQ_DIST
    out = {"N": N, "m": m, "d": d, "q": q, "L": L, "S": S}
    model.set_option("profile", 1)
    out["value_512_batches"] = phased(model, lambda: model.acq_joint(Xv, q, kind, None, thetas, prob, Z), reps)
    out["value_grad_16_batches"] = phased(model, lambda: model.acq_joint(Xg, q, kind, None, thetas, prob, Z, grad=True), reps)
    model.set_option("profile", 0)
    model.set_pending_points(P, Zp, W=W)
    pend = lambda: model.acq_pending(Xg.reshape(-1, d), kind, None, thetas, prob, W=W, grad=True)      # noqa: E731
    pend()
    out["pending_value_grad_128_points_wall_ms"] = round(med(pend, reps), 3)
    # whole batches through the evaluators, alternating
    space = B.Design_space([{"name": "x", "type": "continuous", "domain": (0, 1), "dimensionality": d}])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=thetas, prob_dist=prob), device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer="lbfgs")
    greedy_acq = B.uEI_pending(model, space, optimizer=opt, utility=U)
    joint_acq = B.uEI_joint(model, space, optimizer=opt, utility=U, q=q, n_samples=S)
    evaluators = {"greedy": B.CompositeGreedyBatch(greedy_acq, q), "joint": B.CompositeJointBatch(joint_acq, q),
                  "joint_warm": B.CompositeJointBatch(joint_acq, q, warm_start=B.CompositeGreedyBatch(greedy_acq, q))}
    times, alphas = {k: [] for k in evaluators}, {k: [] for k in evaluators}
    Zq = rng.normal(size=(S, m, q))                                 # the common normals of the quality figure: none of the evaluators saw them
    for _ in range(n_batches):
        for name, ev in evaluators.items():
            t0 = time.perf_counter()
            Xq = ev.compute_batch()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert Xq.shape == (q, d)
            alphas[name].append(float(model.acq_joint(Xq[None], q, kind, None, thetas, prob, Zq)[0]))
    out["compute_batch_q%d" % q] = {k: {"wall_ms": [round(t, 1) for t in times[k]], "joint_alpha_common_Z": [round(a, 6) for a in alphas[k]]}
                                    for k in evaluators}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="only N = 1024")
    ap.add_argument("--batches", type=int, default=2, help="compute_batch rounds per evaluator")
    a = ap.parse_args()
    print(json.dumps({"joint_latency": [case(N, a.reps, a.batches) for N in ([1024] if a.small else [1024, 4096])]}))


if __name__ == "__main__":
    main()
