"""Latency of the feasibility-aware recommendation step against the unconstrained one, in one process, at
N = 1024, d = 6, m = 4, H = 10 resident hyper-samples, L in {1, 5} utility parameters and K in {1, 8} constraints:

  * bocf_expected_utility in its Monte-Carlo mode and bocf_expected_utility_constrained on the same rows -- the L x 24 anchors with
    gradients (one L-BFGS step) and the L x 200 starts value-only: the kernels' phase ("eu" / "ceu", device events, bocf_profile_phase) and
    the whole call (wall clock);
  * the whole recommendation step (current_marginal_argmaxes) with and without constraints (wall clock).

    python tools/constrained_recommend_latency.py [--reps 5] [--out profiles/ceu/latency.json]

The two ratios of section 17's report: the kernel phase and the whole call, constrained over unconstrained.  Prints one JSON line."""
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


def timed(model, name, call, reps):
    """(median wall ms, median phase ms) of `call` after one warm-up."""
    call()
    phase_ms(model, name)
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(phase_ms(model, name))
    return float(np.median(wall)), float(np.median(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, d, m, H, S = 1024, 6, 4, 10, 50
    model = model_with_hyper_samples(N, d, m, H)
    model.set_option("profile", 1)
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    mt = model.posterior_mean_at_evaluated_points()
    rows_out = []
    for L in (1, 5):
        rng = np.random.RandomState(L)
        support = rng.uniform(-1, 1, size=(L, m))
        U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.ones(L) / L), device="neg_sq_dist",
                      dfunc=lambda t, y: -2.0 * (np.asarray(y) - t))
        Z = rng.normal(size=(L, S, m))
        batches = {"anchors_grad": (rng.uniform(size=(L * 24, d)), np.repeat(np.arange(L), 24), True),
                   "starts_value": (rng.uniform(size=(L * 200, d)), np.repeat(np.arange(L), 200), False)}
        row = dict(N=N, d=d, m=m, H=H, L=L, S=S)
        for bname, (X, rows, grad) in batches.items():
            w, p = timed(model, "eu", lambda: model.expected_utility(X, "mc", "neg_sq_dist", support, rows, Z=Z, n_hyps=H, grad=grad), a.reps)
            row[bname] = {"expected_utility": {"wall_ms": round(w, 4), "phase_ms": round(p, 4)}}
        times, info = [], {}
        for r in range(a.reps + 1):
            np.random.seed(100 + r)
            t0 = time.perf_counter()
            B.current_marginal_argmaxes(model, space, U, support, None, n_hyps=H, info=info)
            if r:
                times.append(1e3 * (time.perf_counter() - t0))
        row["step"] = {"unconstrained_ms": round(float(np.median(times)), 2), "unconstrained_f_df_calls": int(info["f_df_calls"])}
        for K in (1, 8):
            A = np.random.RandomState(10 + K).normal(size=(K, m))
            oc = B.OutputConstraints(A, [np.quantile(A[k].dot(mt), 0.5 ** (1.0 / K)) for k in range(K)], eta=1e-3)
            model.set_output_constraints(oc)
            u0 = model.train_utility_range("neg_sq_dist", None, support)[0]
            for bname, (X, rows, grad) in batches.items():
                w, p = timed(model, "ceu", lambda: model.expected_utility_constrained(X, "neg_sq_dist", support, rows, u0, Z, n_hyps=H, grad=grad), a.reps)
                base = row[bname]["expected_utility"]
                row[bname]["K%d" % K] = {"wall_ms": round(w, 4), "phase_ms": round(p, 4), "phase_ratio": round(p / base["phase_ms"], 3),
                                         "wall_ratio": round(w / base["wall_ms"], 3)}
            times, info = [], {}
            for r in range(a.reps + 1):
                np.random.seed(100 + r)
                t0 = time.perf_counter()
                B.current_marginal_argmaxes(model, space, U, support, None, n_hyps=H, constraints=oc, info=info)
                if r:
                    times.append(1e3 * (time.perf_counter() - t0))
            t = float(np.median(times))
            per_call = (t / info["f_df_calls"]) / (row["step"]["unconstrained_ms"] / row["step"]["unconstrained_f_df_calls"])
            row["step"]["K%d" % K] = {"ms": round(t, 2), "ratio": round(t / row["step"]["unconstrained_ms"], 3), "f_df_calls": int(info["f_df_calls"]),
                                      "ratio_per_f_df_call": round(per_call, 3),
                                      "pof_min": round(float(np.min(info["pof"])), 4)}
        rows_out.append(row)
    out = {"constrained_recommend_latency": rows_out}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
