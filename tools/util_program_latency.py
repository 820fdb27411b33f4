"""What a user's own utility costs on each of its three paths, at BASELINE configs[2]'s shape (N = 1024, d = 6, m = 4, S = 256 common
random numbers, C = 8192 candidates, L = 4 weighted parameters, fixed hyper-parameters): uEI_noiseless._compute_acq on the whole batch
and on 16 points, and _compute_acq_withGradients on 16 points (the L-BFGS refinement's call), for

    builtin   Utility(device="neg_sq_dist")                      the compiled-in kind
    program   Utility(func, device="program")                    the same expression traced and interpreted on the device
    host      Utility(func, dfunc)  (device=None is forced)      the same callable on the warned host fallback

Wall clock of the Python call (median of --reps), plus the device time of the acquisition kernels alone (phase "acq",
bocf_profile_phase) where the utility runs on the device.

    python tools/util_program_latency.py [--reps 7] [--out profiles/util_program/latency.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bocf_amd as B                                               # noqa: E402
from bocf_amd import _ffi                                          # noqa: E402


def neg_sq_dist(t, y):
    return -np.sum(np.square((y.transpose() - t).transpose()), axis=0)


def d_neg_sq_dist(t, y):
    return -2.0 * (y.transpose() - t).transpose()


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
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, d, m, S, C, L = 1024, 6, 4, 256, 8192, 4
    rng = np.random.RandomState(2)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.5, ARD=True) for _ in range(m)], noise_var=[1e-3] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    Xc, W = rng.uniform(size=(C, d)), rng.normal(size=(S, m))
    dist = B.ParameterDistribution(support=rng.normal(size=(L, m)), prob_dist=np.full(L, 1.0 / L))
    utilities = {"builtin": B.Utility(parameter_dist=dist, device="neg_sq_dist"),
                 "program": B.Utility(func=neg_sq_dist, parameter_dist=dist, device="program"),
                 "host": B.Utility(func=neg_sq_dist, dfunc=d_neg_sq_dist, parameter_dist=dist)}
    utilities["host"]._recognise = lambda m: None                  # the closed set would recognise the expression: force the fallback
    out = {"N": N, "d": d, "m": m, "S": S, "C": C, "L": L, "reps": a.reps}
    prog = utilities["program"]._ensure_program(m)
    out["program"] = {"slots": prog.n_slots, "value_instructions": len(prog.val_code), "gradient_instructions": len(prog.grad_code)}
    values = {}
    for name, U in utilities.items():
        acq = B.uEI_noiseless(model, None, utility=U)
        acq.W_samples = W
        r = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for what, f in (("acq_batch", lambda: acq._compute_acq(Xc)), ("acq_16", lambda: acq._compute_acq(Xc[:16])),
                            ("acq_grad_16", lambda: acq._compute_acq_withGradients(Xc[:16]))):
                values[(name, what)] = f()                         # warm-up: code objects, allocations, uploads
                model.set_option("profile", 1)
                phase(model, "acq")
                wall, best = med(f, a.reps)
                dev = phase(model, "acq") / a.reps
                model.set_option("profile", 0)
                r[what] = {"wall_ms": round(wall, 3), "wall_min_ms": round(best, 3)}
                if name != "host":
                    r[what]["acq_kernels_device_ms"] = round(dev, 4)
        out.setdefault("paths", {})[name] = r
    # the three paths compute the same numbers
    for what in ("acq_batch", "acq_16"):
        for name in ("program", "host"):
            np.testing.assert_allclose(values[(name, what)], values[("builtin", what)], rtol=1e-5, atol=1e-9)
    for name in ("program", "host"):
        np.testing.assert_allclose(values[(name, "acq_grad_16")][1], values[("builtin", "acq_grad_16")][1], rtol=1e-4, atol=1e-8)
    p = out["paths"]
    out["ratios"] = {what: {"program_over_builtin_wall": round(p["program"][what]["wall_ms"] / p["builtin"][what]["wall_ms"], 2),
                            "host_over_program_wall": round(p["host"][what]["wall_ms"] / p["program"][what]["wall_ms"], 2),
                            "program_over_builtin_kernels": round(p["program"][what]["acq_kernels_device_ms"] /
                                                                  max(p["builtin"][what]["acq_kernels_device_ms"], 1e-9), 2)}
                     for what in ("acq_batch", "acq_16", "acq_grad_16")}
    line = json.dumps({"util_program_latency": out})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
