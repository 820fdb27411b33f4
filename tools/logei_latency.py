"""Latency of the log-space expected improvement next to the existing forms on the same shape, in the same process (m = 4, d = 6, fixed
hyper-parameters, L = 4 weighted parameters, S = 256 samples, tau = 1e-3) at (N, C) in {(1024, 8192), (4096, 65536)}: bocf_acq_log_linear
alternating with bocf_acq_linear, bocf_acq_log_mc alternating with bocf_acq_mc -- one call over the C candidates (wall clock, values left on
the device, median of --reps; and the acquisition phase alone, device events, bocf_profile_phase "acq": the kernels) and value + gradient on
16 points, f_df(16) (wall clock).

    python tools/logei_latency.py [--reps 7] [--small]

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


def phase(model, name):
    ms, n = ctypes.c_double(), ctypes.c_longlong()
    _ffi.check(_ffi.load().bocf_profile_phase(model._context().handle, name.encode(), ctypes.byref(ms), ctypes.byref(n), 1), "bocf_profile_phase")
    return ms.value


def wall(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def alternate(model, old, new, reps):
    """(old, new) -> medians of the wall clock and of the acquisition phase in ms over reps alternating calls, after one warm-up each."""
    old(), new()
    phase(model, "acq")
    t = {"old": [], "new": []}
    a = {"old": [], "new": []}
    for _ in range(reps):
        for key, f in (("old", old), ("new", new)):
            t[key].append(wall(f))
            a[key].append(phase(model, "acq"))
    return {k: (round(float(np.median(t[k])), 3), round(float(np.median(a[k])), 4)) for k in t}


def case(N, C, reps, m=4, d=6, L=4, S=256, tau=1e-3):
    rng = np.random.RandomState(N + C)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.5, ARD=True) for _ in range(m)], noise_var=[1e-3] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    Xc = rng.uniform(size=(C, d))
    thetas, prob, W = rng.normal(size=(L, m)), np.full(L, 1.0 / L), rng.normal(size=(S, m))
    kind = _ffi.UTIL_NEG_SQ_DIST
    X16 = Xc[:16]
    out = {"N": N, "C": C, "m": m, "d": d, "L": L, "S": S, "tau": tau, "reps": reps}
    model.set_option("profile", 1)
    pairs = {"linear": ((lambda: model.acq_linear(Xc, _ffi.ACQ_EI, thetas, prob), lambda: model.acq_log_linear(Xc, thetas, prob)),
                        (lambda: model.acq_linear_grad(X16, _ffi.ACQ_EI, thetas, prob), lambda: model.acq_log_linear(X16, thetas, prob, grad=True))),
             "mc": ((lambda: model.acq_mc(Xc, _ffi.ACQ_EI, kind, None, thetas, prob, W=W, fetch=False),
                     lambda: model.acq_log_mc(Xc, kind, None, thetas, prob, tau, W=W, fetch=False)),
                    (lambda: model.acq_mc_grad(X16, kind, None, thetas, prob, W=W), lambda: model.acq_log_mc(X16, kind, None, thetas, prob, tau, W=W, grad=True)))}
    for name, (batch, fdf) in pairs.items():
        b, f = alternate(model, batch[0], batch[1], reps), alternate(model, fdf[0], fdf[1], reps)
        out[name] = {"existing": {"wall_ms": b["old"][0], "acq_phase_ms": b["old"][1], "f_df_16_wall_ms": f["old"][0], "f_df_16_acq_phase_ms": f["old"][1]},
                     "log": {"wall_ms": b["new"][0], "acq_phase_ms": b["new"][1], "f_df_16_wall_ms": f["new"][0], "f_df_16_acq_phase_ms": f["new"][1],
                             "wall_ratio": round(b["new"][0] / b["old"][0], 3), "acq_phase_ratio": round(b["new"][1] / b["old"][1], 3),
                             "f_df_16_wall_ratio": round(f["new"][0] / f["old"][0], 3)}}
    model.set_option("profile", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="only (N = 1024, C = 8192)")
    a = ap.parse_args()
    shapes = [(1024, 8192)] if a.small else [(1024, 8192), (4096, 65536)]
    print(json.dumps({"logei_latency": [case(N, C, a.reps) for N, C in shapes]}))


if __name__ == "__main__":
    main()
