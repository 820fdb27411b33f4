"""Phases of the discrete composite knowledge gradient (m = 4, d = 6, fixed hyper-parameters, na = 128 reference points, Sf = 32 fantasies,
L = 4 weighted parameters): staging the reference set (bocf_set_ref_points), the value form at (N, C) in {(1024, 8192), (4096, 65536)}
in its three modes split into V = R^T K(X, x) (kg_V), the covariances Sigma(x, A) with the raw variances (kg_cov) and the value kernel
(kg_kernel) -- device events, bocf_profile_phase -- the gradient form f_df on 16 points (wall clock), and for scale the uEI step of the
same process at the same shape (wall clock of one acq_mc call + top-16).

    python tools/kg_latency.py [--reps 5] [--small]

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

PHASES = ("kg_ref", "kg_V", "kg_cov", "kg_kernel", "kg_grad")
MODES = (("mean", _ffi.UTIL_LINEAR), ("closed", _ffi.UTIL_NEG_SQ_DIST), ("mc", _ffi.UTIL_NEG_SQ_DIST))


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


def case(N, C, reps, m=4, d=6, na=128, Sf=32, L=4, S=25):
    rng = np.random.RandomState(N + C)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.5, ARD=True) for _ in range(m)], noise_var=[1e-3] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    Xc, A = rng.uniform(size=(C, d)), rng.uniform(size=(na, d))
    thetas, prob = rng.normal(size=(L, m)), np.full(L, 1.0 / L)
    Zf, W = rng.normal(size=(Sf, m)), rng.normal(size=(S, m))
    lib, h = _ffi.load(), model._context().handle
    out = {"N": N, "C": C, "m": m, "d": d, "na": na, "Sf": Sf, "L": L, "S": S}
    model.set_option("profile", 1)
    Ad = _ffi.f64(A)
    _ffi.check(lib.bocf_set_ref_points(h, _ffi.dptr(Ad), na), "bocf_set_ref_points")          # warm-up: code objects, allocations
    phase(model, "kg_ref")
    out["set_ref_points_wall_ms"] = round(med(lambda: _ffi.check(lib.bocf_set_ref_points(h, _ffi.dptr(Ad), na), "bocf_set_ref_points"), reps), 3)
    out["set_ref_points_device_ms"] = round(phase(model, "kg_ref") / reps, 3)
    model.set_reference_points(A)
    for mode, kind in MODES:
        run = lambda: model.acq_kg(Xc, mode, kind, None, thetas, prob, Zf, W=W, fetch=False)   # noqa: E731
        run()
        for p in PHASES:
            phase(model, p)
        wall = med(run, reps)
        ms = {p: phase(model, p) / reps for p in PHASES}
        total = ms["kg_V"] + ms["kg_cov"] + ms["kg_kernel"]
        out[mode] = {"wall_ms": round(wall, 3), "V_ms": round(ms["kg_V"], 3), "cov_ms": round(ms["kg_cov"], 3), "kg_kernel_ms": round(ms["kg_kernel"], 3),
                     "kg_kernel_share": round(ms["kg_kernel"] / total, 3)}
    X16 = Xc[:16]
    for mode, kind in MODES:
        run = lambda: model.acq_kg(X16, mode, kind, None, thetas, prob, Zf, W=W, grad=True)    # noqa: E731
        run()
        out[mode]["f_df_16_wall_ms"] = round(med(run, max(reps, 5)), 3)
    model.set_option("profile", 0)

    def uei():
        model.acq_mc(Xc, _ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, thetas, prob, W=W, fetch=False)
        model.select_topk(16)
    uei()
    out["uEI_step_wall_ms"] = round(med(uei, reps), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="only (N = 1024, C = 8192)")
    a = ap.parse_args()
    shapes = [(1024, 8192)] if a.small else [(1024, 8192), (4096, 65536)]
    print(json.dumps({"kg_latency": [case(N, C, a.reps) for N, C in shapes]}))


if __name__ == "__main__":
    main()
