"""Wall time of one recommendation step (CBO._current_max_value without the objective: the L argmax problems of cbo.py:121-235)
at N = 1024, d = 6, m = 4 and H = 10 hyper-samples, for L = 1 and L = 5 utility parameters, in the Monte-Carlo and the
closed-form branch: the batched device path (bocf_amd.recommend) against the reference's loops restated on the host over the
same device model (recommend.host_evaluator: per hyper-sample a device posterior query, then Python loops over points and samples).

    python tools/recommend_latency.py [--reps 3] [--host-L 1]

The H = 10 hyper-samples come from one updateModel (optimiser + HMC, a few seconds at N = 1024).  The host loops are slow; by default they are timed for L = 1 only (--host-L 5 adds L = 5).  Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bocf_amd as B                                               # noqa: E402
from bocf_amd import recommend as REC                               # noqa: E402


def model_with_hyper_samples(N, d, m, H, seed=0):
    """A learned-hyper-parameter model through the public surface: updateModel runs the optimiser and HMC (gpmodel.py's defaults)
    and keeps H hyper-samples on the device."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, j % d]) + 0.3 * X.sum(1))[:, None] + 1e-3 * rng.normal(size=(N, 1)) for j in range(m)]
    np.random.seed(seed)
    model = B.multi_outputGP(m, exact_feval=[True] * m, fixed_hyps=False, n_samples=H)
    model.updateModel(X, Y)
    assert model.number_of_hyps_samples() == H
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-L", type=int, default=1)
    a = ap.parse_args()
    N, d, m, H = 1024, 6, 4, 10
    model = model_with_hyper_samples(N, d, m, H)
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    psi = B.ExpectationUtility(lambda t, mu, var: REC.closed_form("neg_sq_dist", t, mu, var)[0],
                               lambda t, mu, var: REC.closed_form("neg_sq_dist", t, mu, var)[1])
    for L in (1, 5):
        support = np.random.RandomState(L).uniform(-1, 1, size=(L, m))
        U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.ones(L) / L), device="neg_sq_dist",
                      dfunc=lambda t, y: -2.0 * (np.asarray(y) - t))
        for branch, eu in (("mc", None), ("closed", psi)):
            times, info = [], {}
            for r in range(a.reps + 1):                             # (the first run warms up)
                np.random.seed(100 + r)
                t0 = time.perf_counter()
                B.current_marginal_argmaxes(model, space, U, support, eu, n_hyps=H, info=info)
                if r:
                    times.append(time.perf_counter() - t0)
            row = dict(L=L, branch=branch, N=N, d=d, m=m, H=H, device_ms=round(1e3 * float(np.median(times)), 2),
                       device_f_df_calls=int(info["f_df_calls"]), host_s=None)
            if L <= a.host_L:
                np.random.seed(100)
                t0 = time.perf_counter()
                B.current_marginal_argmaxes(model, space, U, support, eu, n_hyps=H,
                                            evaluator=lambda p, Z, b=branch, e=eu: REC.host_evaluator(model, b, U, p, e, Z, H))
                row["host_s"] = round(time.perf_counter() - t0, 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
