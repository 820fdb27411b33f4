"""Time the acquisition-optimisation step with the anchor refinement on the host (lbfgsb_batched: one f_df callback per trial step) and
on the device (bocf_refine_acq), uEI and maEI at the README shape, both paths in ONE process, alternating, median
of several; beside each the refinement alone on the anchors of the last step, its passes, points evaluated and host synchronisations,
and a sweep of poll_every.   python tools/refine_latency.py [N] [n_starting] [d] [m] [S] [reps]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bocf_amd as B
from bocf_amd import acquisition_optimizer as AO
from bocf_amd import synthetic as R

POLL_SWEEP = (1, 2, 4, 8, 16, 32, 1000)


def median_ms(ts):
    return 1e3 * float(np.median(ts))


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    C = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    d = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    m = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    S = int(sys.argv[5]) if len(sys.argv) > 5 else 256
    reps = int(sys.argv[6]) if len(sys.argv) > 6 else 7
    p = R.synthetic_problem(N, d, m, 8, S, 1236, noise=1e-4)
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=p["lengthscales"][j], ARD=True) for j in range(m)],
                             noise_var=p["noise"], fixed_hyps=True)
    model.updateModel(p["X"], p["Y"])
    space = AO.Design_space(bounds=[(0.0, 1.0)] * d)
    print("N %d, %d starts, d %d, m %d, S %d, 16 anchors, median of %d (host and device alternating)" % (N, C, d, m, S, reps))
    for name in ("uEI", "maEI"):
        acqs = {}
        for refine in ("host", "device"):
            opt = AO.AcquisitionOptimizer(space, n_starting=C, n_anchor=16, refine=refine)
            if name == "uEI":
                U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5] * m]), prob_dist=np.ones(1)), device="neg_sq_dist")
                acq = B.uEI_noiseless(model, space, optimizer=opt, utility=U)
                acq.W_samples = p["W"]
            else:
                U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.full((1, m), 1.0 / m), prob_dist=np.ones(1)), linear=True)
                acq = B.maEI(model, space, optimizer=opt, utility=U)
            acqs[refine] = acq
        ts, out = {"host": [], "device": []}, {}
        for rep in range(reps + 1):                        # (the first round warms up: allocations)
            for refine in ("host", "device"):
                np.random.seed(3)
                t0 = time.perf_counter()
                out[refine] = acqs[refine].optimize()
                if rep:
                    ts[refine].append(time.perf_counter() - t0)
        for refine in ("host", "device"):
            info = acqs[refine].optimizer.last_info
            print("%-4s optimize() refine=%-6s %7.2f ms   passes %4d, points evaluated %5d, host synchronisations %s, fx_min %.12g"
                  % (name, refine, median_ms(ts[refine]), info["f_df_calls"], info["points_evaluated"], info.get("host_syncs", "one per pass"),
                     float(np.asarray(out[refine][1]).reshape(-1)[0])))
        # the refinement alone, on the anchors of the last step
        anchors = acqs["host"].optimizer.last_info["anchor_points"]
        opt = acqs["host"].optimizer.optimizer
        f_df = acqs["host"].acquisition_function_withGradients
        objective = acqs["device"].device_refine_objective()
        kw = dict(maxiter=opt.maxiter, factr=opt.factr, pgtol=opt.pgtol)
        alone = {"host": []}
        alone.update({q: [] for q in POLL_SWEEP})
        syncs = {}
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            opt.optimize_batch(anchors, f_df)
            if rep:
                alone["host"].append(time.perf_counter() - t0)
            for q in POLL_SWEEP:
                t0 = time.perf_counter()
                _, _, info = model.refine_acq(anchors, opt.bounds, poll_every=q, **dict(objective, **kw))
                if rep:
                    alone[q].append(time.perf_counter() - t0)
                syncs[q] = (info["passes"], info["host_syncs"])
        print("%-4s refinement alone: host loop %.2f ms; device loop by poll_every: %s"
              % (name, median_ms(alone["host"]), ", ".join("%d: %.2f ms (%d passes, %d syncs)" % ((q, median_ms(alone[q])) + syncs[q]) for q in POLL_SWEEP)))
        # above the small path of the predict pass: the anchors and two x_baseline rows (A = 18) -- the device loop then predicts twice
        # per pass (the whole batch, and the first 16 running rows gathered)
        X18 = np.vstack([anchors, 0.25 + 0.5 * anchors[:2]])
        t18 = {"host": [], "device": []}
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            opt.optimize_batch(X18, f_df, info=(hinfo := {}))
            t1 = time.perf_counter()
            _, _, dinfo = model.refine_acq(X18, opt.bounds, **dict(objective, **kw))
            t2 = time.perf_counter()
            if rep:
                t18["host"].append(t1 - t0)
                t18["device"].append(t2 - t1)
        print("%-4s refinement alone, A = 18: host loop %.2f ms (%d callbacks); device loop %.2f ms (%d passes, %.3f ms per pass against %.3f at A = 16)"
              % (name, median_ms(t18["host"]), hinfo["f_df_calls"], median_ms(t18["device"]), dinfo["passes"], median_ms(t18["device"]) / dinfo["passes"],
                 median_ms(alone[8]) / syncs[8][0]))


if __name__ == "__main__":
    main()
