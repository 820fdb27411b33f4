"""Every covariance path at extreme hyper-parameters and input scales, against the long-double truth of tests/extremes_ref.py: lengthscales
1e-3 ... 300, kernel variances 1e-6 ... 1e6, noise 1e-10 ... 100, inputs scaled by 1e+-3 and offset by up to 1e6, one ARD kernel with
lengthscales (0.01, 0.5, 100), and a d = 1 ramp whose exponentials run through the subnormal band into zero (bocf_exp_nonpos).  N = 100
(one panel, the fused infer128_kernel for _infer) and N = 130 (two panels, the team schedule, the replicated fit and hypgrad_kernel),
d = 3, 40 candidates (tile path) and the first 8 of them (cross_small_kernel); three outputs per model, each in a different regime, so that
the per-output KernHyp indexing carries unlike magnitudes side by side.

Gates: extremes_ref.floors (the project's tolerances in the unit of the case) or 4 x the fp64 oracle's own error against the truth,
whichever is larger; no oracle term where the inputs carry an offset.  tests/test_extremes_cpu.py shows that the oracle meets these floors
with a decade of room and that the perturbations this file is meant to catch leave them.  Every figure is printed before its assertion:
run with -s.

Measured on the MI355X (-s output; 63 tests in 9.3 s, none above 0.4 s).  Largest error as a fraction of its gate, per regime family, over
both N, all families and both candidate counts ("var" covers predict, the noiseless variance and the small path; dv / dl / dn both routes):
  regime       K rbf  K se  K m52  K m32  alpha    lml      mean     mu_train var      dmean    dvar     dv       dl       dn
  lengthscale  0.50   0.50  0.49   0.50   0.061    0.0039   1.6e-4   1.9e-4   4.9e-6   6.7e-5   1.0e-6   6.1e-6   7.6e-4   7.9e-6
  variance     0.18   -     0.15   0.15   0.011    6.6e-4   2.6e-5   6.0e-6   1.6e-5   8.5e-6   2.9e-7   1.9e-6   1.2e-6   1.7e-6
  noise        0.16   -     0.15   0.14   0.015    0.38     0.012    0.0011   0.0059   0.015    1.7e-4   1.3e-5   2.0e-4   0.0096
  input scale  0.16   -     0.16   0.15   0.0032   9.4e-4   1.6e-5   3.8e-6   1.7e-5   5.0e-6   2.1e-7   2.2e-6   2.0e-6   2.3e-6
  offset       0.11   -     0.14   0.14   0.015    8.5e-4   1.5e-5   4.0e-6   1.0e-5   4.5e-6   2.5e-7   3.2e-6   1.4e-6   2.2e-6
  mixed ARD    0.49   -     0.23   0.26   7.6e-7   1.1e-5   1.0e-7   4.9e-8   5.1e-7   2.9e-8   2.9e-9   2.4e-7   1.0e-7   1.3e-7
  ramp         0.45   0.45  0.32   0.49   1.7e-4   2.6e-5
(noise: the 0.38 is the log-marginal at noise 1e-10, rbf, cond(Ky) 6e9, where 4 x the oracle's own error is the gate; offsets 1e3 and 1e6
have no oracle term and stay at 1.5e-5 of the floor on the mean.)  The device's jitter ladder added nothing in any case.
Before bocf_exp_nonpos_times (kern_family.h) the K ratio was 9.1e4 (Matern52) and 367 (Matern32) at l = 1e-3, and the same on the ramp:
the amplitude multiplied an exponential that had already been rounded into the subnormal range.  Everything else was as above.
Ramp: 174 (rbf, se) / 412 (Matern) entries in the subnormal band, all non-zero on the device; 756 / 2256 / 2352 truly zero; 42 / 132
beyond the -1100 clamp.  Rescaling by 2^10 and 2^-10: no entry of any compared array differs, N = 100 and 130.
Reduced precision, max |var - var_fp64| / sigma_f^2 per family (rbf, Matern52, Matern32), N = 130, C = 300 -- asserted cases:
  predict_f32 (gate 2e-5): l=0.5, s=1e-3, s=1e3 0.35 of the gate; var=1e6 0.37; var=1e-6 0.081
  predict_i8  (gate 1e-9): l=0.5 7.7e-12 3.4e-12 1.3e-12; var=1e-6 1.2e-12 7.4e-13 5.6e-13; var=1e6 4.4e-12 1.7e-12 5.7e-13;
                           s=1e-3 6.4e-12 3.4e-12 1.3e-12; s=1e3 6.0e-12 3.1e-12 1.3e-12
recorded only (predict_f32; predict_i8):
  l=0.02 5.6e-09 1.3e-08 8.4e-09; 2.7e-15 5.3e-15 9.9e-15       l=0.1 2.4e-07 1.5e-07 1.7e-07; 3.0e-13 1.8e-13 1.9e-13
  l=3 2.3e-06 3.2e-06 5.9e-06; 1.5e-12 1.8e-12 2.5e-12          l=30 8.8e-07 7.1e-07 1.1e-06; 4.0e-13 4.8e-13 5.4e-13
  l=300 3.7e-07 3.5e-07 3.5e-07; 1.6e-13 1.4e-13 2.2e-13        var=1e-3 7.2e-06 2.8e-06 1.3e-06; 6.1e-12 2.4e-12 1.4e-12
  var=1e3 7.2e-06 2.5e-06 2.7e-06; 5.0e-12 1.5e-12 8.4e-13      noise=1e-10 1.1e-04 4.7e-06 1.4e-06; 5.6e-10 3.8e-12 1.5e-12
  noise=1e-8 8.6e-05 2.7e-06 1.2e-06; 1.5e-10 3.8e-12 1.0e-12   noise=0.01 2.2e-06 1.4e-06 9.4e-07; 1.6e-12 8.0e-13 6.0e-13
  noise=1 2.9e-07 2.7e-07 2.5e-07; 1.5e-13 1.8e-13 1.7e-13      noise=100 2.6e-08 1.9e-08 2.2e-08; 2.8e-14 2.8e-14 2.8e-14
  o=1e3 7.0e-06 3.7e-06 1.1e-06; 6.9e-12 3.6e-12 1.2e-12        o=1e6 7.3e-06 3.3e-06 1.2e-06; 1.1e-11 2.9e-12 1.5e-12
  s=1e3,o=-500 7.0e-06 3.7e-06 1.1e-06; 6.5e-12 3.2e-12 1.3e-12 ard 1.1e-06 3.2e-07 2.9e-07; 1.0e-12 3.0e-13 2.1e-13
  (l=1e-3: K = sigma_f^2 I, both 0.  predict_f32 at noise <= 1e-8 with rbf, cond 6e9, is 4 ... 5 x its gate of the benign regime.)
Clip case (sigma_f^2 = 1e-12, noise 0): every variance exactly 1e-10 on the fp64, fp32 and int8 paths, 300 and 8 candidates.
Run on the MI355X box: python -m pytest tests/test_gpu_extremes.py -m gpu -s"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extremes_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu

LD = E.LD
D = E.D
SIZES = [100, 130]
QUANTITIES = ("mean", "mu_train", "raw_var", "lml", "alpha", "dmean", "dvar", "dv", "dl", "dn")
STATS = {}                                              # (group, what) -> largest error / gate seen, printed by the last test


@pytest.fixture(scope="module")
def B():
    if not E.have_x87():
        pytest.skip("numpy.longdouble is not the x87 extended format here (eps %g): NO TRUTH, NOTHING CHECKED" % np.finfo(LD).eps)
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


# ------------------------------------------------------------------------------------------------------------------------
# the models: [(kind, case, target slot)] x 3
# ------------------------------------------------------------------------------------------------------------------------
def _specs():
    n = len(E.SAME_X)
    out = [[("rbf", E.SAME_X[k], 0), ("matern52", E.SAME_X[(k + 6) % n], 1), ("matern32", E.SAME_X[(k + 11) % n], 2)] for k in range(n)]
    out += [[(kind, c, s) for s, kind in enumerate(E.FAMILIES)] for c in E.INPUT]
    out += [[("se", E.SE_CASES[i], 3) for i in tr] for tr in ((0, 3, 6), (1, 4, 6), (2, 5, 0))]
    return out


SPECS = _specs()


def _spec_id(spec):
    return "|".join("%s:%s" % (k, c.name) for k, c, _ in spec)


def _kernels(B, spec):
    cls = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
    return [cls[k](len(c.ls), variance=c.variance, lengthscale=c.ls, ARD=True) for k, c, _ in spec]


def _fixed_model(B, spec, X, Y):
    model = B.multi_outputGP(len(spec), kernel=_kernels(B, spec), noise_var=[c.noise for _, c, _ in spec], fixed_hyps=True)
    model.updateModel(X, Y)
    return model


def _infer(B, spec, X, Y):
    """(lml, dv, dl, dn) of model._infer at the hyper-parameters of the spec: the fused launch at N <= 128, the replicated path beyond."""
    learner = B.multi_outputGP(len(spec), kernel=_kernels(B, spec), noise_var=[None] * len(spec), fixed_hyps=False, n_samples=2)
    learner._X, learner._Y = X, Y
    learner._create_sampler_state()
    return learner._infer([(c.variance, c.ls, c.noise) for _, c, _ in spec])


def _data(spec, N, C=E.C_TILE):
    X, Xc = E.inputs(spec[0][1], N, C)
    return np.ascontiguousarray(X), np.ascontiguousarray(Xc), [E.targets(c, N, s)[:, None] for _, c, s in spec]


def _note(group, what, frac):
    STATS[(group, what)] = max(STATS.get((group, what), 0.0), frac)


def _check(tag, group, what, got, want, tol, e_orc):
    frac = E.fraction(got, want, tol[0], tol[1], e_orc)
    print("%s %-24s max |delta| %.3g, of its gate %.3g (oracle's error %.3g)" % (tag, what, E.error(got, want), frac, e_orc))
    _note(group, what.split(",")[0], frac)
    return [] if frac <= 1.0 else ["%s: %.3g of its gate" % (what, frac)]


def _check_k(tag, group, kind, Kd, t, variance, d):
    """get_train_kernel entry by entry: extremes_ref.k_entry_bound."""
    err = np.abs(Kd.astype(LD) - t["K"])
    ratio = float(np.max(err / E.k_entry_bound(t, variance, d)))
    print("%s %-24s largest |delta| / bound %.3g (largest u %.4g)" % (tag, "train kernel, %s" % kind, ratio, float(t["u"].max())))
    _note(group, "K " + kind, ratio)
    return [] if ratio <= 1.0 else ["train kernel: %.3g of its bound" % ratio]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("spec", SPECS, ids=_spec_id)
def test_regimes_against_the_truth(B, spec, N):
    X, Xc, Y = _data(spec, N)
    model = _fixed_model(B, spec, X, Y)
    mean, var = model.predict(Xc)
    nvar = model.posterior_variance_noiseless(Xc)
    mean_s, var_s = model.predict(Xc[:E.C_SMALL])
    nvar_s = model.posterior_variance_noiseless(Xc[:E.C_SMALL])
    mu = model.posterior_mean_at_evaluated_points()
    dm, dvx = model.posterior_mean_gradient(Xc), model.posterior_variance_gradient(Xc)
    dm_s, dvx_s = model.posterior_mean_gradient(Xc[:E.C_SMALL]), model.posterior_variance_gradient(Xc[:E.C_SMALL])
    lml = model.log_likelihood()
    gv, gl, gn = model.log_likelihood_gradients()
    ilml, iv, il, inz = _infer(B, spec, X, Y)
    bad = []
    for j, (kind, c, slot) in enumerate(spec):
        tag = "N %d %-9s %-18s" % (N, kind, c.name)
        jit = float(model.jitter[j])
        if jit == 0.0:
            t, eo = E.case_truth(kind, c.name, N, slot), E.oracle_errors(kind, c.name, N, slot)
        else:                                               # the device's ladder added jitter: the truth is the truth of that Ky
            print("%s device jitter %g" % (tag, jit))
            t = E.truth(kind, X, Y[j], c.variance, c.ls, c.noise, Xc, jitter=jit)
            eo = dict.fromkeys(QUANTITIES, 0.0)
        fl = E.floors(t, c.variance, c.ls, N)
        g, s = c.group, E.C_SMALL
        tvar, tnvar = np.clip(t["raw_var"] + LD(c.noise), 1e-10, None), np.clip(t["raw_var"], 1e-10, None)
        out = _check_k(tag, g, kind, model.get_train_kernel(j), t, c.variance, D)
        out += _check(tag, g, "alpha", model.get_factor(j)[1], t["alpha"], fl["alpha"], eo["alpha"])
        out += _check(tag, g, "lml", lml[j], t["lml"], fl["lml"], eo["lml"])
        out += _check(tag, g, "lml, _infer", ilml[j], t["lml"], fl["lml"], eo["lml"])
        out += _check(tag, g, "mean", mean[j], t["mean"], fl["mean"], eo["mean"])
        out += _check(tag, g, "mean, small path", mean_s[j], t["mean"][:s], fl["mean"], eo["mean"])
        out += _check(tag, g, "mu_train", mu[j], t["mu_train"], fl["mu_train"], eo["mu_train"])
        out += _check(tag, g, "var", var[j], tvar, fl["raw_var"], eo["raw_var"])
        out += _check(tag, g, "var, noiseless", nvar[j], tnvar, fl["raw_var"], eo["raw_var"])
        out += _check(tag, g, "var, small path", var_s[j], tvar[:s], fl["raw_var"], eo["raw_var"])
        out += _check(tag, g, "var, noiseless small", nvar_s[j], tnvar[:s], fl["raw_var"], eo["raw_var"])
        out += _check(tag, g, "dmean", dm[j], t["dmean"], fl["dmean"], eo["dmean"])
        out += _check(tag, g, "dmean, small path", dm_s[j], t["dmean"][:s], fl["dmean"], eo["dmean"])
        out += _check(tag, g, "dvar", dvx[j], t["dvar"], fl["dvar"], eo["dvar"])
        out += _check(tag, g, "dvar, small path", dvx_s[j], t["dvar"][:s], fl["dvar"], eo["dvar"])
        for route, (a, b, cc) in (("fit", (gv, gl, gn)), ("_infer", (iv, il, inz))):
            out += _check(tag, g, "dv, %s" % route, a[j], t["dv"], fl["dv"], eo["dv"])
            out += _check(tag, g, "dl, %s" % route, b[j], t["dl"], fl["dl"], eo["dl"])
            out += _check(tag, g, "dn, %s" % route, cc[j], t["dn"], fl["dn"], eo["dn"])
        bad += ["%s %s" % (tag, o) for o in out]
    assert not bad, "\n".join(bad)


def test_ramp_train_kernel_through_the_subnormal_band(B):
    """d = 1, N = 128, X = linspace(0, 1): u = r2/2, sqrt5 r, sqrt3 r runs from 0 to 1200 over the pairs -- the normal range, the subnormal
    band (u in [708.4, 745.1]), true zero and the -1100 clamp of bocf_exp_nonpos.  Entry by entry within extremes_ref.k_entry_bound; exact
    0 wherever the truth is below 2^-1075 sigma_f^2; symmetric bit for bit; no NaN, no negative entry."""
    kinds = ["rbf", "se", "matern52", "matern32"]
    X = E.ramp_inputs()
    Y = [E.ramp_targets(s)[:, None] for s in range(len(kinds))]
    cls = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
    kern = [cls[k](1, variance=1.0, lengthscale=[E.RAMP_LS[k]], ARD=True) for k in kinds]
    model = B.multi_outputGP(len(kinds), kernel=kern, noise_var=[1e-4] * len(kinds), fixed_hyps=True)
    model.updateModel(X, Y)
    bad = []
    for j, kind in enumerate(kinds):
        t = E.truth(kind, X, Y[j], 1.0, [E.RAMP_LS[kind]], 1e-4, X[:1])
        Kd = model.get_train_kernel(j)
        u = t["u"].astype(float)
        band, gone = (u > 708.4) & (u < 745.14), t["K"] < LD(2) ** -1075
        print("ramp %-9s u up to %.4g: %d entries in the subnormal band (%d of them non-zero on the device), %d truly zero, %d beyond the clamp"
              % (kind, u.max(), band.sum(), np.count_nonzero(Kd[band]), gone.sum(), (u > 1100).sum()))
        assert band.sum() >= 100 and gone.sum() >= 500 and (u > 1100).sum() >= 10       # (the ramp reaches all four ranges)
        bad += _check_k("ramp", "ramp", kind, Kd, t, 1.0, 1)
        assert np.all(np.isfinite(Kd)) and np.all(Kd >= 0.0), kind
        np.testing.assert_array_equal(Kd, Kd.T)
        np.testing.assert_array_equal(Kd[gone], 0.0)
        fl = E.floors(t, 1.0, [E.RAMP_LS[kind]], E.RAMP_N)
        bad += _check("ramp %-9s" % kind, "ramp", "alpha", model.get_factor(j)[1], t["alpha"], fl["alpha"], 0.0)
        bad += _check("ramp %-9s" % kind, "ramp", "lml", model.log_likelihood()[j], t["lml"], fl["lml"], 0.0)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("k", [10, -10])
@pytest.mark.parametrize("N", SIZES)
def test_power_of_two_rescaling_is_exact(B, N, k):
    """X, Xc and every lengthscale times 2^k: no quotient x / l changes, so nothing that depends on them alone may change by one bit, and
    what carries a power of l (dl, both input gradients) changes by exactly 2^-k."""
    f = 2.0 ** k
    base = [(kind, E.BASE, s) for s, kind in enumerate(E.FAMILIES)]
    scaled = [(kind, E.BASE._replace(ls=E.BASE.ls * f, scale=f), s) for kind, _, s in base]
    res = []
    for spec in (base, scaled):
        X, Xc, Y = _data(spec, N)
        model = _fixed_model(B, spec, X, Y)
        r = dict(lml=model.log_likelihood(), pred=model.predict(Xc), small=model.predict(Xc[:E.C_SMALL]),
                 nvar=model.posterior_variance_noiseless(Xc), mu=model.posterior_mean_at_evaluated_points(),
                 K=[model.get_train_kernel(j) for j in range(3)], fac=[model.get_factor(j) for j in range(3)],
                 dm=model.posterior_mean_gradient(Xc), dvx=model.posterior_variance_gradient(Xc),
                 dm_s=model.posterior_mean_gradient(Xc[:E.C_SMALL]), dvx_s=model.posterior_variance_gradient(Xc[:E.C_SMALL]),
                 hyp=model.log_likelihood_gradients(), inf=_infer(B, spec, X, Y))
        res.append(r)
    a, b = res
    same = [("lml", a["lml"], b["lml"]), ("mean", a["pred"][0], b["pred"][0]), ("var", a["pred"][1], b["pred"][1]),
            ("small mean", a["small"][0], b["small"][0]), ("small var", a["small"][1], b["small"][1]), ("noiseless var", a["nvar"], b["nvar"]),
            ("mu_train", a["mu"], b["mu"]), ("dv", a["hyp"][0], b["hyp"][0]), ("dn", a["hyp"][2], b["hyp"][2]),
            ("_infer lml", a["inf"][0], b["inf"][0]), ("_infer dv", a["inf"][1], b["inf"][1]), ("_infer dn", a["inf"][3], b["inf"][3]),
            ("dl x 2^k", a["hyp"][1], b["hyp"][1] * f), ("_infer dl x 2^k", a["inf"][2], b["inf"][2] * f),
            ("dmean x 2^k", a["dm"], b["dm"] * f), ("dvar x 2^k", a["dvx"], b["dvx"] * f),
            ("small dmean x 2^k", a["dm_s"], b["dm_s"] * f), ("small dvar x 2^k", a["dvx_s"], b["dvx_s"] * f)]
    for j in range(3):
        same += [("K %d" % j, a["K"][j], b["K"][j]), ("L %d" % j, a["fac"][j][0], b["fac"][j][0]), ("alpha %d" % j, a["fac"][j][1], b["fac"][j][1])]
    diff = {name: int(np.sum(np.asarray(x) != np.asarray(y))) for name, x, y in same}
    print("N %d, 2^%d: entries that differ: %s" % (N, k, {n: c for n, c in diff.items() if c} or "none"))
    for name, x, y in same:
        np.testing.assert_array_equal(x, y, err_msg="N = %d, 2^%d: %s" % (N, k, name))


REDUCED = (("predict_f32", 2e-5), ("predict_i8", 1e-9))
RESCALED = ("l=0.5", "var=1e-06", "var=1e+06", "s=0.001,o=0", "s=1000,o=0")        # the base case and its exact rescalings


def _reduced(B, case):
    """{option: max |var_option - var_fp64| / sigma_f^2 per output} of the three families at one case, N = 130, C = 300."""
    spec = [(kind, case, s) for s, kind in enumerate(E.FAMILIES)]
    X, Xc, Y = _data(spec, E.N_MAX, E.C_REDUCED)
    model = _fixed_model(B, spec, X, Y)
    mean, var = model.predict(Xc)
    out = {}
    for option, _ in REDUCED:
        model.set_option(option, 1)
        try:
            mean_o, var_o = model.predict(Xc)
        finally:
            model.set_option(option, 0)
        np.testing.assert_array_equal(mean_o, mean)
        assert np.all(var_o >= 1e-10)
        out[option] = np.abs(var_o - var).max(axis=1) / case.variance
    return out


@pytest.mark.parametrize("name", RESCALED)
def test_reduced_precision_variance_of_rescaled_cases(B, name):
    """Options predict_f32 and predict_i8 against the same model's fp64 variance, N = 130, C = 300: 2e-5 sigma_f^2
    (test_reduced_precision_copies_follow_an_append) and 1e-9 sigma_f^2 (test_int8_variance_contraction_against_fp64) -- in the base case
    and in its rescalings, where a failure is a scaling bug and no precision limit."""
    got = _reduced(B, E.BY_NAME[name])
    for option, gate in REDUCED:
        print("%-18s %-11s max |delta var| / sigma_f^2 per family %s (gate %g)" % (name, option, " ".join("%.3g" % v for v in got[option]), gate))
        _note("reduced " + option, name, float(got[option].max() / gate))
    for option, gate in REDUCED:
        assert got[option].max() <= gate, (name, option, got[option])


def test_reduced_precision_variance_elsewhere_is_recorded(B):
    """The other regimes: printed, nothing asserted beyond finite, clipped variances -- the record for later work on those paths."""
    for c in E.CASES:
        if c.name in RESCALED:
            continue
        got = _reduced(B, c)
        print("%-18s %s" % (c.name, "; ".join("%s %s" % (o, " ".join("%.3g" % v for v in got[o])) for o, _ in REDUCED)))


def test_variance_below_the_clip(B):
    """sigma_f^2 = 1e-12, noise 0: every predicted variance is the clip 1e-10, exactly, on every path -- next to an output in the base
    regime, which keeps its own variances."""
    spec = [("rbf", E.CLIP_CASE, 0), ("matern52", E.BASE, 1), ("matern32", E.CLIP_CASE, 2)]
    X, Xc, Y = _data(spec, E.N_MAX, E.C_REDUCED)
    model = _fixed_model(B, spec, X, Y)
    base = E.case_truth("matern52", E.BASE.name, E.N_MAX)
    for option in (None, "predict_f32", "predict_i8"):
        if option:
            model.set_option(option, 1)
        try:
            got = [model.predict(Xc)[1], model.posterior_variance_noiseless(Xc), model.predict(Xc[:E.C_SMALL])[1],
                   model.posterior_variance_noiseless(Xc[:E.C_SMALL])]
        finally:
            if option:
                model.set_option(option, 0)
        for v in got:
            print("clip, %-11s %3d candidates: outputs 0 and 2 in [%g, %g]" % (option or "fp64", v.shape[1], v[[0, 2]].min(), v[[0, 2]].max()))
            np.testing.assert_array_equal(v[[0, 2]], 1e-10)
        if option is None:
            assert E.fraction(got[1][1][:E.C_TILE], np.clip(base["raw_var"], 1e-10, None), 0.0, 1e-8) <= 1.0


def test_zz_largest_error_per_regime():
    """Prints what the tests above saw: per regime family and quantity the largest error as a fraction of its gate."""
    groups = sorted({g for g, _ in STATS})
    for g in groups:
        print("%-20s %s" % (g, "  ".join("%s %.2g" % (w, STATS[(gg, w)]) for gg, w in sorted(STATS) if gg == g)))
    for g in groups:
        print("%-20s largest %.3g" % (g, max(v for (gg, _), v in STATS.items() if gg == g)))
