"""What the extreme-regime tests share (tests/test_extremes_cpu.py, tests/test_gpu_extremes.py): the table of cases -- lengthscales from
1e-3 to 300, kernel variances from 1e-6 to 1e6, noise from 1e-10 to 100, inputs scaled and offset, one ARD kernel with six decades between
its lengthscales, and a d = 1 ramp whose exponentials run through the subnormal band into zero -- an extended-precision truth of every
quantity the device returns for them, and the gates.  Test infrastructure only: nothing under bocf_amd/ imports it.

The truth is numpy.longdouble (x87: eps 1.08e-19) from the fp64 SCALED coordinates Xs = fl(X / l), Xcs = fl(Xc / l): the problem the device
solves after scale_inputs_kernel (fp64 division is correctly rounded on both sides), so that offset inputs have an exact reference too.
The gates are the project's own tolerances, each absolute one multiplied by the unit of the case (sigma_f, sigma_f^2, 1 / l_q, ...), and
max(that floor, 4 x the fp64 oracle's own error against the truth) where the oracle runs (oracle.truth.gate's rule)."""
import collections
import functools

import numpy as np

from oracle import cpu_ref as R

LD = np.longdouble
FAMILIES = ("rbf", "matern52", "matern32")
D = 3
A_DIR = np.array([1.0, 0.7, 0.4])                       # y = sin(2 pi x . a) + 0.1 eps, times sigma_f
SEED = 6                                                # (how it was chosen: tests/test_extremes_cpu.py)
N_MAX, C_TILE, C_SMALL, C_REDUCED = 130, 40, 8, 300

Case = collections.namedtuple("Case", "name group ls variance noise scale offset")


def have_x87():
    return np.finfo(LD).eps < 2e-19


def _ard(ell):
    return ell * (1.0 + 0.1 * np.arange(D))


def _cases():
    out = []
    for ell in (1e-3, 0.02, 0.1, 0.5, 3.0, 30.0, 300.0):
        out.append(Case("l=%g" % ell, "lengthscale", _ard(ell), 1.0, 1e-4, 1.0, 0.0))
    for v in (1e-6, 1e-3, 1e3, 1e6):
        out.append(Case("var=%g" % v, "variance", _ard(0.5), v, 1e-4 * v, 1.0, 0.0))
    for nz in (1e-10, 1e-8, 1e-2, 1.0, 100.0):
        out.append(Case("noise=%g" % nz, "noise", _ard(0.5), 1.0, nz, 1.0, 0.0))
    for s, o in ((1e3, 0.0), (1e-3, 0.0), (1.0, 1e3), (1.0, 1e6), (1e3, -500.0)):
        out.append(Case("s=%g,o=%g" % (s, o), "offset" if (o and s == 1.0) else "input", _ard(0.5 * s), 1.0, 1e-4, s, o))
    out.append(Case("ard=(0.01,0.5,100)", "mixed", np.array([0.01, 0.5, 100.0]), 1.0, 1e-4, 1.0, 0.0))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
BASE = BY_NAME["l=0.5"]
SAME_X = [c for c in CASES if c.scale == 1.0 and c.offset == 0.0]         # the 17 regimes on the base inputs
INPUT = [c for c in CASES if not (c.scale == 1.0 and c.offset == 0.0)]    # the 5 regimes that move the inputs
SE_CASES = [c for c in CASES if c.group == "lengthscale"]                 # kernel id 1 runs the lengthscale cases too
CLIP_CASE = Case("clip", "clip", _ard(0.5), 1e-12, 0.0, 1.0, 0.0)


@functools.lru_cache(maxsize=None)
def _draws():
    rng = np.random.RandomState(SEED)
    X0 = rng.uniform(size=(N_MAX, D))
    eps = rng.normal(size=(len(FAMILIES) + 1, N_MAX))
    Xc0 = rng.uniform(-0.3, 1.3, size=(C_REDUCED, D))   # candidates reach beyond the data: no raw variance anywhere near the 1e-10 clip
    for a in (X0, eps, Xc0):
        a.setflags(write=False)
    return X0, eps, Xc0


def inputs(case, N, C=C_TILE):
    """(X (N, d), Xc (C, d)) of a case: the base draw scaled and offset."""
    X0, _, Xc0 = _draws()
    return case.scale * X0[:N] + case.offset, case.scale * Xc0[:C] + case.offset


def targets(case, N, slot):
    """y of output slot `slot`: the same function of the BASE inputs whatever the case does to them, times sigma_f."""
    X0, eps, _ = _draws()
    return np.sqrt(case.variance) * (np.sin(2.0 * np.pi * X0[:N].dot(A_DIR)) + 0.1 * eps[slot, :N])


# ------------------------------------------------------------------------------------------------------------------------
# the ramp: d = 1, N = 128, the decay argument u of every family runs from 0 to ~1200 over the pairs
# ------------------------------------------------------------------------------------------------------------------------
RAMP_N = 128
RAMP_U = 1200.0
RAMP_LS = {"rbf": 1.0 / np.sqrt(2.0 * RAMP_U), "se": 1.0 / np.sqrt(2.0 * RAMP_U), "matern52": np.sqrt(5.0) / RAMP_U,
           "matern32": np.sqrt(3.0) / RAMP_U}


def ramp_inputs():
    return np.linspace(0.0, 1.0, RAMP_N)[:, None]


def ramp_targets(slot):
    return np.sin(7.0 * ramp_inputs()[:, 0] + slot)


# ------------------------------------------------------------------------------------------------------------------------
# the truth
# ------------------------------------------------------------------------------------------------------------------------
_SQRT5, _SQRT3 = np.sqrt(LD(5)), np.sqrt(LD(3))
_LOG2PI = np.log(LD(8) * np.arctan(LD(1)))
_TINY = LD(2) ** -1022


def _family(kind):
    return "rbf" if kind == "se" else kind


def kernel_pieces(kind, r2, variance, flush=False, amp_r2=None):
    """(u, e^-u, k, f) of kern_family.h from r2, in long double.  flush: the exponential set to zero below 2^-1022 (a perturbation);
    amp_r2: the r2 the Matern52 amplitude sees instead of the true one (a perturbation)."""
    fam = _family(kind)
    v = LD(variance)
    if fam == "rbf":
        u = r2 / 2
    else:
        u = (_SQRT5 if fam == "matern52" else _SQRT3) * np.sqrt(r2)
    e = np.exp(-u)
    if flush:
        e = np.where(e < _TINY, LD(0), e)
    if fam == "rbf":
        return u, e, v * e, v * e
    if fam == "matern52":
        a2 = r2 if amp_r2 is None else amp_r2
        return u, e, v * (1 + u + LD(5) / 3 * a2) * e, LD(5) / 3 * v * (1 + u) * e
    return u, e, v * (1 + u) * e, 3 * v * e


def chol_ld(A):
    """Plain column Cholesky, lower."""
    L = np.array(A, dtype=LD)
    n = L.shape[0]
    for k in range(n):
        if not L[k, k] > 0:
            raise np.linalg.LinAlgError("truth: pivot %d not positive" % k)
        L[k, k] = np.sqrt(L[k, k])
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return np.tril(L)


def solve_lower(L, B):
    Z = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        Z[i] = (Z[i] - L[i, :i].dot(Z[:i])) / L[i, i]
    return Z


def truth(kind, X, y, variance, ls, noise, Xc, jitter=0.0, flush=False, amp_unscaled=False):
    """One output, everything in long double from Xs = fl(X / ls), Xcs = fl(Xc / ls).  Returns a dict of long-double arrays:
    K, u (N, N); alpha (N), lml; dv, dl (d), dn with their sums of absolute terms dv_abs, dl_abs, dn_abs; mean (C), raw_var (C) =
    sigma_f^2 - ||L^-1 k*||^2 (no noise, no clip), mu_train (N), dmean, dvar (C, d); cond: the fp64 2-norm condition of Ky."""
    ls = np.asarray(ls, dtype=float)
    Xs, Xcs = np.asarray(X, dtype=float) / ls, np.asarray(Xc, dtype=float) / ls
    N = Xs.shape[0]
    lsl, v = ls.astype(LD), LD(variance)
    Dt = Xs.astype(LD)[:, None, :] - Xs.astype(LD)[None, :, :]
    r2 = np.square(Dt).sum(-1)
    amp_r2 = np.square(Dt * lsl).sum(-1) if amp_unscaled else None
    u, e, K, f = kernel_pieces(kind, r2, variance, flush, amp_r2)
    Ky = K.copy()
    Ky[np.diag_indices(N)] += LD(noise) + LD(1e-8) + LD(jitter)
    L = chol_ld(Ky)
    y = np.asarray(y, dtype=float).reshape(N).astype(LD)
    ymean = y.sum() / N
    yc = y - ymean
    Li = solve_lower(L, np.eye(N, dtype=LD))
    alpha = Li.T.dot(Li.dot(yc))
    lml = -(N * _LOG2PI + 2 * np.log(np.diag(L)).sum() + yc.dot(alpha)) / 2
    Kinv = Li.T.dot(Li)
    G = (np.outer(alpha, alpha) - Kinv) / 2
    dn, dn_abs = np.trace(G), np.abs(np.diag(G)).sum()
    dv, dv_abs = (G * K).sum() / v, np.abs(G * K).sum() / v
    Gf = G * f
    dl = np.array([(Gf * np.square(Dt[:, :, q])).sum() / lsl[q] for q in range(ls.size)], dtype=LD)
    dl_abs = np.array([np.abs(Gf * np.square(Dt[:, :, q])).sum() / lsl[q] for q in range(ls.size)], dtype=LD)
    # candidates: Dc[c, i, q] = scaled (xc_q - x_iq)
    Dc = Xcs.astype(LD)[:, None, :] - Xs.astype(LD)[None, :, :]
    r2c = np.square(Dc).sum(-1)
    amp_r2c = np.square(Dc * lsl).sum(-1) if amp_unscaled else None
    _, _, Kc, fc = kernel_pieces(kind, r2c, variance, flush, amp_r2c)              # (C, N)
    V = Li.dot(Kc.T)
    raw_var = v - np.square(V).sum(0)
    w = -2 * Kc.dot(Kinv)                                                           # (C, N)
    dmean = -np.einsum("i,ci,ciq->cq", alpha, fc, Dc) / lsl
    dvar = -np.einsum("ci,ci,ciq->cq", w, fc, Dc) / lsl
    cond = float(np.linalg.cond(Ky.astype(float)))
    return dict(K=K, u=u, alpha=alpha, lml=lml, dv=dv, dl=dl, dn=dn, dv_abs=dv_abs, dl_abs=dl_abs, dn_abs=dn_abs, mean=Kc.dot(alpha) + ymean,
                raw_var=raw_var, mu_train=K.dot(alpha) + ymean, dmean=dmean, dvar=dvar, cond=cond, ymean=ymean)


@functools.lru_cache(maxsize=None)
def case_truth(kind, name, N, slot=None):
    """The truth of a case (cached, read-only).  The targets are those of the family's slot unless `slot` says otherwise."""
    case = CLIP_CASE if name == "clip" else BY_NAME[name]
    X, Xc = inputs(case, N)
    s = FAMILIES.index(_family(kind)) if slot is None else slot
    return truth(kind, X, targets(case, N, s), case.variance, case.ls, case.noise, Xc)


def oracle_fit(kind, case, N, slot=None):
    """oracle.cpu_ref's fit of a case; None where its Cholesky fails even with jitter."""
    X, _ = inputs(case, N)
    s = FAMILIES.index(_family(kind)) if slot is None else slot
    try:
        return R.GPFit(kind, X, targets(case, N, s), case.variance, case.ls, case.noise)
    except np.linalg.LinAlgError:
        return None


def oracle_quantities(fit, Xc):
    """The oracle's values of what `truth` returns, as fp64 arrays under the same names."""
    dv, dl, dn = fit.lml_gradients()
    return dict(alpha=fit.alpha[:, 0], lml=fit.log_marginal, dv=dv, dl=dl, dn=dn, mean=fit.posterior_mean(Xc)[:, 0],
                raw_var=fit.raw_posterior_variance(Xc)[:, 0], mu_train=fit.posterior_mean(fit.X)[:, 0],
                dmean=fit.posterior_mean_gradient(Xc), dvar=fit.posterior_variance_gradient(Xc))


# ------------------------------------------------------------------------------------------------------------------------
# the gates
# ------------------------------------------------------------------------------------------------------------------------
def floors(t, variance, ls, N):
    """name -> (rtol, atol): the project's tolerances with every absolute one in the unit of the case.
    mean, mu_train      rtol 1e-6, atol 1e-7 sigma_f            test_random_shapes
    raw_var             1e-8 sigma_f^2                           test_random_shapes
    lml                 rtol 1e-9, atol 1e-9                     test_random_shapes
    alpha               rtol 1e-6, atol 1e-9 / sigma_f           tests/test_gpu_incremental.py
    dmean               rtol 1e-5, atol 1e-6 sigma_f / l_q       test_random_shapes
    dvar                rtol 1e-4, atol 1e-7 sigma_f^2 / l_q     test_random_shapes
    dv, dl, dn          rtol 1e-6, atol N^2 2^-53 sum |terms|    test_hyper_gradients_golden + fp64 summation of N^2 terms"""
    sf, ls = np.sqrt(variance), np.asarray(ls, dtype=float)
    sumtol = N * N * 2.0 ** -53
    return dict(mean=(1e-6, 1e-7 * sf), mu_train=(1e-6, 1e-7 * sf), raw_var=(0.0, 1e-8 * variance), lml=(1e-9, 1e-9),
                alpha=(1e-6, 1e-9 / sf), dmean=(1e-5, 1e-6 * sf / ls), dvar=(1e-4, 1e-7 * variance / ls),
                dv=(1e-6, sumtol * float(t["dv_abs"])), dl=(1e-6, sumtol * t["dl_abs"].astype(float)), dn=(1e-6, sumtol * float(t["dn_abs"])))


def error(got, want):
    """max |got - want| with the difference taken in long double."""
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD))))


def fraction(got, want, rtol, atol, e_oracle=0.0):
    """The largest |got - want| / max(atol + rtol |want|, 4 e_oracle) over the entries: <= 1 passes."""
    want = np.asarray(want, dtype=LD)
    err = np.abs(np.asarray(got, dtype=LD) - want).astype(float)
    allow = np.maximum(np.asarray(atol, dtype=float) + rtol * np.abs(want).astype(float), 4.0 * e_oracle)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0.0, 0.0, err / allow)))                # (an allowance of zero admits an exact zero only)


def k_entry_bound(t, variance, d):
    """|K_dev - K_true| <= (d + 10) (1 + u) 2^-53 K_true + sigma_f^2 2^-1074, per entry (long double: the second term is below fp64's
    normal range).  d differences, d fused multiply-adds, a square root and a product for u, whose rounding the exponential amplifies by
    u; the polynomial's <= 1 ulp and the amplitude's few roundings; one subnormal ulp."""
    return (d + 10) * (1 + t["u"]) * LD(2) ** -53 * t["K"] + LD(variance) * LD(2) ** -1074


@functools.lru_cache(maxsize=None)
def oracle_errors(kind, name, N, slot=None):
    """name -> max |oracle - truth| per quantity, the err_oracle of the gates; every entry 0.0 where the oracle does not serve: inputs with
    an offset (its ||x||^2 + ||y||^2 - 2 x.y distance degrades there, tests/test_extremes_cpu.py records how far) or a failed Cholesky.
    Also "jitter": what the oracle's jitchol added (nan: it failed), and "values": the oracle's quantities themselves (None: it failed)."""
    case = BY_NAME[name]
    t = case_truth(kind, name, N, slot)
    zero = dict.fromkeys(floors(t, case.variance, case.ls, N), 0.0)
    fit = oracle_fit(kind, case, N, slot)
    if fit is None:
        return dict(zero, jitter=float("nan"), values=None)
    o = oracle_quantities(fit, inputs(case, N)[1])
    raw = {q: error(o[q], t[q]) for q in zero}
    return dict(zero if case.offset else raw, jitter=fit.jitter, values=o)
