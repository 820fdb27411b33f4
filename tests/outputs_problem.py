"""The problems the output-count sweep shares (tests/test_output_counts_cpu.py, tests/test_gpu_output_counts.py): one seeded problem per
number of outputs m = 1 ... 16 -- d = 3, N = 40, noise 1e-4, output j with kernel family MIXED[j % 4], variances and ARD lengthscales
distinct per output as in kg_ref.problem -- the oracle's fit of it (computed once per m, never modified), the inputs of every acquisition
the sweep runs, and the gates the sweep applies: the project's own, named after the tests they come from.  Test infrastructure only:
nothing under bocf_amd/ imports it.

Shapes: the smallest that still reach the kernels' edges.  C = 130 candidates (one wave per candidate, four per workgroup: the last
workgroup is ragged), S = 65 normals (past one wave of samples, ragged), L = 2 weighted utility parameters; KG: 7 reference points, 4
fantasies; pending: 3 points; constrained: 2 rows; paths: 130 features, 5 paths.

The evaluated points lie in [0, 0.7]^3 and the targets have amplitude 0.3, the candidates cover the unit box: with 40 evaluated points
spread over the whole box and targets of amplitude 1 only 1 ... 22 % of the candidates improve on the best evaluated point under
neg_sum_exp (which has no parameter to place), and a comparison of zeros checks nothing.  The utility parameters are placed from the
oracle's posterior alone: supports are tried in a fixed, seeded order and the first one the ORACLE accepts is taken (at least a quarter of
the candidates with a value above 10^3 x the absolute tolerance of the comparison, every gradient coordinate above 10^4 x its absolute
tolerance at some candidate, no Monte-Carlo sample within 1e-7 of its hinge, at most 5 % of the gradient
candidates with a sample within 1e-6 x the utility's scale of it).  The device never enters the choice."""
import functools

import numpy as np

import constrained_ref as CR
import kg_ref as K
import paths_ref as PTH
import pending_ref as PR

from oracle import cpu_ref as R

MS = list(range(1, 17))
MIXED = ["se", "matern52", "rbf", "matern32"]           # output j: MIXED[j % 4]
D, N, C, S, L = 3, 40, 130, 65, 2
NOISE = 1e-4
NGRAD = 40                                              # the gradient checks use the first 40 candidates (tile path), as NGRAD of the pending / constrained tests
PROB = np.array([0.4, 0.6])
NA, SF = 7, 4                                           # KG: reference points, fantasies
RP = 3                                                  # pending points
KC, ETA = 2, 0.05                                       # constraint rows and their smoothing width
F_PATHS, S_PATHS = 130, 5
UTILS = ["linear", "neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock"]
SEEDS = {m: 4200 + m for m in MS}
SEEDS[12] = 4300                                        # (seed 4212: 8 % of the candidates improve under rosenbrock whatever its parameter)

# ---- gates: (rtol, atol), copied from the tests named
MC_VALUE = (1e-5, 1e-9)                                 # test_mc_acquisition_every_output_count
ACQ_VALUE, ACQ_GRAD = (1e-5, 1e-10), (1e-4, 1e-8)       # test_fixed_hyps_every_dimension: maEI, uEI with gradient; their gradients
EU_RTOL, EU_ATOL_SCALE = 1e-9, 1e-9                     # test_expected_utility_matches_oracle_fixed_hyps: atol = 1e-9 max |reference|
KG_RTOL, KG_ATOL_SCALE, KG_TIE = 1e-5, 1e-12, 1e-6      # test_kg_values / test_kg_gradients: atol = 1e-12 x term size; near-tie: gap < 1e-6 max |KG|
PEND_RTOL, PEND_ATOL_SCALE, PEND_NEAR = 1e-5, 1e-12, 1e-6   # test_gpu_pending: atol = 1e-12 x scale; near a threshold: gap < 1e-6 scale
CON_VALUE, CON_BEST = (1e-5, 1e-12), (1e-6, 1e-9)       # test_gpu_constrained: values, feasible best; gradients rtol 1e-4, atol 1e-9 max(1, max |g|)
CON_GRAD_RTOL, CON_GRAD_ATOL = 1e-4, 1e-9
LEFT_OUT = 0.05                                         # the largest share of candidates a gradient check may leave out
NONZERO_SHARE = 0.25
MEAN_RTOL, MEAN_ATOL, VAR_GATE = 1e-6, 1e-7, 1e-8       # test_random_shapes: mean, variance |delta| <= 1e-8 max sigma_f^2
SELECT_VALUE = (1e-13, 1e-13)                           # test_thompson_select_against_numpy: the k selected values against U of the samples ranked
PATH_VALUE_SCALE = 1e-10                                # test_gpu_paths.py: path values |delta| <= 1e-10 max sigma_f^2; their input gradients carry 1 / min l
K_SELECT = 9
MC_HINGE = 1e-7                                         # no sample's utility within this of the best-so-far (value gates are 1e-9 .. 1e-10)


def utilities(m):
    """The device utilities an m-output model takes: rosenbrock needs an even m."""
    return [u for u in UTILS if u != "rosenbrock" or m % 2 == 0]


def kinds(m):
    return [MIXED[j % 4] for j in range(m)]


@functools.lru_cache(maxsize=None)
def problem(m, n_train=N):
    """kg_ref.problem with the evaluated points in [0, 0.7]^d and targets of amplitude 0.3 (see the module text), and the normals and
    point sets of the acquisitions from a second stream: the data do not move when one of those shapes does."""
    seed = SEEDS[m] + (0 if n_train == N else 1000)
    rng = np.random.RandomState(seed)
    X = 0.7 * rng.uniform(size=(n_train, D))
    Xc = rng.uniform(size=(C, D))
    variances = rng.uniform(0.8, 1.6, size=m)
    lengthscales = rng.uniform(0.4, 0.7, size=(m, D)) * np.sqrt(D)
    freq = rng.uniform(1.0, 3.0, size=(m, D))
    phase = rng.uniform(0, 2 * np.pi, size=(m, D))
    Y = [0.3 * np.sum(np.sin(X * freq[j] + phase[j]), 1) / np.sqrt(D) + 0.01 * rng.normal(size=n_train) for j in range(m)]
    rng = np.random.RandomState(9000 + seed)
    return dict(m=m, kinds=kinds(m), X=X, Y=Y, var=variances, ls=lengthscales, nz=np.full(m, NOISE), Xc=Xc, W=rng.normal(size=(S, m)),
                Zf=rng.normal(size=(SF, m)), A=rng.uniform(size=(NA, D)), Zeu=rng.normal(size=(L, S, m)),
                rows=np.arange(C) % L)


@functools.lru_cache(maxsize=None)
def oracle(m, n_train=N):
    """(problem, LookAhead over the oracle's fits, the same fits as a MultiOutputGPRef) of an output count: read-only."""
    p = problem(m, n_train)
    la = K.LookAhead.fit(p["kinds"], p["X"], p["Y"], p["var"], p["ls"], p["nz"])
    ref = R.MultiOutputGPRef(p["kinds"], p["var"], list(p["ls"]), list(p["nz"]))
    ref.output = list(la.fits)
    return p, la, ref


def hyper_lookaheads(m, H):
    """One LookAhead per hyper-sample, scaled as _hyper_model of test_gpu_kg.py scales them: variances x (1 + 0.1 h), lengthscales x (1 - 0.05 h)."""
    p = problem(m)
    return [K.LookAhead.fit(p["kinds"], p["X"], p["Y"], p["var"] * (1 + 0.1 * h), p["ls"] * (1 - 0.05 * h), p["nz"]) for h in range(H)]


def posterior_of(la, Xc, grad=True):
    """What the acquisitions read, from a LookAhead: mean, var (noise included, clipped), var0 (noiseless, clipped), mu_eval, and the input
    gradients at the first NGRAD candidates."""
    mean, var = CR.posterior(la, Xc)
    out = dict(mean=mean, var=var, sigma=np.sqrt(var), mu_eval=CR.train_mean(la),
               var0=np.stack([f.posterior_variance_noiseless(Xc)[:, 0] for f in la.fits]))
    if grad:
        Xg = Xc[:NGRAD]
        out["dmean"] = np.stack([f.posterior_mean_gradient(Xg) for f in la.fits])
        out["dvar"] = np.stack([f.posterior_variance_gradient(Xg) for f in la.fits])
    return out


@functools.lru_cache(maxsize=None)
def posterior(m):
    p, la, _ = oracle(m)
    return posterior_of(la, p["Xc"])


# ---- perturbations of a posterior (tests/test_output_counts_cpu.py): the arrays are copied, the cached ones stay as they are
def shifted(post, j, step=0.1):
    """Output j alone: its posterior mean moved by step x its posterior standard deviation, its input gradients scaled by 1 + step (a
    gradient that is linear in the means, such as that of theta . mu, does not see the first)."""
    out = dict(post)
    out["mean"] = post["mean"].copy()
    out["mean"][j] += step * post["sigma"][j]
    for k in ("dmean", "dvar"):
        out[k] = post[k].copy()
        out[k][j] *= 1.0 + step
    return out


def swapped(post, j):
    """Outputs j and j + 1 exchanged in everything the model hands over -- the normals and the utility parameters stay in place."""
    out = {}
    for k, v in post.items():
        v = v.copy()
        v[[j, j + 1]] = v[[j + 1, j]]
        out[k] = v
    return out


# ---- the utilities, vectorised over trailing axes (checked against oracle.cpu_ref.utility_grad in the CPU file)
def utility_grad_vec(kind, theta, y, params=None):
    """dU/dy for y (m, ...) -> (m, ...)."""
    theta = np.atleast_1d(np.asarray(theta, dtype=float))
    sh = (-1,) + (1,) * (y.ndim - 1)
    if kind == "linear":
        return np.broadcast_to(theta.reshape(sh), y.shape).copy()
    if kind == "neg_sq_dist":
        return -2.0 * (y - theta.reshape(sh))
    if kind == "neg_sum_exp":
        return -np.exp(y)
    if kind == "neg_exp_cos":
        e = np.exp(-y / np.pi)
        return np.asarray(params, dtype=float).reshape(sh) * (np.pi * e * np.sin(np.pi * y) + e * np.cos(np.pi * y) / np.pi)
    if kind == "rosenbrock":
        h = y.shape[0] // 2
        g = np.zeros_like(y)
        g[:h] = 2.0 * (theta[0] - y[:h])
        g[h:2 * h] = -200.0 * y[h:2 * h]
        return g
    raise ValueError(kind)


def mc_grad_vec(post, W, kind, thetas, prob, params=None):
    """oracle.cpu_ref.mc_acq_with_gradient at the first NGRAD candidates, vectorised: (acq (n,), dacq (n, d), gap (n,) = the smallest
    |U - best| over parameters and samples, scale = the largest |U| met)."""
    mu, sg = post["mean"][:, :NGRAD], post["sigma"][:, :NGRAD]
    dmu, dvar = post["dmean"], post["dvar"]
    m, n = mu.shape
    acq, dacq, gap, scale = np.zeros(n), np.zeros((n, dmu.shape[2])), np.full(n, np.inf), 0.0
    y = mu[:, None, :] + sg[:, None, :] * W.T[:, :, None]                        # (m, S, n)
    for l, th in enumerate(np.atleast_2d(thetas)):
        best = np.max(R.utility_eval(kind, th, post["mu_eval"], params))
        u = R.utility_eval(kind, th, y.reshape(m, -1), params).reshape(y.shape[1:])
        gap, scale = np.minimum(gap, np.min(np.abs(u - best), 0)), max(scale, float(np.max(np.abs(u))), abs(float(best)))
        g = utility_grad_vec(kind, th, y, params) * (u > best)[None]
        acq += prob[l] * np.maximum(u - best, 0.0).mean(0)
        a, b = g.mean(1), (g * W.T[:, :, None]).mean(1) * 0.5 / sg
        dacq += prob[l] * (np.einsum("jn,jnq->nq", a, dmu) + np.einsum("jn,jnq->nq", b, dvar))
    return acq, dacq, gap, scale


def mc_values(post, W, kind, thetas, prob, params=None, acq="EI"):
    return R.mc_acq(post["mean"], post["sigma"], post["mu_eval"], W, kind, thetas, prob, acq, params)[0][:, 0]


def ma_values(post, thetas, prob, acq="EI"):
    return R.ma_acq(post["mean"], post["var"], post["mu_eval"], thetas, prob, acq)[0][:, 0]


def ma_grad(post, thetas, prob, acq="EI"):
    a, da = R.ma_acq_with_gradient(post["mean"][:, :NGRAD], post["var"][:, :NGRAD], post["dmean"], post["dvar"], post["mu_eval"], thetas, prob, acq)
    return a[:, 0], da


def share(values, atol):
    """The share of the candidates whose reference value lies above 10^3 x the absolute tolerance of its comparison."""
    return float(np.mean(np.asarray(values) > 1e3 * atol))


def every_coordinate(grad, atol):
    """Every input coordinate exceeds 10^4 x its absolute tolerance at some candidate."""
    return bool(np.all(np.abs(grad).max(0) > 1e4 * atol))


def _support_candidates(m, kind):
    """The supports (thetas (L, theta_dim), params) tried for a utility, in their fixed order."""
    post = posterior(m)
    rng = np.random.RandomState(7000 + 100 * m + UTILS.index(kind))
    mu = post["mean"]
    for t in range(300):
        if kind == "linear":
            yield rng.normal(size=(L, m)), None
        elif kind == "neg_sq_dist":
            i, k = rng.randint(0, C, 2)
            yield np.stack([mu[:, i], mu[:, k]]) + 0.05 * rng.normal(size=(L, m)), None
        elif kind == "neg_sum_exp":
            yield np.zeros((L, 1)), None
            return
        elif kind == "neg_exp_cos":
            yield np.zeros((L, 1)), rng.uniform(0.5, 1.0, size=m)
        else:                                           # rosenbrock: a near the targets first; from many outputs on only a large a, whose
            yield (1.0 if t < 60 else 10.0) * rng.uniform(-0.3, 0.8, size=(L, 1)), None      # (a - y)^2 outweighs the 100 y^2 terms, lets a quarter improve


def accepts(m, kind, thetas, params):
    """The input conditions of a support, on the oracle's posterior alone."""
    post, W = posterior(m), problem(m)["W"]
    if share(mc_values(post, W, kind, thetas, PROB, params, "EI"), MC_VALUE[1]) < NONZERO_SHARE:
        return False
    if share(mc_values(post, W, kind, thetas, PROB, params, "PI"), MC_VALUE[1]) < NONZERO_SHARE:
        return False
    a, da, gap, scale = mc_grad_vec(post, W, kind, thetas, PROB, params)
    if not every_coordinate(da, ACQ_GRAD[1]) or gap.min() < MC_HINGE or np.mean(gap < PEND_NEAR * scale) > LEFT_OUT:
        return False
    if kind == "linear":
        for acq in ("EI", "PI"):
            if share(ma_values(post, thetas, PROB, acq), ACQ_VALUE[1]) < NONZERO_SHARE or not every_coordinate(ma_grad(post, thetas, PROB, acq)[1], ACQ_GRAD[1]):
                return False
    return True


@functools.lru_cache(maxsize=None)
def support(m, kind):
    """(thetas (L, theta_dim), params or None) of a utility: the first of _support_candidates the oracle accepts."""
    for thetas, params in _support_candidates(m, kind):
        if accepts(m, kind, thetas, params):
            return thetas, params
    raise AssertionError("m = %d, %s: no support meets the input conditions" % (m, kind))


# ---- expected utility: the restatement of tests/test_gpu_recommend.py (_restated) on posterior arrays, each candidate with its own row
def expected_utility(post, mode, kind, thetas, rows, Z, params=None, n=None, grad=True):
    """(v (n,), dv (NGRAD, d)), or v alone with grad=False, under the noiseless posterior: "mean" theta . mu, "closed" kg_ref.closed_form, "mc" the sum over the S
    normals Z[row] of U(theta, mu + sigma o z)."""
    mean, var = post["mean"], post["var0"]
    n = mean.shape[1] if n is None else n
    val, dval = np.zeros(n), (np.zeros((min(n, NGRAD), post["dmean"].shape[2])) if grad else None)
    for l, th in enumerate(np.atleast_2d(thetas)):
        sel = np.flatnonzero(rows[:n] == l)
        mu, s2 = mean[:, sel], var[:, sel]
        if mode == "mc":
            sg = np.sqrt(s2)
            y = mu[:, :, None] + sg[:, :, None] * Z[l].T[:, None, :]              # (m, n_l, S)
            val[sel] = R.utility_eval(kind, th, y.reshape(len(mu), -1), params).reshape(len(sel), -1).sum(-1)
            g = utility_grad_vec(kind, th, y, params)
            A, Bv = g.sum(-1), (g * Z[l].T[:, None, :]).sum(-1) / (2 * sg)
        else:
            v, A, Bv = K.inner_value(mode, kind, th, mu, s2, partials=True)
            val[sel] = v
        if not grad:
            continue
        gs = sel < NGRAD
        dval[sel[gs]] = np.einsum("ji,jiq->iq", A[:, gs], post["dmean"][:, sel[gs]]) + np.einsum("ji,jiq->iq", Bv[:, gs], post["dvar"][:, sel[gs]])
    return (val, dval) if grad else val


def eu_cases(m):
    """(mode, utility) pairs the device admits (_cases of tests/test_gpu_recommend.py)."""
    out = [("mean", "linear")]
    out += [("closed", k) for k in ("neg_sq_dist", "neg_sum_exp", "rosenbrock") if k in utilities(m)]
    out += [("mc", k) for k in utilities(m)]
    return out


kg_cases = eu_cases                                     # the knowledge gradient admits the same (mode, utility) pairs


def kg_reference(las, p, mode, kind, thetas, params, grad=False, n=None, Zf=None, W=None, A=None):
    """_ref_kg of tests/test_gpu_kg.py: the mean over the hyper-samples' restatements (kg, gap, vscale, dkg)."""
    Xc = p["Xc"] if n is None else p["Xc"][:n]
    Zf, W, A = (p["Zf"] if Zf is None else Zf), (p["W"] if W is None else W), (p["A"] if A is None else A)
    rs = [la.kg(Xc, A, Zf, thetas, PROB, mode, kind, W, params, grad=grad) for la in las]
    out = dict(kg=np.mean([r["kg"] for r in rs], 0), gap=np.min([r["gap"] for r in rs], 0), vscale=max(r["vscale"] for r in rs))
    if grad:
        out["dkg"] = np.mean([r["dkg"] for r in rs], 0)
    return out


# ---- pending points and constraints: drawn in a fixed order, the first the oracle accepts
def pending_inputs(m, kind, draw=0):
    """The dict tests/pending_ref.case_reference takes (H = 1).  Draws 0 .. 9 put the pending points anywhere in the unit box, the later
    ones among the evaluated points ([0, 0.7]^3), where the joint samples stay near the evaluated utilities: a lower threshold, a smaller scale."""
    p = problem(m)
    rng = np.random.RandomState(5000 + 100 * m + draw)
    thetas, params = support(m, kind)
    return dict(kinds=p["kinds"], X=p["X"], Y=p["Y"], var=p["var"], ls=p["ls"], nz=p["nz"], Xc=p["Xc"], P=(1.0 if draw < 10 else 0.7) * rng.uniform(size=(RP, D)),
                Zp=rng.normal(size=(S, m, RP)), W=p["W"], thetas=thetas, prob=PROB, params=params, kind=kind, H=1)


def pending_ok(ref, refg):
    """At least a quarter of the candidates carry a value, at most 5 % of the gradient candidates sit near a threshold, every coordinate
    carries a gradient at a kept candidate."""
    keep = refg["gap"] >= PEND_NEAR * refg["scale"]
    gscale = np.abs(refg["dalpha"]).max()
    return (share(ref["alpha"], PEND_ATOL_SCALE * ref["scale"]) >= NONZERO_SHARE and np.mean(~keep) <= LEFT_OUT
            and gscale > 0 and every_coordinate(refg["dalpha"][keep], PEND_ATOL_SCALE * gscale))


@functools.lru_cache(maxsize=None)
def pending_case(m, kind):
    """(inputs, restatement of all candidates, restatement with gradients of the first NGRAD) of the first accepted draw."""
    _, la, _ = oracle(m)
    for draw in range(30):
        inp = pending_inputs(m, kind, draw)
        ref = PR.case_reference(inp, [la])
        if share(ref["alpha"], PEND_ATOL_SCALE * ref["scale"]) < NONZERO_SHARE:
            continue
        refg = PR.case_reference(inp, [la], grad=True, n=NGRAD)
        if pending_ok(ref, refg):
            return inp, ref, refg
    raise AssertionError("m = %d, %s: no pending set meets the input conditions" % (m, kind))


def constrained_reference(post, p, kind, thetas, params, con, grad=False, best=None, W=None, n=None):
    """tests/constrained_ref.constrained on all candidates, or with gradients on the first n (NGRAD by default)."""
    A, b, eta = con
    n = (NGRAD if grad else C) if n is None else n
    return CR.constrained(post["mean"][:, :n], post["var"][:, :n], post["mu_eval"], p["W"] if W is None else W, thetas, PROB, kind, params, A, b, eta,
                          post["dmean"][:, :n] if grad else None, post["dvar"][:, :n] if grad else None, best=best)


def constrained_ok(ref, refg):
    g = refg["dalpha"]
    return (share(ref["alpha"], CON_VALUE[1]) >= NONZERO_SHARE and ref["n_feasible"] > 0
            and every_coordinate(g, CON_GRAD_ATOL * max(1.0, np.abs(g).max())) and min(ref["gap"].min(), refg["gap"].min()) >= MC_HINGE)


@functools.lru_cache(maxsize=None)
def constrained_case(m, kind):
    """((A, b, eta), restatement of all candidates, restatement with gradients of the first NGRAD): constraints drawn as
    tests/test_gpu_constrained.py draws them (few feasible evaluated points: a weak incumbent), the first draw the oracle accepts."""
    p, post = problem(m), posterior(m)
    thetas, params = support(m, kind)
    for draw in range(40):
        con = CR.draw_constraints(np.random.RandomState(6000 + 100 * m + draw), post["mu_eval"], KC, ETA, share=0.15)
        ref = constrained_reference(post, p, kind, thetas, params, con)
        refg = constrained_reference(post, p, kind, thetas, params, con, grad=True)
        if constrained_ok(ref, refg):
            return con, ref, refg
    raise AssertionError("m = %d, %s: no constraints meet the input conditions" % (m, kind))


# ---- sample paths and the selection
def path_thetas(m, kind):
    """(theta (S_PATHS, theta_dim), params): one parameter row per path, from the utility's support.  The selection entry points take
    rosenbrock at an odd m as well (h = m >> 1 pairs, the last output unread, as oracle.cpu_ref.utility_eval): fixed parameters there."""
    thetas, params = support(m, kind) if kind in utilities(m) else (np.array([[0.3], [0.5]]), None)
    return np.concatenate([thetas, thetas[::-1] + 0.1, thetas[:1] - 0.1])[:S_PATHS], params


def path_seed(m):
    return 700 + m


@functools.lru_cache(maxsize=None)
def paths(m):
    """The S_PATHS sample paths of the oracle's fit from the draws of seed path_seed(m), in multi_outputGP.draw_paths' order."""
    p, _, ref = oracle(m)
    return PTH.Paths(ref, [y[:, None] for y in p["Y"]], *PTH.draw(p["kinds"], N, D, F_PATHS, S_PATHS, np.random.RandomState(path_seed(m))))


def path_rows():
    return np.arange(NGRAD) % S_PATHS


def path_utility_from(F, G, kind, th, params):
    """bocf_path_utility from path values F (m, n >= NGRAD, S_PATHS) and their input gradients G (m, NGRAD, S_PATHS, d): candidate i on
    path i mod S_PATHS -> (u (NGRAD,), du/dx (NGRAD, d), amp)."""
    rows = path_rows()
    ar = np.arange(NGRAD)
    y = F[:, ar, rows]                                                      # (m, NGRAD)
    u = np.array([R.utility_eval(kind, th[rows[i]], y[:, i], params) for i in ar])
    dU = np.stack([R.utility_grad(kind, th[rows[i]], y[:, i], params) for i in ar], 1)       # (m, NGRAD)
    return u, np.einsum("ji,jiq->iq", dU, G[:, ar, rows, :]), path_utility_amp(dU)


def path_utility_amp(dU):
    """The factor on the path-utility gates.  The path values carry an error of at most PATH_VALUE_SCALE max sigma_f^2 each (their own
    gate), so to first order U(theta, f) carries at most sum_j |dU/dy_j| times that: amp = max(1, max_i sum_j |dU/dy_j|) over the compared
    rows, from the REFERENCE's values alone.  For the two utilities test_path_utility_value_and_gradient gates it is no looser than that
    test's factor: 1 for linear with a unit theta, and for neg_sq_dist sum_j 2 |y_j - theta_j| <= 2 m max(1, max |theta| + 3).  The same factor
    stands on the gradient gate (PATH_VALUE_SCALE max sigma_f^2 / min l), as there."""
    return max(1.0, float(np.abs(dU).sum(0).max()))


def selection_values(F, kind, th, params, k=K_SELECT):
    """(S_PATHS, k): per path the k largest U(theta_s, F[:, c, s]) over the candidates, descending -- what bocf_thompson_select returns for
    ANY sample block F (joint posterior samples or path values)."""
    return np.stack([np.sort(R.utility_eval(kind, th[s], F[:, :, s], params))[::-1][:k] for s in range(F.shape[2])])


# ---- the LDS-table limits of kg.hip and pending.hip (64 KiB), for the closed-form neg_sq_dist case (theta_dim = m)
TABLE_LIMIT = 65536
KG_LIMIT_CASES = [(16, 252), (16, 253), (8, 507), (8, 508)]          # (m, reference points): either side of the limit, at the run-time and at a templated m
PENDING_LIMIT_CASES = [(16, 6), (16, 7), (8, 14), (8, 15)]           # (m, pending points)


def kg_table_bytes(m, na, S_mc=0):
    """kg_table_bytes of kg.hip: 8 (2 m na + Sf m + L theta_dim + 2 L + [m S in the Monte-Carlo mode] + BOCF_MAX_M)."""
    return 8 * (2 * m * na + SF * m + L * m + 2 * L + m * S_mc + 16)


def pending_table_bytes(m, r):
    """pending_table_bytes of pending.hip: 8 (m r S + m S + L S + L theta_dim + L + BOCF_MAX_M)."""
    return 8 * (m * r * S + m * S + L * S + L * m + L + 16)


def kg_limit_points(na):
    return np.random.RandomState(na).uniform(size=(na, D))


def pending_limit_inputs(m, r):
    """The pending case of a table-limit test: r points among the evaluated ones ([0, 0.7]^3, as the later draws of pending_inputs)."""
    inp = dict(pending_inputs(m, "neg_sq_dist"))
    rng = np.random.RandomState(40 + r)
    inp["P"], inp["Zp"] = 0.7 * rng.uniform(size=(r, D)), rng.normal(size=(S, m, r))
    return inp
