"""The output-count sweep of tests/test_gpu_output_counts.py is not vacuous: on the oracle alone, for every m = 1 ... 16, every output j
moves every quantity the sweep compares by more than the sweep's gate at some candidate the sweep keeps (so a kernel that dropped,
duplicated or mis-indexed an output could not pass), exchanging two neighbouring outputs while their utility parameters and normals stay
in place does the same (so a wrong stride between mean[j * ld + c] and theta[j] could not pass), and the inputs of
tests/outputs_problem.py meet the conditions stated there: a quarter of the candidates with a value well above the absolute tolerance,
every gradient coordinate well above its own, at most 5 % of the gradient candidates left out near a tie or a threshold.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_ref as K  # noqa: E402
import outputs_problem as P  # noqa: E402
import pending_ref as PR  # noqa: E402

from oracle import cpu_ref as R  # noqa: E402

NG = 4                                                  # candidates of the look-ahead restatements and of the constrained gradient here: a subset of the
                                                        # sweep's -- a move among them is a move among all


class _Memo(K.LookAhead):
    """A LookAhead that computes each posterior quantity of a point set once: the restatements of one output count ask for the same
    means, variances, covariances and their gradients for every utility and every perturbed normal."""

    def __init__(self, fits):
        K.LookAhead.__init__(self, fits)
        self._memo = {}

    def _once(self, name, *args):
        key = (name,) + tuple(np.atleast_2d(a).tobytes() for a in args)
        if key not in self._memo:
            self._memo[key] = getattr(K.LookAhead, name)(self, *args)
        return self._memo[key]

    def mean(self, P_):
        return self._once("mean", P_)

    def var_raw(self, P_):
        return self._once("var_raw", P_)

    def cov(self, X1, X2):
        return self._once("cov", X1, X2)

    def var_grad(self, P_):
        return self._once("var_grad", P_)

    def cov_grad(self, Xc, A):
        return self._once("cov_grad", Xc, A)


def _moved(got, base, rtol, atol):
    """Some entry differs by more than the gate np.testing.assert_allclose(got, base, rtol, atol) applies."""
    return bool(np.any(np.abs(got - base) > atol + rtol * np.abs(base)))


# ---- the quantities of the sweep from posterior arrays: name -> (value, rtol, atol)
def _array_quantities(m, post, W=None):
    p = P.problem(m)
    W = p["W"] if W is None else W
    out = {}
    thetas, _ = P.support(m, "linear")
    for acq in ("EI", "PI"):
        out["ma" + acq] = (P.ma_values(post, thetas, P.PROB, acq),) + P.ACQ_VALUE
        out["d ma" + acq] = (P.ma_grad(post, thetas, P.PROB, acq)[1],) + P.ACQ_GRAD
    for kind in P.utilities(m):
        thetas, params = P.support(m, kind)
        for acq in ("EI", "PI"):
            out["u%s %s" % (acq, kind)] = (P.mc_values(post, W, kind, thetas, P.PROB, params, acq),) + P.MC_VALUE
        a, da, _, _ = P.mc_grad_vec(post, W, kind, thetas, P.PROB, params)
        out["uEI with gradient " + kind] = (a,) + P.ACQ_VALUE
        out["d uEI " + kind] = (da,) + P.ACQ_GRAD
        con, cref, crefg = P.constrained_case(m, kind)
        best = cref["best"], cref["n_feasible"]          # (the incumbent comes from the evaluated points)
        out["constrained " + kind] = (P.constrained_reference(post, p, kind, thetas, params, con, best=best, W=W)["alpha"],) + P.CON_VALUE
        top = np.argsort(-crefg["alpha"], kind="stable")[:NG]               # the gradient candidates of the sweep with the largest values
        sub = {k: (v[:, top] if k != "mu_eval" else v) for k, v in post.items() if k != "var0"}
        g = P.constrained_reference(sub, p, kind, thetas, params, con, grad=True, best=best, W=W, n=NG)["dalpha"]
        out["d constrained " + kind] = (g, P.CON_GRAD_RTOL, P.CON_GRAD_ATOL * max(1.0, np.abs(crefg["dalpha"]).max()))
    return out


def _eu_quantities(m, post, base=None):
    """The expected utilities; their absolute gates scale with the UNPERTURBED reference (`base`: its quantities)."""
    p = P.problem(m)
    out = {}
    for mode, kind in P.eu_cases(m):
        thetas, params = P.support(m, kind)
        v, g = P.expected_utility(post, mode, kind, thetas, p["rows"], p["Zeu"], params)
        names = "EU %s %s" % (mode, kind), "d EU %s %s" % (mode, kind)
        sv, sg = (np.abs(v).max(), np.abs(g).max()) if base is None else (np.abs(base[names[0]][0]).max(), np.abs(base[names[1]][0]).max())
        out[names[0]] = (v, P.EU_RTOL, P.EU_ATOL_SCALE * sv)
        out[names[1]] = (g, P.EU_RTOL, P.EU_ATOL_SCALE * sg)
    return out


def _lookahead_quantities(m, la, Zf, W, zero=None):
    """KG (every admitted mode and utility, values and gradients, on the first NG candidates) and the pending-point acquisition (every
    utility, values and gradients, on the NG gradient candidates of the sweep with the largest values).  zero: the output whose normals
    are set to zero in the pending inputs."""
    p = P.problem(m)
    out = {}
    for mode, kind in P.kg_cases(m):
        thetas, params = P.support(m, kind)
        r = P.kg_reference([la], p, mode, kind, thetas, params, grad=True, n=NG, Zf=Zf, W=W)
        out["KG %s %s" % (mode, kind)] = (r["kg"], P.KG_RTOL, P.KG_ATOL_SCALE * r["vscale"])
        out["d KG %s %s" % (mode, kind)] = (r["dkg"], P.KG_RTOL, P.KG_ATOL_SCALE * np.abs(r["dkg"]).max())
    for kind in P.utilities(m):
        inp = dict(P.pending_case(m, kind)[0], W=W)
        if zero is not None:
            inp["Zp"] = inp["Zp"].copy()
            inp["Zp"][:, zero, :] = 0.0
        best = PR.best_so_far(P.oracle(m)[1], inp["thetas"], kind, inp["params"])           # (the incumbent comes from the evaluated points)
        top = np.argsort(-P.pending_case(m, kind)[2]["alpha"], kind="stable")[:NG]           # the gradient candidates with the largest values
        r = PR.pending(la, inp["Xc"][:P.NGRAD][top], inp["P"], inp["Zp"], W, inp["thetas"], inp["prob"], kind, inp["params"], best=best, grad=True)
        out["pending " + kind] = (r["alpha"], P.PEND_RTOL, P.PEND_ATOL_SCALE * r["scale"])
        out["d pending " + kind] = (r["dalpha"], P.PEND_RTOL, P.PEND_ATOL_SCALE * max(np.abs(r["dalpha"]).max(), 1e-300))
    return out


def _path_quantities(m, F, G, base=None):
    """What test_thompson_and_pathwise_selection compares, from a sample block F (m, C, S_PATHS) and its input gradients G (m, NGRAD,
    S_PATHS, d): the values themselves, and for every utility (rosenbrock at an odd m included) the k selected values of every path --
    bocf_thompson_select ranks any sample block, joint posterior samples and path values alike, so one block stands for both -- and
    bocf_path_utility with its gradient.  The path-utility gates take their factor from the UNPERTURBED block (`base`)."""
    p = P.problem(m)
    vgate = P.PATH_VALUE_SCALE * p["var"].max()
    out = {"path values": (F, 0.0, vgate)}
    for kind in P.UTILS:
        th, params = P.path_thetas(m, kind)
        out["selection " + kind] = (P.selection_values(F, kind, th, params),) + P.SELECT_VALUE
        u, du, amp = P.path_utility_from(F, G, kind, th, params)
        if base is not None:
            amp = base["path utility " + kind][2] / vgate
        out["path utility " + kind] = (u, 0.0, vgate * amp)
        out["d path utility " + kind] = (du, 0.0, vgate / p["ls"].min() * amp)
    return out


def _unread_by_rosenbrock(m, outputs):
    """The path quantities that must NOT move when only `outputs` change: rosenbrock reads y_0 ... y_{2h - 1}, h = m >> 1 -- at an odd m the
    last output is unread by design (at m = 1 it is the constant 0)."""
    if m % 2 == 0 or any(j < m - 1 for j in outputs):
        return ()
    return ("selection rosenbrock", "path utility rosenbrock", "d path utility rosenbrock")


def _assert_paths_moved(m, what, base, got, outputs):
    still = _unread_by_rosenbrock(m, outputs)
    _assert_all_moved(m, what, base, got, skip=still)
    for name in still:
        np.testing.assert_array_equal(got[name][0], base[name][0], err_msg="m = %d, %s: %s reads the last output" % (m, what, name))


def _assert_all_moved(m, what, base, got, skip=()):
    for name, (b, rtol, atol) in base.items():
        if name in skip:
            continue
        assert _moved(got[name][0], b, rtol, atol), "m = %d, %s: %s does not move beyond its gate" % (m, what, name)


# ---- the restatements this file and the sweep lean on
@pytest.mark.parametrize("m", [1, 4, 9, 16])
def test_vectorised_restatements_equal_the_oracles(m):
    p, post = P.problem(m), P.posterior(m)
    rng = np.random.RandomState(m)
    for kind in P.utilities(m):
        thetas, params = P.support(m, kind)
        y = rng.normal(size=(m, 5))
        want = np.stack([R.utility_grad(kind, thetas[0], y[:, i], params) for i in range(5)], 1)
        np.testing.assert_allclose(P.utility_grad_vec(kind, thetas[0], y, params), want, rtol=1e-14, atol=1e-15)
        a, da, _, _ = P.mc_grad_vec(post, p["W"], kind, thetas, P.PROB, params)
        ra, rda = R.mc_acq_with_gradient(post["mean"][:, :P.NGRAD], post["sigma"][:, :P.NGRAD], post["dmean"], post["dvar"], post["mu_eval"], p["W"],
                                         kind, thetas, P.PROB, params)
        np.testing.assert_allclose(a, ra[:, 0], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(da, rda, rtol=1e-11, atol=1e-14)
    # the expected utility under the noiseless posterior: the gradient against central differences of the value along the posterior's own path
    la = P.oracle(m)[1]
    h, X = 1e-6, p["Xc"][:P.NGRAD]
    for mode, kind in P.eu_cases(m):
        thetas, params = P.support(m, kind)
        _, g = P.expected_utility(post, mode, kind, thetas, p["rows"], p["Zeu"], params, n=P.NGRAD)
        for q in range(P.D):
            e = np.zeros(P.D)
            e[q] = h
            vp = P.expected_utility(P.posterior_of(la, X + e, grad=False), mode, kind, thetas, p["rows"], p["Zeu"], params, n=P.NGRAD, grad=False)
            vm = P.expected_utility(P.posterior_of(la, X - e, grad=False), mode, kind, thetas, p["rows"], p["Zeu"], params, n=P.NGRAD, grad=False)
            np.testing.assert_allclose(g[:, q], (vp - vm) / (2 * h), rtol=2e-4, atol=2e-5 * np.abs(g).max(), err_msg="%s %s coordinate %d" % (mode, kind, q))


# ---- input conditions
@pytest.mark.parametrize("m", P.MS)
def test_input_conditions(m):
    p, la, _ = P.oracle(m)
    post = P.posterior(m)
    for kind in P.utilities(m):
        thetas, params = P.support(m, kind)
        assert thetas.shape[0] == P.L
        assert P.accepts(m, kind, thetas, params)
        ei, pi = (P.mc_values(post, p["W"], kind, thetas, P.PROB, params, a) for a in ("EI", "PI"))
        a, da, gap, scale = P.mc_grad_vec(post, p["W"], kind, thetas, P.PROB, params)
        assert P.share(ei, P.MC_VALUE[1]) >= P.NONZERO_SHARE and P.share(pi, P.MC_VALUE[1]) >= P.NONZERO_SHARE
        assert P.every_coordinate(da, P.ACQ_GRAD[1]) and gap.min() >= P.MC_HINGE and np.mean(gap < P.PEND_NEAR * scale) <= P.LEFT_OUT
        inp, ref, refg = P.pending_case(m, kind)
        assert P.pending_ok(ref, refg) and ref["cond"] <= 1e4
        con, cref, crefg = P.constrained_case(m, kind)
        assert P.constrained_ok(cref, crefg) and 0 < cref["n_feasible"] < P.N
        print("m %2d %-12s share > 1e3 atol: uEI %.2f uPI %.2f pending %.2f constrained %.2f; smallest hinge gap %.2g; pending near a threshold %.3f"
              % (m, kind, P.share(ei, P.MC_VALUE[1]), P.share(pi, P.MC_VALUE[1]), P.share(ref["alpha"], P.PEND_ATOL_SCALE * ref["scale"]),
                 P.share(cref["alpha"], P.CON_VALUE[1]), gap.min(), np.mean(refg["gap"] < P.PEND_NEAR * refg["scale"])))
    thetas, _ = P.support(m, "linear")
    for acq in ("EI", "PI"):
        assert P.share(P.ma_values(post, thetas, P.PROB, acq), P.ACQ_VALUE[1]) >= P.NONZERO_SHARE
        assert P.every_coordinate(P.ma_grad(post, thetas, P.PROB, acq)[1], P.ACQ_GRAD[1])
    if m > 1:                                            # distinct per output: parameters, variances, lengthscales
        for kind in ("linear", "neg_sq_dist"):
            th = P.support(m, kind)[0]
            assert all(len(set(np.round(row, 12))) == m for row in th)
        assert len(set(P.support(m, "neg_exp_cos")[1])) == m and len(set(p["var"])) == m and len(set(map(tuple, p["ls"]))) == m
    for mode, kind in P.kg_cases(m):                     # the near-tie rule of test_kg_gradients leaves out at most 5 %
        thetas, params = P.support(m, kind)
        r = P.kg_reference([la], p, mode, kind, thetas, params, grad=True, n=P.NGRAD)
        keep = r["gap"] >= P.KG_TIE * np.max(np.abs(r["kg"]))
        assert np.mean(~keep) <= P.LEFT_OUT, (mode, kind)
        assert P.every_coordinate(r["dkg"][keep], P.KG_ATOL_SCALE * np.abs(r["dkg"]).max())


def test_input_conditions_of_the_table_limit_cases():
    """Either side of the LDS-table limits, at the run-time m = 16 and at the templated m = 8: the sizes fall where the GPU tests say, and
    the reference points and pending sets meet the left-out cap."""
    for (m, lo), (m2, hi) in zip(P.KG_LIMIT_CASES[::2], P.KG_LIMIT_CASES[1::2]):
        assert m == m2 and hi == lo + 1 and P.kg_table_bytes(m, lo) <= P.TABLE_LIMIT < P.kg_table_bytes(m, hi)
    for (m, lo), (m2, hi) in zip(P.PENDING_LIMIT_CASES[::2], P.PENDING_LIMIT_CASES[1::2]):
        assert m == m2 and hi == lo + 1 and P.pending_table_bytes(m, lo) <= P.TABLE_LIMIT < P.pending_table_bytes(m, hi)
    for m, na in P.KG_LIMIT_CASES:
        p, la, _ = P.oracle(m)
        thetas, params = P.support(m, "neg_sq_dist")
        r = P.kg_reference([la], p, "closed", "neg_sq_dist", thetas, params, grad=True, n=P.NGRAD, A=P.kg_limit_points(na))
        assert np.mean(r["gap"] < P.KG_TIE * np.max(np.abs(r["kg"]))) <= P.LEFT_OUT
    for m, r_ in P.PENDING_LIMIT_CASES:
        refg = PR.case_reference(P.pending_limit_inputs(m, r_), [P.oracle(m)[1]], grad=True, n=P.NGRAD)
        assert np.mean(refg["gap"] < P.PEND_NEAR * refg["scale"]) <= P.LEFT_OUT and refg["alpha"].max() > 1e3 * P.PEND_ATOL_SCALE * refg["scale"]
        assert refg["cond"] <= 1e4


# ---- sensitivity
@pytest.mark.parametrize("m", P.MS)
def test_every_output_moves_every_comparison(m):
    """Output j alone -- its posterior mean shifted by 0.1 sigma_j, its input gradients scaled by 1.1 and column j of the Monte-Carlo
    normals set to zero for the quantities computed from posterior arrays (a shift alone need not flip one of the 65 indicator samples of
    uPI), column j of every normal set to zero for the look-ahead quantities (KG, pending), output j of the sample block shifted by 0.1
    sigma_j and its input gradients scaled by 1.1 for the path and selection quantities -- moves every compared quantity beyond its gate
    at some kept candidate.  The one exception is asserted as such: rosenbrock at an odd m does not read the last output."""
    p, la, _ = P.oracle(m)
    la = _Memo(la.fits)
    post = P.posterior(m)
    base = _array_quantities(m, post)
    base_eu = _eu_quantities(m, post)
    base_la = _lookahead_quantities(m, la, p["Zf"], p["W"])
    Fp, Gp = P.paths(m).values(p["Xc"]), P.paths(m).gradients(p["Xc"][:P.NGRAD])
    base_p = _path_quantities(m, Fp, Gp)
    for j in range(m):
        F2, G2 = Fp.copy(), Gp.copy()
        F2[j] += 0.1 * post["sigma"][j][:, None]
        G2[j] *= 1.1
        _assert_paths_moved(m, "output %d of the sample block shifted" % j, base_p, _path_quantities(m, F2, G2, base_p), [j])
        sh = P.shifted(post, j)
        Zf, W = p["Zf"].copy(), p["W"].copy()
        Zf[:, j], W[:, j] = 0.0, 0.0
        _assert_all_moved(m, "output %d shifted" % j, base, _array_quantities(m, sh, W))
        _assert_all_moved(m, "output %d shifted" % j, base_eu, _eu_quantities(m, sh, base_eu))
        _assert_all_moved(m, "normals of output %d zeroed" % j, base_la, _lookahead_quantities(m, la, Zf, W, zero=j))


# ---- output order
def _symmetric(m, j):
    """Quantities that do not change when outputs j and j + 1 trade places although nothing else does: closed forms without a per-output
    parameter (neg_sum_exp; rosenbrock unless the pair straddles its two halves) -- a kernel that exchanged them would be right too."""
    out = {"EU closed neg_sum_exp", "d EU closed neg_sum_exp"}
    if j + 1 != m // 2:
        out |= {"EU closed rosenbrock", "d EU closed rosenbrock"}
    return out


def _symmetric_paths(m, j):
    """Path quantities that do not change when outputs j and j + 1 of the sample block trade places: neg_sum_exp has no per-output
    parameter and no per-output normal here (U is symmetric in y), rosenbrock is symmetric inside each of its halves; the gradient of
    rosenbrock pairs dU/dy_j with df_j/dx and is symmetric likewise."""
    out = {"selection neg_sum_exp", "path utility neg_sum_exp", "d path utility neg_sum_exp"}
    h = m // 2
    if j + 1 != h and j + 1 < 2 * h:                     # both inside one half (a pair that takes in the unread last output does move)
        out |= {"selection rosenbrock", "path utility rosenbrock", "d path utility rosenbrock"}
    return out


@pytest.mark.parametrize("m", P.MS[1:])
def test_output_order_moves_every_comparison(m):
    """Outputs j and j + 1 exchanged in everything the model hands over, utility parameters and normals left in place."""
    p, la, _ = P.oracle(m)
    post = P.posterior(m)
    base = _array_quantities(m, post)
    base_eu = _eu_quantities(m, post)
    base_la = _lookahead_quantities(m, la, p["Zf"], p["W"])
    Fp, Gp = P.paths(m).values(p["Xc"]), P.paths(m).gradients(p["Xc"][:P.NGRAD])
    base_p = _path_quantities(m, Fp, Gp)
    for j in range(m - 1):
        F2, G2 = Fp.copy(), Gp.copy()
        F2[[j, j + 1]], G2[[j, j + 1]] = Fp[[j + 1, j]], Gp[[j + 1, j]]
        _assert_all_moved(m, "outputs %d and %d of the sample block exchanged" % (j, j + 1), base_p, _path_quantities(m, F2, G2, base_p),
                          skip=_symmetric_paths(m, j))
        sw = P.swapped(post, j)
        _assert_all_moved(m, "outputs %d and %d exchanged" % (j, j + 1), base, _array_quantities(m, sw))
        _assert_all_moved(m, "outputs %d and %d exchanged" % (j, j + 1), base_eu, _eu_quantities(m, sw, base_eu), skip=_symmetric(m, j))
        fits = list(la.fits)
        fits[j], fits[j + 1] = fits[j + 1], fits[j]
        _assert_all_moved(m, "outputs %d and %d exchanged" % (j, j + 1), base_la, _lookahead_quantities(m, _Memo(fits), p["Zf"], p["W"]))


# ---- rosenbrock
@pytest.mark.parametrize("m", [2, 4, 8, 16])
def test_rosenbrock_reference_reads_every_output_at_even_counts(m):
    """h = m / 2: U = -sum_{j < h} (a - y_j)^2 + 100 y_{j + h}^2 -- every one of y_0 ... y_{m - 1} moves the value and carries a gradient."""
    rng = np.random.RandomState(m)
    y, a = rng.uniform(0.2, 1.0, size=m), np.array([0.7])
    h = m // 2
    u = R.utility_eval("rosenbrock", a, y)
    assert np.isclose(u, -sum((a[0] - y[j]) ** 2 + 100.0 * y[j + h] ** 2 for j in range(h)), rtol=1e-14)
    g = R.utility_grad("rosenbrock", a, y)
    for k in range(m):
        y2 = y.copy()
        y2[k] += 0.1
        assert abs(R.utility_eval("rosenbrock", a, y2) - u) > 1e-3 and g[k] != 0.0, k
    np.testing.assert_allclose(P.utility_grad_vec("rosenbrock", a, y[:, None])[:, 0], g, rtol=1e-15)


@pytest.mark.parametrize("m", [1, 9, 15])
def test_rosenbrock_reference_at_odd_counts_leaves_the_last_output_unread(m):
    """What the selection entry points (which take rosenbrock at any m) are compared with: h = (m - 1) / 2 pairs."""
    y, a = np.random.RandomState(m).uniform(0.2, 1.0, size=m), np.array([0.7])
    y2 = y.copy()
    y2[-1] += 1.0
    assert R.utility_eval("rosenbrock", a, y2) == R.utility_eval("rosenbrock", a, y)
    assert R.utility_eval("rosenbrock", a, y) == R.utility_eval("rosenbrock", a, y[:m - 1]) if m > 1 else R.utility_eval("rosenbrock", a, y) == 0
