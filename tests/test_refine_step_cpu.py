"""CPU-only checks of the anchor refinement's state machine (bocf_amd/csrc/refine_step.h) and of its Python
surface.  The header is driven through tests/refine_step_driver.cpp -- built once as it is and once with AddressSanitizer and
UndefinedBehaviorSanitizer, every driver test runs against both -- and compared with lbfgsb_batched_numpy, the NumPy statement of the
algorithm, on the same analytic objectives.  The tolerances are those of the project's comparison of the C++ routine with that
statement (tests/test_optimizer_cpu.py): X to 1e-6, F to rtol 1e-10 / atol 1e-12, equal iteration and evaluation counts per row when a
count cuts the run, iterations within 3 otherwise.  The stepwise machine does not wait for the slowest line search, so the counts
compared are per row, never passes."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_cases as C  # noqa: E402
from refine_cases import FACTR, MAXITER, NAN_GRADIENT, NONFINITE_START, PGTOL, poly_f_df, qsin_problem, run_driver  # noqa: E402

from bocf_amd import acquisition_optimizer as AO  # noqa: E402

ROOT = C.ROOT
SETTINGS = C.SETTINGS + [dict(m=1), dict(maxiter=0)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    if not os.path.exists(C.CLANG):
        pytest.skip("no clang++ next to hipcc")
    return C.build_driver(tmp_path_factory.mktemp("refine_step"), sanitized=request.param == "sanitized")


def numpy_reference(f_df, X0, bounds, **kw):
    return C.host_reference(f_df, X0, bounds, **kw)


def compare(got, ref, cut):
    C.compare(got, ref, cut)
    assert got["frozen"] == 1


@pytest.mark.parametrize("boxed", [True, False])
@pytest.mark.parametrize("d", [6, 1, 32])
def test_quadratic_plus_sine_equals_numpy_statement(driver, boxed, d):
    f_df, numbers, rng = qsin_problem(d)
    bounds = [(0.0, 1.0)] * d if boxed else [(-np.inf, np.inf)] * d
    X0 = rng.uniform(size=(16, d))
    for kw in SETTINGS:
        got = run_driver(driver, "qsin", X0, bounds, numbers, **kw)
        compare(got, numpy_reference(f_df, X0, bounds, **kw), cut="maxfun" in kw or "maxiter" in kw)
        if boxed:
            assert np.all(got["X"] >= 0.0) and np.all(got["X"] <= 1.0)
        if kw.get("maxiter") == 0:                         # the clamped starts, evaluated once
            assert np.array_equal(got["X"], np.clip(X0, *zip(*bounds)) if boxed else X0)
            assert np.all(got["evaluations"] == 1) and np.all(got["reasons"] == MAXITER) and got["passes"] == 1


@pytest.mark.parametrize("boxed", [True, False])
@pytest.mark.parametrize("d", [6, 1, 32])
def test_polynomial_equals_numpy_statement(driver, boxed, d):
    X0, bounds = C.poly_problem(d, boxed)
    for kw in SETTINGS:
        got = run_driver(driver, "poly", X0, bounds, **kw)
        compare(got, numpy_reference(poly_f_df, X0, bounds, **kw), cut="maxfun" in kw or "maxiter" in kw)


def test_optimal_start_is_evaluated_once(driver):
    got = run_driver(driver, "sq", [[0.9, 0.1], [0.25, 0.25], [0.0, 1.0]], [(0, 1)] * 2, [0.25])
    assert np.allclose(got["X"], 0.25, atol=1e-6) and np.allclose(got["F"], 0.0, atol=1e-10)
    assert got["evaluations"][1] == 1 and got["reasons"][1] == PGTOL and got["iterations"][1] == 0
    assert got["frozen"] == 1


def test_start_on_a_bound_with_the_gradient_pushing_outwards(driver):
    # the minimum of sum (x - 1.5)^2 over [0, 1]^2 is the corner (1, 1); row 0 starts there, row 1 has one coordinate held from the start
    f_df = lambda X: (((X - 1.5) ** 2).sum(1), 2 * (X - 1.5))
    X0 = [[1.0, 1.0], [1.0, 0.2]]
    got = run_driver(driver, "sq", X0, [(0, 1)] * 2, [1.5])
    assert got["evaluations"][0] == 1 and got["reasons"][0] == PGTOL and np.array_equal(got["X"][0], [1.0, 1.0])
    compare(got, numpy_reference(f_df, X0, [(0, 1)] * 2), cut=False)
    assert np.array_equal(got["X"][1], [1.0, 1.0])


def test_infinite_beyond_a_plane(driver):
    def f_inf(X):
        return np.where(X[:, 0] > 0.5, np.inf, ((X - 0.2) ** 2).sum(1)), 2 * (X - 0.2)
    X0 = [[0.4, 0.4], [0.7, 0.7]]
    got = run_driver(driver, "sqinf", X0, [(0, 1)] * 2, [0.2])
    assert np.allclose(got["X"][0], 0.2, atol=1e-6)
    assert np.array_equal(got["X"][1], [0.7, 0.7]) and np.isinf(got["F"][1]) and got["reasons"][1] == NONFINITE_START and got["evaluations"][1] == 1
    compare(got, numpy_reference(f_inf, X0, [(0, 1)] * 2), cut=False)
    # trial points beyond the plane are rejected, not accepted: started close to it and pulled across (minimum at 0.9), the row stays below
    f_far = lambda X: (np.where(X[:, 0] > 0.5, np.inf, ((X - 0.9) ** 2).sum(1)), 2 * (X - 0.9))
    got = run_driver(driver, "sqinf", [[0.45, 0.3]], [(0, 1)] * 2, [0.9])
    assert got["X"][0, 0] <= 0.5 and np.isfinite(got["F"][0]) and got["evaluations"][0] > got["iterations"][0] + 1
    compare(got, numpy_reference(f_far, [[0.45, 0.3]], [(0, 1)] * 2), cut=False)


def test_nan_gradient_ends_the_row(driver):
    got = run_driver(driver, "sqnan", [[0.1, 0.4], [0.9, 0.9]], [(0, 1)] * 2, [0.6])
    assert got["reasons"][0] == NAN_GRADIENT and got["evaluations"][0] == 1 and np.array_equal(got["X"][0], [0.1, 0.4])
    assert np.allclose(got["X"][1], 0.6, atol=1e-6) and got["reasons"][1] in (PGTOL, FACTR)
    assert got["frozen"] == 1


def test_frozen_rows_stay_byte_identical(driver):
    f_df, numbers, rng = qsin_problem(4)
    X0 = rng.uniform(size=(5, 4))
    for kw in (dict(), dict(maxfun=3), dict(maxiter=0)):
        assert run_driver(driver, "qsin", X0, [(0.0, 1.0)] * 4, numbers, extra=25, **kw)["frozen"] == 1


def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    assert re.search(r"\bint\s+bocf_refine_acq\s*\(\s*bocf_ctx\s*\*", header)
    assert "BOCF_REFINE_LINEAR" in header and "BOCF_REFINE_MC" in header
    from bocf_amd import _ffi
    assert "bocf_refine_acq" in _ffi.SIGNATURES
    lib = _ffi.load()
    assert hasattr(lib, "bocf_refine_acq")
    step = open(os.path.join(ROOT, "bocf_amd", "csrc", "refine_step.h")).read()
    assert "hip/hip_runtime.h" not in step and "fp contract(off)" in step


def test_probes_hook_is_in_the_probes_library_only_and_bound_as_defined():
    """The hook that runs refine_advance_kernel on the polynomial is no launcher probe (tests/test_host_cpu.py counts those by their
    bocf_probe_ prefix): the same three statements for it -- the binding knows exactly the hooks the source defines under BOCF_PROBES,
    the header declares none, the product library exports none and the probes library all."""
    from bocf_amd import _ffi
    src = open(os.path.join(ROOT, "bocf_amd", "csrc", "capi_probe.hip")).read()
    assert src.lstrip().split("\n")[0].startswith("//") and "#ifdef BOCF_PROBES" in src.split("#include")[0]    # the whole file is probes-only
    defined = set(re.findall(r"^int (bocf_refine_probe_[a-z0-9_]+)\(", src, re.M))
    assert defined == {"bocf_refine_probe_poly"} == set(_ffi.HOOK_SIGNATURES)
    assert not defined & set(_ffi.SIGNATURES) and not defined & set(_ffi.PROBE_SIGNATURES)
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    for name in defined:
        assert name not in header and not hasattr(lib, name), name
    with open(_ffi.LIB_PATH, "rb") as f:
        assert b"bocf_refine_probe_" not in f.read()
    with _ffi.probes_library() as plib:
        for name in defined:
            assert getattr(plib, name) is not None, name


def test_unscaled_d32_problem_under_the_cut_settings_and_the_reference_pair_beyond_them(driver):
    """The quadratic-plus-sine exactly as test_native_batched_lbfgs_equals_numpy_statement builds it (no 6 / d), at d = 32.  Cut by a
    count the runs are short and the counts must be equal: asserted.  Under the settings that run to convergence the project's own pair
    -- bocf_lbfgsb_batched against the NumPy statement -- is printed with the driver's figures, as the record of why
    test_quadratic_plus_sine_equals_numpy_statement scales the problem (refine_cases.qsin_problem)."""
    for boxed in (True, False):
        f_df, numbers, rng = qsin_problem(32, scaled=False)
        bounds = [(0.0, 1.0)] * 32 if boxed else [(-np.inf, np.inf)] * 32
        X0 = rng.uniform(size=(16, 32))
        for kw in (dict(maxfun=7), dict(maxiter=3), dict(maxiter=0)):
            compare(run_driver(driver, "qsin", X0, bounds, numbers, **kw), numpy_reference(f_df, X0, bounds, **kw), cut=True)
        for kw in (dict(), dict(factr=1e1, pgtol=1e-10), dict(m=1)):
            ref = numpy_reference(f_df, X0, bounds, **kw)
            cxx = C.host_reference(f_df, X0, bounds, loop=AO.lbfgsb_batched, **kw)
            got = run_driver(driver, "qsin", X0, bounds, numbers, **kw)
            print("unscaled d 32 boxed %s %s (at most %d iterations): against the NumPy statement, iterations differ by up to %d (C++ routine) / %d "
                  "(state machine), X by %.3g / %.3g" % (boxed, kw, ref["iterations"].max(), np.abs(cxx["iterations"] - ref["iterations"]).max(),
                                                        np.abs(got["iterations"] - ref["iterations"]).max(), np.abs(cxx["X"] - ref["X"]).max(),
                                                        np.abs(got["X"] - ref["X"]).max()))
            assert got["frozen"] == 1 and np.all(got["reasons"] != 0)
            np.testing.assert_allclose(got["F"], ref["F"], rtol=1e-6, atol=1e-9)     # (the same optimum; not the comparison of the scaled problem)


# ---- the Python surface, against a fake model
class FakeModel(object):
    analytical_gradient_prediction = True
    output_dim = 2

    def __init__(self):
        self.calls = []

    def number_of_hyps_samples(self):
        return 1

    def acq_linear(self, *a, **kw):
        raise AssertionError("not reached")

    def refine_acq(self, X0, bounds, **kw):
        self.calls.append(("refine_acq", np.array(X0), list(bounds), kw))
        X0 = np.atleast_2d(X0)
        return X0.copy(), np.zeros(len(X0)), dict(f_df_calls=1, points_evaluated=len(X0), iterations=np.zeros(len(X0), int), host_syncs=2,
                                                  reasons=["maxiter"] * len(X0))


def _utility(full_support=True, device="neg_sq_dist", func=None):
    from bocf_amd.utility import ParameterDistribution, Utility
    support = np.array([[0.1, 0.2], [0.3, 0.4]]) if full_support else np.random.RandomState(0).rand(30, 2)
    dist = ParameterDistribution(support=support, prob_dist=np.full(len(support), 1.0 / len(support)))
    return Utility(func=func, parameter_dist=dist, device=device)


def test_python_surface_default_and_refusals():
    from bocf_amd import acquisitions as ACQ
    space = AO.Design_space(bounds=[(0.0, 1.0)] * 3)
    assert AO.AcquisitionOptimizer(space).refine == "host"
    with pytest.raises(ValueError, match="refine"):
        AO.AcquisitionOptimizer(space, refine="gpu")
    opt = AO.AcquisitionOptimizer(space, refine="device", n_starting=8, n_anchor=2)
    model = FakeModel()
    state = np.random.get_state()
    # 1. the parameter distribution does not have full support
    for cls in (ACQ.maEI, ACQ.uEI_noiseless):
        acq = cls(model, space, optimizer=opt, utility=_utility(full_support=False, device="linear" if cls is ACQ.maEI else "neg_sq_dist"))
        with pytest.raises(NotImplementedError, match="full support"):
            opt.optimize(f=acq.acquisition_function, f_df=acq.acquisition_function_withGradients)
    # 2. the utility is a host callable
    acq = ACQ.uEI_noiseless(model, space, optimizer=opt, utility=_utility(device=None, func=lambda theta, y: -np.sum(np.abs(y - theta) ** 1.5, axis=0)))
    with pytest.raises(NotImplementedError, match="host callable"):
        opt.optimize(f=acq.acquisition_function, f_df=acq.acquisition_function_withGradients)
    # 3. the acquisition is not one of the covered classes (a plain function has no owner at all)
    acq = ACQ.uEI_pending(FakePendingModel(), space, optimizer=opt, utility=_utility())
    with pytest.raises(NotImplementedError, match="does not cover uEI_pending"):
        opt.optimize(f=acq.acquisition_function, f_df=acq.acquisition_function_withGradients)
    with pytest.raises(NotImplementedError, match="cannot call a Python f_df"):
        opt.optimize(f=lambda X: X.sum(1, keepdims=True), f_df=lambda X: (X.sum(1, keepdims=True), np.ones_like(X)))
    assert model.calls == []                               # refused before anything ran
    np.random.set_state(state)


class FakePendingModel(FakeModel):
    def acq_pending(self, *a, **kw):
        raise AssertionError("not reached")


def test_python_surface_passes_the_objective_to_the_model():
    from bocf_amd import _ffi, acquisitions as ACQ
    space = AO.Design_space(bounds=[(0.0, 1.0)] * 3)
    opt = AO.AcquisitionOptimizer(space, refine="device", n_starting=8, n_anchor=2)
    model = FakeModel()
    acq = ACQ.maPI(model, space, optimizer=opt, utility=_utility(device="linear"))
    owner, kw = opt._device_objective(acq.acquisition_function_withGradients)
    assert owner is acq and kw["form"] == _ffi.REFINE_LINEAR and kw["kind"] == _ffi.ACQ_PI and kw["thetas"].shape == (2, 2)
    acq = ACQ.uEI_noiseless(model, space, optimizer=opt, utility=_utility())
    owner, kw = opt._device_objective(acq.acquisition_function_withGradients)
    assert kw["form"] == _ffi.REFINE_MC and kw["util_kind"] == _ffi.UTIL_NEG_SQ_DIST and kw["W"] is acq.W_samples and kw["program"] is None
    info = {}
    X = opt._refine_on_device(np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]]), (owner, kw), info)
    name, X0, bounds, sent = model.calls[0]
    assert name == "refine_acq" and X.shape == (2, 3) and bounds == [(0.0, 1.0)] * 3
    assert sent["maxiter"] == 500 and sent["factr"] == 1e6 and sent["pgtol"] == 1e-5 and sent["form"] == _ffi.REFINE_MC
    assert set(info) >= {"f_df_calls", "points_evaluated", "iterations", "host_syncs"}
