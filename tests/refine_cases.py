"""What the refinement's CPU and GPU tests share (tests/test_refine_step_cpu.py, tests/test_gpu_refine.py): the driver of
bocf_amd/csrc/refine_step.h (tests/refine_step_driver.cpp) built and run, the analytic objectives as NumPy statements, the NumPy
statement of the algorithm with per-row evaluation counts, and the comparison with the project's own tolerances
(tests/test_optimizer_cpu.py: X to 1e-6, F to rtol 1e-10 / atol 1e-12, equal iteration and evaluation counts per row when a count
cuts the run, iterations within 3 otherwise).  Test infrastructure only: nothing under bocf_amd/ imports it."""
import os
import subprocess

import numpy as np

from bocf_amd import acquisition_optimizer as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
PGTOL, FACTR, ARC_FAILED, MAXITER, MAXFUN, NONFINITE_START, NAN_GRADIENT = range(1, 8)
DEFAULTS = dict(maxiter=500, m=10, factr=1e6, pgtol=1e-5, max_ls=20, c1=1e-4, maxfun=None)
SETTINGS = [dict(), dict(maxfun=7), dict(maxiter=3), dict(factr=1e1, pgtol=1e-10)]
CUT = lambda kw: "maxfun" in kw or "maxiter" in kw


def build_driver(directory, sanitized=False):
    exe = os.path.join(str(directory), "refine_step_driver_" + ("sanitized" if sanitized else "plain"))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitized else []
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror"] + extra + [os.path.join(ROOT, "tests", "refine_step_driver.cpp"), "-o", exe])
    return exe


def run_driver(driver, objective, X0, bounds, numbers=(), extra=3, **kw):
    """The driver's rows: X, F, iterations, evaluations, reasons (bit-exact: the doubles travel as hex), passes, frozen."""
    s = dict(DEFAULTS, **kw)
    X0 = np.atleast_2d(np.asarray(X0, dtype=float))
    A, d = X0.shape
    head = [objective, d, s["m"], A, s["maxiter"], s["max_ls"], -1 if s["maxfun"] is None else s["maxfun"], float(s["factr"]).hex(),
            float(s["pgtol"]).hex(), float(s["c1"]).hex(), extra]
    vals = [b[0] for b in bounds] + [b[1] for b in bounds] + list(X0.ravel()) + list(np.asarray(numbers, dtype=float).ravel())
    text = " ".join(str(h) for h in head) + "\n" + " ".join(float(v).hex() for v in vals) + "\n"
    out = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == A + 2
    X, F, it, nf, why = np.empty((A, d)), np.empty(A), np.empty(A, int), np.empty(A, int), np.empty(A, int)
    for a, line in enumerate(lines[:A]):
        xs, f, counts = line.split("|")
        X[a] = [float.fromhex(t) for t in xs.split()]
        F[a] = float.fromhex(f.strip())
        it[a], nf[a], why[a] = (int(t) for t in counts.split())
    assert lines[A].startswith("passes ") and lines[A + 1].startswith("frozen ")
    return dict(X=X, F=F, iterations=it, evaluations=nf, reasons=why, passes=int(lines[A].split()[1]), frozen=int(lines[A + 1].split()[1]))


def host_reference(f_df, X0, bounds, loop=AO.lbfgsb_batched_numpy, **kw):
    """`loop` (lbfgsb_batched_numpy or lbfgsb_batched) on f_df, with per-row evaluation counts (the rows of every f_df call)."""
    nfun = np.zeros(np.atleast_2d(X0).shape[0], dtype=int)

    def counted(Z, rows):
        nfun[rows] += 1
        return f_df(Z)
    info = {}
    X, F = loop(counted, X0, bounds, info=info, with_rows=True, **kw)
    return dict(X=X, F=F, iterations=np.asarray(info["iterations"]), evaluations=nfun, passes=info["f_df_calls"])


def compare(got, ref, cut, what=""):
    """The figures first (run with -s to keep them), then the assertions."""
    with np.errstate(invalid="ignore"):
        dx = np.nanmax(np.abs(got["X"] - ref["X"]))
        df = np.nanmax(np.abs(got["F"] - ref["F"]))
    dit = np.abs(got["iterations"] - ref["iterations"]).max()
    dnf = np.abs(got["evaluations"] - ref["evaluations"]).max()
    print("%s max |dX| %.3g, max |dF| %.3g, iterations differ by <= %d (max %d), evaluations by <= %d (max %d)"
          % (what, dx, df, dit, ref["iterations"].max(), dnf, ref["evaluations"].max()))
    np.testing.assert_allclose(got["X"], ref["X"], rtol=1e-6, atol=1e-6, err_msg=what)
    np.testing.assert_allclose(got["F"], ref["F"], rtol=1e-10, atol=1e-12, err_msg=what)
    if cut:
        assert np.array_equal(got["iterations"], ref["iterations"]), what
        assert np.array_equal(got["evaluations"], ref["evaluations"]), what
    else:
        assert dit <= 3, what
    assert np.all(np.asarray(got["reasons"]) != 0), what


# ---- objectives, as NumPy statements of what the driver evaluates
def qsin_problem(d, seed=3, scaled=True):
    """The quadratic-plus-sine of test_native_batched_lbfgs_equals_numpy_statement; at d = 6 it is that problem to the bit.  The Gram
    term is scaled by 6 / d so that its spectrum (largest eigenvalue about 4 d of an unscaled d x d Gaussian Gram matrix, against the
    0.5 of the shift) keeps the scale of the d = 6 problem the tolerances were taken from: unscaled at d = 32 the condition number is
    several hundred, a run takes a hundred iterations that end in the rounding noise of the relative-decrease test, and the project's own
    C++ routine then differs from the NumPy statement by up to 15 iterations and 1e-4 in X -- no implementation meets a bound of 3 there
    (test_unscaled_d32_problem_under_the_cut_settings_and_the_reference_pair_beyond_them prints those figures and keeps the unscaled
    problem, scaled=False, under the settings a count cuts, where the counts must be equal)."""
    rng = np.random.RandomState(seed)
    Q = rng.randn(d, d)
    Q = Q @ Q.T * (6.0 / d if scaled else 1.0) + 0.5 * np.eye(d)
    c = rng.randn(d)

    def f_df(X):
        Z = X - 0.3
        return 0.5 * np.einsum('ad,de,ae->a', Z, Q, Z) - Z @ c + 0.05 * np.sin(3 * Z).sum(1), Z @ Q - c + 0.15 * np.cos(3 * Z)
    return f_df, np.concatenate([Q.ravel(), c]), rng


def poly_f_df(X):
    """bocf_amd/csrc/refine_poly.h."""
    d = X.shape[1]
    k = np.arange(d)
    U = X - (0.25 * (k % 4) - 0.3)
    a = 1.0 + 0.5 * (k % 3)
    Un, Up = np.roll(U, -1, axis=1), np.roll(U, 1, axis=1)
    return (a * U * U + 0.05 * U * U * U + 0.1 * U * Un).sum(1), 2.0 * a * U + 0.15 * U * U + 0.1 * (Un + Up)


def poly_problem(d, boxed, A=9):
    rng = np.random.RandomState(11)
    bounds = [(-0.5, 0.6)] * d if boxed else [(-np.inf, np.inf)] * d
    return rng.uniform(-1.0, 1.0, size=(A, d)), bounds       # (some starts outside the box: clamped)
