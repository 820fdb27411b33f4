"""CPU checks of the utility programs (bocf_amd/utility_program.py, include/bocf_hip.h): the tracer, its derivative and its encoder
against the callables themselves through the NumPy interpreter of the ENCODED blob, the limits, the round trips, and the host-side
validator bocf_check_utility_program -- what it accepts and every field it rejects."""
import ctypes
import os
import pickle
import re
import struct

import numpy as np
import pytest

import bocf_amd as B
from bocf_amd import utility_program as UP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = np.pi


def _weights(m):
    return [1.0 + 0.25 * j for j in range(m)]


# ---- the five utilities written the way the reference's experiment scripts write them (U and its dfunc), for m outputs
def neg_sq_dist(p, y):                                      # test_1a.py:89-92, test_4a.py:84-87
    aux = (y.transpose() - p).transpose()
    return -np.sum(np.square(aux), axis=0)


def d_neg_sq_dist(p, y):
    return -2 * (np.squeeze(y) - p)


def linear(p, y):                                           # test_1b.py:89-90
    return np.dot(p, y)


def d_linear(p, y):
    return np.asarray(p, dtype=float)


def neg_sum_exp(p, y):                                      # test_2a.py:60-62
    aux = -np.exp(y)
    return np.sum(aux, axis=0)


def d_neg_sum_exp(p, y):
    return -np.exp(y)


def make_neg_exp_cos(m):                                    # test_3a.py:53-66
    c = _weights(m)

    def U(p, y):
        y_copy = np.squeeze(y)
        aux = np.multiply(np.exp(-y_copy / PI), np.cos(PI * y_copy))
        return -np.dot(c, aux)

    def dU(p, y):
        y_copy = np.squeeze(y)
        aux = -PI * np.multiply(np.exp(-y_copy / PI), np.sin(PI * y_copy)) - np.multiply(np.exp(-y_copy / PI), np.cos(PI * y_copy)) / PI
        return -np.multiply(c, aux)
    return U, dU


def make_rosenbrock(m):                                     # test_5a.py:48-59 (d - 1 = m / 2)
    h = m // 2

    def U(a, y):
        val = 0
        for j in range(h):
            val -= (a - y[j]) ** 2 + 100 * y[j + h] ** 2
        return val

    def dU(a, y):
        g = np.zeros((m,))
        for j in range(h):
            g[j] = 2 * (np.squeeze(a) - y[j])
            g[j + h] = -200 * y[j + h]
        return g
    return U, dU


# ---- three outside the closed set
def abs15(t, y):                                            # the callable of tests/test_host_cpu.py:316
    return -np.sum(np.abs((np.asarray(y).T - t).T) ** 1.5, axis=0)


def tanh_ratio(t, y):
    return -np.sum(np.tanh(y) ** 2 / (1 + y ** 2), axis=0)


def hinge(t, y):
    return np.sum(2.0 * UP.maximum(y - 0.25, 0.0) - UP.minimum(y, 0.5) ** 2, axis=0)


def cases(m):
    """(name, func, dfunc or None, theta_dim, arithmetic only)"""
    nec, dnec = make_neg_exp_cos(m)
    ros, dros = make_rosenbrock(m)
    out = [("neg_sq_dist", neg_sq_dist, d_neg_sq_dist, m, True), ("linear", linear, d_linear, m, True),
           ("neg_sum_exp", neg_sum_exp, d_neg_sum_exp, 1, False), ("neg_exp_cos", nec, dnec, 1, False),
           ("abs15", abs15, None, m, False), ("tanh_ratio", tanh_ratio, None, 1, False), ("hinge", hinge, None, 1, False)]
    if m % 2 == 0:
        out.insert(4, ("rosenbrock", ros, dros, 1, True))
    return out


REFERENCE_FIVE = ("neg_sq_dist", "linear", "neg_sum_exp", "neg_exp_cos", "rosenbrock")


def header_limits():
    text = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    return {k: int(v, 0) for k, v in re.findall(r"#define (BOCF_PROG_[A-Z_]+) (0x[0-9a-fA-F]+|\d+)", text)}


@pytest.fixture(scope="module")
def traced():
    """{(name, m): (Program, func, dfunc, theta_dim, arithmetic only)}, traced once."""
    out = {}
    for m in (4, 5, 16):
        for name, f, df, td, arith in cases(m):
            out[(name, m)] = (UP.trace(f, m, td), f, df, td, arith)
    return out


def _points(m, td, n=50, seed=11, positive=False):
    """50 seeded points.  The bounds below are relative to the RESULT, and the callables sum in an order of their own (np.dot is a BLAS
    dot, np.sum is pairwise) while a program sums left to right: a reordering costs about one ulp of the largest TERM, which is unbounded
    relative to a result that cancels to nearly zero.  For the + - x / utilities (bound 1e-14) the points are therefore drawn where no sum
    cancels -- positive theta and y, every term of one sign -- so that the bound measures the arithmetic and not the cancellation."""
    rng = np.random.RandomState(seed + m)
    if positive:
        return rng.uniform(0.2, 1.0, size=td), rng.uniform(0.25, 1.5, size=(m, n))
    return rng.uniform(-1.0, 1.0, size=td), rng.uniform(-1.5, 1.5, size=(m, n))


def test_interpreter_of_the_encoded_blob_equals_the_callable(traced):
    for (name, m), (prog, f, _, td, arith) in traced.items():
        theta, Y = _points(m, td, positive=arith)
        prog = UP.Program.from_bytes(prog.to_bytes())        # what is interpreted is the ENCODED program
        want = np.array([float(np.squeeze(f(theta, Y[:, i]))) for i in range(Y.shape[1])])
        got = prog.value(theta, Y)
        np.testing.assert_allclose(got, want, rtol=1e-14 if arith else 1e-12, atol=0, err_msg="%s m=%d" % (name, m))
        cols = np.array([prog.value(theta, Y[:, i]) for i in range(Y.shape[1])])
        assert np.array_equal(cols, got), (name, m)          # vectorised == column by column, exactly
        v2, g = prog.value_and_grad(theta, Y)
        assert np.array_equal(v2, got), (name, m)            # the gradient section's U is the value section's
        gcols = np.stack([prog.value_and_grad(theta, Y[:, i])[1] for i in range(Y.shape[1])], -1)
        assert np.array_equal(gcols, g), (name, m)


def test_gradient_section(traced):
    for (name, m), (prog, f, df, td, _) in traced.items():
        theta, Y = _points(m, td)
        g = prog.value_and_grad(theta, Y)[1]
        assert g.shape == Y.shape
        if df is not None:                                   # the scripts' own dfunc
            want = np.stack([np.asarray(df(theta, Y[:, i]), dtype=float).reshape(-1) for i in range(Y.shape[1])], -1)
            np.testing.assert_allclose(g, want, rtol=1e-12, atol=0, err_msg="%s m=%d" % (name, m))
        else:                                                # central differences of the value section
            h = 1e-6
            fd = np.empty_like(Y)
            for j in range(m):
                Yp, Ym = Y.copy(), Y.copy()
                Yp[j] += h
                Ym[j] -= h
                fd[j] = (prog.value(theta, Yp) - prog.value(theta, Ym)) / (2 * h)
            np.testing.assert_allclose(g, fd, rtol=1e-5, atol=0, err_msg="%s m=%d" % (name, m))


def test_reference_utilities_fit_the_limits_at_max_m(traced):
    lim = header_limits()
    assert (lim["BOCF_PROG_MAX_INSTR"], lim["BOCF_PROG_MAX_SLOTS"], lim["BOCF_PROG_MAX_CONSTS"]) == (UP.MAX_INSTR, UP.MAX_SLOTS, UP.MAX_CONSTS)
    assert (lim["BOCF_PROG_MAGIC"], lim["BOCF_PROG_VERSION"], lim["BOCF_PROG_HEADER_WORDS"]) == (UP.MAGIC, UP.VERSION, UP.HEADER_WORDS)
    for name in REFERENCE_FIVE:
        prog = traced[(name, 16)][0]
        assert 1 <= len(prog.val_code) <= lim["BOCF_PROG_MAX_INSTR"] and 1 <= len(prog.grad_code) <= lim["BOCF_PROG_MAX_INSTR"], name
        assert 1 <= prog.n_slots <= lim["BOCF_PROG_MAX_SLOTS"] and prog.consts.size <= lim["BOCF_PROG_MAX_CONSTS"], name
    # slots are the values alive at once, not the instruction count
    nec = traced[("neg_exp_cos", 16)][0]
    assert nec.n_slots < len(nec.grad_code) // 4
    # a program beyond a limit raises and names the limit
    with pytest.raises(UP.ProgramLimitError, match="BOCF_PROG_MAX_INSTR"):
        UP.trace(lambda t, y: sum(np.exp(y[0] * (k + 2.0)) for k in range(lim["BOCF_PROG_MAX_INSTR"])), 1, 1)


def test_blob_and_pickled_utility_round_trip(traced):
    for (name, m), (prog, _, _, td, _) in traced.items():
        blob = prog.to_bytes()
        assert len(blob) == 4 * UP.HEADER_WORDS + 8 * (len(prog.val_code) + len(prog.grad_code) + prog.consts.size)
        again = UP.Program.from_bytes(blob)
        assert again.to_bytes() == blob and (again.m, again.theta_dim, again.n_slots) == (m, td, prog.n_slots)
    m = 3
    theta = np.array([[0.3, -0.1, 0.2], [0.0, 0.4, -0.3]])
    U = B.Utility(func=abs15, parameter_dist=B.ParameterDistribution(support=theta, prob_dist=np.array([0.25, 0.75])), device="program")
    assert U.program_blob is None                            # traced at the first device_kind(m), where m is known
    assert U.device_kind(m) == B._ffi.UTIL_PROGRAM == 5
    V = pickle.loads(pickle.dumps(U))
    assert V.device == "program" and V.program_blob == U.program_blob and V.device_kind(m) == B._ffi.UTIL_PROGRAM
    W = B.Utility(func=lambda t, y: abs15(t, y), parameter_dist=U.parameter_dist, device="program")     # a lambda does not pickle ...
    W.device_kind(m)
    W2 = pickle.loads(pickle.dumps(W))                       # ... its traced program stands in for it
    y = np.random.RandomState(3).uniform(-1, 1, size=(m, 7))
    np.testing.assert_allclose(W2.eval_func(theta[0], y), abs15(theta[0], y), rtol=1e-12)
    np.testing.assert_allclose(W2.eval_gradient(theta[0], y), U.eval_gradient(theta[0], y), rtol=0, atol=0)
    want = -1.5 * np.sign((y.T - theta[0]).T) * np.abs((y.T - theta[0]).T) ** 0.5
    np.testing.assert_allclose(U.eval_gradient(theta[0], y), want, rtol=1e-12)      # no dfunc given: the program's gradient section
    with pytest.raises(ValueError):
        B.Utility(func=abs15, parameter_dist=U.parameter_dist, device="nope")
    with pytest.raises(ValueError):
        B.Utility(parameter_dist=U.parameter_dist, device="program")                # nothing to trace


def _check(blob, m, td):
    lib = B._ffi.load()
    rc = lib.bocf_check_utility_program(bytes(blob), len(blob), m, td)
    return rc, lib.bocf_last_error().decode()


def test_validator_accepts_every_traced_program(traced):
    for (name, m), (prog, _, _, td, _) in traced.items():
        rc, err = _check(prog.to_bytes(), m, td)
        assert rc == 0, (name, m, err)
    rc, err = _check(traced[("linear", 4)][0].to_bytes(), 5, 4)
    assert rc != 0 and "m = " in err
    rc, err = _check(traced[("linear", 4)][0].to_bytes(), 4, 3)
    assert rc != 0 and "theta_dim" in err


def _words(blob):
    n = (len(blob) - 0) // 4
    return list(struct.unpack("<%dI" % n, blob))


def _pack(words):
    return struct.pack("<%dI" % len(words), *words)


def test_validator_rejects_and_names_the_field(traced):
    prog = traced[("neg_exp_cos", 4)][0]                     # uses slots, inputs and constants; "linear" uses parameters
    blob, m, td = prog.to_bytes(), 4, 1
    H = UP.HEADER_WORDS
    w = _words(blob)
    first_slot_read = next(i for i, (_, _, a, b) in enumerate(prog.val_code) if a >> 14 == UP.K_SLOT)
    first_input = next(i for i, (_, _, a, b) in enumerate(prog.val_code) if a >> 14 == UP.K_INPUT)
    first_const = next(i for i, (_, _, a, b) in enumerate(prog.val_code) if b >> 14 == UP.K_CONST or a >> 14 == UP.K_CONST)

    def with_word(i, v, base=w):
        x = list(base)
        x[i] = v
        return _pack(x)

    def operand_a(i, kind, idx):
        return (w[H + 2 * i + 1] & 0xffff0000) | kind << 14 | idx
    bad = {
        "truncated": (blob[:-8], "truncated"),
        "truncated header": (blob[:40], "truncated"),
        "version": (with_word(1, UP.VERSION + 1), "version"),
        "opcode": (with_word(H, (w[H] & ~0xff) | len(UP.OPS)), "opcode"),
        "slot index": (with_word(H + 2 * first_slot_read + 1, operand_a(first_slot_read, UP.K_SLOT, prog.n_slots)), "slot index"),
        "destination": (with_word(H, (w[H] & 0xff) | prog.n_slots << 8), "slot index"),
        "read before write": (with_word(H + 1, operand_a(0, UP.K_SLOT, prog.n_slots - 1)), "read before it is written"),
        "input index": (with_word(H + 2 * first_input + 1, operand_a(first_input, UP.K_INPUT, m)), "input index"),
        "constant index": (with_word(H + 2 * first_const + 1, (w[H + 2 * first_const + 1] & 0xffff) | (UP.K_CONST << 14 | prog.consts.size) << 16
                                     if prog.val_code[first_const][3] >> 14 == UP.K_CONST else operand_a(first_const, UP.K_CONST, prog.consts.size)),
                           "constant index"),
        "non-finite constant": (blob[:-8] + struct.pack("<d", float("inf")), "not finite"),
        "nan constant": (blob[:-8] + struct.pack("<d", float("nan")), "not finite"),
        "section too long": (with_word(5, UP.MAX_INSTR + 1), "BOCF_PROG_MAX_INSTR"),
        "gradient section too long": (with_word(6, UP.MAX_INSTR + 1), "BOCF_PROG_MAX_INSTR"),
        "too many slots": (with_word(4, UP.MAX_SLOTS + 1), "BOCF_PROG_MAX_SLOTS"),
        "output slot": (with_word(8, prog.n_slots), "output"),
    }
    for what, (b, word) in bad.items():
        rc, err = _check(b, m, td)
        assert rc != 0 and word in err, (what, rc, err)
    lin = traced[("linear", 4)][0]
    lw = _words(lin.to_bytes())
    i = next(i for i, (_, _, a, b) in enumerate(lin.val_code) if a >> 14 == UP.K_PARAM)
    lw[H + 2 * i + 1] = (lw[H + 2 * i + 1] & 0xffff0000) | UP.K_PARAM << 14 | 4
    rc, err = _check(_pack(lw), 4, 4)
    assert rc != 0 and "parameter index" in err, err
    assert _check(blob, m, td)[0] == 0                       # (the untouched blob is fine)


def test_trace_errors():
    with pytest.raises(UP.TraceError, match="control flow"):
        UP.trace(lambda t, y: y[0] if y[0] > 0 else -y[0], 2, 1)
    with pytest.raises(UP.TraceError):
        UP.trace(lambda t, y: np.sum(np.maximum(y, 0.0)), 2, 1)
    with pytest.raises(UP.TraceError):
        UP.trace(lambda t, y: np.max(y), 2, 1)
    prog = UP.trace(lambda t, y: np.sum(UP.maximum(y, 0.0)), 2, 1)
    assert prog.value([0.0], np.array([-1.0, 2.0])) == 2.0
    assert UP.maximum(np.array([1.0, -2.0]), 0.0).tolist() == [1.0, 0.0]     # plain numbers pass through
    c = 3.0
    prog = UP.trace(lambda t, y: c * y[0] + t[0], 1, 1)      # a constant of the closure is a literal of the program
    assert prog.value([0.5], np.array([2.0])) == 6.5 and 3.0 in prog.consts
    one = UP.trace(lambda t, y: y[0], 3, 1)                  # U = y_0: one instruction
    assert len(one.val_code) == 1 and one.value([0.0], np.array([1.25, 0.0, 0.0])) == 1.25
    assert B.TraceError is UP.TraceError
    U = B.Utility(func=lambda t, y: np.sum(np.maximum(y, 0.0)), device="program",
                  parameter_dist=B.ParameterDistribution(support=np.ones((1, 1)), prob_dist=np.ones(1)))
    with pytest.raises(UP.TraceError):                       # an explicit request does not fall back
        U.device_kind(2)


def test_default_behaviour_is_unchanged():
    m = 3
    dist = B.ParameterDistribution(support=np.array([[0.3, -0.1, 0.2]]), prob_dist=np.ones(1))
    for f in (abs15, tanh_ratio, hinge):
        U = B.Utility(func=f, parameter_dist=dist)
        with pytest.raises(NotImplementedError):
            U.device_kind(m)
        assert U.device is None and U.program_blob is None   # device=None never traces
    U = B.Utility(func=neg_sq_dist, parameter_dist=dist)
    assert U.device_kind(m) == B._ffi.UTIL_NEG_SQ_DIST       # the closed set is still recognised
