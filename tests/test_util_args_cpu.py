"""CPU-only checks of the utility-argument block (bocf_amd/csrc/util_args.h): the checks bocf_acq_kg, bocf_acq_pending,
bocf_acq_mc_constrained and bocf_feasible_best share -- which argument lists they refuse, with which text, and which fault is reported
when a list has several -- and the two packers' exact doubles.  The header is driven through tests/util_args_driver.cpp, built once as
it is and once with AddressSanitizer and UndefinedBehaviorSanitizer; every test runs against both.

Every expected text is a literal copied from the entry points as they stood before the header existed (capi_kg.hip, capi_pending.hip,
capi_constrained.hip), and `parent_verdict` is a transcription of their check sequence: nothing expected here comes from the header."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

LINEAR, NEG_SQ_DIST, NEG_SUM_EXP, NEG_EXP_COS, ROSENBROCK, PROGRAM = range(6)
MEAN, CLOSED, MC = range(3)
MODES = {MEAN: "mean", CLOSED: "closed", MC: "mc"}

NO_PROGRAM = {
    "bocf_acq_kg": "the knowledge gradient does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities",
    "bocf_acq_pending": "the pending-point acquisition does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities",
    "bocf_acq_mc_constrained": "the constrained acquisition does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities",
    "bocf_feasible_best": "the constrained acquisition does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities",
}
WHO = sorted(NO_PROGRAM)
UNKNOWN_KIND = "unknown utility kind"
BAD_L = "L out of range (1 .. 32)"
BAD_THETA = "theta must be (L, 1 <= theta_dim <= 16)"
THETA_DIM = "theta_dim must equal m"
ROSENBROCK_ODD = "rosenbrock utility needs even m"
NO_CLOSED_FORM = "no closed-form expectation for this utility (use the Monte-Carlo mode)"
BAD_PARAMS = "bad utility parameters"
NEG_EXP_COS_WEIGHTS = "neg_exp_cos needs m weights"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ next to hipcc")
    exe = str(tmp_path_factory.mktemp("util_args") / ("util_args_driver_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror"] + extra + [os.path.join(ROOT, "tests", "util_args_driver.cpp"), "-o", exe])
    return exe


def run(driver, command, lines):
    out = subprocess.run([driver, command], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines), (len(got), len(lines), out.stderr)
    return got


def case(kind=NEG_SQ_DIST, n_params=0, params_null=False, theta_null=False, theta_dim=None, L=1, m=2, mode=MC):
    return dict(kind=kind, n_params=n_params, params_null=params_null, theta_null=theta_null, theta_dim=m if theta_dim is None else theta_dim,
                L=L, m=m, mode=mode)


def verdicts(driver, who, cases):
    """What the two-part checker says of each case when `who` calls it: None when it accepts, else the text behind "who: "."""
    lines = ["%s|%s|%d %d %d %d %d %d %d %d" % (who, NO_PROGRAM[who], c["kind"], c["n_params"], c["params_null"], c["theta_null"], c["theta_dim"],
                                                 c["L"], c["m"], c["mode"]) for c in cases]
    out = []
    for got in run(driver, "check", lines):
        if got == "ok":
            out.append(None)
        else:
            assert got.startswith(who + ": "), got
            out.append(got[len(who) + 2:])
    return out


def parent_verdict(who, kind, n_params, params_null, theta_null, theta_dim, L, m, mode):
    """The check sequence of bocf_acq_kg before the header (the three improvement entry points: the same sequence at mode = MC)."""
    if kind == PROGRAM:
        return NO_PROGRAM[who]
    if kind < LINEAR or kind > ROSENBROCK:
        return UNKNOWN_KIND
    if L < 1 or L > 32:
        return BAD_L
    if theta_dim < 1 or theta_dim > 16 or theta_null:
        return BAD_THETA
    if (mode == MEAN or kind in (LINEAR, NEG_SQ_DIST)) and theta_dim != m:
        return THETA_DIM
    if mode != MEAN and kind == ROSENBROCK and m % 2:
        return ROSENBROCK_ODD
    if mode == CLOSED and kind in (LINEAR, NEG_EXP_COS):
        return NO_CLOSED_FORM
    if n_params < 0 or n_params > 16 or (n_params > 0 and params_null):
        return BAD_PARAMS
    if mode == MC and kind == NEG_EXP_COS and n_params != m:
        return NEG_EXP_COS_WEIGHTS
    return None


def expect(driver, who, table):
    got = verdicts(driver, who, [c for c, _ in table])
    for (c, want), g in zip(table, got):
        assert g == want, (who, c, g, want)


@pytest.mark.parametrize("who", WHO)
def test_a_program_is_refused_in_the_callers_words(driver, who):
    assert len(set(NO_PROGRAM.values())) == 3
    expect(driver, who, [(case(kind=PROGRAM, mode=mode, m=m, L=L), NO_PROGRAM[who]) for mode in MODES for m in (1, 2, 15, 16) for L in (1, 32)])


@pytest.mark.parametrize("who", WHO)
def test_each_refusal(driver, who):
    table = []
    for m, L, mode in itertools.product((1, 2, 15, 16), (1, 32), MODES):
        ok = NEG_SUM_EXP                                      # reads neither theta's width nor parameters: accepted wherever nothing else is wrong
        table += [
            (case(kind=-1, m=m, L=L, mode=mode), UNKNOWN_KIND),
            (case(kind=6, m=m, L=L, mode=mode), UNKNOWN_KIND),
            (case(kind=ok, m=m, L=0, mode=mode), BAD_L),
            (case(kind=ok, m=m, L=33, mode=mode), BAD_L),
            (case(kind=ok, m=m, L=L, mode=mode, theta_null=True), BAD_THETA),
            (case(kind=ok, m=m, L=L, mode=mode, theta_dim=0), BAD_THETA),
            (case(kind=ok, m=m, L=L, mode=mode, theta_dim=17), BAD_THETA),
            (case(kind=LINEAR, m=m, L=L, mode=mode, theta_dim=m % 16 + 1), THETA_DIM),
            (case(kind=NEG_SQ_DIST, m=m, L=L, mode=mode, theta_dim=m % 16 + 1), THETA_DIM),
        ]
        # a theta of another width than m: in the mean form every kind reads theta . mu; otherwise only the two kinds above mind
        for kind in (NEG_SUM_EXP, NEG_EXP_COS, ROSENBROCK):
            table.append((case(kind=kind, m=m, L=L, mode=MEAN, theta_dim=m % 16 + 1), THETA_DIM))
        table.append((case(kind=NEG_SUM_EXP, m=m, L=L, mode=mode, theta_dim=m % 16 + 1), THETA_DIM if mode == MEAN else None))
        table.append((case(kind=ROSENBROCK, m=m, L=L, mode=mode), ROSENBROCK_ODD if (m % 2 and mode != MEAN) else None))
        if mode == CLOSED:
            table += [(case(kind=LINEAR, m=m, L=L, mode=mode), NO_CLOSED_FORM), (case(kind=NEG_EXP_COS, m=m, L=L, mode=mode, n_params=m), NO_CLOSED_FORM)]
        else:
            table.append((case(kind=LINEAR, m=m, L=L, mode=mode), None))
        table += [
            (case(kind=ok, m=m, L=L, mode=mode, n_params=-1), BAD_PARAMS),
            (case(kind=ok, m=m, L=L, mode=mode, n_params=17), BAD_PARAMS),
            (case(kind=ok, m=m, L=L, mode=mode, n_params=3, params_null=True), BAD_PARAMS),
            (case(kind=ok, m=m, L=L, mode=mode, n_params=3), None),
            (case(kind=ok, m=m, L=L, mode=mode, n_params=0, params_null=True), None),
            (case(kind=ok, m=m, L=L, mode=mode, n_params=16), None),
        ]
        if mode != CLOSED:                                    # the weights are counted in the Monte-Carlo form only
            table.append((case(kind=NEG_EXP_COS, m=m, L=L, mode=mode, n_params=m % 16 + 1), NEG_EXP_COS_WEIGHTS if mode == MC else None))
            table.append((case(kind=NEG_EXP_COS, m=m, L=L, mode=mode, n_params=m), None))
    expect(driver, who, table)


@pytest.mark.parametrize("who", WHO)
def test_the_earlier_of_two_faults_is_reported(driver, who):
    """The checks in their order: program, kind, L, theta, theta_dim = m, rosenbrock, closed form, parameters, neg_exp_cos weights.  For
    each neighbouring pair one list that fails both.  Two pairs cannot fail together -- theta_dim = m binds LINEAR / NEG_SQ_DIST (or the
    mean form) and the rosenbrock check another kind outside the mean form; the rosenbrock and closed-form checks bind different kinds
    -- so each of the three meets its next neighbour that can."""
    for m, L in itertools.product((1, 2, 15, 16), (1, 32)):
        odd = m if m % 2 else m - 1                           # 1, 1, 15, 15
        expect(driver, who, [
            (case(kind=PROGRAM, m=m, L=0), NO_PROGRAM[who]),                                          # program (also > ROSENBROCK: "unknown") | L
            (case(kind=-1, m=m, L=0), UNKNOWN_KIND),                                                  # kind | L
            (case(kind=6, m=m, L=33, theta_null=True), UNKNOWN_KIND),
            (case(m=m, L=0, theta_null=True), BAD_L),                                                 # L | theta
            (case(m=m, L=33, theta_dim=0), BAD_L),
            (case(kind=LINEAR, m=m, L=L, theta_dim=17), BAD_THETA),                                   # theta | theta_dim = m
            (case(kind=NEG_SQ_DIST, m=m, L=L, theta_dim=m % 16 + 1, theta_null=True), BAD_THETA),
            (case(kind=LINEAR, m=m, L=L, theta_dim=m % 16 + 1, mode=CLOSED), THETA_DIM),              # theta_dim = m | closed form
            (case(kind=NEG_SQ_DIST, m=m, L=L, theta_dim=m % 16 + 1, n_params=-1), THETA_DIM),         # theta_dim = m | parameters
            (case(kind=ROSENBROCK, m=odd, L=L, n_params=17), ROSENBROCK_ODD),                         # rosenbrock | parameters
            (case(kind=ROSENBROCK, m=odd, L=L, n_params=2, params_null=True, mode=CLOSED), ROSENBROCK_ODD),
            (case(kind=LINEAR, m=m, L=L, mode=CLOSED, n_params=17), NO_CLOSED_FORM),                  # closed form | parameters
            (case(kind=NEG_EXP_COS, m=m, L=L, mode=CLOSED, n_params=m, params_null=True), NO_CLOSED_FORM),
            (case(kind=NEG_EXP_COS, m=m, L=L, n_params=17), BAD_PARAMS),                              # parameters | neg_exp_cos weights
            (case(kind=NEG_EXP_COS, m=m, L=L, n_params=m % 16 + 1, params_null=True), BAD_PARAMS),
        ])


@pytest.mark.parametrize("who", WHO)
def test_every_list_of_a_grid_gets_the_verdict_it_got_before(driver, who):
    cases = [case(kind=kind, n_params=n_params, params_null=params_null, theta_null=theta_null, theta_dim=theta_dim, L=L, m=m, mode=mode)
             for kind in range(-1, 7) for n_params in (-1, 0, 1, 2, 15, 16, 17) for params_null in (False, True) for theta_null in (False, True)
             for theta_dim in (0, 1, 2, 15, 16, 17) for L in (0, 1, 32, 33) for m in (1, 2, 15, 16) for mode in MODES]
    got = verdicts(driver, who, cases)
    for c, g in zip(cases, got):
        assert g == parent_verdict(who, **c), (who, c, g)


def floats(tokens):
    return [float(t) for t in tokens]


@pytest.mark.parametrize("L", [1, 3, 32])
@pytest.mark.parametrize("theta_dim", [1, 2, 16])
def test_pack(driver, L, theta_dim):
    theta = [0.1 * (i + 1) / 3.0 for i in range(L * theta_dim)]
    prob = [(l + 1.0) / 7.0 for l in range(L)]
    tail = [-1.0 / (i + 3.0) for i in range(5)]
    lines, want = [], []
    for n_params, prob_given, n_tail in itertools.product((0, 1, 3, 16), (0, 1), (0, 5)):
        params = [2.0 ** -i + 0.3 for i in range(n_params)]
        vals = theta + (prob if prob_given else []) + params + tail[:n_tail]
        lines.append(" ".join(["%d %d %d %d %d" % (L, theta_dim, n_params, prob_given, n_tail)] + [repr(v) for v in vals]))
        nth = L * theta_dim
        block = theta + (prob if prob_given else [1.0 / L] * L) + params + [0.0] * (16 - n_params) + tail[:n_tail]
        want.append(([0, nth, nth + L, nth + L + 16, nth + L + 16 + n_tail], block))
    for line, got, (offsets, block) in zip(lines, run(driver, "pack", lines), want):
        got = got.split()
        assert [int(t) for t in got[:5]] == offsets, line
        assert floats(got[5:]) == block, line                # exact: copies, zeros, and 1.0 / L as the double division gives it


@pytest.mark.parametrize("theta_dim,per,tw", [(0, 1, 1), (1, 3, 3), (3, 2, 3), (16, 16, 16)])
def test_pack_rows(driver, theta_dim, per, tw):
    lines, want = [], []
    for P, n_params in itertools.product((1, 4), (0, 2, 16)):
        theta = [[1.0 + p + 0.01 * q for q in range(theta_dim)] for p in range(P)]
        params = [0.5 / (i + 1.0) for i in range(n_params)]
        lines.append(" ".join(["%d %d %d %d" % (theta_dim, P, per, n_params)] + [repr(v) for row in theta for v in row] + [repr(v) for v in params]))
        want.append([v for row in theta for v in row + [0.0] * (tw - theta_dim)] + params + [0.0] * (16 - n_params))
    for line, got, block in zip(lines, run(driver, "rows", lines), want):
        got = got.split()
        assert [int(got[0]), int(got[1])] == [tw, len(block)], line
        assert floats(got[2:]) == block, line
