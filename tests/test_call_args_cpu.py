"""The argument checks of the entry points that evaluate a utility over the posterior (bocf_amd/csrc/call_args.h), through their stand-alone
driver (tests/call_args_driver.cpp), built plain and with AddressSanitizer + UBSan.  Per entry point: one fault per check, in the order
the entry point makes them; for every adjacent pair of checks the earlier of two faults; acceptance at both ends of every range.

The expected texts are the literals of the entry points as they stood before the checks moved into the header (capi.hip, capi_kg.hip,
capi_pending.hip, capi_joint.hip, capi_constrained.hip, capi_loo.hip, capi_thompson.hip, util_args.h): bocf_last_error() is part of the
ABI's observable behaviour, so every line is compared whole.  The check of the resident utility program stays with the entry point (it
reads the program); the driver takes it as passed and goes on with what stands behind it, as the entry point does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

NOT_FITTED = "model not fitted"
NO_FACTOR = "the context holds a host-given posterior (bocf_set_posterior): it has no factor to sample from; fit first"
NO_GRADIENTS = "the context holds a host-given posterior (bocf_set_posterior): it carries no gradients; fit first"
WHOLE = "the fitted outputs are not a whole number of hyper-samples (option hyper_samples)"
WHOLE_OLD = "the fitted outputs are not a multiple of option hyper_samples"
MANY = "more outputs per hyper-sample than the device utilities take (16)"
MANY_OLD = "too many outputs per hyper-sample"
BEST_GROUP = "option best_group is not a valid hyper-sample index"
ACQ_KIND = "unknown acquisition kind"
UTIL_KIND = "unknown utility kind"
MODE = "unknown mode"
NO_MC = "no Monte-Carlo samples set (bocf_set_mc_samples)"
MC_256 = "more than 256 Monte-Carlo samples"
NO_EU = "no Monte-Carlo samples set (bocf_set_eu_samples)"
NO_CANDIDATES = "no resident candidates (bocf_set_candidates)"
DIM = "input dimension too large"
THETA_DIM = "theta_dim must equal m"
L_RANGE = "L out of range (1 .. 32)"
THETA = "theta must be (L, 1 <= theta_dim <= 16)"
EVEN_M = "rosenbrock utility needs even m"
NO_CLOSED = "no closed-form expectation for this utility (use the Monte-Carlo mode)"
BAD_PARAMS = "bad utility parameters"
WEIGHTS = "neg_exp_cos needs m weights"
PROGRAM_CLOSED = "a utility program has no closed-form expectation (BOCF_EU_CLOSED): use the Monte-Carlo mode"
NO_PROGRAM = "the %s does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities"
BAD_SAMPLES = "model not fitted / bad samples"

# faults of the group checks, first-generation order (whole groups, best_group, at most 16) and the three faults by themselves
F_WHOLE, F_BEST, F_MANY = dict(m=5, H=2), dict(best_group=2), dict(m=17, kind=2, theta_dim=16)
GROUPS_OLD = [(F_WHOLE, WHOLE_OLD), (F_BEST, BEST_GROUP), (F_MANY, MANY_OLD)]
# util_args.h's block in the Monte-Carlo form, in its order (tests/test_util_args_cpu.py has the block by itself)
UTIL_MC = [(dict(L=0), L_RANGE), (dict(theta_null=1), THETA), (dict(theta_dim=3), THETA_DIM), (dict(kind=4, theta_dim=1, m=3, eu_m=3, cq_m=3), EVEN_M),
           (dict(n_params=2), BAD_PARAMS), (dict(kind=3, theta_dim=1), WEIGHTS)]
# pairs of adjacent checks that cannot both be at fault: each looks at another utility kind
X_KINDS = {(THETA_DIM, EVEN_M)}

SEQUENCES = {
    "bocf_acq_linear": [(dict(fitted=0), NOT_FITTED), (dict(acq_kind=2), ACQ_KIND)] + GROUPS_OLD,
    "bocf_acq_mc": [(dict(fitted=0), NOT_FITTED), (dict(acq_kind=2), ACQ_KIND), (dict(kind=6), UTIL_KIND), (dict(S_mc=0), NO_MC)] + GROUPS_OLD + [
        (dict(theta_dim=3), THETA_DIM), (dict(kind=4, theta_dim=1, m=3), "rosenbrock utility needs theta_dim >= 1 and even m"),
        (dict(kind=3, theta_dim=1), WEIGHTS), (dict(n_params=2), "util_params is null")],
    "bocf_set_mc_samples": [(dict(fitted=0), BAD_SAMPLES)] + GROUPS_OLD,
    "bocf_expected_utility": [
        (dict(fitted=0), NOT_FITTED), (dict(canned=1), "the context holds a host-given posterior (bocf_set_posterior): fit first"), (dict(mode=3), MODE),
        (dict(kind=6), UTIL_KIND)] + GROUPS_OLD + [
        (dict(L=0), "theta must be (L >= 1, theta_dim >= 1)"), (dict(mode=1, kind=5), PROGRAM_CLOSED), (dict(theta_dim=3), THETA_DIM),
        (dict(kind=4, theta_dim=1, m=3, eu_m=3), EVEN_M), (dict(mode=1, kind=3, theta_dim=1), NO_CLOSED),
        (dict(kind=3, theta_dim=1, n_params=2, params_null=0), WEIGHTS), (dict(n_params=17, params_null=0), BAD_PARAMS), (dict(eu_S=0), NO_EU),
        (dict(eu_L=2), "fewer Monte-Carlo sample blocks than parameters"), (dict(eu_m=3), "the Monte-Carlo samples were set for another output count"),
        (dict(grad=1, d=65), DIM), (dict(n_hyps=0), "n_hyps must be >= 1"), (dict(n_hyps=3, m=8, H=2), "n_hyps exceeds the resident hyper-samples"),
        (dict(val_null=1), "null output / row_param"), (dict(rows=2), "row_param out of range [0, L)")],
    "bocf_acq_kg": [
        (dict(fitted=0), NOT_FITTED), (dict(canned=1), NO_FACTOR), (dict(mode=3), MODE), (dict(kind=5), NO_PROGRAM % "knowledge gradient"),
        (dict(kind=6), UTIL_KIND), (F_WHOLE, WHOLE), (F_MANY, MANY), (dict(L=0), L_RANGE), (dict(theta_null=1), THETA), (dict(theta_dim=3), THETA_DIM),
        (dict(kind=4, theta_dim=1, m=3), EVEN_M), (dict(mode=1, kind=3, theta_dim=1), NO_CLOSED), (dict(n_params=2), BAD_PARAMS),
        (dict(kind=3, theta_dim=1), WEIGHTS), (dict(z_null=1), "null Zf"), (dict(S=0), "Sf out of range (1 .. 256)"), (dict(S_mc=0), NO_MC),
        (dict(S_mc=257), MC_256), (dict(kg_na=0), "no reference points: call bocf_set_ref_points after the fit"), (dict(C=0), NO_CANDIDATES), (dict(d=33), DIM)],
    "bocf_acq_pending": [
        (dict(fitted=0), NOT_FITTED), (dict(canned=1), NO_FACTOR), (dict(kind=5), NO_PROGRAM % "pending-point acquisition"), (dict(kind=6), UTIL_KIND),
        (F_WHOLE, WHOLE), (F_MANY, MANY)] + UTIL_MC + [
        (dict(S_mc=0), NO_MC), (dict(S_mc=257), MC_256), (dict(pd_r=0), "no pending points: call bocf_set_pending_points after the fit"),
        (dict(pd_S=24), "the number of Monte-Carlo samples changed since bocf_set_pending_points"), (dict(C=0), NO_CANDIDATES), (dict(d=33), DIM),
        (F_BEST, BEST_GROUP)],
    "bocf_acq_joint": [
        (dict(fitted=0), NOT_FITTED), (dict(canned=1), NO_FACTOR), (dict(kind=5), NO_PROGRAM % "joint acquisition"), (dict(kind=6), UTIL_KIND),
        (F_WHOLE, WHOLE), (F_MANY, MANY)] + UTIL_MC + [
        (dict(q=0), "q out of range (1 .. 8)"), (dict(z_null=1), "null Z"), (dict(S=0), "S out of range (1 .. 256)"), (dict(C=0), NO_CANDIDATES),
        (dict(q=2), "the number of resident candidates is not a multiple of q"), (dict(d=33), DIM), (F_BEST, BEST_GROUP)],
    "bocf_feasible_best": [
        (dict(fitted=0), NOT_FITTED), (dict(kind=5), NO_PROGRAM % "constrained acquisition"), (dict(kind=6), UTIL_KIND),
        (dict(cq_K=0), "no output constraints resident (bocf_set_output_constraints)"), (F_WHOLE, WHOLE), (F_MANY, MANY),
        (dict(cq_m=3), "the resident output constraints were given for another m than the outputs per hyper-sample"), (F_BEST, BEST_GROUP)] + UTIL_MC,
    "bocf_loo_utility": [
        (dict(fitted=0), NOT_FITTED), (dict(canned=1), NO_FACTOR), (dict(flags=4), "unknown flags (BOCF_ADD_NOISE | BOCF_CLIP)"), (dict(mode=3), MODE),
        (dict(group=-1), "group out of range (0 .. hyper_samples - 1)"), (F_WHOLE, WHOLE), (dict(group=1), "group out of range (-1 or 0 .. hyper_samples - 1)"),
        (F_MANY, MANY), (dict(kind=6), UTIL_KIND)] + UTIL_MC + [
        (dict(eu_S=0), NO_EU), (dict(eu_L=2), "fewer Monte-Carlo sample blocks than parameters (bocf_set_eu_samples)"),
        (dict(eu_m=3), "the Monte-Carlo samples were set for another output count (bocf_set_eu_samples)"), (dict(val_null=1), "null val_out")],
}
SEQUENCES["bocf_acq_linear_grad"] = SEQUENCES["bocf_acq_linear"]            # (no check of d: the pair shares one sequence)
SEQUENCES["bocf_acq_mc_grad"] = [SEQUENCES["bocf_acq_mc"][0]] + SEQUENCES["bocf_acq_mc"][2:] + [(dict(d=65), DIM)]   # no acquisition kind; d last
SEQUENCES["bocf_set_eu_samples"] = SEQUENCES["bocf_set_mc_samples"]
SEQUENCES["bocf_acq_mc_constrained"] = SEQUENCES["bocf_feasible_best"] + [(dict(S_mc=0), NO_MC), (dict(C=0), NO_CANDIDATES),
                                                                          (dict(canned=1, grad=1), NO_GRADIENTS), (dict(d=65, grad=1), DIM)]
# the program branch of bocf_loo_utility, from the outputs per hyper-sample on
LOO_PROGRAM = [(F_MANY, MANY), (dict(kind=5, mode=1), PROGRAM_CLOSED), (dict(kind=5, L=0), L_RANGE), (dict(kind=5, theta_null=1), THETA), (dict(kind=5, eu_S=0), NO_EU)]

# Adjacent checks that cannot both be at fault (None), or the two faults together where the plain union of the two settings is not it.
PAIRS = {
    ("bocf_acq_mc", THETA_DIM): None, ("bocf_acq_mc", "rosenbrock utility needs theta_dim >= 1 and even m"): None,   # each looks at another utility kind
    ("bocf_acq_mc_grad", THETA_DIM): None, ("bocf_acq_mc_grad", "rosenbrock utility needs theta_dim >= 1 and even m"): None,
    ("bocf_expected_utility", THETA_DIM): None, ("bocf_expected_utility", EVEN_M): None, ("bocf_expected_utility", NO_CLOSED): None,   # other kinds, other modes
    ("bocf_expected_utility", WEIGHTS): dict(kind=3, theta_dim=1, n_params=2, params_null=1),
    ("bocf_expected_utility", "n_hyps must be >= 1"): None,                     # n_hyps too small, too large
    ("bocf_acq_kg", NO_PROGRAM % "knowledge gradient"): None,                   # the kind is a program, or out of range
    ("bocf_acq_kg", THETA_DIM): None, ("bocf_acq_kg", EVEN_M): None,
    ("bocf_acq_kg", NO_MC): None,                                               # no samples, too many
    ("bocf_acq_pending", NO_PROGRAM % "pending-point acquisition"): None, ("bocf_acq_pending", NO_MC): None,
    ("bocf_acq_pending", MC_256): dict(S_mc=257, pd_S=257, pd_r=0),
    ("bocf_acq_joint", NO_PROGRAM % "joint acquisition"): None,
    ("bocf_acq_joint", NO_CANDIDATES): None,                                    # no candidate is a multiple of every q
    ("bocf_feasible_best", NO_PROGRAM % "constrained acquisition"): None, ("bocf_acq_mc_constrained", NO_PROGRAM % "constrained acquisition"): None,
    ("bocf_loo_utility", "group out of range (0 .. hyper_samples - 1)"): dict(group=-2, m=5, H=2),
    ("bocf_loo_utility", WHOLE): None,                                          # without whole groups there is no range of groups
}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    assert os.path.exists(CLANG), "no clang++ next to hipcc"
    exe = str(tmp_path_factory.mktemp("call_args") / ("call_args_driver_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror"] + extra + [os.path.join(ROOT, "tests", "call_args_driver.cpp"), "-o", exe])
    return exe


STATE = ["fitted", "canned", "N", "d", "m", "H", "best_group", "C", "S_mc", "eu_S", "eu_L", "eu_m", "cq_K", "cq_m", "kg_na", "pd_r", "pd_S"]
BLOCK = ["kind", "n_params", "params_null", "theta_null", "theta_dim", "L"]
CALL = ["acq_kind", "mode", "grad", "group", "flags", "n_hyps", "rows", "val_null", "z_null", "S", "q"]
DEFAULTS = dict(fitted=1, canned=0, N=20, d=3, m=4, H=1, best_group=-1, C=5, S_mc=25, eu_S=25, eu_L=3, eu_m=4, cq_K=2, cq_m=4, kg_na=3, pd_r=2, pd_S=25,
                kind=1, n_params=0, params_null=1, theta_null=0, theta_dim=4, L=3,
                acq_kind=0, mode=2, grad=0, group=0, flags=3, n_hyps=1, rows=1, val_null=0, z_null=0, S=8, q=1)


def _line(who, **kw):
    c = dict(DEFAULTS)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return "|".join([who] + [" ".join(str(c[k]) for k in part) for part in (STATE, BLOCK, CALL)])


def _verdicts(driver, lines):
    out = subprocess.run([driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines), (got, out.stderr)
    return got


@pytest.mark.parametrize("who", sorted(SEQUENCES))
def test_one_fault_per_check_in_the_entry_points_order(driver, who):
    seq = SEQUENCES[who]
    for (fault, text), g in zip(seq, _verdicts(driver, [_line(who, **f) for f, _ in seq])):
        assert g == who + ": " + text, (fault, g)
    assert _verdicts(driver, [_line(who)]) == ["ok 4"]           # (and without a fault there is no refusal)


@pytest.mark.parametrize("who", sorted(SEQUENCES))
def test_the_earlier_of_two_faults_is_reported(driver, who):
    seq = SEQUENCES[who]
    cases = []
    for (f0, t0), (f1, t1) in zip(seq, seq[1:]):
        both = PAIRS.get((who, t0), dict(f1, **f0))
        if both is not None and (t0, t1) not in X_KINDS:
            cases.append((both, t0))
    assert len(cases) >= len(seq) - 5
    for (both, text), g in zip(cases, _verdicts(driver, [_line(who, **b) for b, _ in cases])):
        assert g == who + ": " + text, (both, g)


def test_the_program_branch_of_loo_utility(driver):
    who = "bocf_loo_utility"
    for (fault, text), g in zip(LOO_PROGRAM, _verdicts(driver, [_line(who, **f) for f, _ in LOO_PROGRAM])):
        assert g == who + ": " + text, (fault, g)
    pairs = [(dict(m=17, theta_dim=16, kind=5, mode=1), MANY), (dict(kind=5, mode=1, L=0), PROGRAM_CLOSED), (dict(kind=5, L=0, theta_null=1), L_RANGE),
             (dict(kind=5, theta_null=1, eu_S=0), THETA)]
    for (both, text), g in zip(pairs, _verdicts(driver, [_line(who, **b) for b, _ in pairs])):
        assert g == who + ": " + text, (both, g)


def test_what_stands_behind_the_resident_programs_check(driver):
    """A program is accepted by the three families that take one; the checks behind the resident program's own still run, in their order."""
    lines = [_line("bocf_acq_mc", kind=5, theta_dim=7), _line("bocf_acq_mc", kind=5, theta_dim=0, theta_null=1), _line("bocf_acq_mc_grad", kind=5),
             _line("bocf_expected_utility", kind=5, theta_dim=7), _line("bocf_loo_utility", kind=5, theta_dim=7),
             _line("bocf_acq_mc_grad", kind=5, d=65), _line("bocf_expected_utility", kind=5, eu_S=0), _line("bocf_expected_utility", kind=5, C=0),
             _line("bocf_loo_utility", kind=5, val_null=1), _line("bocf_loo_utility", kind=5, mode=0), _line("bocf_expected_utility", kind=5, mode=0)]
    assert _verdicts(driver, lines) == ["ok 4 program"] * 5 + ["bocf_acq_mc_grad: " + DIM, "bocf_expected_utility: " + NO_EU, "nothing 4 program",
                                                                "bocf_loo_utility: null val_out", "ok 4", "ok 4"]


def test_acceptance_at_both_ends_of_every_range(driver):
    ok = {
        "bocf_acq_linear": [dict(acq_kind=1), dict(m=16), dict(m=8, H=2, best_group=1), dict(best_group=0), dict(canned=1), dict(C=0), dict(d=65)],
        "bocf_acq_linear_grad": [dict(acq_kind=1), dict(m=16), dict(m=8, H=2, best_group=1), dict(canned=1), dict(C=0), dict(d=65)],
        "bocf_acq_mc": [dict(acq_kind=1), dict(kind=0), dict(S_mc=1), dict(m=16, theta_dim=16), dict(m=8, H=2, best_group=1), dict(kind=4, theta_dim=1),
                        dict(kind=3, theta_dim=1, n_params=4, params_null=0), dict(kind=2, theta_dim=0, theta_null=1), dict(L=0), dict(canned=1), dict(C=0), dict(d=65)],
        "bocf_acq_mc_grad": [dict(acq_kind=2), dict(d=64), dict(canned=1), dict(S_mc=1), dict(m=16, theta_dim=16), dict(C=0)],
        "bocf_set_mc_samples": [dict(S=1), dict(m=16), dict(m=8, H=2, best_group=1), dict(canned=1), dict(L=0)],
        "bocf_set_eu_samples": [dict(S=1, L=1), dict(m=16), dict(m=8, H=2, best_group=1), dict(canned=1)],
        "bocf_expected_utility": [dict(mode=0, kind=4, eu_S=0), dict(mode=1), dict(mode=1, kind=4, theta_dim=1, eu_S=0), dict(L=1), dict(theta_dim=1, kind=2),
                                  dict(kind=3, theta_dim=1, n_params=4, params_null=0), dict(kind=2, n_params=16, params_null=0), dict(eu_L=3), dict(grad=1, d=64),
                                  dict(d=65), dict(m=8, H=2, n_hyps=2), dict(n_hyps=7), dict(m=16, theta_dim=16, eu_m=16), dict(m=8, H=2, best_group=1)],
        "bocf_acq_kg": [dict(mode=0), dict(mode=1, S_mc=0), dict(L=1), dict(L=32), dict(theta_dim=1, kind=2), dict(m=16, theta_dim=16), dict(S=1), dict(S=256),
                        dict(S_mc=1), dict(S_mc=256), dict(kg_na=1), dict(C=1), dict(d=32), dict(best_group=5), dict(kind=2, n_params=16, params_null=0), dict(m=8, H=2)],
        "bocf_acq_pending": [dict(L=1), dict(L=32), dict(S_mc=1, pd_S=1), dict(S_mc=256, pd_S=256), dict(pd_r=1), dict(C=1), dict(d=32), dict(m=8, H=2, best_group=1),
                             dict(m=16, theta_dim=16), dict(kind=0)],
        "bocf_acq_joint": [dict(q=8, C=8), dict(q=5), dict(S=1), dict(S=256), dict(C=1), dict(d=32), dict(m=8, H=2, best_group=1), dict(m=16, theta_dim=16), dict(S_mc=0),
                           dict(L=32)],
        "bocf_feasible_best": [dict(cq_K=1), dict(canned=1), dict(m=8, H=2, best_group=1), dict(m=16, theta_dim=16, cq_m=16), dict(S_mc=0), dict(C=0), dict(L=32)],
        "bocf_acq_mc_constrained": [dict(cq_K=1), dict(canned=1), dict(S_mc=1), dict(C=1), dict(grad=1, d=64), dict(d=65), dict(m=8, H=2, best_group=1)],
        "bocf_loo_utility": [dict(flags=0), dict(mode=0, kind=4, eu_S=0), dict(mode=1, eu_S=0), dict(m=8, H=2, group=1), dict(L=1, eu_L=1), dict(L=32, eu_L=32),
                             dict(m=16, theta_dim=16, eu_m=16), dict(best_group=5), dict(C=0), dict(kind=3, theta_dim=1, n_params=4, params_null=0)],
    }
    assert sorted(ok) == sorted(SEQUENCES)
    for who, cases in sorted(ok.items()):
        for case, g in zip(cases, _verdicts(driver, [_line(who, **c) for c in cases])):
            assert g == "ok %d" % (16 if case.get("m") == 16 else 4), (who, case, g)
    # no resident candidate: nothing to do for the expected utility, whatever the rows
    assert _verdicts(driver, [_line("bocf_expected_utility", C=0, rows=0, val_null=1)]) == ["nothing 4"]
    # every way to the refusals that have more than one
    many = [("bocf_set_mc_samples", dict(z_null=1), BAD_SAMPLES), ("bocf_set_mc_samples", dict(S=0), BAD_SAMPLES), ("bocf_set_eu_samples", dict(z_null=1), BAD_SAMPLES),
            ("bocf_set_eu_samples", dict(S=0), BAD_SAMPLES), ("bocf_set_eu_samples", dict(L=0), BAD_SAMPLES), ("bocf_acq_mc", dict(kind=-1), UTIL_KIND),
            ("bocf_acq_mc", dict(kind=4, theta_dim=0), "rosenbrock utility needs theta_dim >= 1 and even m"), ("bocf_expected_utility", dict(mode=-1), MODE),
            ("bocf_expected_utility", dict(theta_dim=0), "theta must be (L >= 1, theta_dim >= 1)"),
            ("bocf_expected_utility", dict(theta_null=1), "theta must be (L >= 1, theta_dim >= 1)"), ("bocf_expected_utility", dict(mode=1, kind=0), NO_CLOSED),
            ("bocf_expected_utility", dict(n_params=-1), BAD_PARAMS), ("bocf_expected_utility", dict(n_params=2), BAD_PARAMS),
            ("bocf_expected_utility", dict(rows=0), "null output / row_param"), ("bocf_expected_utility", dict(rows=3), "row_param out of range [0, L)"),
            ("bocf_acq_kg", dict(L=33), L_RANGE), ("bocf_acq_kg", dict(theta_dim=17, kind=2), THETA), ("bocf_acq_kg", dict(S=257), "Sf out of range (1 .. 256)"),
            ("bocf_acq_kg", dict(mode=-1), MODE), ("bocf_acq_joint", dict(q=9), "q out of range (1 .. 8)"), ("bocf_acq_joint", dict(S=257), "S out of range (1 .. 256)"),
            ("bocf_loo_utility", dict(flags=-1), "unknown flags (BOCF_ADD_NOISE | BOCF_CLIP)"), ("bocf_loo_utility", dict(kind=-1), UTIL_KIND),
            ("bocf_loo_utility", dict(m=8, H=2, group=2), "group out of range (-1 or 0 .. hyper_samples - 1)")]
    for (who, fault, text), g in zip(many, _verdicts(driver, [_line(who, **f) for who, f, _ in many])):
        assert g == who + ": " + text, (who, fault, g)
