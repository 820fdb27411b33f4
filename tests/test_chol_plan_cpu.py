"""CPU-only checks of the factorization planner (bocf_amd/csrc/chol_plan.h): plan_cholesky decides the whole schedule of a Cholesky before
anything is enqueued.  A table of decisions pinned from the schedule rules (schedule, panel groups, team sizes), the two families where the
tail of the hybrid schedule has no team of two workgroups (planned as the launched schedule), and the plan's invariants over a sweep of
sizes, output counts, device sizes and option values.  The header is driven through tests/chol_plan_driver.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ next to hipcc")
    exe = str(tmp_path_factory.mktemp("chol_plan") / "chol_plan_driver")
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "chol_plan_driver.cpp"), "-o", exe])
    return exe


# inputs of a context on a 256-CU device with the inverse stream and working CU masks; options at their defaults
BASE = dict(ncu=256, inv_stream=1, cu_masks_ok=1, gated_off=0, sched_retry=0, refit=0, want_kinv=0)


def plans(driver, cases):
    lines = []
    for case in cases:
        kv = dict(BASE, **case)
        lines.append(" ".join("%s=%d" % (k, v) for k, v in kv.items()))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return [dict((k, int(v)) for k, v in (tok.split("=") for tok in line.split())) for line in out if line]


# (inputs and options, expected fields of the plan)
TABLE = [
    # config 2: 8 panels, 4 outputs -> ONE team launch, teams of 64 workgroups (256 CUs / 4 outputs)
    (dict(nb=8, m=4), dict(schedule=3, mb=4, T=64, T_tail=0, panels=0, kinv=0, inv_after=-1)),
    (dict(nb=8, m=4, want_kinv=1), dict(schedule=3, mb=4, T=64, kinv=1)),
    # config 3: 32 panels, 4 outputs, second fit -> hybrid: team groups of 6 panels over the first 16 block rows, tail on 5/8 of the CUs
    (dict(nb=32, m=4, refit=1), dict(schedule=5, h=16, panels=6, G=3, mb=4, T=64, T_tail=40, inv_after=15)),
    (dict(nb=32, m=4, refit=1, team_hybrid=1), dict(schedule=5, h=16, panels=0, G=3, mb=4, T=0, T_tail=40, inv_after=15)),
    # one output, 28 panels: the first fit of a context never runs a gated schedule -> hybrid; the second, CU masks accepted -> reserved chain
    (dict(nb=28, m=1), dict(schedule=5, h=16, panels=6, G=2, mb=1, T=256, T_tail=160)),
    (dict(nb=28, m=1, refit=1), dict(schedule=2, reserved_cus=8, inv_after=-1)),
    # after a time-out: the redo and every fit once gated schedules are off -> launched
    (dict(nb=32, m=4, refit=1, sched_retry=1), dict(schedule=0, G=3, flag_ints=0)),
    (dict(nb=32, m=4, refit=1, gated_off=1), dict(schedule=0, G=3, flag_ints=0)),
    (dict(nb=8, m=4, refit=1, sched_retry=1), dict(schedule=0, G=1)),
    (dict(nb=28, m=1, refit=1, gated_off=1), dict(schedule=0, G=2)),
    # teams off: launched, G by size (1 below 16 panels, 2 from 16, 3 from 32)
    (dict(nb=15, m=4, team_fit=0), dict(schedule=0, G=1, inv_after=-1)),
    (dict(nb=16, m=4, team_fit=0), dict(schedule=0, G=2, inv_after=-1)),
    (dict(nb=32, m=4, team_fit=0), dict(schedule=0, G=3, inv_after=15)),
    # reserved chain forced: applies on a second fit with CU masks, not when the runtime refused them
    (dict(nb=26, m=4, refit=1, lookahead=2), dict(schedule=2, reserved_cus=8, inv_after=15, flag_ints=132, err_off=130)),
    (dict(nb=26, m=4, refit=1, lookahead=2, cu_masks_ok=0), dict(schedule=0, G=2, inv_after=15)),
    # the two families that changed: the hybrid's tail would get teams of one workgroup -> the launched schedule, before anything is enqueued
    (dict(nb=25, m=2, ncu=6), dict(schedule=0, G=2, inv_after=15)),
    (dict(nb=25, m=2, force_cu_count=6), dict(schedule=0, G=2, inv_after=15)),
    (dict(nb=32, m=65), dict(schedule=0, G=3)),
    (dict(nb=32, m=64), dict(schedule=5, mb=64, T_tail=2)),
]


def test_pinned_decisions(driver):
    got = plans(driver, [case for case, _ in TABLE])
    for (case, want), plan in zip(TABLE, got):
        assert {k: plan[k] for k in want} == want, (case, plan)


def test_team_counter_layout(driver):
    """Team schedules: per-output counters (4 nb + 4 nb^2 ints, rounded to 16 bytes), then the time-out word and three spare ints."""
    for nb, m in ((8, 4), (32, 4), (25, 3)):
        words = ((4 * nb + 4 * nb * nb + 3) // 4) * 4
        plan = plans(driver, [dict(nb=nb, m=m, refit=1)])[0]
        assert plan["schedule"] in (3, 5)
        assert plan["err_off"] == m * words and plan["flag_ints"] == m * words + 4


def test_invariants_over_the_sweep(driver):
    """Every team launch has teams of at least two workgroups that are all resident at once; a hybrid plan has both parts applicable;
    the time-out word lies inside the counter block; no gated schedule after a time-out."""
    r = subprocess.run([driver, "--sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "violations 0" in r.stdout, r.stdout
