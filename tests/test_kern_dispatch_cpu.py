"""CPU-only checks of the kernel dispatch (bocf_amd/csrc/kern_dispatch.h): how a runtime (input dimension, kernel id) reaches the <D, family>
instantiation of a kernel, that a dimension outside 1 ... 32 is reported and not silently dropped, and how a list of per-output kernel ids
is cut into runs of one launch each.  The header is driven through tests/kern_dispatch_driver.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FAMILY = {0: 0, 1: 0, 2: 2, 3: 3}      # kernel ids 0 (RBF) and 1 (SE) are one family


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ next to hipcc")
    exe = str(tmp_path_factory.mktemp("kern_dispatch") / "kern_dispatch_driver")
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "kern_dispatch_driver.cpp"), "-o", exe])
    return exe


def run(driver, *args):
    out = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.split("\n") if line]


def test_every_dimension_and_id_reaches_its_instantiation(driver):
    got = {(int(l[0]), int(l[1])): l[2:] for l in run(driver, "dispatch")}
    assert sorted(got) == [(d, i) for d in range(34) for i in range(4)]
    for (d, i), reached in got.items():
        if 1 <= d <= 32:
            assert reached == [str(d), str(FAMILY[i])], (d, i, reached)
        else:
            assert reached == ["none"], (d, i, reached)


def runs(driver, kernel_id, kids=None, m=None):
    args = ["null", m] if kids is None else kids
    return [tuple(int(t) for t in l) for l in run(driver, "runs", kernel_id, *args)]


def test_family_runs(driver):
    # no list: one run of every output with the model's kernel id, whatever it is (the family mapping is bocf_dispatch_family's)
    assert runs(driver, 2, m=5) == [(0, 5, 2)]
    assert runs(driver, 1, m=1) == [(0, 1, 1)]
    # a list overrides the model's id; equal neighbours share a run; ids 0 and 1 are different ids and not merged here
    assert runs(driver, 0, kids=[3, 3, 3, 3]) == [(0, 4, 3)]
    assert runs(driver, 0, kids=[2, 0, 0, 3, 1, 2]) == [(0, 1, 2), (1, 2, 0), (3, 1, 3), (4, 1, 1), (5, 1, 2)]
    assert runs(driver, 3, kids=[2]) == [(0, 1, 2)]
