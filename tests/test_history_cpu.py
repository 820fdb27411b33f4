"""The catalogue of the call-history tests (tests/history_calls.py) is complete and well-formed.  No device: the header is parsed, the
inputs are generated, the calls' sources are read; nothing is run."""
import collections
import inspect
import os
import re

import numpy as np
import pytest

import history_calls as H
from bocf_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2), (5, 3), (2, 1), (2, 2)]                 # (d, m) of the problems of tests/test_gpu_history.py


def header_functions():
    """Every function include/bocf_hip.h declares (comments removed; the callback typedef is no function)."""
    with open(os.path.join(ROOT, "include", "bocf_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return set(re.findall(r"^\s*(?:int|void|const\s+char\s*\*)\s*(bocf_\w+)\s*\(", text, flags=re.M))


def test_the_header_parse_finds_what_the_binding_declares():
    assert header_functions() == set(_ffi.SIGNATURES)
    assert len(header_functions()) > 70


def test_every_entry_point_is_catalogued_or_excluded_with_a_reason():
    declared = header_functions()
    reached = {e for c in H.CALLS.values() for e in c.entries}
    assert reached <= declared, sorted(reached - declared)
    assert set(H.EXCLUDED) <= declared, sorted(set(H.EXCLUDED) - declared)
    assert not reached & set(H.EXCLUDED), sorted(reached & set(H.EXCLUDED))
    missing = declared - reached - set(H.EXCLUDED)
    assert not missing, "entry points that no call of tests/history_calls.py reaches and EXCLUDED does not explain: %s" % sorted(missing)
    for name, reason in H.EXCLUDED.items():
        assert isinstance(reason, str) and len(reason.strip()) > 10 and "\n" not in reason, name


def test_every_call_declares_entries_and_known_sizes_and_options():
    options = {o[0] for o in _ffi.options()}
    for c in H.CALLS.values():
        assert c.entries, c.name
        assert set(c.sizes) <= set(H.SIZES), c.name
        assert len(set(c.sizes)) == len(c.sizes), c.name
        assert set(c.options) <= options, c.name
        src = inspect.getsource(c.fn)
        for o in c.options:
            assert '"%s"' % o in src, (c.name, o)
        assert bool(c.options) == ("set_option" in src or "_with_option" in src), c.name


# what the issue lists, family by family
FAMILIES = {
    "predict": ["posterior_mean", "predict_tile", "predict_small", "predict_full_cov", "predict_f32", "predict_i8", "gradients_small",
                "gradients_tile", "mean_at_train"],
    "improvement": ["acq_linear_ei", "acq_linear_pi", "acq_linear_grad", "acq_mc_ei", "acq_mc_pi", "acq_mc_program", "acq_mc_grad", "acq_mc_topk"],
    "look-ahead": ["kg_closed", "kg_closed_grad", "kg_mc", "kg_mc_grad", "cov_precomputed", "conditioned_variance", "covariance_gradient",
                   "posterior_cov"],
    "pending": ["pending", "pending_grad"],
    "joint": ["joint", "joint_grad"],
    "constrained": ["constrained_mc", "constrained_mc_grad", "constrained_eu"],
    "recommendation": ["eu_mean", "eu_closed", "eu_mc", "eu_mc_grad"],
    "risk and log": ["risk_quantile", "risk_tail_mean", "linear_ucb", "log_linear", "log_mc"],
    "samples": ["posterior_samples", "thompson_topk", "paths"],
    "refinement": ["refine_linear", "refine_mc"],
    "diagnostics": ["loo", "loo_utility", "lml_gradients", "factor"],
}


def test_every_family_is_in_the_catalogue_and_nothing_else():
    listed = [n for names in FAMILIES.values() for n in names]
    assert sorted(listed) == sorted(H.CALLS)


def test_the_two_variants_differ_in_every_size():
    for name, (a, b) in H.SIZES.items():
        assert a != b and a >= 1 and b >= 1, name
    for c in H.CALLS.values():
        sa, sb = c.sizes_of("a"), c.sizes_of("b")
        assert set(sa) == set(sb) == set(c.sizes)
        for s in c.sizes:
            assert sa[s] != sb[s], (c.name, s)


def test_both_variants_stay_within_the_documented_limits():
    for name, limit in H.LIMITS.items():
        assert max(H.SIZES[name]) <= limit, name
    assert H.SIZES["Cs"][1] == 16 and H.SIZES["C"][0] > 16 and H.SIZES["A"][0] <= 16 < H.SIZES["A"][1]      # both sides of the small path
    assert H.SIZES["C"][0] < 128 < H.SIZES["C"][1] and H.SIZES["na"][0] < 128 < H.SIZES["na"][1] and H.SIZES["F"][0] < 128 < H.SIZES["F"][1]
    for c in H.CALLS.values():
        for v in H.VARIANTS:
            n = c.sizes_of(v)
            rows = n.get("C") or n.get("Cs") or n.get("A") or (n["B"] * n["q"] if "B" in n else None)
            if "k" in n:
                assert n["k"] <= min(rows, H.LIMITS["k"]), (c.name, v)
            if "B" in n:
                assert rows <= H.JOINT_GRAD_POINTS, (c.name, v)
            if "S" in n and c.name.startswith("risk"):
                assert 0 <= n["S"] // 4 <= n["S"] - 1


@pytest.mark.parametrize("d,m", SHAPES)
def test_inputs_are_deterministic_and_have_the_declared_sizes(d, m):
    make = H._inputs.__wrapped__                          # (past the cache: two independent generations)
    for c in H.CALLS.values():
        for v in H.VARIANTS:
            one, two = make(c.name, c.sizes, v, d, m), make(c.name, c.sizes, v, d, m)
            assert one.keys() == two.keys()
            for key in one:
                if isinstance(one[key], np.ndarray):
                    assert one[key].tobytes() == two[key].tobytes() and one[key].shape == two[key].shape, (c.name, v, key)
                    assert np.all(np.isfinite(one[key])), (c.name, v, key)
                else:
                    assert one[key] == two[key], (c.name, v, key)
            n = c.sizes_of(v)
            assert one["n"] == n
            rows = n.get("C") or n.get("Cs") or n.get("A") or (n["B"] * n["q"] if "B" in n else None)
            want = {"X": (rows, d), "W": (n.get("S"), m), "thetas": (n.get("L"), m), "prob": (n.get("L"),), "rows": (rows or 0,),
                    "Zeu": (n.get("L"), n.get("S"), m), "A": (n.get("na"), d), "Zf": (n.get("Sf"), m), "P": (n.get("r"), d),
                    "Zp": (n.get("S"), m, n.get("r")), "Zq": (n.get("S"), m, n.get("q")), "thetasP": (n.get("P"), m),
                    "Zpath": (n.get("P"), m, rows), "row_path": (rows,), "Zs": (m, rows, n.get("S")), "cA": (n.get("K"), m), "x1": (1, d)}
            for key, shape in want.items():
                if key in one:
                    assert one[key].shape == shape, (c.name, v, key, one[key].shape, shape)
            if "prob" in one:
                assert abs(one["prob"].sum() - 1.0) < 1e-12 and np.all(one["prob"] > 0)
            if "rows" in one and one["rows"].size:
                assert one["rows"].min() >= 0 and one["rows"].max() < n["L"]
            if "row_path" in one:
                assert one["row_path"].min() >= 0 and one["row_path"].max() < n["P"]
        # the variants are different problems, not one sliced
        a, b = c.inputs("a", d, m), c.inputs("b", d, m)
        if "X" in a:
            assert a["X"].shape != b["X"].shape
    assert H.CALLS["acq_mc_ei"].inputs("a", d, m)["X"].tobytes() != H.CALLS["acq_mc_pi"].inputs("a", d, m)["X"].tobytes()      # keyed by the call's name


@pytest.mark.parametrize("d,m", SHAPES)
def test_the_shared_twin_hands_the_same_arrays_to_every_call(d, m):
    make = H._inputs.__wrapped__
    seen = {}
    for c in H.CALLS.values():
        for v in H.VARIANTS:
            own, twin = c.inputs(v, d, m), c.inputs(v, d, m, shared=True)
            again = make(c.name, c.sizes, v, d, m, True)
            assert own.keys() == twin.keys() and own["n"] == twin["n"]
            for key, a in twin.items():
                if not isinstance(a, np.ndarray):
                    assert a == own[key], (c.name, v, key)
                    continue
                assert a.shape == own[key].shape and a.dtype == own[key].dtype and a.tobytes() == again[key].tobytes(), (c.name, v, key)
                if key in H.SHARED:
                    first = seen.setdefault((key, a.shape, twin["n"].get("L") if key == "rows" else None), (c.name, a))
                    assert first[1].tobytes() == a.tobytes(), (c.name, first[0], key)
            if "prob" in twin:
                assert abs(twin["prob"].sum() - 1.0) < 1e-12
            if twin.get("rows") is not None and twin["rows"].size:
                assert twin["rows"].max() < twin["n"]["L"]
    users = collections.Counter(key for key, _, _ in seen)
    assert users["X"] >= 2 and users["W"] >= 2 and users["thetas"] >= 2                  # (both variants of each)
    # ... and they really are shared: the Monte-Carlo acquisitions of a variant get one X, one W, one theta
    a, b = H.CALLS["acq_mc_ei"].inputs("b", d, m, shared=True), H.CALLS["kg_mc"].inputs("b", d, m, shared=True)
    for key in ("X", "W", "thetas", "prob"):
        assert a[key].tobytes() == b[key].tobytes()


def test_no_call_leans_on_resident_state_or_the_global_random_stream():
    helpers = [H._both_predicts, H._gradients, H._kg, H._constrained_mc, H._constraints, H._refined, H._with_option, H._utility, H._path_groups]
    for fn in [c.fn for c in H.CALLS.values()] + helpers:
        src = inspect.getsource(fn)
        assert not re.search(r"\b(W|Z|X|X0|Zf|Zp|thetas|prob)\s*=\s*None\b", src), src
        assert not re.search(r"\bNone\s*,\s*\d", src), src                 # (no positional None in front of a candidate count)
        assert "np.random" not in src and "numpy.random" not in src, src
        for first in re.findall(r"model\.(?:predict|predict_noiseless|posterior_\w+|acq_\w+|expected_utility\w*|path_values|path_utility|"
                                r"pathwise_topk|thompson_topk|refine_acq)\(\s*([^,)]+)", src):
            assert first.strip() != "None", src
    # every X a call hands over is its own input
    for c in H.CALLS.values():
        src = inspect.getsource(c.fn)
        if c.sizes and c.name != "loo_utility":
            assert 'i["X"]' in src, c.name
    # the one call that has to feed the global stream seeds it from its inputs and puts it back
    state = np.random.get_state()
    with H.seeded_global_stream(5):
        first = np.random.normal(size=3)
    with H.seeded_global_stream(5):
        assert np.array_equal(np.random.normal(size=3), first)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]


def test_the_program_blob_is_accepted_by_the_host_check():
    for m in (1, 2, 3):
        blob = H.program_blob(m)
        assert _ffi.load().bocf_check_utility_program(blob, len(blob), m, m) == 0
