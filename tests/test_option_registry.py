"""No option without a test (CPU): every option rt_debug_set_option accepts is in the registry tests/option_cases.py -- with the values
the GPU suite runs it with (tests/test_gpu_option_matrix.py, tests/fuzz_parity.py) or the reason why it is exempt -- and the registry
names no option the library has dropped.  An option added to csrc/rt_api.hip without a test fails here, on the next CPU run."""
import itertools
import os

import option_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def library_options():
    with open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", "rt_api.hip")) as f:
        return option_cases.library_options(f.read())


def test_every_option_of_the_library_is_in_the_registry_and_no_other():
    have = library_options()
    assert len(have) >= 21, "the option names could not be read from rt_debug_set_option: %r" % (have,)
    missing = [n for n in have if n not in option_cases.OPTIONS]
    gone = [n for n in option_cases.OPTIONS if n not in have]
    assert not missing, "options without an entry in tests/option_cases.py (add the values to run them with, or an exemption): %s" % missing
    assert not gone, "tests/option_cases.py names options the library no longer has: %s" % gone


def test_registry_entries_are_well_formed():
    for name, o in option_cases.OPTIONS.items():
        assert o["kind"] in ("build", "launch", "exempt"), name
        if o["kind"] == "exempt":
            assert len(o.get("reason", "")) > 20 and "values" not in o, name
        else:
            assert o["values"] and "reason" not in o, name
            for k, v in o.get("needs", {}).items():
                assert v in option_cases.OPTIONS[k]["values"], (name, k, v)
    assert sorted(n for n, o in option_cases.OPTIONS.items() if o["kind"] == "exempt") == ["dist_check_seconds", "verbose"]


def test_the_extraction_sees_an_option_that_is_added():
    """the guard's own reader, on a made-up source: a new `n == "..."` inside the function is found, one outside it is not"""
    src = 'int other() { if (n == "elsewhere") return 0; }\nextern "C" int rt_debug_set_option(rt_context *c)\n{\n    if (is(n == "lds_top")) x = 1;\n' \
          '    else if (n == "brand_new") y = 2;\n    return RT_OK;\n}\nint after() { return n == "later"; }\n'
    assert option_cases.library_options(src) == ["brand_new", "lds_top"]


def test_gpu_matrix_runs_every_registry_value():
    """The GPU module's tables against the registry: the builder rows are a pairwise cover of the builder options' values, every launch
    value has a case of its own, every remaining build value is in a row, and the fuzz draw can reach every value."""
    import test_gpu_option_matrix as M
    crossed = ["leaf_max", "fast_bvh", "wide_sah", "split_refs", "build_batch"]
    for a, b in itertools.combinations(crossed, 2):
        for va, vb in itertools.product(option_cases.OPTIONS[a]["values"], option_cases.OPTIONS[b]["values"]):
            assert any(r[a] == va and r[b] == vb for r in M.BUILD_ROWS), "no builder row with %s=%s and %s=%s" % (a, va, b, vb)
    rows = M.BUILD_ROWS + [dict(x, fail_ploc_rounds=1) for _, x, _ in M.FALLBACK_ROWS]
    for n, v in option_cases.exercised("build"):
        assert any(r.get(n) == v for r in rows), "builder option %s=%s is in no row" % (n, v)
    for n, v in option_cases.exercised("launch"):
        assert option_cases.with_needs({n: v}) in M.LAUNCH_CASES, "launch option %s=%s has no case" % (n, v)
    for combo in M.LAUNCH_COMBOS + M.TRACE_CASES:
        for n, v in combo.items():
            assert v in option_cases.OPTIONS[n]["values"], (n, v)
    # the fuzz draw: 1 - 4 options (plus what they need), values from the registry, and over many draws every value
    import numpy as np
    r = np.random.default_rng(1)
    seen = set()
    for _ in range(3000):
        opts = option_cases.draw(r)
        assert 1 <= len(opts) <= 6
        for n, v in opts.items():
            assert v in option_cases.OPTIONS[n]["values"]
            seen.add((n, repr(v)))
    assert seen == {(n, repr(v)) for n, v in option_cases.exercised()}


def test_fuzz_option_stream_leaves_the_scene_stream_alone():
    """about a third of the draws get options, from a generator of their own: the same seed gives the same options, and another stream
    than the scenes' (np.random.default_rng(seed))"""
    import fuzz_parity
    a = list(itertools.islice(fuzz_parity.option_stream(11), 100))
    assert a == list(itertools.islice(fuzz_parity.option_stream(11), 100))
    assert a != list(itertools.islice(fuzz_parity.option_stream(12), 100))
    assert 20 <= sum(1 for o in a if o) <= 47
