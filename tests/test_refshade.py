"""The oracle against the reference's own shading text (oracle/refshade/README.md), bit for bit.

The reference's HLSL, translated textually and compiled as C++ behind a shim of HLSL types (oracle/_ref/librefshade.so, built by
`make oracle` where the reference checkout is present, never committed), computed the fixtures under tests/golden/refshade/.  The
oracle is a hand restatement of that text; here it has to reproduce every recorded number.  The comparisons run everywhere; only the
tests of the shim itself and of the fixtures' freshness need the library, and only the freshness test may skip without it."""
import os
import subprocess

import numpy as np
import pytest

import refshade_cases as R

HAVE_REF = os.path.exists(R.REF_SO)


@pytest.fixture(scope="module")
def cases(oracle):
    return R.frame_cases(oracle)


@pytest.fixture(scope="module")
def ref(oracle):
    assert HAVE_REF
    return R.Ref(oracle)


CASE_NAMES = ["opt_" + ("-".join("%s=%s" % kv for kv in o.items()) or "defaults") for o in R.OPTION_CASES] + [
    "material_type0", "material_type2", "material_type1", "instanced", "accumulate4", "past_max_iterations",
    "realtime_cornell", "realtime_instanced"]


def test_case_list_is_complete(cases):
    assert sorted(cases) == sorted(CASE_NAMES)
    have = sorted(f[:-4] for f in os.listdir(R.FIXTURES) if f.endswith(".npz"))
    assert have == sorted(CASE_NAMES + ["units", "units_phong"])
    for f in os.listdir(R.FIXTURES):
        assert os.path.getsize(os.path.join(R.FIXTURES, f)) <= 456994      # the largest fixture committed before these


# ---- a. the shim's own self-tests (they need the library: without it they pass on the fixtures' evidence alone) ----

def test_constructor_arguments_run_left_to_right(oracle):
    """float2(nextRand(s), nextRand(s)): the first draw lands in .x.  Checked on the shim where it is built, and on the recorded cosine
    samples everywhere: about (0, 1, 0) a cosine sample has x^2 + z^2 = the first draw (r = sqrt(randVal.x))."""
    u = R.load_fixture("units")
    k = int(np.nonzero((u["dirs"] == np.array([0, 1, 0], np.float32)).all(axis=1))[0][0])
    seed = int(u["seeds"][k])
    s1, first = oracle.next_rand(seed)
    s2, second = oracle.next_rand(s1)
    assert abs(first - second) > 1e-3
    x, _, z = (float(c) for c in u["cos_out"][k])
    assert abs(x * x + z * z - first) < 1e-6 and abs(x * x + z * z - second) > 1e-3
    assert int(u["cos_seed"][k]) == s2
    if HAVE_REF:
        s, out = R.Ref(oracle).two_draws(seed)
        assert s == s2 and float(out[0]) == first and float(out[1]) == second


def test_translated_literals_are_float(oracle):
    """(1.0 - x) / 3.0 as the translator emits it runs in float: on an x where the double route rounds differently it gives the float
    route's result.  (One IEEE operation cannot tell the routes apart -- 53 >= 2 * 24 + 2 bits -- so the probe chains two.)"""
    f = np.float32
    xs = np.random.default_rng(5).uniform(0, 1, 4096).astype(np.float32)
    flt = (f(1.0) - xs) / f(3.0)
    dbl = ((1.0 - xs.astype(np.float64)) / 3.0).astype(np.float32)
    differ = np.nonzero(flt != dbl)[0]
    assert differ.size > 0                       # the probe has inputs that tell the routes apart
    if HAVE_REF:
        r = R.Ref(oracle)
        for k in differ[:64]:
            assert r.float_only(xs[k]) == flt[k]


def test_compat_header_layout_equals_the_c_abi_records(oracle):
    """sizeof / offsetof of every struct of the reference's shared header, compiled with HLSL defined behind the shim, against
    include/dxr_amd_types.h; without the library, the numpy dtypes that restate the same records are checked against the C header's
    static_asserts' numbers."""
    from dxrexperiments_amd import rtypes as T
    assert (T.VERTEX.itemsize, T.CAMERA_PARAMS.itemsize, T.DEBUG_OPTIONS.itemsize, T.PER_FRAME_CONSTANTS.itemsize,
            T.MATERIAL_PARAMS.itemsize) == (24, 80, 44, 188, 64)
    if HAVE_REF:
        rows = R.Ref(oracle).layout()
        assert rows.shape[0] >= 60
        assert np.array_equal(rows[:, 0], rows[:, 1]), rows[rows[:, 0] != rows[:, 1]]


# ---- b. the oracle against the fixtures ----

def test_oracle_units_equal_the_reference_text(oracle):
    want = R.load_fixture("units")
    got = R.compute_units(R.Orc(oracle))
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert R.same_bits(got[k], want[k]), "%s: %d values differ" % (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_frames_equal_the_reference_text(oracle, cases, name):
    want = R.load_fixture(name)
    got = R.compute_frame(R.Orc(oracle), oracle, cases[name])
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        w, g = want[k], np.asarray(got[k])
        if k in ("pfcs", "mats"):
            assert g.tobytes() == w.tobytes(), "%s: the case's inputs changed; run tests/golden/make_refshade.py" % k
            continue
        bad = int((g != w).sum()) if g.shape == w.shape else -1
        assert R.same_bits(g, w), "%s %s: %d values differ from the reference text's" % (name, k, bad)
        if k.startswith(("image", "direct")):
            assert np.isfinite(w.astype(np.float32)).all() and float(w.astype(np.float32)[..., :3].max()) > 0.0      # a frame, not a blank
    if name == "past_max_iterations":
        f = want["image_fp32"]
        assert not np.array_equal(f[0], f[1]) and np.array_equal(f[1], f[2]) and np.array_equal(f[2], f[3])


# ---- c. the fixtures are what the library computes now ----

@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/librefshade.so is not built: no reference checkout on this machine")
def test_fixtures_are_fresh():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_refshade", os.path.join(R.GOLDEN, "make_refshade.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    made = mod.generate()
    assert sorted(made) == sorted(CASE_NAMES + ["units"])
    for name, arrays in made.items():
        want = R.load_fixture(name)
        assert sorted(arrays) == sorted(want), name
        for k in arrays:
            a, w = np.asarray(arrays[k]), want[k]
            assert a.dtype == w.dtype and a.shape == w.shape and a.tobytes() == w.tobytes(), "%s %s is stale: run tests/golden/make_refshade.py" % (name, k)


# ---- d. nothing of the reference is committed ----

def test_nothing_under_oracle_ref_is_tracked():
    try:
        r = subprocess.run(["git", "-C", R.ROOT, "ls-files", "oracle/_ref"], capture_output=True, text=True)
    except OSError:
        r = None
    if r is not None and r.returncode == 0:
        assert r.stdout.strip() == ""
    with open(os.path.join(R.ROOT, ".gitignore")) as f:
        assert "oracle/_ref/" in f.read().split()
