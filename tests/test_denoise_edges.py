"""The two statements of the DenoiseCompositor -- oracle/oracle_shade.h, what the kernels of rt_denoise.hip are compared with, and
tests/golden/nversion_denoise.py, written from the HLSL text in vectorised numpy -- against each other at the edges (denoise_cases.py): every
shape that straddles the kernels' tiles and halo x every radius, every input family (impulses and steps at the tile seams; black texels, negative
values, -0, subnormals, sums that overflow; +-inf and NaN) x every radius at two shapes, and the parameter edges.  Both passes, bit for bit, the
sign of a zero included; where both hold a NaN any payload passes.  No GPU.

pow() is the one operation HLSL leaves to the driver; the engine defines it (oracle_math.h pow_, held to float64 by
test_oracle.py), so the second statement is handed that definition as its pow and the composite after gamma is compared by bits as well."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import denoise_cases as DC                               # noqa: E402
import nversion_denoise as ND                            # noqa: E402

CASES = DC.enumeration()
_inputs = {}


def inputs(family, shape):
    if (family, shape) not in _inputs:
        d, i = DC.FAMILIES[family](*shape)
        d.setflags(write=False); i.setflags(write=False)
        _inputs[family, shape] = d, i
    return _inputs[family, shape]


@pytest.mark.parametrize("name,family,shape,over", CASES, ids=[c[0] for c in CASES])
def test_oracle_and_second_statement_agree_at_the_edges(oracle, name, family, shape, over):
    direct, indirect = inputs(family, shape)
    p = DC.default_params(oracle.DENOISE_PARAMS)
    for k, v in over.items():
        p[k] = v
    oh, ov = oracle.denoise(direct, indirect, p)
    nh, nv = ND.denoise(direct, indirect, p["exposure"], p["gamma"], p["tonemap"], p["gammaCorrect"], p["maxKernelSize"], p["debugVisualize"],
                        pow=lambda x, y: oracle.math("pow", x, y))
    assert DC.equal_bits(oh, nh, "pass H")
    assert DC.equal_bits(ov, nv, "pass V")
    assert (oh[..., 3] == 1.0).all() and (ov[..., 3] == 1.0).all()


def test_the_enumeration_is_what_it_claims():
    """every shape x radius, every family x radius at the two family shapes, every parameter edge; the 5-tap unroll's residues all occur; the hostile
    families hold every class they name, and black texels at the same place in both images"""
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)
    have = {(f, s, o["maxKernelSize"]) for _, f, s, o in CASES if list(o) == ["maxKernelSize"]}
    assert {case_id for case_id in map(DC.case_id, DC.PARAM_EDGES)} <= {DC.case_id(o) for _, f, s, o in CASES if s == DC.PARAM_SHAPE}
    assert all(("benign", s, k) in have for s in DC.SHAPES for k in DC.RADII)
    assert all((f, s, k) in have for f in DC.FAMILIES for s in DC.FAMILY_SHAPES for k in DC.RADII)
    assert {(2 * k + 1) % 5 for k in DC.RADII} == {0, 1, 2, 3, 4}
    assert all(s[0] * s[1] < 70000 for s in DC.SHAPES)
    for shape in DC.FAMILY_SHAPES + [DC.PARAM_SHAPE]:
        d, i = DC.hostile_nonfinite(*shape)
        for img in (d, i):
            assert np.isposinf(img).any() and np.isneginf(img).any() and np.isnan(img).any()
        d, i = DC.hostile_finite(*shape)
        for img in (d, i):
            u = img.view(np.uint32)
            assert np.isfinite(img).all() and (u == 0x80000000).any() and (img < 0).any() and (img >= 1e3).any() and (img > 1e38).any()
            assert ((u & 0x7F800000 == 0) & (u & 0x7FFFFF != 0)).any()
        assert ((d[..., :3] == 0).all(axis=2) & (i[..., :3] == 0).all(axis=2)).any()
        d2, i2 = DC.hostile_finite(*shape)
        assert d.tobytes() == d2.tobytes() and i.tobytes() == i2.tobytes()
    d, i = DC.impulse(513, 129)
    for y, x in ((0, 0), (128, 512), (64, 256), (32, 255), (96, 256), (32, 7), (96, 8), (63, 128), (64, 384), (32, 511), (96, 512)):
        assert i[y, x, 0] == 1.0, (y, x)
    assert i[..., 0].sum() == len(DC.impulse_texels(513, 129))


def test_equal_bits_sees_signs_and_payloads():
    a = np.array([[[0.0, 1.0, np.nan, np.inf]]], np.float32)
    b = a.copy()
    assert DC.equal_bits(a, b)
    b.view(np.uint32)[0, 0, 2] = 0x7FC00001               # another NaN payload passes
    assert DC.equal_bits(a, b)
    b[0, 0, 0] = -0.0
    with pytest.raises(AssertionError, match="1 of 4 values differ.*\\(0, 0, 0\\)"):
        DC.equal_bits(a, b, "zero")
    b[0, 0, 0] = 0.0
    b[0, 0, 2] = 3.0
    with pytest.raises(AssertionError):
        DC.equal_bits(a, b)                               # a NaN against a number
    with pytest.raises(AssertionError):
        DC.equal_bits(a.astype(np.float16), b.astype(np.float16))
    assert DC.equal_bits(a.astype(np.float16), a.astype(np.float16))


def test_hlsl_min_max_of_the_second_statement():
    """the rule stated in nversion_denoise.py: the non-NaN operand; -0 < +0"""
    nan, f = np.float32(np.nan), np.float32
    bits = lambda x: np.asarray(x, np.float32).view(np.uint32).tolist()       # noqa: E731
    a = np.array([nan, 2.0, nan, -0.0, 0.0, -1.0, np.inf], np.float32)
    b = np.array([1.0, nan, nan, 0.0, -0.0, -2.0, 3.0], np.float32)
    assert bits(ND.hlsl_max(a, b)[[0, 1, 3, 4, 5, 6]]) == bits([1.0, 2.0, 0.0, 0.0, -1.0, np.inf]) and np.isnan(ND.hlsl_max(a, b)[2])
    assert bits(ND.hlsl_min(a, b)[[0, 1, 3, 4, 5, 6]]) == bits([1.0, 2.0, -0.0, -0.0, -2.0, 3.0]) and np.isnan(ND.hlsl_min(a, b)[2])
    assert bits(ND.hlsl_saturate(np.array([nan, -0.0, -3.0, 0.25, 7.0, np.inf, -np.inf], np.float32))) == bits([0.0, 0.0, 0.0, 0.25, 1.0, 1.0, 0.0])
    assert bits(ND.hlsl_max(f(nan), f(0.0))) == bits(0.0)
