"""The post chain on the GPU at its edges: the DenoiseCompositor kernels (rt_denoise.hip: k_denoise_h, k_denoise_v) against the oracle over the
enumeration of denoise_cases.py -- shapes that straddle the 256 x 1 blocks, the 8 x 64 tiles and the 20-texel halo, every residue of the 5-tap
unroll, impulses and steps at the tile seams, black texels, negative values, -0, subnormals, overflowing sums, +-inf, NaN, the parameter edges --,
and the three places where the device rounds binary32 to binary16 (k_denoise_f16, k_f32_to_f16, accumulate()'s RGBA16F storage under both
roundings) against numpy's float16 and the oracle's round_to_half over half_cases.py: every half, every tie, subnormals, 65504 / 65520, overflow,
inf, NaN.  Every comparison is equal_bits: the same bits, the sign of a zero included; where both sides hold a NaN any payload passes.
test_denoise_edges.py holds the oracle to the second statement of the shaders over the same enumeration."""
import numpy as np
import pytest

import denoise_cases as DC
import half_cases
from dxrexperiments_amd import rtypes as T, scenes
from util import cam_array

pytestmark = pytest.mark.gpu

GROUPS = DC.groups()


def set_params(dn, prm):
    for k in prm.dtype.names:
        dn.params[k] = prm[k]


def check_dispatch(dn, oracle, td, ti, direct, indirect, prm, what):
    set_params(dn, prm)
    dn.dispatch(td.ptr, ti.ptr)
    oh, ov = oracle.denoise(direct, indirect, prm)
    assert DC.equal_bits(dn.read_intermediate(), oh, what + " pass H")
    assert DC.equal_bits(dn.read_output(), ov, what + " pass V")


@pytest.mark.parametrize("name,family,shape,overs", GROUPS, ids=[g[0] for g in GROUPS])
def test_denoiser_kernels_equal_the_oracle_at_the_edges(gpu, capi, oracle, name, family, shape, overs):
    """one denoiser object and one upload per (family, shape); the dispatches differ in their parameters only"""
    W, H = shape
    direct, indirect = DC.FAMILIES[family](W, H)
    dn = capi.Denoiser(gpu)
    dn.create_output(W, H)
    td, ti = gpu.upload(direct), gpu.upload(indirect)
    failed = []
    for over in overs:
        prm = DC.default_params(oracle.DENOISE_PARAMS)
        for k, v in over.items():
            prm[k] = v
        try:
            check_dispatch(dn, oracle, td, ti, direct, indirect, prm, "%s %s" % (name, DC.case_id(over)))
        except AssertionError as e:                      # every parameter set is run and named, not only the first that differs
            failed.append(str(e))
    assert not failed, "%d of %d parameter sets differ:\n%s" % (len(failed), len(overs), "\n".join(failed))


def test_denoiser_output_created_again_at_other_sizes(gpu, capi, oracle):
    """513 x 129 -> 7 x 3 -> 277 x 63 on one object: every dispatch equals the oracle's; one whose size is not the output resource's is refused"""
    dn = capi.Denoiser(gpu)
    prm = DC.default_params(oracle.DENOISE_PARAMS)
    for (W, H), K in (((513, 129), 12), ((7, 3), 20), ((277, 63), 7)):
        direct, indirect = DC.hostile_finite(W, H, seed=W)
        td, ti = gpu.upload(direct), gpu.upload(indirect)
        dn.create_output(W, H)
        prm["maxKernelSize"] = K
        check_dispatch(dn, oracle, td, ti, direct, indirect, prm, "%dx%d" % (W, H))
        for w, h in ((W + 1, H), (W, H + 1), (W - 1, H), (H, W)):
            with pytest.raises(capi.RtError):
                capi._check(capi.lib().rt_denoiser_dispatch(dn.h, td.ptr, ti.ptr, w, h))
        assert DC.equal_bits(dn.read_output(), oracle.denoise(direct, indirect, prm)[1], "after the refused dispatches")


@pytest.mark.parametrize("family", ("benign", "hostile_finite"))
def test_denoiser_with_one_buffer_as_both_inputs(gpu, capi, oracle, family):
    W, H = 277, 63
    img = DC.FAMILIES[family](W, H)[1]
    dn = capi.Denoiser(gpu)
    dn.create_output(W, H)
    t = gpu.upload(img)
    for K in (3, 12):
        prm = DC.default_params(oracle.DENOISE_PARAMS)
        prm["maxKernelSize"] = K
        check_dispatch(dn, oracle, t, t, img, img, prm, "aliased K=%d" % K)


# ---- binary32 -> binary16 on the device ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def half_image():
    img = half_cases.image()
    with np.errstate(over="ignore"):
        want = img.astype(np.float16)
    img.setflags(write=False); want.setflags(write=False)
    return img, want


def test_denoiser_f16_read_out_rounds_to_nearest_even(gpu, capi, half_image):
    """k_denoise_f16.  debugVisualize = 2 without tone map and gamma and with exposure 1 hands the input's RGB through both passes (x * 1 is x),
    which the fp32 denoiser shows first; the RGBA16F denoiser's two read-outs are then the conversion of the value set itself"""
    img, want = half_image
    H, W = img.shape[:2]
    t = gpu.upload(img)
    for fmt in (T.FORMAT_R32G32B32A32_FLOAT, T.FORMAT_R16G16B16A16_FLOAT):
        dn = capi.Denoiser(gpu)
        dn.create_output(W, H, fmt)
        dn.params["debugVisualize"], dn.params["tonemap"], dn.params["gammaCorrect"], dn.params["exposure"] = 2, 0, 0, 1.0
        dn.dispatch(t.ptr, t.ptr)
        for which, got in (("pass H", dn.read_intermediate()), ("pass V", dn.read_output())):
            assert DC.equal_bits(got, img if fmt == T.FORMAT_R32G32B32A32_FLOAT else want, "%s, format %d" % (which, fmt))


def test_pipeline_f16_read_out_rounds_to_nearest_even(gpu, capi, half_image):
    """k_f32_to_f16: the RGBA16F view of the progressive pipeline's fp32 accumulation image"""
    img, want = half_image
    p = capi.Pipeline(gpu)
    p.create_output(img.shape[1], img.shape[0], T.FORMAT_R16G16B16A16_FLOAT)
    p.write_output(img)
    assert DC.equal_bits(p.read_output(), want, "RGBA16F read-out")


@pytest.mark.parametrize("rounding", (T.ROUND_NEAREST_EVEN, T.ROUND_TOWARD_ZERO), ids=("nearest_even", "toward_zero"))
def test_accumulation_storage_rounding_over_the_value_set(gpu, capi, oracle, half_image, rounding):
    """accumulate() of rt_pipeline.hip with the mean stored as RGBA16F.  One triangle behind the camera and a black environment: every pixel
    misses, cur = (0, 0, 0, 1).  The frame with accumCount 1 on prev = 2 x values (exact; inf and NaN stay) stores round((1 * prev + 0) / 2) =
    round(values); -0 alone arrives as +0 (-0 + 0).  Held to the oracle's twin, and independently to numpy's float16 (nearest even) and the oracle's
    round_to_half, itself held to IEEE by test_round_to_half_is_ieee (toward zero: 65504 is the end, not infinity).  Then two frames through
    render_batch, the other path to the same rounding."""
    img, _ = half_image
    H, W = img.shape[:2]
    f16 = 1 if rounding == T.ROUND_NEAREST_EVEN else 2
    v = np.zeros(3, T.VERTEX)
    v["position"] = [(-1, -1, 10), (1, -1, 10), (0, 1, 10)]
    v["normal"] = (0, 0, 1)
    idx = np.array([[0, 1, 2]], np.uint32)
    mat = T.default_material()
    sc = capi.Scene(gpu)
    sc.add_model(capi.Model(gpu, v, idx))
    p = capi.Pipeline(gpu)
    p.set_scene(sc)
    p.add_material(mat)
    p.set_environment_constant((0.0, 0.0, 0.0))
    p.create_output(W, H)
    p.build_acceleration_structures()
    p.set_accumulation_storage(T.FORMAT_R16G16B16A16_FLOAT, rounding)
    osc = oracle.Scene()
    osc.add_instance(osc.add_model(v, idx))
    osc.build()
    host = capi.ProgressiveHost(7)
    cam = cam_array(scenes.cornell_camera(), W / H)
    black = (0.0, 0.0, 0.0)

    pfc = host.update(cam, 0.0, 1, W, H)
    assert int(pfc["cameraParams"]["accumCount"]) == 0
    p.update(pfc)
    p.render()
    acc, st = osc.render(mat, pfc, W, H, env_constant=black, accum_f16=f16, nthreads=8)
    assert st["primary_hits"] == 0
    assert DC.equal_bits(p.read_output(), acc, "first frame")

    prev = img * np.float32(2.0)
    p.write_output(prev)
    pfc = host.update(cam, 0.0, 2, W, H)
    assert int(pfc["cameraParams"]["accumCount"]) == 1
    p.update(pfc)
    p.render()
    got = p.read_output()
    acc, st = osc.render(mat, pfc, W, H, accum=prev.copy(), env_constant=black, accum_f16=f16, nthreads=8)
    assert st["primary_hits"] == 0
    assert DC.equal_bits(got, acc, "mean of 2 x values and 0")
    with np.errstate(over="ignore", invalid="ignore"):
        mean = (np.float32(1.0) * prev[..., :3] + np.float32(0.0)) / np.float32(2.0)
        assert DC.equal_bits(mean, img[..., :3] + np.float32(0.0), "the mean is the value set")          # (+ 0: -0 -> +0)
        want = mean.astype(np.float16).astype(np.float32) if f16 == 1 else oracle.round_to_half(mean, False)
    assert DC.equal_bits(got[..., :3], want, "independent rounding")

    more = [host.update(cam, 0.0, f, W, H) for f in (3, 4)]
    p.render_batch(more)
    for pfc in more:
        acc, _ = osc.render(mat, pfc, W, H, accum=acc, env_constant=black, accum_f16=f16, nthreads=8)
    assert DC.equal_bits(p.read_output(), acc, "two more frames in one set")
