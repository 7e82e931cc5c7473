"""The HIP kernels against the reference's own shading text, bit for bit: the fixtures under tests/golden/refshade/ were computed by
the reference's HLSL compiled as C++ (oracle/refshade/README.md).  Nothing here reads the reference, the library built from it or the
oracle's shading code: only the recorded inputs and outputs.  The device sampler and math exports are those of tests/test_gpu_math.py;
frames go through the C ABI, with fp32 and with RGBA16F accumulation storage, frame by frame and as one deferred set."""
import numpy as np
import pytest

import refshade_cases as R
from dxrexperiments_amd import rtypes as T
from test_refshade import CASE_NAMES

pytestmark = pytest.mark.gpu


def test_device_units_equal_the_reference_text(gpu):
    u = R.load_fixture("units")
    for kind in ("cos", "uniform", "perp"):
        out, _, so = gpu.sample(R.SAMPLE[kind], u["seeds"], u["dirs"], 0.0)
        assert R.same_bits(out, u[kind + "_out"]), "%s: %d values differ" % (kind, int((out != u[kind + "_out"]).sum()))
        assert np.array_equal(so, u[kind + "_seed"]), kind
    exps = gpu.math(2, (np.float32(1.0) - u["roughness"]) * np.float32(12.0))            # exp: the exponent shade() derives from a roughness
    assert R.same_bits(exps, u["exponents"])
    for k, e in enumerate(u["exponents"]):
        out, pb, so = gpu.sample(R.SAMPLE["phong"], u["seeds"], u["dirs"], float(e))
        assert R.same_bits(out, u["phong%d_out" % k]) and R.same_bits(pb, u["phong%d_pdf_brdf" % k]), "phong, roughness %g" % R.ROUGHNESS[k]
        assert np.array_equal(so, u["phong%d_seed" % k])
    # Fresnel from the device's own pow and the text's expression f0 + (1 - f0) * pow(1 - cosi, 5): the device has no Fresnel export, so
    # its dot product is restated here in fp32 numpy (three products, summed in order) and only pow runs on the device
    f = np.float32
    I, N, f0 = u["dirs"], u["normals"], u["f0"]
    d = (-I[:, 0]) * N[:, 0]
    d = d + (-I[:, 1]) * N[:, 1]
    d = d + (-I[:, 2]) * N[:, 2]
    cosi = np.minimum(np.maximum(d, f(0.0)), f(1.0))
    p = gpu.math(4, f(1.0) - cosi, np.full_like(cosi, 5.0))
    got = f0 + (f(1.0) - f0) * p[:, None]
    assert R.same_bits(got.astype(np.float32), u["fresnel_out"])


def make_pipeline(capi, ctx, case, kind):
    models, inst = R._scene(case["scene"])
    gm = [capi.Model(ctx, path=m) if isinstance(m, str) else capi.Model(ctx, m[0], m[1]) for m in models]
    sc = capi.Scene(ctx)
    for mi, x in inst:
        sc.add_model(gm[mi], x)
    p = capi.Pipeline(ctx, kind)
    p.set_scene(sc)
    return p


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_frames_equal_the_reference_text(gpu, capi, name):
    want = R.load_fixture(name)
    pfcs, mats = want["pfcs"], want["mats"]
    # scene, size and environment are the case's (tests/refshade_cases.py: plain data, no oracle); constants and materials are the recorded ones
    case = dict(R.CASE_SHAPES[name])
    W, H, env = case["W"], case["H"], R.env_faces(case)
    realtime = name.startswith("realtime")
    p = make_pipeline(capi, gpu, case, capi.PIPELINE_REALTIME if realtime else capi.PIPELINE_PROGRESSIVE)
    for m in mats:
        p.add_material(m)
    if env is not None:
        p.set_environment_cube(env)
    else:
        p.set_environment_constant((0.5, 0.5, 0.5))
    p.create_output(W, H)
    p.build_acceleration_structures()
    if realtime:
        for f in range(pfcs.shape[0]):
            p.update(pfcs[f])
            p.render()
            for out, key in ((0, "direct%d"), (1, "indirect%d")):
                img = p.read_output(out)
                assert R.same_bits(img, want[key % f]), "%s %s: %d values differ" % (name, key % f, int((img != want[key % f]).sum()))
        st = p.stats()
        assert [st[k] for k in R.STAT_KEYS] == [int(x) for x in want["stats"]]
        return
    storages = [k[len("image_"):] for k in want if k.startswith("image_")]
    assert "fp32" in storages and "f16n" in storages
    for storage in storages:
        ref = want["image_" + storage].astype(np.float32)
        per_frame = ref.ndim == 4
        for deferred in (0, 4):
            if storage == "fp32":
                p.set_accumulation_storage(T.FORMAT_R32G32B32A32_FLOAT)
            else:
                p.set_accumulation_storage(T.FORMAT_R16G16B16A16_FLOAT, T.ROUND_NEAREST_EVEN if storage == "f16n" else T.ROUND_TOWARD_ZERO)
            p.set_deferred(deferred)
            p.clear_output()
            for f in range(pfcs.shape[0]):
                p.update(pfcs[f])
                p.render()
                if per_frame and not deferred:
                    img = p.read_output()
                    assert R.same_bits(img, ref[f]), "%s %s frame %d: %d values differ" % (name, storage, f, int((img != ref[f]).sum()))
            img = p.read_output()
            last = ref[-1] if per_frame else ref
            assert R.same_bits(img, last), "%s %s deferred=%d: %d values differ" % (name, storage, deferred, int((img != last).sum()))
            if not deferred:
                st = p.stats()
                assert [st[k] for k in R.STAT_KEYS] == [int(x) for x in want["stats"]]
    p.set_deferred(0)
