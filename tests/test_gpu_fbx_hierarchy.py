"""A binary FBX with a node hierarchy, loaded through rt_model_create_from_file and rendered on the GPU: the flattened arrays
(tests/test_fbx_hierarchy.py holds them to an independent evaluation) feed the BLAS build unchanged, so both pipelines are bit-identical
to the oracle fed what rt_fbx_read returned for the same file.  One file: the three-level hierarchy (a) and the instanced pair (g) of
tests/fbx_hierarchy_tools.py, 36 triangles once flattened."""
import numpy as np
import pytest

from dxrexperiments_amd import rtypes as T, scenes
from util import cam_array

import fbx_hierarchy_tools as H

pytestmark = pytest.mark.gpu

W = HT = 64


@pytest.fixture(scope="module")
def hierarchy(capi, tmp_path_factory):
    """(path, verts, tris): the file and what the device-free reader makes of it"""
    cases = H.cases()
    geoms, models = H.combine(cases["a_three_levels"], cases["g_instanced_geometry"])
    path = str(tmp_path_factory.mktemp("fbx") / "hierarchy.fbx")
    H.write(path, geoms, models)
    v, i = capi.fbx_read(path)
    assert i.shape == (36, 3)
    return path, v, i


def ground_quad(y=-3.0, half=9.0):
    v = np.zeros(4, T.VERTEX)
    v["position"] = [(-half, y, -half), (-half, y, half), (half, y, half), (half, y, -half)]
    v["normal"] = (0.0, 1.0, 0.0)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def test_progressive_frames_of_a_flattened_hierarchy(gpu, capi, oracle, hierarchy):
    path, v, i = hierarchy
    model = capi.Model(gpu, path=path)
    gv, gi = model.geometry()                                     # rt_model_read_geometry: exactly the reader's arrays
    assert np.array_equal(gv.view(np.uint8), v.view(np.uint8)) and np.array_equal(gi, i)
    qv, qi = ground_quad()
    ground = capi.Model(gpu, qv, qi)
    sc = capi.Scene(gpu)
    sc.add_model(ground)
    sc.add_model(model)
    osc = oracle.Scene()
    osc.add_instance(osc.add_model(qv, qi))
    osc.add_instance(osc.add_model(v, i))
    osc.build()
    mats = np.stack([T.default_material(), T.default_material()])
    p = capi.Pipeline(gpu)
    p.set_scene(sc)
    for m in mats:
        p.add_material(m)
    env = scenes.sky_cubemap(8)
    p.set_environment_cube(env)
    p.create_output(W, HT)
    p.build_acceleration_structures()
    host = capi.ProgressiveHost(17)
    cam = cam_array(dict(eye=(0.0, 10.0, 10.0), at=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=0.8), W / HT)
    acc = np.zeros((HT, W, 4), np.float32)
    for f in range(2):
        pfc = host.update(cam, 0.0, f + 1, W, HT)
        p.update(pfc)
        p.render()
        if f == 0:
            _, prim, inst = p.primary_hits(W * HT)
            seen = np.unique(prim[inst == 1])
            assert (seen < 12).any() and ((seen >= 12) & (seen < 24)).any() and (seen >= 24).any()      # all three flattened meshes are in view
        acc, _ = osc.render(mats, pfc, W, HT, accum=acc, env_faces=env, nthreads=4)
    img = p.read_output()
    assert np.isfinite(img).all()
    assert np.array_equal(img, acc), "%d of %d pixels differ from the oracle" % (int((img != acc).any(axis=2).sum()), W * HT)


def test_realtime_aovs_of_two_instances_of_a_flattened_hierarchy(gpu, capi, oracle, hierarchy):
    """The two-level path: one BLAS from the file, two TLAS instances, RealtimeRaytracingPipeline's two AOVs."""
    path, v, i = hierarchy
    model = capi.Model(gpu, path=path)
    a = np.radians(40.0)
    second = np.array([0.8 * np.cos(a), 0, 0.8 * np.sin(a), 1.0, 0, 0.8, 0, 4.5, -0.8 * np.sin(a), 0, 0.8 * np.cos(a), -2.0], np.float32)
    sc = capi.Scene(gpu)
    osc = oracle.Scene()
    om = osc.add_model(v, i)
    for x in (None, second):
        sc.add_model(model, x)
        osc.add_instance(om, x)
    osc.build()
    mats = []
    for k in range(2):
        m = T.default_material()
        m["albedo"][:3] = (0.8, 0.3, 0.2) if k else (0.2, 0.5, 0.8)
        m["type"] = k
        mats.append(m)
    p = capi.Pipeline(gpu, capi.PIPELINE_REALTIME)
    p.set_scene(sc)
    for m in mats:
        p.add_material(m)
    env = scenes.sky_cubemap(8)
    p.set_environment_cube(env)
    p.create_output(W, HT)
    p.build_acceleration_structures()
    host = capi.ProgressiveHost(18)
    cam = cam_array(dict(eye=(0.0, 4.0, 16.0), at=(0.0, 2.0, 0.0), up=(0, 1, 0), fov=0.8), W / HT)
    pfc = host.update_realtime(cam, 0.0, 1, W, HT)
    p.update(pfc)
    p.render()
    d, ind, ost = osc.render_realtime(np.stack(mats), pfc, W, HT, env_faces=env, nthreads=4)
    gst = p.stats()
    for key in ("rays_primary", "rays_secondary", "rays_shadow", "primary_hits", "secondary_hits"):
        assert gst[key] == ost[key], key
    assert 0 < ost["primary_hits"] < W * HT
    assert np.array_equal(p.read_output(0), d), "direct-lighting AOV differs"
    assert np.array_equal(p.read_output(1), ind), "indirect-specular AOV differs"
