"""What every entry point that needs a built scene answers when the scene is not one: the return code and the exact rt_last_error() text, in
every state a scene can be in between two builds.  The texts are written out here; nothing is formed by calling the library or taken from the
shadow model of tests/scene_edit_model.py.  One triangle, two instances: the states are host logic, no larger scene shows more of it."""
import ctypes as C
import types

import numpy as np
import pytest

from dxrexperiments_amd import rtypes as T

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_STATE = 0, -4
W, H = 8, 8

APPLIES = "rt_scene_update or rt_scene_build applies them"
VERTEX_SETTERS = "(rt_model_set_vertices / _set_positions / _recompute_normals)"
ONE_TRANSFORM = "1 instance transform pending (rt_scene_set_instance_transform): " + APPLIES
TWO_TRANSFORMS = "2 instance transforms pending (rt_scene_set_instance_transform): " + APPLIES
MASKS = "instance masks pending (rt_scene_set_instance_mask): " + APPLIES
TRANSFORM_AND_MASKS = "1 instance transform and instance masks pending (rt_scene_set_instance_transform): " + APPLIES
VERTICES = "new vertices of the models of 2 instances pending " + VERTEX_SETTERS + ": " + APPLIES
VERTICES_AND_MASKS = "new vertices of the models of 2 instances and instance masks pending " + VERTEX_SETTERS + ": " + APPLIES
EVERYTHING = "new vertices of the models of 2 instances and 1 instance transform and instance masks pending " + VERTEX_SETTERS + ": " + APPLIES
NO_INDEX = "scene not built or index out of range"
NO_INSTANCE = "scene not built or instance out of range"
WIDE_WRITE = "rt_debug_wide_write: scene not built, or a different node count"
NOT_SPLIT = "rt_scene_refs_read: no triangle of this model is split"
NONE_VISIBLE = "rt_scene_update: no instance is visible: every instance mask is 0 (rt_scene_set_instance_mask)"

# the lookups that take `which` (-1: the TLAS, k: the BLAS of instance k's model); every output pointer may be null
LOOKUPS = {
    "rt_scene_bvh_info": lambda L, s, which: L.rt_scene_bvh_info(s, which, None, None, None),
    "rt_scene_bvh_read": lambda L, s, which: L.rt_scene_bvh_read(s, which, None, None, None),
    "rt_scene_wide_info": lambda L, s, which: L.rt_scene_wide_info(s, which, None, None, None),
    "rt_scene_wide_read": lambda L, s, which: L.rt_scene_wide_read(s, which, None, None),
    "rt_scene_refs_info": lambda L, s, which: L.rt_scene_refs_info(s, which, None, None),
    "rt_scene_refs_read": lambda L, s, which: L.rt_scene_refs_read(s, which, None, None, None),
}


def shifted(x):
    m = T.IDENTITY_3X4.copy()
    m[3] = x
    return m


def fresh(capi, ctx):
    """one triangle under two instances, not built; a pipeline on the scene that lacks nothing but the acceleration structures"""
    v = np.zeros(3, T.VERTEX)
    v["position"] = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    v["normal"] = (0, 0, 1)
    model = capi.Model(ctx, v, [(0, 1, 2)])
    sc = capi.Scene(ctx)
    sc.add_model(model)
    sc.add_model(model, shifted(3.0))
    pipe = capi.Pipeline(ctx)
    pipe.set_scene(sc)
    pipe.add_material(T.default_material())
    pipe.set_environment_constant((0.5, 0.5, 0.5))
    pipe.create_output(W, H)
    host = capi.ProgressiveHost(1234)
    pipe.update(host.update(capi.camera_array((0.3, 0.3, 3.0), (0.3, 0.3, 0.0), (0, 1, 0), 0.8, W / H), 0.0, 1, W, H))
    return types.SimpleNamespace(capi=capi, ctx=ctx, model=model, sc=sc, pipe=pipe, host=host)


def answer(capi, rc):
    """(code, message) of a call that has just returned rc; a success leaves the last message alone, so there is none to compare"""
    return (rc, capi.lib().rt_last_error().decode() if rc != RT_OK else None)


def wide_write(f, which, n_nodes):
    nodes = np.zeros((1, 16), np.uint32)
    return answer(f.capi, f.capi.lib().rt_debug_wide_write(f.sc.h, which, nodes.ctypes.data, n_nodes))


def trace(f):
    o = np.array([[0.25, 0.25, 1.0, 0.0]], np.float32)
    d = np.array([[0.0, 0.0, -1.0, 10.0]], np.float32)
    out = [np.zeros(1, np.float32) for _ in range(3)] + [np.zeros(1, np.uint32) for _ in range(2)]
    rc = f.capi.lib().rt_trace_batch(f.ctx.h, f.sc.h, o.ctypes.data, d.ctypes.data, 1, 0, 0, 0, *[a.ctypes.data for a in out], None, None)
    return answer(f.capi, rc), out


def render(f):
    return answer(f.capi, f.capi.lib().rt_pipeline_render(f.pipe.h, W, H))


def assert_refused(f, pending, label):
    """every entry point refuses with RT_ERR_STATE; pending: the text of what is pending, or None for a scene that is simply not built"""
    L, s = f.capi.lib(), f.sc.h
    for name, call in LOOKUPS.items():
        for which in (-1, 0, 1):
            assert answer(f.capi, call(L, s, which)) == (RT_ERR_STATE, "%s: %s" % (name, pending or NO_INDEX)), (label, name, which)
    for i in (0, 1):
        want = "rt_scene_instance_info: " + pending if pending else NO_INSTANCE
        assert answer(f.capi, L.rt_scene_instance_info(s, i, None, None)) == (RT_ERR_STATE, want), (label, i)
    # (rt_debug_wide_write does not look at what is pending: one text)
    assert wide_write(f, 0, 1000) == (RT_ERR_STATE, WIDE_WRITE), label
    assert wide_write(f, -1, 1000) == (RT_ERR_STATE, WIDE_WRITE), label
    assert trace(f)[0] == (RT_ERR_STATE, "rt_trace_batch: " + (pending or "scene not built")), label
    assert render(f) == (RT_ERR_STATE, "render: " + (pending or "acceleration structures not built")), label


def assert_clean(f, n, label):
    """a built scene of n instances with nothing pending: every entry point answers, and refuses what is not there"""
    L, s = f.capi.lib(), f.sc.h
    for name, call in LOOKUPS.items():
        for which in range(-1, n):
            want = (RT_OK, None)
            if name.startswith("rt_scene_refs") and which < 0:
                want = (RT_ERR_STATE, "%s: %s" % (name, NO_INDEX))           # (the TLAS has no references)
            elif name == "rt_scene_refs_read":
                want = (RT_ERR_STATE, NOT_SPLIT)
            assert answer(f.capi, call(L, s, which)) == want, (label, name, which)
        for which in (n, n + 1, 1000, 2 ** 31 - 1):
            assert answer(f.capi, call(L, s, which)) == (RT_ERR_STATE, "%s: %s" % (name, NO_INDEX)), (label, name, which)
    n_tris, n_refs = C.c_uint32(0), C.c_uint32(1)
    assert L.rt_scene_refs_info(s, 0, C.byref(n_tris), C.byref(n_refs)) == RT_OK
    assert (n_tris.value, n_refs.value) == (1, 0), label
    for i in range(n):
        assert answer(f.capi, L.rt_scene_instance_info(s, i, None, None)) == (RT_OK, None), (label, i)
    for i in (n, n + 1, 2 ** 32 - 1):
        assert answer(f.capi, L.rt_scene_instance_info(s, i, None, None)) == (RT_ERR_STATE, NO_INSTANCE), (label, i)
    n_nodes = f.sc.wide_counts(0)[0]
    for which, count in ((0, n_nodes + 1), (-1, 1000), (n, n_nodes), (1000, n_nodes)):
        assert wide_write(f, which, count) == (RT_ERR_STATE, WIDE_WRITE), (label, which, count)
    got, out = trace(f)
    assert got == (RT_OK, None), label
    assert out[0][0] == 1.0 and out[3][0] == 0 and out[4][0] == 0, (label, out)      # (the ray meets instance 0's triangle at t = 1)
    assert render(f) == (RT_OK, None), label


def test_never_built(gpu, capi):
    f = fresh(capi, gpu)
    assert_refused(f, None, "never built")
    # setters on a scene that was never built leave nothing pending: the build reads what is stored
    f.sc.set_transform(1, shifted(4.0))
    f.sc.set_mask(1, 0)
    f.model.set_positions([(0, 0, 0), (2, 0, 0), (0, 2, 0)])
    assert_refused(f, None, "never built, after setters")


def test_built_then_add_model(gpu, capi):
    f = fresh(capi, gpu)
    f.sc.build()
    f.sc.add_model(f.model, shifted(6.0))
    assert_refused(f, None, "add_model after a build")
    f.sc.set_transform(0, shifted(1.0))
    f.sc.set_mask(2, 0)
    assert_refused(f, None, "add_model after a build, then setters")
    rc = capi.lib().rt_scene_update(f.sc.h)
    assert answer(capi, rc) == (RT_ERR_STATE, "rt_scene_update: the scene has not been built since its last rt_scene_add_model "
                                               "(an update builds no BLAS: rt_scene_build)")
    f.sc.set_mask(2, 0xFF)
    f.sc.set_transform(0)
    f.sc.build()
    assert_clean(f, 3, "built again")


def test_pending_transforms(gpu, capi):
    f = fresh(capi, gpu)
    f.sc.build()
    f.sc.set_transform(1, shifted(4.0))
    assert_refused(f, ONE_TRANSFORM, "one transform")
    f.sc.set_transform(1, shifted(5.0))                # (the same instance again: still one)
    assert_refused(f, ONE_TRANSFORM, "one transform, set twice")
    f.sc.set_transform(0, shifted(0.0))
    assert_refused(f, TWO_TRANSFORMS, "two transforms")
    f.sc.update()
    assert_clean(f, 2, "after the update")


def test_pending_masks(gpu, capi):
    f = fresh(capi, gpu)
    f.sc.build()
    f.sc.set_mask(1, 0x01)                             # (visible before and after: nothing is pending)
    assert_clean(f, 2, "another non-zero mask")
    f.sc.set_mask(1, 0)
    assert_refused(f, MASKS, "one instance hidden")
    f.sc.set_transform(0, shifted(0.0))
    assert_refused(f, TRANSFORM_AND_MASKS, "one instance hidden, one transform")
    f.sc.update()
    assert_clean(f, 2, "after the update")


def test_pending_vertices(gpu, capi):
    f = fresh(capi, gpu)
    f.sc.build()
    f.model.set_positions([(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    assert_refused(f, VERTICES, "new vertices")
    f.sc.set_mask(1, 0)
    assert_refused(f, VERTICES_AND_MASKS, "new vertices, one instance hidden")
    f.sc.update()
    assert_clean(f, 2, "after the update")


def test_everything_pending_and_no_instance_visible(gpu, capi):
    f = fresh(capi, gpu)
    f.sc.build()
    f.model.set_positions([(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    f.sc.set_transform(1, shifted(4.0))
    f.sc.set_mask(1, 0)
    assert_refused(f, EVERYTHING, "vertices, a transform and masks")
    # every mask zero: the update is refused and keeps the state, with everything that was pending
    f.sc.set_mask(0, 0)
    assert_refused(f, EVERYTHING, "vertices, a transform and masks, nothing visible")
    for _ in range(2):
        assert answer(capi, capi.lib().rt_scene_update(f.sc.h)) == (RT_ERR_STATE, NONE_VISIBLE)
        assert_refused(f, EVERYTHING, "after the refused update")
    f.sc.set_mask(0, 0xFF)
    f.sc.update()
    assert_clean(f, 2, "after the update")


def test_built_and_clean(gpu, capi):
    f = fresh(capi, gpu)
    f.sc.build()
    assert_clean(f, 2, "built")
    f.sc.update()                                      # (nothing to apply)
    assert_clean(f, 2, "built, updated with nothing pending")
    # the setters' own refusals: an instance, or a range of them, that the scene does not have
    L, s, x = capi.lib(), f.sc.h, np.tile(T.IDENTITY_3X4, 2)
    m = np.zeros(3, np.uint8)
    assert answer(capi, L.rt_scene_set_instance_transform(s, 2, x.ctypes.data)) == \
        (RT_ERR_STATE, "rt_scene_set_instance_transform: instance 2 out of range: the scene has 2")
    assert answer(capi, L.rt_scene_set_instance_transforms(s, 1, 2, x.ctypes.data)) == \
        (RT_ERR_STATE, "rt_scene_set_instance_transforms: instances 1 .. 3 out of range: the scene has 2")
    assert answer(capi, L.rt_scene_set_instance_mask(s, 5, 0)) == (RT_ERR_STATE, "rt_scene_set_instance_mask: instance 5 out of range: the scene has 2")
    assert answer(capi, L.rt_scene_set_instance_masks(s, 3, 0, m.ctypes.data)) == \
        (RT_ERR_STATE, "rt_scene_set_instance_masks: instances 3 .. 3 out of range: the scene has 2")
    assert answer(capi, L.rt_scene_get_instance_masks(s, 0, 3, m.ctypes.data)) == \
        (RT_ERR_STATE, "rt_scene_get_instance_masks: instances 0 .. 3 out of range: the scene has 2")
    assert_clean(f, 2, "after the refused setters")
