"""Object lifecycle on the GPU: repeated create / build / render / destroy cycles must not leak device memory,
and handles may be destroyed in any order (the library reference-counts them)."""
import ctypes as C
import gc

import numpy as np
import pytest

from dxrexperiments_amd import rtypes as T, scenes
from util import cam_array

pytestmark = pytest.mark.gpu


def free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def cycle(capi, gpu, order):
    v, t = scenes.blob_mesh(level=2)
    model = capi.Model(gpu, v, t)
    sc = capi.Scene(gpu)
    sc.add_model(model)
    sc.add_model(model, scenes.instance_grid(2)[1])
    # a chain of four joints, each half a unit above its parent; the second instance follows the third joint
    sk = capi.Skeleton(gpu, np.array([-1, 0, 1, 2], np.int32), np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (4, 1)))
    sk.set_pose(np.tile(np.array([0, 0.5, 0, 0, 0, 0, 1, 1, 1, 1], np.float32), (4, 1)))
    sc.attach(1, sk, [2], scenes.instance_grid(2)[1:2])
    skinned = capi.Model(gpu, v, t)
    skinned.set_skin(np.arange(v.shape[0], dtype=np.uint32).reshape(-1, 1) % 4, np.ones((v.shape[0], 1), np.float32), 4)
    p = capi.Pipeline(gpu)
    p.set_scene(sc)
    p.add_material(T.default_material())
    p.add_material(T.default_material())
    p.set_environment_cube(scenes.sky_cubemap(8))
    p.create_output(160, 96)
    p.build_acceleration_structures()
    p.enable_timing(2)
    host = capi.ProgressiveHost(1)
    cam = cam_array(dict(eye=(0, 1, 6), at=(0, 0, 0), up=(0, 1, 0), fov=0.8), 160 / 96)
    for f in range(2):
        p.update(host.update(cam, 0.0, f + 1, 160, 96))
        p.render()
    img = p.read_output()
    assert np.isfinite(img).all()
    dn = capi.Denoiser(gpu)
    dn.create_output(160, 96)
    skinned.set_bones_from(sk)          # queued, not waited for: the skeleton's holders are this kernel and the scene when the handles go
    objs = {"pipeline": p, "scene": sc, "model": model, "denoiser": dn, "host": host, "skeleton": sk}
    for name in order:
        objs.pop(name).close()
    skinned.close()
    return img


def test_no_device_memory_leak_and_any_destroy_order(gpu, capi):
    orders = [("skeleton", "pipeline", "scene", "model", "denoiser", "host"), ("model", "scene", "pipeline", "host", "denoiser", "skeleton"),
              ("scene", "denoiser", "model", "skeleton", "host", "pipeline")]
    first = cycle(capi, gpu, orders[0])
    gc.collect()
    gpu.synchronize()
    base = free_bytes()
    for k in range(30):
        img = cycle(capi, gpu, orders[k % 3])
        assert np.array_equal(img, first)
    gc.collect()
    gpu.synchronize()
    leaked = base - free_bytes()
    assert leaked < (8 << 20), "device memory shrank by %d bytes over 30 create/destroy cycles" % leaked


def context_first_cycle(capi, order):
    """a context whose own handle goes first: the objects made on it keep it alive, still render, and the last of them takes it along"""
    v, t = scenes.blob_mesh(level=2)
    ctx = capi.Context(0)
    model = capi.Model(ctx, v, t)
    sc = capi.Scene(ctx)
    sc.add_model(model)
    p = capi.Pipeline(ctx)
    p.set_scene(sc)
    p.add_material(T.default_material())
    p.set_environment_cube(scenes.sky_cubemap(8))
    p.create_output(64, 64)
    p.build_acceleration_structures()
    host = capi.ProgressiveHost(1)
    ctx.close()
    p.update(host.update(cam_array(dict(eye=(0, 1, 6), at=(0, 0, 0), up=(0, 1, 0), fov=0.8), 1.0), 0.0, 1, 64, 64))
    p.render()
    img = p.read_output()
    assert np.isfinite(img).all()
    objs = {"pipeline": p, "scene": sc, "model": model}
    for name in order:
        objs.pop(name).close()
    host.close()
    return img


def test_context_handle_closed_first_leaks_nothing(gpu, capi):
    orders = [("pipeline", "scene", "model"), ("model", "scene", "pipeline"), ("scene", "model", "pipeline")]
    first = context_first_cycle(capi, orders[0])
    gc.collect()
    gpu.synchronize()
    base = free_bytes()
    for k in range(30):
        assert np.array_equal(context_first_cycle(capi, orders[k % 3]), first)
    gc.collect()
    gpu.synchronize()
    leaked = base - free_bytes()
    assert leaked < (8 << 20), "device memory shrank by %d bytes over 30 cycles whose context handle went first" % leaked


RT_ERR_OOM = -5                                                  # include/dxr_amd_types.h


def _cable_rays(v, t):
    """a fixed set of rays from inside the hall: 3000 at the centroids of triangles drawn from the whole mesh (most of them the slivers of
    cables and slats), 1000 in random directions"""
    r = np.random.default_rng(11)
    pos = v["position"].astype(np.float64)
    eye = np.array([2.0, 3.0, 1.0])
    aim = pos[t[r.integers(0, t.shape[0], 3000)]].mean(axis=1) - eye
    d = np.concatenate([aim, r.normal(size=(1000, 3))])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.empty((d.shape[0], 4), np.float32)
    o[:, :3], o[:, 3] = eye, 1e-3
    dd = np.empty_like(o)
    dd[:, :3], dd[:, 3] = d, 1e30
    return o, dd


def _build_and_trace(capi, ctx, v, t, rays):
    model = capi.Model(ctx, v, t)
    sc = capi.Scene(ctx)
    try:
        sc.add_model(model)
        sc.build()
        return sc.trace(*rays)
    finally:
        sc.close()
        model.close()


def _ladder_of_failed_builds(capi, ctx, v, t, rays):
    want = _build_and_trace(capi, ctx, v, t, rays)
    assert np.unique(want["prim"]).size > 500, "the rays hit next to nothing"
    gc.collect()
    ctx.synchronize()
    base = free_bytes()
    raised, built = [], []
    try:
        for k in range(11):
            capi.lib().rt_debug_set_alloc_limit(1024 * 4 ** k)
            model = sc = None
            try:
                model = capi.Model(ctx, v, t)
                sc = capi.Scene(ctx)
                sc.add_model(model)
                sc.build()
                built.append(k)
            except capi.RtError as e:
                assert e.code == RT_ERR_OOM, "rung %d (limit %d bytes): %r" % (k, 1024 * 4 ** k, e)
                raised.append(k)
            finally:
                if sc is not None:
                    sc.close()
                if model is not None:
                    model.close()
    finally:
        capi.lib().rt_debug_set_alloc_limit(0)
    # 1 KiB does not hold the vertex upload (271 KB), 1 GiB holds every buffer of a 6771-triangle build
    assert raised and built and raised[0] == 0 and built[-1] == 10, (raised, built)
    gc.collect()
    ctx.synchronize()
    leaked = base - free_bytes()
    assert leaked < (8 << 20), "device memory shrank by %d bytes over the failed builds of rungs %s" % (leaked, raised)
    got = _build_and_trace(capi, ctx, v, t, rays)
    for k in ("t", "u", "v", "prim", "inst"):
        assert np.array_equal(want[k].view(np.uint32), got[k].view(np.uint32)), k
    return raised


def test_failed_builds_leak_nothing(gpu, capi):
    """A build that runs out of device memory anywhere -- the vertex upload, the arena, the records, the split references, the reference
    sort, either layout -- gives back what it had reserved and leaves the context usable.  Every failure is an allocation the host
    refuses (rt_debug_set_alloc_limit walked up from 1 KiB to 1 GiB in steps of 4x); the mesh is the hall of cables whose triangles
    are held as split references.  Then the same with the LBVH layout and with one record per triangle, on a second context."""
    v, t = scenes.stadium_class(5, 0.25, ("hall", "cables", "slats"))
    rays = _cable_rays(v, t)
    _ladder_of_failed_builds(capi, gpu, v, t, rays)
    for name, value in (("fast_bvh", "lbvh"), ("split_refs", 0)):
        ctx = capi.Context(0)
        try:
            ctx.set_option(name, value)
            _ladder_of_failed_builds(capi, ctx, v, t, rays)
        finally:
            ctx.close()


def _atrium_pipeline(capi, ctx, model, W, H):
    sc = capi.Scene(ctx)
    sc.add_model(model)
    p = capi.Pipeline(ctx)
    p.set_scene(sc)
    p.add_material(T.default_material())
    p.set_environment_cube(scenes.sky_cubemap(16))
    p.create_output(W, H)
    p.build_acceleration_structures()
    return p


def _five_frames(capi, p, pfcs, limit=0):
    """frame 1 by render(), frames 2 - 5 as one render_batch, with device allocations above `limit` bytes refused: the image and the totals"""
    try:
        capi.lib().rt_debug_set_alloc_limit(limit)
        p.update(pfcs[0])
        p.render()
        p.render_batch(pfcs[1:5])
    finally:
        capi.lib().rt_debug_set_alloc_limit(0)
    return p.read_output(), p.totals()


def test_failed_render_reservations_leak_nothing(gpu, capi):
    """The ladder of the builds, for the render path: on a fresh pipeline, set up and built, device allocations above a limit are refused
    (rt_debug_set_alloc_limit, 1 KiB walked up to 256 MiB in steps of 4x) while one render() and a render_batch of four frames reserve the
    materials, counters, queues, totals, constants, shadow cache and retry list.  Every rung either reports RT_ERR_OOM or gives the image
    and the ray totals of the unrestricted run bit for bit; afterwards the last pipeline still renders what an unrestricted one does and
    the device's free memory is where it was.  The scene is the atrium of test_gpu_deferred_and_queues.py."""
    from test_gpu_batch import frames_of
    W, H = 64, 48
    model = capi.Model(gpu, *scenes.sponza_class(seed=42))
    cam = cam_array(scenes.sponza_camera(), W / H)
    pfcs = frames_of(capi, cam, 8, W, H)
    ref = _atrium_pipeline(capi, gpu, model, W, H)
    want, want_totals = _five_frames(capi, ref, pfcs)
    gc.collect()
    gpu.synchronize()
    base = free_bytes()
    raised, rendered, p = [], [], None
    for k in range(10):
        if p is not None:
            p.close()
        p = _atrium_pipeline(capi, gpu, model, W, H)
        try:
            got, got_totals = _five_frames(capi, p, pfcs, 1024 * 4 ** k)
        except capi.RtError as e:
            assert e.code == RT_ERR_OOM, "rung %d (limit %d bytes): %r" % (k, 1024 * 4 ** k, e)
            raised.append(k)
            continue
        assert np.array_equal(got, want), "rung %d: %d pixels differ" % (k, int((got != want).any(axis=2).sum()))
        assert got_totals == want_totals, (k, got_totals, want_totals)
        rendered.append(k)
    assert raised and rendered and rendered[-1] == 9, (raised, rendered)
    for c in pfcs[5:]:
        for q in (p, ref):
            q.update(c); q.render()
    assert np.array_equal(p.read_output(), ref.read_output())
    assert p.totals() == ref.totals()
    p.close()
    gc.collect()
    gpu.synchronize()
    leaked = base - free_bytes()
    assert leaked < (8 << 20), "device memory shrank by %d bytes over the refused reservations of rungs %s" % (leaked, raised)
