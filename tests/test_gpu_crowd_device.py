"""Crowds driven from device memory (rt_crowd_set_layout + rt_crowd_set_blend_device; include/dxr_amd.h "Posed skeletons", crowds): every
actor is, byte for byte, the actor rt_crowd_set_blend makes of the same layers -- and the numpy statement -- with the times and weights read
from device arrays and every segment found by the kernel; the search over clips of 1, 2, 3, 8 and 33 keys at every kind of time; NaN times,
which the host never sees; weights from the layout and from an array; the held pose as a base; back-to-back calls; every refusal with its
message, and nothing changed by it; stale layouts; an attached scene; the example.  No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import crowd_cases as CC
import crowd_device_cases as CD
import skeleton_blend_cases as B
import skeleton_cases as S
from test_gpu_crowd import assert_numpy, reads, scene_of, skeleton_with
from test_gpu_scene_update import arrays, assert_bytes_equal
from util import random_xforms

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")


def on_device(gpu, a):
    return gpu.upload(np.ascontiguousarray(a, F))


def assert_same(got, want, what, skip=()):
    """pose, joints and palette, every actor byte for byte (but the actors of `skip`)"""
    for name, g, w in zip(("pose", "joints", "palette"), got, want):
        assert g.shape == w.shape, what
        for a in range(g.shape[0]):
            if a not in skip:
                assert g[a].tobytes() == w[a].tobytes(), "%s: actor %d: %s differs from the host path" % (what, a, name)


def pose_both(gpu, device, host, layers, times=None, weights=None, null_weights=False):
    """`device` posed by set_blend_device from arrays holding the layers' times and weights (or those given), `host` by set_blend of the same
    layers; returns both crowds' reads"""
    t, w = CD.split(layers)
    t = t if times is None else np.asarray(times, F)
    w = w if weights is None else np.asarray(weights, F)
    dt, dw = on_device(gpu, t), on_device(gpu, w)
    device.set_blend_device(dt.ptr, None if null_weights else dw.ptr)
    host.set_blend(CD.with_values(layers, t, None if null_weights else w))
    out = reads(device, 0, device.n_actors), reads(host, 0, host.n_actors)
    dt.close(); dw.close()
    return out


# ---- device crowd == host crowd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_actors", CD.ACTORS)
@pytest.mark.parametrize("family,n", CD.RIGS)
def test_device_crowd_equals_host_crowd(gpu, capi, family, n, n_actors):
    """1, 3 and (rigs of up to 65 joints) 8 layers: set_layout + set_blend_device == a second crowd given set_blend of the same layers, pose,
    joints and palette of every actor; and == numpy.  The layout poses nothing and counts no pose: the crowd is unposed until the first call"""
    parents, ib, clips, masks = CC.rig(family, n)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    device, host = capi.Crowd(shared, n_actors), capi.Crowd(shared, n_actors)
    held = CC.numpy_actors(n_actors, shared.info()[1])
    assert device.layout() == 0
    for n_layers in CD.layer_counts(n):
        what = "%s %d, %d actors, %d layers" % (family, n, n_actors, n_layers)
        layers = CC.actor_layers(clips, len(masks), n_actors, n_layers, seed=n)
        device.set_layout(layers)
        assert device.layout() == n_layers and host.layout() == 0
        if n_layers == 1:
            with pytest.raises(capi.RtError, match="the crowd has no pose yet") as e:
                device.pose()
            assert e.value.code == -4, "a layout poses nothing"
        got, want = pose_both(gpu, device, host, layers)
        assert_same(got, want, what)
        for a in held:
            assert_numpy(got, a, parents, ib, B.blended(clips, masks, layers[a]), what)
    # one layer is rt_crowd_set_times with the times on the device
    times = CC.actor_times(clips, n_actors)
    device.set_layout([[(c, NAN)] for c, _ in times])
    dt = on_device(gpu, [t for _, t in times])
    device.set_blend_device(dt.ptr)
    host.set_times([c for c, _ in times], [t for _, t in times])
    assert_same(reads(device, 0, n_actors), reads(host, 0, n_actors), "%s %d, %d actors: set_times" % (family, n, n_actors))
    dt.close(); device.close(); host.close(); shared.close()


# ---- the search ------------------------------------------------------------------------------------------------------------------------------
def test_the_search_on_the_device(gpu, capi):
    """65 joints, clips of 1, 2, 3, 8 and 33 keys, one actor per (clip, t) over skeleton_cases.sample_times: below, on and just under every
    key, inside every segment, beyond the last, -inf and +inf -- as the base layer, and as an additive layer over another clip, where lane 1
    does the searching"""
    parents, ib, clips, masks = CD.search_rig()
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    actors = [(c, float(t)) for c, (times, _) in enumerate(clips) for t in S.sample_times(times)]
    assert len(actors) == sum(3 * k + 2 for k in CD.SEARCH_KEYS) <= 300
    device, host = capi.Crowd(shared, len(actors)), capi.Crowd(shared, len(actors))
    layers = [[(c, t)] for c, t in actors]
    device.set_layout(layers)
    got, want = pose_both(gpu, device, host, layers)
    assert_same(got, want, "the search, base layer")
    for a, (c, t) in enumerate(actors):
        assert_numpy(got, a, parents, ib, S.sampled(*clips[c], t), "the search, base layer: clip %d at %r" % (c, t))
    layers = [[((c + 1) % len(clips), 0.3), (c, t, 0.75, a % 3, B.ADDITIVE if a % 2 else B.BLEND)] for a, (c, t) in enumerate(actors)]
    device.set_layout(layers)
    got, want = pose_both(gpu, device, host, layers)
    assert_same(got, want, "the search, layer 1")
    for a in range(0, len(actors), 7):
        assert_numpy(got, a, parents, ib, B.blended(clips, masks, layers[a]), "the search, layer 1: actor %d" % a)
    device.close(); host.close(); shared.close()


# ---- NaN times -------------------------------------------------------------------------------------------------------------------------------
def test_nan_times(gpu, capi):
    """NaN-timed actors among finite ones: the neighbours are byte-equal to the host crowd; a NaN actor is the numpy statement with the
    segment (0, NaN); on the one-key clip a NaN time is time 0 exactly"""
    parents, ib, clips, masks = CD.search_rig()
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    one = 0                                              # (the clip of one key)
    layers = [[(2, 0.4), (3, 0.9, 0.5, 0, B.BLEND)],
              [(2, NAN), (3, 0.9, 0.5, 0, B.BLEND)],     # the base
              [(3, 0.1), (2, 0.7, 0.5, None, B.ADDITIVE)],
              [(3, 0.1), (4, NAN, 0.5, None, B.ADDITIVE)],   # an additive layer, on the 33-key clip
              [(4, 5.0), (1, NAN, 0.25, 2, B.BLEND)],    # a masked replacing layer, on the clip of one segment
              [(one, NAN), (one, NAN, 0.5, 1, B.ADDITIVE)],  # one key: (0, 0)
              [(1, float("inf")), (4, float("-inf"), 1.5, None, B.BLEND)]]
    nan_actors = (1, 3, 4)
    n_actors = len(layers)
    device, host = capi.Crowd(shared, n_actors), capi.Crowd(shared, n_actors)
    device.set_layout(layers)
    t, w = CD.split(layers)
    dt, dw = on_device(gpu, t), on_device(gpu, w)
    device.set_blend_device(dt.ptr, dw.ptr)
    host.set_blend(CD.with_values(layers, np.where(np.isnan(t), F(0.0), t), w))           # (the host refuses a NaN: time 0 in its place)
    got, want = reads(device, 0, n_actors), reads(host, 0, n_actors)
    assert_same(got, want, "NaN times: the neighbours, and the one-key clip at time 0", skip=nan_actors)
    for a in range(n_actors):
        assert_numpy(got, a, parents, ib, CD.blended(clips, masks, layers[a]), "NaN times", nans=True)
    for a in nan_actors:
        assert np.isnan(got[0][a]).any(), "actor %d: (0, NaN) samples NaN" % a
    assert all(np.isfinite(got[1][a]).all() for a in range(n_actors) if a not in nan_actors)
    assert np.isnan(got[0][1][:, 0:3]).all() and got[0][1][0, 3:7].tolist() == [0, 0, 0, 1], "a NaN base: NaN translations, and (0, 0, 0, 1) where the mask is 0"
    dt.close(); dw.close(); device.close(); host.close(); shared.close()


# ---- weights ---------------------------------------------------------------------------------------------------------------------------------
def test_weights_from_the_layout_and_from_an_array(gpu, capi):
    """weights == NULL takes the layout's; an array overrides them; a NaN in the base layer's weight changes no byte (it is not read)"""
    n, n_actors, n_layers = 65, 5, 3
    parents, ib, clips, masks = CC.rig("random", n, seed=5)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    device, host = capi.Crowd(shared, n_actors), capi.Crowd(shared, n_actors)
    layers = CC.actor_layers(clips, len(masks), n_actors, n_layers, seed=77)
    device.set_layout(layers)
    got, want = pose_both(gpu, device, host, layers, null_weights=True)
    assert_same(got, want, "weights == NULL: the layout's")
    for a in range(n_actors):
        assert_numpy(got, a, parents, ib, B.blended(clips, masks, layers[a]), "weights == NULL")
    _, w = CD.split(layers)
    other = (w * F(0.5) + F(0.3)).astype(F)              # (no weight of the layout maps to itself)
    got2, want2 = pose_both(gpu, device, host, layers, weights=other)
    assert_same(got2, want2, "an array of weights")
    assert all(got2[0][a].tobytes() != got[0][a].tobytes() for a in range(n_actors)), "the array did not override the layout's weights"
    for a in range(n_actors):
        assert_numpy(got2, a, parents, ib, B.blended(clips, masks, CD.with_values(layers, CD.split(layers)[0], other)[a]), "an array of weights")
    poisoned = other.copy()
    poisoned[:, 0] = np.nan
    t, _ = CD.split(layers)
    dt, dw = on_device(gpu, t), on_device(gpu, poisoned)
    device.set_blend_device(dt.ptr, dw.ptr)
    assert_same(reads(device, 0, n_actors), got2, "a NaN weight on the base layer")
    # ... and the layout's own weights are still there
    device.set_blend_device(dt.ptr)
    assert_same(reads(device, 0, n_actors), got, "weights == NULL again")
    dt.close(); dw.close(); device.close(); host.close(); shared.close()


# ---- the held pose as a base -------------------------------------------------------------------------------------------------------------------
def test_the_held_pose_as_a_base_and_back_to_back_calls(gpu, capi):
    """RT_SKELETON_CURRENT_POSE on layer 0 under an additive (or replacing) layer: two calls in a row, from two different pairs of device
    arrays and with nothing read in between, equal the host path called twice -- each call saw its own arrays, and each actor its own held pose"""
    n, n_actors = 65, 7
    parents, ib, clips, masks = CC.rig("random", n, seed=9)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    device, host = capi.Crowd(shared, n_actors), capi.Crowd(shared, n_actors)
    layout = [[(None, 0.0), (a % 3, 0.0, 0.5, (a % 4) - 1 if a % 4 else None, B.ADDITIVE if a != 3 else B.BLEND)] for a in range(n_actors)]
    with pytest.raises(capi.RtError, match=r"rt_crowd_set_layout: actor 0: layer 0 names RT_SKELETON_CURRENT_POSE: the crowd has no pose yet \(rt_crowd_set_poses") as e:
        device.set_layout(layout)
    assert e.value.code == -4 and device.layout() == 0
    poses = CC.actor_poses(parents, n_actors, seed=11)
    device.set_poses(poses); host.set_poses(poses)
    device.set_layout(layout)
    steps = []
    for step in range(2):
        t = np.array([[NAN, 0.3 + 0.1 * a + step] for a in range(n_actors)], F)         # (the time of a held base is not read)
        w = np.array([[NAN, 0.25 + 0.125 * ((a + step) % 5)] for a in range(n_actors)], F)
        steps.append((on_device(gpu, t), on_device(gpu, w), t, w))
    for dt, dw, _, _ in steps:                           # back to back: nothing is read, nothing waits
        device.set_blend_device(dt.ptr, dw.ptr)
    current = [p for p in poses]
    for _, _, t, w in steps:
        mine = CD.with_values(layout, np.where(np.isnan(t), F(0.0), t), np.where(np.isnan(w), F(1.0), w))
        host.set_blend(mine)
        current = [B.blended(clips, masks, mine[a], current[a]) for a in range(n_actors)]
    got = reads(device, 0, n_actors)
    assert_same(got, reads(host, 0, n_actors), "the held pose, two calls")
    for a in range(n_actors):
        assert_numpy(got, a, parents, ib, current[a], "the held pose, two calls")
    assert len({got[0][a].tobytes() for a in range(n_actors)}) == n_actors
    for dt, dw, _, _ in steps:
        dt.close(); dw.close()
    device.close(); host.close(); shared.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages(gpu, capi):
    """every refusal with its code and message; a refused call leaves every read, and the layout, unchanged; a layout goes stale when the
    skeleton's clips or masks are cleared, not when one is added; a fresh layout after re-adding the clips works"""
    lib = capi.lib()
    n, n_actors = 9, 4
    parents, ib, clips, masks = CC.rig("random", n, seed=2)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    crowd, host = capi.Crowd(shared, n_actors), capi.Crowd(shared, n_actors)
    ok = [(0, 0.0), (1, 0.5, 0.5, None, B.BLEND)]
    t = np.array([[0.1 * a, 0.5 + 0.2 * a] for a in range(n_actors)], F)
    dt = on_device(gpu, t)
    with pytest.raises(capi.RtError, match=r"rt_crowd_set_blend_device: the crowd has no layout \(rt_crowd_set_layout gives it one\)") as e:
        crowd.set_blend_device(dt.ptr)
    assert e.value.code == -4
    crowd.set_layout([ok] * n_actors)
    assert lib.rt_crowd_set_blend_device(crowd.h, None, None) == -1 and b"null" in lib.rt_last_error()
    with pytest.raises(capi.RtError, match="the crowd has no pose yet"):
        crowd.pose()                                     # (nothing has posed it: not the layout, not a refused call)
    crowd.set_blend_device(dt.ptr)
    before = reads(crowd, 0, n_actors)

    def unchanged(what):
        assert crowd.layout() == 2, what
        assert_same(reads(crowd, 0, n_actors), before, what)
        crowd.set_blend_device(dt.ptr)                   # ... and the layout it had still poses what it posed
        assert_same(reads(crowd, 0, n_actors), before, what + ": the layout it had")

    for at in (0, n_actors // 2, n_actors - 1):
        for bad, code, message in (
                ([(0, 0.0), (1, 0.5, 0.5, None, 2)], -1, r"actor %d: layer 1 has mode 2: RT_LAYER_BLEND \(0\) or RT_LAYER_ADDITIVE \(1\)"),
                ([(0, 0.0, 1.0, None, B.ADDITIVE), ok[1]], -1, r"actor %d: layer 0 is additive: the base layer is RT_LAYER_BLEND"),
                ([(0, 0.0), (None, 0.0)], -1, r"actor %d: layer 1 names RT_SKELETON_CURRENT_POSE: only layer 0 may"),
                ([(3, 0.0), ok[1]], -4, r"actor %d: layer 0 names clip 3: the skeleton has 3 \(rt_skeleton_add_clip adds one\)"),
                ([(0, 0.0), (1, 0.5, 0.5, 3, B.BLEND)], -4, r"actor %d: layer 1 names mask 3: the skeleton has 3 \(rt_skeleton_add_mask adds one\)")):
            layers = [ok] * n_actors
            layers[at] = bad
            with pytest.raises(capi.RtError, match="rt_crowd_set_layout: " + message % at) as e:
                crowd.set_layout(layers)
            assert e.value.code == code, message
        unchanged("a bad actor %d" % at)
    # arguments before state, across actors; the first bad actor wins; a NaN time is no refusal
    with pytest.raises(capi.RtError, match=r"rt_crowd_set_layout: actor 3: layer 1 has mode 7") as e:
        crowd.set_layout([[(7, 0.0), ok[1]], ok, ok, [(0, 0.0), (1, 0.5, 0.5, None, 7)]])
    assert e.value.code == -1
    with pytest.raises(capi.RtError, match=r"rt_crowd_set_layout: actor 1: layer 0 names clip 5") as e:
        crowd.set_layout([ok, [(5, NAN), ok[1]], ok, [(9, 0.0), ok[1]]])
    assert e.value.code == -4
    for n_layers in (0, 9):
        a = np.zeros((n_actors, n_layers), capi.Skeleton.layers([]).dtype)
        assert lib.rt_crowd_set_layout(crowd.h, n_layers, a.ctypes.data) == -1 and b"rt_crowd_set_layout: %d layers: 1 .. 8 are supported" % n_layers in lib.rt_last_error()
    unchanged("layouts refused")
    lib.rt_debug_set_alloc_limit(64)                     # the slots cannot be allocated: nothing changes
    with pytest.raises(capi.RtError, match="hipMalloc") as e:
        crowd.set_layout([ok + [ok[1]]] * n_actors)
    assert e.value.code == -5
    lib.rt_debug_set_alloc_limit(0)
    unchanged("the slots could not be allocated")
    # the host's calls neither use the layout nor disturb it
    crowd.set_times([0, 1, 2, 1], [0.0, 0.5, 0.2, 9.0])
    crowd.set_blend([[(2, 0.1), (0, 0.0, 0.25, 1, B.ADDITIVE), (1, 0.3)]] * n_actors)
    crowd.set_poses(CC.actor_poses(parents, n_actors, seed=1))
    crowd.set_blend_device(dt.ptr)
    unchanged("after set_times, set_blend and set_poses")
    # adding keeps ids and addresses: not stale
    extra = S.clip(parents, 4, 99)
    assert shared.add_clip(*extra) == 3 and shared.add_mask(masks[0]) == 3
    crowd.set_blend_device(dt.ptr)
    unchanged("a clip and a mask added")
    # clearing frees what the slots point to: stale, whichever was cleared
    shared.clear_masks()
    with pytest.raises(capi.RtError, match=r"rt_crowd_set_blend_device: the layout is stale: the skeleton's masks were cleared after it was set \(rt_crowd_set_layout sets a new one\)") as e:
        crowd.set_blend_device(dt.ptr)
    assert e.value.code == -4 and crowd.layout() == 2
    assert_same(reads(crowd, 0, n_actors), before, "a stale layout")
    crowd.set_layout([ok] * n_actors)                    # (no layer names a mask)
    crowd.set_blend_device(dt.ptr)
    assert_same(reads(crowd, 0, n_actors), before, "a fresh layout after the masks were cleared")
    shared.clear_masks()                                 # nothing to clear: nothing goes stale
    crowd.set_blend_device(dt.ptr)
    shared.clear_clips()
    with pytest.raises(capi.RtError, match=r"rt_crowd_set_blend_device: the layout is stale: the skeleton's clips were cleared after it was set \(rt_crowd_set_layout sets a new one\)") as e:
        crowd.set_blend_device(dt.ptr)
    assert e.value.code == -4
    assert_same(reads(crowd, 0, n_actors), before, "a stale layout")
    with pytest.raises(capi.RtError, match=r"rt_crowd_set_layout: actor 0: layer 0 names clip 0: the skeleton has 0") as e:
        crowd.set_layout([ok] * n_actors)
    assert e.value.code == -4
    with pytest.raises(capi.RtError, match="the layout is stale"):
        crowd.set_blend_device(dt.ptr)
    # a fresh layout after re-adding the clips works
    assert [shared.add_clip(*c) for c in clips] == [0, 1, 2]
    with pytest.raises(capi.RtError, match="the layout is stale"):
        crowd.set_blend_device(dt.ptr)                   # (the ids are back, the addresses are not)
    crowd.set_layout([ok] * n_actors)
    crowd.set_blend_device(dt.ptr)
    host.set_blend(CD.with_values([ok] * n_actors, t))
    assert_same(reads(crowd, 0, n_actors), reads(host, 0, n_actors), "a fresh layout after re-adding the clips")
    assert_same(reads(crowd, 0, n_actors), before, "... which are the clips it had")
    dt.close(); crowd.close(); host.close(); shared.close()


# ---- an attached scene -------------------------------------------------------------------------------------------------------------------------
def test_a_scene_attached_to_a_device_driven_crowd(gpu, capi):
    """4 actors x 2 boxes: set_blend_device + update gives every scene array of the host path's scene and of a fresh build; between the call and
    the update the scene is stale the way a scene attached to a pose source is (include/dxr_amd.h, "Attached instances": posing touches no
    scene, which stays in the state of its last update; the call counts one pose, so the update is not a no-op and applies it)"""
    n, n_actors, n_inst = 9, 4, 8
    parents, ib, clips, masks = CC.rig("random", n, seed=8)
    for _, keys in clips:
        keys[:, :, 0:3] *= F(4.0)                          # (apart enough for a tree with some depth)
    shared = skeleton_with(capi, gpu, parents, ib, clips, masks)
    device, host = capi.Crowd(shared, n_actors), capi.Crowd(shared, n_actors)
    actors = np.repeat(np.arange(n_actors, dtype=np.uint32), 2)
    joints = np.array([3, 8, 0, 5, 7, 1, 2, 6], np.uint32)
    local = np.stack(random_xforms(n_inst, 21, spread=3.0)).astype(F).reshape(n_inst, 12)
    start = random_xforms(n_inst, 3, spread=6.0)
    a, b = scene_of(capi, gpu, start), scene_of(capi, gpu, start)
    a.attach_crowd(0, device, actors, joints, local)
    b.attach_crowd(0, host, actors, joints, local)
    layout = [[(x % 3, 0.0), ((x + 1) % 3, 0.0, 0.5, x % 3, x % 2)] for x in range(n_actors)]
    device.set_layout(layout)
    with pytest.raises(capi.RtError, match=r"instance 0 is attached to a crowd that has no pose yet") as e:
        a.update()                                       # (a layout is no pose)
    assert e.value.code == -4
    for step in range(2):
        t = np.array([[0.2 + 0.37 * x + step, 0.9 - 0.1 * x + step] for x in range(n_actors)], F)
        w = np.array([[1.0, 0.25 + 0.25 * ((x + step) % 3)] for x in range(n_actors)], F)
        dt, dw = on_device(gpu, t), on_device(gpu, w)
        device.set_blend_device(dt.ptr, dw.ptr)
        host.set_blend(CD.with_values(layout, t, w))
        if step:
            # posing touches no scene: until the update the scene stands, traceable, in the state of its last update -- stale against the crowd
            assert a.transforms().tobytes() == want.tobytes(), "the transforms of the pose before, until the update"
            assert_bytes_equal(arrays(a, n_inst), got, "between the call and the update: the arrays of the pose before")
            assert device.joints().tobytes() != W.tobytes(), "the crowd has moved on"
        a.update(); b.update()
        what = "pose %d" % step
        W = device.joints()
        want = np.stack([S.compose(W[actors[k], joints[k]][None], local[k][None])[0] for k in range(n_inst)])
        assert a.transforms().tobytes() == want.tobytes() == b.transforms().tobytes(), what
        got = arrays(a, n_inst)
        assert_bytes_equal(got, arrays(b, n_inst), what + " vs the host path's scene")
        fresh = scene_of(capi, gpu, list(want))
        assert_bytes_equal(got, arrays(fresh, n_inst), what + " vs a fresh build")
        if step:
            assert got["invs"].tobytes() != before["invs"].tobytes(), "the update applied the pose: the call counted one"
        before = got
        fresh.close(); dt.close(); dw.close()
    a.close(); b.close(); device.close(); host.close(); shared.close()


# ---- the example -----------------------------------------------------------------------------------------------------------------------------
def test_device_crowd_example_through_the_cpp_mirror(tmp_path):
    """examples/realtime_crowd_device.cpp: RtCrowd::setLayout and one upload of every frame's times and weights, then one
    RtCrowd::setBlendDevice and one RtScene::update per frame, end to end; driven through RtCrowd::setBlend instead, the frame is the same frame"""
    exe = os.path.join(S.ROOT, "dxrexperiments_amd", "lib", "realtime_crowd_device")
    images, sums = [], []
    for frames, how in ((1, "device"), (3, "device"), (3, "host")):
        out = tmp_path / ("out%d%s.pfm" % (frames, how))
        r = subprocess.run([exe, "96", "64", str(frames), str(out)] + (["host"] if how == "host" else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert "actors, posed from %s: %d frames" % ("device times" if how == "device" else "host layers", frames) in r.stdout and "TLAS update" in r.stdout
        sums.append(r.stdout.strip().rsplit(" ", 1)[-1])
        raw = out.read_bytes()
        head = b"PF\n96 64\n-1.0\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], "<f4").reshape(64, 96, 3))
    assert images[0].max() > 0.1 and images[0].std() > 0.01            # an image, not a constant
    assert not np.array_equal(images[0], images[1]), "the crowd did not move"
    assert sums[1] == sums[2] and np.array_equal(images[1], images[2]), "device times and host layers give different frames"
