"""The resolve pass of a set of frames against the oracle, frame after frame, and against the same frames rendered one by one.

k_resolve walks the frames of a pixel inside one thread and reads each frame's constants (camera jitter, lights, options, frameCount,
accumCount) in place from the set's array.  Every case here renders frames that all differ -- an unpaused host with the time advancing
moves the directional light, the point light gets a position of its own per frame, the jitter is drawn per frame -- so a kernel that
shaded frame f with the constants of frame 0, of frame f + 1, or of the frame before would miss the oracle's bits.  Every image is compared
bit for bit with the oracle (oracle.pyoracle.Scene.render, frame after frame) and with immediate rendering (set_deferred(0)); ray totals
with the sums of the oracle's per-frame statistics.

Scene: an open-sided room of 166 triangles with three occluders, three instances with three materials (type 1 with a specular ray,
type 2 with reflectivity 0.0005 -- no specular ray, its slot stays "not traced" -- and type 0), seen so that primary rays hit, miss
(through the open side) and reach lit and shadowed points.  Output 48x40: 6x5 whole 8x8 tiles, so the cases about the frame and slot
boundaries also run at 45x37, where the last tile column and row hold slots outside the image."""
import numpy as np
import pytest

from dxrexperiments_amd import rtypes as T, scenes
from util import cam_array

pytestmark = pytest.mark.gpu

COUNTS = ("rays_primary", "rays_secondary", "rays_shadow", "primary_hits", "secondary_hits")
CAMERA = dict(eye=(2.5, 2.6, 9.5), at=(-0.2, 2.0, -1.0), up=(0.0, 1.0, 0.0), fov=0.9)
ENV = scenes.sky_cubemap(8)


def _quad(a, b, c, d, n):
    """n x n cells of the quad a b c d (counter-clockwise seen from its front), two triangles each"""
    a, b, c, d = (np.asarray(p, np.float64) for p in (a, b, c, d))
    tris = []
    for i in range(n):
        for j in range(n):
            u0, u1, v0, v1 = i / n, (i + 1) / n, j / n, (j + 1) / n
            p = lambda u, v: (a * (1 - u) + b * u) * (1 - v) + (d * (1 - u) + c * u) * v
            tris += [(p(u0, v0), p(u1, v0), p(u1, v1)), (p(u0, v0), p(u1, v1), p(u0, v1))]
    return tris


def _box(centre, half):
    c, h = np.asarray(centre, np.float64), np.asarray(half, np.float64)
    k = lambda sx, sy, sz: c + h * (sx, sy, sz)
    faces = [(k(-1, -1, 1), k(1, -1, 1), k(1, 1, 1), k(-1, 1, 1)), (k(1, -1, -1), k(-1, -1, -1), k(-1, 1, -1), k(1, 1, -1)),
             (k(1, -1, 1), k(1, -1, -1), k(1, 1, -1), k(1, 1, 1)), (k(-1, -1, -1), k(-1, -1, 1), k(-1, 1, 1), k(-1, 1, -1)),
             (k(-1, 1, 1), k(1, 1, 1), k(1, 1, -1), k(-1, 1, -1)), (k(-1, -1, -1), k(1, -1, -1), k(1, -1, 1), k(-1, -1, 1))]
    return [t for f in faces for t in _quad(*f, 1)]


def _mesh(tris):
    p = np.asarray(tris, np.float64).reshape(-1, 3).astype(np.float32)
    v = np.zeros(p.shape[0], T.VERTEX)
    v["position"] = p
    fn = np.cross(p[1::3] - p[0::3], p[2::3] - p[0::3])
    v["normal"] = np.repeat((fn / np.linalg.norm(fn, axis=1, keepdims=True)).astype(np.float32), 3, axis=0)
    return v, np.arange(p.shape[0], dtype=np.uint32).reshape(-1, 3)


def room_models():
    """floor, back wall, left wall and half a ceiling facing inward (the right side and the front are open); two boxes on the floor;
    a slab that floats under the point light"""
    room = (_quad((-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), 4) + _quad((-4, 0, -4), (4, 0, -4), (4, 5, -4), (-4, 5, -4), 4)
            + _quad((-4, 0, 4), (-4, 0, -4), (-4, 5, -4), (-4, 5, 4), 4) + _quad((-4, 5, -4), (0, 5, -4), (0, 5, 4), (-4, 5, 4), 4))
    boxes = _box((-1.5, 0.75, -1.0), (0.75, 0.75, 0.75)) + _box((1.6, 1.5, -2.0), (0.5, 1.5, 0.5))
    slab = _box((0.0, 3.2, 0.5), (1.0, 0.15, 1.0)) + _quad((2.0, 0.0, 1.0), (3.0, 0.0, 0.0), (3.0, 2.0, 0.0), (2.0, 2.0, 1.0), 1)
    models = [_mesh(room), _mesh(boxes), _mesh(slab)]
    assert sum(len(i) for _, i in models) <= 500
    return models


def room_materials():
    a, b, c = T.default_material(), T.default_material(), T.default_material()
    a["albedo"] = (0.7, 0.7, 0.65, 1.0); a["reflectivity"] = 0.5; a["roughness"] = 0.4            # type 1: diffuse and specular ray
    b["albedo"] = (0.1, 0.5, 0.9, 1.0); b["type"] = 2; b["reflectivity"] = 0.0005                 # no specular ray: the slot is "not traced"
    c["albedo"] = (0.9, 0.8, 0.1, 1.0); c["type"] = 0; c["emissive"] = (0.2, 0.1, 0.0, 0.5)       # the other branch of mp.type
    return [a, b, c]


MODELS = room_models()
INSTANCES = [(0, None), (1, None), (2, None)]
MATS = room_materials()
_oracle_scene = []
_references = {}


def oracle_scene(oracle):
    if not _oracle_scene:
        sc = oracle.Scene()
        for v, i in MODELS:
            sc.add_model(v, i)
        for mi, x in INSTANCES:
            sc.add_instance(mi, x)
        sc.build()
        _oracle_scene.append(sc)
    return _oracle_scene[0]


def gpu_pipeline(capi, gpu, W, H, kind=None):
    sc = capi.Scene(gpu)
    for v, i in MODELS:
        sc.add_model(capi.Model(gpu, v, i))
    p = capi.Pipeline(gpu) if kind is None else capi.Pipeline(gpu, kind)
    p.set_scene(sc)
    for m in MATS:
        p.add_material(m)
    p.set_environment_cube(ENV)
    p.create_output(W, H)
    p.build_acceleration_structures()
    return p


def frames_of(capi, n, W, H, options=None, realtime=False):
    """n frames of an unpaused host, 0.37 s apart: every frame its own jitter, directional light and point light"""
    host = capi.ProgressiveHost(17)
    host.set_flags(True, False)
    for k, v in (options or {}).items():
        host.options[k] = v
    cam = cam_array(CAMERA, W / H)
    out = []
    for f in range(n):
        c = (host.update_realtime if realtime else host.update)(cam, 3.0 + 0.37 * f, f + 1, W, H)
        c["pointLight"]["worldPos"] = (-1.0 + 0.06 * f, 4.2 - 0.02 * f, 0.5 + 0.05 * f, 1.0)
        out.append(c)
    assert len({c["directionalLight"]["forwardDir"].tobytes() for c in out}) == n
    assert len({c["cameraParams"]["jitters"].tobytes() for c in out}) == n
    return out


def reference(oracle, key, pfcs, W, H, **kw):
    """the oracle's image and summed statistics after these frames; computed once per key, handed out read-only"""
    if key not in _references:
        osc = oracle_scene(oracle)
        acc = np.zeros((H, W, 4), np.float32)
        total = dict.fromkeys(COUNTS, 0)
        for c in pfcs:
            acc, st = osc.render(np.stack(MATS), c, W, H, accum=acc, env_faces=ENV, nthreads=8, **kw)
            for k in COUNTS:
                total[k] += st[k]
        acc.setflags(write=False)
        _references[key] = (acc, total)
    return _references[key]


def render_frames(p, pfcs, S):
    """the frames through update() + render() with sets of S (0: immediate); the read renders what is still held"""
    p.set_deferred(S)
    p.clear_output()
    p.reset_totals()
    for c in pfcs:
        p.update(c)
        p.render()
    return p.read_output(), p.totals()


def check(p, oracle, key, pfcs, W, H, sets, **oracle_kw):
    want, counts = reference(oracle, key, pfcs, W, H, **oracle_kw)
    for S in (0, *sets):
        img, tot = render_frames(p, pfcs, S)
        assert np.array_equal(img, want), "sets of %d: %d pixels differ from the oracle" % (S, int((img != want).any(axis=2).sum()))
        for k in COUNTS:
            assert tot[k] == counts[k], (S, k, tot[k], counts[k])
        assert tot["frames"] == len(pfcs)
    return want, counts


@pytest.mark.parametrize("S", [1, 2, 3, 32])
def test_per_frame_constants(gpu, capi, oracle, S):
    """as many frames as the set holds plus one more set of them, every frame with constants of its own"""
    W, H = 48, 40
    n = {1: 3, 2: 6, 3: 9, 32: 32}[S]
    pfcs = frames_of(capi, n, W, H)
    p = gpu_pipeline(capi, gpu, W, H)
    want, counts = check(p, oracle, ("default", W, H, n), pfcs, W, H, [S])
    assert 0 < counts["primary_hits"] < n * W * H                 # rays hit and miss
    lum = want[..., :3].sum(axis=2)
    assert lum.min() < 0.25 * lum.max()                          # shadowed and lit points


@pytest.mark.parametrize("size", [(48, 40), (45, 37)])
@pytest.mark.parametrize("n,S", [(7, 3), (8, 3), (5, 5), (4, 32)])
def test_last_frame_of_a_set_and_slots_outside_the_image(gpu, capi, oracle, size, n, S):
    """whatever the resolve pass reads ahead for frame f + 1 must not be used -- or fetched from beyond the queues -- behind the last frame
    of a set: sets that end on a full set, on a partial one, on a single frame; at 45x37 the last tile row and column hold slots outside
    the image (threads that take no part), and the last slots of the set's queues belong to them"""
    W, H = size
    pfcs = frames_of(capi, n, W, H)
    p = gpu_pipeline(capi, gpu, W, H)
    check(p, oracle, ("default", W, H, n), pfcs, W, H, [S])


@pytest.mark.parametrize("limits", [(0, 0), (0, 2), (1, 0), (1, 2), (2, 2)])
def test_depth_limits(gpu, capi, oracle, limits):
    """(0, x): no level-1 queue is bound; (2, 2): k_shade_level and the level-by-level resolve"""
    W, H = 48, 40
    pfcs = frames_of(capi, 5, W, H)
    p = gpu_pipeline(capi, gpu, W, H)
    p.set_depth_limits(*limits)
    _, counts = check(p, oracle, ("limits", limits), pfcs, W, H, [3], max_radiance_depth=limits[0], max_shadow_depth=limits[1])
    assert (counts["rays_secondary"] > 0) == (limits[0] > 0) and (counts["rays_shadow"] > 0) == (limits[1] > 0)


def test_no_specular_ray_leaves_untraced_slots(gpu, capi, oracle):
    """the materials of type 2 with reflectivity 0.0005 and of type 0 spawn a diffuse ray only: fewer secondary rays than two per hit"""
    W, H = 48, 40
    pfcs = frames_of(capi, 4, W, H)
    p = gpu_pipeline(capi, gpu, W, H)
    _, counts = check(p, oracle, ("default", W, H, 4), pfcs, W, H, [4])
    assert counts["primary_hits"] < counts["rays_secondary"] < 2 * counts["primary_hits"]


@pytest.mark.parametrize("view", ["skip_unlit", "one_light", "ambient_occlusion", "sum", "running_mean", "rgba16f"])
def test_views_and_modes(gpu, capi, oracle, view):
    W, H = 48, 40
    options = {"one_light": {"debug": 2}, "ambient_occlusion": {"showAmbientOcclusionOnly": 1}}.get(view)
    pfcs = frames_of(capi, 5, W, H, options=options)
    p = gpu_pipeline(capi, gpu, W, H)
    kw = {}
    if view == "skip_unlit":
        p.set_skip_unlit_shadow_rays(True)
    if view == "sum":
        p.set_accumulation_mode(T.ACCUM_SUM)
        kw["accum_mode"] = T.ACCUM_SUM
    if view == "running_mean":
        p.set_accumulation_mode(T.ACCUM_RUNNING_MEAN)
    if view == "rgba16f":
        p.set_accumulation_storage(T.FORMAT_R16G16B16A16_FLOAT, T.ROUND_NEAREST_EVEN)
        kw["accum_f16"] = 1
    key = ("default", W, H, 5) if view in ("skip_unlit", "running_mean") else ("view", view)
    _, counts = check(p, oracle, key, pfcs, W, H, [3], **kw)
    if view == "ambient_occlusion":
        assert counts["rays_shadow"] == 4 * counts["primary_hits"] and counts["rays_secondary"] == 0
    if view == "one_light":
        assert counts["rays_shadow"] == counts["primary_hits"] + counts["secondary_hits"]
    if view == "skip_unlit":
        assert 0 < p.totals()["rays_shadow_skipped"] < counts["rays_shadow"]


def test_realtime_pipeline_writes_its_aovs(gpu, capi, oracle):
    """a realtime-kind pipeline keeps no accumulator and takes no part in sets (render_batch and set_deferred refuse it): every frame goes
    through the single-frame resolve kernel, which shares its shading functions with the set form, and leaves both AOVs of that frame"""
    W, H = 48, 40
    pfcs = frames_of(capi, 3, W, H, realtime=True)
    p = gpu_pipeline(capi, gpu, W, H, kind=capi.PIPELINE_REALTIME)
    with pytest.raises(capi.RtError):
        p.render_batch(pfcs)
    with pytest.raises(capi.RtError):
        p.set_deferred(3)
    osc = oracle_scene(oracle)
    p.reset_totals()
    total = dict.fromkeys(COUNTS, 0)
    for c in pfcs:
        p.update(c)
        p.render()
        direct, indirect, st = osc.render_realtime(np.stack(MATS), c, W, H, env_faces=ENV, nthreads=8)
        for k in COUNTS:
            total[k] += st[k]
        assert np.array_equal(p.read_output(0), direct) and np.array_equal(p.read_output(1), indirect)
    tot = p.totals()
    for k in COUNTS:
        assert tot[k] == total[k], (k, tot[k], total[k])
