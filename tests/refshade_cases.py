"""The cases of the refshade check: what tests/golden/make_refshade.py records from the reference's own shading text compiled as C++
(oracle/refshade, oracle/_ref/librefshade.so) and what tests/test_refshade.py (CPU: the oracle) and tests/test_gpu_refshade.py (the
kernels) are held to, bit for bit.  A plain module, as tests/s2_truth.py.

A "backend" computes the cases: Ref (librefshade.so; only where the reference checkout was there at build time) or Orc (the
oracle).  The GPU test has its own in tests/test_gpu_refshade.py.  compute_units() / compute_frame() return dicts of arrays; the
committed fixtures are exactly those dicts, one .npz per case under tests/golden/refshade/.
"""
import ctypes as C
import os

import numpy as np

from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_pipeline import OPTION_CASES
from util import CORNELL_OBJ, GOLDEN, random_xforms, triangle_soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "librefshade.so")
FIXTURES = os.path.join(GOLDEN, "refshade")
N_UNIT = 4096
ROUGHNESS = (0.0, 0.5, 1.0)
SAMPLE = dict(cos=0, uniform=1, phong=2, perp=3)


def same_bits(a, b):
    """equal bit for bit; a NaN equals a NaN whatever its payload (x86 and gfx950 produce different default NaNs)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(a) & np.isnan(b)
    return np.array_equal(a.view(u)[~nan], b.view(u)[~nan])


# ---- unit vectors -------------------------------------------------------------------------------------------------------------

def unit_inputs():
    r = np.random.default_rng(2024)
    v0 = r.integers(0, 2 ** 32, N_UNIT, dtype=np.uint64).astype(np.uint32)
    v1 = r.integers(0, 2 ** 32, N_UNIT, dtype=np.uint64).astype(np.uint32)
    v0[:8] = [0, 1, 2, 95, 96 * 80 - 1, 0xFFFFFFFF, 0, 0x80000000]              # pixel indices and frame counts as the shaders seed with
    v1[:8] = [0, 1, 1, 2, 3, 0xFFFFFFFF, 0xFFFFFFFF, 7]
    seeds = r.integers(0, 2 ** 32, N_UNIT, dtype=np.uint64).astype(np.uint32)
    seeds[:4] = [0, 1, 0xFFFFFFFF, 0x00FFFFFF]
    d = r.standard_normal((N_UNIT, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    # where getPerpendicularVector's branches flip: the axes, two equal components, all equal, signed zeros, one tiny component
    s = np.float32(np.sqrt(0.5))
    t = np.float32(1.0 / np.sqrt(3.0))
    special = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
               (s, s, 0), (s, 0, s), (0, s, s), (-s, s, 0), (s, 0, -s), (0, -s, -s), (s, -s, 0),
               (t, t, t), (-t, t, t), (t, -t, t), (t, t, -t), (-t, -t, -t),
               (-0.0, 1, 0), (0.0, 1, -0.0), (1, -0.0, -0.0), (-0.0, -0.0, 1), (-0.0, -1, 0.0),
               (1e-30, 1, 0), (1, 1e-30, 0), (0, 1, 1e-30), (1e-45, s, s), (s, 1e-45, s), (s, s, -1e-45), (1e-20, 1e-20, 1),
               (0.6, 0.8, 0), (0.8, 0.6, 0), (0, 0.6, 0.8), (0.6, 0, 0.8)]
    d[:len(special)] = np.array(special, np.float32)
    n = r.standard_normal((N_UNIT, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = n.astype(np.float32)
    n[:8] = d[:8]                                                                 # I == N, I == -N ... : cosi saturates at both ends
    n[8:16] = -d[8:16]
    f0 = r.uniform(0, 1, (N_UNIT, 3)).astype(np.float32)
    f0[:3] = [(0.58, 0.58, 0.58), (0, 0, 0), (1, 1, 1)]
    return dict(v0=v0, v1=v1, seeds=seeds, dirs=d, normals=n, f0=f0, roughness=np.array(ROUGHNESS, np.float32))


def compute_units(backend):
    i = unit_inputs()
    out = dict(i)
    out["rng_seed"], out["rng_state"], out["rng_rand"] = backend.rng(i["v0"], i["v1"])
    out["exponents"] = np.array([backend.exponent(x) for x in ROUGHNESS], np.float32)
    for kind in ("cos", "uniform", "perp"):
        o, _, so = backend.sample(kind, i["seeds"], i["dirs"], 0.0)
        out[kind + "_out"], out[kind + "_seed"] = o, so
    for k, e in enumerate(out["exponents"]):
        o, pb, so = backend.sample("phong", i["seeds"], i["dirs"], float(e))
        out["phong%d_out" % k], out["phong%d_pdf_brdf" % k], out["phong%d_seed" % k] = o, pb, so
    out["fresnel_out"] = backend.fresnel(i["dirs"], i["normals"], i["f0"])
    return out


# ---- frames --------------------------------------------------------------------------------------------------------------------

def _scene(name):
    """-> (models [(verts, idx) or an .obj path], instances [(model, xform or None)])"""
    if name == "cornell":
        return [CORNELL_OBJ], [(0, None)]
    if name == "instanced":                     # tests/test_gpu_pipeline.py test_instanced_scene_materials_and_misses
        xf = random_xforms(24, seed=5, spread=6.0)
        return [scenes.blob_mesh(level=2), triangle_soup(200, seed=2, extent=1.5, size=0.5)], [(k % 2, xf[k]) for k in range(24)] + [(0, None)]
    if name == "instanced12":                   # tests/test_gpu_realtime_denoise.py test_realtime_pipeline_instanced_with_misses
        xf = random_xforms(12, seed=8, spread=5.0)
        return [scenes.blob_mesh(level=2), triangle_soup(150, seed=4, extent=1.5, size=0.5)], [(k % 2, xf[k]) for k in range(12)]
    raise KeyError(name)


def _cam(c, aspect):
    return np.array([*c["eye"], *c["at"], *c["up"], c["fov"], aspect], np.float32)


def _pfcs(orc, host_seed, cam, W, H, frames, opts=None, realtime=False):
    """per-frame constants by the oracle's restatement of the reference's update() (inputs only: the fixtures record them)"""
    host = orc.Progressive(host_seed)
    o = np.frombuffer(host.options_buffer(), dtype=T.DEBUG_OPTIONS, count=1)
    for k, v in (opts or {}).items():
        o[k] = v
    out = []
    for f in frames:
        p = np.frombuffer(host.update(cam, 0.0, f, W, H).tobytes(), T.PER_FRAME_CONSTANTS, count=1)[0].copy()
        if realtime:                             # RealtimeRaytracingPipeline::update: no accumulation, no iteration limit
            p["cameraParams"]["accumCount"] = 0
            p["options"]["maxIterations"] = 0
        out.append(p)
    return np.stack(out)


def _opt_id(o):
    return "-".join("%s=%s" % kv for kv in o.items()) or "defaults"


def frame_cases(orc):
    """every recorded frame: name -> dict(kind, scene, W, H, mats, env (cube side or 0), env_constant, pfcs, storages)"""
    cases = {}
    cornell = scenes.cornell_camera()

    def add(name, kind, scene, W, H, mats, env, pfcs, storages=("fp32", "f16n"), env_constant=(0.5, 0.5, 0.5), per_frame=False):
        assert CASE_SHAPES[name] == dict(scene=scene, W=W, H=H, env=env), name
        cases[name] = dict(kind=kind, scene=scene, W=W, H=H, mats=np.atleast_1d(np.asarray(mats, T.MATERIAL_PARAMS)), env=env,
                           env_constant=np.array(env_constant, np.float32), pfcs=pfcs, storages=storages, per_frame=per_frame)

    for o in OPTION_CASES:                       # tests/test_gpu_pipeline.py test_cornell_options_vs_oracle: 96 x 80, two frames
        W, H = 96, 80
        add("opt_" + _opt_id(o), "progressive", "cornell", W, H, T.default_material(), 16, _pfcs(orc, 7, _cam(cornell, W / H), W, H, (1, 2), o),
            storages=("fp32", "f16n", "f16z") if not o else ("fp32", "f16n"))
    for mtype, refl in ((0, 0.7), (2, 0.4), (1, 0.0)):       # test_material_types_and_depth_limits, at the text's depth limits
        W, H = 64, 48
        m = T.default_material()
        m["type"], m["reflectivity"], m["emissive"] = mtype, refl, (0.1, 0.2, 0.3, 0.5)
        p = _pfcs(orc, 3, _cam(cornell, W / H), W, H, (5,))
        p["cameraParams"]["accumCount"] = 0
        add("material_type%d" % mtype, "progressive", "cornell", W, H, m, 0, p)
    W, H = 96, 54                                # instances, one material each, misses into a cube environment
    r = np.random.default_rng(1)
    mats = []
    for k in range(25):
        m = T.default_material()
        m["albedo"][:3] = r.uniform(0.1, 0.9, 3)
        m["roughness"] = r.uniform(0.2, 0.9)
        m["type"] = k % 3
        mats.append(m)
    add("instanced", "progressive", "instanced", W, H, np.stack(mats), 8,
        _pfcs(orc, 11, _cam(dict(eye=(0, 3, 16), at=(0, 0, 0), up=(0, 1, 0), fov=0.8), W / H), W, H, (1, 2)))
    W, H = 64, 48                                # four accumulated frames: fp32, and RGBA16F under both roundings
    add("accumulate4", "progressive", "cornell", W, H, T.default_material(), 0, _pfcs(orc, 5, _cam(cornell, W / H), W, H, (1, 2, 3, 4)),
        storages=("fp32", "f16n", "f16z"), per_frame=True)
    W, H = 32, 32                                # frames three and four are past maxIterations = 2: RayGen returns at once
    add("past_max_iterations", "progressive", "cornell", W, H, T.default_material(), 0,
        _pfcs(orc, 1, _cam(cornell, 1.0), W, H, (1, 2, 3, 4), {"maxIterations": 2}), per_frame=True)
    W, H = 96, 80                                # the two realtime AOVs
    add("realtime_cornell", "realtime", "cornell", W, H, T.default_material(), 16, _pfcs(orc, 9, _cam(cornell, W / H), W, H, (1, 2), realtime=True))
    W, H = 96, 64
    mats = []
    for k in range(12):
        m = T.default_material()
        m["albedo"][:3] = (0.2 + 0.05 * k, 0.9 - 0.05 * k, 0.5)
        m["type"] = k % 3
        mats.append(m)
    add("realtime_instanced", "realtime", "instanced12", W, H, np.stack(mats), 8,
        _pfcs(orc, 10, _cam(dict(eye=(0, 2, 14), at=(0, 0, 0), up=(0, 1, 0), fov=0.8), W / H), W, H, (3,), realtime=True))
    return cases


def _shapes():
    """name -> scene, size and cube side of every case: what a fixture does not record (it records constants, materials and images)"""
    out = {"opt_" + _opt_id(o): dict(scene="cornell", W=96, H=80, env=16) for o in OPTION_CASES}
    out.update({"material_type%d" % t: dict(scene="cornell", W=64, H=48, env=0) for t in (0, 1, 2)})
    out.update(instanced=dict(scene="instanced", W=96, H=54, env=8), accumulate4=dict(scene="cornell", W=64, H=48, env=0),
               past_max_iterations=dict(scene="cornell", W=32, H=32, env=0), realtime_cornell=dict(scene="cornell", W=96, H=80, env=16),
               realtime_instanced=dict(scene="instanced12", W=96, H=64, env=8))
    return out


CASE_SHAPES = _shapes()

STORAGE_F16 = dict(fp32=0, f16n=1, f16z=2)       # accum_f16 of the oracle / accum_mode bits 8-9
STAT_KEYS = ("rays_primary", "rays_secondary", "rays_shadow", "primary_hits", "secondary_hits")


def env_faces(case):
    return scenes.sky_cubemap(case["env"]) if case["env"] else None


def build_scene(orc, scene):
    models, inst = _scene(scene)
    sc = orc.Scene()
    for m in models:
        v, i = orc.obj_load(m) if isinstance(m, str) else m
        sc.add_model(v, i)
    for mi, x in inst:
        sc.add_instance(mi, x)
    sc.build()
    return sc


def compute_frame(backend, orc, case):
    """the arrays a fixture holds: inputs (pfcs, mats) and, per storage, the image after the last frame; ray counts of the last frame"""
    sc = build_scene(orc, case["scene"])
    W, H, env = case["W"], case["H"], env_faces(case)
    out = dict(pfcs=case["pfcs"], mats=case["mats"])
    if case["kind"] == "realtime":
        for f, pfc in enumerate(case["pfcs"]):
            d, i, st = backend.render_realtime(sc, case["mats"], pfc, W, H, env, case["env_constant"])
            out["direct%d" % f], out["indirect%d" % f] = d, i
        out["stats"] = np.array([st[k] for k in STAT_KEYS], np.uint64)
        return out
    for storage in case["storages"]:
        acc = np.zeros((H, W, 4), np.float32)
        frames = []
        for pfc in case["pfcs"]:
            acc, st = backend.render(sc, case["mats"], pfc, W, H, acc, env, case["env_constant"], STORAGE_F16[storage])
            frames.append(acc.copy())
        img = np.stack(frames) if case["per_frame"] else acc
        out["image_" + storage] = img if storage == "fp32" else img.astype(np.float16)      # exact: every stored value is an fp16 number
        if storage != "fp32":
            assert np.array_equal(img.astype(np.float16).astype(np.float32), img)
    out["stats"] = np.array([st[k] for k in STAT_KEYS], np.uint64)
    return out


# ---- backends -------------------------------------------------------------------------------------------------------------------

class Orc:
    """the oracle (oracle/pyoracle.py)"""

    def __init__(self, orc):
        self.o = orc

    def rng(self, v0, v1):
        seed = np.array([self.o.init_rand(int(a), int(b)) for a, b in zip(v0, v1)], np.uint32)
        nxt = [self.o.next_rand(int(s)) for s in seed]
        return seed, np.array([s for s, _ in nxt], np.uint32), np.array([f for _, f in nxt], np.float32)

    def exponent(self, roughness):
        f = np.float32
        return float(self.o.math("exp", np.array([(f(1.0) - f(roughness)) * f(12.0)], np.float32))[0])

    def sample(self, kind, seeds, vecs, exponent):
        return self.o.sample(kind, seeds, vecs, exponent)

    def fresnel(self, I, N, f0):
        return np.stack([self.o.fresnel(I[k], N[k], f0[k]) for k in range(I.shape[0])])

    def render(self, sc, mats, pfc, W, H, acc, env, env_constant, f16):
        return sc.render(mats, pfc, W, H, accum=acc, env_faces=env, env_constant=env_constant, accum_f16=f16, nthreads=8)

    def render_realtime(self, sc, mats, pfc, W, H, env, env_constant):
        return sc.render_realtime(mats, pfc, W, H, env_faces=env, env_constant=env_constant, nthreads=8)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Ref:
    """oracle/_ref/librefshade.so: the reference's shading text behind oracle/refshade's shim and harness"""

    def __init__(self, orc):
        orc.lib()                                # liboracle.so first: librefshade.so links against it
        L = C.CDLL(REF_SO)
        p = C.c_void_p
        L.ref_rng_batch.argtypes = [p] * 5 + [C.c_size_t]
        L.ref_sample_batch.argtypes = [C.c_int, p, p, C.c_float, p, p, p, C.c_size_t]
        L.ref_fresnel_batch.argtypes = [p] * 4 + [C.c_size_t]
        L.ref_phong_exponent.restype = C.c_float
        L.ref_phong_exponent.argtypes = [C.c_float]
        L.ref_selftest_two_draws.argtypes = [p, p]
        L.ref_selftest_float_only.restype = C.c_float
        L.ref_selftest_float_only.argtypes = [C.c_float]
        L.ref_layout.argtypes = [p, C.c_int]
        L.ref_render_progressive.argtypes = [p, p, C.c_uint32, p, C.c_int, p, p] + [C.c_uint32] * 7 + [C.c_int, p, C.c_int, p]
        L.ref_render_realtime.argtypes = [p, p, C.c_uint32, p, C.c_int, p, p] + [C.c_uint32] * 2 + [p, p, C.c_int, p]
        self.L, self.o = L, orc

    def rng(self, v0, v1):
        n = v0.size
        seed, state, rand = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.float32)
        self.L.ref_rng_batch(_p(np.ascontiguousarray(v0)), _p(np.ascontiguousarray(v1)), _p(seed), _p(state), _p(rand), n)
        return seed, state, rand

    def exponent(self, roughness):
        return float(self.L.ref_phong_exponent(roughness))

    def sample(self, kind, seeds, vecs, exponent):
        seeds = np.ascontiguousarray(seeds, np.uint32)
        vecs = np.ascontiguousarray(vecs, np.float32).reshape(-1, 3)
        n = seeds.size
        out, pb, so = np.empty((n, 3), np.float32), np.empty((n, 2), np.float32), np.empty(n, np.uint32)
        self.L.ref_sample_batch(SAMPLE[kind], _p(seeds), _p(vecs), exponent, _p(out), _p(pb), _p(so), n)
        return out, pb, so

    def fresnel(self, I, N, f0):
        I, N, f0 = (np.ascontiguousarray(a, np.float32) for a in (I, N, f0))
        out = np.empty_like(I)
        self.L.ref_fresnel_batch(_p(I), _p(N), _p(f0), _p(out), I.shape[0])
        return out

    def two_draws(self, seed):
        s = np.array([seed], np.uint32)
        out = np.empty(2, np.float32)
        self.L.ref_selftest_two_draws(_p(s), _p(out))
        return int(s[0]), out

    def float_only(self, x):
        return np.float32(self.L.ref_selftest_float_only(float(x)))

    def layout(self):
        rows = np.zeros((512, 2), np.uint32)
        n = self.L.ref_layout(_p(rows), 512)
        assert 0 < n <= 512
        return rows[:n]

    def render(self, sc, mats, pfc, W, H, acc, env, env_constant, f16):
        mats, pfc = np.ascontiguousarray(mats), np.ascontiguousarray(pfc)
        env = None if env is None else np.ascontiguousarray(env, np.float32)
        ec = np.ascontiguousarray(env_constant, np.float32)
        st = self.o.RenderStats()
        rc = self.L.ref_render_progressive(sc.h, _p(mats), mats.nbytes // 64, _p(env), 0 if env is None else env.shape[1], _p(ec), _p(pfc),
                                           W, H, 0, 0, W, H, f16 << 8, 0, _p(acc), 1, C.byref(st))
        assert rc == 0, rc
        return acc, st.as_dict()

    def render_realtime(self, sc, mats, pfc, W, H, env, env_constant):
        mats, pfc = np.ascontiguousarray(mats), np.ascontiguousarray(pfc)
        env = None if env is None else np.ascontiguousarray(env, np.float32)
        ec = np.ascontiguousarray(env_constant, np.float32)
        d, i = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
        st = self.o.RenderStats()
        rc = self.L.ref_render_realtime(sc.h, _p(mats), mats.nbytes // 64, _p(env), 0 if env is None else env.shape[1], _p(ec), _p(pfc),
                                        W, H, _p(d), _p(i), 1, C.byref(st))
        assert rc == 0, rc
        return d, i, st.as_dict()


def fixture_path(name):
    return os.path.join(FIXTURES, name + ".npz")


def split_units(arrays):
    """the unit vectors as two files (each within the size bound of a committed fixture): the Phong lobe's outputs, and the rest"""
    return {"units_phong": {k: v for k, v in arrays.items() if k.startswith("phong")},
            "units": {k: v for k, v in arrays.items() if not k.startswith("phong")}}


def load_fixture(name):
    out = {}
    for n in ((name, "units_phong") if name == "units" else (name,)):
        with np.load(fixture_path(n)) as z:
            out.update({k: z[k] for k in z.files})
    return out
