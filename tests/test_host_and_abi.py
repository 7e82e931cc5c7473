"""CPU-only: the C-ABI library loads and exports every declared symbol; host-side frame
logic (camera basis, update()) matches the oracle and the committed fixture; the product
package never touches the oracle; multi-GPU host logic over gloo (world_size 2)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from dxrexperiments_amd import rtypes as T, scenes
from util import GOLDEN, cam_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(capi):
    names = declared_symbols()
    assert len(names) > 50
    lib = capi.lib()
    for n in names:
        assert hasattr(lib, n), "libdxrexperiments_amd.so does not export %s" % n
        assert n in capi.SIGNATURES, "capi.py has no signature for %s" % n
    assert set(capi.SIGNATURES) == set(names)
    assert b"gfx950" in lib.rt_version()


def test_no_gpu_means_loud_failure_not_fallback(capi):
    """On a machine without a HIP device the product must refuse to work."""
    try:
        n = capi.device_count()
    except capi.RtError:
        n = 0
    if n == 0:
        with pytest.raises(capi.RtError):
            capi.Context(0)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "dxrexperiments_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "pyoracle" not in text and "liboracle" not in text and "oracle/" not in text.replace("the oracle/", ""), f
    bench = open(os.path.join(ROOT, "bench.py")).read()
    assert bench.count("from oracle import") == 1 and "def cpu_baseline" in bench     # only inside the cpu_baseline leg


def test_record_layouts(capi):
    assert T.PER_FRAME_CONSTANTS.itemsize == 188 and T.MATERIAL_PARAMS.itemsize == 64 and T.VERTEX.itemsize == 24
    assert T.PER_FRAME_CONSTANTS.fields["options"][1] == 144 and T.DEBUG_OPTIONS.fields["environmentStrength"][1] == 36
    import ctypes
    assert ctypes.sizeof(capi.Stats) == 5 * 8 + 8 * 4 + 8 + 8       # (+ rays_shadow_skipped, appended in round 2)


def test_camera_basis_matches_oracle_and_definition(capi, oracle):
    for cam, aspect in ((scenes.cornell_camera(), 1.0), (scenes.sponza_camera(), 1920 / 1080),
                        (dict(eye=(8, 10, 30), at=(0, 1.5, 0), up=(0, 1, 0), fov=float(np.float32(np.pi / 4))), 1920 / 1080)):
        f, u = capi.camera_look(cam["eye"], cam["at"], cam["up"])
        of, ou = oracle.camera_look(cam["eye"], cam["at"], cam["up"])
        assert np.array_equal(f, of) and np.array_equal(u, ou)
        U, V, W = capi.camera_basis(f, u, cam["fov"], aspect)
        oU, oV, oW = oracle.camera_basis(f, u, cam["fov"], aspect)
        assert np.array_equal(U, oU) and np.array_equal(V, oV) and np.array_equal(W, oW)
        # calculateCameraVariables: |V| = |W| tan(fov/2), |U| = |V| aspect, mutually orthogonal, .w = 0
        assert abs(np.linalg.norm(V[:3]) - np.tan(0.5 * cam["fov"])) < 1e-6
        assert abs(np.linalg.norm(U[:3]) - np.linalg.norm(V[:3]) * aspect) < 1e-6
        assert abs(U[:3] @ V[:3]) < 1e-6 and abs(U[:3] @ W[:3]) < 1e-6 and U[3] == V[3] == W[3] == 0


def test_progressive_update_matches_oracle_and_fixture(capi, oracle):
    g = np.load(os.path.join(GOLDEN, "host_update_golden.npz"))
    host = capi.ProgressiveHost(int(g["seed"]))
    oh = oracle.Progressive(int(g["seed"]))
    acc = []
    for i, cam in enumerate(g["cams"]):
        pfc = host.update(cam, 0.5 * i, 10 + i, 1920, 1080)
        want = oh.update(cam, 0.5 * i, 10 + i, 1920, 1080)
        assert pfc.tobytes() == want.tobytes() == g["pfc"][i].tobytes()
        acc.append(int(pfc["cameraParams"]["accumCount"]))
        assert int(pfc["cameraParams"]["frameCount"]) == 10 + i
    assert acc == [0, 1, 2, 0, 1, 0]                 # restarts whenever the camera changed (.cpp:183-186)
    p0 = np.frombuffer(g["pfc"][0].tobytes(), T.PER_FRAME_CONSTANTS)[0]
    # paused animation: t = 142 s -> rotY(sin(28.4) * 3.14 / 2) of (0.3, -0.2, -1) (.cpp:179-181,197-201)
    a = np.sin(np.float32(142.0) * np.float32(0.2)) * 3.14 * 0.5
    want = np.array([0.3 * np.cos(a) - np.sin(a), -0.2, -0.3 * np.sin(a) - np.cos(a)])
    assert np.allclose(p0["directionalLight"]["forwardDir"][:3], want, atol=1e-6)
    assert p0["options"]["maxIterations"] == 1024 and p0["options"]["cosineHemisphereSampling"] == 1
    assert abs(p0["cameraParams"]["jitters"][0]) <= 0.5 / 1920 and abs(p0["cameraParams"]["jitters"][1]) <= 0.5 / 1080
    assert p0["pointLight"]["color"].tolist() == pytest.approx([0.2, 0.8, 0.6, 2.0])


def test_jitter_stream_is_mt19937(capi, oracle):
    """ProgressiveRaytracingPipeline.cpp:190-192 draws the two jitters from a std::mt19937 through a uniform_real_distribution<float>.
    The generator is pinned by the C++ standard (the 10000th output of a default-seeded engine is 4123659995) and checked here against an
    independent implementation -- numpy's MT19937 with the classic init_genrand seeding --; the mapping to [0, 1) is implementation
    defined (MSVC and libstdc++ differ) and is this engine's own: the top 24 bits times 2^-24."""
    bg = np.random.MT19937()
    bg._legacy_seeding(5489)
    raw = bg.random_raw(10000)
    assert int(raw[-1]) == 4123659995                                  # [rand.predef]: the standard's own known answer
    seed = 20240
    bg._legacy_seeding(seed)
    host, oh = capi.ProgressiveHost(seed), oracle.Progressive(seed)
    cam = cam_array(scenes.cornell_camera(), 16 / 9)
    for f in range(64):
        u = [np.float32(int(bg.random_raw()) >> 8) * np.float32(1.0 / 16777216.0) for _ in range(2)]
        want = [(u[0] - np.float32(0.5)) / np.float32(1920), (u[1] - np.float32(0.5)) / np.float32(1080)]
        for pfc in (host.update(cam, 0.0, f + 1, 1920, 1080), np.frombuffer(oh.update(cam, 0.0, f + 1, 1920, 1080).tobytes(), T.PER_FRAME_CONSTANTS)[0]):
            assert pfc["cameraParams"]["jitters"].tolist() == [float(want[0]), float(want[1])], f


def test_progressive_flags_and_reset(capi):
    host = capi.ProgressiveHost(5)
    cam = cam_array(scenes.cornell_camera(), 1.0)
    a = [int(host.update(cam, 0.0, i, 64, 64)["cameraParams"]["accumCount"]) for i in range(3)]
    host.reset()
    b = int(host.update(cam, 0.0, 3, 64, 64)["cameraParams"]["accumCount"])
    host.set_flags(accumulation_enabled=False)
    c = [int(host.update(cam, 0.0, i, 64, 64)["cameraParams"]["accumCount"]) for i in range(2)]
    assert a == [0, 1, 2] and b == 0 and c == [0, 0]
    host.set_flags(animation_paused=False)
    d0 = host.update(cam, 1.0, 1, 64, 64)["directionalLight"]["forwardDir"].copy()
    d1 = host.update(cam, 2.0, 1, 64, 64)["directionalLight"]["forwardDir"].copy()
    assert not np.array_equal(d0, d1)


def test_host_state_round_trip(capi):
    """The host half of an accumulation checkpoint: accumCount, last camera, options, flags and the RNG stream."""
    cam = cam_array(scenes.cornell_camera(), 1.0)
    a = capi.ProgressiveHost(77)
    a.options["noIndirectDiffuse"] = 1
    for f in range(5):
        a.update(cam, 0.0, f + 1, 64, 48)
    blob = a.save_state()
    b = capi.ProgressiveHost(1)          # different seed, default options: everything must come from the blob
    b.load_state(blob)
    for f in range(5, 9):
        pa, pb = a.update(cam, 0.0, f + 1, 64, 48), b.update(cam, 0.0, f + 1, 64, 48)
        assert pa.tobytes() == pb.tobytes()
        assert int(pb["cameraParams"]["accumCount"]) == f and int(pb["options"]["noIndirectDiffuse"]) == 1
    with pytest.raises(capi.RtError):
        b.load_state(blob[:-3])
    with pytest.raises(capi.RtError):
        b.load_state(b"\0" * len(blob))


def test_image_writers(capi, tmp_path):
    """PFM and EXR are lossless; the PNG decodes (zlib stream, CRCs) to the display transform of the image."""
    import struct
    import zlib
    r = np.random.default_rng(8)
    img = r.uniform(-0.2, 3.0, (37, 53, 4)).astype(np.float32)
    img[0, 0, 0] = np.nan
    pfm, png = str(tmp_path / "a.pfm"), str(tmp_path / "a.png")
    capi.write_pfm(pfm, img)
    raw = open(pfm, "rb").read()
    head = b"PF\n53 37\n-1.0\n"
    assert raw.startswith(head)
    back = np.frombuffer(raw[len(head):], "<f4").reshape(37, 53, 3)[::-1]
    assert np.array_equal(back, img[..., :3], equal_nan=True)
    capi.write_png(png, img, exposure=1.5, gamma=2.2, tonemap=True)
    raw = open(png, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(raw):
        n, typ = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(typ + body)
        chunks.setdefault(typ, b"")
        chunks[typ] += body
        pos += 12 + n
    assert struct.unpack(">IIBBBBB", chunks[b"IHDR"]) == (53, 37, 8, 2, 0, 0, 0) and b"IEND" in chunks
    px = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(37, 53 * 3 + 1)
    assert (px[:, 0] == 0).all()
    v = np.nan_to_num(img[..., :3].astype(np.float64) * 1.5, nan=0.0).clip(0, None)
    want = (v / (1 + v)) ** (1 / 2.2) * 255
    got = px[:, 1:].reshape(37, 53, 3).astype(np.float64)
    assert np.abs(got - want).max() <= 0.51
    with pytest.raises(capi.RtError):
        capi.write_png(str(tmp_path / "no" / "dir.png"), img)
    # OpenEXR: parsed here from the published file layout (magic, version, attribute list, offset table, one scan line per
    # chunk, channels in alphabetical order) -- lossless, alpha included
    exr = str(tmp_path / "a.exr")
    capi.write_exr(exr, img)
    raw = open(exr, "rb").read()
    assert struct.unpack("<I", raw[:4])[0] == 20000630 and raw[4:8] == b"\x02\x00\x00\x00"
    pos, attrs = 8, {}
    while raw[pos] != 0:
        e = raw.index(b"\0", pos); name = raw[pos:e].decode(); pos = e + 1
        e = raw.index(b"\0", pos); typ = raw[pos:e].decode(); pos = e + 1
        n = struct.unpack("<i", raw[pos:pos + 4])[0]
        attrs[name] = (typ, raw[pos + 4:pos + 4 + n]); pos += 4 + n
    pos += 1
    assert attrs["compression"] == ("compression", b"\0") and attrs["lineOrder"] == ("lineOrder", b"\0")
    assert struct.unpack("<4i", attrs["dataWindow"][1]) == (0, 0, 52, 36) and attrs["dataWindow"] == attrs["displayWindow"]
    ch, names = attrs["channels"][1], []
    q = 0
    while ch[q] != 0:
        e = ch.index(b"\0", q); names.append(ch[q:e].decode())
        assert struct.unpack("<i4Bii", ch[e + 1:e + 17]) == (2, 0, 0, 0, 0, 1, 1)         # FLOAT, not perceptually linear, sampling 1 x 1
        q = e + 17
    assert names == ["A", "B", "G", "R"] and q + 1 == len(ch)
    offsets = struct.unpack("<37Q", raw[pos:pos + 37 * 8])
    back = np.empty((37, 53, 4), np.float32)
    for y, off in enumerate(offsets):
        yy, nbytes = struct.unpack("<ii", raw[off:off + 8])
        assert yy == y and nbytes == 53 * 16
        line = np.frombuffer(raw[off + 8:off + 8 + nbytes], "<f4").reshape(4, 53)
        back[y] = line[::-1].T                       # file order A B G R -> R G B A
    assert offsets[-1] + 8 + 53 * 16 == len(raw)
    assert np.array_equal(back, img, equal_nan=True)


def test_scene_generators_are_deterministic():
    v1, t1 = scenes.sponza_class(detail=0.25)
    v2, t2 = scenes.sponza_class(detail=0.25)
    assert np.array_equal(v1, v2) and np.array_equal(t1, t2)
    assert t1.max() < v1.shape[0]
    x = scenes.instance_grid(4)
    assert x.shape == (16, 12) and np.isfinite(x).all()
    f = scenes.sky_cubemap(8)
    assert f.shape == (6, 8, 8, 4) and (f[..., :3] >= 0).all()


GLOO_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from dxrexperiments_amd import distributed as D, rtypes as T
from oracle import pyoracle as O          # stand-in renderer for the CPU test (test infrastructure)
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "cornell64_golden.npz"))
v, i = O.obj_load(os.path.join(sys.argv[1], "tests", "golden", "cornell.obj"))
sc = O.Scene(); sc.add_instance(sc.add_model(v, i)); sc.build()
N = 4
mine = D.shard_frames(rank, world, N)
acc = np.zeros((64, 64, 4), np.float32)
for f in mine:
    sc.render(T.default_material(), g["pfc"][f], 64, 64, accum=acc, env_constant=(0.5, 0.5, 0.5), accum_mode=T.ACCUM_SUM)
mean, total = D.reduce_accumulation(torch.from_numpy(acc), len(mine))
assert total == N, total
err = float(np.abs(mean.numpy() - g["images"][N - 1]).max())
rms = float(np.sqrt(np.mean((mean.numpy().astype(np.float64) - g["images"][N - 1]) ** 2)))
assert rms <= 1e-5 and err <= 1e-5, (rms, err)
rows = D.tile_rows(rank, world, 64, band=16)
own = torch.zeros(64, dtype=torch.int32)
for y0, y1 in rows: own[y0:y1] += 1
dist.all_reduce(own)
assert bool((own == 1).all())             # tile partition covers every row exactly once
# partitioning B end to end: every rank renders only its bands into a zero buffer, combine_tiles gathers them
tiled = np.zeros((64, 64, 4), np.float32)
for y0, y1 in rows:
    sc.render(T.default_material(), g["pfc"][0], 64, 64, accum=tiled, env_constant=(0.5, 0.5, 0.5), tile=(0, y0, 64, y1))
whole = D.combine_tiles(torch.from_numpy(tiled.copy())).numpy()
assert np.array_equal(whole, g["images"][0]), "tiled frame differs from the golden frame"
# the same with ONE all-gather of the disjoint bands (half the bytes; rt_dist_gather_bands' scheme); foreign rows hold junk
junk = tiled.copy()
for r in range(world):
    if r != rank:
        for y0, y1 in D.tile_rows(r, world, 64, band=16): junk[y0:y1] = -7.0
whole = D.gather_tiles(torch.from_numpy(junk), band=16).numpy()
assert np.array_equal(whole, g["images"][0]), "gathered frame differs from the golden frame"
# ragged: 64 rows in bands of 24 -> bands of 24, 24, 16 rows; rank 1 owns one band, rank 0 two (one slot is padding)
rag = np.full((64, 64, 4), float(rank + 1), np.float32)
out = D.gather_tiles(torch.from_numpy(rag), band=24).numpy()
want = np.zeros(64, np.float32)
for r in range(world):
    for y0, y1 in D.tile_rows(r, world, 64, band=24): want[y0:y1] = r + 1
assert np.array_equal(out[:, 0, 0], want)
dist.barrier(); dist.destroy_process_group()
open(os.path.join(sys.argv[2], "ok_%d" % rank), "w").write("%s %g" % (mine, rms))
'''


@pytest.mark.parametrize("world", (2, 8))
def test_sample_sharding_over_gloo(tmp_path, oracle, world):
    """N>1 path on CPU: the processes shard the frames, one all-reduce(sum), mean == single-process result; tiles through an all-reduce and an
    all-gather.  world 8: four frames and four bands over eight ranks -- half the ranks hold nothing, and must still take part."""
    script = tmp_path / "worker.py"
    script.write_text(GLOO_WORKER)
    port = 29600 + (os.getpid() + 7 * world) % 300
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % world, "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script), ROOT, str(tmp_path)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert all((tmp_path / ("ok_%d" % k)).exists() for k in range(world)), r.stdout[-2000:]


STRONG_WORKER = r'''
import importlib.util, os, sys
import numpy as np, torch, torch.distributed as dist
root = sys.argv[1]
sys.path.insert(0, root)
from dxrexperiments_amd import distributed as D
spec = importlib.util.spec_from_file_location("bench_module", os.path.join(root, "bench.py"))
bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
def frame(f):          # a stand-in for frame f of the global sequence: every rank can make any frame, renders only its own
    return np.random.default_rng(1000 + f).random((24, 32, 4), dtype=np.float32)
for T_all, batch in ((256, 32), (7, 32), (1, 32), (61, 8)):
    mine, sets, per_set = bench.fixed_total_plan(rank, world, T_all, batch)
    assert mine == D.shard_frames(rank, world, T_all) and len(mine) == D.frames_per_rank(world, T_all)[rank]
    assert per_set <= min(batch, 32) and sets * per_set >= len(mine) and (sets == 0 or (sets - 1) * per_set < len(mine))
    acc = np.zeros((24, 32, 4), np.float32)
    for f in mine:                           # RT_ACCUM_SUM: the rank's frames added in its own order
        acc = acc + frame(f)
    mean, total = D.reduce_accumulation(torch.from_numpy(acc), len(mine))      # ONE all-reduce (+ the frame count)
    assert total == T_all
    run = np.zeros((24, 32, 4), np.float32)  # the single-GPU running mean of ALL frames in order (ProgressiveRaytracing.hlsl:36-38)
    for f in range(T_all):
        run = (np.float32(f) * run + frame(f)) / np.float32(f + 1)
    rms = float(np.sqrt(np.mean((mean.numpy().astype(np.float64) - run) ** 2)))
    assert rms <= 1e-5, (T_all, rms)
# configs[4]'s tile partition at the height bench.py runs it for: 1080 rows in bands of 16 = 67 full bands + one of 8 rows, dealt round-robin
# (world 8: ranks 0 - 3 own nine bands, 4 - 7 eight; the last band is short) -- every rank fills its own rows, ONE all-gather delivers the frame
H, Wd = 1080, 8
rows = D.tile_rows(rank, world, H, band=16)
assert sum(b - a for a, b in rows) == sum(min(16, H - 16 * b) for b in range(rank, 68, world))
img = np.full((H, Wd, 4), -7.0, np.float32)          # foreign rows hold junk
for y0, y1 in rows:
    img[y0:y1] = (np.arange(y0, y1, dtype=np.float32)[:, None, None] * 8.0 + np.arange(Wd, dtype=np.float32)[None, :, None]) + np.arange(4, dtype=np.float32) * 0.25
whole = D.gather_tiles(torch.from_numpy(img), band=16).numpy()
want = (np.arange(H, dtype=np.float32)[:, None, None] * 8.0 + np.arange(Wd, dtype=np.float32)[None, :, None]) + np.arange(4, dtype=np.float32) * 0.25
assert np.array_equal(whole, want), "gathered 1080-row frame differs"
dist.barrier(); dist.destroy_process_group()
open(os.path.join(sys.argv[2], "strong_ok_%d" % rank), "w").write("ok")
'''


@pytest.mark.parametrize("world", (2, 8))
def test_fixed_total_strong_scaling_and_tiles_over_gloo(tmp_path, world):
    """bench.py --total-frames (BASELINE configs[2] as written: 256 frames IN ALL over the ranks, one all-reduce): the host logic of the
    pass -- shards, sets of launches, SUM + all-reduce + mean -- on CPU processes over gloo, ragged totals included; and configs[4]'s tile
    partition at 1080 rows (68 bands of 16, the last one short) through one all-gather.  world 8 is the node the driver measures on
    (no 8-GPU curve exists yet -- this is the plan's day-one safety, not a measurement)."""
    script = tmp_path / "strong_worker.py"
    script.write_text(STRONG_WORKER)
    port = 29300 + (os.getpid() + 7 * world) % 300
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % world, "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script), ROOT, str(tmp_path)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert all((tmp_path / ("strong_ok_%d" % k)).exists() for k in range(world)), r.stdout[-2000:]


def test_shard_helpers(capi):
    """The partitions are host logic of the C ABI (rt_shard_frame_count, rt_tile_bands, rt_tile_gather_layout)."""
    from dxrexperiments_amd import distributed as D
    for world in (1, 2, 3, 8):
        fr = [D.shard_frames(r, world, 21) for r in range(world)]
        assert sorted(sum(fr, [])) == list(range(21))
        assert [len(x) for x in fr] == D.frames_per_rank(world, 21)
        rows = sum((D.tile_rows(r, world, 1080) for r in range(world)), [])
        assert sum(b - a for a, b in rows) == 1080
        assert sorted(rows) == [(y, min(y + 16, 1080)) for y in range(0, 1080, 16)]          # bands of 16 rows, each owned once
        slots, floats = capi.tile_gather_layout(1920, 1080, 16, world)
        assert slots == -(-68 // world) and floats == slots * 16 * 1920 * 4
        assert all(len(D.tile_rows(r, world, 1080)) <= slots for r in range(world))
    with pytest.raises(capi.RtError):
        capi.tile_bands(1080, 0, 0, 1)
    with pytest.raises(capi.RtError):
        capi.shard_frame_count(3, 2, 10)


def test_bench_obj_workload(capi):
    """bench.py --obj PATH [--camera ...]: the headline line from a user mesh (north_star says "Sponza OBJ"; whoever holds the
    real file gets the same JSON line from it).  Without a GPU: the argument parsing, the product's own OBJ reader on the
    committed susanne.obj, the workload description the line will carry, and the default / explicit camera."""
    import importlib.util
    import os
    from dxrexperiments_amd import scenes
    from util import GOLDEN
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    obj = os.path.join(GOLDEN, "susanne.obj")
    args = bench.parse(["--obj", obj])
    v, t, workload, cam = bench.headline_workload(args, capi, scenes, np)
    assert t.shape == (968, 3) and "susanne.obj" in workload and "968 triangles" in workload
    lo, hi = v["position"].min(axis=0), v["position"].max(axis=0)
    assert np.allclose(cam["at"], 0.5 * (lo + hi)) and np.linalg.norm(np.array(cam["eye"]) - np.array(cam["at"])) > 0.5 * np.linalg.norm(hi - lo)
    args = bench.parse(["--obj", obj, "--camera", "1", "2", "3", "0", "0.5", "0", "--fov", "0.9", "--batch", "4"])
    _, _, _, cam = bench.headline_workload(args, capi, scenes, np)
    assert cam["eye"] == (1.0, 2.0, 3.0) and cam["at"] == (0.0, 0.5, 0.0) and cam["fov"] == 0.9 and args.batch == 4
    args = bench.parse([])
    v, t, workload, cam = bench.headline_workload(args, capi, scenes, np)
    assert "BASELINE configs[1]" in workload and t.shape[0] == 261936 and cam == scenes.sponza_camera()


def test_bench_frame_sets():
    """bench.py splits its K timed frames evenly over ceil(K / --batch) sets of launches (at most 32 frames each)"""
    import re
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert re.search(r'"--batch", type=int, default=32', src)
    def split(K, batch):
        n_sets = (K + max(1, min(batch, 32)) - 1) // max(1, min(batch, 32))
        return n_sets, (K + n_sets - 1) // n_sets
    assert split(20, 32) == (1, 20) and split(60, 32) == (2, 30) and split(20, 16) == (2, 10) and split(5, 32) == (1, 5) and split(20, 1) == (20, 1) and split(128, 99) == (4, 32)
    # ... and that is the expression bench.py uses
    assert "n_sets = (K + max(1, min(args.batch, 32)) - 1) // max(1, min(args.batch, 32))" in src and "S = (K + n_sets - 1) // n_sets" in src


def test_bench_options_and_output_dump(tmp_path):
    """bench.py --full is off by default; --dump-outputs DIR writes the accumulated image as DIR/output.npy, float32 -- whole up to
    64 MB, above that a fixed sample of its pixels that stays within 64 MB and is the same for every run"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", str(tmp_path)])
    assert a.full and a.dump_outputs == str(tmp_path)
    img = np.random.default_rng(5).random((1080, 1920, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "small"), img)
    got = np.load(tmp_path / "small" / "output.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)
    big = np.random.default_rng(6).random((2160, 3840, 4)).astype(np.float32)      # 133 MB
    for d in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / d), big)
    s1, s2 = np.load(tmp_path / "big1" / "output.npy"), np.load(tmp_path / "big2" / "output.npy")
    assert os.path.getsize(tmp_path / "big1" / "output.npy") <= 64 << 20
    assert s1.dtype == np.float32 and s1.shape[1] == 4 and s1.shape[0] > 3_000_000 and np.array_equal(s1, s2)
    assert np.isin(s1[:1000, 0], big[..., 0]).all()
