"""The product's host-side code under AddressSanitizer + UndefinedBehaviorSanitizer (round 5, VERDICT r4 task 7).

rt_obj.cpp, rt_fbx.cpp (zlib, 32- / 64-bit records), rt_dds.cpp, rt_image.cpp and rt_host.cpp parse untrusted files and hostile arguments
inside the product library; they need no device, so THE SAME SOURCES are compiled here with `g++ -fsanitize=address,undefined
-fno-sanitize-recover=undefined` into tests/cpp/fuzz_parsers.cpp and driven with a 10^5-case mutation fuzz seeded from the reference's
own assets -- susanne.obj / cornell.obj (committed re-emissions + the reference's own susanne.obj), ground.fbx (committed re-emission +
the reference's file), CathedralRadiance.dds (a 32^2 down-sample written here as DDS in both header forms + the reference's 4 MB map
rebuilt from tests/golden/reference_assets) -- and from FBX files the tests' writer synthesises in every container variant.  Zero sanitizer reports, every accepted
mesh self-consistent, every short buffer refused.  (GPU AddressSanitizer is not available on this pool; this is the CPU build.)
Import behaviour kept: libs/DXRFramework/RtModel.cpp:24-82; DDS call site src/ProgressiveRaytracingPipeline.cpp:114-118."""
import os
import struct
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "dxrexperiments_amd", "csrc")
OUT = os.path.join(ROOT, "build_san")
SOURCES = ["rt_obj.cpp", "rt_fbx.cpp", "rt_dds.cpp", "rt_image.cpp", "rt_host.cpp"]
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]


def _newer(target, deps):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def fuzzer():
    os.makedirs(OUT, exist_ok=True)
    headers = [os.path.join(CSRC, "rt_internal.h"), os.path.join(ROOT, "include", "dxr_amd.h"), os.path.join(ROOT, "include", "dxr_amd_types.h")]

    def compile_one(src):
        obj = os.path.join(OUT, src.replace(".cpp", ".o"))
        if not _newer(obj, [os.path.join(CSRC, src)] + headers):
            r = subprocess.run(["g++"] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 0, r.stdout[-3000:]
        return obj

    with ThreadPoolExecutor(5) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    exe = os.path.join(OUT, "fuzz_parsers")
    drv = os.path.join(ROOT, "tests", "cpp", "fuzz_parsers.cpp")
    if not _newer(exe, objs + [drv]):
        r = subprocess.run(["g++"] + FLAGS + [drv] + objs + ["-lz", "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
    return exe


def write_dds(path, faces, half, dx10, mips=1):
    """faces float32 [6, s, s, 4] -> a DDS cube map: RGBA16F or RGBA32F, DX10 extended header or legacy FourCC, `mips` levels per face
    (lower levels by 2x2 box filter), the layout DirectXTK's loader reads (src/ProgressiveRaytracingPipeline.cpp:114-118)."""
    s = faces.shape[1]
    hdr = bytearray(128)
    hdr[0:4] = b"DDS "
    struct.pack_into("<IIIIIII", hdr, 4, 124, 0x1 | 0x2 | 0x4 | 0x1000 | (0x20000 if mips > 1 else 0), s, s, 0, 0, mips)
    struct.pack_into("<II", hdr, 76, 32, 0x4)
    hdr[84:88] = b"DX10" if dx10 else struct.pack("<I", 113 if half else 116)
    struct.pack_into("<II", hdr, 108, 0x1000 | 0x8 | (0x400000 if mips > 1 else 0), 0xfe00)
    body = bytes(hdr)
    if dx10:
        body += struct.pack("<IIIII", 10 if half else 2, 3, 0x4, 1, 0)
    for f in range(6):
        lvl = faces[f]
        for m in range(mips):
            body += (lvl.astype(np.float16) if half else lvl.astype(np.float32)).tobytes()
            if lvl.shape[0] > 1:
                lvl = 0.25 * (lvl[0::2, 0::2] + lvl[1::2, 0::2] + lvl[0::2, 1::2] + lvl[1::2, 1::2])
    open(path, "wb").write(body)


def _seeds(tmp):
    import fbx_tools as F
    seeds = [("obj", os.path.join(GOLDEN, "cornell.obj"), 30000), ("obj", os.path.join(GOLDEN, "susanne.obj"), 600),
             ("fbx", os.path.join(GOLDEN, "ground.fbx"), 10000)]
    # FBX in every container variant the reader knows: 32- / 64-bit records, raw / zlib arrays, both normal mappings, indexed normals, a Model transform
    sq = dict(positions=np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 1.5, 0.2]], np.float64), polygons=[[0, 1, 2, 3], [3, 2, 4]],
              normals=np.tile(np.array([[0.0, 0.0, 1.0]]), (7, 1)), mapping="ByPolygonVertex")
    bv = dict(sq, normals=np.tile(np.array([[0.0, 0.6, 0.8]]), (5, 1)), mapping="ByVertice", translation=(1.0, 2.0, 3.0), rotation=(10.0, 20.0, 30.0), scaling=(1.0, 2.0, 0.5))
    ix = dict(sq, normals=np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]), normals_index=[0, 0, 0, 0, 1, 1, 1])
    for k, (meshes, version, compress) in enumerate((([sq, bv], 7500, False), ([bv, ix], 7400, False), ([sq, ix, bv], 7500, True), ([ix], 7300, True))):
        p = os.path.join(tmp, "synth%d.fbx" % k)
        F.write(p, meshes, version=version, compress=compress)
        seeds.append(("fbx", p, 9000))
    faces = np.load(os.path.join(GOLDEN, "cathedral32.npz"))["faces32"].reshape(6, 32, 32, 4)
    for k, (half, dx10, mips) in enumerate(((True, True, 6), (False, False, 1), (True, False, 3))):
        p = os.path.join(tmp, "cube%d.dds" % k)
        write_dds(p, faces[:, ::2, ::2] if not half else faces, half, dx10, mips)
        seeds.append(("dds", p, 8000))
    # the reference's own files as well (the big DDS: few cases, it is 4 MB per write)
    from util import reference_asset
    seeds += [("fbx", reference_asset("ground.fbx", tmp), 4000), ("obj", reference_asset("susanne.obj", tmp), 300),
              ("dds", reference_asset("CathedralRadiance.dds", tmp), 150)]
    seeds.append(("host", "-", 12000))
    return seeds


def test_mutation_fuzz_of_the_host_side_readers_under_asan_ubsan(fuzzer, tmp_path):
    seeds = _seeds(str(tmp_path))
    assert sum(n for _, _, n in seeds) >= 100000
    scratch = "/dev/shm" if os.access("/dev/shm", os.W_OK) else str(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:allocator_may_return_null=1:max_allocation_size_mb=2048", UBSAN_OPTIONS="print_stacktrace=1")

    def run(job):
        k, (kind, path, n) = job
        tmpf = os.path.join(scratch, "dxr_fuzz_%d_%d" % (os.getpid(), k))
        try:
            r = subprocess.run([fuzzer, kind, path, str(n), str(1000 + k), tmpf], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        finally:
            if os.path.exists(tmpf):
                os.remove(tmpf)
        return kind, path, n, r

    with ThreadPoolExecutor(min(6, os.cpu_count() or 1)) as ex:
        results = list(ex.map(run, enumerate(seeds)))
    total = 0
    for kind, path, n, r in results:
        assert r.returncode == 0, "%s fuzz of %s: exit %d\n%s\n%s" % (kind, path, r.returncode, r.stdout[-500:], r.stderr[-4000:])
        assert "0 sanitizer reports" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        total += n
    assert total >= 100000


def test_dds_writer_of_this_test_is_read_back_exactly(capi, tmp_path):
    """the DDS seeds are real DDS files: the product's reader returns the texels they were written from (fp32 exact, fp16 after rounding)"""
    faces = np.load(os.path.join(GOLDEN, "cathedral32.npz"))["faces32"].reshape(6, 32, 32, 4)
    for half, dx10, mips in ((True, True, 6), (False, False, 1), (True, False, 3), (False, True, 2)):
        p = str(tmp_path / "c.dds")
        write_dds(p, faces, half, dx10, mips)
        got = capi.dds_read_cube(p)
        assert got.shape == (6, 32, 32, 4)
        want = faces.astype(np.float16).astype(np.float32) if half else faces
        assert np.array_equal(np.asarray(got).reshape(6, 32, 32, 4), want)
