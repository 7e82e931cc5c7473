"""CPU-only side of rigid animation (rt_scene_set_instance_transform(s), rt_scene_update, rt_scene_update_ms): the exports, their binding and
their citations; and the instance transform's arithmetic, the device's own text kept host-compilable (dxrexperiments_amd/csrc/rt_xform.h),
as a stand-alone CPU program under AddressSanitizer + UndefinedBehaviorSanitizer: the hard families' matrices through invert3x4 give the
oracle's inverses bit for bit, without a report.  (The GPU side: tests/test_gpu_scene_update.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from dxrexperiments_amd import rtypes as T
from util import HARD_FAMILIES, hard_xforms, random_xforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dxrexperiments_amd", "csrc")
NEW = ("rt_scene_set_instance_transform", "rt_scene_set_instance_transforms", "rt_scene_update", "rt_scene_update_ms")


def test_exports_and_their_argument_types(capi):
    u32, p = C.c_uint32, C.c_void_p
    want = {"rt_scene_set_instance_transform": [p, u32, p], "rt_scene_set_instance_transforms": [p, u32, u32, p], "rt_scene_update": [p],
            "rt_scene_update_ms": [p, C.POINTER(C.c_float)]}
    lib = capi.lib()
    for name in NEW:
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and args == want[name], name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(NEW) <= exported, set(NEW) - exported
    for method in ("set_transform", "set_transforms", "update", "update_ms"):
        assert callable(getattr(capi.Scene, method))


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared under a comment that cites the instance descriptor's transform (TopLevelASGenerator.cpp:344-362) or the
    generators' updateOnly, and says that the reference's RtScene does not expose it; the C++ mirror says the same"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in NEW:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        comments = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)
        near = " ".join(comments[-2:])
        assert "EXTENSION" in near, name
        assert "TopLevelASGenerator.cpp:344-362" in near or "updateOnly" in near or "rt_scene_build_ms" in near, name
    block = text[text.index("Rigid animation"):text.index("int rt_scene_update_ms")]
    assert "TopLevelASGenerator.cpp:344-362" in block and "updateOnly" in block and "BottomLevelASGenerator.h:136-176" in block
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    assert re.search(r"void setTransform\(uint32_t \w+, const Matrix &\w+\)", mirror) and re.search(r"void update\(RtContext::SharedPtr \w+\)", mirror)
    assert "EXTENSIONS" in mirror[:mirror.index("void setTransform")]


def test_setters_refuse_null_handles(capi):
    """argument checks need no device"""
    x = np.zeros(12, np.float32)
    assert capi.lib().rt_scene_set_instance_transform(None, 0, x.ctypes.data_as(C.c_void_p)) != 0
    assert capi.lib().rt_scene_set_instance_transforms(None, 0, 1, x.ctypes.data_as(C.c_void_p)) != 0
    assert capi.lib().rt_scene_update(None) != 0
    assert capi.lib().rt_scene_update_ms(None, None) != 0


def reference_inverse(m):
    """the definition in numpy fp32 (DESIGN.md "Instances"): adjugate / determinant, operation order fixed"""
    f = np.float32
    a, b, c, tx, d, e, ff, ty, g, h, i, tz = [f(v) for v in m]
    with np.errstate(all="ignore"):
        A = e * i - ff * h; B = ff * g - d * i; Cc = d * h - e * g
        det = a * A; det = det + b * B; det = det + c * Cc
        inv = f(1.0) / det
        o = np.zeros(12, np.float32)
        o[0] = A * inv; o[1] = (c * h - b * i) * inv; o[2] = (b * ff - c * e) * inv
        o[4] = B * inv; o[5] = (a * i - c * g) * inv; o[6] = (c * d - a * ff) * inv
        o[8] = Cc * inv; o[9] = (b * g - a * h) * inv; o[10] = (a * e - b * d) * inv
        for r in range(3):
            s = o[4 * r] * tx; s = s + o[4 * r + 1] * ty; s = s + o[4 * r + 2] * tz
            o[4 * r + 3] = -s
    return o


def test_shared_inverse_text_under_asan_ubsan(oracle, tmp_path):
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "invert3x4_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "invert3x4_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    neg_zero = ident.copy(); neg_zero[1] = -0.0
    mats = np.concatenate([hard_xforms(fam, 12, seed=13) for fam in HARD_FAMILIES + ("extreme", "degenerate")] + [random_xforms(12, 3), ident[None], neg_zero[None]])
    (tmp_path / "in.bin").write_bytes(mats.astype(np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "0 sanitizer reports" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.float32).reshape(-1, 13)
    assert got.shape[0] == mats.shape[0]
    assert got[:, 12].tolist() == [0.0] * (len(mats) - 2) + [1.0, 1.0]         # (-0 compares equal to 0: still the identity)
    # the oracle's inverses of the same matrices (its scene build; identity instances keep their matrix as it is)
    tri_v = np.zeros(3, T.VERTEX)
    tri_v["position"] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    osc = oracle.Scene()
    osc.add_model(tri_v, np.array([[0, 1, 2]], np.uint32))
    for m in mats[:-2]:
        osc.add_instance(0, m)
    osc.build()
    for k, m in enumerate(mats[:-2]):
        want = reference_inverse(m)
        assert got[k, :12].tobytes() == want.tobytes() or np.array_equal(got[k, :12], want, equal_nan=True), (k, got[k, :12], want)
        assert np.array_equal(got[k, :12], osc.instance_info(k)[1], equal_nan=True), (k, got[k, :12], osc.instance_info(k)[1])
