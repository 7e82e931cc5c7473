"""CPU-only side of skeletal animation (rt_model_set_skin, rt_model_get_skin, rt_model_set_bones): the exports, their binding, their
citations, the header's statement of the definition, the C++ mirror and the example; and the host side of a skin -- validation and the
slot-major 16-bit packing, a header of its own (dxrexperiments_amd/csrc/rt_skin.h) -- as a stand-alone CPU program under AddressSanitizer +
UndefinedBehaviorSanitizer against a numpy packing.  (The GPU side: tests/test_gpu_model_skin.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import skin_cases as K

ROOT = K.ROOT
NEW = ("rt_model_set_skin", "rt_model_get_skin", "rt_model_set_bones")


def test_exports_and_their_argument_types(capi):
    u32, p, pu = C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)
    want = {"rt_model_set_skin": [p, u32, u32, p, p], "rt_model_get_skin": [p, pu, pu], "rt_model_set_bones": [p, p, u32]}
    lib = capi.lib()
    for name in NEW:
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and args == want[name], name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(NEW) <= exported, set(NEW) - exported
    for method in ("set_skin", "clear_skin", "skin", "set_bones", "set_bones_device"):
        assert callable(getattr(capi.Model, method))


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared under a comment marked EXTENSION that cites the import that drops the bones (RtModel.cpp:26) and the
    generators' never-taken update path (BottomLevelASGenerator.h:136-176); the header states the definition and the states; the C++ mirror
    has the methods, marked the same way; the example exists and is built"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in NEW:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near and "RtModel.cpp:26" in near and "BottomLevelASGenerator.h:136-176" in near, name
    block = text[text.index("Skeletal animation"):text.index("int rt_model_set_bones")].replace("\n * ", " ")
    for words in ("B[e] = weights[v][0] * M_bone[v][0][e]", "B[e] = B[e] + weights[v][k] * M_bone[v][k][e]", "in slot order", "a zero weight is not skipped",
                  "((B[r][0] x + B[r][1] y) + B[r][2] z) + B[r][3]", "(B[r][0] nx + B[r][1] ny) + B[r][2] nz", "0 < d < inf", "never renormalised",
                  "rest pose", "REST POSE", "never from the previous pose", "RT_ERR_STATE", "RT_ERR_INVALID_ARG", "rt_scene_update", "rt_model_recompute_normals",
                  "RT_MEM_HOST", "RT_MEM_DEVICE", "names the vertex and the slot"):
        assert words in block, words
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    model = mirror[mirror.index("class RtModel"):mirror.index("class RtScene")]
    for sig in (r"void setSkin\(const uint32_t \*boneIndices, const float \*weights, uint32_t influences, uint32_t numBones\)", r"void clearSkin\(\)",
                r"void setBones\(const float \*bones3x4, bool deviceMemory = false\)"):
        assert re.search(sig, model), sig
    above = model[model.index("void recomputeNormals"):model.index("void setSkin")]
    assert "EXTENSIONS" in above and "RtModel.cpp:26" in above and "BottomLevelASGenerator.h:136-176" in above
    example = open(os.path.join(ROOT, "examples", "realtime_skinned.cpp")).read()
    assert "setSkin(" in example and "setBones(" in example and "->update(context)" in example
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_skinned" in make.split("BIN =")[1].splitlines()[0] and "examples/realtime_skinned.cpp" in make


def test_lds_limit_is_a_named_constant():
    """RT_SKIN_LDS_BONES is defined in rt_skin.h; a palette of that many bones fits the LDS a block may take with eight blocks on a CU"""
    n = K.lds_bones()
    assert 1 <= n and 48 * n * 8 <= 160 * 1024


def test_null_handles_and_null_arrays_are_refused(capi):
    """argument checks need no device"""
    x = np.zeros(24, np.float32)
    b = np.zeros(8, np.uint32)
    lib = capi.lib()
    px, pb = x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    k, n = C.c_uint32(7), C.c_uint32(7)
    assert lib.rt_model_set_skin(None, 1, 1, pb, px) == -1
    assert b"null" in lib.rt_last_error()
    assert lib.rt_model_set_skin(None, 0, 0, None, None) == -1
    assert lib.rt_model_get_skin(None, C.byref(k), C.byref(n)) == -1
    assert lib.rt_model_set_bones(None, px, 0) == -1
    assert b"null" in lib.rt_last_error()


def skins():
    """(n_verts, influences, n_bones, bones[V, K], weights[V, K]) the stand-alone program is fed, and what it must say (0: packed)"""
    out = []
    for nv in (1, 65, 901):
        for k in (1, 8):
            for n_bones in (1, 3, 65536):
                out.append((nv, k, n_bones, K.random_bones(nv, k, n_bones, seed=nv + k), K.random_weights(nv, k, nv * k, "wild"), (0, 0, 0)))
    assert out[-1][3].max() == 65535
    nv, k = 65, 3
    bones, weights = K.random_bones(nv, k, 7, seed=5), K.random_weights(nv, k, 6)
    bad = bones.copy()
    bad[41, 2] = 7                                      # an index == n_bones ...
    bad[50, 0] = 0xFFFFFFFF                             # (... and a later one that would pass if it were cut to 16 bits and compared)
    out.append((nv, k, 7, bad, weights, (4, 41, 2)))
    top = bones.copy()
    top[64, 2] = 65536
    out.append((nv, k, 65536, top, weights, (4, 64, 2)))
    for k_bad in (0, 9):
        out.append((nv, k_bad, 7, np.zeros((nv, k_bad), np.uint32), np.zeros((nv, k_bad), np.float32), (2, 0, 0)))
    for n_bad in (0, 65537):
        out.append((nv, k, n_bad, bones, weights, (3, 0, 0)))
    return out


def test_validation_and_packing_under_asan_ubsan(tmp_path):
    """V in {1, 65, 901} x K in {1, 8} x n_bones in {1, 3, 65536 with index 65535 in use}: the program's packed arrays == the numpy packing,
    weights bit for bit; refused: an index == n_bones (vertex and slot named), K = 0 and 9, n_bones = 0 and 65537, null arrays; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "skin_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "skin_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cases = skins()
    blob = b"".join(np.array([nv, k, nb], np.uint32).tobytes() + np.ascontiguousarray(b, np.uint32).tobytes() + np.ascontiguousarray(w, np.float32).tobytes()
                    for nv, k, nb, b, w, _ in cases)
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d skins, 0 sanitizer reports" % len(cases) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    raw = (tmp_path / "out.bin").read_bytes()
    at = 0
    for nv, k, nb, b, w, want in cases:
        assert tuple(np.frombuffer(raw, np.uint32, 3, at)) == want, (nv, k, nb, want)
        at += 12
        if want[0] == 0:
            pb, pw = K.pack(b, w)
            n = nv * k
            assert np.frombuffer(raw, np.uint16, n, at).tobytes() == pb.tobytes(), (nv, k, nb)
            at += 2 * n
            assert np.frombuffer(raw, np.float32, n, at).tobytes() == pw.tobytes(), (nv, k, nb)
            at += 4 * n
    assert at == len(raw)
