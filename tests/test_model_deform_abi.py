"""CPU-only side of deforming meshes (rt_model_set_vertices, rt_model_set_positions, rt_model_recompute_normals): the exports, their
binding, their citations and the C++ mirror; and the vertex -> triangle CSR that recompute_normals sums over, which is host code in a header
of its own (dxrexperiments_amd/csrc/rt_adjacency.h), as a stand-alone CPU program under AddressSanitizer + UndefinedBehaviorSanitizer against
a numpy CSR.  (The GPU side: tests/test_gpu_model_deform.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from deform_cases import csr_of, index_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_model_set_vertices", "rt_model_set_positions", "rt_model_recompute_normals")


def test_exports_and_their_argument_types(capi):
    u32, p = C.c_uint32, C.c_void_p
    want = {"rt_model_set_vertices": [p, u32, u32, p, u32], "rt_model_set_positions": [p, u32, u32, p, u32], "rt_model_recompute_normals": [p]}
    lib = capi.lib()
    for name in NEW:
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and args == want[name], name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(NEW) <= exported, set(NEW) - exported
    for method in ("set_vertices", "set_positions", "set_vertices_device", "set_positions_device", "recompute_normals"):
        assert callable(getattr(capi.Model, method))


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared under a comment marked EXTENSION that cites the generators' allowUpdate / updateOnly
    (BottomLevelASGenerator.h:136-176); the header states the definition; the C++ mirror has the methods, marked the same way"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in NEW:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near and "BottomLevelASGenerator.h:136-176" in near, name
    block = text[text.index("Deforming meshes"):text.index("int rt_model_recompute_normals")]
    for words in ("RT_MEM_HOST", "RT_MEM_DEVICE", "STALE", "RT_ERR_STATE", "rt_scene_update", "array for array", "fresh models", "ascending", "no\n * atomics"):
        assert words in block or words.replace("\n * ", " ") in block.replace("\n * ", " "), words
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    model = mirror[mirror.index("class RtModel"):mirror.index("class RtScene")]
    for sig in (r"void setVertices\(const rt_vertex \*\w+, uint32_t \w+", r"void setPositions\(const float \*\w+, uint32_t \w+", r"void recomputeNormals\(\)"):
        assert re.search(sig, model), sig
    assert "EXTENSIONS" in model[:model.index("void setVertices")] and "BottomLevelASGenerator.h:136-176" in model[:model.index("void setVertices")]
    assert os.path.exists(os.path.join(ROOT, "examples", "realtime_deform.cpp"))
    assert "$(LIBDIR)/realtime_deform" in open(os.path.join(ROOT, "Makefile")).read().split("BIN =")[1].splitlines()[0]


def test_setters_refuse_null_handles(capi):
    """argument checks need no device"""
    x = np.zeros(24, np.float32)
    lib = capi.lib()
    assert lib.rt_model_set_vertices(None, 0, 1, x.ctypes.data_as(C.c_void_p), 0) == -1
    assert lib.rt_model_set_positions(None, 0, 1, x.ctypes.data_as(C.c_void_p), 0) == -1
    assert lib.rt_model_recompute_normals(None) == -1
    assert b"null" in lib.rt_last_error()


def test_adjacency_under_asan_ubsan(tmp_path):
    """the grid (valence 1 .. 6), a soup, a vertex no triangle names, triangles naming a vertex twice and thrice, a fan, one triangle: the
    program's CSR == the numpy one; an index out of range is refused; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "adjacency_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "adjacency_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cases = list(index_lists().values()) + [(3, np.array([[0, 1, 3]], np.uint32))]      # (the last: index 3 of 3 vertices)
    blob = b"".join(np.array([nv, len(idx)], np.uint32).tobytes() + np.ascontiguousarray(idx, np.uint32).tobytes() for nv, idx in cases)
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d index lists, 0 sanitizer reports" % len(cases) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint32)
    at = 0
    for nv, idx in cases[:-1]:
        off, tris = csr_of(nv, idx)
        assert got[at] == 1
        assert np.array_equal(got[at + 1:at + 2 + nv], off), (nv, idx)
        assert np.array_equal(got[at + 2 + nv:at + 2 + nv + len(tris)], tris), (nv, idx)
        at += 2 + nv + len(tris)
    assert got[at] == 0 and at + 1 == len(got)
    # what the cases are there for
    off, _ = csr_of(*index_lists()["grid"])
    assert sorted(set(np.diff(off).tolist())) == [1, 2, 3, 6]
    assert set(np.diff(csr_of(*index_lists()["soup"])[0]).tolist()) == {1}
    assert np.diff(csr_of(*index_lists()["unnamed"])[0]).tolist() == [1, 2, 2, 0, 1, 0]
    assert np.diff(csr_of(*index_lists()["twice"])[0]).tolist() == [3, 2, 2, 1]
