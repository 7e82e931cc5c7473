"""CPU-only side of morph targets (rt_model_set_morph_targets, rt_model_get_morph_targets, rt_model_set_morph_weights): the exports, their
binding, their citations, the header's statement of the definition, the C++ mirror and the example; and the host side of the targets --
validation and the SELL-64 packing, a header of its own (dxrexperiments_amd/csrc/rt_morph.h) -- as a stand-alone CPU program under
AddressSanitizer + UndefinedBehaviorSanitizer against a numpy packing.  (The GPU side: tests/test_gpu_model_morph.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import morph_cases as M

ROOT = M.ROOT
NEW = ("rt_model_set_morph_targets", "rt_model_get_morph_targets", "rt_model_set_morph_weights")


def test_exports_and_their_argument_types(capi):
    u32, p, pu = C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)
    want = {"rt_model_set_morph_targets": [p, u32, p, p, p, p], "rt_model_get_morph_targets": [p, pu, pu, pu], "rt_model_set_morph_weights": [p, p, u32]}
    lib = capi.lib()
    for name in NEW:
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and args == want[name], name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(NEW) <= exported, set(NEW) - exported
    for method in ("set_morph_targets", "clear_morph_targets", "morph_targets", "set_morph_weights", "set_morph_weights_device"):
        assert callable(getattr(capi.Model, method))


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared under a comment marked EXTENSION that cites the import that reads only positions and normals (RtModel.cpp:26)
    and the generators' never-taken update path (BottomLevelASGenerator.h:136-176); the header states the definition, the validation and
    where the result goes; the C++ mirror has the methods, marked the same way; the example exists and is built"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in NEW:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near and "RtModel.cpp:26" in near and "BottomLevelASGenerator.h:136-176" in near, name
    assert "Morph targets -- EXTENSIONS" in text
    block = re.sub(r"\n \*\s+", " ", text[text.index("Morph targets -- EXTENSIONS"):text.index("int rt_model_set_morph_weights")])
    for words in ("RtModel.cpp:26, :38-45", "target_offsets[t] .. target_offsets[t + 1] - 1", "position_deltas[3 e ..]", "normal_deltas[3 e ..]",
                  "A dense target simply lists every vertex", "a target with no entries is legal", "fp32 throughout", "one rounded operation", "no contraction",
                  "copied bit for bit, all 24 bytes", "in ascending target order", "p_c = p_c + (w_t * dp_c)", "s_c = s_c + (w_t * dn_c)",
                  "a zero weight is not skipped", "-0 + (+0 * d) is +0", "a NaN weight reaches the vertex", "((sx sx) + sy sy) + sz sz", "0 < d < inf",
                  "rt_model_recompute_normals", "the base normal is copied bit for bit", "NaN, inf, negative weights and weights above 1 are no errors",
                  "nothing changes when it refuses", "n_targets > 65536", "stored in 16 bits", "target_offsets[0] != 0", "the message names the target",
                  "a vertex index >= V", "ascend strictly", "at most once", "names the target and the entry", "RT_ERR_UNSUPPORTED", "2^32 cells",
                  "n_targets == 0", "frees their buffers", "BASE", "the skin's rest pose", "built scenes stay built", "captures the base anew",
                  "never from the previous result", "NO SKIN", "WITH A SKIN", "CHANGED", "STALE", "names the pending vertices", "rt_scene_update",
                  "rt_model_read_geometry returns the morphed vertices", "The model's vertices are not touched", "the next rt_model_set_bones poses the morphed rest pose",
                  "rt_model_set_morph_weights, rt_model_set_bones, rt_scene_update", "recaptured by neither", "RT_MEM_HOST", "RT_MEM_DEVICE",
                  "RT_ERR_INVALID_ARG", "RT_ERR_STATE", "names rt_model_set_morph_targets", "leave the base alone"):
        assert words in block, words
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    model = mirror[mirror.index("class RtModel"):mirror.index("class RtScene")]
    for sig in (r"void setMorphTargets\(uint32_t numTargets, const uint32_t \*targetOffsets, const uint32_t \*vertexIndices, const float \*positionDeltas,\s+"
                r"const float \*normalDeltas = nullptr\)", r"void clearMorphTargets\(\)", r"void setMorphWeights\(const float \*weights, bool deviceMemory = false\)"):
        assert re.search(sig, model), sig
    above = model[model.index("void setBones"):model.index("void setMorphTargets")]
    assert "EXTENSIONS" in above and "RtModel.cpp:26" in above and "BottomLevelASGenerator.h:136-176" in above
    example = open(os.path.join(ROOT, "examples", "realtime_morph.cpp")).read()
    assert "setMorphTargets(" in example and "setMorphWeights(" in example and "->update(context)" in example and "std::sin(" in example
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_morph" in make.split("BIN =")[1].splitlines()[0] and "examples/realtime_morph.cpp" in make


def test_null_handles_are_refused(capi):
    """argument checks need no device"""
    x = np.zeros(24, np.float32)
    o = np.zeros(8, np.uint32)
    lib = capi.lib()
    px, po = x.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)
    a, b, c = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    assert lib.rt_model_set_morph_targets(None, 1, po, po, px, px) == -1
    assert b"null" in lib.rt_last_error()
    assert lib.rt_model_set_morph_targets(None, 0, None, None, None, None) == -1
    assert lib.rt_model_get_morph_targets(None, C.byref(a), C.byref(b), C.byref(c)) == -1
    assert (a.value, b.value, c.value) == (7, 7, 7)
    assert lib.rt_model_set_morph_weights(None, px, 0) == -1
    assert b"null" in lib.rt_last_error()


def test_numpy_pack_puts_entries_where_the_layout_says():
    """the restated packing against the sentence itself, entry by entry, on a small case with a width-0 slice"""
    nv = 200
    off, idx, dp, dn, _ = M.targets(M.runs("gap", nv, 5, 3), None, 4, True)
    count, slice_cell, target, pdp, pdn = M.pack(nv, off, idx, dp, dn)
    assert slice_cell[1] > 0 and slice_cell[2] == slice_cell[1] and slice_cell[3] > slice_cell[2] and len(slice_cell) == 5
    seen = np.zeros(nv, np.int64)
    used = np.zeros(len(target), bool)
    for t in range(5):
        for e in range(off[t], off[t + 1]):
            v = int(idx[e])
            cell = int(slice_cell[v >> 6]) + 64 * int(seen[v]) + (v & 63)
            seen[v] += 1
            used[cell] = True
            assert target[cell] == t and pdp[3 * cell:3 * cell + 3].tobytes() == dp[e].tobytes() and pdn[3 * cell:3 * cell + 3].tobytes() == dn[e].tobytes()
    assert np.array_equal(seen, count)
    assert not target[~used].any() and not pdp.view(np.uint32).reshape(-1, 3)[~used].any() and not pdn.view(np.uint32).reshape(-1, 3)[~used].any()


def target_sets():
    """(n_verts, offsets, indices, dpos, dnrm or None, what the stand-alone program must say (0, 0, 0: packed))"""
    out = []
    seed = 0
    for nv in (1, 63, 64, 65, 130, 257, 901):            # V not a multiple of 64 among them
        for shape in M.SHAPES:                          # gap: a slice of width 0 between two others (from 130 on); spike: one vertex named
            for nt in (1, 3, 70):                       # by every target next to vertices named by none; sparse: an empty target
                seed += 1
                off, idx, dp, dn, _ = M.targets(M.runs(shape, nv, nt, seed), None, seed, normals=seed % 2 == 0)
                out.append((nv, off, idx, dp, dn, (0, 0, 0)))
    off, idx, dp, dn, active = M.targets(M.runs("sparse", 901, 3, 5)[:1] + M.runs("sparse", 901, 3, 6)[:1] + M.runs("spike", 901, 1, 7), M.MAX_TARGETS, 8)
    assert active == [0, 1, 65535] and len(off) == 65537 and off[1] > 0 and off[2] > off[1] and off[65535] == off[2] and off[65536] == off[2] + 1
    out.append((901, off, idx, dp, dn, (0, 0, 0)))
    out.append((901, np.append(off, off[-1]), idx, dp, dn, (2, 0, 0)))                    # 65537 targets
    nv = 130
    off, idx, dp, dn, _ = M.targets(M.runs("dense", nv, 4, 9), None, 9)
    out.append((nv, off + np.uint32(1), idx, dp, dn, (3, 0, 0)))                          # offsets[0] != 0
    bad = off.copy()
    bad[3] = bad[2] - 1                                                                   # target 2's offsets decrease
    out.append((nv, bad, idx, dp, dn, (4, 2, 0)))
    bad = idx.copy()
    bad[2 * nv + 129] = nv                                                                # an index == V ...
    bad[3 * nv + 7] = 0xFFFFFFFF                                                          # (... and a later, larger one)
    out.append((nv, off, bad, dp, dn, (5, 2, 2 * nv + 129)))
    bad = idx.copy()
    bad[nv + 41] = bad[nv + 40]                                                           # a vertex twice in target 1
    out.append((nv, off, bad, dp, dn, (6, 1, nv + 41)))
    bad = idx.copy()
    bad[3 * nv + 10], bad[3 * nv + 11] = idx[3 * nv + 11], idx[3 * nv + 10]               # descending in target 3
    out.append((nv, off, bad, dp, dn, (6, 3, 3 * nv + 11)))
    return out


def test_validation_and_packing_under_asan_ubsan(tmp_path):
    """V in {1, 63, 64, 65, 130, 257, 901} x every run shape x 1, 3, 70 targets, with and without normal deltas, and 65536 targets with
    entries only in targets 0, 1 and 65535: the program's packed arrays == the numpy packing, deltas bit for bit; refused, with the target
    and the entry named: 65537 targets, offsets[0] != 0, decreasing offsets, an index == V, a vertex twice, descending indices, null arrays;
    and (from arrays the program makes itself) a layout of exactly 2^32 cells; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "morph_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "morph_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cases = target_sets()
    blob = b"".join(np.array([nv, len(off) - 1, len(idx), dn is not None], np.uint32).tobytes() + np.ascontiguousarray(off, np.uint32).tobytes() +
                    np.ascontiguousarray(idx, np.uint32).tobytes() + np.ascontiguousarray(dp, np.float32).tobytes() +
                    (b"" if dn is None else np.ascontiguousarray(dn, np.float32).tobytes()) for nv, off, idx, dp, dn, _ in cases)
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d target sets, 0 sanitizer reports" % len(cases) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.returncode, r.stderr[-3000:])
    raw = (tmp_path / "out.bin").read_bytes()
    at = 0
    for n, (nv, off, idx, dp, dn, want) in enumerate(cases):
        assert tuple(np.frombuffer(raw, np.uint32, 3, at)) == want, (n, nv, want)
        at += 12
        if want[0] == 0:
            for name, a in zip(("count", "slice_cell", "target", "dpos", "dnrm"), M.pack(nv, off, idx, dp, dn)):
                if a is None:
                    continue
                assert raw[at:at + a.nbytes] == a.tobytes(), (n, nv, name)
                at += a.nbytes
    assert at == len(raw)
