"""CPU-only side of posed skeletons (rt_skeleton_*, rt_model_set_bones_from_skeleton): the exports, their binding, their citations, the
header's statement of the definition, the C++ mirror and the example; the host side of a skeleton -- validation, the level table, the segment
search, a header of its own (dxrexperiments_amd/csrc/rt_skeleton.h) -- as a stand-alone CPU program under AddressSanitizer +
UndefinedBehaviorSanitizer against numpy; and the numpy restatement itself (tests/skeleton_cases.py) against the geometry it states.  (The GPU
side: tests/test_gpu_skeleton.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import skeleton_cases as S

ROOT = S.ROOT
NEW = ("rt_skeleton_create", "rt_skeleton_destroy", "rt_skeleton_get_info", "rt_skeleton_set_pose", "rt_skeleton_add_clip", "rt_skeleton_clear_clips",
       "rt_skeleton_set_time", "rt_skeleton_read_pose", "rt_skeleton_read_joints", "rt_skeleton_read_palette", "rt_skeleton_get_palette_device_ptr",
       "rt_model_set_bones_from_skeleton")


def test_exports_and_their_argument_types(capi):
    u32, p, pu, pp, f = C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.c_float
    want = {"rt_skeleton_create": [p, u32, p, p, pp], "rt_skeleton_destroy": [p], "rt_skeleton_get_info": [p, pu, pu, pu],
            "rt_skeleton_set_pose": [p, p, u32], "rt_skeleton_add_clip": [p, u32, p, p, pu], "rt_skeleton_clear_clips": [p],
            "rt_skeleton_set_time": [p, u32, f], "rt_skeleton_read_pose": [p, p], "rt_skeleton_read_joints": [p, p], "rt_skeleton_read_palette": [p, p],
            "rt_skeleton_get_palette_device_ptr": [p, pp], "rt_model_set_bones_from_skeleton": [p, p]}
    assert set(want) == set(NEW)
    lib = capi.lib()
    for name in NEW:
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and args == want[name], name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(NEW) <= exported, set(NEW) - exported
    for method in ("set_pose", "set_pose_device", "add_clip", "clear_clips", "set_time", "pose", "joints", "palette", "palette_ptr", "info", "close"):
        assert callable(getattr(capi.Skeleton, method)), method
    assert callable(capi.Model.set_bones_from)


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared under a comment marked EXTENSION that cites the import that drops bones and node animation (RtModel.cpp:26)
    and the generators' never-taken update path (BottomLevelASGenerator.h:136-176); the header states the definition in full; the sentence
    about rt_model_set_bones knowing no hierarchy stands; the C++ mirror has the class and the overload, marked the same way; the example
    exists and is built"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    assert re.search(r"^typedef struct rt_skeleton\s+rt_skeleton;", text, flags=re.M)
    for name in NEW:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near and "RtModel.cpp:26" in near and "BottomLevelASGenerator.h:136-176" in near, name
    assert "the library knows no hierarchy" in text
    block = re.sub(r"\s+", " ", text[text.index("Posed skeletons"):text.index("int rt_model_set_bones_from_skeleton")].replace("\n * ", " "))
    for words in ("aiProcess_PreTransformVertices", "xx = x*x, yy = y*y, zz = z*z, xy = x*y, xz = x*z, yz = y*z, wx = w*x, wy = w*y, wz = w*z",
                  "R00 = 1 - 2*(yy + zz) R01 = 2*(xy - wz) R02 = 2*(xz + wy)", "R10 = 2*(xy + wz) R11 = 1 - 2*(xx + zz) R12 = 2*(yz - wx)",
                  "R20 = 2*(xz - wy) R21 = 2*(yz + wx) R22 = 1 - 2*(xx + yy)", "L[r][c] = R[r][c] * s_c", "L[r][3] = t_r", "turns +x into +y",
                  "C[r][c] = (A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c]", "C[r][3] = ((A[r][0] B[0][3] + A[r][1] B[1][3]) + A[r][2] B[2][3]) + A[r][3]",
                  "W_j = L_j for a root, bit for bit", "W_j = W_parent(j) o L_j", "M_j = W_j o inverse_bind_j, always multiplied, for an identity too",
                  "K == 1 or t <= times[0] gives i = 0, a = 0", "t >= times[K-1] gives i = K-2, a = 1", "a = (t - times[i]) / (times[i+1] - times[i])",
                  "Looping is the caller's", "A_c + (a * (B_c - A_c))", "d = ((Ax Bx + Ay By) + Az Bz) + Aw Bw", "a NaN d negates nothing",
                  "n = ((qx qx + qy qy) + qz qz) + qw qw", "0 < n < inf, else (0, 0, 0, 1)", "rt_model_recompute_normals", "not normalised by rt_skeleton_set_pose",
                  "no contraction", "nothing changes when a call refuses", "touches no model and no scene", "the message names the joint", "the message names the key",
                  "the message names rt_skeleton_set_pose", "RT_ERR_STATE", "RT_ERR_INVALID_ARG", "RT_MEM_HOST", "RT_MEM_DEVICE", "keeps earlier clip ids valid",
                  "1 .. 65536", "reads a live palette"):
        assert words in block, words
    tail = text[text.index("int rt_skeleton_get_palette_device_ptr"):text.index("int rt_model_set_bones_from_skeleton")]
    for words in ("exactly rt_model_set_bones(m, palette, RT_MEM_DEVICE)", "gives both numbers", "different contexts", "rt_model_set_skin", "rt_scene_update"):
        assert words in re.sub(r"\s+", " ", tail.replace("\n * ", " ")), words
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    sk = mirror[mirror.index("class RtSkeleton"):mirror.index("class RtModel")]
    for sig in (r"static SharedPtr create\(RtContext::SharedPtr context, const int32_t \*parents, const float \*inverseBind3x4, uint32_t numJoints\)",
                r"void setPose\(const float \*trs, bool deviceMemory = false\)", r"uint32_t addClip\(const float \*times, const float \*trs, uint32_t numKeys\)",
                r"void setTime\(uint32_t clip, float t\)"):
        assert re.search(sig, sk), sig
    above = mirror[mirror.index("RtSkeleton -- EXTENSION"):mirror.index("class RtSkeleton")]
    assert "RtModel.cpp:26" in above and "BottomLevelASGenerator.h:136-176" in above
    model = mirror[mirror.index("class RtModel"):mirror.index("class RtScene")]
    assert re.search(r"void setBones\(const RtSkeleton::SharedPtr &skeleton\)", model)
    above = model[model.index("void setBones(const float"):model.index("void setBones(const RtSkeleton")]
    assert "EXTENSION" in above and "RtModel.cpp:26" in above and "BottomLevelASGenerator.h:136-176" in above
    example = open(os.path.join(ROOT, "examples", "realtime_character.cpp")).read()
    for words in ("RtSkeleton::create(", "addClip(", "setTime(clip", "setBones(skeleton)", "->update(context)", "JOINTS = 4, KEYS = 3"):
        assert words in example, words
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_character" in make.split("BIN =")[1].splitlines()[0] and "examples/realtime_character.cpp" in make
    assert "rt_skeleton.hip" in make.split("SRCS =")[1].split("HDRS")[0]


def test_lds_limit_is_a_named_constant():
    """RT_SKELETON_LDS_JOINTS is defined in rt_skeleton.h, with its reasoning; 48 B per joint of W, and the 8 B per joint of the level table and
    offsets the comment counts beside them, fit the 64 KiB the comment claims (a block's limit on every CDNA part)"""
    n = S.lds_joints()
    text = open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", "rt_skeleton.h")).read()
    comment = text[:text.index("#define RT_SKELETON_LDS_JOINTS")].split("\n\n")[-1]
    assert "64 KiB" in comment and "48 B per joint" in comment and "160 KiB" in comment
    assert 1 <= n and 48 * n <= 64 * 1024 and (48 + 8) * n + 4 <= 64 * 1024
    assert n >= 300, "a character's 50 - 300 joints are posed from LDS"
    assert "hip" not in re.sub(r"//.*", "", text).lower(), "rt_skeleton.h is host code without HIP"


def test_null_handles_and_null_arrays_are_refused(capi):
    """argument checks need no device"""
    lib = capi.lib()
    x = np.zeros(120, np.float32)
    par = np.array([-1, 0, 1], np.int32)
    px, pp = x.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p)
    h, u, ptr = C.c_void_p(), C.c_uint32(7), C.c_void_p()
    fake = C.c_void_p(8)                                 # (a non-null handle that the checks must not follow)
    for rc in (lib.rt_skeleton_create(None, 3, pp, px, C.byref(h)), lib.rt_skeleton_create(fake, 3, pp, px, None),
               lib.rt_skeleton_create(fake, 3, None, px, C.byref(h)), lib.rt_skeleton_create(fake, 3, pp, None, C.byref(h)),
               lib.rt_skeleton_get_info(None, C.byref(u), C.byref(u), C.byref(u)), lib.rt_skeleton_set_pose(None, px, 0),
               lib.rt_skeleton_add_clip(None, 1, px, px, C.byref(u)), lib.rt_skeleton_clear_clips(None), lib.rt_skeleton_set_time(None, 0, 0.0),
               lib.rt_skeleton_read_pose(None, px), lib.rt_skeleton_read_joints(None, px), lib.rt_skeleton_read_palette(None, px),
               lib.rt_skeleton_get_palette_device_ptr(None, C.byref(ptr)), lib.rt_model_set_bones_from_skeleton(None, fake),
               lib.rt_model_set_bones_from_skeleton(fake, None)):
        assert rc == -1
        assert b"null" in lib.rt_last_error()
    assert h.value is None and u.value == 7 and ptr.value is None
    # the hierarchy is validated before anything touches the context: the joint is named
    bad = np.array([-1, 0, 2, 1], np.int32)
    assert lib.rt_skeleton_create(fake, 4, bad.ctypes.data_as(C.c_void_p), px, C.byref(h)) == -1 and b"joint 2 names parent 2" in lib.rt_last_error()
    bad = np.array([-1, -2], np.int32)
    assert lib.rt_skeleton_create(fake, 2, bad.ctypes.data_as(C.c_void_p), px, C.byref(h)) == -1 and b"joint 1 names parent -2" in lib.rt_last_error()
    for n in (0, 65537):
        assert lib.rt_skeleton_create(fake, n, pp, px, C.byref(h)) == -1 and b"1 .. 65536" in lib.rt_last_error()
    assert lib.rt_skeleton_destroy(None) == 0            # (as rt_model_destroy)


# ---- rt_skeleton.h under sanitizers ------------------------------------------------------------------------------------------------------
def host_cases():
    """(kind, payload, expected): hierarchies of 1, 65 and 65536 joints of every family, every refusal; key times and queries"""
    out = []
    for n in (1, 65, 65536):
        for family in S.HIERARCHIES:
            out.append((0, S.hierarchy(family, n, seed=n), (0, 0)))
    p = S.hierarchy("random", 65, 3)
    for j, v, what in ((40, 40, "parent == j"), (7, 64, "parent > j"), (0, 0, "joint 0 its own parent"), (33, -2, "parent < -1"), (64, -2 ** 31, "INT_MIN")):
        bad = p.copy()
        bad[j] = v
        if j != 64:
            bad[64] = 64                                 # (a later one that must not be the one named)
        out.append((0, bad, (3, j)))
    out.append((0, np.zeros(0, np.int32), (2, 0)))
    out.append((0, np.full(65537, -1, np.int32), (2, 0)))
    for K in (1, 2, 3, 17):
        times, _ = S.clip(np.array([-1], np.int32), K, seed=K)
        out.append((1, (times, np.array(S.sample_times(times), np.float32)), (0, 0)))
    t = np.array([0.0, 1.0, 2.0, 3.0], np.float32)
    none = np.zeros(0, np.float32)
    for bad, want in ((np.array([0.0, 2.0, 1.0, 3.0], np.float32), (4, 2)), (np.array([0.0, 1.0, 1.0, 3.0], np.float32), (4, 2)),
                      (np.array([1.0, 0.0], np.float32), (4, 1)), (np.array([0.0, np.nan, 2.0], np.float32), (3, 1)),
                      (np.array([np.inf], np.float32), (3, 0)), (np.array([0.0, 1.0, -np.inf], np.float32), (3, 2)), (none, (2, 0))):
        out.append((1, (bad, t), want))
    return out


def test_hierarchies_and_segments_under_asan_ubsan(tmp_path):
    """the program's level order, level offsets and packed table == numpy's for 1, 65 and 65536 joints of every family; its (i, a) pairs ==
    numpy's, a bit for bit, for K = 1, 2, 3, 17 below, on, between and beyond the keys; refused: parent == j, > j, < -1 (the first such joint
    named), 0 and 65537 joints, unsorted, equal and non-finite times (the key named), no keys, null arrays; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "skeleton_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "skeleton_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cases = host_cases()
    blob = b""
    for kind, payload, _ in cases:
        if kind == 0:
            blob += np.array([0, len(payload)], np.uint32).tobytes() + np.ascontiguousarray(payload, np.int32).tobytes()
        else:
            times, ts = payload
            blob += np.array([1, len(times)], np.uint32).tobytes() + times.tobytes() + np.array([len(ts)], np.uint32).tobytes() + ts.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d cases, 0 sanitizer reports" % len(cases) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    raw = (tmp_path / "out.bin").read_bytes()
    at = 0
    for kind, payload, want in cases:
        assert tuple(np.frombuffer(raw, np.uint32, 2, at)) == want, (kind, len(payload), want)
        at += 8
        if want[0] != 0:
            continue
        if kind == 0:
            n = len(payload)
            order, offsets = S.levels_of(payload)
            n_levels = int(np.frombuffer(raw, np.uint32, 1, at)[0])
            assert n_levels == len(offsets) - 1, n
            at += 4
            assert np.frombuffer(raw, np.uint32, n, at).tobytes() == order.tobytes(), n
            at += 4 * n
            assert np.frombuffer(raw, np.uint32, n_levels + 1, at).tobytes() == offsets.tobytes(), n
            at += 4 * (n_levels + 1)
            par = payload[order].astype(np.int64)
            table = (order.astype(np.int64) | (np.where(par < 0, 0xFFFF, par) << 16)).astype(np.uint32)
            assert np.frombuffer(raw, np.uint32, n, at).tobytes() == table.tobytes(), n
            at += 4 * n
        else:
            times, ts = payload
            for t in ts:
                i, a = S.segment(times, t)
                assert int(np.frombuffer(raw, np.uint32, 1, at)[0]) == i and np.frombuffer(raw, np.float32, 1, at + 4).tobytes() == np.float32(a).tobytes(), (len(times), t)
                at += 8
    assert at == len(raw)


def test_what_the_cases_are_there_for():
    """the generators give what they say: levels, roots, zero quaternions, negative and zero scales, -0, poison above descendants"""
    assert len(S.levels_of(S.hierarchy("forest", 65))[1]) == 2 and len(S.levels_of(S.hierarchy("chain", 300))[1]) == 301
    assert list(S.levels_of(S.hierarchy("star", 65))[1]) == [0, 1, 65]
    p = S.hierarchy("random", 257, 1)
    assert (p < np.arange(257)).all() and p.min() == -1 and (p[1:] == -1).any() and len(S.levels_of(p)[1]) > 4
    assert (S.hierarchy("roots", 65, 2) == -1).sum() >= 9
    raw = S.pose("raw", p, 3)
    length = np.linalg.norm(raw[:, 3:7].astype(np.float64), axis=1)
    assert (length == 0).any() and (length[length > 0] < 0.9).any() and (length > 1.1).any()
    mirror = S.pose("mirror", p, 4)
    assert (mirror[:, 7:10] < 0).any() and (mirror[:, 7:10] == 0).any()
    nz = S.pose("neg_zero", p, 5)
    assert (np.signbit(nz) & (nz == 0)).any() and (~np.signbit(nz) & (nz == 0)).any()
    bad = S.pose("nan_inf", p, 6)
    a, b = S.poisoned(p)
    assert np.isnan(bad[a]).sum() == 1 and np.isinf(bad[b]).sum() == 1 and np.isfinite(np.delete(bad, [a, b], axis=0)).all()
    assert S.descendants(p, [a]).sum() > 1 and S.descendants(p, [b]).sum() > 1
    W, M = S.posed(p, S.inverse_binds(257, 7), bad)
    assert np.array_equal(np.isnan(W).any(axis=1) | np.isinf(W).any(axis=1), S.descendants(p, [a, b]))
    times, keys = S.clip(p, 17, 8)
    assert len(times) == 17 and keys.shape == (17, 257, 10) and (np.diff(times) > 0).all()


# ---- the restatement is geometry ---------------------------------------------------------------------------------------------------------
def test_local_of_is_the_rotation_of_its_quaternion():
    """for 10^5 unit quaternions (s = 1) the nine entries of local_of are within 8 * 2^-24 of the same formula in float64 on the same fp32
    inputs.  The bound is derived: with |q| = 1 every product xx .. wz is at most 1 in magnitude and rounds once (2^-25 each, relative to
    1), their sum or difference rounds once more (its magnitude is at most 1: 2^-25), doubling is exact and doubles what has gathered --
    three roundings of magnitude <= 1, doubled: 6 * 2^-25 = 3 * 2^-24 --, and the final subtraction from 1 rounds a value of magnitude at
    most 1 once (2^-25); the fp32 inputs' own |q| - 1 is common to both sides.  3.5 * 2^-24, held to 8 * 2^-24; a numpy run shows 2.5 * 2^-24.
    And the hand case: q = (0, 0, sqrt(1/2), sqrt(1/2)) turns +x into +y -- column vectors."""
    rng = np.random.default_rng(11)
    n = 100000
    trs = np.zeros((n, 10), np.float32)
    trs[:, 3:7] = S.unit_quaternions(n, rng)
    trs[:, 7:10] = 1.0
    L = S.local_of(trs)
    x, y, z, w = (trs[:, 3 + c].astype(np.float64) for c in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    got = L.reshape(n, 3, 4)[:, :, :3].reshape(n, 9).astype(np.float64)
    err = np.abs(got - R).max()
    print("local_of vs float64: max error %.3f * 2^-24" % (err * 2.0 ** 24))
    assert err <= 8 * 2.0 ** -24
    assert (L.reshape(n, 3, 4)[:, :, 3] == 0).all()
    # what it states is a rotation: orthonormal to the same order
    R3 = got.reshape(n, 3, 3)
    assert np.abs(np.einsum("nij,nkj->nik", R3, R3) - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(R3) - 1).max() < 1e-6
    h = np.float32(np.sqrt(0.5))
    hand = S.local_of(np.array([[1, 2, 3, 0, 0, h, h, 1, 1, 1]], np.float32)).reshape(3, 4)
    assert np.abs(hand[:, :3] @ np.array([1.0, 0.0, 0.0]) - np.array([0.0, 1.0, 0.0])).max() <= 8 * 2.0 ** -24
    assert np.abs(hand[:, :3] @ np.array([0.0, 1.0, 0.0]) - np.array([-1.0, 0.0, 0.0])).max() <= 8 * 2.0 ** -24
    assert list(hand[:, 3]) == [1.0, 2.0, 3.0]
    # T.R.S: the scale acts first (column c of R times s_c), the translation last
    scaled = S.local_of(np.array([[0, 0, 0, 0, 0, h, h, 2, 3, 4]], np.float32)).reshape(3, 4)
    assert np.abs(scaled[:, :3] @ np.array([1.0, 0.0, 0.0]) - np.array([0.0, 2.0, 0.0])).max() <= 16 * 2.0 ** -24
    # compose is the affine product, a child under its parent: the chain's end is where float64 puts it
    p = np.array([-1, 0, 1], np.int32)
    pose = S.pose("unit", p, 12)
    W, M = S.posed(p, S.inverse_binds(3, 13), pose)
    full = [np.vstack([S.local_of(pose[j:j + 1]).reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]) for j in range(3)]
    assert np.abs((full[0] @ full[1] @ full[2])[:3] - W[2].reshape(3, 4)).max() < 1e-5
    assert W[0].tobytes() == S.local_of(pose[0:1]).tobytes()
