"""CPU-only side of device-sourced instance transforms and attached instances (rt_scene_set_instance_transforms_mem,
rt_scene_get_instance_transforms, rt_scene_attach_instances, rt_scene_detach_instances, rt_scene_get_instance_attachment,
rt_skeleton_get_joints_device_ptr): the exports, their binding, their citations, the header's statement of the rules, the C++ mirror, the
example and its Makefile rule; and the host side of an attachment -- a header of its own, dxrexperiments_amd/csrc/rt_attach.h -- as a
stand-alone CPU program under AddressSanitizer + UndefinedBehaviorSanitizer against numpy.  (The GPU side: tests/test_gpu_instance_attach.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from skin_cases import ROOT

NEW = ("rt_scene_set_instance_transforms_mem", "rt_scene_get_instance_transforms", "rt_scene_attach_instances", "rt_scene_detach_instances",
       "rt_scene_get_instance_attachment", "rt_skeleton_get_joints_device_ptr")
BOUND, LOCAL = 0x40000000, 0x80000000


def test_exports_and_their_argument_types(capi):
    u32, p, pu, pp = C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)
    want = {"rt_scene_set_instance_transforms_mem": [p, u32, u32, p, u32], "rt_scene_get_instance_transforms": [p, u32, u32, p],
            "rt_scene_attach_instances": [p, u32, u32, p, p, p], "rt_scene_detach_instances": [p, u32, u32],
            "rt_scene_get_instance_attachment": [p, u32, pp, pu], "rt_skeleton_get_joints_device_ptr": [p, pp]}
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
    for method in ("set_transforms_device", "transforms", "attach", "detach", "attachment"):
        assert callable(getattr(capi.Scene, method)), method
    assert callable(capi.Skeleton.joints_ptr)


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared under a comment marked EXTENSION that cites the Transform member of the instance descriptor
    (TopLevelASGenerator.cpp:344-362), the reference's one statement of a transform (RtScene.h:30) and the generators' never-taken update
    path (TopLevelASGenerator.h:144-163); the block states the rules; the sentences about posing and about rt_skeleton_read_joints stand; the
    C++ mirror has the methods, marked the same way; the example exists and is built"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in NEW:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near and "TopLevelASGenerator.cpp:344-362" in near and "RtScene.h:30" in near and "TopLevelASGenerator.h:144-163" in near, name
    assert "Setting a pose touches no model and no scene." in text
    assert "for attaching instances to joints" in re.sub(r"\s+", " ", text.replace("\n * ", " "))
    block = text[text.index("Attached instances -- EXTENSIONS"):text.index("int rt_scene_set_instance_transforms_mem")]
    block = re.sub(r"\s+", " ", block.replace("\n * ", " "))
    for words in ("RtScene.h:30", "libs/DXRFramework/Helpers/TopLevelASGenerator.cpp:344-362", "Helpers/TopLevelASGenerator.h:144-163",
                  "RT_MEM_HOST is exactly rt_scene_set_instance_transforms", "copied device to device, on the context's stream, into storage the scene owns",
                  "reserved once", "free again once the stream has passed the call", "a producer on another stream is the caller's to order",
                  "Nothing is downloaded and nothing waits", "an unknown `mem` is RT_ERR_INVALID_ARG", "count == 0 a no-op",
                  "host-set instances keep the upload they have", "follows in the final join", "no new synchronisation goes in front of the kernels",
                  "T_i = W_j o local_i", "every product and every sum one rounded operation, no contraction, always multiplied, for an identity too",
                  "T_i = W_j bit for bit", "NaN, inf and zero scales are no errors", "exactly a transform set by rt_scene_set_instance_transforms_mem(RT_MEM_DEVICE)",
                  "update == build, with attachments", "a frame is rt_skeleton_set_time, rt_scene_update", "copied to the device once",
                  "Attaching changes no stored transform", "Attaching again replaces the binding", "Posing a skeleton touches no model and no scene",
                  "stays built and traceable in the state of its last update", "The skeleton counts its poses", "no longer the \"nothing pending\" no-op",
                  "with one bump of the generation", "the message names rt_skeleton_set_pose", "everything pending is kept",
                  "the message names the instance and rt_scene_detach_instances", "marks nothing", "is not attached is a no-op",
                  "the message names the entry and both numbers", "a skeleton of another context", "nothing changes when a call refuses",
                  "retains an attached skeleton as it retains its models", "simply keep their last transform", "its own record of the pose it last applied"):
        assert words in block, words
    getter = text[text.index("int rt_scene_set_instance_transforms_mem"):text.index("int rt_scene_get_instance_transforms")]
    assert "pending or applied" in getter and "only then does the call synchronise" in re.sub(r"\s+", " ", getter.replace("\n * ", " "))
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    scene = mirror[mirror.index("class RtScene"):mirror.index("class RtProgram")]
    for sig in (r"void setTransforms\(uint32_t first, uint32_t count, const float \*transforms3x4, bool deviceMemory = false\)",
                r"void getTransforms\(uint32_t first, uint32_t count, float \*transforms3x4\) const",
                r"void attach\(uint32_t first, uint32_t count, RtSkeleton::SharedPtr skeleton, const uint32_t \*joints, const float \*locals = nullptr\)",
                r"void detach\(uint32_t first, uint32_t count\)"):
        assert re.search(sig, scene), sig
    above = scene[scene.index("void update(RtContext::SharedPtr context)"):scene.index("void setTransforms(")]
    assert "EXTENSIONS" in above and "RtScene.h:30" in above and "TopLevelASGenerator.cpp:344-362" in above and "TopLevelASGenerator.h:144-163" in above
    example = open(os.path.join(ROOT, "examples", "realtime_machines.cpp")).read()
    for words in ("RtSkeleton::create(", "addClip(", "scene->attach(0, BOXES, skeleton, joints, locals)", "skeleton->setTime(clip, t)", "scene->update(context)",
                  "getTransforms(", "parents[JOINTS] = {-1, 0, 1, 1, 0}", "KEYS = 3"):
        assert words in example, words
    loop = example[example.index("for (UINT frame = 1"):example.index("denoiser->readOutput")]
    assert "setTransform" not in loop and "setPose" not in loop, "a frame is setTime + update only"
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_machines" in make.split("BIN =")[1].splitlines()[0]
    assert re.search(r"^\$\(LIBDIR\)/realtime_machines: examples/realtime_machines\.cpp \$\(LIB\)", make, flags=re.M)
    header = open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", "rt_attach.h")).read()
    assert "hip" not in re.sub(r"//.*", "", header).lower(), "rt_attach.h is host code without HIP"


def test_null_handles_are_refused_without_a_device(capi):
    """argument checks need no device, and touch no output"""
    lib = capi.lib()
    x = np.zeros(24, np.float32)
    j = np.zeros(2, np.uint32)
    px, pj = x.ctypes.data_as(C.c_void_p), j.ctypes.data_as(C.c_void_p)
    sk, u, ptr = C.c_void_p(), C.c_uint32(7), C.c_void_p()
    fake = C.c_void_p(8)                                 # (a non-null handle that the checks must not follow)
    for rc in (lib.rt_scene_set_instance_transforms_mem(None, 0, 1, px, 1), lib.rt_scene_get_instance_transforms(None, 0, 1, px),
               lib.rt_scene_attach_instances(None, 0, 2, fake, pj, px), lib.rt_scene_attach_instances(fake, 0, 2, None, pj, px),
               lib.rt_scene_detach_instances(None, 0, 1), lib.rt_scene_get_instance_attachment(None, 0, C.byref(sk), C.byref(u)),
               lib.rt_skeleton_get_joints_device_ptr(None, C.byref(ptr)), lib.rt_skeleton_get_joints_device_ptr(fake, None)):
        assert rc == -1
        assert b"null" in lib.rt_last_error()
    assert sk.value is None and u.value == 7 and ptr.value is None


# ---- rt_attach.h under sanitizers --------------------------------------------------------------------------------------------------------
def host_cases():
    """(n_instances, first, count, n_joints, joints or None, has_local, words, n_read, expected (rc, bad))"""
    r = np.random.default_rng(5)
    out = []
    for n, first, count in ((1, 0, 1), (300, 0, 300), (300, 100, 65), (300, 299, 1), (300, 300, 0), (65536, 65000, 536), (7, 3, 0)):
        for nj in (1, 65, 65536):
            joints = r.integers(0, nj, count).astype(np.uint32)
            if count:
                joints[-1] = nj - 1                      # (the last legal joint)
            for n_words in (0, first + count // 2, n):   # no words, words for a part of the range, for every instance
                words = np.zeros(n_words, np.uint32)
                some = r.uniform(size=n_words) < 0.02
                words[some] = (r.integers(0, 65536, int(some.sum())) | BOUND | np.where(r.uniform(size=int(some.sum())) < 0.5, LOCAL, 0)).astype(np.uint32)
                if n_words:
                    words[0] = r.integers(0, 65536)      # (a joint without the bound bit: not attached)
                out.append((n, first, count, nj, joints, bool(n_words & 1), words, count, (0, 0)))
    none = np.zeros(0, np.uint32)
    # refusals: a null array; ranges beyond the instances (nothing is read: the arrays are empty); joints == and > n_joints, the first named
    out.append((5, 0, 2, 4, None, False, none, 0, (1, 0)))
    for n, first, count in ((5, 4, 2), (5, 6, 0), (5, 0, 6), (0, 0, 1), (5, 5, 1), (5, 1, 0xFFFFFFFF), (5, 0xFFFFFFFF, 2)):
        out.append((n, first, count, 4, none, True, none, 0, (2, 0)))
    for entry, value in ((0, 4), (3, 4), (7, 0xFFFFFFFF), (7, 65536)):
        joints = r.integers(0, 4, 8).astype(np.uint32)
        joints[entry] = value
        joints[7] = max(joints[7], 4)                    # (a later one that must not be the one named, unless it is the first)
        out.append((20, 5, 8, 4, joints, True, none, 8, (3, entry)))
    return out


def test_bindings_under_asan_ubsan(tmp_path):
    """the program's verdicts, the packed words (joint, bound bit, local bit) and the search of a range == numpy's, for ranges at both ends of
    lists of 1, 300 and 65536 instances, empty ranges, skeletons of 1, 65 and 65536 joints, scenes with no words, words for a part of the range
    and for every instance; refused: a null array, ranges beyond the instances (wrapping sums among them), joints == and > n_joints with the
    first such entry named; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "attach_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "attach_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cases = host_cases()
    blob = b""
    for n, first, count, nj, joints, has_local, words, n_read, _ in cases:
        blob += np.array([n, first, count, nj, joints is not None, has_local, len(words), n_read], np.uint32).tobytes()
        if joints is not None:
            blob += joints[:n_read].tobytes()
        blob += words.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d cases, 0 sanitizer reports" % len(cases) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    raw = (tmp_path / "out.bin").read_bytes()
    at = 0
    for n, first, count, nj, joints, has_local, words, n_read, want in cases:
        assert tuple(int(x) for x in np.frombuffer(raw, np.uint32, 2, at)) == want, (n, first, count, nj, want)
        at += 8
        if want[0] != 0:
            continue
        packed = np.frombuffer(raw, np.uint32, count, at)
        at += 4 * count
        assert np.array_equal(packed, joints | np.uint32(BOUND) | np.uint32(LOCAL if has_local else 0)), (n, first, count)
        assert np.array_equal(packed & 0xFFFF, joints & 0xFFFF) and (nj > 65535 or np.array_equal(packed & 0xFFFF, joints))
        held, which = (int(x) for x in np.frombuffer(raw, np.uint32, 2, at))
        at += 8
        inside = np.nonzero(words[first:first + count] & BOUND)[0]
        assert held == (1 if len(inside) else 0) and (not held or which == first + int(inside[0])), (n, first, count, len(words))
    assert at == len(raw)
    assert sum(1 for c in cases if c[-1] == (0, 0)) >= 60
