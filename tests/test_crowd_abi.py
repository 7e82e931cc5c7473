"""CPU-only side of crowds (rt_crowd_*, rt_model_set_bones_from_crowd, rt_scene_attach_instances_crowd,
rt_scene_get_instance_crowd_attachment): the exports, their binding, their citations and the header's statement of the definition, the C++
mirror, the example and the documents; null arguments refused without a device; the device arithmetic written once, in a header both
translation units include; and the host's check and packing of every actor's layer list (dxrexperiments_amd/csrc/rt_crowd.h) as a
stand-alone CPU program under AddressSanitizer + UndefinedBehaviorSanitizer against its Python restatement (tests/crowd_cases.py).  (The GPU
side: tests/test_gpu_crowd.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import crowd_cases as CC
import skeleton_cases as S
from dxrexperiments_amd import rtypes as T

ROOT = S.ROOT
u32, p, pp, pu = C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)
WANT = {
    "rt_crowd_create": [p, u32, pp],
    "rt_crowd_destroy": [p],
    "rt_crowd_get_info": [p, pp, pu, pu],
    "rt_crowd_set_poses": [p, p, u32],
    "rt_crowd_set_times": [p, p, p],
    "rt_crowd_set_blend": [p, u32, p],
    "rt_crowd_read_pose": [p, u32, u32, p],
    "rt_crowd_read_joints": [p, u32, u32, p],
    "rt_crowd_read_palette": [p, u32, u32, p],
    "rt_crowd_get_joints_device_ptr": [p, pp],
    "rt_crowd_get_palette_device_ptr": [p, pp],
    "rt_model_set_bones_from_crowd": [p, p, u32],
    "rt_scene_attach_instances_crowd": [p, u32, u32, p, p, p, p],
    "rt_scene_get_instance_crowd_attachment": [p, u32, pp, pu, pu],
}
POSE_CITATION = ("RtModel.cpp:26", "BottomLevelASGenerator.h:136-176")
SCENE_CITATION = ("TopLevelASGenerator.cpp:344-362", "RtScene.h:30", "TopLevelASGenerator.h:144-163")


def test_exports_and_their_argument_types(capi):
    lib = capi.lib()
    for name, want in WANT.items():
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and args == want, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want, name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert set(WANT) <= exported, set(WANT) - exported
    for method in ("set_poses", "set_poses_device", "set_times", "set_blend", "pose", "joints", "palette", "joints_ptr", "palette_ptr", "info", "close"):
        assert callable(getattr(capi.Crowd, method)), method
    assert callable(capi.Model.set_bones_from_crowd) and callable(capi.Scene.attach_crowd) and callable(capi.Scene.crowd_attachment)


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared, with the arguments the issue of crowds gave it, under a comment marked EXTENSION with the citation of its
    neighbours; the definition stands in the "Posed skeletons" comment; the semantics are in the header"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in WANT:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near, name
        for words in (SCENE_CITATION if name.startswith("rt_scene") else POSE_CITATION):
            assert words in near, (name, words)
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int rt_crowd_create(rt_skeleton *sk, uint32_t n_actors, rt_crowd **out);",
                 "int rt_crowd_destroy(rt_crowd *c);",
                 "int rt_crowd_get_info(const rt_crowd *c, rt_skeleton **sk, uint32_t *n_actors, uint32_t *n_joints);",
                 "int rt_crowd_set_poses(rt_crowd *c, const float *trs /* n_actors x n_joints x 10 */, uint32_t mem);",
                 "int rt_crowd_set_times(rt_crowd *c, const uint32_t *clips /* n_actors */, const float *times /* n_actors */);",
                 "int rt_crowd_set_blend(rt_crowd *c, uint32_t n_layers, const rt_skeleton_layer *layers /* n_actors x n_layers, actor major, host */);",
                 "int rt_crowd_read_pose(rt_crowd *c, uint32_t first_actor, uint32_t count, float *trs",
                 "int rt_crowd_read_joints(rt_crowd *c, uint32_t first_actor, uint32_t count, float *world3x4",
                 "int rt_crowd_read_palette(rt_crowd *c, uint32_t first_actor, uint32_t count, float *palette3x4",
                 "int rt_crowd_get_joints_device_ptr(rt_crowd *c, void **ptr);",
                 "int rt_crowd_get_palette_device_ptr(rt_crowd *c, void **ptr);",
                 "int rt_model_set_bones_from_crowd(rt_model *m, rt_crowd *c, uint32_t actor);",
                 "int rt_scene_attach_instances_crowd(rt_scene *s, uint32_t first, uint32_t count, rt_crowd *c, const uint32_t *actors /* count */, const uint32_t *joints /* count */, const float *local3x4",
                 "int rt_scene_get_instance_crowd_attachment(const rt_scene *s, uint32_t instance, rt_crowd **c /* NULL: none */, uint32_t *actor, uint32_t *joint);"):
        assert decl in flat, decl
    assert "typedef struct rt_crowd rt_crowd;" in text
    block = re.sub(r"\s+", " ", text[text.index("Posed skeletons"):text.index("int rt_skeleton_create")].replace("\n * ", " "))
    for words in ("a CROWD is n_actors poses of ONE skeleton", "Actor a of a crowd is, bit for bit, a skeleton given the same call", "pose[n_actors][n_joints][10]",
                  "joints[n_actors][n_joints][12]", "palette[n_actors][n_joints][12]", "that actor's own held pose", "counts one pose for the whole crowd",
                  "one kernel launch", "No per-actor IK"):
        assert words in block, words
    rest = re.sub(r"\s+", " ", text[text.index("int rt_crowd_create"):].replace("\n * ", " "))
    for words in ("one layer without a mask is rt_skeleton_set_time, bit for bit", "the message names the actor and the layer", "the first bad actor wins",
                  "two page-locked slots written in turn", "does not wait for the device", "Nothing changes when the call refuses", "RT_ERR_UNSUPPORTED",
                  "exactly rt_model_set_bones(m, palette + actor * n_joints * 12, RT_MEM_DEVICE)", "reports skeleton attachments only",
                  "rt_scene_detach_instances lets go of either kind"):
        assert words in rest, words


def test_the_mirror_the_example_and_the_documents():
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    crowd = mirror[mirror.index("---- RtCrowd"):mirror.index("class RtModel")]
    for sig in (r"static SharedPtr create\(RtSkeleton::SharedPtr skeleton, uint32_t numActors\)", r"void setPoses\(const float \*trs\)",
                r"void setTimes\(const uint32_t \*clips, const float \*times\)", r"void setBlend\(const rt_skeleton_layer \*layers, uint32_t numLayers\)"):
        assert re.search(sig, crowd), sig
    assert "EXTENSION" in crowd and "RtModel.cpp:26" in crowd
    assert re.search(r"void setBones\(const std::shared_ptr<RtCrowd> &crowd, uint32_t actor\)", mirror)
    assert re.search(r"void attach\(uint32_t first, uint32_t count, const std::shared_ptr<RtCrowd> &crowd, const uint32_t \*actors, const uint32_t \*joints", mirror)
    example = open(os.path.join(ROOT, "examples", "realtime_crowd.cpp")).read()
    for words in ("RtSkeleton::create(", "RtCrowd::create(", "addClip(", "setTimes(", "attach(", "->update(context)"):
        assert words in example, words
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_crowd" in make.split("BIN =")[1].splitlines()[0] and "examples/realtime_crowd.cpp" in make
    assert "rt_crowd.hip" in make.split("SRCS =")[1].split("HDRS")[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for words in ("rt_crowd", "k_crowd_pose", "tools/crowd_update.py"):
        assert words in design, words
    readme = open(os.path.join(ROOT, "README.md")).read()
    for words in ("rt_crowd.hip", "rt_crowd.h", "rt_pose_device.h", "realtime_crowd.cpp"):
        assert words in readme, words


def test_the_pose_arithmetic_is_written_once():
    """local_of, compose, unit_or_identity, sample_joint, hamilton, the body of one blend layer, the store of a local pose and the walk over
    the levels with its palette step are defined in rt_pose_device.h and nowhere else; both translation units include it and neither takes a
    level table's entry apart itself; rt_crowd.h is host code without HIP"""
    csrc = os.path.join(ROOT, "dxrexperiments_amd", "csrc")
    shared = open(os.path.join(csrc, "rt_pose_device.h")).read()
    for name in ("local_of", "compose", "unit_or_identity", "sample_joint", "hamilton", "blend_layer", "blend_joint", "store_pose", "walk_levels"):
        define = r"^RT_DEV void %s\(" % name
        assert len(re.findall(define, shared, flags=re.M)) == 1, name
        for unit in ("rt_skeleton.hip", "rt_crowd.hip"):
            body = open(os.path.join(csrc, unit)).read()
            assert not re.search(define, body, flags=re.M) and '#include "rt_pose_device.h"' in body, (name, unit)
    for unit in ("rt_skeleton.hip", "rt_crowd.hip"):
        body = re.sub(r"//.*", "", open(os.path.join(csrc, unit)).read())
        assert "P[c] + w *" not in body and "rsqrt_ieee" not in body, unit
        assert "entry >> 16" not in body and "walk_levels<" in body and "store_pose(" in body, unit
    header = open(os.path.join(csrc, "rt_crowd.h")).read()
    assert "static inline int rt_crowd_validate_layers(" in header and "static inline void rt_crowd_pack_layers(" in header
    assert "hip" not in re.sub(r"//.*", "", header).lower(), "rt_crowd.h is host code without HIP"


def test_null_handles_and_null_arrays_are_refused(capi):
    """argument checks need no device"""
    lib = capi.lib()
    x = np.zeros(16, np.float32)
    w = np.zeros(4, np.uint32)
    layers = capi.Skeleton.layers([(0, 0.0)])
    px, pw, pl = x.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), layers.ctypes.data_as(C.c_void_p)
    u = C.c_uint32(7)
    h = C.c_void_p(0)
    fake = C.c_void_p(8)                                 # (a non-null handle that the checks must not follow)
    for rc in (lib.rt_crowd_create(None, 1, C.byref(h)), lib.rt_crowd_create(fake, 1, None), lib.rt_crowd_get_info(None, None, C.byref(u), None),
               lib.rt_crowd_set_poses(None, px, 0), lib.rt_crowd_set_poses(fake, None, 0), lib.rt_crowd_set_times(None, pw, px), lib.rt_crowd_set_times(fake, None, px),
               lib.rt_crowd_set_times(fake, pw, None), lib.rt_crowd_set_blend(None, 1, pl), lib.rt_crowd_set_blend(fake, 1, None),
               lib.rt_crowd_read_pose(None, 0, 1, px), lib.rt_crowd_read_pose(fake, 0, 1, None), lib.rt_crowd_read_joints(None, 0, 1, px),
               lib.rt_crowd_read_joints(fake, 0, 1, None), lib.rt_crowd_read_palette(None, 0, 1, px), lib.rt_crowd_read_palette(fake, 0, 1, None),
               lib.rt_crowd_get_joints_device_ptr(None, C.byref(h)), lib.rt_crowd_get_joints_device_ptr(fake, None), lib.rt_crowd_get_palette_device_ptr(None, C.byref(h)),
               lib.rt_crowd_get_palette_device_ptr(fake, None), lib.rt_model_set_bones_from_crowd(None, fake, 0), lib.rt_model_set_bones_from_crowd(fake, None, 0),
               lib.rt_scene_attach_instances_crowd(None, 0, 1, fake, pw, pw, None), lib.rt_scene_attach_instances_crowd(fake, 0, 1, None, pw, pw, None),
               lib.rt_scene_attach_instances_crowd(fake, 0, 1, fake, None, pw, None), lib.rt_scene_attach_instances_crowd(fake, 0, 1, fake, pw, None, None),
               lib.rt_scene_get_instance_crowd_attachment(None, 0, C.byref(h), C.byref(u), C.byref(u))):
        assert rc == -1
        assert b"null" in lib.rt_last_error()
    assert u.value == 7 and not h.value
    assert lib.rt_crowd_destroy(None) == 0               # (as every destroy: a null handle is nothing to do)


def test_actor_lists_under_asan_ubsan(tmp_path):
    """the program's (code, actor, layer) and packed records == the Python restatement's for every case; a list the validator must not read
    has no record behind its pointer, so that reading it is a report; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "crowd_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "crowd_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cases = CC.layer_cases()
    blob = b""
    for lists, n_layers, n_clips, n_masks, posed, null, n_joints in cases:
        flat = [rec for records in lists for rec in records]
        a = np.array(flat, T.SKELETON_LAYER) if flat else np.zeros(0, T.SKELETON_LAYER)
        blob += np.array([len(lists), n_layers, len(a), n_clips, n_masks, int(posed), int(null), n_joints], np.uint32).tobytes() + a.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d cases, 0 sanitizer reports" % len(cases) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint32)
    at = 0
    seen, named = set(), set()
    for lists, n_layers, n_clips, n_masks, posed, null, n_joints in cases:
        want = (1, 0, 0) if null else CC.validate(lists, n_clips, n_masks, posed)
        assert tuple(int(x) for x in got[at:at + 3]) == want, (lists, n_clips, n_masks, posed, want)
        at += 3
        seen.add(want[0])
        if want[0] > 2:
            named.add((want[0] >= 7, want[1] == 0, want[1] == len(lists) - 1, n_layers))
        if want[0] == 0:
            for records in lists:
                for k, rec in enumerate(records):
                    assert tuple(int(x) for x in got[at:at + 9]) == CC.packed(rec, k, n_joints), (rec, k, n_joints)
                    at += 9
    assert at == len(got)
    assert seen == set(range(10)), "a refusal no case reaches"
    for group in (False, True):
        for n_layers in (1, 8):
            assert (group, True, False, n_layers) in named or (group, True, True, n_layers) in named, "the first actor bad"
            assert (group, False, True, n_layers) in named, "the last actor bad"


def test_what_the_cases_are_there_for():
    """the rigs straddle a wave, the widest block and reach the LDS limit as a chain; neighbouring actors sit on different clips; the numpy
    statement is held to every actor of a small case and to the first, a middle and the last of a large one"""
    assert [n for _, n in CC.RIGS] == [1, 5, 3, 9, 64, 65, 256, 257, S.lds_joints()] and CC.RIGS[-1][0] == "chain" and CC.ACTORS == (1, 2, 300)
    parents, ib, clips, masks = CC.rig("random", 65)
    assert [len(t) for t, _ in clips] == [1, 3, 2] and len(masks) == 3 and ib.shape == (65, 12)
    times = CC.actor_times(clips, 300)
    assert all(times[a][0] != times[a + 1][0] for a in range(299))
    assert len({t for c, t in times if c == 1}) >= 8
    assert CC.numpy_actors(2, 1024) == [0, 1] or CC.numpy_actors(2, 1024) == [0, 1, 2][:2]
    assert CC.numpy_actors(300, 1024) == [0, 150, 299] and CC.numpy_actors(300, 1) == list(range(300))
    layers = CC.actor_layers(clips, 3, 4, 3)
    assert len(layers) == 4 and all(len(l) == 3 for l in layers) and layers[0] != layers[1]
    assert CC.actor_poses(parents, 5).shape == (5, 65, 10)
