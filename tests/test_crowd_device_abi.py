"""CPU-only side of crowds driven from device memory (rt_crowd_set_layout, rt_crowd_get_layout, rt_crowd_set_blend_device): the exports,
their binding, their citations and the header's statement of the split -- structure on the host, scalars on the device -- and of what a NaN
time does; the C++ mirror, the example and the documents; null arguments refused without a device; the segment and the layer record written
once, for the host and for the kernel; and the host's check and packing of a layout (dxrexperiments_amd/csrc/rt_crowd.h) as a stand-alone
CPU program under AddressSanitizer + UndefinedBehaviorSanitizer against its Python restatement (tests/crowd_device_cases.py).  (The GPU side:
tests/test_gpu_crowd_device.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import crowd_device_cases as CD
import skeleton_cases as S
from dxrexperiments_amd import rtypes as T

ROOT = S.ROOT
u32, p, pu = C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)
WANT = {
    "rt_crowd_set_layout": [p, u32, p],
    "rt_crowd_get_layout": [p, pu],
    "rt_crowd_set_blend_device": [p, p, p],
}
POSE_CITATION = ("RtModel.cpp:26", "BottomLevelASGenerator.h:136-176")


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
    for method in ("set_layout", "layout", "set_blend_device"):
        assert callable(getattr(capi.Crowd, method)), method


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared, with the arguments the issue gave it, under a comment marked EXTENSION with both citations; the "Posed
    skeletons" block says what is now true and keeps its other sentences"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in WANT:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near, name
        for words in POSE_CITATION:
            assert words in near, (name, words)
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int rt_crowd_set_layout(rt_crowd *c, uint32_t n_layers, const rt_skeleton_layer *layers /* n_actors x n_layers, actor major, host */);",
                 "int rt_crowd_get_layout(const rt_crowd *c, uint32_t *n_layers /* 0: none */);",
                 "int rt_crowd_set_blend_device(rt_crowd *c, const float *times /* n_actors x n_layers, device */, const float *weights /* n_actors x n_layers, device, or NULL */);"):
        assert decl in flat, decl
    block = re.sub(r"\s+", " ", text[text.index("Posed skeletons"):text.index("int rt_skeleton_create")].replace("\n * ", " "))
    for words in ("No per-actor IK", "no posing of a sub-range of actors", "no rigs above 1024 joints", "Actor a of a crowd is, bit for bit, a skeleton given the same call",
                  "counts one pose for the whole crowd", "Times and weights may be read from device memory (rt_crowd_set_blend_device)",
                  "is the host's (rt_crowd_set_layout)", "indices that become addresses", "it gives (0, NaN)", "it gives (0, 0)", "inside [0, n_keys)",
                  "memory-safe whatever the arrays hold"):
        assert words in block, words
    assert "no times or layers read from device memory" not in block
    rest = re.sub(r"\s+", " ", text[text.index("int rt_crowd_set_blend("):text.index("int rt_crowd_read_pose")].replace("\n * ", " "))
    for words in ("The `time` of an entry is not read", "with every time taken as 0", "the first bad actor wins", "uploaded ONCE", "It poses nothing and counts no pose",
                  "neither use it nor disturb it", "Nothing changes when the call refuses", "Exactly ONE kernel launch on the context's stream", "no upload, no host loop over the actors, no wait",
                  "rt_crowd_set_times with the times on the device", "It counts one pose for the whole crowd", "as in rt_skeleton_solve_ik", "memory-safe for any 32 bits",
                  "the arrays are the caller's again once the stream has passed the launch", "a STALE layout", "both messages name rt_crowd_set_layout"):
        assert words in rest, words


def test_the_mirror_the_example_and_the_documents():
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    crowd = mirror[mirror.index("---- RtCrowd"):mirror.index("class RtModel")]
    for sig in (r"void setLayout\(const rt_skeleton_layer \*layers, uint32_t numLayers\)", r"void setBlendDevice\(const float \*times, const float \*weights = nullptr\)"):
        at = re.search(sig, crowd)
        assert at, sig
        comment = "\n".join(line for line in crowd[:at.start()].splitlines()[-4:] if line.strip().startswith("//"))
        assert "EXTENSION" in comment and "RtModel.cpp:26" in comment and "BottomLevelASGenerator.h:136-176" in comment, sig
    example = open(os.path.join(ROOT, "examples", "realtime_crowd_device.cpp")).read()
    for words in ("RtSkeleton::create(", "RtCrowd::create(", "addClip(", "setLayout(", "setBlendDevice(", "rt_device_alloc(", "rt_device_upload(", "attach(", "->update(context)"):
        assert words in example, words
    loop = example[example.index("for (UINT frame = 1;"):example.index("denoiser->readOutput")]
    assert "setBlendDevice(" in loop and "rt_device_upload" not in loop and "setLayout" not in loop, "nothing is uploaded inside the loop"
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_crowd_device" in make.split("BIN =")[1].splitlines()[0]
    rule = re.search(r"^\$\(LIBDIR\)/realtime_crowd_device: examples/realtime_crowd_device\.cpp .*\n\t\$\(CXX\) \$\(HOSTFLAGS\)", make, flags=re.M)
    assert rule, "built by the host compiler like the other examples"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for words in ("rt_crowd_set_layout", "rt_crowd_set_blend_device", "rt_crowd_lds_bytes_device", "(0, NaN)"):
        assert words in design, words
    readme = open(os.path.join(ROOT, "README.md")).read()
    for words in ("realtime_crowd_device.cpp", "rt_crowd_set_blend_device", "crowd_layout_sanitized.cpp"):
        assert words in readme, words


def test_the_segment_and_the_record_are_written_once():
    """rt_skeleton_segment and the sampling half of a record are RT_HOST_DEVICE functions of rt_skeleton.h, which the packing of the host and
    the kernel both call; the slot and its packing stand in rt_crowd.h; both headers stay host code without HIP; the kernel has no search of
    its own"""
    csrc = os.path.join(ROOT, "dxrexperiments_amd", "csrc")
    sk = open(os.path.join(csrc, "rt_skeleton.h")).read()
    cr = open(os.path.join(csrc, "rt_crowd.h")).read()
    assert len(re.findall(r"^RT_HOST_DEVICE static inline void rt_skeleton_segment\(", sk, flags=re.M)) == 1
    assert len(re.findall(r"^RT_HOST_DEVICE static inline void rt_skeleton_sample_layer\(", sk, flags=re.M)) == 1
    pack = sk[sk.index("static inline void rt_skeleton_pack_layer("):]
    pack = pack[:pack.index("\n}\n")]
    assert "rt_skeleton_sample_layer(" in pack and "rt_skeleton_segment(" not in pack and "key_a" not in pack
    assert len(re.findall(r"rt_skeleton_segment\(", re.sub(r"//.*", "", sk))) == 2, "the definition and the one call"
    assert "struct rt_crowd_slot {" in cr and "static inline void rt_crowd_pack_slots(" in cr and "static inline size_t rt_crowd_lds_bytes_device(" in cr
    of_slot = cr[cr.index("RT_HOST_DEVICE static inline void rt_crowd_layer_of_slot("):]
    assert "rt_skeleton_sample_layer(" in of_slot[:of_slot.index("\n}\n")]
    for name, header in (("rt_skeleton.h", sk), ("rt_crowd.h", cr)):
        assert "hip" not in re.sub(r"//.*", "", header).lower(), "%s is host code without HIP" % name
    kernel = re.sub(r"//.*", "", open(os.path.join(csrc, "rt_crowd.hip")).read())
    assert "rt_crowd_layer_of_slot(" in kernel and "rt_skeleton_segment" not in kernel and "mid" not in re.findall(r"k_crowd_pose\(.*?\n}\n", kernel, flags=re.S)[0]
    assert len(re.findall(r"template <uint32_t BLOCK, bool DEVICE>\s*__global__ void __launch_bounds__\(BLOCK\) k_crowd_pose\(", kernel)) == 1, "one kernel, two forms"
    assert len(re.findall(r"<<<", kernel)) == 2, "one launch per form"


def test_null_arguments_are_refused(capi):
    """argument checks need no device"""
    lib = capi.lib()
    layers = capi.Skeleton.layers([(0, 0.0)])
    pl = layers.ctypes.data_as(C.c_void_p)
    u = C.c_uint32(7)
    fake = C.c_void_p(8)                                 # (a non-null handle, or device address, that the checks must not follow)
    for rc in (lib.rt_crowd_set_layout(None, 1, pl), lib.rt_crowd_set_layout(fake, 1, None), lib.rt_crowd_get_layout(None, C.byref(u)), lib.rt_crowd_get_layout(fake, None),
               lib.rt_crowd_set_blend_device(None, fake, None), lib.rt_crowd_set_blend_device(fake, None, None), lib.rt_crowd_set_blend_device(fake, None, fake)):
        assert rc == -1
        assert b"null" in lib.rt_last_error()
    assert u.value == 7


def test_layouts_under_asan_ubsan(tmp_path):
    """the program's (code, actor, layer) and packed slots == the Python restatement's for every case -- a NaN time among them, which a
    layout accepts --; for clips of 1, 2, 3, 8 and 33 unevenly spaced keys and every time of skeleton_cases.sample_times plus NaN the record
    made of a slot equals the record rt_skeleton_pack_layer makes, word for word (the program's own check), its (i, a) is the restatement's,
    and for a NaN it is (0, NaN), or (0, 0) on one key; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "crowd_layout_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "crowd_layout_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cases = CD.layout_cases()
    blob = np.array([len(cases)], np.uint32).tobytes()
    for lists, n_layers, n_clips, n_masks, posed, null, n_joints in cases:
        flat = [rec for records in lists for rec in records]
        a = np.array(flat, T.SKELETON_LAYER) if flat else np.zeros(0, T.SKELETON_LAYER)
        blob += np.array([len(lists), n_layers, len(a), n_clips, n_masks, int(posed), int(null), n_joints], np.uint32).tobytes() + a.tobytes()
    parents = S.hierarchy("forest", 1)
    clips = [S.clip(parents, k, 70 + k)[0] for k in CD.SEARCH_KEYS]
    assert all(len(set(np.diff(t).tolist())) == len(t) - 1 for t in clips), "uneven spacing"
    blob += np.array([len(clips)], np.uint32).tobytes()
    n_queries = 0
    for times in clips:
        qs = np.array(CD.search_queries(times), np.float32)
        assert np.isnan(qs).sum() == 1 and len(qs) == len(S.sample_times(times)) + 1
        blob += np.array([len(times)], np.uint32).tobytes() + times.tobytes() + np.array([len(qs)], np.uint32).tobytes() + qs.tobytes()
        n_queries += len(qs)
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d cases, %d queries, 0 sanitizer reports" % (len(cases), n_queries) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.returncode, r.stdout, r.stderr[-3000:])
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint32)
    at = 0
    seen, nan_accepted = set(), 0
    for lists, n_layers, n_clips, n_masks, posed, null, n_joints in cases:
        want = (1, 0, 0) if null else CD.validate(lists, n_clips, n_masks, posed)
        assert tuple(int(x) for x in got[at:at + 3]) == want, (lists, n_clips, n_masks, posed, want)
        at += 3
        seen.add(want[0])
        if want[0] == 0:
            nan_accepted += any(np.isnan(rec[1]) and rec[0] != CD.N for records in lists for rec in records)
            for records in lists:
                for k, rec in enumerate(records):
                    assert tuple(int(x) for x in got[at:at + 7]) == CD.slot_words(rec, k), (rec, k)
                    at += 7
    assert seen == set(range(10)) - {6}, "a refusal no case reaches, or a NaN time refused"
    assert nan_accepted >= 10, "layouts whose times are NaN are accepted"
    for times in clips:
        for t in CD.search_queries(times):
            i, a = CD.segment(times, t)
            gi, ga = int(got[at]), got[at + 1:at + 2].view(np.float32)[0]
            at += 2
            if np.isnan(t):
                assert (gi, bool(np.isnan(ga))) == (0, True) if len(times) > 1 else (gi, int(got[at - 1])) == (0, 0), (len(times), gi, ga)
            assert gi == i and (np.isnan(ga) if np.isnan(a) else ga.tobytes() == np.float32(a).tobytes()), (len(times), t, gi, ga, i, a)
    assert at == len(got)
