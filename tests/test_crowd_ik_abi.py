"""CPU-only side of inverse kinematics for crowds (rt_crowd_set_ik_chains, rt_crowd_get_ik_chains, rt_crowd_solve_ik): the exports, their
binding, their citations and what the header now says of a crowd's chains and an actor's values; the C++ mirror, the example and the
documents; null arguments refused without a device; the packing of a chain list and the lane of a constraint written once, for the skeleton
and for the crowd; and the host's check and packing (dxrexperiments_amd/csrc/rt_crowd_ik.h, rt_skeleton.h) as a stand-alone CPU program
under AddressSanitizer + UndefinedBehaviorSanitizer against its Python restatement (tests/crowd_ik_cases.py).  (The GPU side:
tests/test_gpu_crowd_ik.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import crowd_ik_cases as CI
import ik_cases as IK
import skeleton_cases as S
from dxrexperiments_amd import rtypes as T
from test_skeleton_ik_abi import constraint_lists

ROOT = S.ROOT
CSRC = os.path.join(ROOT, "dxrexperiments_amd", "csrc")
u32, p, pu = C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)
WANT = {
    "rt_crowd_set_ik_chains": [p, u32, p],
    "rt_crowd_get_ik_chains": [p, pu],
    "rt_crowd_solve_ik": [p, p, p, p, u32],
}
POSE_CITATION = ("RtModel.cpp:26", "BottomLevelASGenerator.h:136-176")


def code_of(name):
    """a source file without its comments"""
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


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
    for method in ("set_ik_chains", "ik_chains", "solve_ik", "solve_ik_device"):
        assert callable(getattr(capi.Crowd, method)), method


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared, with the arguments the issue gave it, under a comment marked EXTENSION with both citations; the "Posed
    skeletons" block says what is now true of a crowd's IK -- the chains are the crowd's, an actor brings values -- and what a NaN weight in
    device memory does; the calls state their refusals, their launches and their uploads"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in WANT:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near, name
        for words in POSE_CITATION:
            assert words in near, (name, words)
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int rt_crowd_set_ik_chains(rt_crowd *c, uint32_t n, const rt_skeleton_ik *chains /* n, host */);",
                 "int rt_crowd_get_ik_chains(const rt_crowd *c, uint32_t *n /* 0: none */);",
                 "int rt_crowd_solve_ik(rt_crowd *c, const float *targets /* n_actors x n x 3 */, const float *poles /* n_actors x n x 3, or NULL */, "
                 "const float *weights /* n_actors x n, or NULL */, uint32_t mem /* RT_MEM_HOST | RT_MEM_DEVICE */);"):
        assert decl in flat, decl
    block = re.sub(r"\s+", " ", text[text.index("Posed skeletons"):text.index("int rt_skeleton_create")].replace("\n * ", " "))
    for words in ("No per-actor IK chains: every actor solves the crowd's one list (rt_crowd_set_ik_chains) with its own targets, poles and weights (rt_crowd_solve_ik)",
                  "no posing of a sub-range of actors", "no rigs above 1024 joints", "the host checks the list once", "plain floats that are taken as given",
                  "is given rt_skeleton_solve_ik with the constraints (kind_k, joint_k, target[a * n + k], pole[a * n + k], weight[a * n + k])",
                  "for every weight that is not NaN", "from the pose the actor holds when the call is made", "a NaN weight in DEVICE memory is no error",
                  "every quaternion that constraint writes is (0, 0, 0, 1)"):
        assert words in block, words
    rest = re.sub(r"\s+", " ", text[text.index("int rt_model_set_bones_from_crowd("):text.index("Attached instances -- EXTENSIONS")].replace("\n * ", " "))
    for words in ("the `target` of an entry is not read", "the defaults of rt_crowd_solve_ik calls that bring no poles or no weights", "the same codes in the same order",
                  "the messages those of rt_skeleton_solve_ik under this call's name", "it needs no pose", "poses nothing, counts no pose, touches no device memory",
                  "no other crowd call uses it or disturbs it", "the crowd keeps the list it had", "rt_crowd_set_blend_device, rt_crowd_solve_ik, rt_scene_update",
                  "It counts one pose for the whole crowd", "the message names rt_crowd_set_ik_chains", "exactly ONE kernel launch on the context's stream: no upload, no host loop over the actors, no wait",
                  "memory-safe for any 32 bits in the three arrays", "a NaN weight is RT_ERR_INVALID_ARG (the message names the actor and the constraint; the first bad actor wins)",
                  "in ONE upload", "the two page-locked staging slots", "the call does not wait", "Nothing changes when the call refuses"):
        assert words in rest, words


def test_the_mirror_the_example_and_the_documents():
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    crowd = mirror[mirror.index("---- RtCrowd"):mirror.index("class RtModel")]
    for sig in (r"void setIKChains\(const rt_skeleton_ik \*chains, uint32_t count\)", r"void solveIK\(const float \*targets, const float \*poles = nullptr, const float \*weights = nullptr\)",
                r"void solveIKDevice\(const float \*targets, const float \*poles = nullptr, const float \*weights = nullptr\)"):
        at = re.search(sig, crowd)
        assert at, sig
        comment = "\n".join(line for line in crowd[:at.start()].splitlines()[-4:] if line.strip().startswith("//"))
        assert "EXTENSION" in comment and "RtModel.cpp:26" in comment and "BottomLevelASGenerator.h:136-176" in comment, sig
    example = open(os.path.join(ROOT, "examples", "realtime_crowd_reach.cpp")).read()
    for words in ("RtSkeleton::create(", "RtCrowd::create(", "addClip(", "setLayout(", "setIKChains(", "setBlendDevice(", "solveIKDevice(", "rt_device_alloc(", "rt_device_upload(",
                  "attach(", "->update(context)", "RT_IK_TWO_BONE", "rt_crowd_read_joints", "largest tip-to-target distance"):
        assert words in example, words
    loop = example[example.index("for (UINT frame = 1;"):example.index("denoiser->readOutput")]
    assert "setBlendDevice(" in loop and "solveIKDevice(" in loop and "->update(context)" in loop
    for words in ("rt_device_upload", "setLayout", "setIKChains", "setPoses", "solveIK(", "setBlend("):
        assert words not in loop, "nothing is uploaded inside the loop: " + words
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_crowd_reach" in make.split("BIN =")[1].splitlines()[0]
    assert re.search(r"^\$\(LIBDIR\)/realtime_crowd_reach: examples/realtime_crowd_reach\.cpp .*\n\t\$\(CXX\) \$\(HOSTFLAGS\)", make, flags=re.M), "built by the host compiler like the other examples"
    assert "$(CSRC)/rt_crowd_ik.hip" in make.split("SRCS =")[1].split("HDRS")[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for words in ("rt_crowd_set_ik_chains", "rt_crowd_solve_ik", "k_crowd_ik", "ik_solve_lane", "crowd_ik.py"):
        assert words in design, words
    assert "a solved actor is a skeleton of its own" not in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    for words in ("realtime_crowd_reach.cpp", "rt_crowd_solve_ik", "rt_crowd_ik.hip", "crowd_ik_sanitized.cpp"):
        assert words in readme, words


def test_the_packing_and_the_lane_are_written_once():
    """IkEntry, IkTable and rt_skeleton_pack_ik stand in rt_skeleton.h, and both units pack with that one function; the refusals of a list are
    one text; the lane of a constraint is ik_solve_lane of rt_pose_device.h, the only place that calls rt_ik_solve, and both kernels call
    it; the new host header stays free of HIP; the kernel is where the issue put it: one template, one launch, one barrier between the
    solve and the pose, the walk rt_pose_device.h's"""
    sk_h = open(os.path.join(CSRC, "rt_skeleton.h")).read()
    assert len(re.findall(r"^struct IkEntry \{", sk_h, flags=re.M)) == 1 and len(re.findall(r"^struct IkTable \{", sk_h, flags=re.M)) == 1
    assert len(re.findall(r"^static inline void rt_skeleton_pack_ik\(", sk_h, flags=re.M)) == 1
    assert len(re.findall(r"^static inline int rt_skeleton_ik_refusal\(", sk_h, flags=re.M)) == 1
    sk, cr, ik = code_of("rt_skeleton.hip"), code_of("rt_crowd.hip"), code_of("rt_crowd_ik.hip")
    for name, unit in (("rt_skeleton.hip", sk), ("rt_crowd_ik.hip", ik)):
        assert "struct IkEntry" not in unit and "struct IkTable" not in unit, name
        assert len(re.findall(r"rt_skeleton_pack_ik\(", unit)) == 1, name
        assert len(re.findall(r"rt_pose_refuse_ik\(", unit)) >= 1, name
        assert ".kind = " not in unit and "e.p = " not in unit, name + " packs by hand"
        assert "rt_ik_solve(" not in unit, name
        assert len(re.findall(r"ik_solve_lane\(", unit)) == 1, name
    assert "are not independent" not in sk + cr + ik and sk_h.count("are not independent") == 1, "the refusals of a list are one text"
    dev = code_of("rt_pose_device.h")
    assert len(re.findall(r"RT_DEV void ik_solve_lane\(", dev)) == 1 and len(re.findall(r"rt_ik_solve\(", dev)) == 1
    lane = dev[dev.index("RT_DEV void ik_solve_lane("):]
    assert "rt_ik_solve(" in lane[:lane.index("\n}\n")]
    assert "rt_ik_solve" not in cr and "k_crowd_ik" not in cr
    for name in ("rt_crowd_ik.h", "rt_crowd.h", "rt_skeleton.h"):
        assert "hip" not in code_of(name).lower(), "%s is host code without HIP" % name
    host = code_of("rt_crowd_ik.h")
    for words in ("static inline void rt_crowd_ik_chains(", "static inline int rt_crowd_ik_check_values(", "static inline void rt_crowd_ik_pack_values("):
        assert words in host, words
    assert len(re.findall(r"template <uint32_t BLOCK>\s*__global__ void __launch_bounds__\(BLOCK\) k_crowd_ik\(const IkTable chains,", ik)) == 1
    kernel = re.findall(r"k_crowd_ik\(const IkTable chains,.*?\n}\n", ik, flags=re.S)[0]
    assert len(re.findall(r"__syncthreads\(\)", kernel)) == 2, "one barrier between the solve and the pose, one before the walk"
    assert kernel.index("ik_solve_lane(") < kernel.index("__syncthreads()") < kernel.index("local_of(") < kernel.index("walk_levels<BLOCK, true>(")
    assert "float *pose, float *joints," in kernel, "pose and joints are read and written in place: not __restrict__"
    assert len(re.findall(r"<<<", ik)) == 1 and "rt_crowd_block(" in ik and "rt_crowd_lds_bytes(" in ik
    assert "crowd_stage(" in ik and "int crowd_stage(rt_crowd *c, size_t bytes, CrowdStage **out);" in open(os.path.join(CSRC, "rt_internal.h")).read()
    assert len(re.findall(r"^int crowd_stage\(", cr, flags=re.M)) == 1 and "hipHostMalloc" not in ik, "both units stage through the one definition"


def test_null_arguments_are_refused(capi):
    """argument checks need no device"""
    lib = capi.lib()
    chains = capi.Skeleton.constraints([("aim", 0, (0, 0, 0), (0, 1, 0))])
    pc = chains.ctypes.data_as(C.c_void_p)
    u = C.c_uint32(7)
    fake = C.c_void_p(8)                                 # (a non-null handle, or device address, that the checks must not follow)
    for rc in (lib.rt_crowd_set_ik_chains(None, 1, pc), lib.rt_crowd_set_ik_chains(fake, 1, None), lib.rt_crowd_get_ik_chains(None, C.byref(u)),
               lib.rt_crowd_get_ik_chains(fake, None), lib.rt_crowd_solve_ik(None, fake, None, None, 1), lib.rt_crowd_solve_ik(fake, None, None, None, 1),
               lib.rt_crowd_solve_ik(fake, None, fake, fake, 0)):
        assert rc == -1
        assert b"null" in lib.rt_last_error()
    assert u.value == 7


def test_chains_and_values_under_asan_ubsan(tmp_path):
    """the program's (code, indices) for chain lists == ik_cases.validate with a pose taken for granted -- a list the check must not read has
    no record behind its pointer --; the packed table == its Python restatement, entry for entry, every target zero; the host-value check's
    (code, actor, constraint) and the block of the one upload == their restatements; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "crowd_ik_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "crowd_ik_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    lists = constraint_lists()
    blob = np.array([len(lists)], np.uint32).tobytes()
    for records, n, parents, posed, null in lists:
        a = np.zeros(len(records), T.SKELETON_IK)
        for k, rec in enumerate(records):
            a[k] = (rec[0], rec[1], (np.nan, np.inf, -1.0), rec[3], rec[4])           # (a target is not read: a NaN there is fine)
        blob += np.array([n, len(a), len(parents), int(null)], np.uint32).tobytes() + a.tobytes() + parents.tobytes()
    calls = CI.value_cases()
    blob += np.array([len(calls)], np.uint32).tobytes()
    for n_actors, n, targets, poles, weights in calls:
        blob += np.array([n_actors, n, poles is not None, weights is not None], np.uint32).tobytes() + targets.tobytes()
        blob += (b"" if poles is None else poles.tobytes()) + (b"" if weights is None else weights.tobytes())
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d lists, %d calls, 0 sanitizer reports" % (len(lists), len(calls)) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.returncode, r.stdout, r.stderr[-3000:])
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint32)
    at = 0
    seen, packed = set(), 0
    for records, n, parents, posed, null in lists:
        want = (1, (0, 0, 0)) if null else (2, (0, 0, 0)) if n != len(records) else IK.validate(records, parents, True)
        assert (int(got[at]), tuple(int(x) for x in got[at + 1:at + 4])) == want, (records, parents.tolist(), want)
        at += 4
        seen.add(want[0])
        if want[0] == 0:
            table = got[at:at + 12 * n].reshape(n, 12)
            assert table.tobytes() == CI.packed_table(records, parents).tobytes(), (records, parents.tolist())
            assert not table[:, 5:8].any(), "a chain has no target"
            at += 12 * n
            packed += 1
    assert seen == set(range(8)), "a refusal no case reaches, or a pose asked for"
    assert packed >= 50
    refused = 0
    for n_actors, n, targets, poles, weights in calls:
        want = CI.check_values(weights)
        assert tuple(int(x) for x in got[at:at + 3]) == want, (n_actors, n, want)
        off_p, off_w, floats, block = CI.value_block(targets, poles, weights)
        assert tuple(int(x) for x in got[at + 3:at + 6]) == (off_p, off_w, floats)
        assert got[at + 6:at + 6 + floats].tobytes() == block.tobytes()
        at += 6 + floats
        refused += want[0] == 6
    assert refused >= 20 and any(np.isnan(t).all() and CI.check_values(w)[0] == 0 for _, _, t, _, w in calls), "NaN targets are no refusal"
    assert at == len(got)
