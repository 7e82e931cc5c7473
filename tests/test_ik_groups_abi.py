"""CPU-only side of ordered IK groups (rt_skeleton_solve_ik_groups, rt_crowd_set_ik_chain_groups, rt_crowd_get_ik_chain_groups): the exports,
their binding, their citations and what the header now says of constraints that depend on one another; the C++ mirror, the example, the
Makefile and the documents; null arguments refused without a device; the kernel and its single launch in the unit of their own, the crowd
reaching it through one function; and the host's check, its refusals, the packed table and the group ends
(dxrexperiments_amd/csrc/rt_ik_groups.h) as a stand-alone CPU program under AddressSanitizer + UndefinedBehaviorSanitizer against their
Python restatement (tests/ik_group_cases.py).  (The GPU side: tests/test_gpu_ik_groups.py.)"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

import crowd_ik_cases as CI
import ik_cases as IK
import ik_group_cases as G
import skeleton_cases as S
from dxrexperiments_amd import rtypes as T

ROOT = S.ROOT
CSRC = os.path.join(ROOT, "dxrexperiments_amd", "csrc")
u32, p, pu = C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)
WANT = {
    "rt_skeleton_solve_ik_groups": [p, u32, p, p],
    "rt_crowd_set_ik_chain_groups": [p, u32, p, p],
    "rt_crowd_get_ik_chain_groups": [p, pu, pu],
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
    assert callable(capi.Skeleton.solve_ik_groups) and callable(capi.Crowd.set_ik_chain_groups) and callable(capi.Crowd.ik_chain_groups)
    sizes, a = capi.Skeleton.constraint_groups([[("two_bone", 3, (1, 2, 3), (4, 5, 6))], [("aim", 3, (0, 1, 0), (0, 1, 0), 0.5), (1, 2, (0, 0, 1), (1, 0, 0))]])
    assert sizes.dtype == np.uint32 and sizes.tolist() == [1, 2] and a.dtype == T.SKELETON_IK and a["kind"].tolist() == [0, 1, 1] and a["joint"].tolist() == [3, 3, 2]


def test_declarations_cite_what_they_stand_in_for():
    """each export is declared as the issue gave it under a comment marked EXTENSION with both citations; the limit of eight groups is
    defined and called a choice; the "Posed skeletons" block states the definition and no longer leaves dependent constraints to two
    calls alone; the calls state their refusals in order and their launches"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    for name in WANT:
        at = re.search(r"^int %s\s*\(" % name, text, flags=re.M)
        assert at, name
        near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
        assert "EXTENSION" in near, name
        for words in POSE_CITATION:
            assert words in near, (name, words)
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int rt_skeleton_solve_ik_groups(rt_skeleton *sk, uint32_t n_groups, const uint32_t *group_sizes /* n_groups, host */, "
                 "const rt_skeleton_ik *constraints /* sum of the sizes, host */);",
                 "int rt_crowd_set_ik_chain_groups(rt_crowd *c, uint32_t n_groups, const uint32_t *group_sizes /* n_groups, host */, "
                 "const rt_skeleton_ik *chains /* sum of the sizes, host */);",
                 "int rt_crowd_get_ik_chain_groups(const rt_crowd *c, uint32_t *n_groups /* 0: none */, uint32_t *group_sizes /* RT_SKELETON_MAX_IK_GROUPS, or NULL */);"):
        assert decl in flat, decl
    types = open(os.path.join(ROOT, "include", "dxr_amd_types.h")).read()
    assert re.search(r"^#define RT_SKELETON_MAX_IK_GROUPS 8u$", types, flags=re.M)
    assert "Eight is a choice" in re.sub(r"\s+", " ", types.replace("\n * ", " "))
    block = re.sub(r"\s+", " ", text[text.index("Posed skeletons"):text.index("int rt_skeleton_create")].replace("\n * ", " "))
    for words in ("GROUPS (rt_skeleton_solve_ik_groups, rt_crowd_set_ik_chain_groups)", "1 .. RT_SKELETON_MAX_IK_GROUPS (8) groups", "The constraints WITHIN a group are independent",
                  "ACROSS groups anything goes", "exactly as n_groups successive rt_skeleton_solve_ik calls would, one per group in order, bit for bit",
                  "group g reads the W of the pose that group g - 1 left", "the whole list is checked before anything is solved", "a list of one group is rt_skeleton_solve_ik itself",
                  "Eight groups is a choice", "is given rt_skeleton_solve_ik_groups with the same constraints", "later groups solve against the pose that gives"):
        assert words in block, words
    rest = re.sub(r"\s+", " ", text[text.index("int rt_skeleton_solve_ik("):text.index("Attached instances -- EXTENSIONS")].replace("\n * ", " "))
    for words in ("exactly ONE kernel launch on the context's stream, one block that solves a group, walks the pose and meets at a barrier before the next group",
                  "A larger skeleton is checked as a whole and then takes the loop of rt_skeleton_solve_ik, two launches per group", "group_sizes is not read",
                  "a group of size 0 (the message names the group)", "no constraint is read", "says to put the reader in a later group", "nothing changes when the call refuses",
                  "rt_crowd_solve_ik keeps its signature and solves whatever list the crowd holds", "rt_crowd_get_ik_chains answers that n", "exactly ONE launch per rt_crowd_solve_ik",
                  "rt_crowd_set_ik_chains sets a list of one group", "After rt_crowd_set_ik_chains it says 1 and {n}", "the crowd keeps the list it had"):
        assert words in rest, words


def test_the_mirror_the_example_the_makefile_and_the_documents():
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    for sig in (r"void solveIKGroups\(const rt_skeleton_ik \*constraints, const uint32_t \*groupSizes, uint32_t numGroups\)",
                r"void setIKChainGroups\(const rt_skeleton_ik \*chains, const uint32_t \*groupSizes, uint32_t numGroups\)"):
        at = re.search(sig, mirror)
        assert at, sig
        comment = "\n".join(line for line in mirror[:at.start()].splitlines()[-4:] if line.strip().startswith("//"))
        assert "EXTENSION" in comment and "RtModel.cpp:26" in comment and "BottomLevelASGenerator.h:136-176" in comment, sig
    assert "dependent ones take two calls" not in mirror
    example = open(os.path.join(ROOT, "examples", "realtime_crowd_grasp.cpp")).read()
    for words in ("RtSkeleton::create(", "RtCrowd::create(", "addClip(", "setLayout(", "setIKChainGroups(", "setBlendDevice(", "solveIKDevice(", "solveIKGroups(", "rt_device_alloc(",
                  "rt_device_upload(", "attach(", "->update(context)", "RT_IK_TWO_BONE", "RT_IK_AIM", "rt_crowd_read_joints", "largest tip-to-target distance",
                  "largest angle between the aimed axis and the direction to the target", "byte for byte: %s"):
        assert words in example, words
    loop = example[example.index("for (UINT frame = 1;"):example.index("denoiser->readOutput")]
    assert loop.count("setBlendDevice(") == 1 and loop.count("solveIKDevice(") == 1 and loop.count("->update(context)") == 1
    for words in ("rt_device_upload", "setLayout", "setIKChains", "setIKChainGroups", "setPoses", "solveIK(", "setBlend("):
        assert words not in loop, "nothing is uploaded inside the loop: " + words
    assert "std::sin" not in example and "std::cos" not in example, "the example's inputs are + - * / and fmod alone: tests/golden/make_ik_group_bounds.py restates them"
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_crowd_grasp" in make.split("BIN =")[1].splitlines()[0]
    assert re.search(r"^\$\(LIBDIR\)/realtime_crowd_grasp: examples/realtime_crowd_grasp\.cpp .*\n\t\$\(CXX\) \$\(HOSTFLAGS\)", make, flags=re.M), "built by the host compiler like the other examples"
    assert "$(CSRC)/rt_ik_groups.hip" in make.split("SRCS =")[1].split("HDRS")[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for words in ("rt_skeleton_solve_ik_groups", "rt_crowd_set_ik_chain_groups", "k_ik_groups", "rt_ik_groups.hip", "ik_groups.py"):
        assert words in design, words
    assert "(they take two calls)" not in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    for words in ("realtime_crowd_grasp.cpp", "rt_skeleton_solve_ik_groups", "rt_ik_groups.hip", "rt_ik_groups.h", "ik_groups_sanitized.cpp", "tools/ik_groups.py"):
        assert words in readme, words
    bounds = json.load(open(os.path.join(ROOT, "tests", "golden", "ik_group_bounds.json")))
    assert set(bounds) >= {"frames", "aim_angle", "tip_to_target"} and os.path.exists(os.path.join(ROOT, "tests", "golden", "make_ik_group_bounds.py"))


def test_the_kernel_and_its_launch_live_in_the_unit_of_their_own():
    """k_ik_groups is one template in rt_ik_groups.hip with the arguments the issue gave it, its entry read before the loop, a uniform loop
    whose barriers stand outside divergent code, in the order solve, barrier, local_of, barrier, walk, barrier; one launch in the unit; the
    lane, the walk and the packing are the shared ones; the crowd reaches the launch through the one function rt_internal.h declares; the
    check's header is host code without HIP and words its own refusal its own way"""
    unit, crowd_ik, crowd, sk = code_of("rt_ik_groups.hip"), code_of("rt_crowd_ik.hip"), code_of("rt_crowd.hip"), code_of("rt_skeleton.hip")
    assert len(re.findall(r"template <uint32_t BLOCK>\s*__global__ void __launch_bounds__\(BLOCK\) k_ik_groups\(const IkTable chains, uint32_t n, uint64_t ends, uint32_t n_groups,", unit)) == 1
    kernel = re.findall(r"k_ik_groups\(const IkTable chains,.*?\n}\n", unit, flags=re.S)[0]
    assert "float *pose, float *joints," in kernel, "pose and joints are read and written in place: not __restrict__"
    loop = kernel[kernel.index("for (uint32_t g = 0; g < n_groups; g++)"):]
    assert "chains.e[tid]" in kernel[:kernel.index("for (uint32_t g = 0;")] and "chains." not in loop, "the entry is read once, before the loop"
    assert "targets ?" in kernel and "poles ?" in kernel and "weights ?" in kernel
    assert len(re.findall(r"__syncthreads\(\)", loop)) == 3 and len(re.findall(r"__syncthreads\(\)", kernel)) == 3
    order = [loop.index(w) for w in ("ik_solve_lane(", "__syncthreads()", "local_of(", "walk_levels<BLOCK, true>(")]
    assert order == sorted(order) and loop.index("walk_levels<BLOCK, true>(") < loop.rindex("__syncthreads()")
    for line in loop.splitlines():
        if "__syncthreads()" in line:
            assert line.startswith("        __syncthreads();"), "a barrier inside divergent code: " + line
    assert len(re.findall(r"<<<", unit)) == 1 and "rt_crowd_block(" in unit and "rt_crowd_lds_bytes(" in unit
    assert len(re.findall(r"ik_solve_lane\(", unit)) == 1 and "rt_ik_solve(" not in unit and "struct IkEntry" not in unit and ".kind = " not in unit
    assert len(re.findall(r"rt_skeleton_pack_ik\(", unit)) == 2, "the skeleton's call and the crowd's list both pack with the one function"
    for name in WANT:
        assert len(re.findall(r"^int %s\(" % name, unit, flags=re.M)) == 1, name
        assert name not in crowd_ik + crowd + sk, name
    assert "k_ik_groups" not in crowd_ik + crowd + sk
    internal = open(os.path.join(CSRC, "rt_internal.h")).read()
    assert "int rt_ik_groups_solve_crowd(rt_crowd *c, const float *targets, const float *poles, const float *weights);" in internal
    assert len(re.findall(r"rt_ik_groups_solve_crowd\(", crowd_ik)) == 1 and len(re.findall(r"^int rt_ik_groups_solve_crowd\(", unit, flags=re.M)) == 1
    assert "ik_group_ends" in internal and "n_ik_groups" in internal
    host = code_of("rt_ik_groups.h")
    assert "hip" not in host.lower(), "rt_ik_groups.h is host code without HIP"
    for words in ("static inline int rt_ik_groups_validate(", "static inline int rt_ik_groups_refusal(", "static inline uint64_t rt_ik_group_ends("):
        assert words in host, words
    assert "are not independent" not in host + unit and "put the reader in a later group" in host
    assert len(re.findall(r"rt_skeleton_validate_ik\(", host)) == 2, "the whole list, then each group's sub-list: the check of a constraint is reused"


def test_null_arguments_are_refused(capi):
    """argument checks need no device"""
    lib = capi.lib()
    sizes, a = capi.Skeleton.constraint_groups([[("aim", 0, (0, 0, 0), (0, 1, 0))]])
    ps, pa = sizes.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)
    u = C.c_uint32(7)
    fake = C.c_void_p(8)                                 # (a non-null handle that the checks must not follow)
    for rc in (lib.rt_skeleton_solve_ik_groups(None, 1, ps, pa), lib.rt_skeleton_solve_ik_groups(fake, 1, None, pa), lib.rt_skeleton_solve_ik_groups(fake, 1, ps, None),
               lib.rt_crowd_set_ik_chain_groups(None, 1, ps, pa), lib.rt_crowd_set_ik_chain_groups(fake, 1, None, pa), lib.rt_crowd_set_ik_chain_groups(fake, 1, ps, None),
               lib.rt_crowd_get_ik_chain_groups(None, C.byref(u), None), lib.rt_crowd_get_ik_chain_groups(fake, None, None)):
        assert rc == -1
        assert b"null" in lib.rt_last_error()
    assert u.value == 7


def test_the_check_under_asan_ubsan(tmp_path):
    """the program's (code, indices, total) for every list of ik_group_cases.check_cases == the Python restatement -- a list whose sizes or
    records must not be read has none behind its pointer --; the text of every refusal this check adds == its restatement, every other under
    the call's name, with its class; the packed table and the group ends of every list that passes == their restatements; every code is
    reached; no report"""
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "ik_groups_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "ik_groups_sanitized.cpp")
    assert re.search(r"^int main\(", open(src).read(), flags=re.M), "a program of its own"
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    cases = G.check_cases()
    blob = np.array([len(cases)], np.uint32).tobytes()
    for sizes, n_groups, records, parents, posed, null_sizes, null_records in cases:
        a = np.zeros(len(records), T.SKELETON_IK)
        for k, rec in enumerate(records):
            a[k] = rec
        blob += np.array([n_groups, len(sizes), len(a), len(parents), int(posed), int(null_sizes), int(null_records)], np.uint32).tobytes()
        blob += np.array(sizes, np.uint32).tobytes() + a.tobytes() + np.asarray(parents, np.int32).tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d lists, 0 sanitizer reports" % len(cases) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.returncode, r.stdout, r.stderr[-3000:])
    raw = (tmp_path / "out.bin").read_bytes()
    at, seen, packed = 0, set(), 0
    for sizes, n_groups, records, parents, posed, null_sizes, null_records in cases:
        told = sizes if n_groups == len(sizes) else [None] * min(n_groups, 9)       # (a count out of range: no size stands behind the pointer)
        want, bad = G.validate(told, records, parents, posed, null_sizes or null_records)
        got = np.frombuffer(raw, np.uint32, 6, at)
        what = (sizes, n_groups, records, np.asarray(parents).tolist())
        assert (int(got[0]), tuple(int(x) for x in got[1:5])) == (want, bad), (what, want, bad)
        total = min(sum(sizes), 0xFFFFFFFF) if want not in (1, 9, 10) else None
        if total is not None:
            assert int(got[5]) == total, what
        msg = raw[at + 24:at + 280].split(b"\0")[0].decode()
        rc = int(np.frombuffer(raw, np.int32, 1, at + 280)[0])
        at += 284
        seen.add(want)
        if want:
            assert rc == (-4 if want == 8 else -1), (what, want, rc)
            assert msg.startswith("who: "), msg
            text = G.refusal("who", want, bad, n_groups, total)
            assert text is None or msg == text, (msg, text)
            if want in range(3, 7):
                assert "constraint %d" % bad[0] in msg, msg
        else:
            assert msg == "" and rc == 0
        if want in (0, 8):
            n = len(records)
            table = np.frombuffer(raw, np.uint32, 12 * n, at).reshape(n, 12)
            entries = CI.packed_table(records, parents)
            entries[:, 5:8] = np.array([rec[2] for rec in records], np.float32).view(np.uint32)      # (a skeleton's entry carries its target)
            assert table.tobytes() == entries.tobytes(), what
            ends = np.frombuffer(raw, np.uint32, 2, at + 48 * n)
            assert int(ends[0]) | int(ends[1]) << 32 == G.group_ends(sizes), what
            at += 48 * n + 8
            packed += 1
    assert at == len(raw)
    assert seen == {0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11}, seen
    assert packed >= 10
