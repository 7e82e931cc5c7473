"""CPU-only side of two-bone reach and aim constraints (rt_skeleton_solve_ik): the export, its binding, the constraint record and its numpy
dtype, its citations and the header's statement of the definition, the C++ mirror and the example; null arguments refused without a device;
the host's check of a constraint list (dxrexperiments_amd/csrc/rt_skeleton.h: rt_skeleton_validate_ik) and the solver of one constraint
(dxrexperiments_amd/csrc/rt_ik.h) as a stand-alone CPU program under AddressSanitizer + UndefinedBehaviorSanitizer, against their Python
restatements (tests/ik_cases.py), the solver bit for bit; and the restatement against geometry, in float64.  (The GPU side:
tests/test_gpu_skeleton_ik.py.)"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ik_cases as K
import skeleton_cases as S
from dxrexperiments_amd import rtypes as T

ROOT = S.ROOT
F = np.float32
BOUNDS = os.path.join(ROOT, "tests", "golden", "ik_bounds.json")
HOLD = 4.0                      # times the recorded errors: rounding depends on the case, and seeds not drawn may round worse


def test_export_and_its_argument_types(capi):
    want = [C.c_void_p, C.c_uint32, C.c_void_p]
    res, args = capi.SIGNATURES["rt_skeleton_solve_ik"]
    assert res is C.c_int and args == want
    fn = capi.lib().rt_skeleton_solve_ik
    assert fn.restype is C.c_int and list(fn.argtypes) == want
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "rt_skeleton_solve_ik" in set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for method in ("solve_ik", "constraints"):
        assert callable(getattr(capi.Skeleton, method)), method


def test_the_constraint_record_is_36_bytes(tmp_path, capi):
    """sizeof(rt_skeleton_ik) == 36 in C99 with the members where the numpy dtype puts them, the constants are the header's, and
    Skeleton.constraints fills the record from tuples and dicts"""
    src = tmp_path / "ik.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dxr_amd_types.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %u %u %u\\n", '
                   "sizeof(rt_skeleton_ik), offsetof(rt_skeleton_ik, kind), offsetof(rt_skeleton_ik, joint), offsetof(rt_skeleton_ik, target), "
                   "offsetof(rt_skeleton_ik, pole), offsetof(rt_skeleton_ik, weight), RT_SKELETON_MAX_IK, RT_IK_TWO_BONE, RT_IK_AIM); return 0; }\n")
    exe = tmp_path / "ik"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    d = T.SKELETON_IK
    names = ("kind", "joint", "target", "pole", "weight")
    assert d.itemsize == 36 and got[0] == 36
    assert got[1:6] == [d.fields[name][1] for name in names] == [0, 4, 8, 20, 32]
    assert [d.fields[name][0] for name in names] == [np.dtype("<u4"), np.dtype("<u4"), np.dtype(("<f4", (3,))), np.dtype(("<f4", (3,))), np.dtype("<f4")]
    assert got[6:] == [T.SKELETON_MAX_IK, T.IK_TWO_BONE, T.IK_AIM] == [32, 0, 1] == [K.MAX_IK, K.TWO_BONE, K.AIM]
    types = open(os.path.join(ROOT, "include", "dxr_amd_types.h")).read()
    assert re.search(r"static_assert\(sizeof\(rt_skeleton_ik\) == 36,", types)
    a = capi.Skeleton.constraints([("two_bone", 3, (1, 2, 3), (4, 5, 6)), (1, 7, [0.5, 0, 0], [0, 1, 0], 0.25),
                                   {"kind": "aim", "joint": 2, "target": (1, 1, 1), "pole": (0, 0, 1)}, {"kind": 0, "joint": 9, "target": (0, 0, 0), "pole": (1, 0, 0), "weight": -0.5}])
    assert a.dtype == d
    assert a["kind"].tolist() == [0, 1, 1, 0] and a["joint"].tolist() == [3, 7, 2, 9] and a["weight"].tolist() == [1.0, 0.25, 1.0, -0.5]
    assert a["target"].tolist() == [[1, 2, 3], [0.5, 0, 0], [1, 1, 1], [0, 0, 0]] and a["pole"].tolist() == [[4, 5, 6], [0, 1, 0], [0, 0, 1], [1, 0, 0]]


def test_declaration_cites_what_it_stands_in_for():
    """the export is declared under a comment marked EXTENSION with the citation the neighbouring skeleton exports carry; the header states the
    definition; DESIGN.md has IK in scope; the C++ mirror has the method; the example exists and is built; rt_ik.h and rt_skeleton.h are free
    of HIP"""
    text = open(os.path.join(ROOT, "include", "dxr_amd.h")).read()
    at = re.search(r"^int rt_skeleton_solve_ik\s*\(", text, flags=re.M)
    assert at
    near = re.findall(r"/\*.*?\*/", text[:at.start()], flags=re.S)[-1]
    assert "EXTENSION" in near and "RtModel.cpp:26" in near and "BottomLevelASGenerator.h:136-176" in near
    assert re.search(r"^int rt_skeleton_solve_ik\(rt_skeleton \*sk, uint32_t n, const rt_skeleton_ik \*constraints /\* n, host \*/\);", text, flags=re.M)
    block = re.sub(r"\s+", " ", text[text.index("Posed skeletons"):text.index("int rt_model_set_bones_from_skeleton")].replace("\n * ", " "))
    for words in ("1 .. RT_SKELETON_MAX_IK (32)", "unit(v) = v * (1 / sqrt(v.v)) if 0 < v.v < inf, else the zero vector and NO ANSWER",
                  "rot(q, v) = (v + (w * t)) + (q_xyz x t) with t = 2 * (q_xyz x v)", "the lowest index on a tie", "if s.s < 1e-6, or unit(s) has no answer, the half turn (perp(u), 0)",
                  "the quaternion (u x h, u.h) normalised by the rule", "never fmin or fmax", "the quiet NaN 0x7FC00000", "used as given, bit for bit", "I = inverse(W_p)",
                  "An aim's axis is not transformed", "pa = t_a, pb = L_a(t_b), pc = L_a(L_b(t_c))", "lo = |l1 - l2|, hi = l1 + l2", "x = ((l1 l1 - l2 l2) + d d) / (2 d)",
                  "h = sqrt(hh if hh > 0 else 0)", "m = unit(k - n * (k.n)) with k = P - pa", "pb' = (pa + n * x) + m * h and pc' = pa + n * d", "A' = normalised(Da (x) A)",
                  "b1 = pa + rot(Da, pb - pa) and c1 = pa + rot(Da, pc - pa)", "B' = normalised((conj(A') (x) (Db (x) A')) (x) B)", "v = unit(rot(Q, axis)) and w = unit(T - t_j)",
                  "Q' = normalised(between(v, w) (x) Q)", "q_c = A_c + (weight * (A'_c - A_c))", "A weight of 0 therefore writes normalised(A)", "keep their bits", "INDEPENDENT",
                  "that is two calls, the second seeing the first's pose", "posed exactly as rt_skeleton_set_pose poses", "when a and b carry uniform scale",
                  "No joint limits, no chains longer than two bones, no CCD or FABRIK", "the message names both constraints and the shared joint",
                  "nothing is uploaded and nothing waits", "Every constraint is held to the first group before the state is looked at"):
        assert words in block, words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_skeleton_ik" in design and "rt_skeleton_solve_ik" in design and "skeleton_ik_timing.py" in design
    mirror = open(os.path.join(ROOT, "dxrexperiments_amd", "include", "DXRFramework.h")).read()
    sk = mirror[mirror.index("class RtSkeleton"):mirror.index("class RtModel")]
    assert re.search(r"void solveIK\(const rt_skeleton_ik \*constraints, uint32_t count\)", sk)
    above = sk[:sk.index("void solveIK")].split("void setBlend")[1]
    assert "EXTENSION" in above and "RtModel.cpp:26" in above and "BottomLevelASGenerator.h:136-176" in above
    example = open(os.path.join(ROOT, "examples", "realtime_reach.cpp")).read()
    for words in ("RtSkeleton::create(", "addClip(", "setTime(", "solveIK(", "setBones(skeleton)", "->update(context)", "RT_IK_TWO_BONE", "RT_IK_AIM", "attach(", "rt_skeleton_read_joints"):
        assert words in example, words
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/realtime_reach" in make.split("BIN =")[1].splitlines()[0] and "examples/realtime_reach.cpp" in make
    header = open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", "rt_skeleton.h")).read()
    assert "static inline int rt_skeleton_validate_ik(" in header
    for name in ("rt_skeleton.h", "rt_ik.h", "rt_xform.h"):
        code = re.sub(r"//.*", "", open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", name)).read())
        assert "hip/" not in code.lower() and "#include <hip" not in code.lower(), name
    assert "hip" not in re.sub(r"//.*", "", header).lower(), "rt_skeleton.h is host code without HIP"
    ik = open(os.path.join(ROOT, "dxrexperiments_amd", "csrc", "rt_ik.h")).read()
    assert "clang fp contract(off)" in ik and "RT_HOST_DEVICE" in ik and "fmin" not in ik and "fmax" not in ik and "acos" not in ik and "sin" not in re.sub(r"//.*", "", ik)


def test_null_handles_and_null_arrays_are_refused(capi):
    """argument checks need no device"""
    lib = capi.lib()
    a = capi.Skeleton.constraints([("aim", 0, (1, 0, 0), (0, 1, 0))])
    fake = C.c_void_p(8)                                 # (a non-null handle that the checks must not follow)
    for rc in (lib.rt_skeleton_solve_ik(None, 1, a.ctypes.data_as(C.c_void_p)), lib.rt_skeleton_solve_ik(fake, 1, None)):
        assert rc == -1
        assert b"null" in lib.rt_last_error()


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program():
    out_dir = os.path.join(ROOT, "build_san")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "ik_sanitized")
    src = os.path.join(ROOT, "tests", "cpp", "ik_sanitized.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def run(program, mode, blob, n_cases, tmp_path):
    (tmp_path / "in.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "%d cases, 0 sanitizer reports" % n_cases in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return (tmp_path / "out.bin").read_bytes()


def constraint_lists():
    """(records, n, parents, posed, null): every refusal on its own, on the first, a middle and the last constraint; an argument's refusal
    before the state's; both orders of a dependent pair; 0, 33 and 2^32 - 1 constraints with no record to read; a null list; 32 independent
    constraints on the 65-joint comb; and 300 generated lists"""
    N, NAN = 0xFFFFFFFF, float("nan")
    comb = K.comb()
    z, x = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    out = []

    def add(records, parents=comb, posed=True, n=None, null=False):
        out.append((list(records), len(records) if n is None else n, np.asarray(parents, np.int32), posed, null))

    for n in (1, 2, 31, 32):
        add(K.comb_constraints(n, n))
        add(K.comb_constraints(n, n), posed=False)
    add([], n=0); add([], n=33); add([], n=N); add([], n=1, null=True)
    full = K.comb_constraints(32, 3)
    for at in (0, 15, 31):
        for bad in ((2, 3, z, x, 1.0), (N, 3, z, x, 1.0), (K.AIM, 65, z, x, 1.0), (K.TWO_BONE, N, z, x, 1.0), (K.TWO_BONE, 0, z, x, 1.0), (K.TWO_BONE, 1, z, x, 1.0),
                    (K.TWO_BONE, 49, z, x, 1.0), (K.AIM, 64, z, x, NAN), (K.TWO_BONE, 48, z, x, NAN), (K.AIM, 0, z, x, 1.0), (K.AIM, 1 + 3 * (at // 2), z, x, 1.0)):
            records = list(full)
            records[at] = bad
            add(records)
            add(records, posed=False)
    arm = [-1, 0, 1, 2, 3]                               # a chain: shoulder 1, elbow 2, hand 3, a finger 4
    add([(K.TWO_BONE, 3, z, x, 1.0), (K.AIM, 3, z, x, 1.0)], arm)                # an aim on the hand whose arm is solved: both orders
    add([(K.AIM, 3, z, x, 1.0), (K.TWO_BONE, 3, z, x, 1.0)], arm)
    add([(K.TWO_BONE, 3, z, x, 1.0), (K.AIM, 4, z, x, 1.0)], arm)                # the finger reads the arm
    add([(K.AIM, 4, z, x, 1.0), (K.TWO_BONE, 3, z, x, 1.0)], arm)                # the arm does not read the finger: but the finger reads the arm
    add([(K.AIM, 4, z, x, 1.0), (K.AIM, 0, z, x, 1.0)], arm)                     # an aim on the root is read by everything
    add([(K.AIM, 4, z, x, 1.0), (K.AIM, 4, z, x, 1.0)], arm)                     # two constraints that write the same joint
    add([(K.TWO_BONE, 3, z, x, 1.0), (K.TWO_BONE, 4, z, x, 1.0)], arm)           # overlapping chains
    add([(K.TWO_BONE, 2, z, x, 1.0)], arm); add([(K.TWO_BONE, 1, z, x, 1.0)], arm); add([(K.AIM, 0, z, x, np.inf)], [-1])
    add([(K.AIM, 7, z, x, NAN), (2, 0, z, x, 1.0)], arm, posed=False)            # the first constraint's refusal is named, before the state
    rng = np.random.default_rng(9)
    for _ in range(300):
        nj = int(rng.integers(1, 40))
        parents = S.hierarchy(("random", "roots", "chain", "star")[int(rng.integers(0, 4))], nj, int(rng.integers(0, 1000)))
        records = []
        for k in range(int(rng.integers(1, 5))):
            records.append((int(rng.choice([0, 1, 2], p=[0.5, 0.45, 0.05])), int(rng.integers(0, nj + 1)) if rng.uniform() < 0.1 else int(rng.integers(0, nj)), z, x,
                            float(rng.choice(K.WEIGHTS + (NAN,), p=[0.19] * 5 + [0.05]))))
        add(records, parents, posed=bool(rng.integers(0, 4)))
    return out


def test_constraint_lists_under_asan_ubsan(program, tmp_path):
    """the program's (code, indices) == the Python restatement's for every case; a list the validator must not read has no record behind its
    pointer, so that reading it is a report; no report"""
    cases = constraint_lists()
    blob = b""
    for records, n, parents, posed, null in cases:
        a = np.zeros(len(records), T.SKELETON_IK)
        for k, r in enumerate(records):
            a[k] = r
        blob += np.array([n, len(a), len(parents), int(posed), int(null)], np.uint32).tobytes() + a.tobytes() + parents.tobytes()
    got = np.frombuffer(run(program, "validate", blob, len(cases), tmp_path), np.uint32).reshape(-1, 4)
    assert len(got) == len(cases)
    seen = set()
    for (records, n, parents, posed, null), row in zip(cases, got):
        if null:
            want = (1, (0, 0, 0))
        elif n != len(records):
            want = (2, (0, 0, 0))
        else:
            want = K.validate(records, parents, posed)
        assert (int(row[0]), tuple(int(x) for x in row[1:])) == want, (records, parents.tolist(), posed, want)
        seen.add(want[0])
    assert seen == set(range(9)), "a refusal no case reaches"
    arm = [c for c in cases if len(c[2]) == 5 and len(c[0]) == 2][:2]
    assert [K.validate(c[0], c[2], True) for c in arm] == [(7, (1, 0, 3)), (7, (1, 0, 2))], "both orders of a dependent pair are refused"
    # (the arm reads its hand, which the aim writes; the aim, walked first, reads the elbow, which the arm writes)
    assert K.validate(K.comb_constraints(32, 3), K.comb(), True)[0] == 0 and len(K.comb()) == 65


def blob_of(b):
    n = len(b["kind"])
    words = np.zeros((n, 51), np.uint32)
    words[:, 0], words[:, 1] = b["kind"], b["has_parent"]
    floats = np.concatenate([b["tip"], b["mid"], b["root"], b["W"], b["target"], b["pole"], np.asarray(b["weight"], F)[:, None]], axis=1)
    assert floats.dtype == F and floats.shape == (n, 49)
    words[:, 2:] = np.ascontiguousarray(floats).view(np.uint32)
    return words.tobytes()


def test_the_solver_under_asan_ubsan_is_the_restatement_bit_for_bit(program, tmp_path):
    """rt_ik_solve compiled for the CPU gives the bytes of ik_cases.solve_batch over every family, each at the weights 0, 0.25, 1, -0.5,
    1.5; no report"""
    families = K.bitwise_families()
    assert len(families) >= 29
    for name, b in families.items():
        n = len(b["kind"])
        got = np.frombuffer(run(program, "solve", blob_of(b), n, tmp_path), F).reshape(n, 8)
        qa, qb = K.solve_batch(b)
        want = np.concatenate([qa, qb], axis=1)
        assert want.dtype == F
        differ = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
        assert len(differ) == 0, (name, differ[:5], got[differ[:2]], want[differ[:2]])


# ---- the restatement is what it states -----------------------------------------------------------------------------------------------------
def measured():
    """the largest errors of the restatement over the rigid families (ik_cases.rigid_families: committed seeds), as ik_bounds.json records
    them: tools of the test, not of the library -- python tests/test_skeleton_ik_abi.py rewrites the file"""
    out = {"cases": {}, "tip_over_chain_length": 0.0, "aim": 0.0, "wrong_side_over_chain_length": 0.0}
    for name, b in K.rigid_families().items():
        qa, qb = K.solve_batch(b)
        err, side = K.geometry_errors(b, qa, qb)
        out["cases"][name] = len(err)
        if side is None:
            out["aim"] = max(out["aim"], float(err.max()))
        else:
            out["tip_over_chain_length"] = max(out["tip_over_chain_length"], float(err.max()))
            out["wrong_side_over_chain_length"] = max(out["wrong_side_over_chain_length"], float(-side.min()))
    return out


def test_the_restatement_reaches_and_aims_in_float64():
    """over the rigid families -- uniform scale on a and b, ancestors from util.random_xforms, every case counted -- float64 forward
    kinematics of the solved fp32 pose puts the tip at the clamped target, the middle joint on the pole's side of the axis (it may stand
    on the axis, where the chain is straight or folded: not beyond it by more than rounding) and the aimed axis on the target's direction:
    within 4 x the errors recorded in tests/golden/ik_bounds.json, which were measured with this restatement over these seeds"""
    bounds = json.load(open(BOUNDS))
    families = K.rigid_families()
    assert {name: len(b["kind"]) for name, b in families.items()} == bounds["cases"], "no case may be left out of a rigid family"
    assert 0 < bounds["tip_over_chain_length"] < 1e-4 and 0 < bounds["aim"] < 1e-4 and 0 <= bounds["wrong_side_over_chain_length"] < 1e-4, "rounding, not fractions of the chain"
    for name, b in families.items():
        assert (b["weight"] == 1).all()
        trace = {}
        qa, qb = K.solve_batch(b, trace)
        err, side = K.geometry_errors(b, qa, qb)
        print(name, len(err), "largest error", err.max(), "" if side is None else "least side %g" % side.min())
        if side is None:
            assert trace["aim"].all()
            assert err.max() <= HOLD * bounds["aim"], name
        else:
            assert trace["solve"].all() and (trace["pole"] == 0).all(), name
            assert (trace["clamp"] == {"reachable": 0, "nearly_straight": 0, "out_of_reach": 1, "too_close": -1}[name]).all(), name
            assert err.max() <= HOLD * bounds["tip_over_chain_length"], name
            assert side.min() >= -HOLD * bounds["wrong_side_over_chain_length"], name
    # where the chain really bends, the middle joint stands well off the axis on the pole's side
    b = families["reachable"]
    _, side = K.geometry_errors(b, *K.solve_batch(b))
    assert side.min() > 0.05


def test_a_weight_of_zero_writes_the_normalised_input_and_one_the_solution():
    b = K.chains("reachable", 64, 7)
    zero = dict(b, weight=np.zeros(64, F))
    qa, qb = K.solve_batch(zero)
    A, Bq = K.B.normalised(b["root"][:, 3:7]), K.B.normalised(b["mid"][:, 3:7])
    assert qa.tobytes() == K.B.normalised(A).tobytes() and qb.tobytes() == K.B.normalised(Bq).tobytes()      # (the rule normalises what it blends: A once more)
    assert np.abs(qa - A).max() < 2e-7 and np.abs(qb - Bq).max() < 2e-7
    half = dict(b, weight=np.full(64, 0.5, F))
    e1, _ = K.geometry_errors(b, *K.solve_batch(b))
    eh, _ = K.geometry_errors(b, *K.solve_batch(half))
    assert e1.max() < 1e-4 and eh.min() > 1e-3, "half the weight stops short of the target"


def test_what_the_cases_are_there_for():
    """every path of the definition is taken by a case that names it"""
    d = K.degenerate()

    def paths(name):
        t = {}
        K.solve_batch(d[name], t)
        return t

    assert not paths("target_on_a")["solve"].any()
    assert (paths("pole_on_axis_first_fallback")["pole"] == 1).all() and paths("pole_on_axis_first_fallback")["solve"].all()
    assert (paths("pole_and_middle_on_axis_perp")["pole"] == 2).all() and paths("pole_and_middle_on_axis_perp")["solve"].all() and len(d["pole_and_middle_on_axis_perp"]["kind"]) == 3
    assert not paths("zero_first_bone")["solve"].any() and not paths("zero_second_bone")["solve"].any() and not paths("equal_bones_target_on_a")["solve"].any()
    assert paths("equal_bones_target_near_a")["solve"].all()
    assert paths("aim_parallel")["aim"].all() and not paths("aim_parallel")["half"].any()
    anti = paths("aim_antiparallel")
    assert anti["aim"].all() and anti["half"].all()
    u = K.unit(d["aim_antiparallel"]["pole"])[0]
    least = [int(np.argmin(np.abs(u[k]))) for k in range(3)]
    assert least == [0, 1, 2], "the half turn is taken about perp(u) with each choice of e"
    assert not paths("aim_zero_axis")["aim"].any() and not paths("aim_target_on_joint")["aim"].any()
    t = {}
    K.solve_batch(K.aims(64, 140), t)
    assert t["half"].sum() >= 1 and t["aim"].all()
    nf = K.non_finite()
    for name in ("target", "pole", "tip", "mid", "root", "W"):
        flat = nf[name].reshape(len(nf[name]), -1)
        assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any(), name
    fam = K.bitwise_families()
    assert all(set(np.unique(b["weight"]).tolist()) == set(float(F(w)) for w in K.WEIGHTS) for b in fam.values())
    assert fam["non_uniform_scales"]["root"][:, 7].tobytes() != fam["non_uniform_scales"]["root"][:, 8].tobytes()
    assert np.abs(np.linalg.norm(fam["non_unit_quaternions"]["root"][:, 3:7], axis=1) - 1).max() > 0.3


if __name__ == "__main__":
    with open(BOUNDS, "w") as f:
        json.dump(measured(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(BOUNDS).read())
