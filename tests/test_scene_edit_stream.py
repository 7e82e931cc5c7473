"""tests/scene_edit_sweep.py and tests/scene_edit_model.py without a GPU.  The sweep's plans are drawn on the shadow model alone, so what the seeds
and counts of tests/test_gpu_scene_edit_sweep.py cover can be said here: every operation kind succeeds and every refusable one is refused, an
update applies each non-empty subset of {transforms, masks, vertices, poses}, and the interleavings the sweep exists for all occur.  The GPU
classes are replaced by a stand-in that obeys a second shadow model, in the manner of tests/test_fuzz_stream.py, so that run() walks its
sequences; and the shadow model itself is held to hand-written outcomes, rule by rule (the numbers are those of scene_edit_model's docstring)."""
import numpy as np

import ik_cases
import scene_edit_model as M
import scene_edit_sweep as sweep
import skeleton_blend_cases
import skeleton_cases
import skin_cases
from deform_cases import grid_mesh, normals_of
from test_gpu_scene_edit_sweep import SEEDS, SEQUENCES

OK, INVALID, STATE = M.OK, M.ERR_INVALID_ARG, M.ERR_STATE
X = np.arange(12, dtype=np.float32)
Y = X + 100
# what the sweep required before morph targets and skeletons joined it: all of it stays required
OLD_KINDS = {"set_transform", "set_transforms", "set_mask", "set_masks", "add_model", "build", "update", "probe", "set_vertices", "set_positions",
             "recompute_normals", "set_skin", "clear_skin", "set_bones"}
OLD_REFUSABLE = ("set_transform", "set_transforms", "set_mask", "set_masks", "set_vertices", "set_positions", "set_skin", "set_bones", "update", "build")
OLD_SUBSETS = [frozenset(x) for x in (("transforms",), ("masks",), ("vertices",), ("transforms", "masks"), ("transforms", "vertices"), ("masks", "vertices"),
                                      ("transforms", "masks", "vertices"))]
OLD_EVENTS = ({("ok", k) for k in OLD_KINDS if k != "probe"} | {("refused", k) for k in OLD_REFUSABLE} | {("update applies", sub) for sub in OLD_SUBSETS}
              | {"no-op update", "all hidden refused with transforms and vertices pending, then applied", "hidden and shown again with no update in between",
                 "one instance set twice before one update", "an instance pending and of a changed model", "shared model: scene 0 updated before scene 1",
                 "shared model: scene 1 updated before scene 0", "shared model: one scene back by build, the other by update", "the visible count goes to 1",
                 "the visible count comes back from 1", "a single identity instance transformed", "a single instance back to the identity",
                 "a setter between add_model and build", "set_vertices after set_skin, then set_bones", "split references come and go"})


class ModelBackend:
    """the stand-in for the library and the oracle: a second shadow model takes the calls; a checkpoint compares what the readers return"""

    def __init__(self, plan, ctx, tally):
        self.world, self.tally = sweep.fresh_world(plan), tally

    def do(self, op):
        return sweep.apply_to_model(self.world, op)[0]

    def checkpoint(self, n, op, world):
        assert self.world.snapshot() == world.snapshot()
        assert self.world.scenes[op["s"]].readable()
        self.tally["checkpoints"] = self.tally.get("checkpoints", 0) + 1
        self.tally["frame checkpoints"] = self.tally.get("frame checkpoints", 0) + bool(op["frames"])
        assert self.world.readers() == world.readers()

    def close(self):
        pass


def world(n_instances=3, n_scenes=1, side=5):
    w = M.World()
    w.add_model(*grid_mesh(side))
    for _ in range(n_scenes):
        s = w.scenes[w.add_scene()]
        for k in range(n_instances):
            s.add_model(0, X * k if k else None)
    return w


# ---- the stream ---------------------------------------------------------------------------------------------------------------------------
def op_bytes(plan):
    return [sweep.describe(n, op) + repr(sorted((k, v.tobytes()) for k, v in op.items() if isinstance(v, np.ndarray))) for n, op in enumerate(plan.ops)]


def test_the_stream_of_a_seed_is_deterministic():
    a, b = sweep.plan_sequence(SEEDS[0], 1), sweep.plan_sequence(SEEDS[0], 1)
    assert op_bytes(a) == op_bytes(b) and a.kinds == b.kinds and a.options == b.options
    assert 30 <= len(a.ops) <= 75
    assert op_bytes(a) != op_bytes(sweep.plan_sequence(SEEDS[0], 2)) and op_bytes(a) != op_bytes(sweep.plan_sequence(SEEDS[1], 1))
    logs = []
    for _ in range(2):
        log, tally = [], {}
        assert sweep.run(2, SEEDS[0], None, tally=tally, log=log, backend=ModelBackend) is None
        logs.append((log, tally))
    assert logs[0] == logs[1] and logs[0][1]["sequences"] == 2


def test_a_wrong_return_code_is_reported_with_the_log():
    class Wrong(ModelBackend):
        def do(self, op):
            code = super().do(op)
            return OK if op["op"] == "update" and code != OK else code          # (a library that does not refuse an update)

    bad = sweep.run(SEQUENCES, SEEDS[0], None, backend=Wrong)
    assert bad and bad.startswith("MISMATCH seed %d sequence" % SEEDS[0]) and "the shadow model says -4" in bad
    assert "  0: " in bad and "update" in bad.splitlines()[-1]


def test_what_the_gpu_seeds_cover():
    events, tally, predicted = set(), {}, []
    for seed in SEEDS:
        per_seed = set()
        for it in range(SEQUENCES):
            plan = sweep.plan_sequence(seed, it)
            assert 2 <= len(plan.kinds) <= 3 and 1 <= len(plan.initial) <= 2 and len(plan.initial[0]) in sweep.COUNTS
            per_seed |= sweep.events_of(plan)
        predicted.append(sweep.per_seed_events() <= per_seed)
        events |= per_seed
        assert sweep.run(SEQUENCES, seed, None, tally=tally, backend=ModelBackend) is None
    missing = sweep.required_events() - events
    assert not missing, sorted(str(m) for m in missing)
    assert all(predicted)                # (the GPU test asserts the device-side tally of it for every seed)
    # every kind of call went through run() both ways, and the checkpoints the GPU test counts are there
    for kind in sweep.ALL_KINDS:
        assert tally.get("ok " + kind, 0) > 0 or kind == "probe", kind
    for kind in sweep.REFUSABLE + ("probe",):
        assert tally.get("refused " + kind, 0) > 0, kind
    assert tally["sequences"] == len(SEEDS) * SEQUENCES and tally["checkpoints"] >= 3 * tally["sequences"] and tally["frame checkpoints"] >= 2 * tally["sequences"]
    plans = [sweep.plan_sequence(seed, it) for seed in SEEDS for it in range(SEQUENCES)]
    assert any(p.options for p in plans) and not all(p.options for p in plans)
    assert any(p.shared for p in plans) and {k for p in plans for k in p.kinds} == set(sweep.KINDS)
    assert {p.normals for p in plans} == {True, False} and {p.n_joints for p in plans} == {sweep.N_BONES, sweep.WIDE_BONES}
    assert any(p.shared and p.kinds[0] == "character" for p in plans)       # the model that two scenes hold is, somewhere, the character
    assert sweep.required_events() >= OLD_EVENTS and set(sweep.ALL_KINDS) >= OLD_KINDS      # the list only grows
    # ... by rules 28 - 40: the seven kinds, every refusal and motif, every subset with "poses" in it, what the GPU test tallies
    new = {("ok", k) for k in ("set_transforms_mem", "attach", "detach", "skeleton_add_mask", "skeleton_clear_masks", "skeleton_set_blend",
                               "skeleton_solve_ik")}
    new |= {("refused", k, why) for k, why in sweep.REFUSALS} | {("motif", m) for m in sweep.MOTIFS} | {("update applies", sub) for sub in sweep.SUBSETS}
    assert len(sweep.SUBSETS) == 15 and len(sweep.MOTIFS) == 22 and len(sweep.REFUSALS) == 37 and new | set(sweep.TALLY_KEYS) <= sweep.required_events()
    assert set(sweep.TALLY_KEYS) <= sweep.per_seed_events()


# ---- mutants: a library with one rule of the morph targets and skeletons, or of attachments, blends and solves, wrong ---------------------
class Readers(ModelBackend):
    """a stand-in that is compared as the library is: through its return codes and, at a checkpoint, through what the readers return of the
    models, the skeletons and the checkpoint's own scene.  The rest pose and the morph base are seen by nobody."""

    def checkpoint(self, n, op, world):
        mine, theirs = self.world.readers(), world.readers()
        assert mine[:2] == theirs[:2] and mine[2][op["s"]] == theirs[2][op["s"]], "the readers differ"
        for a, b in zip(mine[2], theirs[2]):               # transforms() of every other scene that is fresh
            assert b[1] != M.FRESH or a[2] == b[2], "transforms() of another scene differ"

    def model(self, op):
        return self.world.models[op["m"]]


class RecapturesBase(Readers):
    """(a) set_skin recaptures the morph base"""

    def do(self, op):
        code = super().do(op)
        if op["op"] == "set_skin" and code == OK and self.model(op).morph is not None:
            self.model(op).morph["base"] = self.model(op).verts.copy()
        return code


class RestMorphMarksStale(Readers):
    """(b) a rest-pose morph marks the scenes stale"""

    def do(self, op):
        code = super().do(op)
        if op["op"] == "set_morph_weights" and code == OK and self.model(op).skin is not None:
            self.model(op)._changed()
        return code


class RestMorphWritesVertices(Readers):
    """(c) a rest-pose morph also writes the current vertices"""

    def do(self, op):
        code = super().do(op)
        if op["op"] == "set_morph_weights" and code == OK and self.model(op).skin is not None:
            self.model(op).verts[:] = self.model(op).skin["rest"]
        return code


class Accumulates(Readers):
    """(d) set_morph_weights works on the previous result instead of the base"""

    def do(self, op):
        code = super().do(op)
        if op["op"] == "set_morph_weights" and code == OK:
            m = self.model(op)
            m.morph["base"] = (m.verts if m.skin is None else m.skin["rest"]).copy()
        return code


class LatePalette(Readers):
    """(e) set_bones_from reads the palette when the scene is updated, not when it is called"""

    def __init__(self, *a):
        super().__init__(*a)
        self.late = {}

    def do(self, op):
        if op["op"] in ("update", "build"):
            for m, k in list(self.late.items()):
                mo, sk = self.world.models[m], self.world.skeletons[k]
                if id(mo) in self.world.scenes[op["s"]].pending_models:
                    if sk.palette is not None and mo.skin is not None and mo.skin["n_bones"] == len(sk.parents):
                        mo.verts[:] = skin_cases.skinned(mo.skin["rest"], mo.skin["bones"], mo.skin["weights"], sk.palette)
                    del self.late[m]
        code = super().do(op)
        if op["op"] == "set_bones_from" and code == OK:
            self.late[op["m"]] = op["k"]
        return code


class RefusalDropsTargets(Readers):
    """(f) a refused set_morph_targets drops the old targets"""

    def do(self, op):
        code = super().do(op)
        if op["op"] == "set_morph_targets" and code != OK:
            self.model(op).morph = None
        return code


class ClearSkinKeepsTheRedirection(Readers):
    """(g) after clear_skin, morph results still go to the old rest pose: nowhere that anything reads"""

    def __init__(self, *a):
        super().__init__(*a)
        self.ghost = set()

    def do(self, op):
        if op["op"] == "set_morph_weights" and op["m"] in self.ghost and self.model(op).morph is not None:
            return OK
        code = super().do(op)
        if op["op"] == "clear_skin" and code == OK:
            self.ghost.add(op["m"])
        if op["op"] == "set_skin" and code == OK:
            self.ghost.discard(op["m"])
        return code


# where each mutant may show: a return code of the call itself or of a probe, or the readers at a checkpoint.  (a), (c), (d) and (g) change
# only arrays that no reader returns.  With the producers of Planner.epilogue stubbed out every one of the seven is still reported for every
# seed, so none is caught ONLY because of the epilogue -- the seeds were chosen so -- but some reports come in a later sequence, the plans
# being other plans once the epilogue's draws are gone: (b) for seed 242, (d) for all three seeds, (f) for seed 46.
class Attachments(Readers):
    """the mutants of rules 28 - 40 look at the stand-in's own scene and skeleton"""

    def scene(self, op):
        return self.world.scenes[op["s"]]

    def skeleton(self, op):
        return self.world.skeletons[op["k"]]


class PoseAloneIsNoUpdate(Attachments):
    """(h) an update treats "only a pose since last time" as a no-op"""

    def do(self, op):
        if op["op"] == "update" and self.scene(op).state != M.UNBUILT and self.scene(op).pending() == {"poses"}:
            return OK
        return super().do(op)


class SolveDoesNotCount(Attachments):
    """(i) solve_ik does not count as a pose"""
    kind = "skeleton_solve_ik"

    def do(self, op):
        code = super().do(op)
        if op["op"] == self.kind and code == OK:
            self.skeleton(op).poses -= 1
        return code


class BlendDoesNotCount(SolveDoesNotCount):
    """(i) set_blend does not count as a pose"""
    kind = "skeleton_set_blend"


class DetachRestores(Attachments):
    """(j) detach restores the transform held before the attachment"""

    def __init__(self, *a):
        super().__init__(*a)
        self.held = {}

    def do(self, op):
        sc = self.scene(op) if op["op"] in ("attach", "detach") else None
        before = None if sc is None else (dict(sc.att), list(sc.inst))
        code = super().do(op)
        if code == OK and op["op"] == "attach":
            for i in range(op["first"], op["first"] + len(op["joints"])):
                if i not in before[0]:
                    self.held[(op["s"], i)] = before[1][i][1]
        if code == OK and op["op"] == "detach":
            for i in range(op["first"], op["first"] + op["count"]):
                if i in before[0]:
                    sc.inst[i] = (sc.inst[i][0], self.held.pop((op["s"], i)))
        return code


class AttachWritesAtOnce(Attachments):
    """(k) attach writes the composed transform at once"""

    def do(self, op):
        code = super().do(op)
        if code == OK and op["op"] == "attach" and self.skeleton(op).pose is not None:
            sc = self.scene(op)
            for i in range(op["first"], op["first"] + len(op["joints"])):
                a = sc.att[i]
                w = a["sk"].joints[a["joint"]]
                sc.inst[i] = (sc.inst[i][0], w.copy() if a["local"] is None else skeleton_cases.compose(w, a["local"])[0])
        return code


class ComposesFromTheJointsAtTheAttach(Attachments):
    """(l) an update composes from W as it was at the attach"""

    def do(self, op):
        code = super().do(op)
        if code == OK and op["op"] == "attach" and self.skeleton(op).pose is not None:
            for i in range(op["first"], op["first"] + len(op["joints"])):
                self.scene(op).att[i]["w0"] = self.skeleton(op).joints.copy()
        if code == OK and op["op"] in ("update", "build"):
            sc = self.scene(op)
            for i, a in sc.att.items():
                if a.get("w0") is not None:
                    w = a["w0"][a["joint"]]
                    sc.inst[i] = (sc.inst[i][0], w.copy() if a["local"] is None else skeleton_cases.compose(w, a["local"])[0])
        return code


class RefusedBlendStillPoses(Attachments):
    """(m) a refused blend still poses"""

    def do(self, op):
        code = super().do(op)
        sk = self.skeleton(op) if op["op"] == "skeleton_set_blend" else None
        if sk is not None and code != OK and sk.clips:
            sk.set_pose(skeleton_cases.sampled(sk.clips[0][0], sk.clips[0][1], -np.inf))
        return code


class BlendReadsThePoseBeforeTheSolve(Attachments):
    """(n) a blend on the current pose reads the pose before the preceding solve"""

    def __init__(self, *a):
        super().__init__(*a)
        self.before_solve = None

    def do(self, op):
        solve = op["op"] == "skeleton_solve_ik"
        held = self.skeleton(op).pose if solve else None
        code = super().do(op)
        if code == OK and op["op"] == "skeleton_set_blend" and op["layers"][0][0] is None and self.before_solve is not None:
            sk = self.skeleton(op)
            sk.poses -= 1
            sk.set_pose(skeleton_blend_cases.blended(sk.clips, sk.masks, op["layers"], current=self.before_solve))
        if code == OK and op["op"] in sweep.POSE_OPS:
            self.before_solve = held.copy() if solve and held is not None else None
        if code == OK and op["op"] == "set_bones_from" and op.get("destroy"):
            self.before_solve = None
        return code


class FollowsTheReplacement(Attachments):
    """(o) instances of a destroyed skeleton follow its replacement"""

    def do(self, op):
        old = self.world.skeletons[op["k"]] if op["op"] == "set_bones_from" else None
        code = super().do(op)
        if old is not None and self.world.skeletons[op["k"]] is not old:
            for sc in self.world.scenes:
                for a in sc.att.values():
                    if a["sk"] is old:
                        a["sk"], a["seen"] = self.world.skeletons[op["k"]], None
        return code


class SetterOverAnAttachedRange(Attachments):
    """(p) a transform setter over an attached range is accepted and wins the next update"""

    def __init__(self, *a):
        super().__init__(*a)
        self.won = {}                                      # (scene, instance) -> the floats a setter gave an attached instance

    def do(self, op):
        code = super().do(op)
        sc = self.scene(op) if op["op"] in sweep.SCENE_OPS else None
        if code != OK and op["op"] in ("set_transform", "set_transforms", "set_transforms_mem"):
            first, n = (op["i"], 1) if op["op"] == "set_transform" else (op["first"], len(op["xs"]))
            if first + n <= len(sc.inst):                    # refused for the attachment alone: taken, as if nobody were attached there
                held = {i: sc.att.pop(i) for i in range(first, first + n) if i in sc.att}
                code = super().do(op)
                for i, a in held.items():
                    sc.att[i] = a
                    self.won[(op["s"], i)] = sc.inst[i][1]
        if code == OK and op["op"] in ("update", "build"):  # ... and the joint does not take the instance back
            for (s, i) in [k for k in self.won if k[0] == op["s"]]:
                sc.inst[i] = (sc.inst[i][0], self.won.pop((s, i)))
        return code


class RefusedUpdateRecordsThePose(Attachments):
    """(q) a refused update (nothing visible, or an unposed attachment) still records the pose as applied, so the pose is lost"""

    def do(self, op):
        code = super().do(op)
        if code != OK and op["op"] in ("update", "build") and self.scene(op).state != M.UNBUILT:
            for a in self.scene(op).att.values():
                a["seen"] = a["sk"].poses
        return code


class ReattachKeepsTheLocal(Attachments):
    """(r) re-attaching without locals keeps the old local"""

    def do(self, op):
        old = {i: a["local"] for i, a in self.scene(op).att.items()} if op["op"] == "attach" else {}
        code = super().do(op)
        if code == OK and op["op"] == "attach" and op["locals"] is None:
            for i in range(op["first"], op["first"] + len(op["joints"])):
                if old.get(i) is not None:
                    self.scene(op).att[i]["local"] = old[i]
        return code


MUTANTS = [(RecapturesBase, ("update", "build")), (RestMorphMarksStale, ("probe",)), (RestMorphWritesVertices, ("update", "build")),
           (Accumulates, ("update", "build")), (LatePalette, ("update", "build")), (RefusalDropsTargets, ("set_morph_weights", "update", "build")),
           (ClearSkinKeepsTheRedirection, ("probe", "update", "build")),
           # rules 28 - 40.  (h), (i), (l), (q) and (r) leave an attached instance where it was or put it elsewhere: transforms() at the update
           # itself; (j) and (k) change floats that the next update or build of the scene shows; (m) and (n) change the skeleton's pose: every
           # checkpoint reads it, and a call that needs a pose (or must be refused for want of one) answers otherwise; (o): the update is
           # refused for the replacement's missing pose, or moves the instances; (p): the setter's code, before any update could show more
           (PoseAloneIsNoUpdate, ("update",)), (SolveDoesNotCount, ("update",)), (BlendDoesNotCount, ("update",)), (DetachRestores, ("update", "build")),
           (AttachWritesAtOnce, ("update", "build")), (ComposesFromTheJointsAtTheAttach, ("update", "build")),
           (RefusedBlendStillPoses, ("update", "build", "set_bones_from", "skeleton_set_blend", "skeleton_solve_ik")),
           (BlendReadsThePoseBeforeTheSolve, ("update", "build")), (FollowsTheReplacement, ("update", "build")),
           (SetterOverAnAttachedRange, ("set_transform", "set_transforms", "set_transforms_mem")), (RefusedUpdateRecordsThePose, ("update", "build")),
           (ReattachKeepsTheLocal, ("update", "build"))]


def test_every_mutant_of_the_new_rules_is_reported():
    for mutant, where in MUTANTS:
        for seed in SEEDS:
            bad = sweep.run(SEQUENCES, seed, None, backend=mutant)
            assert bad and bad.startswith("MISMATCH seed %d sequence" % seed), (mutant.__doc__, seed)
            last = bad.splitlines()[-1]
            assert last.split(":", 1)[1].split()[0] in where, (mutant.__doc__, seed, last)
    for seed in SEEDS:                                     # the stand-in with every rule right is not
        assert sweep.run(SEQUENCES, seed, None, backend=Readers) is None


# ---- the shadow model, rule by rule -------------------------------------------------------------------------------------------------------------
def one_target(m, entries, normals=None):
    """one target over the model: entries [(vertex, (dx, dy, dz))]"""
    return m.set_morph_targets([0, len(entries)], [v for v, _ in entries], np.array([d for _, d in entries], np.float32), normals)


def moved(verts, **by):
    """a copy of verts with float32 additions applied: moved(v, x=2.0) or moved(v, v2=(1, 0, 0))"""
    out = verts.copy()
    for key, d in by.items():
        if key in "xyz":
            out["position"][:, "xyz".index(key)] += np.float32(d)
        else:
            out["position"][int(key[1:])] += np.asarray(d, np.float32)
    return out


def shift_x(n_bones=1, by=2.0):
    p = skin_cases.identity_palette(n_bones)
    p[:, 3] = by
    return p


def test_morph_weights_without_a_skin_write_the_vertices_from_the_base():
    w = world(side=4)
    s, m = w.scenes[0], w.models[0]
    s.build()
    base = m.verts.copy()
    assert m.set_morph_weights([1.0]) == STATE and m.morph_query() == (0, 0, False)                 # rule 20
    assert one_target(m, [(2, (1, 0, 0)), (5, (0, 2, 0))]) == OK and m.morph_query() == (1, 2, False)
    assert s.state == M.FRESH and m.geometry().tobytes() == base.tobytes()                          # rule 17
    assert m.set_morph_weights([0.5]) == OK and s.state == M.STALE                                  # rule 21
    assert m.geometry().tobytes() == moved(base, v2=(0.5, 0, 0), v5=(0, 1, 0)).tobytes()
    assert s.update() == (OK, frozenset(["vertices"]))
    assert m.set_morph_weights([2.0]) == OK                                                         # from the base, not from the last result
    assert m.geometry().tobytes() == moved(base, v2=(2, 0, 0), v5=(0, 4, 0)).tobytes()
    assert m.set_positions(7, [[9, 9, 9]]) == OK and m.recompute_normals() == OK                    # rule 24: the current vertices, not the base
    assert m.set_morph_weights([1.0]) == OK                                                         # the whole mesh: vertex 7 and the normals too
    assert m.geometry().tobytes() == moved(base, v2=(1, 0, 0), v5=(0, 2, 0)).tobytes()
    s.update()
    last = m.geometry().copy()
    assert m.clear_morph_targets() == OK and s.state == M.FRESH and m.geometry().tobytes() == last.tobytes()        # rule 19
    assert m.set_morph_weights([1.0]) == STATE


def test_with_a_skin_the_weights_write_the_rest_pose_and_no_scene_goes_stale():
    w = world(side=4)
    s, m = w.scenes[0], w.models[0]
    s.build()
    R = m.verts.copy()
    m.set_skin(np.zeros((16, 1), np.uint32), np.ones((16, 1), np.float32), 1)
    assert one_target(m, [(2, (1, 0, 0))]) == OK                                                    # rule 17: the base is the rest pose, R
    assert m.set_morph_weights([1.0]) == OK and s.state == M.FRESH and s.readable()                 # rule 22
    assert m.geometry().tobytes() == R.tobytes() and m.skin["rest"].tobytes() == moved(R, v2=(1, 0, 0)).tobytes()
    assert m.set_bones(shift_x()) == OK and s.state == M.STALE
    P = moved(moved(R, v2=(1, 0, 0)), x=2.0)
    assert m.geometry().tobytes() == P.tobytes()                                                    # the pose of the morphed rest pose
    s.update()
    m.set_skin(np.zeros((16, 1), np.uint32), np.ones((16, 1), np.float32), 1)                        # rule 23: the rest pose is P now, the base still R
    assert m.skin["rest"].tobytes() == P.tobytes() and m.morph["base"].tobytes() == R.tobytes()
    assert m.set_morph_weights([0.0]) == OK and m.skin["rest"].tobytes() == R.tobytes() and s.state == M.FRESH
    m.set_bones(shift_x())
    assert m.geometry().tobytes() == moved(R, x=2.0).tobytes()
    s.update()
    assert m.clear_skin() == OK and m.set_morph_weights([3.0]) == OK and s.state == M.STALE         # rule 23: to the vertices again, from R
    assert m.geometry().tobytes() == moved(R, v2=(3, 0, 0)).tobytes()


def test_targets_before_the_skin_keep_the_base_they_captured():
    w = world(side=4)
    s, m = w.scenes[0], w.models[0]
    s.build()
    A = m.verts.copy()
    one_target(m, [(3, (0, 0, 1))])                                                                 # the base is A
    assert m.set_positions(0, [[5, 5, 5]]) == OK
    C = m.verts.copy()
    m.set_skin(np.zeros((16, 1), np.uint32), np.ones((16, 1), np.float32), 1)                        # the rest pose is C
    s.update()
    assert m.skin["rest"].tobytes() == C.tobytes() and m.morph["base"].tobytes() == A.tobytes()      # rule 23
    assert m.set_morph_weights([1.0]) == OK and s.state == M.FRESH and m.geometry().tobytes() == C.tobytes()
    m.set_bones(shift_x(by=-1.0))
    assert m.geometry().tobytes() == moved(moved(A, v3=(0, 0, 1)), x=-1.0).tobytes()                # vertex 0 is A's again: the rest pose was overwritten whole
    one_target(m, [(3, (0, 0, 1))])                                                                 # set again: the base is the rest pose as the weights left it
    assert m.set_morph_weights([1.0]) == OK and m.skin["rest"].tobytes() == moved(moved(A, v3=(0, 0, 1)), v3=(0, 0, 1)).tobytes()


def test_targets_that_are_refused_leave_the_old_ones():
    w = world(side=4)
    s, m = w.scenes[0], w.models[0]
    s.build()
    assert one_target(m, [(2, (1, 0, 0)), (5, (0, 2, 0))], np.ones((2, 3), np.float32)) == OK and m.morph_query() == (1, 2, True)
    m.set_positions(1, [[7, 7, 7]])
    before = w.snapshot()
    d = np.zeros((4, 3), np.float32)
    for off, idx in (([1, 4], [0, 1, 2, 3]), ([0, 3, 2, 4], [0, 1, 2, 3]), ([0, 2, 4], [0, 1, 2, 16]), ([0, 2, 4], [0, 1, 3, 3]), ([0, 2, 4], [0, 1, 3, 2])):
        assert m.set_morph_targets(off, idx, d) == INVALID and w.snapshot() == before, (off, idx)    # rules 18, 10
    assert m.set_morph_targets(np.zeros(65538, np.uint32), [], d[:0]) == INVALID and w.snapshot() == before
    assert m.set_morph_targets(np.zeros(65537, np.uint32), [], d[:0]) == OK and m.morph_query() == (65536, 0, False)
    assert m.morph["base"][1]["position"].tolist() == [7, 7, 7]                                      # replaced: the base is captured anew


def two_joints():
    sk = M.Skeleton([-1, 0], skin_cases.identity_palette(2))
    trs = np.zeros((2, 10), np.float32)
    trs[:, 6] = 1                                           # q = (0, 0, 0, 1)
    trs[:, 7:10] = 1
    trs[0, 0], trs[1, 1] = 1, 2                             # the root one along x, its child two along y
    return sk, trs


def translation(x, y, z):
    return [1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z]


def test_a_skeleton_poses_samples_and_refuses():
    w = world(side=4)
    s, m = w.scenes[0], w.models[0]
    s.build()
    sk, trs = two_joints()
    w.skeletons.append(sk)
    before = w.snapshot()
    assert sk.set_time(0, 0.0) == STATE and w.snapshot() == before                                  # rule 26: no clip yet
    assert sk.readers() is None
    assert sk.set_pose(trs) == OK and s.state == M.FRESH and m.geometry().tobytes() == before[0][0][0]       # rule 25
    assert sk.joints.tolist() == [translation(1, 0, 0), translation(1, 2, 0)] and sk.palette.tolist() == sk.joints.tolist()
    far = trs.copy()
    far[0, 0] = 3
    keys = np.stack([trs, far])
    before = w.snapshot()
    for times in ([0, np.nan], [0, np.inf], [-np.inf, 0], [1, 1], [1, 0], []):
        assert sk.add_clip(np.array(times, np.float32), keys[:len(times)]) == INVALID and w.snapshot() == before
    assert sk.add_clip([0, 1], keys) == OK and len(sk.clips) == 1 and s.state == M.FRESH
    before = w.snapshot()
    assert sk.set_time(0, np.nan) == INVALID and sk.set_time(1, 0.5) == STATE and w.snapshot() == before
    assert sk.set_time(0, 0.5) == OK and sk.joints.tolist() == [translation(2, 0, 0), translation(2, 2, 0)] and sk.pose[0, 0] == 2
    assert sk.set_time(0, -3.0) == OK and sk.joints[0].tolist() == translation(1, 0, 0)              # before the first key
    assert sk.set_time(0, 1.0) == OK and sk.joints[1].tolist() == translation(3, 2, 0)               # on the last key
    assert sk.set_time(0, np.inf) == OK and sk.joints[1].tolist() == translation(3, 2, 0)
    assert sk.clear_clips() == OK and sk.pose[0, 0] == 3 and sk.set_time(0, 0.0) == STATE            # the pose stays; no clip 0 any more
    assert sk.add_clip([5], keys[:1]) == OK and sk.set_time(0, 99.0) == OK and sk.pose[0, 0] == 1    # ids start at 0 again; one key: that key
    assert s.state == M.FRESH and m.geometry().tobytes() == before[0][0][0]


def test_set_bones_from_takes_the_palette_as_it_is_at_the_call():
    w = world(side=4)
    s, m = w.scenes[0], w.models[0]
    s.build()
    R = m.verts.copy()
    sk, trs = two_joints()
    w.skeletons.append(sk)
    bones = np.zeros((16, 1), np.uint32)
    bones[8:] = 1
    before = w.snapshot()
    assert m.set_bones_from(sk) == STATE                                                            # rule 27: no pose, and no skin either
    sk.set_pose(trs)
    assert m.set_bones_from(sk) == STATE                                                            # no skin
    m.set_skin(np.zeros((16, 1), np.uint32), np.ones((16, 1), np.float32), 3)
    assert m.set_bones_from(sk) == STATE and s.state == M.FRESH and m.geometry().tobytes() == R.tobytes()      # three bones, two joints
    m.set_skin(bones, np.ones((16, 1), np.float32), 2)
    fresh = M.Skeleton([-1, 0], skin_cases.identity_palette(2))
    assert m.set_bones_from(fresh) == STATE                                                         # before that skeleton's first pose
    assert m.set_bones_from(sk) == OK and s.state == M.STALE
    want = R.copy()
    want["position"][:, 0] += np.float32(1)                 # both joints stand one along x,
    want["position"][8:, 1] += np.float32(2)                # the child two along y
    assert m.geometry().tobytes() == want.tobytes()
    trs[0, 0] = 50
    assert sk.set_pose(trs) == OK and m.geometry().tobytes() == want.tobytes()                      # a later pose reaches no vertex
    assert s.update() == (OK, frozenset(["vertices"])) and m.geometry().tobytes() == want.tobytes()


# (rules 28 - 40)
def row(x, y, z):
    return np.array(translation(x, y, z), np.float32)


def attached_world(n_instances=3, n_scenes=1):
    """world() and a skeleton of two joints in slot 0: posed with `trs`, the root stands at (1, 0, 0) and its child at (1, 2, 0)"""
    w = world(n_instances, n_scenes)
    w.add_skeleton([-1, 0], skin_cases.identity_palette(2))
    return w, w.scenes[0], w.skeletons[0], two_joints()[1]


def test_transforms_from_device_memory_are_the_host_setter():
    w = world()
    s = w.scenes[0]
    s.build()
    assert s.set_transforms_mem(1, [Y, None], "device") == OK and s.state == M.STALE and s.pending() == {"transforms"}           # rule 28
    assert s.transforms().tolist() == [M.IDENTITY_FLOATS.tolist(), Y.tolist(), M.IDENTITY_FLOATS.tolist()]
    before = w.snapshot()
    assert s.set_transforms_mem(2, [Y, Y], "device") == STATE and s.set_transforms_mem(4, [], "host") == STATE and w.snapshot() == before
    assert s.set_transforms_mem(3, [], "device") == OK and w.snapshot() == before
    assert s.update() == (OK, frozenset(["transforms"])) and s.transforms()[1].tolist() == Y.tolist()
    assert s.set_transforms_mem(0, [Y], "host") == OK and s.transforms()[0].tolist() == Y.tolist() and s.state == M.STALE


def test_attach_refuses_the_range_before_the_joint():
    w, s, sk, trs = attached_world()
    s.build()
    before = w.snapshot()
    assert s.attach(2, sk, [0, 1]) == STATE and s.attach(4, sk, []) == STATE                        # rule 29: beyond the instances
    assert s.attach(0, sk, [2]) == INVALID and s.attach(1, sk, [0, 2], [X, X]) == INVALID           # a joint >= n_joints
    assert s.attach(2, sk, [0, 5]) == STATE                                                         # both: the range wins
    assert s.attach(3, sk, []) == OK and s.attach(0, sk, []) == OK                                  # count 0
    assert w.snapshot() == before and s.state == M.FRESH and s.attachment(0) is None                # rule 10


def test_an_attached_instance_follows_its_joint_at_the_update():
    w, s, sk, trs = attached_world()
    s.build()
    assert s.attach(1, sk, [1]) == OK and s.state == M.STALE and s.pending() == {"transforms"}      # rule 30: pending, and no float changed
    assert s.transforms()[1].tolist() == X.tolist() and s.attachment(1) == (sk, 1) and s.attachment(0) is None
    before = w.snapshot()
    assert s.update() == (STATE, None) and s.build() == (STATE, None) and w.snapshot() == before    # rule 35: no pose yet
    assert sk.set_pose(trs) == OK and s.state == M.STALE and s.pending() == {"transforms", "poses"}
    assert s.update() == (OK, frozenset(["transforms", "poses"]))
    assert s.transforms()[1].tobytes() == row(1, 2, 0).tobytes() and s.transforms()[2].tolist() == (X * 2).tolist()     # rule 34: W bit for bit
    far = trs.copy()
    far[0, 0] = 3
    assert sk.set_pose(far) == OK and s.state == M.FRESH and s.readable() and s.pending() == {"poses"}      # rule 33
    assert s.transforms()[1].tobytes() == row(1, 2, 0).tobytes()
    assert s.update() == (OK, frozenset(["poses"])) and s.transforms()[1].tobytes() == row(3, 2, 0).tobytes()
    assert s.update() == (OK, frozenset())                                                          # rule 11: counted once
    assert s.attach(1, sk, [0], [row(0, 0, 5)]) == OK and s.transforms()[1].tobytes() == row(3, 2, 0).tobytes()       # attached again: replaced
    assert s.update() == (OK, frozenset(["transforms", "poses"])) and s.transforms()[1].tobytes() == row(3, 0, 5).tobytes() and s.attachment(1) == (sk, 0)
    assert s.attach(1, sk, [0]) == OK and s.update()[0] == OK and s.transforms()[1].tobytes() == row(3, 0, 0).tobytes()  # without locals: the local is gone


def test_an_attachment_on_an_unbuilt_scene_only_stores():
    w, s, sk, trs = attached_world()
    assert s.attach(0, sk, [0, 1], [row(0, 0, 1), row(0, 0, 2)]) == OK and s.state == M.UNBUILT and not s.pending()         # rule 30
    assert s.transforms()[0].tolist() == M.IDENTITY_FLOATS.tolist()
    assert s.build() == (STATE, None)                                                               # rule 35
    sk.set_pose(trs)
    assert s.build()[0] == OK and s.transforms()[:2].tolist() == [row(1, 0, 1).tolist(), row(1, 2, 2).tolist()]


def test_the_joints_are_those_at_the_update_not_at_the_attach():
    w, s, sk, trs = attached_world()
    s.build()
    sk.set_pose(trs)
    s.attach(2, sk, [0])
    far = trs.copy()
    far[0, 0] = 7
    sk.set_pose(far)
    assert s.update()[0] == OK and s.transforms()[2].tobytes() == row(7, 0, 0).tobytes()            # rule 34


def test_a_composed_identity_is_the_identity():
    w, s, sk, trs = attached_world(n_instances=1)
    s.build()
    s.attach(0, sk, [0])
    trs[0, 0] = 0
    sk.set_pose(trs)
    assert s.update()[0] == OK and s.inst[0][1] is not None and M.is_identity(s.inst[0][1])         # rule 34
    sk.set_pose(two_joints()[1])
    assert s.update()[0] == OK and not M.is_identity(s.inst[0][1])


def test_transform_setters_over_an_attached_range_are_refused():
    w, s, sk, trs = attached_world()
    s.build()
    s.attach(1, sk, [0])
    before = w.snapshot()
    for call in (lambda: s.set_transform(1, Y), lambda: s.set_transforms(0, [Y, Y]), lambda: s.set_transforms(1, [Y, Y]),
                 lambda: s.set_transforms_mem(1, [Y], "device"), lambda: s.set_transforms_mem(0, [Y, Y, Y], "host")):
        assert call() == STATE and w.snapshot() == before                                           # rule 31
    assert s.set_transforms(1, []) == OK and w.snapshot() == before                                 # (count 0 holds nobody)
    assert s.set_transform(0, Y) == OK and s.set_transforms_mem(2, [Y], "device") == OK


def test_detach_keeps_what_the_last_update_gave():
    w, s, sk, trs = attached_world()
    s.build()
    s.attach(1, sk, [1])
    sk.set_pose(trs)
    s.update()
    far = trs.copy()
    far[0, 0] = 3
    sk.set_pose(far)
    before = w.snapshot()
    assert s.detach(2, 2) == STATE and s.detach(4, 0) == STATE and w.snapshot() == before           # rule 32
    assert s.detach(0, 1) == OK and s.detach(3, 0) == OK and w.snapshot() == before                 # nobody attached there: a no-op
    assert s.detach(0, 3) == OK and s.attachment(1) is None and s.state == M.FRESH and not s.pending()
    assert s.update() == (OK, frozenset()) and s.transforms()[1].tobytes() == row(1, 2, 0).tobytes()        # the first pose, not the second
    assert s.set_transform(1, Y) == OK                                                              # ... and the setters take it again
    s.update()
    assert s.attach(2, sk, [0]) == OK and s.detach(2, 1) == OK                                      # let go before any update: the floats never changed
    assert s.update()[0] == OK and s.transforms()[2].tolist() == (X * 2).tolist()


def test_a_refused_update_keeps_the_pose_pending_too():
    w, s, sk, trs = attached_world()
    s.build()
    s.attach(1, sk, [0])
    sk.set_pose(trs)
    s.update()
    s.set_masks(0, [0, 0, 0])
    far = trs.copy()
    far[0, 0] = 3
    sk.set_pose(far)
    before = w.snapshot()
    assert s.update() == (STATE, None) and w.snapshot() == before                                   # rules 12, 35
    s.set_mask(0, 1)
    assert s.update() == (OK, frozenset(["masks", "poses"])) and s.transforms()[1].tobytes() == row(3, 0, 0).tobytes()      # the hidden instance too


def test_a_binding_holds_the_skeleton_not_its_slot():
    w, a, sk, trs = attached_world(n_scenes=2)
    b = w.scenes[1]
    for s in (a, b):
        s.build()
        s.attach(1, sk, [0])
    sk.set_pose(trs)
    assert a.update()[0] == OK and b.pending() == {"transforms", "poses"} and b.update()[0] == OK
    far = trs.copy()
    far[0, 0] = 3
    sk.set_pose(far)                                                                                # one pose, two scenes: each keeps its own record
    assert b.update() == (OK, frozenset(["poses"])) and a.pending() == {"poses"} and a.transforms()[1].tobytes() == row(1, 0, 0).tobytes()
    assert a.update() == (OK, frozenset(["poses"])) and a.transforms()[1].tobytes() == row(3, 0, 0).tobytes()
    w.replace_skeleton(0)                                                                           # rule 36: destroyed; a new one in the slot
    new = w.skeletons[0]
    assert new is not sk and new.pose is None and new.uid != sk.uid and a.attachment(1) == (sk, 0)
    new.set_pose(trs)
    assert a.pending() == frozenset() and a.update() == (OK, frozenset()) and a.transforms()[1].tobytes() == row(3, 0, 0).tobytes()
    assert a.attach(2, new, [1]) == OK and a.update()[0] == OK and a.transforms()[2].tobytes() == row(1, 2, 0).tobytes()


def test_masks_and_blends():
    B = skeleton_blend_cases
    w, s, sk, trs = attached_world()
    far = trs.copy()
    far[0, 0] = 3
    assert sk.add_clip([0, 1], np.stack([trs, far])) == OK
    assert sk.num_masks() == 0 and sk.add_mask([1, 0]) == OK and sk.num_masks() == 1                # rule 37
    assert sk.clear_masks() == OK and sk.num_masks() == 0 and sk.add_mask([1, 0]) == OK and sk.add_mask([0, 1]) == OK and sk.num_masks() == 2
    base, nan = (0, 0.0, 1.0, None, B.BLEND), float("nan")
    assert sk.set_blend([(None, 0.0, 1.0, None, B.BLEND)]) == STATE and sk.readers() is None and sk.poses == 0      # rule 38: no pose to be current
    assert sk.set_blend([(None, 0.0, 1.0, None, B.BLEND), (0, nan, 1.0, None, B.BLEND)]) == INVALID                 # the first group first
    assert sk.set_blend([base]) == OK and sk.pose.tobytes() == trs.tobytes() and sk.poses == 1                      # one layer: set_time
    before = w.snapshot()
    for layers, code in (([base] * 9, INVALID), ([], INVALID), ([(0, 0.0, 1.0, None, B.ADDITIVE)], INVALID), ([base, (None, 0.0, 1.0, None, B.BLEND)], INVALID),
                         ([base, (0, nan, 1.0, None, B.BLEND)], INVALID), ([(1, 0.0, 1.0, None, B.BLEND)], STATE), ([base, (0, 0.0, 1.0, 2, B.BLEND)], STATE),
                         ([(1, 0.0, 1.0, None, B.BLEND), (0, nan, 1.0, None, B.BLEND)], INVALID)):
        assert sk.set_blend(layers) == code and w.snapshot() == before, layers                      # rules 38, 40: a refusal poses nothing, counts nothing
    assert sk.set_blend([(None, 0.0, 1.0, None, B.BLEND), (0, 1.0, 0.5, 0, B.BLEND)]) == OK and sk.poses == 2       # the current pose, half way to the last key
    assert sk.pose[0, 0] == 2 and sk.pose[1].tobytes() == trs[1].tobytes()                          # where the mask is 1; the child's weight is 0
    assert sk.joints.tolist() == [translation(2, 0, 0), translation(2, 2, 0)] and sk.num_masks() == 2


def test_solve_ik_refuses_and_solves():
    w, s, sk, trs = attached_world()
    aim = (ik_cases.AIM, 0, (0.0, 2.0, 0.0), (1.0, 0.0, 0.0), 1.0)
    assert sk.solve_ik([aim]) == STATE and sk.poses == 0                                            # rule 39: no pose yet
    assert sk.solve_ik([aim[:4] + (float("nan"),)]) == INVALID                                      # ... but the first group is held to first
    trs[0, 0] = 0
    sk.set_pose(trs)
    before = w.snapshot()
    for cs in ([aim] * 33, [], [(7,) + aim[1:]], [(ik_cases.AIM, 2) + aim[2:]], [(ik_cases.TWO_BONE, 1) + aim[2:]], [aim[:4] + (float("nan"),)],
               [aim, aim], [aim, (ik_cases.AIM, 1) + aim[2:]]):
        assert sk.solve_ik(cs) == INVALID and w.snapshot() == before, cs                            # rules 39, 40
    want = ik_cases.solved(sk.parents, sk.pose, sk.joints, [aim])
    assert sk.solve_ik([aim]) == OK and sk.poses == 2 and sk.pose.tobytes() == want.tobytes()
    assert sk.pose[:, [0, 1, 2, 7, 8, 9]].tobytes() == trs[:, [0, 1, 2, 7, 8, 9]].tobytes() and sk.pose[1].tobytes() == trs[1].tobytes()
    assert np.allclose(sk.joints[0].reshape(3, 4)[:, 0], [0, 1, 0], atol=1e-6)                      # the root's +x now points at the target


def test_every_producer_counts_as_one_pose():
    w, s, sk, trs = attached_world()
    s.build()
    s.attach(1, sk, [0])
    sk.add_clip([0, 1], np.stack([trs, trs]))
    B = skeleton_blend_cases
    for n, pose in enumerate((lambda: sk.set_pose(trs), lambda: sk.set_time(0, 0.5), lambda: sk.set_blend([(0, 0.5, 1.0, None, B.BLEND)]),
                              lambda: sk.solve_ik([(ik_cases.AIM, 1, (0.0, 2.0, 0.0), (1.0, 0.0, 0.0), 0.25)]))):
        assert pose() == OK and sk.poses == n + 1 and "poses" in s.pending()                        # rule 40
        assert s.update()[0] == OK and s.update() == (OK, frozenset())
    assert sk.set_time(0, float("nan")) == INVALID and sk.set_time(3, 0.0) == STATE and sk.solve_ik([]) == INVALID and sk.set_blend([]) == INVALID
    assert sk.poses == 4 and s.update() == (OK, frozenset())                                        # a refused one counts as none


# (rules 1 - 16)
def test_setters_before_the_first_build_only_store():
    w = world()
    s = w.scenes[0]
    assert s.set_transform(1, Y) == OK and s.set_mask(2, 0) == OK and w.models[0].set_positions(0, np.zeros((2, 3))) == OK
    assert s.state == M.UNBUILT and not s.pending()                      # rule 1
    assert s.update() == (STATE, None)
    assert s.build() == (OK, frozenset()) and s.state == M.FRESH and s.applied_vis == [0, 1]
    assert s.inst[1][1].tolist() == Y.tolist() and s.masks == [0xFF, 0xFF, 0]


def test_a_transform_makes_stale_and_the_second_update_is_a_no_op():
    w = world()
    s = w.scenes[0]
    s.build()
    assert s.set_transforms(1, [Y, None]) == OK and s.state == M.STALE and not s.readable()         # rules 2, 13
    assert s.update() == (OK, frozenset(["transforms"])) and s.readable()
    assert s.inst[2][1] is None
    before = w.snapshot()
    assert s.update() == (OK, frozenset()) and w.snapshot() == before                               # rule 11


def test_masks_that_change_no_visibility_leave_the_scene_fresh():
    w = world()
    s = w.scenes[0]
    s.set_mask(1, 0)
    s.build()
    assert s.set_masks(0, [0x01, 0, 0x80]) == OK and s.state == M.FRESH and s.masks == [0x01, 0, 0x80]      # rule 3
    assert s.update() == (OK, frozenset())
    assert s.set_mask(1, 0x02) == OK and s.state == M.STALE
    assert s.set_mask(1, 0) == OK and s.state == M.STALE                 # hidden again with no update in between: still an update to make
    assert s.update() == (OK, frozenset(["masks"])) and s.applied_vis == [0, 2]


def test_setters_with_no_count_and_out_of_range_setters():
    w = world()
    s, m = w.scenes[0], w.models[0]
    s.build()
    before = w.snapshot()
    for first in (0, 3):                                                 # rule 6, also at first == n
        assert s.set_transforms(first, []) == OK and s.set_masks(first, []) == OK
    for first in (0, 25):
        assert m.set_vertices(first, np.zeros(0, M.VERTEX)) == OK and m.set_positions(first, np.zeros((0, 3))) == OK
    assert w.snapshot() == before and s.state == M.FRESH
    for call in (lambda: s.set_transform(3, Y), lambda: s.set_transforms(2, [Y, Y]), lambda: s.set_transforms(4, []), lambda: s.set_mask(3, 0),
                 lambda: s.set_masks(1, [0, 0, 0]), lambda: m.set_vertices(25, np.zeros(1, M.VERTEX)), lambda: m.set_positions(24, np.zeros((2, 3))),
                 lambda: m.set_vertices(26, np.zeros(0, M.VERTEX))):
        assert call() == STATE                                           # rule 7
        assert w.snapshot() == before                                    # rule 10


def test_skins_that_are_refused_and_bones_without_a_skin():
    w = world()
    s, m = w.scenes[0], w.models[0]
    s.build()
    assert m.set_bones(skin_cases.identity_palette(2)) == STATE           # rule 8
    bones, weights = skin_cases.random_bones(25, 4, 2, 1), skin_cases.random_weights(25, 4, 2)
    assert m.set_skin(bones, weights, 2) == OK and s.state == M.FRESH     # rule 5
    before = w.snapshot()
    bad = bones.copy()
    bad[24, 3] = 2
    for call in (lambda: m.set_skin(bad, weights, 2), lambda: m.set_skin(np.zeros((25, 9), np.uint32), np.ones((25, 9), np.float32), 2),
                 lambda: m.set_skin(bones, weights, 0), lambda: m.set_skin(bones, weights, 65537)):
        assert call() == INVALID and w.snapshot() == before              # rules 9, 10
    assert m.clear_skin() == OK and m.skin is None and s.state == M.FRESH


def test_the_rest_pose_is_the_vertices_at_set_skin():
    w = world(side=4)
    s, m = w.scenes[0], w.models[0]
    s.build()
    rest = m.verts.copy()
    bones, weights = np.zeros((16, 1), np.uint32), np.ones((16, 1), np.float32)
    m.set_skin(bones, weights, 1)
    moved = rest[4:9].copy()
    moved["position"] += 1
    assert m.set_vertices(4, moved) == OK and s.state == M.STALE          # rule 4
    assert m.geometry()[4:9].tobytes() == moved.tobytes() and m.skin["rest"].tobytes() == rest.tobytes()      # rules 15, 16
    s.update()
    shift = skin_cases.identity_palette(1)
    shift[0, 3] = 2.0
    assert m.set_bones(shift) == OK and s.state == M.STALE
    want = rest.copy()
    want["position"][:, 0] += np.float32(2.0)
    assert m.geometry().tobytes() == want.tobytes()                      # every vertex from the rest pose: the moved ones are overwritten
    assert s.update() == (OK, frozenset(["vertices"]))
    m.set_skin(bones, weights, 1)                                         # rule 14: set again, the skin captures the vertices as they are now
    assert m.skin["rest"].tobytes() == want.tobytes()


def test_an_update_with_nothing_visible_keeps_everything_pending():
    w = world()
    s, m = w.scenes[0], w.models[0]
    s.build()
    s.set_transform(0, Y)
    m.recompute_normals()
    assert m.verts["normal"].tobytes() == normals_of(m.verts["position"], m.idx).tobytes()
    s.set_masks(0, [0, 0, 0])
    before = w.snapshot()
    assert s.update() == (STATE, None) and s.build() == (STATE, None) and w.snapshot() == before              # rule 12
    assert s.pending() == frozenset(["transforms", "masks", "vertices"])
    s.set_mask(1, 0x40)
    assert s.update() == (OK, frozenset(["transforms", "masks", "vertices"])) and s.applied_vis == [1] and s.state == M.FRESH


def test_a_shared_model_leaves_every_built_scene_stale():
    w = world(n_scenes=3)
    a, b, c = w.scenes
    a.build()
    b.build()
    w.models[0].set_positions(3, np.ones((2, 3)))
    assert a.state == b.state == M.STALE and c.state == M.UNBUILT        # rule 4; a scene never built stays so (rule 1)
    assert b.update() == (OK, frozenset(["vertices"])) and a.state == M.STALE
    assert a.build() == (OK, frozenset(["vertices"])) and a.state == M.FRESH
    assert c.update() == (STATE, None) and c.build() == (OK, frozenset())


def test_add_model_takes_the_scene_back_to_unbuilt():
    w = world()
    s = w.scenes[0]
    s.build()
    s.set_transform(0, Y)
    assert s.add_model(0, Y) == OK and s.state == M.UNBUILT and s.masks[3] == 0xFF and not s.pending()
    assert s.set_mask(3, 0) == OK and s.set_transform(3, None) == OK and s.state == M.UNBUILT
    assert s.update() == (STATE, None)
    assert s.build() == (OK, frozenset()) and s.applied_vis == [0, 1, 2] and s.inst[0][1].tolist() == Y.tolist() and s.inst[3][1] is None
