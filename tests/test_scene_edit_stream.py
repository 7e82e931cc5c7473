"""tests/scene_edit_sweep.py and tests/scene_edit_model.py without a GPU.  The sweep's plans are drawn on the shadow model alone, so what the seeds
and counts of tests/test_gpu_scene_edit_sweep.py cover can be said here: every operation kind succeeds and every refusable one is refused, an
update applies each non-empty subset of {transforms, masks, vertices}, and the interleavings the sweep exists for all occur.  The GPU classes are
replaced by a stand-in that obeys a second shadow model, in the manner of tests/test_fuzz_stream.py, so that run() walks its sequences; and the
shadow model itself is held to hand-written outcomes, rule by rule (the numbers are those of scene_edit_model's docstring)."""
import numpy as np

import scene_edit_model as M
import scene_edit_sweep as sweep
import skin_cases
from deform_cases import grid_mesh, normals_of
from test_gpu_scene_edit_sweep import SEEDS, SEQUENCES

OK, INVALID, STATE = M.OK, M.ERR_INVALID_ARG, M.ERR_STATE
X = np.arange(12, dtype=np.float32)
Y = X + 100


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
        predicted.append("split references come and go" in per_seed)
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


# ---- the shadow model, rule by rule -------------------------------------------------------------------------------------------------------------
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
