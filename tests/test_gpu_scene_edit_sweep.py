"""A bounded run of the sweep over sequences of scene edits (tests/scene_edit_sweep.py) under `pytest -m gpu`: every operation's return code
against the shadow model of tests/scene_edit_model.py, and at every successful update or build the whole scene -- TLAS, instance records, every
BLAS, masks(), transforms(), the attachments, geometry(), the skin and morph queries, every posed skeleton and its mask count, 1,500 rays, and at
every third checkpoint and behind every update whose only cause was a pose frames of two long-lived pipelines -- bit for bit against a fresh
build of the shadow model's final state and the oracle.  What these seeds and counts cover is asserted on the CPU by
tests/test_scene_edit_stream.py, which also shows that seven wrong rules of morph targets and skeletons and twelve of device transforms,
attachments, blends and inverse kinematics would each be reported.

Measured on an MI355X, the oracle's share included: 6.8 s (seed 93), 6.1 s (seed 46), 7.0 s (seed 242) for 12 sequences each -- 1,777
operations (594, 569, 614), 435 checkpoints (145, 135, 155), 136 of them with frames (43, 50, 43) (before device transforms, attachments,
blends and inverse kinematics joined: seeds 5, 269 and 329, 8 sequences each, 1,082 operations, 223 checkpoints, 78 of them with frames, 1.3,
1.8 and 1.6 s; before morph targets and skeletons joined: seeds 11, 88 and 3, 1,222 operations, 332 checkpoints, 7.2, 7.0 and 4.2 s).  If a
case grows past about 10 s, cut sequences, not checks, and choose the seeds again so that test_scene_edit_stream.py still finds everything it
lists."""
import pytest

pytestmark = pytest.mark.gpu

SEEDS = (93, 46, 242)
SEQUENCES = 12                          # per seed


@pytest.mark.parametrize("seed", SEEDS)
def test_bounded_scene_edit_sweep(gpu, oracle, capi, seed):
    import scene_edit_sweep as sweep
    tally = {}
    bad = sweep.run(SEQUENCES, seed, gpu, tally=tally)
    assert bad is None, bad
    print("seed %d: %r" % (seed, {k: tally[k] for k in sorted(tally)}))
    assert tally["sequences"] == SEQUENCES and tally["checkpoints"] >= 3 * SEQUENCES and tally["frame checkpoints"] >= 2 * SEQUENCES, tally
    # seen on the device (the plans of every seed say so, tests/test_scene_edit_stream.py): a model has split references at one checkpoint and
    # none at a later one
    assert tally.get("checkpoints with split references", 0) > 0 and tally.get("checkpoints where split references are gone again", 0) > 0, tally
    # ... and the paths of morph targets and skeletons: a checkpoint over vertices that set_bones_from posed, one after weights went into a
    # rest pose, a scene that stayed readable behind such weights, a skeleton destroyed with its palette still queued for reading
    for key in ("checkpoints after set_bones_from", "checkpoints after a rest-pose morph", "probes of a fresh scene", "checkpoints with a posed skeleton",
                "skeletons destroyed right after set_bones_from"):
        assert tally.get(key, 0) > 0, (key, tally)
    # ... and those of attachments, blends and solves: an attached instance at a checkpoint, visible and hidden; an update whose only cause was
    # a pose, also with frames behind it; a pose that a blend and one that a solve left; instances whose skeleton has been destroyed
    for key in sweep.TALLY_KEYS:
        assert tally.get(key, 0) > 0, (key, tally)
    assert len(sweep.TALLY_KEYS) == 7
