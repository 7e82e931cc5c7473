"""A bounded run of the sweep over sequences of scene edits (tests/scene_edit_sweep.py) under `pytest -m gpu`: every operation's return code
against the shadow model of tests/scene_edit_model.py, and at every successful update or build the whole scene -- TLAS, instance records, every
BLAS, masks(), geometry(), the skin and morph queries, every posed skeleton, 1,500 rays, and at every third checkpoint frames of two long-lived
pipelines -- bit for bit against a fresh build of the shadow model's final state and the oracle.  What these seeds and counts cover is asserted
on the CPU by tests/test_scene_edit_stream.py, which also shows that seven wrong rules of morph targets and skeletons would each be reported.

Measured on an MI355X, the oracle's share included: 1.3 s (seed 5), 1.8 s (seed 269), 1.6 s (seed 329) for 8 sequences each -- 1,082
operations, 223 checkpoints, 78 of them with frames (before morph targets and skeletons joined: seeds 11, 88 and 3, 1,222 operations, 332
checkpoints, 7.2, 7.0 and 4.2 s).  If a case grows past about 10 s, cut sequences, not checks, and choose the seeds again so that
test_scene_edit_stream.py still finds everything it lists."""
import pytest

pytestmark = pytest.mark.gpu

SEEDS = (5, 269, 329)
SEQUENCES = 8                           # per seed


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
