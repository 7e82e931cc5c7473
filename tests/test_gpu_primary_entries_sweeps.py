"""The primary stage's entry lists under the suite's broad sweeps, with the lists FORCED ON (primary_entries=1).

By default only sets of four frames or more start their primary rays from entry lists, so the single frames that most of the suite renders
walk from the root.  Here the machinery of tests/test_gpu_option_matrix.py and tests/fuzz_parity.py runs once more with the option set, against
the CPU oracle, which knows nothing of lists:

  * every launch option of the registry (tests/option_cases.py) and every combination of LAUNCH_COMBOS, each next to primary_entries=1 --
    short stacks and the retry launch, no LDS top, other grids, the shadow cache's shapes, sets cut by batch_max, counted queues, the
    persistent primary launch (which keeps the root) -- on the single-level launch scenes, frame by frame and as one deferred set;
  * every row of the builder options' pairwise cover (other leaf sizes, the LBVH layout, the surface-area collapse, split references on and
    off), the PLOC fallback, and the lists' own options (a capacity of 1, cuts of 32 and 7), likewise;
  * the bounded fuzz sweeps of tests/test_gpu_fuzz.py, seeds and all, with RT_DEBUG_OPTIONS=primary_entries=1 in the environment, so that
    the contexts the sweep makes for its own option draws force the lists on too: random scenes, sizes down to one tile column, realtime and
    progressive pipelines, depths, animated instances, sets and single frames.
"""
import pytest

import fuzz_parity
import option_cases
import test_gpu_option_matrix as M

pytestmark = pytest.mark.gpu

ON = {"primary_entries": 1}
SCENES = ("atrium", "cables")           # the single-level launch scenes (cables: split references, the reference-aware kernels)
LAUNCH = [dict(c, **ON) for c in M.LAUNCH_CASES]
BUILD = [dict(r, **ON) for r in M.BUILD_ROWS] + [dict(fail_ploc_rounds=1, **ON), dict(fail_ploc_rounds=1, split_refs=0, **ON)]
OWN = [dict(ON), dict(ON, primary_entries_cap=1), dict(ON, primary_entries_cap=3), dict(ON, primary_entries_cut=32), dict(ON, primary_entries_cut=7),
       dict(ON, primary_entries_cap=1, lds_stack_rows=6, primary_persistent=0), dict(ON, lds_top=0, lds_stack_rows=6, primary_persistent=0, primary_retry_cap=7)]
CASES = LAUNCH + BUILD + OWN


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda c: M._case_id(CASES[c]))
def test_options_next_to_forced_lists_render_the_oracles_image(oracle, capi, case, scene):
    opts = CASES[case]
    frames = max([3] + [option_cases.OPTIONS[n].get("frames", 3) for n in opts if n in option_cases.OPTIONS])
    truth = M.launch_truth(oracle, capi, scene)
    ctx = M.context(capi, opts)
    try:
        sc = M.gpu_scene(capi, ctx, truth.models, truth.inst)
        what = "%s %s" % (scene, opts)
        M.check_frames(capi, ctx, sc, truth, frames, 0, what + ", frame by frame")
        M.check_frames(capi, ctx, sc, truth, frames, frames, what + ", one deferred set")
    finally:
        ctx.close()


def test_the_forced_option_reaches_the_walk(capi):
    """what the cases above rely on: a single frame of a single-level scene under primary_entries=1 is walked from lists, under the environment's
    spelling of the option as well; under primary_persistent=1 it is not"""
    import os
    from dxrexperiments_amd import rtypes as T
    from util import cam_array, triangle_soup
    W, H = 64, 40

    def lists(ctx):
        sc = capi.Scene(ctx)
        sc.add_model(capi.Model(ctx, *triangle_soup(3000, seed=3)))
        p = capi.Pipeline(ctx)
        p.set_scene(sc)
        p.add_material(T.default_material())
        p.set_environment_constant((0.5, 0.5, 0.5))
        p.create_output(W, H)
        p.build_acceleration_structures()
        p.update(capi.ProgressiveHost(1).update(cam_array(dict(eye=(0, 0, 30), at=(0, 0, 0), up=(0, 1, 0), fov=0.8), W / H), 0.0, 1, W, H))
        p.render()
        return p.primary_entries()[0] is not None

    for opts, want in ((dict(ON), True), ({}, False), (dict(ON, primary_persistent=1), False)):
        ctx = M.context(capi, opts)
        assert lists(ctx) == want, opts
        ctx.close()
    old = os.environ.get("RT_DEBUG_OPTIONS")
    os.environ["RT_DEBUG_OPTIONS"] = "primary_entries=1"
    try:
        ctx = capi.Context(0)
        assert lists(ctx)
        ctx.close()
    finally:
        if old is None:
            del os.environ["RT_DEBUG_OPTIONS"]
        else:
            os.environ["RT_DEBUG_OPTIONS"] = old


@pytest.mark.parametrize("seed", [11, 12])
def test_bounded_fuzz_parity_with_forced_lists(oracle, capi, monkeypatch, seed):
    monkeypatch.setenv("RT_DEBUG_OPTIONS", "primary_entries=1")
    ctx = capi.Context(0)
    try:
        tally = {}
        assert fuzz_parity.run(100, seed, ctx, verbose=False, tally=tally) is None
        assert tally["draws"] == 100
    finally:
        ctx.close()
