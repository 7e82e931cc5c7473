"""The two counting passes (rt_pipeline_count_work, rt_pipeline_count_walk) enumerate the same queues of the last frame, beyond the
default depth limits and beyond single frames.

Both replay what the last set of launches left behind: the primary rays, the shadow rays of the primary hits, the radiance rays of
every level, the shadow rays of all deeper levels (csrc/rt_pipeline_inspect.hip, for_each_queue).  One pass traces every ray again in
canonical order, the other walks the queues with the production traversal; whatever tree they walk, the RAYS they find are the
frame's.  Held here on a 64 x 64 Cornell frame with three radiance levels and shadow rays from two of them: the two passes agree on
the rays of every stage, the primary rays are the pixels of every frame of the set, the deep levels were reached (the same frames with
one radiance level trace fewer secondary rays), both calls are repeatable, and the image
cannot tell that they ran."""
import numpy as np
import pytest

from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from test_gpu_pipeline import make_gpu_pipeline
from util import CORNELL_OBJ, cam_array, random_xforms

pytestmark = pytest.mark.gpu

W = H = 64
STAGES = ("primary", "shadow0", "secondary", "shadow1")


def mirror():
    """every hit spawns a specular ray: the chains reach the last level"""
    m = T.default_material()
    m["type"] = 2; m["reflectivity"] = 0.6; m["roughness"] = 0.3
    return m


@pytest.mark.parametrize("case", ["one_frame", "batch_of_three", "sized_by_count", "two_level"])
def test_both_counting_passes_see_the_same_queues_at_depth_three(gpu, oracle, capi, case):
    v, i = oracle.obj_load(CORNELL_OBJ)
    inst = [(0, None), (0, random_xforms(1, 11, spread=0.5)[0])] if case == "two_level" else [(0, None)]
    p = make_gpu_pipeline(capi, gpu, [(v, i)], inst, [mirror()] * len(inst), W, H)
    if case == "sized_by_count":
        p.set_queue_budget(1)
    frames = 3 if case == "batch_of_three" else 1
    pfcs = frames_of(capi, cam_array(scenes.cornell_camera(), W / H), frames, W, H)       # (one camera: the frames share U, V, W)

    def render():
        p.clear_output()
        if frames > 1:
            p.render_batch(pfcs)
        else:
            p.update(pfcs[0])
            p.render()
        return p.stats()["rays_secondary"]

    one_bounce = render()                   # the reference's depth limits: one radiance level
    p.set_depth_limits(3, 3)
    assert render() > one_bounce            # ... and three: the same rays at level 1, so the rest are rays of levels 2 and 3
    assert p.queue_memory()[1] == (case == "sized_by_count")
    img, st = p.read_output(), p.stats()
    work, walk = p.count_work(), p.count_walk()
    print(case, {s: (work[s]["rays"], walk[s]["rays"]) for s in STAGES}, st)
    for s in STAGES:
        assert work[s]["rays"] == walk[s]["rays"], s
    assert walk["primary"]["rays"] == W * H * frames
    assert walk["shadow1"]["rays"] > 0 and walk["secondary"]["rays"] > 0
    assert p.count_work() == work and p.count_walk() == walk
    assert np.array_equal(img, p.read_output())
    if case == "one_frame":
        assert walk["secondary"]["rays"] == st["rays_secondary"]
        assert walk["shadow0"]["rays"] + walk["shadow1"]["rays"] == st["rays_shadow"] and st["rays_shadow_skipped"] == 0
    p.close()
