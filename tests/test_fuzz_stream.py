"""tests/fuzz_parity.py without a GPU: the sweep's scene / material / frame / option stream.  The GPU classes and the oracle's renderer are
replaced by stand-ins that agree with each other, so that run() walks its draws and only what it DRAWS is looked at: the `desc` of the first
ten draws of seed 11 (one of the two seeds of tests/test_gpu_fuzz.py) is pinned as it was before draws were animated -- the animation draws
from a generator of its own (fuzz_parity.animation_rng) and must not move the stream -- and the setters an animated draw issues are those
its description names."""
import types

import numpy as np

ZERO = dict.fromkeys(("rays_primary", "rays_secondary", "rays_shadow", "primary_hits", "secondary_hits"), 0)

# draws 0 - 9 of seed 11 without the key `animated`
SEED_11 = [
    {'it': 0, 'tris': [515], 'instances': 1, 'size': (188, 99), 'realtime': False, 'depth': (4, 4), 'seamless': True, 'options': {}, 'lights': 'moving', 'accum_f16': 0, 'set': 'render_batch, counted queues'},
    {'it': 1, 'tris': [6962], 'instances': 1, 'size': (49, 35), 'realtime': True, 'depth': (1, 2), 'seamless': True, 'options': {}, 'lights': 'moving', 'accum_f16': 0},
    {'it': 2, 'tris': [98], 'instances': 1, 'size': (170, 70), 'realtime': False, 'depth': (0, 1), 'seamless': True, 'options': {}, 'lights': 'random', 'accum_f16': 0, 'set': 'deferred'},
    {'it': 3, 'tris': [34], 'instances': 1, 'size': (151, 11), 'realtime': True, 'depth': (2, 3), 'seamless': True, 'options': {'lds_top': 0, 'queue_budget_mb': 1, 'primary_retry_cap': 7, 'lds_stack_rows': 6}, 'lights': 'reference', 'accum_f16': 0},
    {'it': 4, 'tris': [184], 'instances': 28, 'size': (144, 52), 'realtime': False, 'depth': (0, 2), 'seamless': True, 'options': {}, 'lights': 'reference', 'accum_f16': 0, 'set': 'deferred, small sets, counted queues'},
    {'it': 5, 'tris': [80, 356], 'instances': 1, 'size': (85, 18), 'realtime': True, 'depth': (3, 0), 'seamless': False, 'options': {}, 'lights': 'moving', 'accum_f16': 0},
    {'it': 6, 'tris': [80, 329], 'instances': 1, 'size': (58, 55), 'realtime': True, 'depth': (3, 3), 'seamless': True, 'options': {}, 'lights': 'moving', 'accum_f16': 0},
    {'it': 7, 'tris': [2048], 'instances': 1, 'size': (171, 65), 'realtime': False, 'depth': (2, 3), 'seamless': True, 'options': {}, 'lights': 'reference', 'accum_f16': 0, 'set': 'render_batch, counted queues'},
    {'it': 8, 'tris': [173], 'instances': 25, 'size': (13, 27), 'realtime': True, 'depth': (0, 3), 'seamless': False, 'options': {'leaf_max': 8, 'lds_top': 0, 'persistent_blocks_per_cu': 1, 'shadow_cache_pixels': 0}, 'lights': 'random', 'accum_f16': 0},
    {'it': 9, 'tris': [423], 'instances': 1, 'size': (58, 103), 'realtime': True, 'depth': (3, 3), 'seamless': True, 'options': {}, 'lights': 'random', 'accum_f16': 0},
]


class Anything:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return lambda *a, **k: None


class Pipe(Anything):
    def create_output(self, W, H):
        self.shape = (H, W, 4)

    def read_output(self, k=0):
        return np.zeros(self.shape, np.float32)

    def stats(self):
        return dict(ZERO)


class OracleScene(Anything):
    def render(self, mats, pfc, W, H, **k):
        return np.zeros((H, W, 4), np.float32), dict(ZERO)

    def render_realtime(self, mats, pfc, W, H, **k):
        return np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), dict(ZERO)


def test_animation_leaves_the_stream_of_seed_11_alone(capi, oracle, monkeypatch):
    import fuzz_parity
    calls = []

    class Scene(Anything):
        def set_transform(self, i, x):
            calls.append(("set_transform", [i]))

        def set_transforms(self, first, xs):
            calls.append(("set_transforms", list(range(first, first + len(xs)))))

        def update(self):
            calls.append(("update", []))

    monkeypatch.setattr(fuzz_parity, "capi", types.SimpleNamespace(
        Context=Anything, Model=Anything, Scene=Scene, Pipeline=Pipe, ProgressiveHost=capi.ProgressiveHost,
        PIPELINE_REALTIME=capi.PIPELINE_REALTIME, PIPELINE_PROGRESSIVE=capi.PIPELINE_PROGRESSIVE))
    monkeypatch.setattr(fuzz_parity, "oracle", types.SimpleNamespace(Scene=OracleScene, obj_load=oracle.obj_load, set_cube_seamless=lambda on: None))
    descs, tally = [], {}
    assert fuzz_parity.run(60, 11, Anything(), verbose=False, tally=tally, descs=descs) is None
    for got, want in zip(descs[:10], SEED_11):
        got = dict(got)
        got.pop("animated")
        assert got == want
    # every animated draw: one update, after setters that cover exactly the instances its description names, by the call it names
    animated = [d["animated"] for d in descs if d["animated"]]
    assert tally == dict(draws=60, animated=len(animated), with_identity=sum(bool(a["identity"]) for a in animated), with_hard=sum(bool(a["hard"]) for a in animated))
    assert animated and tally["with_identity"] and tally["with_hard"]
    assert [c[0] for c in calls].count("update") == len(animated)
    at = 0
    for a in animated:
        end = at + [c[0] for c in calls[at:]].index("update")
        assert {c[0] for c in calls[at:end]} == {a["by"]}, a
        assert sorted(i for c in calls[at:end] for i in c[1]) == a["moved"], a
        assert set(a["identity"]) | set(a["hard"]) <= set(a["moved"])
        at = end + 1
    assert at == len(calls)
