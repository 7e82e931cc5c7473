"""Crowds (include/dxr_amd.h "Posed skeletons", crowds) for the tests: the restatement of the host's check of every actor's layer list and of
the packed layer records (dxrexperiments_amd/csrc/rt_crowd.h), the rigs and actor counts the GPU tests pose, and per-actor calls that tell
neighbouring actors apart.  The arithmetic of a pose is not restated here: actor a of a crowd is a skeleton given the same call, so the numpy
statement is tests/skeleton_cases.py and tests/skeleton_blend_cases.py, by import."""
import numpy as np

import skeleton_blend_cases as B
import skeleton_cases as S

F = np.float32
N = 0xFFFFFFFF
NAN = float("nan")
LDS = S.lds_joints()

# (family, joints): 1 joint; a forest of roots only; a chain of 3; a star; 64 and 65 joints, which straddle a wave; 256 and 257, which
# straddle the widest block; the LDS limit as a chain, and so as many levels as joints
RIGS = (("forest", 1), ("forest", 5), ("chain", 3), ("star", 9), ("random", 64), ("random", 65), ("random", 256), ("random", 257), ("chain", LDS))
ACTORS = (1, 2, 300)            # 300: more blocks than the 256 CUs, so blocks queue behind one another


# ---- the host's check (rt_crowd_validate_layers) -------------------------------------------------------------------------------------------
def validate(lists, n_clips, n_masks, posed):
    """(what, actor, layer) for one list of raw records per actor, all as long: every actor's list is held to skeleton_blend_cases.validate;
    every actor to 2 .. 6 before any actor to 7 .. 9; the first bad actor wins; 2 names actor 0"""
    for limits in ((N, N, True), (n_clips, n_masks, posed)):
        for a, records in enumerate(lists):
            what, layer = B.validate(records, *limits)
            if what:
                return what, (0 if what <= 2 else a), layer
    return 0, 0, 0


def packed(record, k, n_joints):
    """the nine words tests/cpp/crowd_sanitized.cpp writes for layer k of a validated list: where key_a, key_b, ref_a and ref_b stand in floats
    from the clip's base, the clip, the bits of a and of the weight, mask + 1 and the mode.  Clip c has c + 1 keys at 0, 1 .. c."""
    clip, time, weight, mask, mode = record
    wbits = int(np.array([weight], F).view(np.uint32)[0])
    m = 0 if k == 0 or mask == N else mask + 1
    if clip == N:
        return (N, N, N, N, N, 0, wbits, 0, mode)
    n_keys, per_key = clip + 1, 10 * n_joints
    i, a = S.segment(np.arange(n_keys, dtype=F), time)
    abits = int(np.array([a], F).view(np.uint32)[0])
    one = n_keys == 1
    return (per_key * int(i), per_key * int(i) + (0 if one else per_key), 0, 0 if one else per_key, clip, abits, wbits, m, mode)


def layer_cases():
    """(lists, n_layers, n_clips, n_masks, posed, null, n_joints).  Every refusal code on its own in the first, a middle and the last actor,
    on 1 and on 8 layers; the two groups across actors (a state refusal in an early actor, an argument's in a late one: the late one is
    named); 0 and 9 layers with nothing to read; a null list; generated crowds"""
    ok = (0, 0.5, 1.0, N, 0)
    out = []

    def add(lists, n_clips=3, n_masks=2, posed=True, n_layers=None, null=False, n_joints=7):
        out.append(([list(x) for x in lists], len(lists[0]) if n_layers is None else n_layers, n_clips, n_masks, posed, null, n_joints))

    bad_args = ((0, 0.5, 1.0, N, 2), (0, NAN, 1.0, N, 0))                      # 3, 6 on any layer
    bad_state = ((3, 0.5, 1.0, N, 0), (N - 1, 0.5, 1.0, N, 0))                 # 7 on any layer
    for n_actors in (1, 2, 5):
        for n_layers in (1, 8):
            add([[ok] * n_layers] * n_actors)
            for at in sorted({0, n_actors // 2, n_actors - 1}):
                for layer in sorted({0, n_layers - 1}):
                    for bad in bad_args + bad_state:
                        lists = [[ok] * n_layers for _ in range(n_actors)]
                        lists[at][layer] = bad
                        add(lists); add(lists, posed=False); add(lists, n_clips=0, n_masks=0)
                    if layer > 0:
                        for bad in ((0, 0.5, 1.0, N, 1), (N, 0.5, 1.0, N, 0), (0, 0.5, 1.0, 2, 0), (0, 0.5, 1.0, N - 1, 1)):      # (additive: fine), 5, 8, 8
                            lists = [[ok] * n_layers for _ in range(n_actors)]
                            lists[at][layer] = bad
                            add(lists)
                    else:
                        for bad in ((0, 0.5, 1.0, N, 1), (N, NAN, NAN, 5, 0)):                                                    # 4; the current pose: 9 unless posed
                            lists = [[ok] * n_layers for _ in range(n_actors)]
                            lists[at][layer] = bad
                            add(lists); add(lists, posed=False)
    # the groups across actors: actor 0 names an unknown clip, the last actor has a NaN time -- the NaN is named; and two state refusals: actor 0's
    for n_layers in (1, 8):
        lists = [[ok] * n_layers for _ in range(4)]
        lists[0][n_layers - 1] = (7, 0.0, 1.0, N, 0)
        lists[3][0] = (0, NAN, 1.0, N, 0)
        add(lists)
        lists = [[ok] * n_layers for _ in range(4)]
        lists[0][n_layers - 1] = (7, 0.0, 1.0, N, 0)
        lists[3][0] = (N, 0.0, 1.0, N, 0)
        add(lists, posed=False)
    add([[]] * 3, n_layers=0); add([[]] * 3, n_layers=9); add([[]] * 3, n_layers=N); add([[]] * 2, n_layers=1, null=True)
    rng = np.random.default_rng(6)
    for _ in range(200):
        n_actors, n_layers = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        lists = []
        for a in range(n_actors):
            records = []
            for k in range(n_layers):
                clip = int(rng.choice([0, 1, 2, 3, N, N - 1], p=[0.33, 0.33, 0.3, 0.01, 0.01 if k else 0.03, 0.02 if k else 0.0]))
                records.append((clip, float(rng.choice([0.0, 1.5, 0.25, -np.inf, np.inf, NAN], p=[0.2, 0.2, 0.28, 0.15, 0.15, 0.02])), float(rng.choice(B.WEIGHTS + (NAN,))),
                                int(rng.choice([N, 0, 1, 2], p=[0.5, 0.24, 0.24, 0.02])), int(rng.choice([0, 1, 2], p=[0.58, 0.4, 0.02])) if k else int(rng.choice([0, 1], p=[0.98, 0.02]))))
            lists.append(records)
        add(lists, posed=bool(rng.integers(0, 4)), n_joints=int(rng.choice([1, 7, 65])))
    return out


# ---- what the GPU tests pose ---------------------------------------------------------------------------------------------------------------
def rig(family, n, seed=0):
    """(parents, inverse_bind, clips, masks): three clips of 1, 3 and 2 keys -- the last with raw quaternions, a fifth of them zero -- and
    the three masks of skeleton_blend_cases"""
    parents = S.hierarchy(family, n, seed + n)
    ib = S.inverse_binds(n, seed + n + 1)
    clips = [S.clip(parents, k, seed + 10 * k + n, fam) for k, fam in ((1, "unit"), (3, "unit"), (2, "raw"))]
    return parents, ib, clips, B.masks_for(n, seed + n + 2)


def actor_times(clips, n_actors):
    """(clip, time) per actor: neighbours on different clips, walking through the times below, on, between and beyond each clip's keys"""
    out = []
    for a in range(n_actors):
        c = a % len(clips)
        ts = S.sample_times(clips[c][0])
        out.append((c, float(ts[(a // len(clips)) % len(ts)])))
    return out


def actor_layers(clips, n_masks, n_actors, n_layers, seed=0):
    """a layer list per actor (skeleton_blend_cases.layer_list), each from its own seed"""
    return [B.layer_list(n_layers, clips, n_masks, seed + 31 * a) for a in range(n_actors)]


def actor_poses(parents, n_actors, seed=0):
    """float32[n_actors, n, 10]: the pose families in turn"""
    fams = ("unit", "raw", "mirror", "neg_zero")
    return np.stack([S.pose(fams[a % len(fams)], parents, seed + a) for a in range(n_actors)])


def numpy_actors(n_actors, n_levels):
    """the actors held to the numpy statement too: all of a small case, else the first, a middle and the last (the level walk of
    skeleton_cases.posed is a Python loop); every actor is held to its skeleton"""
    return list(range(n_actors)) if n_actors * n_levels <= 600 else sorted({0, n_actors // 2, n_actors - 1})
