"""Crowds driven from device memory (rt_crowd_set_layout, rt_crowd_set_blend_device; include/dxr_amd.h "Posed skeletons", crowds) for the
tests: the restatement of a layout's check and of its packed slots (dxrexperiments_amd/csrc/rt_crowd.h: rt_crowd_layout_layers,
rt_crowd_pack_slots), the segment of a clip restated for a NaN time -- skeleton_cases.segment raises there, because no host call lets one
through --, the numpy statement of a blend whose times may be NaN, and the rigs the GPU tests pose.  Everything else is crowd_cases.py,
skeleton_blend_cases.py and skeleton_cases.py, by import."""
import contextlib

import numpy as np

import crowd_cases as CC
import skeleton_blend_cases as B
import skeleton_cases as S

F = np.float32
N = 0xFFFFFFFF
NAN = float("nan")
SEARCH_KEYS = (1, 2, 3, 8, 33)          # one key; one segment; a middle key; a power of two; a search of six steps that ends on either side


# ---- the layout (rt_crowd_set_layout) ------------------------------------------------------------------------------------------------------
def without_times(lists):
    """every actor's records with the time taken as 0: what a layout is checked as"""
    return [[(clip, 0.0, weight, mask, mode) for clip, _, weight, mask, mode in records] for records in lists]


def validate(lists, n_clips, n_masks, posed):
    """(what, actor, layer) of a layout: crowd_cases.validate with every time taken as 0 -- the same codes in the same order, and never 6"""
    return CC.validate(without_times(lists), n_clips, n_masks, posed)


def slot_words(record, k):
    """the seven words tests/cpp/crowd_layout_sanitized.cpp writes for the slot of layer k: the clip whose keys the slot names, the clip whose
    device key times it names (0xFFFFFFFF both: RT_SKELETON_CURRENT_POSE), n_keys, mask + 1 (0: none; the base layer's is dropped), the mode,
    the bits of the weight and the pad.  Clip c has c + 1 keys."""
    clip, _, weight, mask, mode = record
    wbits = int(np.array([weight], F).view(np.uint32)[0])
    m = 0 if k == 0 or mask == N else mask + 1
    return (N, N, 0, m, mode, wbits, 0) if clip == N else (clip, clip, clip + 1, m, mode, wbits, 0)


def layout_cases():
    """crowd_cases.layer_cases: every refusal in the first, a middle and the last actor, the groups across actors, nothing to read, a null
    list, generated crowds.  Its NaN times are what a layout must ACCEPT: the cases that rt_crowd_set_blend refuses with 6 and nothing else
    are fine here"""
    return CC.layer_cases()


# ---- the segment, NaN included -------------------------------------------------------------------------------------------------------------
_segment = S.segment            # (the statement for numbers, whatever nan_times() has put in its place meanwhile)


def segment(times, t):
    """(i, a) as rt_skeleton_segment's statements give it for ANY t: skeleton_cases.segment where t is a number; for a NaN, (0, 0) on one key,
    and otherwise both range tests are false, every `times[mid] <= t` is false, so hi comes down to 1, lo stays 0 and a = (NaN - times[0]) /
    (times[1] - times[0]) = NaN"""
    if not np.isnan(t):
        return _segment(times, t)
    return (0, F(0.0)) if len(times) == 1 else (0, F(np.nan))


@contextlib.contextmanager
def nan_times():
    """inside, skeleton_cases.sampled and skeleton_blend_cases.blended find their segments with segment() above"""
    kept = S.segment
    S.segment = segment
    try:
        yield
    finally:
        S.segment = kept


def blended(clips, masks, layers, current=None):
    """skeleton_blend_cases.blended for layers whose times may be NaN"""
    with nan_times():
        return B.blended(clips, masks, layers, current)


def search_queries(times):
    """skeleton_cases.sample_times -- below, on, inside and just under every key, beyond the last, -inf and +inf -- and NaN"""
    return [F(t) for t in S.sample_times(times)] + [F(np.nan)]


# ---- what the GPU tests pose ---------------------------------------------------------------------------------------------------------------
RIGS = (("forest", 1), ("chain", 3), ("random", 65), ("random", 257))       # one joint; levels == joints; a wave's boundary; the widest block's
ACTORS = CC.ACTORS


def layer_counts(n):
    return (1, 3, 8) if n <= 65 else (1, 3)


def search_rig(n=65, seed=40):
    """(parents, inverse_bind, clips, masks): clips of 1, 2, 3, 8 and 33 keys with uneven spacing"""
    parents = S.hierarchy("random", n, seed)
    return parents, S.inverse_binds(n, seed + 1), [S.clip(parents, k, seed + 10 * k) for k in SEARCH_KEYS], B.masks_for(n, seed + 2)


def split(layers):
    """(float32[n_actors, n_layers] times, float32[n_actors, n_layers] weights) of per-actor layer lists"""
    full = [[B.layer_of(l) for l in mine] for mine in layers]
    return np.array([[l[1] for l in mine] for mine in full], F), np.array([[l[2] for l in mine] for mine in full], F)


def with_values(layers, times, weights=None):
    """the layer lists with these times (and weights) in place of their own: what the host path is given to compare"""
    out = []
    for a, mine in enumerate(layers):
        row = []
        for k, l in enumerate(mine):
            clip, _, weight, mask, mode = B.layer_of(l)
            row.append((clip, float(times[a][k]), float(weight if weights is None else weights[a][k]), mask, mode))
        out.append(row)
    return out
