"""Blended and layered clips (rt_skeleton_set_blend): the numpy restatement shared by tests/test_skeleton_blend_abi.py (CPU) and
tests/test_gpu_skeleton_blend.py -- the definition of include/dxr_amd.h "Posed skeletons", "blending", in fp32, in the stated order, written
from that text and not from the kernel, on top of skeleton_cases.sampled / segment / posed -- the host's check of a layer list restated, and
the case generators: layer lists with mixed modes, masks and weights."""
import numpy as np

import skeleton_cases as S

F = np.float32
MAX_LAYERS = 8
CURRENT = None                  # a layer's clip: the pose the skeleton holds (layer 0 only)
BLEND, ADDITIVE = 0, 1
WEIGHTS = (0.0, 0.25, 1.0, -0.5, 1.5)
IDENTITY_Q = np.array([0, 0, 0, 1], F)


# ---- the definition --------------------------------------------------------------------------------------------------------------------
def normalised(q):
    """float32[n, 4] by the sampling rule: n = ((xx + yy) + zz) + ww; q * (1 / sqrt(n)) if 0 < n < inf, else (0, 0, 0, 1)"""
    q = np.ascontiguousarray(q, F)
    with np.errstate(all="ignore"):
        n = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        ok = (n > 0) & np.isfinite(n)
        inv = F(1.0) / np.sqrt(n)
        assert n.dtype == inv.dtype == F
        out = np.empty_like(q)
        for c in range(4):
            out[:, c] = np.where(ok, q[:, c] * inv, IDENTITY_Q[c])
    return out


def hamilton(p, q):
    """p (x) q of float32[n, 4] quaternions (x, y, z, w), grouped as the header groups it"""
    px, py, pz, pw = (np.ascontiguousarray(p[:, c], F) for c in range(4))
    qx, qy, qz, qw = (np.ascontiguousarray(q[:, c], F) for c in range(4))
    with np.errstate(all="ignore"):
        r = np.stack([((pw * qx + px * qw) + py * qz) - pz * qy,
                      ((pw * qy - px * qz) + py * qw) + pz * qx,
                      ((pw * qz + px * qy) - py * qx) + pz * qw,
                      ((pw * qw - px * qx) - py * qy) - pz * qz], axis=1)
    assert r.dtype == F
    return r


def conj(q):
    return np.ascontiguousarray(q, F) * np.array([-1, -1, -1, 1], F)        # (a sign: exact)


def layer_of(layer):
    """(clip, time, weight, mask, mode) of a tuple that may stop after the time or after the weight"""
    layer = tuple(layer) + (0.0, 1.0, None, BLEND)[len(layer) - 1:]
    clip, time, weight, mask, mode = layer
    return clip, time, weight, mask, {"blend": BLEND, "additive": ADDITIVE}.get(mode, mode)


def blended(clips, masks, layers, current=None):
    """the local pose float32[n, 10] a blend leaves.  clips: a list of (times, keys); masks: a list of float32[n]; layers: a list of (clip,
    time, weight, mask, mode) with clip None for `current`, the float32[n, 10] the skeleton holds"""
    P = None
    for k, layer in enumerate(layers):
        clip, time, weight, mask, mode = layer_of(layer)
        if clip is CURRENT:
            assert k == 0
            P = np.array(current, F, copy=True)
            continue
        times, keys = clips[clip]
        Sk = S.sampled(times, keys, time)
        assert Sk.dtype == F
        if k == 0:
            P = Sk.copy()                                # (bit for bit: weight and mask are not read)
            continue
        with np.errstate(all="ignore"):
            w = np.full(len(P), F(weight), F) if mask is None else F(weight) * np.ascontiguousarray(masks[mask], F)
            assert w.dtype == F
            out = P.copy()
            if mode == BLEND:
                d = ((P[:, 3] * Sk[:, 3] + P[:, 4] * Sk[:, 4]) + P[:, 5] * Sk[:, 5]) + P[:, 6] * Sk[:, 6]
                Sk = Sk.copy()
                Sk[d < 0, 3:7] = -Sk[d < 0, 3:7]         # (a NaN d compares false: nothing is negated)
                for c in range(10):
                    out[:, c] = P[:, c] + (w * (Sk[:, c] - P[:, c]))
                out[:, 3:7] = normalised(out[:, 3:7])
            else:
                assert mode == ADDITIVE
                R = S.sampled(times, keys, F(-np.inf))
                assert S.segment(times, F(-np.inf)) == (0, F(0.0))
                for c in (0, 1, 2, 7, 8, 9):
                    out[:, c] = P[:, c] + (w * (Sk[:, c] - R[:, c]))
                D = hamilton(conj(R[:, 3:7]), Sk[:, 3:7])
                D[D[:, 3] < 0] = -D[D[:, 3] < 0]
                E = np.empty_like(D)
                for c in range(3):
                    E[:, c] = w * D[:, c]
                E[:, 3] = F(1.0) + (w * (D[:, 3] - F(1.0)))
                out[:, 3:7] = normalised(hamilton(P[:, 3:7], normalised(E)))
            assert out.dtype == F
            P = out
    return P


# ---- the host's check of a layer list (dxrexperiments_amd/csrc/rt_skeleton.h: rt_skeleton_validate_layers) --------------------------------
NO_MASK = CURRENT_POSE = 0xFFFFFFFF


def validate(records, n_clips, n_masks, posed):
    """(what, layer) for raw records (clip, time, weight, mask, mode) of unsigned words and floats: 0 fine, 2 n_layers outside 1 .. 8,
    3 an unknown mode, 4 an additive layer 0, 5 the current pose on a layer other than 0, 6 a NaN time on a layer that samples -- every
    layer is held to these first --, 7 an unknown clip, 8 an unknown mask (not on layer 0: its mask is not read), 9 the current pose before
    the first pose.  2 .. 6 are RT_ERR_INVALID_ARG, 7 .. 9 RT_ERR_STATE."""
    if not 1 <= len(records) <= MAX_LAYERS:
        return 2, 0
    for k, (clip, time, weight, mask, mode) in enumerate(records):
        if mode not in (BLEND, ADDITIVE):
            return 3, k
        if k == 0 and mode != BLEND:
            return 4, k
        if k > 0 and clip == CURRENT_POSE:
            return 5, k
        if clip != CURRENT_POSE and np.isnan(time):
            return 6, k
    for k, (clip, time, weight, mask, mode) in enumerate(records):
        if clip == CURRENT_POSE:
            if not posed:
                return 9, k
        elif clip >= n_clips:
            return 7, k
        if k > 0 and mask != NO_MASK and mask >= n_masks:
            return 8, k
    return 0, 0


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def masks_for(n, seed):
    """three masks: arange(n) / n (a lane that reads its neighbour's entry is caught), zeros and ones at random, weights in -0.5 .. 1.5"""
    rng = np.random.default_rng(seed)
    return [(np.arange(n, dtype=np.float64) / n).astype(F), (rng.uniform(size=n) < 0.5).astype(F), rng.uniform(-0.5, 1.5, n).astype(F)]


def layer_list(n_layers, clips, n_masks, seed):
    """n_layers layers over `clips` with times below, on, between and beyond their keys; from layer 1 on the modes alternate starting at a
    random one, the layers are masked in pairs (masked, masked, not, not, ... from a random phase), and the weights walk through WEIGHTS from a random start: 8 layers use every weight, both
    modes masked and unmasked"""
    rng = np.random.default_rng(seed)
    out = []
    first_mode, first_weight = int(rng.integers(0, 2)), int(rng.integers(0, len(WEIGHTS)))
    for k in range(n_layers):
        clip = int(rng.integers(0, len(clips)))
        ts = S.sample_times(clips[clip][0])
        t = float(ts[int(rng.integers(0, len(ts)))])
        if k == 0:
            out.append((clip, t, 1.0, None, BLEND))
            continue
        mode = (first_mode + k) % 2
        mask = None if ((k + first_weight) // 2) % 2 == 0 else int(rng.integers(0, n_masks))
        out.append((clip, t, WEIGHTS[(first_weight + k) % len(WEIGHTS)], mask, mode))
    return out
