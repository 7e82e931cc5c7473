"""Inputs, parameter sets and the comparison of the post-chain edge tests (test_denoise_edges.py on the CPU, test_gpu_post_chain_edges.py on
the GPU).  A plain module: everything is a pure function of its arguments and a seed.

The shapes straddle what rt_denoise.hip tiles by -- pass H: blocks of 256 x 1 pixels, pass V: tiles of 8 x 64, both with a halo of MAX_EXTENT = 20
texels --, the radii give every residue of filter_taps' 5-tap unroll (2K + 1 = 1, 3, 5, 7, 9, 15, 25, 39, 41), and the input families put values
where the filter's arithmetic has edges: impulses next to every tile seam (the output is the filter's footprint), black texels (lum == 0: 0 / 0 in
the tone map), negative values, -0, fp32 subnormals, values whose weighted sums overflow, +-inf and NaN."""
import numpy as np

SHAPES = [(1, 1), (1, 65), (7, 3), (8, 64), (9, 65), (19, 21), (21, 41), (40, 128), (255, 2), (256, 1), (257, 5), (277, 63), (513, 129)]    # (W, H)
RADII = [0, 1, 2, 3, 4, 7, 12, 19, 20]
FAMILY_SHAPES = [(277, 63), (21, 41)]
PARAM_SHAPE = (41, 37)
PARAM_FAMILIES = ("benign", "hostile_nonfinite")

H_BLOCK, V_TILE_W, V_TILE_H = 256, 8, 64            # rt_denoise.hip: HB, VW, VH

# the parameter sets test_denoiser_vs_oracle has always run ...
PARAM_CASES = [dict(), dict(maxKernelSize=1), dict(maxKernelSize=20), dict(maxKernelSize=0), dict(debugVisualize=1), dict(debugVisualize=2),
               dict(debugVisualize=3), dict(tonemap=0), dict(gammaCorrect=1), dict(exposure=2.5, gamma=1.8, gammaCorrect=1)]
# ... and where the composite's arithmetic has edges: exposure 0 (0 * inf, then lum == 0 everywhere) and negative (the tone map's max(x, 0) cuts,
# lum + 1 passes through 0), an exponent of 1, of 1 / 0 = inf and a negative one, and the tone map on the direct image alone
PARAM_EDGES = PARAM_CASES + [dict(exposure=0.0), dict(exposure=-1.5), dict(exposure=-1.5, tonemap=0), dict(gammaCorrect=1, gamma=1.0),
                             dict(gammaCorrect=1, gamma=0.0), dict(gammaCorrect=1, gamma=-2.2), dict(gammaCorrect=1, gamma=0.0, tonemap=0),
                             dict(tonemap=1, debugVisualize=3)]


def case_id(over):
    return "-".join("%s=%s" % kv for kv in over.items()) or "defaults"


def default_params(dtype):
    """the reference's defaults (src/DenoiseCompositor.cpp:44-49) as a record of `dtype` (the oracle's or the library's: the same six fields)"""
    prm = np.zeros((), dtype)
    prm["exposure"], prm["gamma"], prm["tonemap"], prm["gammaCorrect"], prm["maxKernelSize"], prm["debugVisualize"] = 1.0, 2.2, 1, 0, 12, 0
    return prm


def synthetic_aovs(W, H, seed):
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    direct = np.zeros((H, W, 4), np.float32)
    direct[..., 0] = 0.5 + 0.5 * np.sin(xx / 9.0)
    direct[..., 1] = (yy // 16 % 2) * 0.8               # hard edges the bilateral weight must respect
    direct[..., 2] = 0.3
    direct[..., 3] = 1.0
    ind = (r.uniform(0, 1, (H, W, 4)) ** 3).astype(np.float32)
    ind[..., 3] = 1.0
    return direct, ind


def benign(W, H, seed=3):
    return synthetic_aovs(W, H, seed)


def seams(W, H):
    """-> (xs, ys): the first column of every pass-H block but the first, the first and the last pass-V tile column boundary; the first row of
    every pass-V tile but the first -- those the shape has"""
    xs = set(range(H_BLOCK, W, H_BLOCK))
    if W > V_TILE_W:
        xs.update((V_TILE_W, (W - 1) // V_TILE_W * V_TILE_W))
    return sorted(xs), list(range(V_TILE_H, H, V_TILE_H))


def impulse_texels(W, H):
    """(y, x) of the impulses: the four corners, the centre, either side of every seam, each side once inside the image (on rows / columns of
    their own where the shape has them) and once on its border, where it may lie within a footprint of a corner's"""
    xs, ys = seams(W, H)
    t = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)}
    for x in xs:
        t.update(((H // 4, x - 1), (3 * H // 4, x), (H - 1, x - 1), (0, x)))
    for y in ys:
        t.update(((y - 1, W // 4), (y, 3 * W // 4), (y - 1, W - 1), (y, 0)))
    return sorted(t)


def impulse(W, H, seed=0):
    direct = np.empty((H, W, 4), np.float32)
    direct[...] = (0.5, 0.25, 0.3, 1.0)
    ind = np.zeros((H, W, 4), np.float32)
    for y, x in impulse_texels(W, H):
        ind[y, x] = 1.0
    return direct, ind


def edges(W, H, seed=0):
    """impulse with a hard step of the direct image across every seam: 0.4 in one channel is 4 after the shader's x 10, so the colour weight is 0
    across the step and the footprint must end there"""
    direct, ind = impulse(W, H)
    xs, ys = seams(W, H)
    for k, x in enumerate(xs):
        direct[:, x:, k % 2] += np.float32(0.4) * (1 if k % 4 < 2 else -1)
    for y in ys:
        direct[y:, :, 2] += np.float32(0.4)
    return direct, ind


def _hostile(W, H, seed, nonfinite):
    direct, ind = synthetic_aovs(W, H, seed)
    r = np.random.default_rng(seed + 1000)
    n_tex = W * H
    n_cls = 6
    n = min(n_tex, max(int(np.ceil(0.02 * n_tex)), 2 * n_cls))
    n_nf = min(n_tex, max(int(np.ceil(0.003 * n_tex)), 3)) if nonfinite else 0
    for img in (direct, ind):
        flat = img.reshape(n_tex, 4)
        at = r.choice(n_tex, n, replace=False)
        for k, p in enumerate(at):
            c = k % n_cls                                # every class occurs, whatever the shape
            if c == 0:
                flat[p] = 0.0                            # black
            elif c == 1:
                flat[p] = -r.uniform(0.0, 2.0, 4)
            elif c == 2:
                flat[p] = -0.0
            elif c == 3:                                 # fp32 subnormals of either sign
                flat[p] = (r.integers(1, 0x800000, 4, dtype=np.uint32) | (r.integers(0, 2, 4, dtype=np.uint32) << 31)).view(np.float32)
            elif c == 4:                                 # HDR, log-uniform in [1e3, 1e30]
                flat[p] = 10.0 ** r.uniform(3.0, 30.0, 4)
            else:                                        # ... and next to FLT_MAX: 41 taps of at most 1e30 cannot overflow, two of these can
                flat[p] = r.uniform(2.0e38, 3.4e38, 4)
        if img is direct:
            black = at[0::n_cls]
        for k, p in enumerate(r.choice(n_tex, n_nf, replace=False)):
            flat[p] = (np.inf, -np.inf, np.nan)[k % 3]
    ind.reshape(n_tex, 4)[black] = 0.0                   # black in BOTH images: filtered + direct == 0, so lum == 0 and the tone map divides 0 by 0
    return direct, ind


def hostile_finite(W, H, seed=5):
    return _hostile(W, H, seed, False)


def hostile_nonfinite(W, H, seed=5):
    return _hostile(W, H, seed, True)


FAMILIES = dict(benign=benign, impulse=impulse, edges=edges, hostile_finite=hostile_finite, hostile_nonfinite=hostile_nonfinite)


def enumeration():
    """-> [(id, family, (W, H), overrides)]: every shape x radius on benign input, every family x radius at FAMILY_SHAPES (the hostile ones with
    and without the tone map), PARAM_EDGES at PARAM_SHAPE on PARAM_FAMILIES.
    Consecutive entries of one (family, shape) differ in their parameters only."""
    out = []
    for W, H in SHAPES:
        for K in RADII:
            out.append(("benign-%dx%d-K%d" % (W, H, K), "benign", (W, H), dict(maxKernelSize=K)))
    for fam in FAMILIES:
        for W, H in FAMILY_SHAPES:
            for K in RADII:
                if fam == "benign" and (W, H) in SHAPES:
                    continue                             # already above
                out.append(("%s-%dx%d-K%d" % (fam, W, H, K), fam, (W, H), dict(maxKernelSize=K)))
            if fam.startswith("hostile"):                # the tone map's max(x, 0) turns every NaN into 0: the composite without it as well
                for K in RADII:
                    out.append(("%s-%dx%d-K%d-linear" % (fam, W, H, K), fam, (W, H), dict(maxKernelSize=K, tonemap=0)))
    for fam in PARAM_FAMILIES:
        for over in PARAM_EDGES:
            out.append(("%s-%dx%d-%s" % (fam, PARAM_SHAPE[0], PARAM_SHAPE[1], case_id(over)), fam, PARAM_SHAPE, over))
    return out


def groups():
    """enumeration() grouped by (family, shape): -> [(id, family, (W, H), [overrides, ...])], one denoiser object each on the GPU"""
    out = {}
    for _, fam, shape, over in enumeration():
        out.setdefault((fam, shape), []).append(over)
    return [("%s-%dx%d" % (fam, shape[0], shape[1]), fam, shape, overs) for (fam, shape), overs in out.items()]


def equal_bits(got, want, what=""):
    """True if the two arrays hold the same bits everywhere -- the sign of a zero included -- except where BOTH are NaN (any payload passes
    there); otherwise an AssertionError with the number of differing values and the first few (y, x, channel, got, want)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = (got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        at = np.argwhere(bad)
        first = "; ".join("%s got %r (%#x) want %r (%#x)" % (tuple(int(v) for v in i), got[tuple(i)], got.view(u)[tuple(i)], want[tuple(i)],
                                                              want.view(u)[tuple(i)]) for i in at[:6])
        raise AssertionError("%s: %d of %d values differ; first: %s" % (what, at.shape[0], got.size, first))
    return True
