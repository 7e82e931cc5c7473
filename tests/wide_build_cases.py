"""The meshes and instance lists the production tree builder is held to its numpy restatement on (tests/wide_build_model.py): shared by
tests/test_wide_build_model.py, which holds the model to what it claims on the CPU, and tests/test_gpu_wide_build.py, which holds the
builder to the model.  Every mesh is a few thousand triangles at most."""
import numpy as np

from dxrexperiments_amd import rtypes as T
from dxrexperiments_amd import scenes
from util import rng, sliver_soup, triangle_soup


def mesh_of(tri):
    """float[n, 3, 3] -> (vertices, indices), own vertices per triangle"""
    pos = np.ascontiguousarray(tri, np.float32).reshape(-1, 3)
    v = np.zeros(pos.shape[0], T.VERTEX)
    v["position"] = pos
    v["normal"][:, 1] = 1.0
    return v, np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)


def corner_soup(n, seed, extent=10.0, size=0.6):
    """n triangles c + (a, 0, 0), c + (0, b, 0), c + (0, 0, d): the box's surface ab + bd + da is at most sqrt(3) times |cross|, so the
    split rule (rt_refs.h: surface > 4 |cross|) never holds a triangle of it as several references -- leaves = triangles, at any n"""
    r = rng(seed)
    c = r.uniform(-extent, extent, (n, 1, 3))
    legs = r.uniform(0.2, 1.0, (n, 3)) * size * r.choice([-1.0, 1.0], (n, 3))
    return mesh_of(c + legs[:, :, None] * np.eye(3)[None])


def clones(n, seed=5):
    """n copies of one triangle: every merged box is the same box, so every choice of PLOC is a tie"""
    v, i = corner_soup(1, seed)
    return mesh_of(np.repeat(v["position"].reshape(1, 3, 3), n, axis=0))


def clones_in_soup(n_clones=600, n_others=1600):
    """A run of clones inside a soup, 2200 leaves: ties that the multi-kernel rounds see -- the run lies across workgroup edges of the pairing
    kernel -- in a tree shallow enough for the collapse (clones alone form a chain three leaves a level deep; see clones2100)"""
    v, i = corner_soup(n_others, seed=81)
    tri = v["position"].reshape(-1, 3, 3).copy()
    return mesh_of(np.concatenate([tri[:n_others // 2], np.repeat(tri[n_others // 2:n_others // 2 + 1], n_clones, axis=0), tri[n_others // 2:]]))


def flat_grid(n_side=48, extent=24.0):
    """a perfectly flat n_side x n_side grid of 2 n_side^2 triangles (the vertices of scenes.displaced_grid at height 0; extent / n_side is
    a power of two): exact area ties everywhere"""
    v, i = scenes.displaced_grid(n_side, seed=7, extent=extent)
    v = v.copy()
    v["position"][:, 1] = 0.0
    return v, i


def two_sheets(n_side=24):
    """two flat grids a hair apart, triangle by triangle in turn: neighbours in Morton order alternate between the sheets"""
    v, i = flat_grid(n_side, extent=12.0)
    tri = v["position"][i]
    up = tri.copy()
    up[:, :, 1] = 0.5
    return mesh_of(np.stack([tri, up], axis=1).reshape(-1, 3, 3))


def far_soup():
    v, i = corner_soup(1500, seed=61, extent=5.0)
    v["position"] += np.float32(4000.0)
    return v, i


def tiny_soup():
    v, i = corner_soup(700, seed=62)
    v["position"] *= np.float32(1e-30)
    return v, i


def sheet():
    """zero thickness: every box is flat on y"""
    v, i = corner_soup(900, seed=63)
    v["position"][:, 1] = 0.25
    return v, i


def huge_vertex():
    """one vertex at +3e38 and one at -3e38: extents that overflow -- an infinite scale, bytes 0"""
    v, i = corner_soup(800, seed=64)
    p = v["position"].reshape(-1, 3, 3)
    p[10, 0, 0] = 3.0e38
    p[11, 1, 1] = -3.0e38
    return v, i


def inexact_extent():
    """the root spans lo = -1e-3 .. hi = 1e4 on x: hi - lo is not a float"""
    v, i = corner_soup(600, seed=65, extent=3.0)
    p = v["position"].reshape(-1, 3, 3)
    p[:, :, 0] = (p[:, :, 0] + 3.7) * 1300.0
    assert p[:, :, 0].min() > 1.0 and p[:, :, 0].max() < 9900.0
    p[5, 0, 0] = -1.0e-3
    p[6, 1, 0] = 1.0e4
    return v, i


def tie_extent():
    """The quantiser's retry, made by hand.  The root spans lo = 2^-11 .. hi = 16320 + 2^-10 on x: hi - lo = 16320 + 2^-11 is a tie between
    two floats and rounds to the even one, 16320 = 255 * 64, so the start scale is 64 -- and fma(255, 64, lo) is the same tie and rounds to
    16320 as well, one ulp short of hi.  Every node that spans the whole x range is on the grid of 128."""
    v, i = corner_soup(600, seed=66, extent=3.0)
    p = v["position"].reshape(-1, 3, 3)
    p[:, :, 0] = (p[:, :, 0] + 3.7) * 2000.0
    assert p[:, :, 0].min() > 1.0 and p[:, :, 0].max() < 16000.0
    p[5, 0, 0] = 2.0 ** -11
    p[6, 1, 0] = 16320.0 + 2.0 ** -10
    return v, i


# the sizes of the PLOC cases: the switch from the LBVH layout (2 leaf_max + 2 leaves: 4 with leaf_max 1, 6 with 2), the workgroup edges of
# everything downstream, the single-workgroup tail (<= 2048 clusters) against one multi-kernel round before it -- at 2049 the halo of the
# pairing kernel is read at eight workgroup edges --, and several multi-kernel rounds
PLOC_SIZES = (3, 4, 5, 6, 255, 256, 257, 511, 513, 2047, 2048, 2049, 6000)


def soup(n):
    return corner_soup(n, seed=300 + n)


MESHES = {
    "clones300": lambda: clones(300),
    "clones2100": lambda: clones(2100),
    "flat_grid": flat_grid,
    "two_sheets": two_sheets,
    "soup3000": lambda: triangle_soup(3000, seed=70),
    "clones_in_soup": clones_in_soup,
    "slivers_small": lambda: sliver_soup(20, seed=21),          # 1272 references of 40 triangles: the single-workgroup tail alone
    "slivers_large": lambda: sliver_soup(60, seed=21),          # more than 2048 references: multi-kernel rounds first
    "far": far_soup,
    "tiny": tiny_soup,
    "sheet": sheet,
    "huge": huge_vertex,
    "inexact": inexact_extent,
    "tie": tie_extent,
}
_cache = {}


def mesh(name):
    if name not in _cache:
        _cache[name] = soup(int(name[4:])) if name.startswith("fat_") else MESHES[name]()
    return _cache[name]


def triangle_boxes(v, i):
    """float32[n, 6]: min / max over the three vertices (a NaN is passed over)"""
    p = v["position"][i]
    return np.concatenate([np.fmin.reduce(p, axis=1), np.fmax.reduce(p, axis=1)], axis=1)
