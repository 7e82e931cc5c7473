"""The primary stage's entry lists (csrc/rt_pipeline_entries.hip k_primary_entries, option primary_entries).

Once per set of launches every 8x8 tile gets a list of the children below a cut through the top of the tree that ANY of its rays, in any
frame of the set, can be made to enter by the walk's own culling, with a lower bound tnear of the entry distance; the tile's rays start
from the list instead of the root.  Two things are held here:

  * the image cannot tell: every case renders with primary_entries=0 (the walk from the root) and with the lists, and compares the
    accumulated image -- for a realtime pipeline both outputs -- and the ray and hit counts bit for bit;
  * the lists are conservative, tested directly: for every pixel of every frame a numpy walk of the cut with the CANONICAL box test
    (oracle.slab_batch on the boxes tests/wide_tree.py decodes, the restatement tests/test_wide_step_edges.py uses; tmax = the extent
    of the scene and the eye) finds the children below the cut that the ray reaches.  Every one of them has to be in its tile's list --
    or, where the tile fell back to a coarser cut, below an entry of the list -- with a tnear <= the ray's own entry distance.  No
    exceptions, and the reference walk alone decides which pairs exist.
"""
import numpy as np
import pytest

from dxrexperiments_amd import rtypes as T, scenes
from test_gpu_batch import frames_of
from util import CORNELL_OBJ, cam_array, primary_rays, triangle_soup
import wide_tree

pytestmark = pytest.mark.gpu

COUNTS = ("rays_primary", "rays_secondary", "rays_shadow", "rays_shadow_skipped", "primary_hits", "secondary_hits", "frames")
EMPTY = 0x7FFFFFFE


def context(capi, **opts):
    ctx = capi.Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


@pytest.fixture(scope="module")
def ctx_off(capi):
    ctx = context(capi, primary_entries=0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx_on(capi):
    ctx = context(capi, primary_entries=1)          # (the default, -1, keeps the lists for sets of four frames or more)
    yield ctx
    ctx.close()


def test_by_default_sets_of_four_frames_or_more_use_lists(capi, gpu, ctx_off):
    W, H = 64, 64
    pfcs = frames_of(capi, cam_array(scenes.cornell_camera(), W / H), 9, W, H)
    auto, off = cornell(capi, gpu, W, H), cornell(capi, ctx_off, W, H)
    for mode, lists in ((0, False), (3, False), (4, True), (9, True)):
        assert_same(run(auto, pfcs[:8] if mode == 4 else pfcs, mode), run(off, pfcs[:8] if mode == 4 else pfcs, mode), "default, mode %d" % mode)
        assert (lists_of(auto)[0] is not None) == lists, mode


def pipeline_of(capi, ctx, model, W, H, kind=None, env=None):
    sc = capi.Scene(ctx)
    sc.add_model(model)
    p = capi.Pipeline(ctx) if kind is None else capi.Pipeline(ctx, kind)
    p.set_scene(sc)
    p.add_material(T.default_material())
    if env is None:
        p.set_environment_constant((0.5, 0.5, 0.5))
    else:
        p.set_environment_cube(env)
    p.create_output(W, H)
    p.build_acceleration_structures()
    p.the_scene = sc
    return p


def cornell(capi, ctx, W, H, kind=None):
    return pipeline_of(capi, ctx, capi.Model(ctx, path=CORNELL_OBJ), W, H, kind)


@pytest.fixture(scope="module")
def atrium_mesh():
    return scenes.sponza_class(seed=42)


def mesh_pipeline(capi, ctx, mesh, W, H):
    return pipeline_of(capi, ctx, capi.Model(ctx, *mesh), W, H, env=scenes.sky_cubemap(16))


def run(p, pfcs, mode):
    """mode 0: frame by frame; n > 0: sets of n frames.  -> (outputs, totals)"""
    p.clear_output()
    p.reset_totals()
    if mode == 0:
        for c in pfcs:
            p.update(c); p.render()
    else:
        for at in range(0, len(pfcs), mode):
            p.render_batch(pfcs[at:at + mode])
    outs = [p.read_output(0)] + ([p.read_output(1)] if p.kind == 1 else [])
    return outs, p.totals()


def assert_same(a, b, what):
    (ia, ta), (ib, tb) = a, b
    for k, (x, y) in enumerate(zip(ia, ib)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "%s: output %d differs on %d pixels" % (what, k, int((x != y).any(axis=2).sum()))
    for k in COUNTS:
        assert ta[k] == tb[k], (what, k, ta[k], tb[k])


def lists_of(p):
    codes, tnear, cut = p.primary_entries()
    return codes, tnear, cut


@pytest.mark.parametrize("size", [(64, 64), (45, 37), (8, 78), (70, 8)])
def test_cornell_single_frames_and_sets(capi, ctx_on, ctx_off, size):
    """partial tiles (45 x 37), one column and one row of tiles included; single frames, sets of 2 and of 5"""
    W, H = size
    cam = cam_array(scenes.cornell_camera(), W / H)
    pfcs = frames_of(capi, cam, 5, W, H)
    on, off = cornell(capi, ctx_on, W, H), cornell(capi, ctx_off, W, H)
    for mode in (0, 2, 5):
        assert_same(run(on, pfcs, mode), run(off, pfcs, mode), "cornell %dx%d mode %d" % (W, H, mode))
        assert lists_of(on)[0] is not None and lists_of(off)[0] is None, "the two runs are not the two walks"
    codes, tnear, cut = lists_of(on)
    assert codes.shape[0] == ((W + 7) // 8) * ((H + 7) // 8)
    n = (codes != EMPTY).argmin(axis=1)             # the first sentinel
    assert np.all(codes[np.arange(codes.shape[0]), n] == EMPTY) and np.all(np.isposinf(tnear[np.arange(codes.shape[0]), n]))
    for t in range(codes.shape[0]):
        assert np.all(np.diff(tnear[t, :n[t]]) >= 0), "tile %d: not sorted by tnear" % t
    assert n.max() >= 1 and np.all(tnear[:, 0][n > 0] >= 0)


def test_cornell_realtime_both_outputs(capi, ctx_on, ctx_off):
    W, H = 64, 64
    cam = cam_array(scenes.cornell_camera(), W / H)
    host = capi.ProgressiveHost(3)
    pfcs = [host.update_realtime(cam, 0.0, f + 1, W, H) for f in range(2)]
    on, off = cornell(capi, ctx_on, W, H, capi.PIPELINE_REALTIME), cornell(capi, ctx_off, W, H, capi.PIPELINE_REALTIME)
    a, b = run(on, pfcs, 0), run(off, pfcs, 0)
    assert len(a[0]) == 2
    assert_same(a, b, "realtime cornell")
    assert lists_of(on)[0] is not None


@pytest.fixture(scope="module")
def atrium_pair(capi, ctx_on, ctx_off, atrium_mesh):
    W, H = 96, 64
    return mesh_pipeline(capi, ctx_on, atrium_mesh, W, H), mesh_pipeline(capi, ctx_off, atrium_mesh, W, H)


@pytest.mark.parametrize("mode", [0, 2, 5])
def test_atrium_from_the_bench_camera(capi, atrium_pair, mode):
    W, H = 96, 64
    on, off = atrium_pair
    pfcs = frames_of(capi, cam_array(scenes.sponza_camera(), W / H), 5, W, H)
    assert_same(run(on, pfcs, mode), run(off, pfcs, mode), "atrium mode %d" % mode)
    assert lists_of(on)[0] is not None and lists_of(off)[0] is None


def test_a_set_of_different_cameras_runs_without_lists(capi, atrium_pair):
    """the tile's directions differ between the frames: the set falls back to the root, the sets around it do not"""
    W, H = 96, 64
    on, off = atrium_pair
    c0 = scenes.sponza_camera()
    c1 = dict(c0, at=tuple(np.add(c0["at"], (0.5, 0.25, 0.0))))
    pfcs = frames_of(capi, cam_array(c0, W / H), 2, W, H) + frames_of(capi, cam_array(c1, W / H), 2, W, H, first=3)
    a = run(on, pfcs, 4)
    assert lists_of(on)[0] is None, "a set whose frames do not share U, V, W used lists"
    assert_same(a, run(off, pfcs, 4), "mixed cameras, one set")
    a = run(on, pfcs, 2)
    assert lists_of(on)[0] is not None
    assert_same(a, run(off, pfcs, 2), "mixed cameras, a set each")


def test_camera_outside_looking_away(capi, ctx_on, ctx_off):
    """every list is empty and every ray misses"""
    W, H = 64, 40
    cam = cam_array(dict(eye=(0.0, 1.0, 30.0), at=(0.0, 1.0, 60.0), up=(0, 1, 0), fov=0.8), W / H)
    pfcs = frames_of(capi, cam, 3, W, H)
    on, off = cornell(capi, ctx_on, W, H), cornell(capi, ctx_off, W, H)
    for mode in (0, 3):
        a = run(on, pfcs, mode)
        assert_same(a, run(off, pfcs, mode), "looking away, mode %d" % mode)
        assert a[1]["primary_hits"] == 0
        codes, tnear, _ = lists_of(on)
        assert np.all(codes[:, 0] == EMPTY), "%d tiles have entries" % int((codes[:, 0] != EMPTY).sum())


def wall_scene(pfc, eye_z):
    """Two walls of 8 x 8 axis-aligned quads facing +z, the near one at z = 0 filling the view of a camera at (0, 0, eye_z) that looks exactly
    along -z: the quads' edges project onto the borders of the 8 x 8 pixel tiles of a 64 x 64 image.  Both windings of every triangle."""
    cp = pfc["cameraParams"]
    U, V, Wv = cp["U"][:3].astype(np.float64), cp["V"][:3].astype(np.float64), cp["W"][:3].astype(np.float64)
    assert Wv[0] == 0 and Wv[1] == 0 and Wv[2] < 0, "the camera does not look exactly along -z"
    pos, idx = [], []
    for z, grow in ((0.0, 1.0), (-2.0, 1.5)):
        s = (eye_z - z) / -Wv[2]
        hx, hy = np.abs(U).max() * s * grow, np.abs(V).max() * s * grow
        xs, ys = np.linspace(-hx, hx, 9), np.linspace(-hy, hy, 9)
        for a in range(8):
            for b in range(8):
                k = len(pos)
                pos += [(xs[a], ys[b], z), (xs[a + 1], ys[b], z), (xs[a + 1], ys[b + 1], z), (xs[a], ys[b + 1], z)]
                idx += [(k, k + 1, k + 2), (k, k + 2, k + 3), (k, k + 2, k + 1), (k, k + 3, k + 2)]
    v = np.zeros(len(pos), T.VERTEX)
    v["position"] = np.array(pos, np.float32)
    v["normal"] = (0, 0, 1)
    return v, np.array(idx, np.uint32)


def test_camera_along_minus_z_at_walls_on_tile_borders(capi, ctx_on, ctx_off):
    """direction intervals that straddle zero (the middle tiles), the steep path (the middle columns and rows have components near zero) and
    boxes that the tiles' frusta graze exactly at their borders"""
    W = H = 64
    cam = cam_array(dict(eye=(0.0, 0.0, 5.0), at=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=0.8), 1.0)
    pfcs = frames_of(capi, cam, 5, W, H)
    mesh = wall_scene(pfcs[0], 5.0)
    on, off = mesh_pipeline(capi, ctx_on, mesh, W, H), mesh_pipeline(capi, ctx_off, mesh, W, H)
    for mode in (0, 2, 5):
        a = run(on, pfcs, mode)
        assert_same(a, run(off, pfcs, mode), "walls, mode %d" % mode)
        assert a[1]["primary_hits"] == 5 * W * H
    assert lists_of(on)[0] is not None


def test_small_stack_and_the_retry_launch(capi, ctx_off):
    """lds_stack_rows=6: most primary rays of a deep soup give up and are walked from the root by the retry launch (primary_persistent=0:
    with so many of them the pipeline would otherwise turn to the persistent primary launch, which starts from the root, after a few sets)"""
    W, H = 96, 64
    mesh = triangle_soup(20000, seed=77, extent=6.0, size=0.5)
    cam = cam_array(dict(eye=(0.0, 1.0, 16.0), at=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=0.8), W / H)
    pfcs = frames_of(capi, cam, 3, W, H)
    want = run(mesh_pipeline(capi, ctx_off, mesh, W, H), pfcs, 0)
    for opts in (dict(lds_stack_rows=6), dict(lds_stack_rows=6, primary_retry_cap=7)):
        ctx = context(capi, primary_persistent=0, primary_entries=1, **opts)
        p = mesh_pipeline(capi, ctx, mesh, W, H)
        for mode in (0, 3):
            assert_same(run(p, pfcs, mode), want, "%r mode %d" % (opts, mode))
            assert lists_of(p)[0] is not None
        ctx.close()


def test_render_bands_with_two_ranks(capi, ctx_on, ctx_off, atrium_mesh):
    W, H = 96, 60
    pfcs = frames_of(capi, cam_array(scenes.sponza_camera(), W / H), 2, W, H)
    imgs = []
    for ctx in (ctx_on, ctx_off):
        p = mesh_pipeline(capi, ctx, atrium_mesh, W, H)
        p.clear_output()
        for c in pfcs:
            p.update(c)
            for r in range(2):
                p.render_bands(8, r, 2)
        imgs.append(p.read_output())
        assert (lists_of(p)[0] is not None) == (ctx is ctx_on)
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))
    whole = mesh_pipeline(capi, ctx_off, atrium_mesh, W, H)
    assert np.array_equal(run(whole, pfcs, 0)[0][0].view(np.uint32), imgs[0].view(np.uint32))


@pytest.mark.parametrize("opts", [dict(primary_entries_cap=1), dict(primary_entries_cap=5), dict(primary_entries_cut=32), dict(primary_entries_cut=7),
                                  dict(primary_entries=1, lds_top=0)])
def test_forced_capacity_and_other_cuts(capi, atrium_pair, atrium_mesh, opts):
    """a capacity of 1 sends nearly every tile to a coarser cut and in the end to the root; other cuts make other lists"""
    W, H = 96, 64
    _, off = atrium_pair
    pfcs = frames_of(capi, cam_array(scenes.sponza_camera(), W / H), 3, W, H)
    ctx = context(capi, **dict(dict(primary_entries=1), **opts))
    p = mesh_pipeline(capi, ctx, atrium_mesh, W, H)
    for mode in (0, 3):
        assert_same(run(p, pfcs, mode), run(off, pfcs, mode), "%r mode %d" % (opts, mode))
    codes, tnear, cut = lists_of(p)
    assert cut == opts.get("primary_entries_cut", 128)
    n = (codes != EMPTY).argmin(axis=1)
    if "primary_entries_cap" in opts:
        assert n.max() <= opts["primary_entries_cap"]
        internal = (codes >= 0) & (codes != EMPTY)
        assert (internal & (codes < cut)).any(), "no tile fell back to a coarser cut"
    ctx.close()


def test_option_values_are_checked(capi):
    ctx = capi.Context(0)
    for name, bad in (("primary_entries", 2), ("primary_entries", -2), ("primary_entries_cut", 129), ("primary_entries_cap", 33), ("primary_entries", "on")):
        with pytest.raises(capi.RtError):
            ctx.set_option(name, bad)
    ctx.close()


# ---- the lists are conservative ---------------------------------------------------------------------------------------------------------

def reference_reach(oracle, dec, cut, O, D):
    """The canonical walk of the cut for every ray: -> (reached bool[n, cut], entry float32[n, cut] of the internal nodes below the cut's
    index, and the frontier pairs (ray, code, entry distance, parent node) -- children that hang below the cut under a reached node)."""
    n = O.shape[0]
    n_nodes = dec["code"].shape[0]
    cut = min(cut, n_nodes)
    reached = np.zeros((n, cut), bool)
    entry = np.zeros((n, cut), np.float32)
    reached[:, 0] = True
    fr = []
    for i in range(cut):
        at = np.nonzero(reached[:, i])[0]
        if at.size == 0:
            continue
        for k in range(4):
            code = int(dec["code"][i, k])
            if code == wide_tree.NONE:
                continue
            hit, e = oracle.slab_batch(O[at], D[at], np.broadcast_to(dec["lo"][i, k], (at.size, 3)), np.broadcast_to(dec["hi"][i, k], (at.size, 3)))
            r = at[hit]
            if 0 <= code < cut:
                reached[r, code] = True
                entry[r, code] = e[hit]
            else:
                fr.append((r, np.full(r.size, code, np.int64), e[hit], np.full(r.size, i, np.int64)))
    cat = lambda j, dt: np.concatenate([f[j] for f in fr]).astype(dt) if fr else np.zeros(0, dt)
    return reached, entry, (cat(0, np.int64), cat(1, np.int64), cat(2, np.float32), cat(3, np.int64))


@pytest.mark.parametrize("scene", ["cornell", "atrium"])
def test_lists_are_conservative(capi, oracle, ctx_on, atrium_mesh, scene):
    W, H, S = 64, 48, 3
    if scene == "cornell":
        p = cornell(capi, ctx_on, W, H)
        cam = cam_array(scenes.cornell_camera(), W / H)
    else:
        p = mesh_pipeline(capi, ctx_on, atrium_mesh, W, H)
        cam = cam_array(scenes.sponza_camera(), W / H)
    pfcs = frames_of(capi, cam, S, W, H)
    p.render_batch(pfcs)
    codes, tnear, cut = lists_of(p)
    tiles_x = W // 8
    assert codes is not None and codes.shape[0] == tiles_x * (H // 8)
    nodes, root, recs = p.the_scene.wide_read(0)
    assert root == 0 and nodes.shape[0] > 0
    dec = wide_tree.decode(nodes)
    parent = np.full(nodes.shape[0], -1, np.int64)
    for k in range(4):
        c = dec["code"][:, k]
        m = (c >= 0) & (c != wide_tree.NONE)
        parent[c[m]] = np.nonzero(m)[0]
    # tmax: the extent of the scene and the eye -- no box of the scene is entered farther away than that
    lo_all = np.nanmin(np.where(dec["code"][0][:, None] != wide_tree.NONE, dec["lo"][0], np.nan), axis=0)
    hi_all = np.nanmax(np.where(dec["code"][0][:, None] != wide_tree.NONE, dec["hi"][0], np.nan), axis=0)
    n_pairs = n_fallback = 0
    for pfc in pfcs:
        O, D = primary_rays(pfc, W, H)
        eye = O[0, :3]
        ext = np.float32(np.linalg.norm(np.maximum(hi_all, eye).astype(np.float64) - np.minimum(lo_all, eye).astype(np.float64)))
        D[:, 3] = ext
        reached, entry, (ray, code, e, par) = reference_reach(oracle, dec, cut, O, D)
        assert ray.size > 0
        tile = (ray // W // 8) * tiles_x + (ray % W) // 8
        # the pair's own entry in its tile's list
        same = codes[tile] == code[:, None]
        have = same.any(axis=1) & (codes[tile] != EMPTY).cumprod(axis=1).astype(bool)[np.arange(ray.size), same.argmax(axis=1)]
        tn = tnear[tile, same.argmax(axis=1)]
        bad = have & ~(tn <= e)
        assert not bad.any(), "%d pairs with tnear above the ray's entry distance, first: ray %d code %d tnear %r entry %r" % (
            int(bad.sum()), ray[bad][0], code[bad][0], tn[bad][0], e[bad][0])
        n_pairs += int(have.sum())
        # a tile that fell back to a coarser cut: the pair hangs below an entry of the list, which the ray reached no later than tnear says
        for j in np.nonzero(~have)[0]:
            a, found = int(par[j]), False
            live = codes[tile[j]][:int((codes[tile[j]] != EMPTY).argmin())]
            while a >= 0 and not found:
                w = np.nonzero(live == a)[0]
                if w.size:
                    assert reached[ray[j], a] and tnear[tile[j], w[0]] <= entry[ray[j], a], (int(ray[j]), a)
                    found = True
                a = int(parent[a])
            assert found, "ray %d (tile %d) reaches the child %d of node %d; neither it nor a node above it is in the tile's list %s" % (
                ray[j], tile[j], code[j], par[j], live)
            n_fallback += 1
    assert n_pairs > 1000, n_pairs
    print("%s: %d (ray, child) pairs held by their own entry, %d by an entry above them; cut %d" % (scene, n_pairs, n_fallback, cut))
