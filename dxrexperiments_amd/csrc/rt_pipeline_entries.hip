// rt_pipeline_entries.hip -- the entry lists of the primary stage, all but the walk that starts from them: when a set of launches
// has lists and how they are cut (rt_entries_choose), the kernel that makes them and its launch (rt_entries_launch), and the call
// that reads them back.  The walk's source is PrimaryEntrySrcT (rt_pipeline_rays.h), its kernel k_primary_from_entries (rt_pipeline.hip).
#include "rt_shade.h"
#include "rt_pipeline_queues.h"

namespace {

// ---- the entry lists of the primary stage ("entry lists") -------------------------------------------------------
// Once per set of launches, for every 8x8 tile of the launch's rectangle: which children below a cut through the top of the tree can
// ANY ray of the tile, in ANY frame of the set, be made to enter by the walk's own culling?  The 64 directions of a tile depend on the
// pixels alone and are the same in every frame (the host has checked that the frames share U, V, W bit for bit; otherwise the set runs
// without lists); the eye moves with the frame's jitter.  So the tile is the set of rays {o + t d : o in [olo, ohi], d in [dlo, dhi]}
// per axis, and a box is tested with an interval form of the slab test:
//   per axis whose direction interval excludes zero (mirrored so that d > 0: near plane lo, far plane hi),
//       tn = (lo - ohi) * (lo - ohi >= 0 ? 1 / dhi : 1 / dlo) - M        <= the near distance of every ray of the tile
//       tf = (hi - olo) * (hi - olo >= 0 ? 1 / dlo : 1 / dhi) + M        >= the far distance of every ray of the tile
//   LO = max(tn.., tmin = 0), HI = min(tf.., tmax);  the tile may hit the box iff  LO <= HI * RT_SLAB_SLACK.
// An axis whose interval contains zero, comes closer to it than 1e-12, or is not finite does not cull (tn = -inf, tf = +inf), and a NaN
// (an axis the builder could not quantise) is ignored by max / min as in wide_step.  Boxes are decoded as wide_step's exact path decodes
// them, fma(q, scale, origin).
// The margin.  What has to pass here is every box that wide_step lets some ray of the tile enter.  Its exact path (steep rays) runs the
// canonical slab test on the decoded box: each plane distance (p - o) * inv has two roundings, <= 2^-23 |t|.  Its quantised-frame path
// takes t(q) -+ D with |t(q) - canonical| <= D, so its near distance is >= canonical - 2 D and its far distance <= canonical + 2 D, where
//   D = 2^-20 (|B| + |inv| (|origin| + 255 scale)) + 1e-37,  |B| = |(origin - o) inv|.
// Over the tile |inv| <= 1 / dlo and |origin - o| <= max(|origin - olo|, |origin - ohi|) =: w, so
//   Dmax = 2^-20 / dlo * (w + |origin| + 255 scale) + 1e-37  >=  every ray's D,  and  >= 2^-20 |t| for every plane of the node
// (|p - o| <= w + 255 scale).  The arithmetic here adds four roundings of its own per bound (the difference, the reciprocal, the product,
// the subtraction of M: <= 2^-22 |t| <= Dmax / 4), and the intervals themselves are widened by 2^-20 of their ends before use, which moves
// a bound by less than 2^-19 |t| <= 2 Dmax.  M = 6 Dmax covers the sum (2 + 1/4 + 2) with room.  The same LO, being a lower bound of what
// either path of wide_step computes as the box's entry distance for any ray of the tile (and of the canonical entry distance), is the
// entry's tnear.
// The pass: nodes are numbered breadth first, children behind their parents, so one sweep over nodes 0 .. cut - 1 with a flag per node
// ("some ray of the tile may step on it") finds every child that hangs below the cut -- a node with index >= cut, or a leaf -- under a
// flagged parent.  Those are the entries; they are sorted by tnear (ties: the smaller HI first) when the sweep is over.  A tile with
// more than `cap` of them runs the sweep again with a quarter of the cut, in the end with the root alone.
// Both families of kernels stay live by design: k_primary / k_walk_primary, untouched, walk from the root (sets shorter than four frames by
// default, sets whose frames differ in U, V, W, two-level scenes, the persistent launch, primary_entries=0), k_primary_from_entries /
// k_walk_primary_from_entries walk from lists.  A trait inside k_primary would have saved the second template and changed the mangled names
// and the register allocation of the first; this way the off path is the parent's code, instruction for instruction.
// The launch: FOUR lanes per tile, one per child slot of the node at hand, 64 tiles (8 x 8 neighbours: what none of a wave's 8 x 2 can
// reach is skipped by the wave) per block; the nodes above the cut are copied into LDS once per block and read from there by all.  (One
// lane per tile reading the nodes from global memory, the first form, took 0.3 ms at 1080p -- one memory round trip per node and half
// the SIMDs empty; profiles/r18/primary_entries.txt.)  The lanes of a tile share its flags, its count and its list; whatever decides
// the control flow is the same in all four.
constexpr int EBLOCK = 256, ETILES = EBLOCK / 4;
__global__ void __launch_bounds__(EBLOCK) k_primary_entries(PipeDev pd, uint2 *__restrict__ entries, uint32_t cut, uint32_t cap)
{
    __shared__ float4 top[RT_ENTRY_CUT_MAX * 4u];
    __shared__ uint32_t flag[(RT_ENTRY_CUT_MAX / 32u) * ETILES];     // [word][tile]
    __shared__ uint2 list[RT_ENTRY_CAP * ETILES];                    // [entry][tile]: (code, tnear)
    __shared__ float list_hi[RT_ENTRY_CAP * ETILES];
    const uint32_t lane = threadIdx.x & 63u, k = threadIdx.x & 3u, tb = threadIdx.x >> 2;
    const uint32_t tiles_x = pd.tiles_x, tiles_y = (pd.fcap >> 6) / tiles_x;
    const uint32_t bw = (tiles_x + 7u) / 8u;
    const uint32_t tx = (blockIdx.x % bw) * 8u + (tb & 7u), ty = (blockIdx.x / bw) * 8u + (tb >> 3);
    const bool valid = tx < tiles_x && ty < tiles_y;
    const uint32_t tile = ty * tiles_x + tx;
    const InstanceRec *in0 = pd.sc.inst;
    const int root = in0->root_code;
    const float inf = __uint_as_float(0x7f800000u);
    const float k20 = 9.5367431640625e-07f;      // 2^-20
    const bool cuttable = root == 0 && cut != 0u;      // (a structure that is one leaf has no node to cut through)
    if (cuttable) {
        const float4 *__restrict__ nodes = (const float4 *)in0->wide;
        for (uint32_t i = threadIdx.x; i < cut * 4u; i += EBLOCK) top[i] = nodes[i];
    }
    __syncthreads();

    // the tile: direction intervals from the 64 slots (whatever pixel a slot of a partial tile names; 16 per lane), eye intervals from
    // the frames (one per lane of the wave)
    float dlo[3] = {inf, inf, inf}, dhi[3] = {-inf, -inf, -inf}, olo[3] = {inf, inf, inf}, ohi[3] = {-inf, -inf, -inf};
    const rt_camera_params &cam0 = pd.n_frames > 1u ? pd.pfcs[0].cameraParams : pd.pfc.cameraParams;
    int finite = 1;
    for (uint32_t w = k * 16u; w < k * 16u + 16u; w++) {
        uint32_t px, py;
        (void)pix_xy(pd, (valid ? tile : 0u) * 64u + w, px, py);
        const RayD r = primary_ray(pd, cam0, px, py);
        const float d[3] = {r.d.x, r.d.y, r.d.z};
        for (int a = 0; a < 3; a++) {
            dlo[a] = fmin2(dlo[a], d[a]); dhi[a] = fmax2(dhi[a], d[a]);
            if (!(__builtin_fabsf(d[a]) <= 3.0e38f)) finite = 0;
        }
    }
    if (lane < pd.n_frames) {
        const RayD r = primary_ray(pd, pd.n_frames > 1u ? pd.pfcs[lane].cameraParams : pd.pfc.cameraParams, pd.x0, pd.y0);
        const float o[3] = {r.o.x, r.o.y, r.o.z};
        for (int a = 0; a < 3; a++) {
            olo[a] = o[a]; ohi[a] = o[a];
            if (!(__builtin_fabsf(o[a]) <= 3.0e38f)) finite = 0;
        }
    }
    for (int a = 0; a < 3; a++) {
        for (int o = 1; o <= 2; o <<= 1) { dlo[a] = fmin2(dlo[a], __shfl_xor(dlo[a], o, 64)); dhi[a] = fmax2(dhi[a], __shfl_xor(dhi[a], o, 64)); }
        for (int o = 1; o < 64; o <<= 1) { olo[a] = fmin2(olo[a], __shfl_xor(olo[a], o, 64)); ohi[a] = fmax2(ohi[a], __shfl_xor(ohi[a], o, 64)); }
    }
    if (__ballot(finite == 0) != 0ull) finite = 0;      // (one bad lane: no axis of any tile of the wave culls)
    // per axis, mirrored so that the directions are positive: sgn = 0: the axis does not cull
    float sgn[3], eo_lo[3], eo_hi[3], inv_lo[3], inv_hi[3];
    for (int a = 0; a < 3; a++) {
        const float lo_w = olo[a] - (__builtin_fabsf(olo[a]) * k20 + 1.0e-30f), hi_w = ohi[a] + (__builtin_fabsf(ohi[a]) * k20 + 1.0e-30f);
        sgn[a] = !finite ? 0.0f : dlo[a] > 1.0e-12f ? 1.0f : dhi[a] < -1.0e-12f ? -1.0f : 0.0f;
        const float m_lo = sgn[a] < 0.0f ? -dhi[a] : dlo[a], m_hi = sgn[a] < 0.0f ? -dlo[a] : dhi[a];      // 0 < m_lo <= m_hi
        inv_hi[a] = 1.0f / (m_lo - m_lo * k20);
        inv_lo[a] = 1.0f / (m_hi + m_hi * k20);
        eo_lo[a] = sgn[a] < 0.0f ? -hi_w : lo_w;
        eo_hi[a] = sgn[a] < 0.0f ? -lo_w : hi_w;
    }

    // The four lanes of a tile talk through LDS with no barrier between them.  That relies on two things and on nothing else: a gfx9 wave
    // runs its lanes in lock-step and its LDS operations complete in program order, so a flag that lane k == 0 initialises (a volatile store)
    // or that any lane sets (atomicOr) is in LDS before the same wave's next volatile read of it; and a child's index is greater than its
    // parent's (breadth-first numbering), so the sweep reads a node's flag only after every step that can set it.  The lists are read
    // behind the block's barrier.  `pending`, `overflow`, `count` and `on` are per-lane copies of PER-TILE values: the four lanes compute each
    // from the same flags and from the same ballot masked to their own quad, so they agree by construction, and every branch on them is one
    // the quad takes together.
    volatile uint32_t *vflag = flag;
    const unsigned long long quad = 0xFull << (lane & ~3u);
    bool pending = valid && cuttable;
    uint32_t count = 0;
    for (uint32_t c = cut; __ballot(pending) != 0ull && c != 0u; c >>= 2) {
        bool overflow = false;
        if (pending) {
            if (k == 0u) for (uint32_t w = 0; w < (c + 31u) / 32u; w++) vflag[w * ETILES + tb] = w == 0u ? 1u : 0u;
            count = 0;
        }
        for (uint32_t i = 0; i < c; i++) {
            const bool on = pending && !overflow && ((vflag[(i >> 5) * ETILES + tb] >> (i & 31u)) & 1u) != 0u;
            if (__ballot(on) == 0ull) continue;
            const float4 q0 = top[4u * i], q1 = top[4u * i + 1u], q2 = top[4u * i + 2u], q3 = top[4u * i + 3u];
            const float org[3] = {q0.x, q0.y, q0.z}, scl[3] = {q0.w, q2.z, q2.w};
            const uint32_t lob[3] = {__float_as_uint(q1.x), __float_as_uint(q1.z), __float_as_uint(q2.x)};
            const uint32_t hib[3] = {__float_as_uint(q1.y), __float_as_uint(q1.w), __float_as_uint(q2.y)};
            const int code = k == 0u ? __float_as_int(q3.x) : k == 1u ? __float_as_int(q3.y) : k == 2u ? __float_as_int(q3.z) : __float_as_int(q3.w);
            float LO = 0.0f, HI = RAY_MAX_T;
            for (int a = 0; a < 3; a++) {
                if (sgn[a] == 0.0f) continue;
                const float w = fmax2(__builtin_fabsf(org[a] - olo[a]), __builtin_fabsf(org[a] - ohi[a]));
                const float margin = 6.0f * ((w + __builtin_fabsf(org[a]) + 255.0f * scl[a]) * inv_hi[a] * k20 + 1.0e-37f);
                const float bl = __builtin_fmaf((float)((lob[a] >> (8u * k)) & 0xffu), scl[a], org[a]);
                const float bh = __builtin_fmaf((float)((hib[a] >> (8u * k)) & 0xffu), scl[a], org[a]);
                const float pn = sgn[a] < 0.0f ? -bh : bl, pf = sgn[a] < 0.0f ? -bl : bh;
                const float nn = pn - eo_hi[a], nf = pf - eo_lo[a];
                const float tn = nn * (nn >= 0.0f ? inv_lo[a] : inv_hi[a]) - margin;
                const float tf = nf * (nf >= 0.0f ? inv_hi[a] : inv_lo[a]) + margin;
                LO = fmax2(LO, tn);
                HI = fmin2(HI, tf);
            }
            const bool hit = on && code != RT_NODE_NONE && LO <= HI * RT_SLAB_SLACK;
            const bool above = hit && code >= 0 && (uint32_t)code < c;
            if (above) atomicOr(&flag[((uint32_t)code >> 5) * ETILES + tb], 1u << ((uint32_t)code & 31u));
            const bool entry = hit && !above;
            const unsigned long long mine = __ballot(entry) & quad;
            const uint32_t n_new = (uint32_t)__popcll(mine);
            if (count + n_new > cap) overflow = true;
            else {
                if (entry) {
                    const uint32_t at = count + (uint32_t)__popcll(mine & lanemask_lt());
                    list[at * ETILES + tb] = make_uint2((uint32_t)code, __float_as_uint(LO));
                    list_hi[at * ETILES + tb] = HI;
                }
                count += n_new;
            }
        }
        pending = pending && overflow;
    }
    __syncthreads();
    if (!valid || k != 0u) return;
    uint2 *out = entries + (size_t)tile * RT_ENTRY_STRIDE;
    if (pending || !cuttable) {      // the coarsest list: the root, from the ray's start
        out[0] = make_uint2((uint32_t)root, 0u);
        count = 1;
    } else {
        for (uint32_t j = 1; j < count; j++) {      // insertion sort by (tnear, HI): a handful of entries per tile
            const uint2 e = list[j * ETILES + tb];
            const float eh = list_hi[j * ETILES + tb], et = __uint_as_float(e.y);
            uint32_t at = j;
            while (at > 0u) {
                const uint2 b = list[(at - 1u) * ETILES + tb];
                const float bh = list_hi[(at - 1u) * ETILES + tb], bt = __uint_as_float(b.y);
                if (bt < et || (bt == et && bh <= eh)) break;
                list[at * ETILES + tb] = b;
                list_hi[at * ETILES + tb] = bh;
                at--;
            }
            list[at * ETILES + tb] = e;
            list_hi[at * ETILES + tb] = eh;
        }
        for (uint32_t j = 0; j < count; j++) out[j] = list[j * ETILES + tb];
    }
    out[count] = make_uint2((uint32_t)RT_NODE_EMPTY, 0x7f800000u);
}

}  // namespace

// Whether the coming set (pd: its frames, slots and primary launch are in) starts its primary rays from lists, and if so the cut, the
// cap and room for the lists.  A tile's 64 directions must be the same in every frame of the set.
int rt_entries_choose(rt_pipeline *p, const PipeDev &pd, const rt_per_frame_constants *frames)
{
    const rt_context *ctx = p->ctx;
    rt_pipeline::PrimaryEntries &pe = p->primary_entries;
    // (auto: sets of at least RT_ENTRY_MIN_FRAMES frames.  The list kernel takes about 0.1 ms at 1080p and a frame's walk gains 0.07 ms: a
    // single frame with lists is 0.04 ms SLOWER than without, a set of 32 frames 2.2 ms faster: profiles/r18/primary_entries.txt)
    pe.on = !p->scene->two_level && !pd.primary_persistent &&
            (ctx->opt_primary_entries < 0 ? pd.sc.top_n != 0 && pd.n_frames >= RT_ENTRY_MIN_FRAMES : ctx->opt_primary_entries != 0);
    for (uint32_t f = 1; pe.on && f < pd.n_frames; f++)
        pe.on = memcmp(&frames[f].cameraParams.U, &frames[0].cameraParams.U, sizeof frames[0].cameraParams.U) == 0 &&
                memcmp(&frames[f].cameraParams.V, &frames[0].cameraParams.V, sizeof frames[0].cameraParams.V) == 0 &&
                memcmp(&frames[f].cameraParams.W, &frames[0].cameraParams.W, sizeof frames[0].cameraParams.W) == 0;
    // (the walk's source divides chunk by frames and tile by tiles_x with 32-bit reciprocals: recip32, PrimaryEntrySrcT.  plan_set's limit of
    // 2^30 slots bounds chunks x frames; tiles x tiles_x it bounds only for images up to 8192 tiles wide or so, hence the second test)
    if ((uint64_t)(pd.cap >> 6) * pd.n_frames >= 0x100000000ull || (uint64_t)(pd.fcap >> 6) * pd.tiles_x >= 0x100000000ull) pe.on = false;
    if (!pe.on) return RT_OK;
    const uint32_t n_nodes = p->scene->inst[0].model->blas.wide_n;
    pe.cut = ctx->opt_primary_entries_cut ? ctx->opt_primary_entries_cut : (uint32_t)RT_TOP_NODES;
    if (pe.cut > n_nodes) pe.cut = n_nodes;
    if (pe.cut > RT_ENTRY_CUT_MAX) pe.cut = RT_ENTRY_CUT_MAX;
    pe.cap = ctx->opt_primary_entries_cap ? ctx->opt_primary_entries_cap : RT_ENTRY_CAP;
    return pe.lists.reserve((size_t)(pd.fcap >> 6) * RT_ENTRY_STRIDE * sizeof(uint2));
}

// the lists of this set, made once for all its frames: 8 x 8 tiles per block
const uint2 *rt_entries_launch(rt_pipeline *p, const PipeDev &pd)
{
    const uint32_t tiles_y = (pd.fcap >> 6) / pd.tiles_x;
    uint2 *lists = p->primary_entries.lists.as<uint2>();
    k_primary_entries<<<((pd.tiles_x + 7u) / 8u) * ((tiles_y + 7u) / 8u), EBLOCK, 0, p->ctx->stream>>>(pd, lists, p->primary_entries.cut, p->primary_entries.cap);
    return lists;
}

extern "C" int rt_debug_read_primary_entries(rt_pipeline *p, uint32_t first_tile, uint32_t count, uint32_t *entries, uint32_t *n_tiles, uint32_t *cut)
{
    RT_REQUIRE(p, "null pipeline");
    RT_TRY(rt_pipeline_flush_pending(p));
    if (!p->rendered) { rt_set_error("nothing rendered yet"); return RT_ERR_STATE; }
    const uint32_t tiles = p->primary_entries.on ? p->last_pd.fcap >> 6 : 0u;
    if (n_tiles) *n_tiles = tiles;
    if (cut) *cut = p->primary_entries.on ? p->primary_entries.cut : 0u;
    if (!entries || count == 0) return RT_OK;
    RT_REQUIRE(first_tile < tiles && count <= tiles - first_tile, "tile out of range");
    RT_TRY(rt_use_device(p->ctx));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    HIP_TRY(hipMemcpy(entries, p->primary_entries.lists.as<uint2>() + (size_t)first_tile * RT_ENTRY_STRIDE, (size_t)count * RT_ENTRY_STRIDE * sizeof(uint2), hipMemcpyDeviceToHost));
    return RT_OK;
}

