// rt_bvh_wide.hip -- the four-wide, quantised traversal layout (WNode, rt_internal.h).
//
// Input: a binary tree over the sorted leaves (the PLOC tree of rt_bvh_ploc.hip, or the canonical LBVH for a TLAS,
// tiny meshes and option fast_bvh=lbvh).  Output: nodes with up to RT_WIDE = FOUR children in one 64-B line.  Child boxes
// are quantised to one byte per plane on a power-of-two grid anchored at the node's own box: origin, three scales,
// 24 plane bytes and four child codes are 64 B.  (Eight children in a 128-B record of which the traversal reads 96 B --
// the L2 line and every fabric / HBM request are 128 B, profiles/r03/slab_fetch.txt, and the tree is a third shallower --
// was round 3's experiment: a third fewer steps, each nearly twice the arithmetic, 29 - 40 % slower;
// profiles/r03/wide8_experiment.md, experiments/r03_wide8.patch.  The code below is written in terms of RT_WIDE; three sizes are still
// those of the eight-wide layout and conservative for four, and each says so where it stands.)
//
// Collapse: breadth first, two launches per level and no host round trip inside a batch of levels (rt_level_scan.h).  A
// frontier element is a binary node that becomes a wide node: its two children are taken, and while fewer than RT_WIDE, the
// child with the largest surface that is not a leaf is replaced by its own two children (surface-area greedy, as in Wald
// et al. 2008 / Ylitie et al. 2017).  Node numbers come from prefix sums (deterministic), level after level, so the array
// is in breadth-first order and its first RT_TOP_NODES entries are the LDS-resident top of the traversal kernels; the
// internal children of a node have consecutive numbers in slot order.
//
// Slots: the children are packed at the front, larger surface first.  Any-hit rays visit the hit children in slot order
// (the likelier occluder first), closest-hit rays sort them by entry distance (rt_wide_step.h).
//
// Exactness: plane = fma(q, scale, origin) is evaluated here with the same expression the traversal uses; every lo
// plane is stepped down and every hi plane up until the decoded box CONTAINS the child's true box, and back in where a
// nearer plane still does: the planes are the tightest the grid has ("Quantiser").  The slab test is
// monotone under box inclusion (DESIGN.md "Exactness rule"), so culling against the decoded boxes never loses a
// candidate the canonical definition accepts.  An axis that cannot be quantised at all (non-finite or overflowing
// extents: huge instance boxes, NaN / inf vertices) gets an infinite scale and q = 0 planes: the decoded planes are
// NaN, which every slab test here ignores, i.e. that axis never culls -- slower, never wrong.
#include "rt_bvh_tree.h"

#include "rt_level_scan.h"

#include <cstddef>
#include <cstring>

namespace {

constexpr unsigned WB = 256;
constexpr uint32_t NO_KID = 0xFFFFFFFFu;
constexpr uint32_t RT_WIDE_MAX_LEVELS = 254;            // of wide nodes; a collapsed level spans one to two binary levels

// The surface-area-optimal collapse (Ylitie, Karras, Laine 2017, section 3.2), one record per internal binary node:
//   cost[i-1], i = 1 .. RT_WIDE: the cheapest way to represent the subtree as a forest of at most i roots (a root is a
//                                leaf or a wide node), in units of (half) surface area;
//   pick[i-1]:  how -- i = 1: 0 leaf, 1 wide node; i >= 2: 0 = as with i - 1 roots, k >= 1: k roots from the left child
//                                and i - k from the right;
//   spread:     the k of the best split of ALL RT_WIDE slots among the two children (what a wide node made of this
//                                binary node does with its slots).
// (conservative: eight costs and picks, of which RT_WIDE = 4 are used -- the eight-wide layout's record, six published words; kept as measured)
struct SahRecord { float cost[8]; uint8_t pick[8]; uint32_t spread; uint32_t pad; };      // 48 B
static_assert(sizeof(SahRecord) == 48 && RT_WIDE <= 8 && RT_WIDE % 2 == 0, "SahRecord layout");

// the binary tree (rt_bvh_tree.h) and what only the collapse knows of it
struct TreeView : BinTree {
    const SahRecord *sah;              // indexed by id - n; nullptr: the area-greedy collapse
    uint32_t leaf_max;
    __device__ bool may_be_leaf(uint32_t id) const { return id < n || (!leaf_prim && size[id] <= leaf_max); }
    __device__ bool is_leaf(uint32_t id) const
    {
        if (id < n) return true;
        if (sah) return sah[id - n].pick[0] == 0;
        return !leaf_prim && size[id] <= leaf_max;
    }
    __device__ int leaf_code(uint32_t id) const
    {
        return leaf_prim ? ~(int)leaf_prim[id] : ~(int)((offset[id] << 3) | (size[id] - 1u));
    }
};

// what the levels of one collapse share in device memory
struct WideLevel { uint32_t count, base; };                 // frontier size, index of its first wide node
struct WideState {
    uint32_t arrivals, error;
    uint32_t done, pad;                                     // levels below `done` were built by k_wide_top
    WideLevel level[RT_WIDE_MAX_LEVELS + 2];
};

// The roots the subtree of `id` contributes when it may use at most `budget` slots, appended to open[] (SAH collapse)
__device__ __forceinline__ void sah_roots(const TreeView &t, uint32_t first_id, uint32_t first_budget, uint32_t open[RT_WIDE], int &nk)
{
    uint32_t st_id[RT_WIDE], st_b[RT_WIDE];
    int sp = 0;
    st_id[0] = first_id; st_b[0] = first_budget; sp = 1;
    while (sp > 0) {
        sp--;
        const uint32_t id = st_id[sp];
        uint32_t i = st_b[sp];
        if (id < t.n) { open[nk++] = id; continue; }
        const SahRecord &r = t.sah[id - t.n];
        while (i > 1 && r.pick[i - 1] == 0) i--;
        if (i == 1) { open[nk++] = id; continue; }
        const uint32_t k = r.pick[i - 1];
        st_id[sp] = t.right[id - t.n]; st_b[sp] = i - k; sp++;       // (left is expanded first: deterministic order)
        st_id[sp] = t.left[id - t.n]; st_b[sp] = k; sp++;
    }
}

// the (up to RT_WIDE) children of frontier node b in their SLOTS (NO_KID: empty slot); returns how many of them are wide
// nodes themselves.
// (Fetching a child's own children's ids together with its size and box -- one trip less per opened child -- was measured:
// the large levels pay more for the extra loads than the small ones gain.)
__device__ __forceinline__ uint32_t expand_node(const TreeView &t, uint32_t b, uint32_t kid[RT_WIDE])
{
    uint32_t open[RT_WIDE];
    int nk = 0;
    if (t.sah) {
        const uint32_t k = t.sah[b - t.n].spread;
        sah_roots(t, t.left[b - t.n], k, open, nk);
        sah_roots(t, t.right[b - t.n], RT_WIDE - k, open, nk);
    } else {
        open[0] = t.left[b - t.n]; open[1] = t.right[b - t.n];
        nk = 2;
        while (nk < RT_WIDE) {
            int best = -1;
            float best_area = -1.0f;
            for (int k = 0; k < nk; k++) {
                if (t.is_leaf(open[k])) continue;
                const float a = box_area(t.box[open[k]]);
                if (a > best_area || best < 0) { best = k; best_area = a; }
            }
            if (best < 0) break;
            const uint32_t id = open[best];
            open[best] = t.left[id - t.n];
            open[nk++] = t.right[id - t.n];
        }
    }
    // (Filling the slots that are still free with the halves of multi-triangle leaves was measured on the four-wide layout:
    // 3 % fewer triangle tests, but more leaf visits, frame 2.67 -> 2.83 ms.)
    for (int k = 0; k < RT_WIDE; k++) kid[k] = NO_KID;
    // packed at the front, larger surface first (insertion sort, stable): any-hit rays walk in slot order
    float ar[RT_WIDE];
    for (int k = 0; k < nk; k++) { ar[k] = box_area(t.box[open[k]]); kid[k] = open[k]; }
    for (int i = 1; i < nk; i++)
        for (int j = i; j > 0 && ar[j] > ar[j - 1]; j--) {
            const float ta = ar[j]; ar[j] = ar[j - 1]; ar[j - 1] = ta;
            const uint32_t tk = kid[j]; kid[j] = kid[j - 1]; kid[j - 1] = tk;
        }
    uint32_t cnt = 0;
    for (int k = 0; k < RT_WIDE; k++)
        if (kid[k] != NO_KID && !t.is_leaf(kid[k])) cnt++;
    return cnt;
}

// The bottom-up pass of the SAH collapse: the climb of rt_bvh_tree.h ("the ordering of a bottom-up climb"), in the shape arrive, then
// publish.  At a parent the first arriver stops; the second fills the parent's record from its children's, publishes it and waits for the
// acknowledgement before it arrives at the next parent.  c_prim = cost of testing one primitive (a TLAS: of entering one instance).
__device__ __forceinline__ float leaf_sah(const TreeView &t, uint32_t id, float c_prim)
{
    return box_area(t.box[id]) * c_prim * (float)(t.leaf_prim ? 1u : t.size[id]);
}

__global__ void __launch_bounds__(WB) k_wide_sah(TreeView t, SahRecord *__restrict__ rec, uint32_t *__restrict__ arrive, float c_node, float c_prim)
{
    const uint32_t leaf = blockIdx.x * WB + threadIdx.x;
    if (leaf >= t.n) return;
    uint32_t cur = leaf;
    const float inf = __builtin_inff();
    for (;;) {
        const uint32_t p = t.parent[cur];
        if (p == 0xFFFFFFFFu) return;                       // cur is the root: its record is complete
        if (climb::arrive(&arrive[p - t.n]) == 0u) return;  // the sibling's climber takes over
        // both children are complete: cost tables of the two (a single primitive costs its leaf whatever the budget)
        float cl[RT_WIDE], cr[RT_WIDE];
        const uint32_t kids[2] = {t.left[p - t.n], t.right[p - t.n]};
        for (int side = 0; side < 2; side++) {
            float *c = side ? cr : cl;
            const uint32_t id = kids[side];
            if (id < t.n) {
                const float v = leaf_sah(t, id, c_prim);
                for (int i = 0; i < RT_WIDE; i++) c[i] = v;
            } else {
                const uint64_t *w = reinterpret_cast<const uint64_t *>(rec[id - t.n].cost);
                for (int i = 0; i < RT_WIDE / 2; i++) {
                    const uint64_t v = climb::load(&w[i]);
                    c[2 * i] = __uint_as_float((uint32_t)v); c[2 * i + 1] = __uint_as_float((uint32_t)(v >> 32));
                }
            }
        }
        // spread(j) = min over k of cl[k] + cr[j - k]: the subtree as j roots, k from the left and j - k from the right
        float cost[8];
        uint32_t pick[8];
        for (int i = 0; i < 8; i++) { cost[i] = inf; pick[i] = 0; }
        uint32_t spread_all = 1;
        for (int j = 2; j <= RT_WIDE; j++) {
            float best = inf;
            uint32_t bk = 1;
            for (int k = 1; k < j; k++) {
                const float v = cl[k - 1] + cr[j - k - 1];
                if (v < best || k == 1) { best = v; bk = (uint32_t)k; }
            }
            cost[j - 1] = best; pick[j - 1] = bk;            // (made monotone below)
            if (j == RT_WIDE) spread_all = bk;
        }
        const float as_node = box_area(t.box[p]) * c_node + cost[RT_WIDE - 1];
        const float as_leaf = t.may_be_leaf(p) ? leaf_sah(t, p, c_prim) : inf;
        // (a NaN cost -- NaN / inf geometry -- compares false everywhere: such a subtree becomes wide nodes down to its primitives)
        const bool leaf = t.may_be_leaf(p) && as_leaf <= as_node;
        cost[0] = leaf ? as_leaf : as_node;
        pick[0] = leaf ? 0u : 1u;
        for (int i = 2; i <= RT_WIDE; i++)
            if (!(cost[i - 1] < cost[i - 2])) { cost[i - 1] = cost[i - 2]; pick[i - 1] = 0u; }
        // publish, wait for the acknowledgement, go on to the parent
        SahRecord *mine = rec + (p - t.n);
        uint64_t *w = reinterpret_cast<uint64_t *>(mine->cost);
        for (int i = 0; i < 4; i++) climb::publish(&w[i], climb::pair(__float_as_uint(cost[2 * i]), __float_as_uint(cost[2 * i + 1])));
        uint64_t pk = 0;
        for (int i = 0; i < 8; i++) pk |= (uint64_t)(pick[i] & 0xffu) << (8 * i);
        climb::publish(&w[4], pk);
        climb::publish(&w[5], (uint64_t)spread_all);
        climb::wait_acknowledged();
        cur = p;
    }
}

// one frontier element -> its children; the workgroups' tallies of children that are wide nodes themselves become the
// offsets of the next frontier, and the last workgroup writes the next level's size
__global__ void __launch_bounds__(WB) k_wide_expand(TreeView t, const uint32_t *__restrict__ frontier, WideState *__restrict__ ws, uint32_t lvl,
                                                    uint32_t *__restrict__ kids, uint32_t *__restrict__ tally, uint32_t fcap)
{
    __shared__ uint32_t lds[WB];
    __shared__ uint32_t lds_flag;
    if (lvl < ws->done) return;                         // k_wide_top has been here
    const WideLevel L = ws->level[lvl];
    if (L.count == 0) {                                 // past the last level of this tree: hand the end on
        if (blockIdx.x == 0 && threadIdx.x == 0) ws->level[lvl + 1] = L;
        return;
    }
    const uint32_t nblocks = (L.count + WB - 1) / WB;
    if (blockIdx.x >= nblocks) return;
    const uint32_t f = blockIdx.x * WB + threadIdx.x;
    uint32_t cnt = 0;
    if (f < L.count) {
        uint32_t kid[RT_WIDE];
        cnt = expand_node(t, frontier[f], kid);
        for (int k = 0; k < RT_WIDE; k++) kids[RT_WIDE * (size_t)f + k] = kid[k];
    }
    uint32_t block_total;
    (void)rt_scan::block_exclusive<WB>(cnt, lds, block_total);
    if (!rt_scan::publish_and_arrive(tally, block_total, &ws->arrivals, nblocks, &lds_flag)) return;
    const uint32_t total = rt_scan::scan_tallies<uint32_t, WB>(tally, nblocks, lds);
    if (threadIdx.x == 0) {
        WideLevel nx = {total, L.base + L.count};
        if (lvl + 1 > RT_WIDE_MAX_LEVELS || total > fcap || (size_t)nx.base + total > (size_t)t.n - 1) {
            ws->error = 1 + lvl;                        // the host reports it
            nx.count = 0;
        }
        ws->level[lvl + 1] = nx;
        ws->arrivals = 0;
    }
}

// quantises the planes of one axis of the boxes in the slots of `valid` onto origin + q * scale; returns false if 255
// steps do not reach.  lo8 / hi8: one byte per slot, slot k in bits 8k..8k+7.
__device__ bool quantise_axis(const Box6 *cb, uint32_t valid, int axis, float origin, float scale, unsigned long long &lo8, unsigned long long &hi8)
{
    lo8 = 0; hi8 = 0;
    bool ok = true;
    for (int k = 0; k < RT_WIDE; k++) {
        int ql = 255, qh = 0;                           // unused slot: an inverted interval (never tested: not in the valid mask)
        if ((valid >> k) & 1u) {
            const float l = cb[k].lo[axis], h = cb[k].hi[axis];
            float fl = __builtin_floorf((l - origin) / scale), fh = __builtin_ceilf((h - origin) / scale);
            fl = fl > 0.0f ? (fl < 255.0f ? fl : 255.0f) : 0.0f;            // (NaN -> 0)
            fh = fh > 0.0f ? (fh < 255.0f ? fh : 255.0f) : 0.0f;
            ql = (int)fl; qh = (int)fh;
            float pl = __builtin_fmaf((float)ql, scale, origin), ph = __builtin_fmaf((float)qh, scale, origin);
            while (ql > 0 && pl > l) { ql--; pl = __builtin_fmaf((float)ql, scale, origin); }
            while (qh < 255 && ph < h) { qh++; ph = __builtin_fmaf((float)qh, scale, origin); }
            // ... and back in where that is tighter: l - origin and h - origin round, so floor / ceil can start one step further out than
            // the grid needs (the quotient is off by far less than a step, so the exact floor / ceil is at most one step in, and the plane
            // behind it may round onto l / h itself: two planes to look at).  A byte moves to the farther of them that still holds
            // the child and decodes to a DIFFERENT float -- not through planes that decode to the same one (zero extents, grids finer
            // than the floats far from the origin): those bytes are as tight as they get.  (One fma and a compare for nearly every
            // plane: the next one in is almost always past the child.)
            if (ql < 255) {
                const float p1 = __builtin_fmaf((float)(ql + 1), scale, origin);
                if (p1 <= l) {
                    const float p2 = __builtin_fmaf((float)(ql + 2), scale, origin);
                    if (ql + 2 <= 255 && p2 <= l && p2 > pl) { ql += 2; pl = p2; }
                    else if (p1 > pl) { ql += 1; pl = p1; }
                }
            }
            if (qh > 0) {
                const float p1 = __builtin_fmaf((float)(qh - 1), scale, origin);
                if (p1 >= h) {
                    const float p2 = __builtin_fmaf((float)(qh - 2), scale, origin);
                    if (qh - 2 >= 0 && p2 >= h && p2 < ph) { qh -= 2; ph = p2; }
                    else if (p1 < ph) { qh -= 1; ph = p1; }
                }
            }
            if (pl > l || ph < h) ok = false;
        }
        lo8 |= (unsigned long long)ql << (8 * k);
        hi8 |= (unsigned long long)qh << (8 * k);
    }
    return ok;
}

// writes wide node `node_index` for frontier node b with the children kid[] in their slots (internal ones: bits of
// `internal`), whose own wide nodes start at index `next_level_base + next` of the array (position `next` of the next frontier)
__device__ __forceinline__ void emit_node(const TreeView &t, uint32_t b, const uint32_t kid[RT_WIDE], uint32_t internal, uint32_t node_index,
                                          uint32_t next_level_base, uint32_t next, uint32_t *__restrict__ next_frontier, WNode *__restrict__ out)
{
    const Box6 nb = t.box[b];
    Box6 cb[RT_WIDE];
    int code[RT_WIDE];
    uint32_t valid = 0;
    for (int k = 0; k < RT_WIDE; k++) {
        const uint32_t id = kid[k];
        code[k] = RT_NODE_NONE;
        if (id == NO_KID) continue;
        valid |= 1u << k;
        cb[k] = t.box[id];
        if (!((internal >> k) & 1u)) code[k] = t.leaf_code(id);
        else {
            next_frontier[next] = id;
            code[k] = (int)(next_level_base + next);    // the next level starts right behind this one
            next++;
        }
    }
    float scale[3];
    unsigned long long lo8[3], hi8[3];
    for (int a = 0; a < 3; a++) {
        const float ext = nb.hi[a] - nb.lo[a];
        // smallest power of two s with 255 * s >= ext (a zero or denormal extent gets the smallest normal number)
        int e = 0;
        const float m = __builtin_frexpf(ext / 255.0f, &e);      // ext / 255 = m * 2^e, m in [0.5, 1)
        float s = (ext > 0.0f && ext < 3.0e38f) ? __builtin_ldexpf(1.0f, m == 0.5f ? e - 1 : e) : 1.17549435e-38f;
        if (!(s >= 1.17549435e-38f)) s = 1.17549435e-38f;
        bool ok = false;
        for (int tries = 0; tries < 8 && !ok; tries++) {
            ok = s < 1.0e38f && quantise_axis(cb, valid, a, nb.lo[a], s, lo8[a], hi8[a]);
            if (!ok) s = s * 2.0f;                      // rounding in fma left the last step short: coarser grid
        }
        scale[a] = s;
        if (!ok) {
            // not quantisable (non-finite or overflowing extents): an infinite scale with q = 0 planes --
            // fma(0, inf, origin) is NaN, which the slab tests ignore: this axis never culls
            scale[a] = __builtin_inff(); lo8[a] = 0; hi8[a] = 0;
        }
    }
    WNode w;
    w.q0 = make_float4(nb.lo[0], nb.lo[1], nb.lo[2], scale[0]);
    w.q1 = make_float4(__uint_as_float((uint32_t)lo8[0]), __uint_as_float((uint32_t)hi8[0]), __uint_as_float((uint32_t)lo8[1]), __uint_as_float((uint32_t)hi8[1]));
    w.q2 = make_float4(__uint_as_float((uint32_t)lo8[2]), __uint_as_float((uint32_t)hi8[2]), scale[1], scale[2]);
    w.q3 = make_float4(__int_as_float(code[0]), __int_as_float(code[1]), __int_as_float(code[2]), __int_as_float(code[3]));
    out[node_index] = w;
}


__global__ void __launch_bounds__(WB) k_wide_emit(TreeView t, const uint32_t *__restrict__ frontier, const WideState *__restrict__ ws, uint32_t lvl,
                                                  const uint32_t *__restrict__ kids, const uint32_t *__restrict__ tally,
                                                  uint32_t *__restrict__ next_frontier, WNode *__restrict__ out)
{
    __shared__ uint32_t lds[WB / 64];
    if (lvl < ws->done) return;
    const WideLevel L = ws->level[lvl];
    const uint32_t count = L.count, base = L.base;
    if (blockIdx.x * WB >= count) return;
    const uint32_t f = blockIdx.x * WB + threadIdx.x;
    uint32_t kid[RT_WIDE], internal = 0, mine = 0;
    for (int k = 0; k < RT_WIDE; k++) kid[k] = NO_KID;
    if (f < count)
        for (int k = 0; k < RT_WIDE; k++) {
            kid[k] = kids[RT_WIDE * (size_t)f + k];
            if (kid[k] != NO_KID && !t.is_leaf(kid[k])) { internal |= 1u << k; mine++; }
        }
    uint32_t block_total;
    const uint32_t next = tally[blockIdx.x] + rt_scan::block_exclusive<WB>(mine, lds, block_total);
    if (f >= count) return;
    emit_node(t, frontier[f], kid, internal, base + f, base + count, next, next_frontier, out);
}

// The top of the tree in ONE workgroup: while a level has at most TOPW nodes, expand, number and emit it between two
// barriers -- a level is ~6 dependent loads whatever its size, and as two launches each it cost 27 us.  Level l has at most
// RT_WIDE^l nodes, so levels 0 .. TOP_SURE-1 (at most 4^2 = 16 nodes) are certain to be handled here; the per-level launches start
// behind them and skip whatever else this kernel got to (ws->done).  (256 threads: the emit code wants 156 VGPRs, 1024 would spill.)
// (TOP_SURE conservative: RT_WIDE^4 = 256 = TOPW would allow 5 -- 3 is what 8^2 <= TOPW allowed the eight-wide layout; kept as measured)
constexpr uint32_t TOPW = 256, TOP_SURE = 3;
__global__ void __launch_bounds__(TOPW) k_wide_top(TreeView t, uint32_t *__restrict__ frontier0, uint32_t *__restrict__ frontier1,
                                                    WideState *__restrict__ ws, uint32_t root, uint32_t fcap, WNode *__restrict__ out)
{
    __shared__ uint32_t lds[TOPW / 64];
    uint32_t *frontier[2] = {frontier0, frontier1};
    uint32_t count = 1, base = 0, lvl = 0, error = 0;
    if (threadIdx.x == 0) frontier0[0] = root;
    __syncthreads();
    while (count > 0 && count <= TOPW) {
        const uint32_t f = threadIdx.x;
        uint32_t kid[RT_WIDE], internal = 0, mine = 0, b = 0;
        for (int k = 0; k < RT_WIDE; k++) kid[k] = NO_KID;
        if (f < count) {
            b = frontier[lvl & 1u][f];
            mine = expand_node(t, b, kid);
            for (int k = 0; k < RT_WIDE; k++)
                if (kid[k] != NO_KID && !t.is_leaf(kid[k])) internal |= 1u << k;
        }
        uint32_t total;
        const uint32_t next = rt_scan::block_exclusive<TOPW>(mine, lds, total);
        if (f < count) emit_node(t, b, kid, internal, base + f, base + count, next, frontier[(lvl & 1u) ^ 1u], out);
        if (threadIdx.x == 0) ws->level[lvl].count = count, ws->level[lvl].base = base;
        base += count;
        count = total;
        lvl++;
        if (lvl > RT_WIDE_MAX_LEVELS || count > fcap || (size_t)base + count > (size_t)t.n - 1) { error = lvl; count = 0; }
        __syncthreads();                                // the next frontier is in global memory: written above, read below
    }
    if (threadIdx.x == 0) {
        // (a tree that ends before level TOP_SURE -- where the per-level launches start -- has its end handed on to there)
        for (uint32_t l = lvl; l <= (count == 0 && lvl < TOP_SURE ? TOP_SURE : lvl); l++) { ws->level[l].count = count; ws->level[l].base = base; }
        ws->done = lvl;
        ws->arrivals = 0;
        ws->error = error;
    }
}

// canonical LBVH (rt_bvh_node[2n-1] + leaf ranges) -> cluster numbering: leaf k -> id k, internal c -> id n + c
__global__ void __launch_bounds__(WB) k_lbvh_to_tree(const rt_bvh_node *__restrict__ nodes, const uint2 *__restrict__ ranges, BinTree t)
{
    const uint32_t c = blockIdx.x * WB + threadIdx.x, n = t.n;
    if (c >= 2 * n - 1) return;
    const rt_bvh_node nd = nodes[c];
    const bool leaf = c >= n - 1;
    const uint32_t id = leaf ? c - (n - 1) : n + c;
    Box6 b;
    for (int k = 0; k < 3; k++) { b.lo[k] = nd.bmin[k]; b.hi[k] = nd.bmax[k]; }
    t.box[id] = b;
    if (leaf) {
        t.size[id] = 1; t.offset[id] = id;
        t.leaf_prim[id] = nd.left;
    } else {
        const uint2 r = ranges[c];
        t.size[id] = r.y - r.x + 1; t.offset[id] = r.x;
        const uint32_t l = nd.left >= n - 1 ? nd.left - (n - 1) : n + nd.left;
        const uint32_t r2 = nd.right >= n - 1 ? nd.right - (n - 1) : n + nd.right;
        t.left[c] = l; t.right[c] = r2;
        t.parent[l] = id; t.parent[r2] = id;
        if (c == 0) t.parent[id] = 0xFFFFFFFFu;
    }
}

// scratch of the collapse: two frontiers, the children of a frontier, one tally per workgroup of a level, the level table, and (option
// wide_sah) the cost records with their arrival counters
struct WideTemps {
    size_t fcap;                 // entries of a frontier
    uint32_t *frontier[2], *kids, *tally;
    WideState *ws;
    SahRecord *sah;
    uint32_t *arrive;
};
void carve_wide(Carver &c, uint32_t n, WideTemps &t)
{
    t.fcap = (size_t)n / 2 + 2;
    for (int k = 0; k < 2; k++) t.frontier[k] = c.take<uint32_t>(t.fcap);
    t.kids = c.take<uint32_t>(RT_WIDE * t.fcap);
    t.tally = c.take<uint32_t>(grid_for(t.fcap, WB));
    t.ws = c.take<WideState>(1);
    t.sah = c.take<SahRecord>(n);
    t.arrive = c.take<uint32_t>(n);
}

// the canonical LBVH as a tree in cluster numbering (rt_build_wide_from_lbvh), and behind it the scratch of its collapse
struct LbvhTreeTemps {
    BinTree tree;
    void *scratch; size_t scratch_bytes;
};
void carve_lbvh_tree(Carver &c, uint32_t n, LbvhTreeTemps &t)
{
    const size_t nn2 = 2 * (size_t)n - 1;
    t.tree.left = c.take<uint32_t>(n - 1); t.tree.right = c.take<uint32_t>(n - 1);
    t.tree.box = c.take<Box6>(nn2);
    t.tree.size = c.take<uint32_t>(nn2); t.tree.offset = c.take<uint32_t>(nn2);
    t.tree.leaf_prim = c.take<uint32_t>(nn2);
    t.tree.parent = c.take<uint32_t>(nn2);
    t.tree.n = n;
    t.scratch_bytes = rt_wide_temp_bytes(n);
    t.scratch = c.take<char>(t.scratch_bytes);
}

// the whole structure is one leaf of `count` primitives, the first ones: no node, and one WNode of room so that nobody holds a null array
int wide_single_leaf(BvhDev &bv, uint32_t count)
{
    bv.wide_n = 0;
    bv.root_code = ~(int)(count - 1);                  // leaf(first 0, count); a TLAS: instance 0
    bv.fast_depth = 0;
    return bv.wide.reserve(sizeof(WNode));
}

}  // namespace

size_t rt_wide_temp_bytes(uint32_t n)
{
    Carver sizing(nullptr);
    WideTemps t;
    carve_wide(sizing, n, t);
    return sizing.offset;
}

int rt_build_wide_layout(rt_context *ctx, BvhDev &bv, const BinTree &tree, uint32_t root, uint32_t leaf_max, void *tmp, size_t tmp_bytes)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = tree.n;
    TreeView t{tree, nullptr, leaf_max};
    bv.wide_n = 0;
    if (!tree.leaf_prim && n <= leaf_max) return wide_single_leaf(bv, n);      // a BLAS of <= leaf_max triangles
    DevBuf own;                        // only if the caller's slice is too small
    if (rt_wide_temp_bytes(n) > tmp_bytes) { RT_TRY(own.reserve(rt_wide_temp_bytes(n))); tmp = own.p; }
    Carver scratch(tmp);
    WideTemps w;
    carve_wide(scratch, n, w);
    const size_t fcap = w.fcap;
    uint32_t *const *frontier = w.frontier;
    RT_TRY(bv.wide.reserve(sizeof(WNode) * (size_t)(n - 1)));
    if (ctx->wide_sah) {
        // which binary nodes become wide nodes, which leaves, and how a wide node spends its slots: one bottom-up pass
        HIP_TRY(hipMemsetAsync(w.arrive, 0, 4 * (size_t)(n - 1), st));
        k_wide_sah<<<grid_for(n, WB), WB, 0, st>>>(t, w.sah, w.arrive, ctx->sah_node, ctx->sah_prim);
        t.sah = w.sah;
    }
    k_wide_top<<<1, TOPW, 0, st>>>(t, frontier[0], frontier[1], w.ws, root, (uint32_t)fcap, bv.wide.as<WNode>());
    // Levels are launched in batches without looking at their sizes: a level has at most RT_WIDE times the nodes of the
    // one before (and never more than fcap), a level past the end of the tree costs two empty launches.  The first batch is sized for
    // a binary tree half again as deep as a balanced one (log8: its depth in steps of three binary levels; a collapsed level spans one
    // to two); the host reads the level table after each batch.  k_wide_top has certainly built levels 0 .. TOP_SURE-1.
    uint32_t lvl = TOP_SURE, levels = 0, wide_n = 0;
    // upper bound of the frontier at level lvl (conservative: RT_WIDE^TOP_SURE = 64 would do; 2 * TOPW = 8^TOP_SURE is the eight-wide
    // layout's, and the workgroups it launches beyond a level's nodes leave at once; kept as measured)
    uint64_t bound = 2 * TOPW;
    uint32_t log8 = 0;
    for (uint32_t m = n; m > 1; m >>= 3) log8++;
    uint32_t batch = 4 + log8 + log8 / 2;
    batch = batch > TOP_SURE + 2 ? batch - TOP_SURE : 2; // (the first levels are k_wide_top's)
    if (ctx->build_batch) batch = ctx->build_batch;      // (tests: force short batches)
    WideState host_state;
    for (bool done = false; !done;) {
        const uint32_t end = lvl + batch < RT_WIDE_MAX_LEVELS + 1 ? lvl + batch : RT_WIDE_MAX_LEVELS + 1;
        for (; lvl < end; lvl++) {
            const unsigned blocks = grid_for((size_t)(bound < fcap ? bound : fcap), WB);
            k_wide_expand<<<blocks, WB, 0, st>>>(t, frontier[lvl & 1], w.ws, lvl, w.kids, w.tally, (uint32_t)fcap);
            k_wide_emit<<<blocks, WB, 0, st>>>(t, frontier[lvl & 1], w.ws, lvl, w.kids, w.tally, frontier[(lvl & 1) ^ 1], bv.wide.as<WNode>());
            bound = bound < fcap ? bound * RT_WIDE : fcap;
        }
        const size_t bytes = offsetof(WideState, level) + sizeof(WideLevel) * (lvl + 1);
        WideState *back = (ctx->pinned && bytes <= 64 * sizeof(uint32_t)) ? (WideState *)ctx->pinned : &host_state;      // page-locked: no staging copy
        HIP_TRY(hipMemcpyAsync(back, w.ws, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipGetLastError());
        const WideLevel *table = back->level;
        if (back->error) { rt_set_error("wide layout: the frontier of level %u does not fit (%u primitives)", back->error, n); return RT_ERR_STATE; }
        for (uint32_t l = 0; l <= lvl && !done; l++)
            if (table[l].count == 0) { levels = l; wide_n = table[l].base; done = true; }
        if (!done && lvl >= RT_WIDE_MAX_LEVELS + 1) { rt_set_error("wide layout: deeper than %u levels", RT_WIDE_MAX_LEVELS); return RT_ERR_STATE; }
        bound = table[lvl].count;
        batch = ctx->build_batch ? ctx->build_batch : 8;
    }
    bv.wide_n = wide_n;
    bv.root_code = 0;
    bv.fast_depth = (RT_WIDE - 1) * levels;        // a step leaves at most three siblings behind
    return RT_OK;
}

// arena bytes rt_build_wide_from_lbvh takes: the tree in cluster numbering + the scratch of the collapse
size_t rt_wide_lbvh_temp_bytes(uint32_t n)
{
    Carver sizing(nullptr);
    LbvhTreeTemps t;
    carve_lbvh_tree(sizing, n, t);
    return sizing.offset;
}

int rt_build_wide_from_lbvh(rt_context *ctx, BvhDev &bv, bool tlas, uint32_t leaf_max)
{
    const uint32_t n = bv.n;
    hipStream_t st = ctx->stream;
    if (n == 1) return wide_single_leaf(bv, 1);         // one primitive has no tree to convert (TLAS: instance 0; BLAS: triangle 0)
    RT_TRY(ctx->build_arena.reserve(rt_wide_lbvh_temp_bytes(n)));
    Carver arena(ctx->build_arena.p);
    LbvhTreeTemps t;
    carve_lbvh_tree(arena, n, t);
    k_lbvh_to_tree<<<grid_for(2 * (size_t)n - 1, WB), WB, 0, st>>>(bv.nodes.as<rt_bvh_node>(), bv.ranges.as<uint2>(), t.tree);
    HIP_TRY(hipGetLastError());
    if (!tlas) t.tree.leaf_prim = nullptr;             // (the leaves of a BLAS are records, not the primitives the conversion wrote there)
    return rt_build_wide_layout(ctx, bv, t.tree, n /* canonical root 0 */, tlas ? 1u : leaf_max, t.scratch, t.scratch_bytes);
}
