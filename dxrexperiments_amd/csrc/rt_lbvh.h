// rt_lbvh.h -- what the BLAS (rt_bvh_build.hip) and the TLAS (rt_scene.hip) share of the LBVH builder: the temporaries of a build, the
// encoding of bounds as inline device code, and the builder's host entry points (defined in rt_bvh_build.hip).  (Box6, grid_for: rt_bvh_tree.h)
#pragma once

#include "rt_bvh_tree.h"

// order-preserving float <-> uint map for atomicMin / atomicMax
__device__ __forceinline__ uint32_t f_enc(float f)
{
    uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f_dec(uint32_t k)
{
    uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(b);
}
#define ENC_POS_INF 0xFF800000u
#define ENC_NEG_INF 0x007FFFFFu

// Temporaries of an LBVH build over n primitives: slices of the context's build arena.  Every builder describes its slices once, to a
// Carver; the arena is sized by running the same description without a base (and for the larger of the LBVH and the PLOC / collapse
// phases, which run one after the other).
struct LbvhTemps {
    Box6 *boxes;
    uint32_t *enc;               // encoded bounds (k_init_bounds .. k_decode_bounds)
    float *bounds;
    uint64_t *keys;              // unsorted Morton keys
    void *sort; size_t sort_bytes;      // room for the radix sort's scratch: what rocPRIM asks for is only known from its query
    uint32_t *refit_enc, *depth;
};
inline void carve_lbvh(Carver &c, uint32_t n, LbvhTemps &t)
{
    t.boxes = c.take<Box6>(n);
    t.enc = c.take<uint32_t>(6);
    t.bounds = c.take<float>(6);
    t.keys = c.take<uint64_t>(n);
    t.sort_bytes = 16 * (size_t)n + (4u << 20);
    t.sort = c.take<char>(t.sort_bytes);
    t.refit_enc = c.take<uint32_t>(8 * (2 * (size_t)n - 1));
    t.depth = c.take<uint32_t>(1);
}
// (the BLAS adds its reference counts, BlasTemps; the TLAS the work memory of its record and world-box kernels, TlasTemps)
template <class Temps, class Carve> int take_build_temps(rt_context *ctx, uint32_t n, Temps &t, Carve carve)
{
    Carver sizing(nullptr);
    carve(sizing, t);
    const size_t ploc = rt_ploc_temp_bytes(n), wide = rt_wide_lbvh_temp_bytes(n);
    size_t most = sizing.offset > ploc ? sizing.offset : ploc;
    most = most > wide ? most : wide;
    RT_TRY(ctx->build_arena.reserve(most));
    Carver c(ctx->build_arena.p);
    carve(c, t);
    return RT_OK;
}

// queues the structure bounds of the n boxes in t.boxes, both corners of each, into t.bounds
void lbvh_queue_box_bounds(rt_context *ctx, uint32_t n, const LbvhTemps &t);
// queues the world boxes of the transformed instances an update lists (rt_scene.hip, k_update_records: its work list `items`, at most
// max_items of INST_BOX_REFS vertex references each) into `enc`, six encoded words per slot of the list.  The kernel reduces bounds as the
// builder's own two do and is compiled with them: alone in another file its instructions come out in another order
constexpr unsigned INST_BOX_REFS = 4096;
void lbvh_queue_instance_boxes(rt_context *ctx, uint32_t max_items, const InstanceRec *inst, const uint32_t *pend_idx, const float *pend_xf, const uint2 *items,
                               const uint32_t *n_items, uint32_t *enc);
// Steps 2..6 for a structure whose primitive boxes and bounds are already on the device.
int lbvh_from_boxes(rt_context *ctx, BvhDev &bv, uint32_t n, const LbvhTemps &t);
// joins the stream and takes the depth and bounds lbvh_from_boxes queued for read-back
int lbvh_collect(rt_context *ctx, BvhDev &bv);
