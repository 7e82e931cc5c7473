// rt_crowd_ik.hip -- inverse kinematics for crowds (include/dxr_amd.h "Posed skeletons", crowds: rt_crowd_set_ik_chains,
// rt_crowd_solve_ik): every actor solves the crowd's ONE list of chains with its own targets, poles and weights, and is posed with the
// result, all actors in one launch.  The chains are the host's -- checked once against the skeleton's hierarchy (rt_skeleton_validate_ik)
// and packed into the table rt_skeleton_solve_ik packs (rt_skeleton_pack_ik) --, the values are arithmetic only and may stand in device
// memory.  The lane of a constraint is ik_solve_lane and the walk over the levels walk_levels, both rt_pose_device.h's and the very
// statements k_skeleton_ik and k_skeleton_pose run: actor a is, bit for bit, a skeleton given rt_skeleton_solve_ik with its values.
// A translation unit of its own beside rt_crowd.hip, which keeps the posing kernel and its two launches.  No reference counterpart, as for
// rt_skeleton.hip (libs/DXRFramework/RtModel.cpp:26 drops bones and node animation).
#include <new>

#include "rt_crowd_ik.h"
#include "rt_internal.h"
#include "rt_pose_device.h"

namespace {

using namespace rtd;

// every actor's values, [n_actors][n] entries each, in device memory: the caller's own (RT_MEM_DEVICE) or the crowd's copy of a host call's
struct CrowdIkValues {
    const float *targets;                // 3 floats an entry
    const float *poles;                  // 3 floats an entry; nullptr: the chains' own
    const float *weights;                // nullptr: the chains' own
};

// ONE block solves and poses ONE actor, blockIdx.x, as k_crowd_pose poses one (the block width and the LDS are that kernel's:
// rt_crowd_block, rt_crowd_lds_bytes).
//   Step 1: lane k < n of the block's first wave solves chain k.  It reads its entry where the table lies, in the kernel-argument segment,
//     by per-lane vector loads at 48 * lane as k_skeleton_ik does -- the by-value table is never copied to scratch
//     (tools/kernel_resources.py) --, then the three values of (actor, k), or the entry's defaults, and runs ik_solve_lane over the actor's
//     slices of `pose` and `joints`: W_p is what the last posing launch left there, exactly what k_skeleton_ik reads.  Every chain is solved
//     from the same input pose; the host has checked that no lane writes a joint another lane reads.  A value never becomes an address.
//   Step 2: one barrier.  The rewritten quaternions go through global memory to the lanes of other waves of the same block.
//   Step 3: phases 0 to 2 of k_crowd_pose with no layers: local_of the pose slice into LDS where W will stand, then walk_levels out to the
//     actor's slices of `joints` and `palette`.
// `pose` and `joints` are read and written in place: not __restrict__.
template <uint32_t BLOCK>
__global__ void __launch_bounds__(BLOCK) k_crowd_ik(const IkTable chains, uint32_t n, CrowdIkValues values, const uint32_t *__restrict__ table,
                                                    const uint32_t *__restrict__ level_offsets, uint32_t n_levels, uint32_t n_joints,
                                                    const float *__restrict__ inverse_bind, float *pose, float *joints, float *__restrict__ palette)
{
    extern __shared__ __align__(8) float s_dyn[];
    const uint32_t N = n_joints;
    float *s_w = s_dyn;                                          // [12][N]
    uint32_t *s_table = (uint32_t *)(s_w + 12u * (size_t)N);     // [N]
    uint32_t *s_off = s_table + N;                               // [n_levels + 1] (n_levels <= N)
    const PoseStorage<0> at = {s_w, s_table, s_off, N};
    const uint32_t tid = threadIdx.x, actor = blockIdx.x;
    pose += RT_SKELETON_POSE_FLOATS * (size_t)N * actor;
    joints += 12u * (size_t)N * actor;
    palette += 12u * (size_t)N * actor;
    if (tid < n) {                                               // (n <= RT_SKELETON_MAX_IK < a wave)
        const IkEntry &e = chains.e[tid];
        const uint32_t kind = e.kind, jc = e.c, jb = e.b, ja = e.a;
        const int32_t jp = e.p;
        const size_t mine = (size_t)actor * n + tid;
        float target[3], pole[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            target[c] = values.targets[3u * mine + c];
            pole[c] = values.poles ? values.poles[3u * mine + c] : e.pole[c];
        }
        const float weight = values.weights ? values.weights[mine] : e.weight;
        ik_solve_lane(kind, jc, jb, ja, jp, target, pole, weight, joints, pose);
    }
    __syncthreads();
    for (uint32_t j = tid; j < n_joints; j += BLOCK) {
        float L[12];
        local_of(pose + RT_SKELETON_POSE_FLOATS * (size_t)j, L);
        at.store(j, L);
        s_table[j] = table[j];
    }
    for (uint32_t l = tid; l <= n_levels; l += BLOCK) s_off[l] = level_offsets[l];
    __syncthreads();
    walk_levels<BLOCK, true>(at, n_levels, n_joints, inverse_bind, joints, palette);
}

template <uint32_t BLOCK>
void launch_ik(rt_crowd *c, const CrowdIkValues &values)
{
    const rt_skeleton *sk = c->sk;
    k_crowd_ik<BLOCK><<<c->n_poses, BLOCK, rt_crowd_lds_bytes(c->n_joints), c->ctx->stream>>>(
        c->ik_chains, c->n_ik_chains, values, sk->table.as<uint32_t>(), sk->d_level_offsets.as<uint32_t>(), sk->n_levels, c->n_joints, sk->inverse_bind.as<float>(),
        c->pose.as<float>(), c->joints.as<float>(), c->palette.as<float>());
}

// the values stand in device memory: ONE launch, queued on the context's stream -- of k_crowd_ik for a list of one group, of k_ik_groups
// (rt_ik_groups.hip) for an ordered list of several
int solve_crowd(rt_crowd *c, const CrowdIkValues &values)
{
    if (c->n_ik_groups > 1u) return rt_ik_groups_solve_crowd(c, values.targets, values.poles, values.weights);
    const uint32_t block = rt_crowd_block(c->n_joints);
    if (block == 64u) launch_ik<64>(c, values);
    else if (block == 128u) launch_ik<128>(c, values);
    else launch_ik<256>(c, values);
    HIP_TRY(hipGetLastError());
    c->queued();              // (once for the whole crowd)
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_crowd_set_ik_chains(rt_crowd *c, uint32_t n, const rt_skeleton_ik *chains)
{
    RT_REQUIRE(c && chains, "null argument");
    const int32_t *parents = c->sk->parents.data();
    uint32_t bad[3] = {0, 0, 0};
    if (n < 1u || n > RT_SKELETON_MAX_IK)                 // (refuses, and reads no entry)
        return rt_pose_refuse_ik(c, "rt_crowd_set_ik_chains", rt_skeleton_validate_ik(n, chains, c->n_joints, parents, true, bad), n, chains, bad);
    rt_skeleton_ik mine[RT_SKELETON_MAX_IK];              // the caller's list without its targets
    rt_crowd_ik_chains(n, chains, mine);
    const int what = rt_skeleton_validate_ik(n, mine, c->n_joints, parents, true, bad);      // (a list needs no pose: `posed` is taken as true)
    if (what) return rt_pose_refuse_ik(c, "rt_crowd_set_ik_chains", what, n, mine, bad);
    // by value into the crowd: a launch already queued holds its own copy of the table it was given, in its kernel arguments
    rt_skeleton_pack_ik(n, mine, parents, c->ik_chains);
    c->n_ik_chains = n;
    c->ik_group_ends = rt_ik_group_ends(1u, &n);          // (a list of one group)
    c->n_ik_groups = 1u;
    return RT_OK;
}

int rt_crowd_get_ik_chains(const rt_crowd *c, uint32_t *n)
{
    RT_REQUIRE(c && n, "null argument");
    *n = c->n_ik_chains;
    return RT_OK;
}

int rt_crowd_solve_ik(rt_crowd *c, const float *targets, const float *poles, const float *weights, uint32_t mem)
{
    RT_REQUIRE(c && targets, "null argument");
    RT_REQUIRE(mem == RT_MEM_HOST || mem == RT_MEM_DEVICE, "unknown memory selector");
    if (c->n_ik_chains == 0u) {
        rt_set_error("rt_crowd_solve_ik: the crowd has no chains (rt_crowd_set_ik_chains gives it a list)");
        return RT_ERR_STATE;
    }
    RT_TRY(rt_pose_require(c, "rt_crowd_solve_ik"));
    const uint32_t n = c->n_ik_chains;
    if (mem == RT_MEM_DEVICE) {
        RT_TRY(rt_use_device(c->ctx));
        return solve_crowd(c, CrowdIkValues{targets, poles, weights});
    }
    uint32_t actor = 0, bad = 0;
    if (rt_crowd_ik_check_values(c->n_poses, n, weights, &actor, &bad)) {
        rt_set_error("rt_crowd_solve_ik: actor %u: the weight of constraint %u is NaN", actor, bad);
        return RT_ERR_INVALID_ARG;
    }
    // the arrays the call brings, one behind another in one staging slot: the one upload of the call
    const rt_crowd_ik_block b = rt_crowd_ik_layout(c->n_poses, n, poles != nullptr, weights != nullptr);
    const size_t bytes = sizeof(float) * b.floats;
    rt_context *ctx = c->ctx;
    RT_TRY(rt_use_device(ctx));
    // (what can refuse comes first, as in rt_crowd_set_blend: a buffer that cannot grow keeps what it has, and nothing has changed)
    RT_TRY(c->ik_values.reserve(bytes));
    CrowdStage *s = nullptr;
    RT_TRY(crowd_stage(c, bytes, &s));
    rt_crowd_ik_pack_values(c->n_poses, n, b, targets, poles, weights, (float *)s->block);
    HIP_TRY(hipMemcpyAsync(c->ik_values.p, s->block, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(s->event, ctx->stream));
    s->in_flight = true;
    const float *base = c->ik_values.as<float>();
    return solve_crowd(c, CrowdIkValues{base, b.has_poles ? base + b.poles : nullptr, b.has_weights ? base + b.weights : nullptr});
}

}  // extern "C"
