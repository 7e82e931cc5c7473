// rt_ik_groups.hip -- ordered groups of IK constraints solved in one launch (include/dxr_amd.h "Posed skeletons", inverse kinematics, groups:
// rt_skeleton_solve_ik_groups, rt_crowd_set_ik_chain_groups, rt_crowd_get_ik_chain_groups): a hand aimed at what its arm has just reached
// for, a foot aimed after its leg is planted.  The constraints of a group are independent and are solved side by side; a later group reads
// the world matrices of the pose the earlier groups left, so between two groups the pose is walked -- inside the kernel, one block per
// actor, with barriers where a skeleton would take two launches per group.  The lane of a constraint is ik_solve_lane and the walk
// walk_levels, both rt_pose_device.h's and the very statements k_skeleton_ik, k_crowd_ik and the pose kernels run: a grouped solve is, bit
// for bit, one rt_skeleton_solve_ik per group in order.  The check and the group ends are rt_ik_groups.h's, the packed table
// rt_skeleton.h's.  No reference counterpart, as for rt_skeleton.hip (libs/DXRFramework/RtModel.cpp:26 drops bones and node animation).
#include <new>

#include "rt_crowd_ik.h"
#include "rt_ik_groups.h"
#include "rt_internal.h"
#include "rt_pose_device.h"

namespace {

using namespace rtd;

// ONE block solves and poses ONE actor, blockIdx.x, stage after stage (the block width and the LDS are k_crowd_pose's: rt_crowd_block,
// rt_crowd_lds_bytes).  `ends`: byte g is the list index one past group g's last constraint (rt_ik_group_ends).
//   Entry read: lane k < n of the block's first wave reads its entry ONCE, before the loop, where the table lies -- in the kernel-argument
//     segment, by per-lane vector loads at 48 * lane as k_skeleton_ik does: the by-value table is never copied to scratch
//     (tools/kernel_resources.py) -- and the three values of (actor, k).  A null `targets` means the entry's own target, pole and weight:
//     the skeleton's form, one block over the skeleton's own buffers.  A value never becomes an address.
//   Group loop, g = 0 .. n_groups - 1 (uniform; every barrier stands outside divergent code):
//     1: the lanes of group g run ik_solve_lane over the actor's slices of `pose` and `joints` in global memory: W_p is what the walk of
//        the stage before left there (stage 0: the last posing launch).
//     2: barrier.  The rewritten quaternions go through global memory to the lanes of other waves of the same block.
//     3: local_of the pose slice into LDS where W will stand (stage 0 also loads the level table and the level offsets, once).
//     4: barrier.
//     5: walk_levels out to the actor's slices of `joints` and `palette`.
//     6: barrier, so that the next stage's lanes see the new W.
// Every stage walks the whole pose and writes joints and palette whole, as rt_skeleton_solve_ik's pose launch does.  `pose` and `joints` are
// read and written in place: not __restrict__.
template <uint32_t BLOCK>
__global__ void __launch_bounds__(BLOCK) k_ik_groups(const IkTable chains, uint32_t n, uint64_t ends, uint32_t n_groups, const float *targets, const float *poles,
                                                     const float *weights, const uint32_t *__restrict__ table, const uint32_t *__restrict__ level_offsets,
                                                     uint32_t n_levels, uint32_t n_joints, const float *__restrict__ inverse_bind, float *pose, float *joints,
                                                     float *__restrict__ palette)
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
    uint32_t kind = RT_IK_AIM, jc = 0u, jb = 0u, ja = 0u;
    int32_t jp = -1;
    float target[3] = {0.0f, 0.0f, 0.0f}, pole[3] = {0.0f, 0.0f, 0.0f}, weight = 0.0f;
    if (tid < n) {                                               // (n <= RT_SKELETON_MAX_IK < a wave)
        const IkEntry &e = chains.e[tid];
        kind = e.kind; jc = e.c; jb = e.b; ja = e.a;
        jp = e.p;
        const size_t mine = (size_t)actor * n + tid;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            target[c] = targets ? targets[3u * mine + c] : e.target[c];
            pole[c] = poles ? poles[3u * mine + c] : e.pole[c];
        }
        weight = weights ? weights[mine] : e.weight;
    }
    uint32_t first = 0u;
    for (uint32_t g = 0; g < n_groups; g++) {                    // (uniform: every lane passes every barrier)
        const uint32_t end = (uint32_t)(ends >> (8u * g)) & 0xFFu;
        if (tid >= first && tid < end && tid < n) ik_solve_lane(kind, jc, jb, ja, jp, target, pole, weight, joints, pose);
        first = end;
        __syncthreads();
        for (uint32_t j = tid; j < n_joints; j += BLOCK) {
            float L[12];
            local_of(pose + RT_SKELETON_POSE_FLOATS * (size_t)j, L);
            at.store(j, L);
            if (g == 0u) s_table[j] = table[j];
        }
        if (g == 0u)
            for (uint32_t l = tid; l <= n_levels; l += BLOCK) s_off[l] = level_offsets[l];
        __syncthreads();
        walk_levels<BLOCK, true>(at, n_levels, n_joints, inverse_bind, joints, palette);
        __syncthreads();
    }
}

// what a launch solves: a packed table, how many entries of it, where its groups end and how many there are
struct GroupedList {
    const IkTable &table;
    uint32_t n;
    uint64_t ends;
    uint32_t n_groups;
};

// ONE launch over n_poses poses of the skeleton `sk`'s rig, queued on the context's stream: a crowd's actors with their values in device
// memory, or (null values) the skeleton's own one pose
int launch_groups(rt_pose_source *src, const rt_skeleton *sk, const GroupedList &l, const float *targets, const float *poles, const float *weights)
{
    const uint32_t N = src->n_joints;
    const size_t lds = rt_crowd_lds_bytes(N);
    hipStream_t st = src->ctx->stream;
    const uint32_t *table = sk->table.as<uint32_t>(), *off = sk->d_level_offsets.as<uint32_t>();
    const float *ib = sk->inverse_bind.as<float>();
    float *pose = src->pose.as<float>(), *joints = src->joints.as<float>(), *palette = src->palette.as<float>();
#define RT_IK_GROUPS_LAUNCH(B) \
    k_ik_groups<B><<<src->n_poses, B, lds, st>>>(l.table, l.n, l.ends, l.n_groups, targets, poles, weights, table, off, sk->n_levels, N, ib, pose, joints, palette)
    const uint32_t block = rt_crowd_block(N);
    if (block == 64u) RT_IK_GROUPS_LAUNCH(64);
    else if (block == 128u) RT_IK_GROUPS_LAUNCH(128);
    else RT_IK_GROUPS_LAUNCH(256);
#undef RT_IK_GROUPS_LAUNCH
    HIP_TRY(hipGetLastError());
    src->queued();            // (once for the whole call)
    return RT_OK;
}

// the refusal behind a code of rt_ik_groups_validate as the last error; its class
int refuse(const rt_pose_source *src, const char *who, int what, uint32_t n_groups, uint32_t total, const rt_skeleton_ik *constraints, const uint32_t bad[4])
{
    char msg[512];
    const int rc = rt_ik_groups_refusal(what, who, n_groups, total, constraints, bad, src->n_joints, src->noun(), src->pose_hint(), msg, sizeof msg);
    rt_set_error("%s", msg);
    return rc;
}

}  // namespace

int rt_ik_groups_solve_crowd(rt_crowd *c, const float *targets, const float *poles, const float *weights)
{
    return launch_groups(c, c->sk, GroupedList{c->ik_chains, c->n_ik_chains, c->ik_group_ends, c->n_ik_groups}, targets, poles, weights);
}

extern "C" {

int rt_skeleton_solve_ik_groups(rt_skeleton *sk, uint32_t n_groups, const uint32_t *group_sizes, const rt_skeleton_ik *constraints)
{
    RT_REQUIRE(sk && group_sizes && constraints, "null argument");
    const int32_t *parents = sk->parents.data();
    uint32_t bad[4] = {0, 0, 0, 0}, total = 0;
    const int what = rt_ik_groups_validate(n_groups, group_sizes, constraints, sk->n_joints, parents, sk->posed, &total, bad);
    if (what) return refuse(sk, "rt_skeleton_solve_ik_groups", what, n_groups, total, constraints, bad);
    if (sk->n_joints > RT_SKELETON_LDS_JOINTS) {         // W does not fit LDS: the groups one by one, two launches each
        uint32_t first = 0;
        for (uint32_t g = 0; g < n_groups; first += group_sizes[g++]) RT_TRY(rt_skeleton_solve_ik(sk, group_sizes[g], constraints + first));
        return RT_OK;
    }
    IkTable table = {};
    rt_skeleton_pack_ik(total, constraints, parents, table);
    RT_TRY(rt_use_device(sk->ctx));
    return launch_groups(sk, sk, GroupedList{table, total, rt_ik_group_ends(n_groups, group_sizes), n_groups}, nullptr, nullptr, nullptr);
}

int rt_crowd_set_ik_chain_groups(rt_crowd *c, uint32_t n_groups, const uint32_t *group_sizes, const rt_skeleton_ik *chains)
{
    RT_REQUIRE(c && group_sizes && chains, "null argument");
    const int32_t *parents = c->sk->parents.data();
    uint32_t bad[4] = {0, 0, 0, 0}, total = 0;
    // (a list needs no pose: `posed` is taken as true; the check reads no target)
    const int what = rt_ik_groups_validate(n_groups, group_sizes, chains, c->n_joints, parents, true, &total, bad);
    if (what) return refuse(c, "rt_crowd_set_ik_chain_groups", what, n_groups, total, chains, bad);
    rt_skeleton_ik mine[RT_SKELETON_MAX_IK];              // the caller's list without its targets
    rt_crowd_ik_chains(total, chains, mine);
    // by value into the crowd: a launch already queued holds its own copy of the table and the ends it was given, in its kernel arguments
    rt_skeleton_pack_ik(total, mine, parents, c->ik_chains);
    c->n_ik_chains = total;
    c->ik_group_ends = rt_ik_group_ends(n_groups, group_sizes);
    c->n_ik_groups = n_groups;
    return RT_OK;
}

int rt_crowd_get_ik_chain_groups(const rt_crowd *c, uint32_t *n_groups, uint32_t *group_sizes)
{
    RT_REQUIRE(c && n_groups, "null argument");
    *n_groups = c->n_ik_groups;
    if (group_sizes) rt_ik_group_sizes(c->ik_group_ends, c->n_ik_groups, group_sizes);
    return RT_OK;
}

}  // extern "C"
