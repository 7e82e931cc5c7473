// rt_pose_device.h -- the device side of a pose (include/dxr_amd.h "Posed skeletons": local, product, sampling, blending; the walk over the
// levels and the palette step, over whichever storage holds W; the lane of an IK constraint), each function written ONCE for the translation
// units that pose: rt_skeleton.hip (one skeleton, one pose), rt_crowd.hip and rt_crowd_ik.hip (n_actors poses of one skeleton).  Actor a of a crowd is, bit for bit, a
// skeleton given the same call because both run these statements and no others; a kernel of either keeps only its own phase 0.
#pragma once

#include "rt_device_math.h"
#include "rt_ik.h"
#include "rt_skeleton.h"

namespace rtd {

// The local matrix of a joint, T.R.S, from its ten floats tx ty tz  qx qy qz qw  sx sy sz: the quaternion as given, never normalised.
RT_DEV void local_of(const float *__restrict__ trs, float L[12])
{
    const float x = trs[3], y = trs[4], z = trs[5], w = trs[6];
    const float sx = trs[7], sy = trs[8], sz = trs[9];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    L[0] = (1.0f - 2.0f * (yy + zz)) * sx; L[1] = (2.0f * (xy - wz)) * sy;        L[2] = (2.0f * (xz + wy)) * sz;         L[3] = trs[0];
    L[4] = (2.0f * (xy + wz)) * sx;        L[5] = (1.0f - 2.0f * (xx + zz)) * sy; L[6] = (2.0f * (yz - wx)) * sz;         L[7] = trs[1];
    L[8] = (2.0f * (xz - wy)) * sx;        L[9] = (2.0f * (yz + wx)) * sy;        L[10] = (1.0f - 2.0f * (xx + yy)) * sz; L[11] = trs[2];
}

// C = A o B of two 3x4 affine matrices, grouped as the header groups it
RT_DEV void compose(const float A[12], const float B[12], float C[12])
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float a0 = A[4 * r], a1 = A[4 * r + 1], a2 = A[4 * r + 2], a3 = A[4 * r + 3];
#pragma unroll
        for (int c = 0; c < 3; c++) C[4 * r + c] = (a0 * B[c] + a1 * B[4 + c]) + a2 * B[8 + c];
        C[4 * r + 3] = ((a0 * B[3] + a1 * B[7]) + a2 * B[11]) + a3;
    }
}

// The quaternion q[0 .. 3] = (x, y, z, w) normalised by the rule of rt_model_recompute_normals, with (0, 0, 0, 1) where that has no answer
RT_DEV void unit_or_identity(float q[4])
{
    const float n = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (n > 0.0f && n < __uint_as_float(0x7f800000u)) {
        const float inv = rsqrt_ieee(n);
#pragma unroll
        for (int c = 0; c < 4; c++) q[c] = q[c] * inv;
    } else {
        q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f; q[3] = 1.0f;
    }
}

// The local pose of joint j between two keys of a clip.  A key is component major (float[10][n_joints]): at every one of the twenty loads the
// lanes of a wave read 64 consecutive floats.  Translation and scale A + (a * (B - A)); the quaternion the same after B has been turned onto
// A's side (d < 0; a NaN d turns nothing), then normalised.
RT_DEV void sample_joint(const float *__restrict__ key_a, const float *__restrict__ key_b, uint32_t n_joints, uint32_t j, float a, float o[10])
{
    float A[10], B[10];
#pragma unroll
    for (int c = 0; c < 10; c++) {
        A[c] = key_a[(size_t)c * n_joints + j];
        B[c] = key_b[(size_t)c * n_joints + j];
    }
    const float d = ((A[3] * B[3] + A[4] * B[4]) + A[5] * B[5]) + A[6] * B[6];
    if (d < 0.0f) {
#pragma unroll
        for (int c = 3; c < 7; c++) B[c] = -B[c];
    }
#pragma unroll
    for (int c = 0; c < 10; c++) o[c] = A[c] + a * (B[c] - A[c]);
    unit_or_identity(o + 3);
}

// the Hamilton product r = p (x) q of quaternions (x, y, z, w), grouped as the header groups it
RT_DEV void hamilton(const float p[4], const float q[4], float r[4])
{
    r[0] = ((p[3] * q[0] + p[0] * q[3]) + p[1] * q[2]) - p[2] * q[1];
    r[1] = ((p[3] * q[1] - p[0] * q[2]) + p[1] * q[3]) + p[2] * q[0];
    r[2] = ((p[3] * q[2] + p[0] * q[1]) - p[1] * q[0]) + p[2] * q[3];
    r[3] = ((p[3] * q[3] - p[0] * q[0]) - p[1] * q[1]) - p[2] * q[2];
}

// One layer k >= 1 of a blend on joint j: sampled as sample_joint samples and blended into, or added onto, the accumulated pose P with
// w = weight (* mask[j]).  `l` is uniform over the wave -- a kernel argument, or a record read through a uniform address -- so the branch
// on its mode is a scalar branch.  P, S and R live in registers.
RT_DEV void blend_layer(const rt_blend_layer &l, uint32_t n_joints, uint32_t j, float P[10])
{
    float S[10];
    sample_joint(l.key_a, l.key_b, n_joints, j, l.a, S);
    const float w = l.mask ? l.weight * l.mask[j] : l.weight;
    if (l.mode == RT_LAYER_ADDITIVE) {
        float R[10], cr[4], D[4], E[4], q[4];
        sample_joint(l.ref_a, l.ref_b, n_joints, j, 0.0f, R);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            P[c] = P[c] + w * (S[c] - R[c]);
            P[7 + c] = P[7 + c] + w * (S[7 + c] - R[7 + c]);
        }
        cr[0] = -R[3]; cr[1] = -R[4]; cr[2] = -R[5]; cr[3] = R[6];
        hamilton(cr, S + 3, D);
        if (D[3] < 0.0f) {
#pragma unroll
            for (int c = 0; c < 4; c++) D[c] = -D[c];
        }
        E[0] = w * D[0]; E[1] = w * D[1]; E[2] = w * D[2];
        E[3] = 1.0f + w * (D[3] - 1.0f);
        unit_or_identity(E);
        hamilton(P + 3, E, q);
        unit_or_identity(q);
#pragma unroll
        for (int c = 0; c < 4; c++) P[3 + c] = q[c];
    } else {
        const float d = ((P[3] * S[3] + P[4] * S[4]) + P[5] * S[5]) + P[6] * S[6];
        if (d < 0.0f) {
#pragma unroll
            for (int c = 3; c < 7; c++) S[c] = -S[c];
        }
#pragma unroll
        for (int c = 0; c < 10; c++) P[c] = P[c] + w * (S[c] - P[c]);
        unit_or_identity(P + 3);
    }
}

// The accumulated pose of joint j under `n_layers` layers: P starts as layer 0's sample, or (key_a == nullptr: RT_SKELETON_CURRENT_POSE) as
// the stored pose `held`, ten floats that this lane alone reads and, afterwards, overwrites; every later layer goes through blend_layer.
// The loop over the layers is uniform.
RT_DEV void blend_joint(const rt_blend_layer *layers, uint32_t n_layers, uint32_t n_joints, uint32_t j, const float *held, float P[10])
{
    if (layers[0].key_a) sample_joint(layers[0].key_a, layers[0].key_b, n_joints, j, layers[0].a, P);
    else {
#pragma unroll
        for (int c = 0; c < 10; c++) P[c] = held[c];
    }
    for (uint32_t k = 1; k < n_layers; k++) blend_layer(layers[k], n_joints, j, P);
}

// the ten floats of joint j's local pose, out to `pose` as rt_skeleton_set_pose takes them
RT_DEV void store_pose(float *pose, uint32_t j, const float P[10])
{
#pragma unroll
    for (int c = 0; c < 10; c++) pose[RT_SKELETON_POSE_FLOATS * (size_t)j + c] = P[c];
}

// Where W and the level tables stand while a pose is walked: load and store move the twelve floats of a joint's W, entry(k) is entry k of
// the level table (joint | parent << 16, rt_skeleton_pack_table) and offset(l) where level l begins.  ROW > 0: LDS, W component major in twelve
// rows of ROW floats beside copies of both tables.  ROW == 0: the same with rows of `n` floats, a row only the launch knows.  ROW < 0: W
// where it ends up, joint major in `joints`, and the tables where the skeleton keeps them, in global memory.
template <int ROW>
struct PoseStorage {
    float *w;
    const uint32_t *table, *off;
    uint32_t n;
    RT_DEV size_t at(uint32_t j, int e) const { return ROW < 0 ? 12u * (size_t)j + e : (size_t)(e * (ROW ? (uint32_t)ROW : n) + j); }
    RT_DEV void load(uint32_t j, float M[12]) const
    {
#pragma unroll
        for (int e = 0; e < 12; e++) M[e] = w[at(j, e)];
    }
    RT_DEV void store(uint32_t j, const float M[12]) const
    {
#pragma unroll
        for (int e = 0; e < 12; e++) w[at(j, e)] = M[e];
    }
    RT_DEV uint32_t entry(uint32_t k) const { return table[k]; }
    RT_DEV uint32_t offset(uint32_t l) const { return off[l]; }
};

// Steps 2 and 3 of a pose by one block of BLOCK lanes, once every joint's L stands in `at` where its W will (a root's W is its L bit for
// bit) and the block has met.  Level by level from level 1, the lanes striding a level's joints and meeting at __syncthreads():
// W_j = W_parent o L_j, in place -- a joint's parent stands in an earlier level, so nothing read in a level is written in it.  Then every
// joint at once: M_j = W_j o inverse_bind_j out to `palette`, and (WRITE_W: the storage is not `joints` itself) W_j out to `joints`.
template <uint32_t BLOCK, bool WRITE_W, class Storage>
RT_DEV void walk_levels(const Storage &at, uint32_t n_levels, uint32_t n_joints, const float *__restrict__ inverse_bind, float *joints, float *__restrict__ palette)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t l = 1; l < n_levels; l++) {            // (uniform: every lane passes every barrier)
        const uint32_t begin = at.offset(l), end = at.offset(l + 1u);
        for (uint32_t k = begin + tid; k < end; k += BLOCK) {
            const uint32_t entry = at.entry(k);
            const uint32_t j = entry & 0xFFFFu, p = entry >> 16;
            float P[12], L[12], W[12];
            at.load(p, P);
            at.load(j, L);
            compose(P, L, W);
            at.store(j, W);
        }
        __syncthreads();
    }
    for (uint32_t j = tid; j < n_joints; j += BLOCK) {
        float W[12], B[12], M[12];
        at.load(j, W);
#pragma unroll
        for (int e = 0; e < 12; e++) B[e] = inverse_bind[12u * (size_t)j + e];
        compose(W, B, M);
#pragma unroll
        for (int e = 0; e < 12; e++) {
            if (WRITE_W) joints[12u * (size_t)j + e] = W[e];
            palette[12u * (size_t)j + e] = M[e];
        }
    }
}

// What the lane of one IK constraint does once it holds its entry (IkEntry, rt_skeleton.h: the chain c, b, a and a's parent p, -1 for a
// root of the skeleton) and its values, written ONCE for k_skeleton_ik (rt_skeleton.hip) and k_crowd_ik (rt_crowd_ik.hip): the thirty floats
// of its three joints from `pose`, the twelve of W_p from `joints` -- the pose before this call: what the last posing launch left --,
// rt_ik_solve (rt_ik.h), and four floats, or eight, back into `pose`.  Nothing of the values becomes an address.  `pose` is read and
// written in place: not __restrict__.
RT_DEV void ik_solve_lane(uint32_t kind, uint32_t jc, uint32_t jb, uint32_t ja, int32_t jp, const float target[3], const float pole[3], float weight,
                          const float *joints, float *pose)
{
    float tip[10], mid[10], root[10], W[12], qa[4], qb[4];
#pragma unroll
    for (int c = 0; c < 10; c++) {
        tip[c] = pose[RT_SKELETON_POSE_FLOATS * (size_t)jc + c];
        mid[c] = pose[RT_SKELETON_POSE_FLOATS * (size_t)jb + c];
        root[c] = pose[RT_SKELETON_POSE_FLOATS * (size_t)ja + c];
    }
    const bool has_parent = jp >= 0;
#pragma unroll
    for (int c = 0; c < 12; c++) W[c] = has_parent ? joints[12u * (size_t)(has_parent ? jp : 0) + c] : 0.0f;
    rt_ik_solve(kind, tip, mid, root, has_parent ? W : nullptr, target, pole, weight, qa, qb);
#pragma unroll
    for (int c = 0; c < 4; c++) pose[RT_SKELETON_POSE_FLOATS * (size_t)ja + 3 + c] = qa[c];
    if (kind == RT_IK_TWO_BONE) {
#pragma unroll
        for (int c = 0; c < 4; c++) pose[RT_SKELETON_POSE_FLOATS * (size_t)jb + 3 + c] = qb[c];
    }
}

}  // namespace rtd
