// rt_ik.h -- the arithmetic of one inverse-kinematics constraint (rt_skeleton_solve_ik; include/dxr_amd.h "Posed skeletons", "inverse
// kinematics"): a two-bone reach or an aim, solved in closed form with + - * / sqrt, comparisons and selects only.  k_skeleton_ik
// (rt_skeleton.hip) runs it on the device, one lane per constraint; tests/cpp/ik_sanitized.cpp compiles this header with g++ for the CPU under
// the sanitizers.  It stays plain C++ (no HIP header needed), the same statements in the same order on both, without contraction, as
// rt_xform.h is written.  Vectors are float[3], quaternions float[4] = (x, y, z, w), matrices float[12] = 3x4 row-major.
#pragma once

#include <stdint.h>

#include "rt_xform.h"        // RT_HOST_DEVICE, invert3x4

#define RT_IK_KIND_TWO_BONE 0u       // (RT_IK_TWO_BONE and RT_IK_AIM of include/dxr_amd_types.h: this header includes no other of the project's)
#define RT_IK_KIND_AIM 1u

#if defined(__clang__)
#define RT_IK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RT_IK_NO_CONTRACT
#endif

RT_HOST_DEVICE static inline float ik_dot(const float u[3], const float v[3])
{
    RT_IK_NO_CONTRACT
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

RT_HOST_DEVICE static inline void ik_cross(const float u[3], const float v[3], float o[3])
{
    RT_IK_NO_CONTRACT
    const float x = u[1] * v[2] - u[2] * v[1], y = u[2] * v[0] - u[0] * v[2], z = u[0] * v[1] - u[1] * v[0];
    o[0] = x; o[1] = y; o[2] = z;
}

RT_HOST_DEVICE static inline void ik_sub(const float u[3], const float v[3], float o[3])
{
    for (int c = 0; c < 3; c++) o[c] = u[c] - v[c];
}

// o = p + v * s, three products and three sums
RT_HOST_DEVICE static inline void ik_along(const float p[3], const float v[3], float s, float o[3])
{
    RT_IK_NO_CONTRACT
    for (int c = 0; c < 3; c++) o[c] = p[c] + v[c] * s;
}

// unit(v): v * (1 / sqrt(v.v)) if 0 < v.v < inf; else the zero vector and false, "no answer"
RT_HOST_DEVICE static inline bool ik_unit(const float v[3], float o[3])
{
    RT_IK_NO_CONTRACT
    const float d = ik_dot(v, v);
    const bool ok = (d > 0.0f) && (d < __builtin_inff());
    const float inv = 1.0f / __builtin_sqrtf(d);
    for (int c = 0; c < 3; c++) o[c] = ok ? v[c] * inv : 0.0f;
    return ok;
}

// the normalisation rule of "sampling": q * (1 / sqrt(n)) if 0 < n < inf, else (0, 0, 0, 1)
RT_HOST_DEVICE static inline void ik_normalise(float q[4])
{
    RT_IK_NO_CONTRACT
    const float n = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    const bool ok = (n > 0.0f) && (n < __builtin_inff());
    const float inv = 1.0f / __builtin_sqrtf(n);
    for (int c = 0; c < 4; c++) q[c] = ok ? q[c] * inv : (c == 3 ? 1.0f : 0.0f);
}

// r = p (x) q, grouped as "blending" groups it; r may be neither p nor q
RT_HOST_DEVICE static inline void ik_hamilton(const float p[4], const float q[4], float r[4])
{
    RT_IK_NO_CONTRACT
    r[0] = ((p[3] * q[0] + p[0] * q[3]) + p[1] * q[2]) - p[2] * q[1];
    r[1] = ((p[3] * q[1] - p[0] * q[2]) + p[1] * q[3]) + p[2] * q[0];
    r[2] = ((p[3] * q[2] + p[0] * q[1]) - p[1] * q[0]) + p[2] * q[3];
    r[3] = ((p[3] * q[3] - p[0] * q[0]) - p[1] * q[1]) - p[2] * q[2];
}

// rot(q, v) = (v + (w * t)) + (q_xyz x t) with t = 2 * (q_xyz x v)
RT_HOST_DEVICE static inline void ik_rot(const float q[4], const float v[3], float o[3])
{
    RT_IK_NO_CONTRACT
    float t[3], u[3];
    ik_cross(q, v, t);
    for (int c = 0; c < 3; c++) t[c] = 2.0f * t[c];
    ik_cross(q, t, u);
    for (int c = 0; c < 3; c++) o[c] = (v[c] + q[3] * t[c]) + u[c];
}

// perp(u) = unit(u x e), e the coordinate axis on which |u| is smallest, the lowest index on a tie (a NaN moves nothing)
RT_HOST_DEVICE static inline void ik_perp(const float u[3], float o[3])
{
    const float ax = __builtin_fabsf(u[0]), ay = __builtin_fabsf(u[1]), az = __builtin_fabsf(u[2]);
    const bool y = ay < ax;
    const float least = y ? ay : ax;
    const bool z = az < least;
    float e[3], x[3];
    e[0] = (!y && !z) ? 1.0f : 0.0f;
    e[1] = (y && !z) ? 1.0f : 0.0f;
    e[2] = z ? 1.0f : 0.0f;
    ik_cross(u, e, x);
    (void)ik_unit(x, o);
}

// between(u, v) for unit u and v: the quaternion of the shortest turn from u to v, by the half vector
RT_HOST_DEVICE static inline void ik_between(const float u[3], const float v[3], float q[4])
{
    RT_IK_NO_CONTRACT
    float s[3], h[3], p[3], x[4];
    for (int c = 0; c < 3; c++) s[c] = u[c] + v[c];
    const float ss = ik_dot(s, s);
    const bool ok = ik_unit(s, h);
    ik_perp(u, p);
    ik_cross(u, h, x);
    x[3] = ik_dot(u, h);
    ik_normalise(x);
    const bool half = (ss < 1e-6f) || !ok;
    for (int c = 0; c < 3; c++) q[c] = half ? p[c] : x[c];
    q[3] = half ? 0.0f : x[3];
}

// turn(a, b) = between(unit(a), unit(b)); the identity (0, 0, 0, 1) where either has no answer
RT_HOST_DEVICE static inline void ik_turn(const float a[3], const float b[3], float q[4])
{
    float u[3], v[3], t[4];
    const bool ok_u = ik_unit(a, u), ok_v = ik_unit(b, v);
    ik_between(u, v, t);
    const bool ok = ok_u && ok_v;
    for (int c = 0; c < 4; c++) q[c] = ok ? t[c] : (c == 3 ? 1.0f : 0.0f);
}

// L = T.R.S of "local", the statements of local_of (rt_skeleton.hip), from t, a quaternion and s
RT_HOST_DEVICE static inline void ik_local(const float t[3], const float q[4], const float s[3], float L[12])
{
    RT_IK_NO_CONTRACT
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    L[0] = (1.0f - 2.0f * (yy + zz)) * s[0]; L[1] = (2.0f * (xy - wz)) * s[1];        L[2] = (2.0f * (xz + wy)) * s[2];         L[3] = t[0];
    L[4] = (2.0f * (xy + wz)) * s[0];        L[5] = (1.0f - 2.0f * (xx + zz)) * s[1]; L[6] = (2.0f * (yz - wx)) * s[2];         L[7] = t[1];
    L[8] = (2.0f * (xz - wy)) * s[0];        L[9] = (2.0f * (yz + wx)) * s[1];        L[10] = (1.0f - 2.0f * (xx + yy)) * s[2]; L[11] = t[2];
}

// M(p), an affine point transform grouped as the last column of the product C = A o B; o may not be p
RT_HOST_DEVICE static inline void ik_point(const float M[12], const float p[3], float o[3])
{
    RT_IK_NO_CONTRACT
    for (int r = 0; r < 3; r++) o[r] = ((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3];
}

// "weight": from the normalised input A towards the solved S by the RT_LAYER_BLEND rule; every NaN leaves as THE quiet NaN
RT_HOST_DEVICE static inline void ik_weigh(const float A[4], const float S[4], float w, float o[4])
{
    RT_IK_NO_CONTRACT
    const float d = ((A[0] * S[0] + A[1] * S[1]) + A[2] * S[2]) + A[3] * S[3];
    const bool flip = d < 0.0f;
    for (int c = 0; c < 4; c++) {
        const float s = flip ? -S[c] : S[c];
        o[c] = A[c] + w * (s - A[c]);
    }
    ik_normalise(o);
    for (int c = 0; c < 4; c++)
        if (o[c] != o[c]) o[c] = __builtin_nanf("");
}

// One constraint.  tip, mid, root: the ten floats tx ty tz  qx qy qz qw  sx sy sz of the joints c, b and a of a two-bone chain; an aim reads
// `tip` alone, the joint it turns.  W_parent: the world matrix of the parent of a (of the aimed joint), or null when that joint is a root of
// the skeleton.  pole: the pole of a two-bone chain, the axis of an aim.  q_root / q_mid: the quaternions to store in a and b; an aim
// writes q_root alone, the quaternion of its joint.
RT_HOST_DEVICE static inline void rt_ik_solve(uint32_t kind, const float tip[10], const float mid[10], const float root[10], const float *W_parent,
                                              const float target[3], const float pole[3], float weight, float q_root[4], float q_mid[4])
{
    RT_IK_NO_CONTRACT
    float T[3], P[3];
    for (int c = 0; c < 3; c++) { T[c] = target[c]; P[c] = pole[c]; }
    if (W_parent) {                                      // into the space of the parent; an aim's axis stays in the joint's own frame
        float I[12], t[3];
        invert3x4(W_parent, I);
        ik_point(I, target, t);
        for (int c = 0; c < 3; c++) T[c] = t[c];
        if (kind == RT_IK_KIND_TWO_BONE) {
            ik_point(I, pole, t);
            for (int c = 0; c < 3; c++) P[c] = t[c];
        }
    }
    if (kind == RT_IK_KIND_AIM) {
        float Q[4], S[4], r[3], v[3], g[3], w[3], D[4], X[4];
        for (int c = 0; c < 4; c++) Q[c] = tip[3 + c];
        ik_normalise(Q);
        ik_rot(Q, P, r);
        const bool ok_v = ik_unit(r, v);
        ik_sub(T, tip, g);
        const bool ok_w = ik_unit(g, w);
        ik_between(v, w, D);
        ik_hamilton(D, Q, X);
        ik_normalise(X);
        const bool ok = ok_v && ok_w;
        for (int c = 0; c < 4; c++) S[c] = ok ? X[c] : Q[c];
        ik_weigh(Q, S, weight, q_root);
        for (int c = 0; c < 4; c++) q_mid[c] = 0.0f;
        return;
    }
    // 1: the stored rotations, normalised
    float A[4], B[4];
    for (int c = 0; c < 4; c++) { A[c] = root[3 + c]; B[c] = mid[3 + c]; }
    ik_normalise(A);
    ik_normalise(B);
    // 2: the chain in parent space
    float La[12], Lb[12], pa[3], pb[3], pc[3], in_a[3];
    ik_local(root, A, root + 7, La);
    ik_local(mid, B, mid + 7, Lb);
    for (int c = 0; c < 3; c++) pa[c] = root[c];
    ik_point(La, mid, pb);
    ik_point(Lb, tip, in_a);
    ik_point(La, in_a, pc);
    // 3, 4: lengths, the direction to the target and the clamped distance
    float e1[3], e2[3], g[3], n[3];
    ik_sub(pb, pa, e1);
    ik_sub(pc, pb, e2);
    ik_sub(T, pa, g);
    const float l1 = __builtin_sqrtf(ik_dot(e1, e1)), l2 = __builtin_sqrtf(ik_dot(e2, e2));
    const bool ok_n = ik_unit(g, n);
    float d = __builtin_sqrtf(ik_dot(g, g));
    const float lo = __builtin_fabsf(l1 - l2), hi = l1 + l2;
    d = d < lo ? lo : d;
    d = d > hi ? hi : d;
    // 5: where there is nothing to solve the rotations stay
    const bool solve = ok_n && (d > 0.0f) && (l1 > 0.0f) && (l2 > 0.0f);
    // 6
    const float x = ((l1 * l1 - l2 * l2) + d * d) / (2.0f * d);
    const float hh = l1 * l1 - x * x;
    const float h = __builtin_sqrtf(hh > 0.0f ? hh : 0.0f);
    float k[3], off[3], m0[3], m1[3], m2[3], m[3];
    ik_sub(P, pa, k);
    float kn = ik_dot(k, n);
    for (int c = 0; c < 3; c++) off[c] = k[c] - n[c] * kn;
    const bool ok0 = ik_unit(off, m0);
    kn = ik_dot(e1, n);
    for (int c = 0; c < 3; c++) off[c] = e1[c] - n[c] * kn;
    const bool ok1 = ik_unit(off, m1);
    ik_perp(n, m2);
    for (int c = 0; c < 3; c++) m[c] = ok0 ? m0[c] : (ok1 ? m1[c] : m2[c]);
    float along[3], pb2[3], pc2[3];
    ik_along(pa, n, x, along);
    ik_along(along, m, h, pb2);
    ik_along(pa, n, d, pc2);
    float to[3], Da[4], A2[4], X[4];
    ik_sub(pb2, pa, to);
    ik_turn(e1, to, Da);
    ik_hamilton(Da, A, A2);
    ik_normalise(A2);
    float b1[3], c1[3], r[3], from[3], ca[3];
    ik_rot(Da, e1, r);
    for (int c = 0; c < 3; c++) b1[c] = pa[c] + r[c];
    ik_sub(pc, pa, ca);
    ik_rot(Da, ca, r);
    for (int c = 0; c < 3; c++) c1[c] = pa[c] + r[c];
    ik_sub(c1, b1, from);
    ik_sub(pc2, b1, to);
    float Db[4], cA[4], Y[4], B2[4];
    ik_turn(from, to, Db);
    ik_hamilton(Db, A2, X);
    cA[0] = -A2[0]; cA[1] = -A2[1]; cA[2] = -A2[2]; cA[3] = A2[3];
    ik_hamilton(cA, X, Y);
    ik_hamilton(Y, B, B2);
    ik_normalise(B2);
    for (int c = 0; c < 4; c++) {
        A2[c] = solve ? A2[c] : A[c];
        B2[c] = solve ? B2[c] : B[c];
    }
    ik_weigh(A, A2, weight, q_root);
    ik_weigh(B, B2, weight, q_mid);
}
