// rt_xform.h -- the instance transform's arithmetic.  The library runs it on the device only: k_update_records (rt_scene.hip) writes
// the transform part of every instance record, for rt_scene_build and rt_scene_update alike.  The one host user of invert3x4 is
// tests/cpp/invert3x4_sanitized.cpp, which compiles this header with g++ for the CPU under the sanitizers: it stays plain C++ (no HIP
// header needed), the same operations in the same order, without contraction.
#pragma once

#if defined(__HIPCC__)
#define RT_HOST_DEVICE __host__ __device__
#else
#define RT_HOST_DEVICE
#endif

// the transform that makes an instance an identity instance (rays walk its BLAS in world space): all twelve floats compare equal
RT_HOST_DEVICE static inline bool is_identity3x4(const float m[12])
{
    bool identity = true;
    for (int k = 0; k < 12; k++) identity = identity && (m[k] == ((k == 0 || k == 5 || k == 10) ? 1.0f : 0.0f));
    return identity;
}

// world-to-object = inverse of the affine 3x4 (adjugate / determinant in fp32,
// operation order fixed: see DESIGN.md "Instances")
RT_HOST_DEVICE static inline void invert3x4(const float m[12], float o[12])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float a = m[0], b = m[1], c = m[2];
    float d = m[4], e = m[5], f = m[6];
    float g = m[8], h = m[9], i = m[10];
    float A = e * i - f * h;
    float B = f * g - d * i;
    float C = d * h - e * g;
    float det = a * A;
    det = det + b * B;
    det = det + c * C;
    float id = 1.0f / det;
    o[0] = A * id; o[1] = (c * h - b * i) * id; o[2] = (b * f - c * e) * id;
    o[4] = B * id; o[5] = (a * i - c * g) * id; o[6] = (c * d - a * f) * id;
    o[8] = C * id; o[9] = (b * g - a * h) * id; o[10] = (a * e - b * d) * id;
    for (int r = 0; r < 3; r++) {
        float s = o[4 * r + 0] * m[3];
        s = s + o[4 * r + 1] * m[7];
        s = s + o[4 * r + 2] * m[11];
        o[4 * r + 3] = -s;
    }
    // IEEE 754 leaves the sign and payload of a NaN result to the hardware (an x86 subtraction passes a NaN operand on as it is, the GPU's
    // applies its negation to it first): every NaN leaves as THE quiet NaN 0x7FC00000, so that host and device agree on those bits too.
    // Everything else above is correctly rounded and the same on both.
    for (int k = 0; k < 12; k++)
        if (o[k] != o[k]) o[k] = __builtin_nanf("");
}

// C = A o B of two 3x4 affine matrices, grouped as include/dxr_amd.h "Posed skeletons" groups it (the statements of `compose`, rt_skeleton.hip):
// what k_gather_transforms (rt_scene.hip) makes the transform of an attached instance with, T = W_joint o local
RT_HOST_DEVICE static inline void compose3x4(const float A[12], const float B[12], float C[12])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int r = 0; r < 3; r++) {
        const float a0 = A[4 * r], a1 = A[4 * r + 1], a2 = A[4 * r + 2], a3 = A[4 * r + 3];
        for (int c = 0; c < 3; c++) C[4 * r + c] = (a0 * B[c] + a1 * B[4 + c]) + a2 * B[8 + c];
        C[4 * r + 3] = ((a0 * B[3] + a1 * B[7]) + a2 * B[11]) + a3;
    }
}
