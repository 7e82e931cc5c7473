/*
 * hlsl_shim.h -- TEST INFRASTRUCTURE ONLY (oracle/refshade).
 *
 * The HLSL types, operators and intrinsics that the reference's shading text uses, so that the text -- translated by translate.py
 * into oracle/_ref/gen/, never committed -- compiles as C++ and runs as the reference of tests/test_refshade.py.
 *
 * Everything lives in namespace hlsl, so that sin, cos, exp, log, pow, sqrt, min, max and abs written in the translated text resolve to
 * the definitions below and never to <math.h>.  The intrinsics whose precision HLSL leaves to the driver are this engine's definitions
 * (DESIGN section 2): they call oracle_math.h and nothing above it.  Operation order, draw order, constants, branches and bindings come
 * from the translated text.  README.md in this folder lists these seams.
 *
 * Vector constructors: translate.py rewrites `float3(a, b, c)` to `float3{a, b, c}`; a braced initialiser list is evaluated left to
 * right (the reference's shader compiler scalarises constructors in source order), a parenthesised argument list is not (g++ goes
 * right to left).  The constructors are templates so that uint and int components convert without a narrowing error.
 */
#ifndef HLSL_SHIM_H
#define HLSL_SHIM_H

#include <stddef.h>
#include <stdint.h>
#include "../oracle_math.h"

namespace hlsl {

typedef uint32_t uint;
typedef uint32_t UINT;
typedef int32_t BOOL;

struct uint2 {
    uint x, y;
    uint2() : x(0), y(0) {}
    template <class A, class B> uint2(A a, B b) : x(uint(a)), y(uint(b)) {}
    uint2 xy() const { return *this; }
};

struct uint3 {
    uint x, y, z;
    uint3() : x(0), y(0), z(0) {}
    template <class A, class B, class C> uint3(A a, B b, C c) : x(uint(a)), y(uint(b)), z(uint(c)) {}
    uint2 xy() const { return uint2{x, y}; }
    uint operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
};

struct float2 {
    float x, y;
    float2() : x(0.0f), y(0.0f) {}
    float2(float s) : x(s), y(s) {}
    explicit float2(uint2 u) : x(float(u.x)), y(float(u.y)) {}
    template <class A, class B> float2(A a, B b) : x(float(a)), y(float(b)) {}
    float2 xy() const { return *this; }
};

struct float3 {
    float x, y, z;
    float3() : x(0.0f), y(0.0f), z(0.0f) {}
    float3(float s) : x(s), y(s), z(s) {}                          /* float3 c = 0.0; return of a float from a float3 function */
    template <class A, class B, class C> float3(A a, B b, C c) : x(float(a)), y(float(b)), z(float(c)) {}
    float3 xyz() const { return *this; }
    float3 rgb() const { return *this; }
    float2 xy() const { return float2{x, y}; }
};

struct float4 {
    float x, y, z, w;
    float4() : x(0.0f), y(0.0f), z(0.0f), w(0.0f) {}
    float4(float s) : x(s), y(s), z(s), w(s) {}
    float4(float3 v, float s) : x(v.x), y(v.y), z(v.z), w(s) {}
    template <class A, class B, class C, class D> float4(A a, B b, C c, D d) : x(float(a)), y(float(b)), z(float(c)), w(float(d)) {}
    float3 xyz() const { return float3{x, y, z}; }
    float3 rgb() const { return float3{x, y, z}; }
    float2 xy() const { return float2{x, y}; }
    float a() const { return w; }
};

typedef float2 XMFLOAT2;
typedef float3 XMFLOAT3;
typedef float4 XMFLOAT4;

/* componentwise + - * / for vector op vector, vector op scalar, scalar op vector; a uint or int operand converts to float first */
#define HLSL_OPS2(V, OP) \
    static inline V operator OP(V a, V b) { return V{a.x OP b.x, a.y OP b.y}; } \
    static inline V operator OP(V a, float b) { return V{a.x OP b, a.y OP b}; } \
    static inline V operator OP(float a, V b) { return V{a OP b.x, a OP b.y}; }
#define HLSL_OPS3(V, OP) \
    static inline V operator OP(V a, V b) { return V{a.x OP b.x, a.y OP b.y, a.z OP b.z}; } \
    static inline V operator OP(V a, float b) { return V{a.x OP b, a.y OP b, a.z OP b}; } \
    static inline V operator OP(float a, V b) { return V{a OP b.x, a OP b.y, a OP b.z}; }
#define HLSL_OPS4(V, OP) \
    static inline V operator OP(V a, V b) { return V{a.x OP b.x, a.y OP b.y, a.z OP b.z, a.w OP b.w}; } \
    static inline V operator OP(V a, float b) { return V{a.x OP b, a.y OP b, a.z OP b, a.w OP b}; } \
    static inline V operator OP(float a, V b) { return V{a OP b.x, a OP b.y, a OP b.z, a OP b.w}; }
HLSL_OPS2(float2, +) HLSL_OPS2(float2, -) HLSL_OPS2(float2, *) HLSL_OPS2(float2, /)
HLSL_OPS3(float3, +) HLSL_OPS3(float3, -) HLSL_OPS3(float3, *) HLSL_OPS3(float3, /)
HLSL_OPS4(float4, +) HLSL_OPS4(float4, -) HLSL_OPS4(float4, *) HLSL_OPS4(float4, /)
#undef HLSL_OPS2
#undef HLSL_OPS3
#undef HLSL_OPS4

static inline float2 operator-(float2 a) { return float2{-a.x, -a.y}; }
static inline float3 operator-(float3 a) { return float3{-a.x, -a.y, -a.z}; }
static inline float4 operator-(float4 a) { return float4{-a.x, -a.y, -a.z, -a.w}; }
static inline float3 &operator+=(float3 &a, float3 b) { a = a + b; return a; }
static inline float2 operator+(uint2 a, float b) { return float2{float(a.x) + b, float(a.y) + b}; }      /* launchIndex.xy + 0.5f */

/* ---- intrinsics: the project's definitions (oracle_math.h), for exactly the list in README.md ---- */

static inline orc::V3 to_v3(float3 a) { return orc::v3(a.x, a.y, a.z); }
static inline float3 from_v3(orc::V3 a) { return float3{a.x, a.y, a.z}; }

static inline float sin(float x) { float s, c; orc::sincos_(x, &s, &c); return s; }
static inline float cos(float x) { float s, c; orc::sincos_(x, &s, &c); return c; }
static inline float exp(float x) { return orc::exp_(x); }
static inline float log(float x) { return orc::log_(x); }
static inline float pow(float x, float y) { return orc::pow_(x, y); }
static inline float sqrt(float x) { return ::sqrtf(x); }
static inline float min(float a, float b) { return orc::fmin_(a, b); }
static inline float max(float a, float b) { return orc::fmax_(a, b); }
static inline float3 max(float3 a, float b) { return float3{orc::fmax_(a.x, b), orc::fmax_(a.y, b), orc::fmax_(a.z, b)}; }
static inline float saturate(float x) { return orc::saturate(x); }
static inline float dot(float3 a, float3 b) { return orc::dot3(to_v3(a), to_v3(b)); }
static inline float3 cross(float3 a, float3 b) { return from_v3(orc::cross3(to_v3(a), to_v3(b))); }
static inline float3 normalize(float3 a) { return from_v3(orc::normalize3(to_v3(a))); }
static inline float length(float3 a) { return orc::length3(to_v3(a)); }
static inline float3 reflect(float3 i, float3 n) { return from_v3(orc::reflect3(to_v3(i), to_v3(n))); }
/* normalize of a float4 (RayGen normalises U, V, W with their w): oracle_math.h's normalize3 carried to four components, the dot
 * summed in component order.  With w == 0, which include/dxr_amd_types.h requires of U, V and W, it equals normalize3 bit for bit. */
static inline float4 normalize(float4 a)
{
    float s = a.x * a.x;
    s = s + a.y * a.y;
    s = s + a.z * a.z;
    s = s + a.w * a.w;
    float r = 1.0f / ::sqrtf(s);
    return float4{a.x * r, a.y * r, a.z * r, a.w * r};
}
/* exact operations, no seam */
static inline float abs(float x) { return ::fabsf(x); }
static inline float3 abs(float3 a) { return float3{::fabsf(a.x), ::fabsf(a.y), ::fabsf(a.z)}; }
/* only wsVectorToLatLong uses these, and nothing calls it (the lat-long path is commented out in the text): they must compile, not agree */
static inline float atan2(float y, float x) { return ::atan2f(y, x); }
static inline float acos(float x) { return ::acosf(x); }

/* ---- resources: what the text declares at file scope; harness.cpp fills and serves them ---- */

struct RaytracingAccelerationStructure {};
struct SamplerState {};
template <class T> struct ConstantBuffer : T {};

template <class T> struct Buffer {              /* Buffer<float3>: a typed view of tightly packed floats */
    const float *data = nullptr;
    T operator[](uint i) const { return T{data[3 * (size_t)i], data[3 * (size_t)i + 1], data[3 * (size_t)i + 2]}; }
};

struct ByteAddressBuffer {
    const uint8_t *bytes = nullptr;
    uint load(uint off) const { uint v; memcpy(&v, bytes + off, 4); return v; }
    uint2 Load2(uint off) const { return uint2{load(off), load(off + 4)}; }
    uint3 Load3(uint off) const { return uint3{load(off), load(off + 4), load(off + 8)}; }
};

struct Texture2D {
    float4 SampleLevel(SamplerState, float2, float) const { return float4(); }       /* declared by the text, never sampled */
};

struct TextureCube {
    const float *faces = nullptr;               /* 6 * size * size * 4 floats, or NULL: a constant colour */
    int size = 0;
    float constant[3] = {0.0f, 0.0f, 0.0f};
    float4 SampleLevel(SamplerState, float3 dir, float lod) const;                    /* harness.cpp: through orc_sample_cube */
};

template <class T> struct RWTexture2D {         /* RWTexture2D<float4>: an fp32 image, or one stored as RGBA16F */
    float *texels = nullptr;
    uint width = 0;
    int f16 = 0;                                /* 0: fp32 storage; 1 / 2: every store rounds to fp16, to nearest even / toward zero */
    struct Texel {
        const RWTexture2D *t;
        uint2 at;
        operator T() const { const float *p = t->texels + ((size_t)at.y * t->width + at.x) * 4; return T{p[0], p[1], p[2], p[3]}; }
        void operator=(T v) const { t->store(at, v); }
    };
    Texel operator[](uint2 at) const { return Texel{this, at}; }
    void store(uint2 at, T v) const;                                                  /* harness.cpp: through orc_round_to_half */
};

struct RayDesc {                                /* an aggregate: the text writes RayDesc ray = { orig, minT, dir, maxT } */
    float3 Origin;
    float TMin;
    float3 Direction;
    float TMax;
};

/* D3D12_RAY_FLAG_* */
enum : uint {
    RAY_FLAG_NONE = 0x00,
    RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH = 0x04,
    RAY_FLAG_SKIP_CLOSEST_HIT_SHADER = 0x08,
    RAY_FLAG_CULL_BACK_FACING_TRIANGLES = 0x10,
};

/* ---- the DXR system values and TraceRay: harness.cpp ---- */

uint3 DispatchRaysIndex();
uint3 DispatchRaysDimensions();
float3 WorldRayOrigin();
float3 WorldRayDirection();
float RayTCurrent();
uint PrimitiveIndex();

enum { MAX_PAYLOAD_BYTES = 64 };
void trace_ray(uint flags, uint instanceMask, uint rayContributionToHitGroupIndex, uint multiplierForGeometryContributionToHitGroupIndex,
               uint missShaderIndex, const RayDesc &ray, void *payload);

/* payloads are untyped bytes to DXR: the shader a record binds reads them as its own payload type, whatever the caller passed */
template <class P>
void TraceRay(RaytracingAccelerationStructure, uint flags, uint instanceMask, uint rayContribution, uint geometryMultiplier,
              uint missShaderIndex, RayDesc ray, P &payload)
{
    static_assert(sizeof(P) <= MAX_PAYLOAD_BYTES, "payload larger than the harness's buffer");
    alignas(16) unsigned char bytes[MAX_PAYLOAD_BYTES] = {0};
    memcpy(bytes, (const void *)&payload, sizeof(P));
    trace_ray(flags, instanceMask, rayContribution, geometryMultiplier, missShaderIndex, ray, bytes);
    memcpy((void *)&payload, bytes, sizeof(P));
}

}  // namespace hlsl

#endif
