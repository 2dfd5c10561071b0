// vd_shade.hpp — what the shading passes share (shadow.hip -> gbuffer.hip, gbuffer_trace.hip -> lighting.hip): the ONE copy of every
// definition that two of them must agree on bit for bit - which pixels receive, where a pixel's world position is, what its normal
// is - and of the plumbing they had each restated: the one-workgroup scan, the 3-float vector, the view of the three images with its
// texel addresses, the checks of those images, the two size limits.  Internal: not part of the C ABI.  The passes still reach each
// other through their exported entry points only.
#pragma once

#include <type_traits>

#include "vd_common.hpp"
#include "../../include/voidin_gbuffer_trace.h"

// ---- limits -----------------------------------------------------------------------------------------------------------------------
constexpr unsigned kMaxPixels = 1u << 30;                  // width * height of an image
constexpr uint64_t kMaxPairs = 0xf0000000ull;              // (point or pixel, light) pairs of a call: what the walk takes as rays

// ---- the one-workgroup exclusive scan ---------------------------------------------------------------------------------------------
constexpr unsigned kScanThreads = 1024u, kScanItems = 4u;

// offsets[i] = count[0] + ... + count[i - 1] for i in [0, n); returns count[0] + ... + count[n - 1] in every thread.  ONE workgroup of
// kScanThreads threads, all of them calling: kScanThreads * kScanItems counts per round.
__device__ __forceinline__ unsigned vd_block_scan(const unsigned* __restrict__ count, unsigned n, unsigned* __restrict__ offsets) {
    __shared__ unsigned wave_sum[kScanThreads / 64u];
    const unsigned lane = vd_lane(), wave = threadIdx.x >> 6;
    unsigned carry = 0u;
    for (unsigned base = 0; base < n; base += kScanThreads * kScanItems) {
        const unsigned i0 = base + threadIdx.x * kScanItems;
        unsigned v[kScanItems], mine = 0u;
#pragma unroll
        for (unsigned q = 0; q < kScanItems; ++q) { v[q] = i0 + q < n ? count[i0 + q] : 0u; mine += v[q]; }
        unsigned incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(incl, off);
            if (lane >= (unsigned)off) incl += o;
        }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        unsigned before = carry, total = 0u;
#pragma unroll
        for (unsigned w = 0; w < kScanThreads / 64u; ++w) { const unsigned s = wave_sum[w]; before += w < wave ? s : 0u; total += s; }
        unsigned run = before + incl - mine;
#pragma unroll
        for (unsigned q = 0; q < kScanItems; ++q) { if (i0 + q < n) offsets[i0 + q] = run; run += v[q]; }
        carry += total;
        __syncthreads();
    }
    return carry;
}

// ---- the vector and the pixel geometry --------------------------------------------------------------------------------------------
// float32, nothing contracted; the order of the operations below IS the definition (include/voidin_gbuffer.h, voidin_gbuffer_trace.h).
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
__device__ __forceinline__ V3 over(V3 a, float s) { return V3{a.x / s, a.y / s, a.z / s}; }

struct Mat4 { float m[16]; };                              // column-major, as VdCameraUniform holds it

__device__ __forceinline__ float unit_to_signed(float u) { return u * 2.0f - 1.0f; }      // [0, 1] -> [-1, 1]

// The centre of pixel (x, y) of a fw x fh image in NDC (uv.wgsl:1-3): y points up.
__device__ __forceinline__ void pixel_ndc(unsigned x, unsigned y, float fw, float fh, float& nx, float& ny) {
    const float ux = ((float)x + 0.5f) / fw, uy = ((float)y + 0.5f) / fh;
    nx = unit_to_signed(ux); ny = unit_to_signed(1.0f - uy);
}

// world_position_from_depth (uv.wgsl:13-22) at that pixel centre: clip_to_world * (ndc, depth, 1), xyz / w by three divisions.
__device__ __forceinline__ V3 position_from_depth(const Mat4& clip_to_world, unsigned x, unsigned y, float fw, float fh, float depth) {
    float nx, ny;
    pixel_ndc(x, y, fw, fh, nx, ny);
    const float* M = clip_to_world.m;
    float w4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) w4[r] = ((M[r] * nx + M[4 + r] * ny) + M[8 + r] * depth) + M[12 + r];
    return V3{w4[0] / w4[3], w4[1] / w4[3], w4[2] / w4[3]};
}

// decode_octahedral_32 (encoding.wgsl:17-28), normalised by three divisions
__device__ __forceinline__ V3 decode_octahedral(unsigned n32) {
    const float vx = unit_to_signed((float)(n32 & 0xffffu) / 65535.0f), vy = unit_to_signed((float)((n32 >> 16) & 0xffffu) / 65535.0f);
    float ax = vx, ay = vy;
    const float az = (1.0f - fabsf(vx)) - fabsf(vy);
    const float tt = (-az > 0.0f) ? -az : 0.0f;
    ax += (ax > 0.0f) ? -tt : tt;
    ay += (ay > 0.0f) ? -tt : tt;
    return over(V3{ax, ay, az}, sqrtf((ax * ax + ay * ay) + az * az));
}

__device__ __forceinline__ float sign1(float a) { return a < 0.0f ? -1.0f : 1.0f; }      // the fold's sign: 0 (and a NaN) count as +1
// floor((q * 0.5 + 0.5) * 65535 + 0.5) as a 16-bit code: a NaN -> 0, clamped to [0, 65535]
__device__ __forceinline__ unsigned oct_code(float q) {
    const float d = floorf((q * 0.5f + 0.5f) * 65535.0f + 0.5f);
    return (unsigned)fminf(fmaxf(d, 0.0f), 65535.0f);      // fmaxf(NaN, 0) = 0
}
// encode_octahedral_32 (encoding.wgsl:4-15) with voidin_gbuffer_trace.h's two departures
__device__ __forceinline__ unsigned encode_octahedral(V3 n) {
    const V3 q = over(n, (fabsf(n.x) + fabsf(n.y)) + fabsf(n.z));
    float ox = q.x, oy = q.y;
    if (q.z < 0.0f) { ox = (1.0f - fabsf(q.y)) * sign1(q.x); oy = (1.0f - fabsf(q.x)) * sign1(q.y); }
    return (oct_code(oy) << 16) | oct_code(ox);
}

// ---- the receiver predicate -------------------------------------------------------------------------------------------------------
// raytraced_shadows.wgsl:80: this material receives light - and nothing else decides it
__device__ __forceinline__ bool receives_light(unsigned material) {
    return material != VD_GBUFFER_NO_MATERIAL && material != VD_GBUFFER_LIGHT_MATERIAL;
}

// ---- the three images -------------------------------------------------------------------------------------------------------------
// The images as the kernels take them, by value: the pitches in bytes (size_t: a row offset may pass 4 GiB), the sizes, and the address
// of a texel.  B = const char: read-only (Images); B = char: the resolve kernel's (Target).
template <typename B>
struct ImagesT {
    template <typename T> using As = typename std::conditional<std::is_const<B>::value, const T, T>::type;
    B* depth; B* normal_uv; As<uint8_t>* material;
    size_t depth_pitch, normal_uv_pitch, material_pitch;
    unsigned width, n_pixels;
    __device__ __forceinline__ As<float>* depth_at(unsigned x, unsigned y) const { return reinterpret_cast<As<float>*>(depth + (size_t)y * depth_pitch + 4u * (size_t)x); }
    // the first word of the pair: the normal
    __device__ __forceinline__ As<uint32_t>* normal_uv_at(unsigned x, unsigned y) const {
        return reinterpret_cast<As<uint32_t>*>(normal_uv + (size_t)y * normal_uv_pitch + 8u * (size_t)x);
    }
    __device__ __forceinline__ As<uint8_t>* material_at(unsigned x, unsigned y) const { return &material[(size_t)y * material_pitch + x]; }
};
typedef ImagesT<const char> Images;
typedef ImagesT<char> Target;

// G: VdGBuffer (-> Images) or VdGBufferTarget (-> Target); the image has been checked.
template <typename B, typename G>
static inline ImagesT<B> vd_images(const G* g) {
    return ImagesT<B>{reinterpret_cast<B*>(g->depth), reinterpret_cast<B*>(g->normal_uv), g->material, g->depth_pitch, g->normal_uv_pitch, g->material_pitch,
                      g->width, g->width * g->height};
}

// The pixel count of an image that is not empty.
static inline int vd_check_pixels(VdCtx* ctx, const char* name, uint32_t width, uint32_t height) {
    return (uint64_t)width * height > kMaxPixels ? vd_fail_arg(ctx, name, "width * height exceeds 2^30") : VD_OK;
}

// VdGBuffer's rules (voidin_gbuffer.h), which VdGBufferTarget shares: neither size is zero.  Tested in this order.
static inline int vd_check_images(VdCtx* ctx, const char* name, const void* depth, const void* normal_uv, const void* material, uint32_t depth_pitch,
                                  uint32_t normal_uv_pitch, uint32_t material_pitch, uint32_t width, uint32_t height) {
    if (!depth || !normal_uv || !material) return vd_fail_arg(ctx, name, "null pointer");
    const int rc = vd_check_pixels(ctx, name, width, height);
    if (rc) return rc;
    if (depth_pitch % 4u || (uint64_t)depth_pitch < 4ull * width) return vd_fail_arg(ctx, name, "depth_pitch is below 4 * width or not a multiple of 4");
    if (normal_uv_pitch % 8u || (uint64_t)normal_uv_pitch < 8ull * width) return vd_fail_arg(ctx, name, "normal_uv_pitch is below 8 * width or not a multiple of 8");
    if (material_pitch < width) return vd_fail_arg(ctx, name, "material_pitch is below width");
    return VD_OK;
}
template <typename G>      // G: VdGBuffer or VdGBufferTarget, not null
static inline int vd_check_images(VdCtx* ctx, const char* name, const G* g) {
    return vd_check_images(ctx, name, g->depth, g->normal_uv, g->material, g->depth_pitch, g->normal_uv_pitch, g->material_pitch, g->width, g->height);
}
