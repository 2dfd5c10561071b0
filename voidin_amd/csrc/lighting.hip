// lighting.hip — the lighting pass (include/voidin_lighting.h): lines 79-117 of src/bin/raytraced_shadows.wgsl for a whole image -
// the base colour, attenuation(), the diffuse and the specular term summed over the lights whose in-range bit is set, in ascending
// order, the occlusion bit halving a term, the final clamp - and the composed calls, which run the pass of gbuffer.hip through its
// exported entry points in front of it.  `pos`, `nor` and "this pixel receives" are voidin_gbuffer.h's, and the kernel calls the same
// functions of vd_shade.hpp that gbuffer.hip makes its points with (pixel_ndc, decode_octahedral, receives_light): one copy of each.
// The one exception is the matrix step of the position, kept as text in the kernel for a measured reason stated there.
//
//   lighting_kernel   ONE PIXEL PER LANE, lane -> pixel i = block * 128 + thread; one 16-byte store a pixel.
//
// Cost follows the set bits, not n_lights.  Per 32-light word the wave ORs its 64 in-range words into one wave-uniform mask (DPP
// inside a row of 16, four v_readlane across the rows; no LDS) and walks the mask's set bits in ascending order; the light record
// of a set bit sits at a wave-uniform index and comes in through scalar loads; a lane adds only when its own bit is set.  The
// ascending walk over a superset keeps every pixel's order of summation.
//
// The bit words are read as whole lines.  W = 1, 2: one 4- or 8-byte load per array and lane - a wave's words are one run of 256 or
// 512 bytes.  W > 2: the 64 W words of a wave are one contiguous run per array; the wave reads it 64 consecutive words at a time
// (256-byte lines, whatever W and whatever the alignment of the arrays) and puts word w of pixel p at LDS[p * (W | 1) + w]: the odd
// stride keeps the per-lane reads of the walk (lane * stride + w) off each other's banks.  The region belongs to the wave alone,
// so there is no barrier - DS operations of one wave execute in order.  2 * 64 * (W | 1) words a wave: 33 KiB a workgroup at W = 32.
// No atomics, no scratch.
#include "vd_shade.hpp"
#include "../../include/voidin_lighting.h"

namespace {

constexpr unsigned kBlock = 128u;                       // two waves: at W = 32 their bit words take 33 KiB of LDS
constexpr unsigned kStageSteps = 4u;                    // loads of 64 words in flight per array while a run is staged

struct View { Mat4 c2w; float eye[3]; };                // clip_to_world; view_position.xyz

__device__ __forceinline__ float pos0(float x) { return x > 0.0f ? x : 0.0f; }      // a NaN gives 0

typedef float StoreF4 __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes in one store at the alignment of a float

// The OR of `v` over the 64 lanes, every lane active: quads, halves and rows of 16 by DPP, the four rows by v_readlane - the result is
// wave-uniform (SGPR).
__device__ __forceinline__ unsigned wave_or(unsigned v) {
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);       // quad_perm [1,0,3,2]
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);       // quad_perm [2,3,0,1]
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);      // row_half_mirror
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);      // row_mirror
    return (unsigned)(__builtin_amdgcn_readlane((int)v, 0) | __builtin_amdgcn_readlane((int)v, 16) | __builtin_amdgcn_readlane((int)v, 32) |
                      __builtin_amdgcn_readlane((int)v, 48));
}

extern __shared__ unsigned lighting_lds[];             // words > 2: (kBlock / 64) regions of 2 * 64 * (words | 1) words

__global__ __launch_bounds__(kBlock) void lighting_kernel(Images im, View view, const VdLight* __restrict__ lights, unsigned n_lights, unsigned words,
                                                          const unsigned* __restrict__ occluded, const unsigned* __restrict__ in_range,
                                                          const VdFlatMaterial* __restrict__ materials, char* __restrict__ rgba, size_t pitch) {
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = vd_lane();
    const unsigned first = blockIdx.x * kBlock + wave * 64u;               // the wave's first pixel: wave-uniform
    if (first >= im.n_pixels) return;
    const unsigned i = first + lane;
    const bool valid = i < im.n_pixels;                                    // every lane stays: the OR below wants them all
    const unsigned y = i / im.width, x = i - y * im.width;

    // the pixel's own loads, all issued before the first is used
    unsigned material = VD_GBUFFER_NO_MATERIAL, n32 = 0u, in01[2] = {0u, 0u}, oc01[2] = {0u, 0u};
    float depth = 0.0f;
    if (valid) {
        material = *im.material_at(x, y);
        depth = *im.depth_at(x, y);
        n32 = *im.normal_uv_at(x, y);
        if (words == 1u) { in01[0] = in_range[i]; oc01[0] = occluded[i]; }
        if (words == 2u) { in01[0] = in_range[2u * (size_t)i]; in01[1] = in_range[2u * (size_t)i + 1u]; oc01[0] = occluded[2u * (size_t)i]; oc01[1] = occluded[2u * (size_t)i + 1u]; }
    }
    const VdFlatMaterial M = materials[material];                          // a byte: never out of range

    // words > 2: the wave's run of bit words, whole lines into its own LDS region
    const unsigned stride = words | 1u;
    unsigned* s_in = lighting_lds + (size_t)wave * (128u * stride);
    unsigned* s_oc = s_in + 64u * stride;
    if (words > 2u) {
        const unsigned left = im.n_pixels - first;
        const unsigned run = (left < 64u ? left : 64u) * words;            // <= 2048 words
        const size_t base = (size_t)first * words;
        for (unsigned r0 = 0; r0 < run; r0 += 64u * kStageSteps) {
            unsigned a[kStageSteps], o[kStageSteps];
#pragma unroll
            for (unsigned q = 0; q < kStageSteps; ++q) {
                const unsigned r = r0 + q * 64u + lane;
                a[q] = r < run ? in_range[base + r] : 0u;
                o[q] = r < run ? occluded[base + r] : 0u;
            }
#pragma unroll
            for (unsigned q = 0; q < kStageSteps; ++q) {
                const unsigned r = r0 + q * 64u + lane;
                if (r < run) {
                    const unsigned p = r / words, at = p * stride + (r - p * words);
                    s_in[at] = a[q]; s_oc[at] = o[q];
                }
            }
        }
        vd_wave_lds_sync();
    }

    // voidin_gbuffer.h's pos and nor.  The matrix step is position_from_depth's (vd_shade.hpp), spelled out: through the function - by
    // reference, by value, split from the NDC step or with its components returned through references, all the same code - the compiler
    // fetches the matrix at the kernel's start and keeps it (70 SGPRs for 62), and at 64 lights all in range the kernel's median was
    // 204.9 / 206.4 us against the parent's 201.6 / 200.0 (profiles/shading_shared.md, section 2).  As written here the kernel is the
    // parent's instruction for instruction.
    float nx, ny;
    pixel_ndc(x, y, (float)im.width, (float)(im.n_pixels / im.width), nx, ny);
    const float* C = view.c2w.m;
    float w4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) w4[r] = ((C[r] * nx + C[4 + r] * ny) + C[8 + r] * depth) + C[12 + r];
    const V3 pos = V3{w4[0] / w4[3], w4[1] / w4[3], w4[2] / w4[3]};
    const V3 nor = decode_octahedral(n32);

    // lines 79-86: the base colour and the specular factor of the pixel
    const bool lit = receives_light(material);
    V3 c;
    if (lit) c = V3{M.albedo[0] * 0.3f + M.emissive[0], M.albedo[1] * 0.3f + M.emissive[1], M.albedo[2] * 0.3f + M.emissive[2]};
    else c = V3{M.albedo[0] + M.emissive[0], M.albedo[1] + M.emissive[1], M.albedo[2] + M.emissive[2]};
    const V3 v = V3{view.eye[0], view.eye[1], view.eye[2]} - pos;
    const V3 rd = over(v, sqrtf(dot3(v, v)));
    const float covr = pos0(dot3(V3{-rd.x, -rd.y, -rd.z}, nor));
    float c16 = covr * covr;
    c16 = c16 * c16; c16 = c16 * c16; c16 = c16 * c16;

    // lines 87-115 over the set bits
    for (unsigned w = 0; w < words; ++w) {
        unsigned inr, occ;
        if (words <= 2u) { inr = w ? in01[1] : in01[0]; occ = w ? oc01[1] : oc01[0]; }
        else { inr = s_in[lane * stride + w]; occ = s_oc[lane * stride + w]; }
        if (!lit) inr = 0u;
        if (w == words - 1u && (n_lights & 31u)) inr &= (1u << (n_lights & 31u)) - 1u;      // bits at and above n_lights are no lights
        unsigned mask = wave_or(inr);
        while (mask) {
            const unsigned b = (unsigned)__builtin_ctz(mask);
            mask &= mask - 1u;
            const VdLight L = lights[w * 32u + b];                                         // a wave-uniform index below n_lights
            if ((inr >> b) & 1u) {
                const V3 d = V3{L.position[0], L.position[1], L.position[2]} - pos;
                const float dist = sqrtf(dot3(d, d));
                const float occlusion = ((occ >> b) & 1u) ? 0.5f : 1.0f;
                const float s = dist / L.radius, s2 = s * s, q = 1.0f - s2;
                const float atten = (s >= 1.0f) ? 0.0f : (q * q) / (1.0f + s2);
                const float shade = pos0(dot3(nor, over(d, dist)));
                c.x = c.x + (((L.color[0] * M.albedo[0]) * shade + (L.color[0] * M.specular) * c16) * occlusion) * atten;
                c.y = c.y + (((L.color[1] * M.albedo[1]) * shade + (L.color[1] * M.specular) * c16) * occlusion) * atten;
                c.z = c.z + (((L.color[2] * M.albedo[2]) * shade + (L.color[2] * M.specular) * c16) * occlusion) * atten;
            }
        }
    }

    // lines 80-82 and 117: one 16-byte store a pixel
    StoreF4 out = {pos0(c.x), pos0(c.y), pos0(c.z), 1.0f};
    if (material == VD_GBUFFER_NO_MATERIAL) out = StoreF4{1.0f, 0.0f, 1.0f, 1.0f};
    if (valid) *reinterpret_cast<StoreF4*>(rgba + (size_t)y * pitch + 16u * (size_t)x) = out;
}

// Everything the step refuses but the two bit arrays.  *empty: the image has no pixel - VD_OK, nothing to do.
int check(VdCtx* ctx, const char* name, const VdCameraUniform* camera, const VdGBuffer* gb, const VdLight* d_lights, uint32_t n_lights,
          const VdFlatMaterial* d_materials, const VdColorTarget* tg, bool* empty) {
    *empty = false;
    if (!gb || !tg) return vd_fail_arg(ctx, name, "null pointer");
    if (tg->width != gb->width || tg->height != gb->height) return vd_fail_arg(ctx, name, "the target's size is not the G-buffer's");
    if (gb->width == 0 || gb->height == 0) { *empty = true; return VD_OK; }
    if (!camera || !d_materials || !tg->rgba || (n_lights && !d_lights)) return vd_fail_arg(ctx, name, "null pointer");
    const int rc = vd_check_images(ctx, name, gb);
    if (rc) return rc;
    if (tg->pitch % 16u || (uint64_t)tg->pitch < 16ull * tg->width) return vd_fail_arg(ctx, name, "the target's pitch is below 16 * width or not a multiple of 16");
    if (n_lights > VD_SHADOW_MAX_LIGHTS) return vd_fail_arg(ctx, name, "more than VD_SHADOW_MAX_LIGHTS lights");
    return VD_OK;
}

// The arguments have been checked and the image is not empty.  Enqueues only.
int launch(VdCtx* ctx, const VdCameraUniform* camera, const VdGBuffer* gb, const VdLight* d_lights, uint32_t n_lights, const uint32_t* d_occluded,
           const uint32_t* d_in_range, const VdFlatMaterial* d_materials, const VdColorTarget* tg) {
    const unsigned n = gb->width * gb->height, words = (n_lights + 31u) / 32u;
    const Images im = vd_images<const char>(gb);
    View view;
    memcpy(view.c2w.m, camera->clip_to_world, sizeof(view.c2w.m));
    memcpy(view.eye, camera->view_position, sizeof(view.eye));
    const size_t lds = words > 2u ? (size_t)(kBlock / 64u) * 128u * (words | 1u) * sizeof(unsigned) : 0;
    hipLaunchKernelGGL(lighting_kernel, dim3((n + kBlock - 1u) / kBlock), dim3(kBlock), lds, ctx->stream, im, view, d_lights, n_lights, words, d_occluded, d_in_range,
                       d_materials, reinterpret_cast<char*>(tg->rgba), (size_t)tg->pitch);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// Both composed forms: exactly one of scene / accel is given (the entry points have checked that it is not null).
int shade_gbuffer(VdCtx* ctx, const char* name, const VdTraceScene* scene, const VdTraceAccel* accel, const VdCameraUniform* camera, const VdGBuffer* gb,
                  const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays, const VdFlatMaterial* d_materials, const VdColorTarget* tg,
                  VdShadowGBufferInfo* out_info) {
    if (out_info) memset(out_info, 0, sizeof(*out_info));
    bool empty;
    int rc = check(ctx, name, camera, gb, d_lights, n_lights, d_materials, tg, &empty);
    if (rc || empty) return rc;
    uint32_t* d_occ = nullptr; uint32_t* d_inr = nullptr;
    if (n_lights) {
        // (the pass would refuse this itself, but only after the arena below had been sized by it)
        if ((uint64_t)gb->width * gb->height * n_lights > kMaxPairs) return vd_fail_arg(ctx, name, "width * height * n_lights exceeds 0xf0000000");
        const size_t n = (size_t)gb->width * gb->height * ((n_lights + 31u) / 32u);
        if ((rc = vd_carve(ctx, &ctx->lighting, [&](Arena& a) { d_occ = a.take<uint32_t>(n); d_inr = a.take<uint32_t>(n); }))) return rc;
        rc = scene ? vd_shadow_gbuffer_dev(ctx, scene, camera, gb, d_lights, n_lights, max_chunk_rays, d_occ, d_inr, out_info)
                   : vd_shadow_gbuffer_prepared_dev(ctx, accel, camera, gb, d_lights, n_lights, max_chunk_rays, d_occ, d_inr, out_info);
        if (rc) return rc;
    }
    if ((rc = launch(ctx, camera, gb, d_lights, n_lights, d_occ, d_inr, d_materials, tg))) return rc;
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VD_OK;
}

}  // namespace

extern "C" {

int vd_lighting_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdGBuffer* gb, const VdLight* d_lights, uint32_t n_lights, const uint32_t* d_occluded,
                    const uint32_t* d_in_range, const VdFlatMaterial* d_materials, const VdColorTarget* target) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    const char* name = "vd_lighting";
    bool empty;
    const int rc = check(ctx, name, camera, gb, d_lights, n_lights, d_materials, target, &empty);
    if (rc || empty) return rc;
    if (n_lights && (!d_occluded || !d_in_range)) return vd_fail_arg(ctx, name, "null pointer");
    return launch(ctx, camera, gb, d_lights, n_lights, d_occluded, d_in_range, d_materials, target);
}

int vd_shade_gbuffer_dev(VdCtx* ctx, const VdTraceScene* d_scene, const VdCameraUniform* camera, const VdGBuffer* gb, const VdLight* d_lights, uint32_t n_lights,
                         uint32_t max_chunk_rays, const VdFlatMaterial* d_materials, const VdColorTarget* target, VdShadowGBufferInfo* out_info) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_scene) return vd_fail_arg(ctx, "vd_shade_gbuffer", "null scene");
    return shade_gbuffer(ctx, "vd_shade_gbuffer", d_scene, nullptr, camera, gb, d_lights, n_lights, max_chunk_rays, d_materials, target, out_info);
}

int vd_shade_gbuffer_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdCameraUniform* camera, const VdGBuffer* gb, const VdLight* d_lights,
                                  uint32_t n_lights, uint32_t max_chunk_rays, const VdFlatMaterial* d_materials, const VdColorTarget* target,
                                  VdShadowGBufferInfo* out_info) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!accel) return vd_fail_arg(ctx, "vd_shade_gbuffer_prepared", "null accel");
    return shade_gbuffer(ctx, "vd_shade_gbuffer_prepared", nullptr, accel, camera, gb, d_lights, n_lights, max_chunk_rays, d_materials, target, out_info);
}

}  // extern "C"
