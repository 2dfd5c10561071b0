/*
 * voidin_shadow.h — the shadow pass for many point lights, an extension of the C ABI of libvoidin_hip.so (voidin_abi.h,
 * whose conventions hold here).
 *
 * The reference's only production use of traverse_tlas is the shadow loop of src/bin/raytraced_shadows.wgsl:87-115: for
 * every G-buffer point it runs over ALL point lights, skips a light the point is out of reach of,
 *
 *     let light_vec = light.position - pos;  let dist = length(light_vec);
 *     if dist - light.radius > 0. { continue; }
 *
 * and fires one shadow ray at each remaining light.  vd_shadow_pass*_dev is that loop for P points and L lights in one call:
 * every (point, light) pair is tested on the device, only the pairs in range become rays (vd_shadow_rays_dev's, bytes
 * included), the any-hit walk of vd_trace_any*_dev answers them, and one bit per pair comes back.
 *
 * Definition (float32, nothing contracted).  For point p and light l:
 *     d        = light.position - pos              (the very subtraction that makes the ray's dir)
 *     dist     = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z)
 *     in_range = !((dist - light.radius) > 0.0f)   (negated on purpose: a NaN radius or distance is IN range, as in the WGSL)
 * With W = words_per_point = (n_lights + 31) / 32, bit (l & 31) of d_in_range[p * W + (l >> 5)] is in_range and the same bit
 * of d_occluded is in_range && hit, where hit is what vd_trace_any*_dev answers on this context, under the options it has
 * (VD_OPT_TRACE_RAY_RANGE included: the ray's pad words are what vd_shadow_rays_dev writes under it), for the ray
 * eye = pos + nor * 0.0001, dir = d.  Every word of every point is written, the bits at and above n_lights as zero, whatever
 * the buffers held before.  The result is a function of the inputs alone: the same bytes for every max_chunk_rays.
 *
 * The calls BLOCK, like every trace call.  n_points == 0 or n_lights == 0: VD_OK, nothing is written (out_info is zeroed).
 * VD_ERR_INVALID_ARG (with a message): null pointers, n_lights > VD_SHADOW_MAX_LIGHTS, n_points * n_lights > 0xf0000000,
 * and whatever the walk refuses.
 */
#ifndef VOIDIN_SHADOW_H
#define VOIDIN_SHADOW_H

#include "voidin_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* crates/pools/src/light.rs:55-62 — 32 B */
typedef struct VdLight {
    float    position[3];
    float    radius;
    float    color[3];           /* not read by the pass */
    uint32_t _pad;
} VdLight;

#define VD_SHADOW_MAX_LIGHTS 1024u

/* What a call did: the rays it wrote and walked (= the in-range pairs), the chunks it cut them into, W. */
typedef struct VdShadowPassInfo {
    uint32_t n_rays;
    uint32_t n_chunks;
    uint32_t words_per_point;
    uint32_t _pad;
} VdShadowPassInfo;

#ifdef __cplusplus
static_assert(sizeof(VdLight) == 32 && sizeof(VdShadowPassInfo) == 16, "shadow pass records");
#else
_Static_assert(sizeof(VdLight) == 32 && sizeof(VdShadowPassInfo) == 16, "shadow pass records");
#endif

/* d_scene: the struct in host memory, its pointers device memory (as vd_trace_any_dev takes it).  d_positions / d_normals:
 * n_points x 3 floats.  d_occluded, d_in_range (may be NULL): n_points * W words.  max_chunk_rays: the rays written and walked
 * at a time (0: the default, 4 Mi) - it bounds the call's scratch (36 bytes per ray of a chunk) and never changes the result;
 * a chunk is a run of whole (light, 512-point tile) cells and holds at least one.  out_info: host memory, may be NULL. */
int vd_shadow_pass_dev(VdCtx* ctx, const VdTraceScene* d_scene, const float* d_positions, const float* d_normals,
                       uint32_t n_points, const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays,
                       uint32_t* d_occluded, uint32_t* d_in_range, VdShadowPassInfo* out_info);
/* ... over a prepared scene: narrow, wide and tight handles alike, as vd_trace_any_prepared_dev takes them. */
int vd_shadow_pass_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const float* d_positions, const float* d_normals,
                                uint32_t n_points, const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays,
                                uint32_t* d_occluded, uint32_t* d_in_range, VdShadowPassInfo* out_info);

#ifdef __cplusplus
}
#endif

#endif /* VOIDIN_SHADOW_H */
