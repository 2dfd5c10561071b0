/*
 * voidin_lighting.h — the lighting pass: the light loop of the shadow shader summed on the device, an extension of the C ABI of
 * libvoidin_hip.so on top of voidin_gbuffer.h (whose conventions, and voidin_shadow.h's and voidin_abi.h's, hold here).
 *
 * vd_shadow_gbuffer*_dev leaves one occlusion bit per pixel and light.  What the reference's shader does with that bit is the rest
 * of its file (src/bin/raytraced_shadows.wgsl:79-117): the base colour, attenuation() (lines 48-55), the diffuse and the specular
 * term, `color += (diff + spec) * occlusion * atten` over the lights in range, the final clamp.  vd_lighting_dev is those lines for
 * a whole image; vd_shade_gbuffer*_dev is the pass and the step in one call - scene + camera + lights in, a lit image out, nothing
 * per pixel through the host.  The shader's textures are out of scope: VdFlatMaterial holds one value per material where the
 * shader samples one per texel, indexed by the material byte, so no index can be out of range.
 *
 * Definition (float32, nothing contracted, divide and square root correctly rounded).
 *     dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z          pos0(x) = x > 0 ? x : 0      (a NaN gives 0)
 * For pixel i with material byte m, `pos` and `nor` exactly as voidin_gbuffer.h defines them, M = materials[m]:
 *   m == VD_GBUFFER_NO_MATERIAL:     rgba = (1, 0, 1, 1)                                            (lines 80-82)
 *   m == VD_GBUFFER_LIGHT_MATERIAL:  c = M.albedo + M.emissive; no light is visited, whatever the bit words hold
 *   otherwise                        c = M.albedo * 0.3f + M.emissive      per component, multiply then add
 *     v    = camera.view_position.xyz - pos;   rd = v / sqrtf(dot(v, v))                             three divisions
 *     covr = pos0(dot(-rd, nor));   c16 = covr squared four times
 *            (a spec decision: WGSL's pow(x, 16.) is not specified to the bit.  For a normal that faces the eye covr is 0, as in the
 *            reference; that is kept.)
 *     then for l = 0 .. n_lights-1 IN ASCENDING ORDER, for every l whose bit in the pixel's in_range words is set - the bit
 *     decides, the rule is not recomputed; bits at and above n_lights are never read as lights; an occluded bit without its
 *     in_range bit means nothing:
 *         d = light.position - pos;   dist = sqrtf(dot(d, d))                                        (voidin_shadow.h's d and dist)
 *         occlusion = occluded bit ? 0.5f : 1.0f
 *         s = dist / light.radius;   s2 = s * s;   q = 1 - s2
 *         atten = (s >= 1) ? 0 : (q * q) / (1 + s2)                          (lines 48-55 with max_intensity = falloff = 1)
 *         ldir = d / dist (three divisions);   shade = pos0(dot(nor, ldir))
 *         per component k:   diff = (light.color[k] * M.albedo[k]) * shade
 *                            spec = (light.color[k] * M.specular) * c16
 *                            c[k] = c[k] + ((diff + spec) * occlusion) * atten
 *     every product is carried out, also with atten == 0: an infinite colour times 0 is a NaN, as in the shader.
 *   rgba = (pos0(c.r), pos0(c.g), pos0(c.b), 1)                                                      (line 117)
 * No NaN ever leaves the call.  Every pixel's 16 bytes are written as ONE 16-byte store; row padding and everything outside the
 * image stay as they are.
 */
#ifndef VOIDIN_LIGHTING_H
#define VOIDIN_LIGHTING_H

#include "voidin_gbuffer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 32 B: what the shader samples from textures, as one value per material */
typedef struct VdFlatMaterial {
    float    albedo[3];          /* albedo.rgb */
    float    specular;           /* metallic_roughness.z */
    float    emissive[3];
    uint32_t _pad;
} VdFlatMaterial;

#define VD_LIGHTING_MATERIALS 256u   /* the material image is R8Uint: the table always has 256 rows */

/* The struct in host memory, its pointer device memory. */
typedef struct VdColorTarget {
    float*   rgba;               /* four floats a pixel */
    uint32_t pitch;              /* bytes per row, multiple of 16, >= 16 * width */
    uint32_t width, height;      /* must equal the G-buffer's */
} VdColorTarget;

#ifdef __cplusplus
static_assert(sizeof(VdFlatMaterial) == 32 && sizeof(VdColorTarget) == 24, "lighting records");
#else
_Static_assert(sizeof(VdFlatMaterial) == 32 && sizeof(VdColorTarget) == 24, "lighting records");
#endif

/* The step alone.  With W = (n_lights + 31) / 32, d_occluded and d_in_range hold W words per PIXEL as vd_shadow_gbuffer_dev writes
 * them, pixel i at i * W.  d_materials: VD_LIGHTING_MATERIALS records.  camera: host memory, read at the call (a captured launch
 * keeps what it was recorded with); view_position and clip_to_world are read.  The call ONLY ENQUEUES on the context's stream: no
 * arena, no read-back, so it can be captured into a graph.
 * n_lights == 0 is legal: W = 0, d_lights and the bit pointers may be NULL, every pixel gets its base colour.
 * width == 0 or height == 0: VD_OK, nothing written.  VD_ERR_INVALID_ARG (with a message), before anything is launched: null
 * pointers (d_lights and the two bit arrays only when n_lights > 0), a target whose size is not the G-buffer's, a pitch below its
 * row or not a multiple of 16, whatever vd_gbuffer_points_dev refuses of a G-buffer, n_lights > VD_SHADOW_MAX_LIGHTS. */
int vd_lighting_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdGBuffer* gb, const VdLight* d_lights, uint32_t n_lights,
                    const uint32_t* d_occluded, const uint32_t* d_in_range, const VdFlatMaterial* d_materials,
                    const VdColorTarget* target);

/* Exactly vd_shadow_gbuffer_dev followed by vd_lighting_dev: the two bit arrays live in a grow-only arena of the context (8 W
 * bytes a pixel).  max_chunk_rays: as the pass takes it.  out_info: host memory, may be NULL; what the pass reports.  The call
 * BLOCKS, like the pass.  With n_lights == 0 it is the step alone (out_info zeroed).  It refuses what either of its two calls
 * refuses, before anything is launched. */
int vd_shade_gbuffer_dev(VdCtx* ctx, const VdTraceScene* d_scene, const VdCameraUniform* camera, const VdGBuffer* gb,
                         const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays, const VdFlatMaterial* d_materials,
                         const VdColorTarget* target, VdShadowGBufferInfo* out_info);
/* ... over a prepared scene: narrow, wide and tight handles alike, as vd_shadow_gbuffer_prepared_dev takes them. */
int vd_shade_gbuffer_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdCameraUniform* camera, const VdGBuffer* gb,
                                  const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays,
                                  const VdFlatMaterial* d_materials, const VdColorTarget* target, VdShadowGBufferInfo* out_info);

#ifdef __cplusplus
}
#endif

#endif /* VOIDIN_LIGHTING_H */
