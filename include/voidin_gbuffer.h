/*
 * voidin_gbuffer.h — the shadow pass straight from the G-buffer, an extension of the C ABI of libvoidin_hip.so on top of
 * voidin_shadow.h (whose conventions, and voidin_abi.h's, hold here).
 *
 * vd_shadow_pass*_dev takes world positions and normals.  What the reference's shadow shader has instead
 * (src/bin/raytraced_shadows.wgsl:62-89) is voidin's GBuffer (crates/app/src/app/gbuffer.rs:15-17): a depth image, an Rg32Uint
 * image whose first word is an octahedral normal (shaders/visibility.wgsl:85-90, shaders/utils/encoding.wgsl:17-28) and an
 * R8Uint material image.  Its lines 62-89 turn these into `pos` and `nor` and decide which pixels run the light loop at all.
 * vd_gbuffer_points_dev is those lines for a whole image, with an ordered compaction; vd_shadow_gbuffer*_dev runs the pass on
 * the result and hands the bits back PER PIXEL, so that the shader binds three images and reads one bit per light.
 *
 * Definition (float32, nothing contracted, divide and square root correctly rounded).  For pixel (x, y), i = y * width + x:
 *     uv   = (((float)x + 0.5f) / (float)width, ((float)y + 0.5f) / (float)height)
 *            (the pixel centre, shaders/utils/uv.wgsl:1-3.  A spec decision: the shader's interpolated `in.uv` is this value up
 *            to the rasteriser, which is not specified to the bit.)
 *     ndc  = (uv.x * 2 - 1, (1 - uv.y) * 2 - 1, depth(x, y))
 *     w4   = clip_to_world * (ndc, 1), every row as ((c0 * ndc.x + c1 * ndc.y) + c2 * ndc.z) + c3   (c0..c3: the columns)
 *     pos  = (w4.x / w4.w, w4.y / w4.w, w4.z / w4.w)                     three true divisions (uv.wgsl:13-22)
 *   the normal, from word 0 `n32` of the pixel's normal_uv pair (encoding.wgsl:17-28):
 *     v    = ((float)(n32 & 0xffff) / 65535.0f, (float)((n32 >> 16) & 0xffff) / 65535.0f);   v = v * 2 - 1
 *     n    = (v.x, v.y, (1 - |v.x|) - |v.y|)
 *     t    = (-n.z > 0) ? -n.z : 0
 *     n.x += (n.x > 0) ? -t : t;   n.y += (n.y > 0) ? -t : t
 *     nor  = n / sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z)                    three divisions
 *   RECEIVER: material(x, y) != VD_GBUFFER_NO_MATERIAL && material(x, y) != VD_GBUFFER_LIGHT_MATERIAL.  Nothing else decides it:
 *   a receiver with depth 0, NaN or infinite stays a receiver, its point is whatever the arithmetic gives and its bits are
 *   whatever the pass gives for that point.
 *   The receivers, in ascending i, are the POINTS 0 .. n_points-1.
 *
 * Depth follows the convention of vd_hiz_build_dev: float32, reverse Z, row 0 at the top.  Every image has a pitch of its own in
 * bytes, because a copy_texture_to_buffer pads rows to 256 bytes; a packed image passes 4 * width, 8 * width and width.
 */
#ifndef VOIDIN_GBUFFER_H
#define VOIDIN_GBUFFER_H

#include "voidin_shadow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VD_GBUFFER_NO_MATERIAL    0u   /* raytraced_shadows.wgsl:80 */
#define VD_GBUFFER_LIGHT_MATERIAL 2u   /* shared.wgsl:1 */

/* The struct in host memory, its pointers device memory. */
typedef struct VdGBuffer {
    const float*    depth;      uint32_t depth_pitch;      /* bytes per row, multiple of 4, >= 4 * width */
    const uint32_t* normal_uv;  uint32_t normal_uv_pitch;  /* bytes per row, multiple of 8, >= 8 * width; word 0 = normal, word 1 = uv (never read) */
    const uint8_t*  material;   uint32_t material_pitch;   /* bytes per row, >= width */
    uint32_t width, height;                                /* width * height <= 2^30, as vd_hiz_layout */
} VdGBuffer;

/* What a vd_shadow_gbuffer*_dev call did: the receivers it found, and of the pass over them the rays, the chunks and W. */
typedef struct VdShadowGBufferInfo {
    uint32_t n_points;
    uint32_t n_rays;
    uint32_t n_chunks;
    uint32_t words_per_point;
} VdShadowGBufferInfo;

#ifdef __cplusplus
static_assert(sizeof(VdGBuffer) == 56 && sizeof(VdShadowGBufferInfo) == 16, "g-buffer records");
#else
_Static_assert(sizeof(VdGBuffer) == 56 && sizeof(VdShadowGBufferInfo) == 16, "g-buffer records");
#endif

/* The points of a G-buffer: d_positions / d_normals (3 floats a point) and d_pixels (the point's i) take width * height entries
 * at most and are written for the points alone - nothing at or beyond n_points; *d_n_points (device) takes the count.  camera:
 * host memory, only clip_to_world is read (at the call: a captured launch keeps the matrix it was recorded with).
 * out_n_points == NULL: the call only enqueues on the context's stream - no read-back, so it can be captured into a graph once
 * the context's tables have their size (they grow with the image, which drains the stream).  Otherwise it BLOCKS and
 * *out_n_points is the count.  The order is defined without an atomic: count per 512-pixel tile, scan, write at the tile's
 * offset plus the ballot rank.
 * width == 0 or height == 0: VD_OK, nothing is written on the device (*out_n_points = 0).  VD_ERR_INVALID_ARG (with a message),
 * before anything is launched: null pointers, a pitch below its row or not a multiple of its element, width * height > 2^30. */
int vd_gbuffer_points_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdGBuffer* gb, float* d_positions, float* d_normals,
                          uint32_t* d_pixels, uint32_t* d_n_points, uint32_t* out_n_points);

/* The shadow loop for every pixel of a G-buffer.  With W = (n_lights + 31) / 32, d_occluded and d_in_range (may be NULL) hold W
 * words per PIXEL, packed, pixel i at i * W.  A receiver's words are exactly the words vd_shadow_pass_dev writes for its point
 * under the context's options (VD_OPT_TRACE_RAY_RANGE included); every other pixel's words are zero.  Every word of every pixel
 * is written whatever the buffers held - also by a call that finds no receiver at all, which walks nothing.  max_chunk_rays: as
 * the pass takes it.  out_info: host memory, may be NULL.  The call BLOCKS, like the pass.  Points, normals and the per-point
 * words live in a grow-only arena of the context (28 bytes + 8 W a receiver).
 * n_lights == 0, width == 0 or height == 0: VD_OK, out_info zeroed, nothing written.  VD_ERR_INVALID_ARG (with a message),
 * before anything is launched: what vd_gbuffer_points_dev refuses, n_lights > VD_SHADOW_MAX_LIGHTS,
 * width * height * n_lights > 0xf0000000, and whatever the pass refuses. */
int vd_shadow_gbuffer_dev(VdCtx* ctx, const VdTraceScene* d_scene, const VdCameraUniform* camera, const VdGBuffer* gb,
                          const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays, uint32_t* d_occluded,
                          uint32_t* d_in_range, VdShadowGBufferInfo* out_info);
/* ... over a prepared scene: narrow, wide and tight handles alike, as vd_shadow_pass_prepared_dev takes them. */
int vd_shadow_gbuffer_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdCameraUniform* camera, const VdGBuffer* gb,
                                   const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays, uint32_t* d_occluded,
                                   uint32_t* d_in_range, VdShadowGBufferInfo* out_info);

#ifdef __cplusplus
}
#endif

#endif /* VOIDIN_GBUFFER_H */
