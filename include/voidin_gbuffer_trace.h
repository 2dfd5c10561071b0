/*
 * voidin_gbuffer_trace.h — the G-buffer from primary rays, an extension of the C ABI of libvoidin_hip.so on top of
 * voidin_gbuffer.h (whose conventions, and voidin_shadow.h's and voidin_abi.h's, hold here).
 *
 * voidin_gbuffer.h READS the three images of voidin's GBuffer (crates/app/src/app/gbuffer.rs:15-17).  In the reference the raster
 * pass writes them (shaders/visibility.wgsl), which needs a Vulkan device.  Its other harness shows the ray-traced equivalent
 * (src/bin/bvh_trace.wgsl:223-248): primary ray -> traverse_tlas -> the triangle's normal.  This header is that chain for a whole
 * image: pixel-centre rays, the closest-hit walk of vd_trace*_dev, and a RESOLVE step that turns every VdHit into the pixel's depth,
 * Rg32Uint normal + uv pair and R8Uint material, in exactly the layout VdGBuffer reads - so the result feeds vd_gbuffer_points_dev
 * and vd_shadow_gbuffer*_dev as it is.
 *
 * Definition (float32, nothing contracted, divide and square root correctly rounded).  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;
 * cross(a, b) = (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y); M * (x, y, z, w) = ((c0*x + c1*y) + c2*z) + c3*w per row
 * (c0..c3: the columns), with the products by w = 1 and w = 0 carried out.
 *
 * The RAY of pixel (x, y), i = y * width + x:
 *     uv   = (((float)x + 0.5f) / (float)width, ((float)y + 0.5f) / (float)height)      the pixel centre, as voidin_gbuffer.h
 *     ndc  = (uv.x * 2 - 1, (1 - uv.y) * 2 - 1)
 *     P    = clip_to_world * (ndc, 1, 1);   eye = (P.x / P.w, P.y / P.w, P.z / P.w)
 *     T    = clip_to_world * (ndc, 0, 1);   dir = T.xyz / sqrtf(dot(T.xyz, T.xyz))                  three divisions each
 *     _pad0 = 0, _pad1 = VD_MAX_DIST: the whole half-line, so VD_OPT_TRACE_RAY_RANGE changes nothing.
 *   A spec decision: the formula of the harness (bvh_trace.wgsl:227-231) at the pixel centre, with the y convention of
 *   ndc_from_uv_raw_depth (shaders/utils/uv.wgsl) - so that world_position_from_depth of the depth written below lands on the same
 *   line.  (vd_primary_rays_dev is the CPU harness's ray, src/bin/bvh_cpu.rs:71-83: pixel corners, another y, a reciprocal.)
 *   The resolve step recomputes this ray from the camera; it takes no ray buffer.
 *
 * A pixel is a MISS - depth = 0, both words 0, material = 0 - unless ALL of these hold for its record h:
 *     h.hit == 1;   h.instance < n_instances;   mesh = instances[h.instance].mesh < n_meshes;
 *     3 * h.triangle + 2 < meshes[mesh].index_count;   meshes[mesh].base_index + 3 * h.triangle + 2 < n_indices;
 *     id_k = indices[base_index + 3 * h.triangle + k] + (uint32_t)vertex_offset < n_vertices for k = 0, 1, 2  (bvh.wgsl:30-33)
 *   (the sums without wrap-around, the vertex id with it, as the shader's u32 has it) - so the call is total on hand-made records.
 *
 * A hit pixel, with I = instances[h.instance] and v_k = the position of vertex id_k:
 *   depth   p = eye + dir * h.dist (multiply, then add);  clip = projection * (view * (p, 1))  (visibility.wgsl:35-40);
 *           depth = clip.z / clip.w, whatever that gives (clip.w == 0: an infinity or a NaN).
 *   u, v    the object-space ray of instance_intersect (bvh.wgsl:82-83): oe = (I.inv_transform * (eye, 1)).xyz,
 *           od = (I.inv_transform * (dir, 0)).xyz; then the expressions of intersect_trig (intersections.wgsl:26-36), all of them
 *           evaluated, none of its early returns taken:  edge1 = v1 - v0, edge2 = v2 - v0, uvec = cross(od, edge2),
 *           inv_det = 1 / dot(edge1, uvec), orig = oe - v0, u = inv_det * dot(orig, uvec), vvec = cross(orig, edge1),
 *           v = inv_det * dot(od, vvec).  The distance is NOT recomputed: h.dist is the walk's.
 *   normal  normals == NULL (geometric): w_k = (I.transform * (v_k, 1)).xyz;  n = cross(w1 - w0, w2 - w0), negated when
 *           dot(n, dir) > 0 (a mirrored instance: the normal faces the eye);  n = n / sqrtf(dot(n, n)).
 *           normals given: n = (n_0 * ((1 - u) - v) + n_1 * u) + n_2 * v per component (n_k: the normal of vertex id_k), then
 *           mat3(I.transform) * n = (c0*n.x + c1*n.y) + c2*n.z (visibility.wgsl:42-43 - NOT the inverse transpose: what the
 *           reference does under a non-uniform scale is kept), then n / sqrtf(dot(n, n)).  No facing flip: the reference has none.
 *   word 0  encode_octahedral_32(n) (shaders/utils/encoding.wgsl:4-15): s = (|n.x| + |n.y|) + |n.z|, q = n / s (three divisions);
 *           q.z < 0: (q.x, q.y) = ((1 - |q.y|) * sign(q.x), (1 - |q.x|) * sign(q.y));  d = floor((q * 0.5 + 0.5) * 65535 + 0.5);
 *           word = d.y << 16 | d.x.  Two departures: the fold's sign(0) counts as +1 (WGSL's is 0, which sends (0, 0, -1) to the
 *           code of (0, 0, 1)), and the float -> u32 conversion sends a NaN to 0 and clamps to [0, 65535] - a normal of length
 *           zero encodes as word 0.
 *   word 1  tex_coords == NULL: 0.  Otherwise t = (t_0 * ((1 - u) - v) + t_1 * u) + t_2 * v per component and
 *           pack2x16float(t) = f16(t.x) | f16(t.y) << 16: round to nearest even, overflow to infinity, f16 subnormals kept, a NaN
 *           stays a NaN (which one is not specified).
 *   material  the low 8 bits of I.material - so material 256 reads downstream as VD_GBUFFER_NO_MATERIAL, "no material".
 *
 * normals and tex_coords are laid out as the reference's MeshPool lays them (crates/pools/src/mesh/mod.rs:316-318): one normal
 * (3 floats) and one uv (2 floats) per position, in the same order - the vertex id that fetches a position fetches its attributes.
 */
#ifndef VOIDIN_GBUFFER_TRACE_H
#define VOIDIN_GBUFFER_TRACE_H

#include "voidin_gbuffer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* VdGBuffer with writable pointers: the same offsets and the same pitch rules (depth_pitch a multiple of 4 and >= 4 * width,
 * normal_uv_pitch a multiple of 8 and >= 8 * width, material_pitch >= width; width * height <= 2^30).  The struct in host memory,
 * its pointers device memory; the word pair of a pixel is written as ONE 8-byte store. */
typedef struct VdGBufferTarget {
    float*    depth;      uint32_t depth_pitch;
    uint32_t* normal_uv;  uint32_t normal_uv_pitch;
    uint8_t*  material;   uint32_t material_pitch;
    uint32_t  width, height;
} VdGBufferTarget;

/* What the resolve step gathers from: the struct in host memory, its pointers device memory. */
typedef struct VdGBufferGeometry {
    const VdInstance* instances;  uint32_t n_instances;
    const VdMeshInfo* meshes;     uint32_t n_meshes;
    const float*      vertices;   uint32_t n_vertices;   /* xyz triples */
    const uint32_t*   indices;    uint32_t n_indices;    /* reordered, as the BLAS build left them */
    const float*      normals;                           /* 3 floats per vertex, may be NULL */
    const float*      tex_coords;                        /* 2 floats per vertex, may be NULL */
} VdGBufferGeometry;

#ifdef __cplusplus
static_assert(sizeof(VdGBufferTarget) == 56 && sizeof(VdGBufferGeometry) == 80, "g-buffer trace records");
#else
_Static_assert(sizeof(VdGBufferTarget) == 56 && sizeof(VdGBufferGeometry) == 80, "g-buffer trace records");
#endif

/* Every call: width == 0 or height == 0 returns VD_OK and writes nothing.  VD_ERR_INVALID_ARG (with a message), before anything is
 * launched: null pointers (normals and tex_coords may be null), a pitch below its row or not a multiple of its element,
 * width * height > 2^30.  camera: host memory, read at the call (a captured launch keeps the matrices it was recorded with).
 * Only pixel bytes are written: 4 + 8 + 1 per pixel; row padding beyond `width` and everything outside the images stay as they are. */

/* The rays above, d_rays[i] for pixel i (width * height of them).  Only clip_to_world is read.  Enqueues on the context's stream. */
int vd_gbuffer_rays_dev(VdCtx* ctx, const VdCameraUniform* camera, uint32_t width, uint32_t height, VdRay* d_rays);

/* The resolve step: d_hits[i] (width * height records, as vd_trace*_dev left them for the rays above - or any records at all) into
 * the three images.  clip_to_world, view and projection are read.  Enqueues on the context's stream. */
int vd_gbuffer_resolve_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdGBufferGeometry* geometry, const VdHit* d_hits,
                           const VdGBufferTarget* target);

/* Exactly vd_gbuffer_rays_dev -> vd_trace_dev -> vd_gbuffer_resolve_dev (the geometry: the scene's own four buffers), the rays and
 * records in a grow-only arena of the context (48 bytes a pixel).  Whatever the walk does about blocking and errors, this does. */
int vd_gbuffer_trace_dev(VdCtx* ctx, const VdTraceScene* d_scene, const float* d_normals, const float* d_tex_coords,
                         const VdCameraUniform* camera, const VdGBufferTarget* target);
/* ... -> vd_trace_prepared_dev -> ...: narrow, wide and tight handles alike.  The handle does not give its buffers away, so the
 * geometry comes beside it: the instances, meshes, vertices and indices it was prepared from. */
int vd_gbuffer_trace_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdGBufferGeometry* geometry,
                                  const VdCameraUniform* camera, const VdGBufferTarget* target);

#ifdef __cplusplus
}
#endif

#endif /* VOIDIN_GBUFFER_TRACE_H */
