// gbuffer_trace.hip — the G-buffer from primary rays (include/voidin_gbuffer_trace.h): the ray-traced equivalent of the raster pass
// that fills voidin's GBuffer (shaders/visibility.wgsl), as the harness does it (src/bin/bvh_trace.wgsl:223-248) - a ray through
// every pixel centre, the closest-hit walk of trace.hip through its exported entry points, and a resolve step that turns the hit
// records into depth / normal + uv / material in the layout gbuffer.hip reads.
//
//   gbuffer_rays_kernel     ray i of pixel i = y * width + x: 32 bytes a lane, two 16-byte stores
//   gbuffer_resolve_kernel  ONE PIXEL PER LANE, lane -> pixel i = block * 256 + thread: the 64 records of a wave are 1 KiB in one
//                           piece, and its stores are 64 neighbours of a row (256 B of depth, 512 B of word pairs, 64 material
//                           bytes - byte stores, so any material pitch and any row start work).  Between them lies a dependent
//                           gather: record -> instance (144 B) -> VdMeshInfo -> 3 indices -> 3 x (position, normal, uv).
//                           Neighbouring pixels mostly see the same instance and nearby triangles, so the lanes of a wave share
//                           the lines they gather.  Each level is ONE batch of independent loads (mesh + material; the mesh record's
//                           three words; the three indices; the instance's matrices beside the three vertices and their
//                           attributes), and a pixel that is a miss leaves the chain at the level that says so - its lanes issue
//                           nothing further.
// No atomics, no LDS, no scratch.
//
// The pixel centre in NDC, the octahedral encoder (beside the decoder that reads its codes back), the view of the three images and
// their checks are vd_shade.hpp's: the one copy that gbuffer.hip reads the images with.
#include "vd_shade.hpp"
#include "../../include/voidin_gbuffer_trace.h"

namespace {

constexpr unsigned kBlock = 256u;

// rows 0..2 of M * (p, w), M column-major: ((c0 * x + c1 * y) + c2 * z) + c3 * w
__device__ __forceinline__ V3 mul43(const float* M, V3 p, float w) {
    return V3{((M[0] * p.x + M[4] * p.y) + M[8] * p.z) + M[12] * w, ((M[1] * p.x + M[5] * p.y) + M[9] * p.z) + M[13] * w,
              ((M[2] * p.x + M[6] * p.y) + M[10] * p.z) + M[14] * w};
}
__device__ __forceinline__ float mul_row(const float* M, int r, float x, float y, float z, float w) {
    return ((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r] * w;
}

struct Camera { Mat4 clip_to_world, view, projection; };

// The ray of pixel (x, y): the header's definition.
__device__ __forceinline__ void pixel_ray(const Mat4& c2w, unsigned x, unsigned y, float fw, float fh, V3& eye, V3& dir) {
    float nx, ny;
    pixel_ndc(x, y, fw, fh, nx, ny);
    const float* M = c2w.m;
    const float pw = mul_row(M, 3, nx, ny, 1.0f, 1.0f);
    eye = V3{mul_row(M, 0, nx, ny, 1.0f, 1.0f) / pw, mul_row(M, 1, nx, ny, 1.0f, 1.0f) / pw, mul_row(M, 2, nx, ny, 1.0f, 1.0f) / pw};
    const V3 t = V3{mul_row(M, 0, nx, ny, 0.0f, 1.0f), mul_row(M, 1, nx, ny, 0.0f, 1.0f), mul_row(M, 2, nx, ny, 0.0f, 1.0f)};
    dir = over(t, sqrtf(dot3(t, t)));
}

__global__ __launch_bounds__(kBlock) void gbuffer_rays_kernel(Mat4 c2w, unsigned width, unsigned n_pixels, float fw, float fh, float4* __restrict__ rays) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_pixels) return;
    const unsigned y = i / width, x = i - y * width;
    V3 eye, dir;
    pixel_ray(c2w, x, y, fw, fh, eye, dir);
    rays[2u * (size_t)i] = make_float4(eye.x, eye.y, eye.z, 0.0f);
    rays[2u * (size_t)i + 1u] = make_float4(dir.x, dir.y, dir.z, VD_MAX_DIST);
}

// What the resolve kernel gathers from (it writes to vd_shade.hpp's Target).
struct Geometry {
    const VdInstance* instances; const VdMeshInfo* meshes; const float* vertices; const uint32_t* indices; const float* normals; const float* tex_coords;
    unsigned n_instances, n_meshes, n_vertices, n_indices;
};

__device__ __forceinline__ V3 load3(const float* p, unsigned id) { const float* q = p + 3u * (size_t)id; return V3{q[0], q[1], q[2]}; }
// (a * ((1 - u) - v) + b * u) + c * v
__device__ __forceinline__ float bary(float a, float b, float c, float w, float u, float v) { return (a * w + b * u) + c * v; }
// one half of pack2x16float: the round-to-nearest-even convert (v_cvt_f16_f32 under the default mode; f16 subnormals are kept)
__device__ __forceinline__ unsigned half_bits(float f) {
    const _Float16 h = (_Float16)f;
    unsigned short b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

__global__ __launch_bounds__(kBlock) void gbuffer_resolve_kernel(Camera cam, Geometry g, Target t, float fw, float fh, const uint4* __restrict__ hits) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.n_pixels) return;
    const unsigned y = i / t.width, x = i - y * t.width;
    const uint4 h = hits[i];                            // {dist, hit, instance, triangle}
    float depth = 0.0f;
    uint2 words = make_uint2(0u, 0u);
    unsigned material = 0u;
    if (h.y == 1u && h.z < g.n_instances) {
        // level 1: the instance's mesh and material (its matrices wait until the pixel is known to be a hit: level 4)
        const float4* ip = reinterpret_cast<const float4*>(g.instances + h.z);
        const uint2 tail = *reinterpret_cast<const uint2*>(ip + 8);      // {mesh, material}
        if (tail.x < g.n_meshes) {
            // level 2: the mesh record's words (`&`: neither test waits for the other's word; the compiler fetches vertex_offset
            // beside the indices, where it is first needed)
            const VdMeshInfo* mp = g.meshes + tail.x;
            const unsigned index_count = mp->index_count, base_index = mp->base_index, vertex_offset = (unsigned)mp->vertex_offset;
            const unsigned long long last = 3ull * h.w + 2ull;
            if ((last < index_count) & (base_index + last < g.n_indices)) {
                // level 3: the three indices
                const uint32_t* ix = g.indices + ((size_t)base_index + 3u * (size_t)h.w);
                const unsigned id0 = ix[0] + vertex_offset, id1 = ix[1] + vertex_offset, id2 = ix[2] + vertex_offset;      // bvh.wgsl:31
                if ((id0 < g.n_vertices) & (id1 < g.n_vertices) & (id2 < g.n_vertices)) {
                    // level 4: the instance's two matrices and the three vertices with their attributes, every load issued before the
                    // first is used
                    float4 c[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) c[k] = ip[k];
                    const V3 v0 = load3(g.vertices, id0), v1 = load3(g.vertices, id1), v2 = load3(g.vertices, id2);
                    V3 n0 = V3{0, 0, 0}, n1 = n0, n2 = n0;
                    float2 t0 = make_float2(0, 0), t1 = t0, t2 = t0;
                    if (g.normals) { n0 = load3(g.normals, id0); n1 = load3(g.normals, id1); n2 = load3(g.normals, id2); }
                    if (g.tex_coords) {
                        t0 = *reinterpret_cast<const float2*>(g.tex_coords + 2u * (size_t)id0);
                        t1 = *reinterpret_cast<const float2*>(g.tex_coords + 2u * (size_t)id1);
                        t2 = *reinterpret_cast<const float2*>(g.tex_coords + 2u * (size_t)id2);
                    }
                    const float T[16] = {c[0].x, c[0].y, c[0].z, c[0].w, c[1].x, c[1].y, c[1].z, c[1].w, c[2].x, c[2].y, c[2].z, c[2].w, c[3].x, c[3].y, c[3].z, c[3].w};
                    const float Ti[16] = {c[4].x, c[4].y, c[4].z, c[4].w, c[5].x, c[5].y, c[5].z, c[5].w, c[6].x, c[6].y, c[6].z, c[6].w, c[7].x, c[7].y, c[7].z, c[7].w};
                    V3 eye, dir;
                    pixel_ray(cam.clip_to_world, x, y, fw, fh, eye, dir);
                    // depth (visibility.wgsl:35-40)
                    const float dist = __uint_as_float(h.x);
                    const V3 p = V3{eye.x + dir.x * dist, eye.y + dir.y * dist, eye.z + dir.z * dist};
                    const float* V = cam.view.m;
                    const float* P = cam.projection.m;
                    const float vx = mul_row(V, 0, p.x, p.y, p.z, 1.0f), vy = mul_row(V, 1, p.x, p.y, p.z, 1.0f), vz = mul_row(V, 2, p.x, p.y, p.z, 1.0f),
                                vw = mul_row(V, 3, p.x, p.y, p.z, 1.0f);
                    depth = mul_row(P, 2, vx, vy, vz, vw) / mul_row(P, 3, vx, vy, vz, vw);
                    // barycentrics (bvh.wgsl:82-83, intersections.wgsl:26-36)
                    const V3 oe = mul43(Ti, eye, 1.0f), od = mul43(Ti, dir, 0.0f);
                    const V3 edge1 = v1 - v0, edge2 = v2 - v0;
                    const V3 uvec = cross3(od, edge2);
                    const float inv_det = 1.0f / dot3(edge1, uvec);
                    const V3 orig = oe - v0;
                    const float u = inv_det * dot3(orig, uvec);
                    const V3 vvec = cross3(orig, edge1);
                    const float v = inv_det * dot3(od, vvec);
                    const float w = (1.0f - u) - v;
                    V3 n;
                    if (g.normals) {                    // visibility.wgsl:42-43
                        const V3 ni = V3{bary(n0.x, n1.x, n2.x, w, u, v), bary(n0.y, n1.y, n2.y, w, u, v), bary(n0.z, n1.z, n2.z, w, u, v)};
                        n = V3{(T[0] * ni.x + T[4] * ni.y) + T[8] * ni.z, (T[1] * ni.x + T[5] * ni.y) + T[9] * ni.z, (T[2] * ni.x + T[6] * ni.y) + T[10] * ni.z};
                    } else {                            // the harness's triangle normal, facing the eye
                        const V3 w0 = mul43(T, v0, 1.0f), w1 = mul43(T, v1, 1.0f), w2 = mul43(T, v2, 1.0f);
                        n = cross3(w1 - w0, w2 - w0);
                        if (dot3(n, dir) > 0.0f) n = V3{-n.x, -n.y, -n.z};
                    }
                    n = over(n, sqrtf(dot3(n, n)));
                    words.x = encode_octahedral(n);
                    if (g.tex_coords) words.y = half_bits(bary(t0.x, t1.x, t2.x, w, u, v)) | (half_bits(bary(t0.y, t1.y, t2.y, w, u, v)) << 16);
                    material = tail.y & 0xffu;
                }
            }
        }
    }
    *t.depth_at(x, y) = depth;
    *reinterpret_cast<uint2*>(t.normal_uv_at(x, y)) = words;      // the pair in one store
    *t.material_at(x, y) = (uint8_t)material;
}

int check_geometry(VdCtx* ctx, const char* name, const VdGBufferGeometry* g) {
    return !g->instances || !g->meshes || !g->vertices || !g->indices ? vd_fail_arg(ctx, name, "null pointer") : VD_OK;
}

Mat4 mat4(const float* m) { Mat4 r; memcpy(r.m, m, sizeof(r.m)); return r; }

// Both launches: the arguments have been checked and the image is not empty.
int launch_rays(VdCtx* ctx, const VdCameraUniform* camera, uint32_t width, uint32_t height, VdRay* d_rays) {
    const unsigned n = width * height;
    hipLaunchKernelGGL(gbuffer_rays_kernel, dim3((n + kBlock - 1u) / kBlock), dim3(kBlock), 0, ctx->stream, mat4(camera->clip_to_world), width, n, (float)width,
                       (float)height, reinterpret_cast<float4*>(d_rays));
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int launch_resolve(VdCtx* ctx, const VdCameraUniform* camera, const VdGBufferGeometry* g, const VdHit* d_hits, const VdGBufferTarget* tg) {
    const unsigned n = tg->width * tg->height;
    const Camera cam = {mat4(camera->clip_to_world), mat4(camera->view), mat4(camera->projection)};
    const Geometry geo = {g->instances, g->meshes, g->vertices, g->indices, g->normals, g->tex_coords, g->n_instances, g->n_meshes, g->n_vertices, g->n_indices};
    hipLaunchKernelGGL(gbuffer_resolve_kernel, dim3((n + kBlock - 1u) / kBlock), dim3(kBlock), 0, ctx->stream, cam, geo, vd_images<char>(tg), (float)tg->width, (float)tg->height,
                       reinterpret_cast<const uint4*>(d_hits));
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// Both composed forms: exactly one of scene / accel is given (the entry points have checked that it is not null).
int gbuffer_trace(VdCtx* ctx, const char* name, const VdTraceScene* scene, const VdTraceAccel* accel, const VdGBufferGeometry* g, const VdCameraUniform* camera,
                  const VdGBufferTarget* tg) {
    if (!tg) return vd_fail_arg(ctx, name, "null pointer");
    if (tg->width == 0 || tg->height == 0) return VD_OK;
    if (!camera) return vd_fail_arg(ctx, name, "null pointer");
    int rc = vd_check_images(ctx, name, tg);
    if (rc || (rc = check_geometry(ctx, name, g))) return rc;
    const unsigned n = tg->width * tg->height;
    VdRay* d_rays = nullptr; VdHit* d_hits = nullptr;
    if ((rc = vd_carve(ctx, &ctx->gbuffer_trace, [&](Arena& a) { d_rays = a.take<VdRay>(n); d_hits = a.take<VdHit>(n); }))) return rc;
    if ((rc = launch_rays(ctx, camera, tg->width, tg->height, d_rays))) return rc;
    rc = scene ? vd_trace_dev(ctx, scene, d_rays, n, d_hits) : vd_trace_prepared_dev(ctx, accel, d_rays, n, d_hits);
    if (rc) return rc;
    return launch_resolve(ctx, camera, g, d_hits, tg);
}

}  // namespace

extern "C" {

int vd_gbuffer_rays_dev(VdCtx* ctx, const VdCameraUniform* camera, uint32_t width, uint32_t height, VdRay* d_rays) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    const char* name = "vd_gbuffer_rays";
    if (width == 0 || height == 0) return VD_OK;
    if (!camera || !d_rays) return vd_fail_arg(ctx, name, "null pointer");
    const int rc = vd_check_pixels(ctx, name, width, height);
    return rc ? rc : launch_rays(ctx, camera, width, height, d_rays);
}

int vd_gbuffer_resolve_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdGBufferGeometry* geometry, const VdHit* d_hits, const VdGBufferTarget* target) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    const char* name = "vd_gbuffer_resolve";
    if (!target) return vd_fail_arg(ctx, name, "null pointer");
    if (target->width == 0 || target->height == 0) return VD_OK;
    if (!camera || !geometry || !d_hits) return vd_fail_arg(ctx, name, "null pointer");
    int rc = vd_check_images(ctx, name, target);
    if (rc || (rc = check_geometry(ctx, name, geometry))) return rc;
    return launch_resolve(ctx, camera, geometry, d_hits, target);
}

int vd_gbuffer_trace_dev(VdCtx* ctx, const VdTraceScene* d_scene, const float* d_normals, const float* d_tex_coords, const VdCameraUniform* camera,
                         const VdGBufferTarget* target) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_scene) return vd_fail_arg(ctx, "vd_gbuffer_trace", "null scene");
    const VdGBufferGeometry g = {d_scene->instances, d_scene->n_instances, d_scene->meshes, d_scene->n_meshes, d_scene->vertices, d_scene->n_vertices,
                                 d_scene->indices, d_scene->n_indices, d_normals, d_tex_coords};
    return gbuffer_trace(ctx, "vd_gbuffer_trace", d_scene, nullptr, &g, camera, target);
}

int vd_gbuffer_trace_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdGBufferGeometry* geometry, const VdCameraUniform* camera,
                                  const VdGBufferTarget* target) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!accel) return vd_fail_arg(ctx, "vd_gbuffer_trace_prepared", "null accel");
    if (!geometry) return vd_fail_arg(ctx, "vd_gbuffer_trace_prepared", "null pointer");
    return gbuffer_trace(ctx, "vd_gbuffer_trace_prepared", nullptr, accel, geometry, camera, target);
}

}  // extern "C"
