// The G-buffer from primary rays through the C++ mirror (include/voidin.hpp): gbuffer_trace and TraceScene::gbuffer_trace against the
// three calls they are made of - gbuffer_rays, the walk, gbuffer_resolve - and the result fed to gbuffer_points as it is.
// A 4 x 1 image under a pinhole at (0, 0, 5) looking down -z with a 90 degree field of view: clip = (x, y, 1/8, 5 - z), and
// clip_to_world is its inverse, so pixel k has eye = (n_k / 8, 0, 4.875) and dir = (n_k, 0, -1) / |..| with n_k = -3/4, -1/4, 1/4, 3/4.
// The rays cross z = 0 at x = 5 n_k, where two octahedra (vertices at +-1) wait for pixels 1 and 3; pixels 0 and 2 see nothing.
// The depth of a hit near z = 0.5 is about 0.028.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/voidin.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <typename T> static T* to_device(const T* host, size_t count) {
    T* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), count * sizeof(T)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

struct Pixels { float depth[4]; uint32_t words[8]; unsigned char material[4]; };

// the three images: rows of 256 bytes, prefilled; -> false when a byte beyond the four pixels changed
static bool read_back(const VdGBufferTarget& t, Pixels* out) {
    unsigned char rows[3][256];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(rows[0], t.depth, 256, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(rows[1], t.normal_uv, 256, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(rows[2], t.material, 256, hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    const size_t used[3] = {16, 32, 4};
    for (int r = 0; r < 3; ++r)
        for (size_t b = used[r]; b < 256; ++b) if (rows[r][b] != 0xC3) return false;
    std::memcpy(out->depth, rows[0], 16); std::memcpy(out->words, rows[1], 32); std::memcpy(out->material, rows[2], 4);
    return true;
}

int main() {
    static_assert(sizeof(VdGBufferTarget) == sizeof(VdGBuffer) && sizeof(VdGBufferGeometry) == 80, "the G-buffer trace records");
    voidin::Gpu gpu(0);
    std::vector<voidin::Vec3> v = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
    std::vector<uint32_t> idx = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    voidin::MeshPool pool(gpu);
    REQUIRE(pool.add({v.data(), v.size(), idx.data(), idx.size()}) == 0);
    const float centre[2][3] = {{-1.05f, 0.1f, 0.0f}, {3.95f, -0.1f, 0.0f}};
    const uint32_t material[2] = {7u, 0x1ffu};
    std::vector<voidin::Instance> inst(2);
    for (int k = 0; k < 2; ++k) {
        std::memset(&inst[k], 0, sizeof(inst[k]));
        for (int d = 0; d < 4; ++d) inst[k].transform[5 * d] = inst[k].inv_transform[5 * d] = 1.0f;
        for (int c = 0; c < 3; ++c) { inst[k].transform[12 + c] = centre[k][c]; inst[k].inv_transform[12 + c] = -centre[k][c]; }
        inst[k].material = material[k];
    }
    pool.generate_tlas(inst);
    const VdTraceScene scene = pool.trace_scene(inst);
    VdTraceScene ds = scene;
    ds.tlas_nodes = to_device(scene.tlas_nodes, scene.n_tlas_nodes); ds.instances = to_device(scene.instances, scene.n_instances);
    ds.meshes = to_device(scene.meshes, scene.n_meshes); ds.bvh_nodes = to_device(scene.bvh_nodes, scene.n_bvh_nodes);
    ds.vertices = to_device(scene.vertices, 3 * (size_t)scene.n_vertices); ds.indices = to_device(scene.indices, scene.n_indices);
    REQUIRE(ds.tlas_nodes && ds.instances && ds.meshes && ds.bvh_nodes && ds.vertices && ds.indices);
    // MeshPool's normals and tex_coords: one per position; the same normal and the same uv everywhere interpolate to themselves
    std::vector<float> normals, uvs;
    for (size_t k = 0; k < scene.n_vertices; ++k) { normals.insert(normals.end(), {0.0f, 0.0f, 1.0f}); uvs.insert(uvs.end(), {0.5f, 0.25f}); }
    const float* d_normals = to_device(normals.data(), normals.size());
    const float* d_uvs = to_device(uvs.data(), uvs.size());
    REQUIRE(d_normals && d_uvs);

    VdCameraUniform camera;
    std::memset(&camera, 0, sizeof(camera));
    camera.clip_to_world[0] = 0.125f; camera.clip_to_world[5] = 0.125f; camera.clip_to_world[10] = 5.0f; camera.clip_to_world[11] = 1.0f; camera.clip_to_world[14] = -0.125f;
    for (int d = 0; d < 4; ++d) camera.view[5 * d] = 1.0f;
    camera.projection[0] = camera.projection[5] = 1.0f; camera.projection[11] = -1.0f; camera.projection[14] = 0.125f; camera.projection[15] = 5.0f;

    std::vector<unsigned char> fill(256, 0xC3);
    VdGBufferTarget target;
    std::memset(&target, 0, sizeof(target));
    target.depth = reinterpret_cast<float*>(to_device(fill.data(), 256)); target.depth_pitch = 256;
    target.normal_uv = reinterpret_cast<uint32_t*>(to_device(fill.data(), 256)); target.normal_uv_pitch = 256;
    target.material = to_device(fill.data(), 256); target.material_pitch = 255;
    target.width = 4; target.height = 1;
    VdRay* d_rays = nullptr; VdHit* d_hits = nullptr;
    REQUIRE(target.depth && target.normal_uv && target.material && hipMalloc(reinterpret_cast<void**>(&d_rays), 4 * sizeof(VdRay)) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&d_hits), 4 * sizeof(VdHit)) == hipSuccess);

    // the three calls
    voidin::TraceScene prepared(gpu, ds);
    voidin::gbuffer_rays(gpu, camera, 4, 1, d_rays);
    VdRay rays[4];
    REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(rays, d_rays, sizeof(rays), hipMemcpyDeviceToHost) == hipSuccess);
    for (int k = 0; k < 4; ++k) {
        const float x = -0.75f + 0.5f * k, len = std::sqrt(x * x + 1.0f);
        REQUIRE(rays[k].eye[0] == x / 8.0f && rays[k].eye[1] == 0.0f && rays[k].eye[2] == 4.875f && rays[k]._pad0 == 0.0f && rays[k]._pad1 == VD_MAX_DIST);
        REQUIRE(std::fabs(rays[k].dir[0] - x / len) < 1e-6f && rays[k].dir[1] == 0.0f && std::fabs(rays[k].dir[2] + 1.0f / len) < 1e-6f);
    }
    prepared.trace(d_rays, 4, d_hits);
    VdHit hits[4];
    REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(hits, d_hits, sizeof(hits), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(hits[0].hit == 0 && hits[1].hit == 1 && hits[1].instance == 0 && hits[2].hit == 0 && hits[3].hit == 1 && hits[3].instance == 1);
    const VdGBufferGeometry with = {ds.instances, ds.n_instances, ds.meshes, ds.n_meshes, ds.vertices, ds.n_vertices, ds.indices, ds.n_indices, d_normals, d_uvs};
    VdGBufferGeometry bare = with;
    bare.normals = nullptr; bare.tex_coords = nullptr;

    for (int attributes = 0; attributes < 2; ++attributes) {
        const VdGBufferGeometry& g = attributes ? with : bare;
        Pixels want, got;
        voidin::gbuffer_resolve(gpu, camera, g, d_hits, target);
        REQUIRE(read_back(target, &want));
        for (int k = 0; k < 4; ++k) {
            if (k % 2 == 0) { REQUIRE(want.depth[k] == 0.0f && want.words[2 * k] == 0u && want.words[2 * k + 1] == 0u && want.material[k] == 0); continue; }
            REQUIRE(want.depth[k] > 0.02f && want.depth[k] < 0.04f && want.material[k] == (material[k / 2] & 0xffu));
            REQUIRE(want.words[2 * k + 1] == (attributes ? 0x34003800u : 0u));                       // f16(0.5) | f16(0.25) << 16
            if (attributes) REQUIRE(want.words[2 * k] == 0x80008000u);                               // (0, 0, 1)
            else REQUIRE((want.words[2 * k] & 0xffffu) != 0x8000u && want.words[2 * k] != 0u);     // a face of the octahedron: x is not 0
        }
        // the composed calls give the same bytes
        for (int form = 0; form < 2; ++form) {
            REQUIRE(hipMemset(target.depth, 0xC3, 256) == hipSuccess && hipMemset(target.normal_uv, 0xC3, 256) == hipSuccess &&
                    hipMemset(target.material, 0xC3, 256) == hipSuccess);
            if (form) prepared.gbuffer_trace(g, camera, target);
            else voidin::gbuffer_trace(gpu, ds, g.normals, g.tex_coords, camera, target);
            REQUIRE(read_back(target, &got));
            REQUIRE(std::memcmp(&got, &want, sizeof(got)) == 0);
        }
    }

    // the consumer: the receivers of the traced image are pixels 1 and 3, their points on the rays at the hit distance
    float* d_pos = nullptr; float* d_nor = nullptr; uint32_t* d_pix = nullptr;
    REQUIRE(hipMalloc(reinterpret_cast<void**>(&d_pos), 48) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_nor), 48) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&d_pix), 20) == hipSuccess);
    REQUIRE(voidin::gbuffer_points(gpu, camera, voidin::gbuffer_of(target), d_pos, d_nor, d_pix, d_pix + 4) == 2u);
    float pos[6]; uint32_t pix[2];
    REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(pos, d_pos, 24, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(pix, d_pix, 8, hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(pix[0] == 1u && pix[1] == 3u);
    for (int k = 0; k < 2; ++k) {
        const VdRay& r = rays[pix[k]];
        for (int c = 0; c < 3; ++c) REQUIRE(std::fabs(pos[3 * k + c] - (r.eye[c] + r.dir[c] * hits[pix[k]].dist)) < 1e-4f * hits[pix[k]].dist);
    }
    std::printf("gbuffer_trace_mirror_test OK: two of four pixels hit; the composed calls give the bytes of rays + walk + resolve, and the points lie on the rays\n");
    return 0;
}
