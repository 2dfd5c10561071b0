// The shadow pass straight from the G-buffer through the C++ mirror (include/voidin.hpp): gbuffer_points, shadow_gbuffer and
// TraceScene::shadow_gbuffer against the composition they replace - gbuffer_points, shadow_pass over the points, the bits put back
// at the points' pixels.  The scene and lights of shadow_pass_mirror_test.cpp, under a 4 x 1 G-buffer whose materials are
// 1, 0, LIGHT_MATERIAL, 7: pixels 0 and 3 receive.  clip_to_world is affine here (w = 1), so a pixel's point is
// (13.3 * ndc.x + 10.025, 0, depth): point 0 next to the origin, point 1 = (20, 0, 0) up to rounding.
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

int main() {
    static_assert(sizeof(VdGBuffer) == 56 && sizeof(VdShadowGBufferInfo) == 16, "the G-buffer records");
    voidin::Gpu gpu(0);
    std::vector<voidin::Vec3> v = {{.4f, 0, 0}, {-.4f, 0, 0}, {0, .4f, 0}, {0, -.4f, 0}, {0, 0, .4f}, {0, 0, -.4f}};
    std::vector<uint32_t> idx = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    voidin::MeshPool pool(gpu);
    REQUIRE(pool.add({v.data(), v.size(), idx.data(), idx.size()}) == 0);
    const float centre[2][3] = {{0.0f, 8.0f, 0.0f}, {10.0f, 2.5f, 0.0f}};
    std::vector<voidin::Instance> inst(2);
    for (int k = 0; k < 2; ++k) {
        std::memset(&inst[k], 0, sizeof(inst[k]));
        for (int d = 0; d < 4; ++d) inst[k].transform[5 * d] = inst[k].inv_transform[5 * d] = 1.0f;
        for (int c = 0; c < 3; ++c) { inst[k].transform[12 + c] = centre[k][c]; inst[k].inv_transform[12 + c] = -centre[k][c]; }
    }
    pool.generate_tlas(inst);
    const VdTraceScene scene = pool.trace_scene(inst);
    VdTraceScene ds = scene;
    ds.tlas_nodes = to_device(scene.tlas_nodes, scene.n_tlas_nodes); ds.instances = to_device(scene.instances, scene.n_instances);
    ds.meshes = to_device(scene.meshes, scene.n_meshes); ds.bvh_nodes = to_device(scene.bvh_nodes, scene.n_bvh_nodes);
    ds.vertices = to_device(scene.vertices, 3 * (size_t)scene.n_vertices); ds.indices = to_device(scene.indices, scene.n_indices);
    REQUIRE(ds.tlas_nodes && ds.instances && ds.meshes && ds.bvh_nodes && ds.vertices && ds.indices);

    const float at[3] = {0.0f, 5.0f, 0.0f};
    const float radius[3] = {100.0f, 1.0f, 6.0f};
    const uint32_t reach[2] = {0x5u, 0x1u};                  // lights 0 and 2 reach point 0, light 0 alone reaches point 1
    VdLight lights[3];
    std::memset(lights, 0, sizeof(lights));
    for (int l = 0; l < 3; ++l) { std::memcpy(lights[l].position, at, sizeof(at)); lights[l].radius = radius[l]; }
    const VdLight* d_lights = to_device(lights, 3);

    // the three images, rows padded as a copy_texture_to_buffer pads them
    VdCameraUniform camera;
    std::memset(&camera, 0, sizeof(camera));
    camera.clip_to_world[0] = 13.3f; camera.clip_to_world[5] = 1.0f; camera.clip_to_world[10] = 1.0f;
    camera.clip_to_world[12] = 10.025f; camera.clip_to_world[15] = 1.0f;
    std::vector<unsigned char> depth_row(256, 0xC3), normal_row(256, 0xC3), material_row(256, 0xC3);
    const float depth[4] = {0.03f, 0.5f, 0.5f, 0.0f};
    const uint32_t normal_uv[8] = {0xffff8000u, 1u, 0u, 2u, 0u, 3u, 0xffff8000u, 4u};       // (0, 1, 0) up to one code step
    const unsigned char material[4] = {1, VD_GBUFFER_NO_MATERIAL, VD_GBUFFER_LIGHT_MATERIAL, 7};
    std::memcpy(depth_row.data(), depth, sizeof(depth)); std::memcpy(normal_row.data(), normal_uv, sizeof(normal_uv));
    std::memcpy(material_row.data(), material, sizeof(material));
    VdGBuffer gb;
    std::memset(&gb, 0, sizeof(gb));
    gb.depth = reinterpret_cast<const float*>(to_device(depth_row.data(), 256)); gb.depth_pitch = 256;
    gb.normal_uv = reinterpret_cast<const uint32_t*>(to_device(normal_row.data(), 256)); gb.normal_uv_pitch = 256;
    gb.material = to_device(material_row.data(), 256); gb.material_pitch = 256;
    gb.width = 4; gb.height = 1;
    REQUIRE(d_lights && gb.depth && gb.normal_uv && gb.material);

    float* d_pos = nullptr; float* d_nor = nullptr; uint32_t* d_pix = nullptr; uint32_t* d_out = nullptr;
    REQUIRE(hipMalloc(reinterpret_cast<void**>(&d_pos), 48) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_nor), 48) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&d_pix), 20) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_out), 64) == hipSuccess);
    REQUIRE(hipMemset(d_pix, 0xEE, 20) == hipSuccess);
    REQUIRE(voidin::gbuffer_points(gpu, camera, gb, d_pos, d_nor, d_pix, d_pix + 4) == 2u);
    float pos[6], nor[6]; uint32_t pix[5];
    REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(pos, d_pos, 24, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(nor, d_nor, 24, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(pix, d_pix, 20, hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(pix[0] == 0u && pix[1] == 3u && pix[2] == 0xEEEEEEEEu && pix[3] == 0xEEEEEEEEu && pix[4] == 2u);      // nothing beyond the count
    REQUIRE(std::fabs(pos[0] - 0.05f) < 1e-5f && pos[1] == 0.0f && pos[2] == 0.03f && std::fabs(pos[3] - 20.0f) < 1e-5f && pos[4] == 0.0f && pos[5] == 0.0f);
    REQUIRE(nor[0] == 0.0f && std::fabs(nor[1] - 1.0f) < 1e-6f && std::fabs(nor[2]) < 2e-5f && nor[3] == 0.0f && std::fabs(nor[4] - 1.0f) < 1e-6f);

    voidin::TraceScene prepared(gpu, ds);
    for (int on = 0; on < 2; ++on) {
        gpu.set_option(VD_OPT_TRACE_RAY_RANGE, on ? 1 : -1);
        // the composition: the pass over the two points; d_out = occluded [2], in range [2]
        uint32_t want[4];
        const VdShadowPassInfo pass = voidin::shadow_pass(gpu, ds, d_pos, d_nor, 2, d_lights, 3, d_out, d_out + 2);
        REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(want, d_out, 16, hipMemcpyDeviceToHost) == hipSuccess);
        REQUIRE(pass.n_rays == 3 && want[2] == reach[0] && want[3] == reach[1]);
        REQUIRE(want[0] == (on ? 0x0u : 0x5u) && want[1] == 0x1u);      // the octahedron behind the light shadows point 0 by default only
        for (int form = 0; form < 2; ++form) {
            uint32_t got[8];                                           // occluded [4 pixels], in range [4 pixels]
            REQUIRE(hipMemset(d_out, 0xEE, 64) == hipSuccess);
            const VdShadowGBufferInfo info = form ? prepared.shadow_gbuffer(camera, gb, d_lights, 3, d_out + 8, d_out + 12)
                                                  : voidin::shadow_gbuffer(gpu, ds, camera, gb, d_lights, 3, d_out + 8, d_out + 12);
            REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(got, d_out + 8, 32, hipMemcpyDeviceToHost) == hipSuccess);
            REQUIRE(info.n_points == 2 && info.n_rays == 3 && info.n_chunks == 1 && info.words_per_point == 1);
            REQUIRE(got[0] == want[0] && got[1] == 0u && got[2] == 0u && got[3] == want[1]);
            REQUIRE(got[4] == want[2] && got[5] == 0u && got[6] == 0u && got[7] == want[3]);
        }
    }
    gpu.set_option(VD_OPT_TRACE_RAY_RANGE, -1);
    std::printf("shadow_gbuffer_mirror_test OK: two of four pixels receive; the call gives the pass's bits at their pixels and zero elsewhere\n");
    return 0;
}
