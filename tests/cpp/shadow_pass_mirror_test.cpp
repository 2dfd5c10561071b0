// The shadow pass through the C++ mirror (include/voidin.hpp): shadow_pass and TraceScene::shadow_pass against the loop of
// shadow_occlusion calls it replaces.  The scene of trace_range_mirror_test.cpp - two octahedra of radius 0.4, point 0 next to the
// origin with octahedron 0 BEHIND the light position (0, 5, 0), point 1 = (20, 0, 0) with octahedron 1 halfway to it - and three
// lights at that position: radius 100 (both points in range), radius 1 (neither), radius 6 (point 0 only: it is 5 away, point 1 20.6).
#include <hip/hip_runtime.h>

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
    static_assert(sizeof(VdLight) == 32, "the reference's Light record");
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
    const float pos[6] = {0.05f, 0.0f, 0.03f, 20.0f, 0.0f, 0.0f}, nor[6] = {0, 1, 0, 0, 1, 0};
    const float radius[3] = {100.0f, 1.0f, 6.0f};
    const uint32_t reach[2] = {0x5u, 0x1u};                  // lights 0 and 2 reach point 0, light 0 alone reaches point 1
    VdLight lights[3];
    std::memset(lights, 0, sizeof(lights));
    for (int l = 0; l < 3; ++l) { std::memcpy(lights[l].position, at, sizeof(at)); lights[l].radius = radius[l]; }
    const float* d_pos = to_device(pos, 6);
    const float* d_nor = to_device(nor, 6);
    const VdLight* d_lights = to_device(lights, 3);
    VdRay* d_rays = nullptr;
    uint32_t* d_out = nullptr;                               // occluded [2], in range [2], one light's flags [2]
    REQUIRE(d_pos && d_nor && d_lights && hipMalloc(reinterpret_cast<void**>(&d_rays), 2 * sizeof(VdRay)) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&d_out), 24) == hipSuccess);

    voidin::TraceScene prepared(gpu, ds);
    for (int on = 0; on < 2; ++on) {
        gpu.set_option(VD_OPT_TRACE_RAY_RANGE, on ? 1 : -1);
        // the loop the pass replaces: one shadow_occlusion per light, masked by the reach
        uint32_t want[2] = {0u, 0u}, flags[2];
        for (int l = 0; l < 3; ++l) {
            voidin::shadow_occlusion(gpu, ds, d_pos, d_nor, 2, lights[l].position, d_rays, d_out + 4);
            REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(flags, d_out + 4, 8, hipMemcpyDeviceToHost) == hipSuccess);
            for (int p = 0; p < 2; ++p) want[p] |= (flags[p] && ((reach[p] >> l) & 1u)) ? 1u << l : 0u;
        }
        REQUIRE(want[0] == (on ? 0x0u : 0x5u) && want[1] == 0x1u);      // the octahedron behind the light shadows point 0 by default only
        for (int form = 0; form < 2; ++form) {
            uint32_t got[4];
            REQUIRE(hipMemset(d_out, 0xEE, 16) == hipSuccess);
            const VdShadowPassInfo info = form ? prepared.shadow_pass(d_pos, d_nor, 2, d_lights, 3, d_out, d_out + 2)
                                               : voidin::shadow_pass(gpu, ds, d_pos, d_nor, 2, d_lights, 3, d_out, d_out + 2);
            REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(got, d_out, 16, hipMemcpyDeviceToHost) == hipSuccess);
            REQUIRE(info.n_rays == 3 && info.n_chunks == 1 && info.words_per_point == 1);
            REQUIRE(got[2] == reach[0] && got[3] == reach[1] && got[0] == want[0] && got[1] == want[1]);
        }
    }
    gpu.set_option(VD_OPT_TRACE_RAY_RANGE, -1);
    std::printf("shadow_pass_mirror_test OK: three of six pairs became rays; the pass gives the bits of the per-light loop\n");
    return 0;
}
