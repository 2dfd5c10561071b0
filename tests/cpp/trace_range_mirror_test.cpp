// Ray intervals through the C++ mirror (include/voidin.hpp): ray_segment and shadow_occlusion under VD_OPT_TRACE_RAY_RANGE.
// Two octahedra of radius 0.4 and a light at L = (0, 5, 0).  Point 0 lies next to the origin: nothing between it and the light,
// octahedron 0 (centre (0, 8, 0)) on the same line BEHIND the light.  Point 1 = (20, 0, 0): octahedron 1 sits halfway between it
// and the light.  By default - the reference's shadow ray has no end - both points are shadowed; under the option only point 1.
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

static bool same(const VdHit& a, const VdHit& b) { return std::memcmp(&a, &b, sizeof(VdHit)) == 0; }

int main() {
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

    const float light[3] = {0.0f, 5.0f, 0.0f};
    const float pos[6] = {0.05f, 0.0f, 0.03f, 20.0f, 0.0f, 0.0f}, nor[6] = {0, 1, 0, 0, 1, 0};
    const float dir0[3] = {light[0] - pos[0], light[1] - pos[1], light[2] - pos[2]};

    // ---- ray_segment, host form.  Without the option the fields are ignored: the ray has no end.
    const VdRay plain = voidin::ray_segment(pos, dir0);
    REQUIRE(plain._pad0 == 0.0f && plain._pad1 == VD_MAX_DIST && plain.eye[0] == pos[0] && plain.dir[1] == dir0[1]);
    std::vector<VdRay> rays = {plain, voidin::ray_segment(pos, dir0, 0.0f, 1.0f)};
    std::vector<VdHit> off = voidin::traverse_tlas(gpu, scene, rays);
    REQUIRE(off[0].hit == 1 && off[0].instance == 0 && off[0].dist > 1.4f && off[0].dist < 1.6f && same(off[0], off[1]));
    const float d = off[0].dist;

    gpu.set_option(VD_OPT_TRACE_RAY_RANGE, 1);
    rays = {plain,                                           // the whole half-line: the bytes of the default
            voidin::ray_segment(pos, dir0, 0.0f, 1.0f),      // ends at the light
            voidin::ray_segment(pos, dir0, 0.0f, 2.0f),      // ends behind the octahedron
            voidin::ray_segment(pos, dir0, 0.0f, d),         // both ends are exclusive
            voidin::ray_segment(pos, dir0, d, 100.0f),       // ... and the far side of the octahedron faces away
            voidin::ray_segment(pos, dir0, 1.0f, 2.0f)};     // from the light on
    std::vector<VdHit> on = voidin::traverse_tlas(gpu, scene, rays);
    REQUIRE(same(on[0], off[0]) && same(on[2], off[0]) && same(on[5], off[0]));
    for (int k : {1, 3, 4}) REQUIRE(on[k].hit == 0 && on[k].dist == VD_MAX_DIST);
    gpu.set_option(VD_OPT_TRACE_RAY_RANGE, -1);

    // ---- shadow_occlusion over the scene on the device
    VdTraceScene ds = scene;
    ds.tlas_nodes = to_device(scene.tlas_nodes, scene.n_tlas_nodes); ds.instances = to_device(scene.instances, scene.n_instances);
    ds.meshes = to_device(scene.meshes, scene.n_meshes); ds.bvh_nodes = to_device(scene.bvh_nodes, scene.n_bvh_nodes);
    ds.vertices = to_device(scene.vertices, 3 * (size_t)scene.n_vertices); ds.indices = to_device(scene.indices, scene.n_indices);
    const float* d_pos = to_device(pos, 6);
    const float* d_nor = to_device(nor, 6);
    VdRay* d_rays = nullptr;
    uint32_t* d_occ = nullptr;
    REQUIRE(ds.tlas_nodes && ds.instances && ds.meshes && ds.bvh_nodes && ds.vertices && ds.indices && d_pos && d_nor);
    REQUIRE(hipMalloc(reinterpret_cast<void**>(&d_rays), 2 * sizeof(VdRay)) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_occ), 8) == hipSuccess);
    uint32_t occ[2];
    VdRay made[2];
    auto run = [&]() {
        voidin::shadow_occlusion(gpu, ds, d_pos, d_nor, 2, light, d_rays, d_occ);
        return hipDeviceSynchronize() == hipSuccess && hipMemcpy(occ, d_occ, 8, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(made, d_rays, sizeof(made), hipMemcpyDeviceToHost) == hipSuccess;
    };
    REQUIRE(run() && occ[0] == 1 && occ[1] == 1 && made[0]._pad0 == 0.0f && made[0]._pad1 == 0.0f);      // the reference's behaviour
    gpu.set_option(VD_OPT_TRACE_RAY_RANGE, 1);
    REQUIRE(run() && occ[0] == 0 && occ[1] == 1 && made[0]._pad0 == 0.0f && made[0]._pad1 == 1.0f && made[1]._pad1 == 1.0f);
    gpu.set_option(VD_OPT_TRACE_RAY_RANGE, -1);
    REQUIRE(run() && occ[0] == 1 && occ[1] == 1);
    std::printf("trace_range_mirror_test OK: the octahedron behind the light at t = %.3f shadows the point by default, not on the segment\n", d);
    return 0;
}
