// The prepared wide scene of the C++ mirror (include/voidin.hpp): TraceScene over a VdTraceSceneWide, refit() and info_wide(),
// with VD_OPT_TRACE_TIGHT_TLAS on.  64 DISJOINT instances: no two can tie in distance, so a ray's record does not depend on the
// top level's shape - the private tight LBVH, before and after the instances moved, must give the bytes of
// traverse_tlas(gpu, VdTraceSceneWide, rays) over TlasWide::build_fast of the same instances.
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

static void place(std::vector<voidin::Instance>& inst, int side, float dx) {
    for (int k = 0; k < side * side; ++k) {
        voidin::Instance& I = inst[k];
        std::memset(&I, 0, sizeof(I));
        for (int d = 0; d < 4; ++d) I.transform[5 * d] = I.inv_transform[5 * d] = 1.0f;
        const float x = 1.5f * (float)(k % side) + dx, y = 1.5f * (float)(k / side);
        I.transform[12] = x; I.transform[13] = y; I.inv_transform[12] = -x; I.inv_transform[13] = -y;
    }
}

int main() {
    voidin::Gpu gpu(0);
    // an octahedron of radius 0.4
    std::vector<voidin::Vec3> v = {{.4f, 0, 0}, {-.4f, 0, 0}, {0, .4f, 0}, {0, -.4f, 0}, {0, 0, .4f}, {0, 0, -.4f}};
    std::vector<uint32_t> idx = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    voidin::MeshPool pool(gpu);
    REQUIRE(pool.add({v.data(), v.size(), idx.data(), idx.size()}) == 0);

    const int side = 8;                                  // 64 instances, 1.5 apart
    std::vector<voidin::Instance> inst(side * side);
    place(inst, side, 0.0f);
    std::vector<VdRay> rays;
    for (int k = 0; k < side * side; ++k)
        for (int j = 0; j < 4; ++j) {                    // rays into every instance where it is and where it will be, one between two
            VdRay r{};
            r.eye[0] = 1.5f * (float)(k % side) + (j == 3 ? 0.75f : 0.017f + 0.16f * (float)j); r.eye[1] = 1.5f * (float)(k / side) + (j == 3 ? 0.75f : 0.031f);
            r.eye[2] = 10.0f;
            r.dir[0] = 0.003f; r.dir[1] = 0.002f; r.dir[2] = -1.0f;      // no zero component: 1 / dir stays finite in the slab test
            rays.push_back(r);
        }

    const VdTraceScene ns = pool.trace_scene(inst);
    auto wide_scene = [&](const voidin::TlasWide& wide, const voidin::Instance* instances) {
        VdTraceSceneWide ws{};
        ws.tlas_nodes = wide.nodes.data(); ws.n_tlas_nodes = (uint32_t)wide.nodes.size();
        ws.instances = instances; ws.n_instances = ns.n_instances; ws.meshes = ns.meshes; ws.n_meshes = ns.n_meshes;
        ws.bvh_nodes = ns.bvh_nodes; ws.n_bvh_nodes = ns.n_bvh_nodes; ws.vertices = ns.vertices; ws.n_vertices = ns.n_vertices;
        ws.indices = ns.indices; ws.n_indices = ns.n_indices;
        return ws;
    };
    voidin::TlasWide wide = voidin::TlasWide::empty();
    wide.build_fast(gpu, inst.data(), inst.size(), pool.mesh_info_cpu.data(), pool.mesh_info_cpu.size());
    const VdTraceSceneWide host_scene = wide_scene(wide, ns.instances);
    const std::vector<VdHit> want = voidin::traverse_tlas(gpu, host_scene, rays);
    size_t hits = 0;
    for (const VdHit& h : want) hits += h.hit;
    REQUIRE(hits > 0 && hits < rays.size());

    // the same scene on the device
    VdTraceSceneWide ds = host_scene;
    voidin::Instance* d_inst = to_device(ns.instances, ns.n_instances);
    ds.tlas_nodes = to_device(host_scene.tlas_nodes, host_scene.n_tlas_nodes); ds.instances = d_inst;
    ds.meshes = to_device(ns.meshes, ns.n_meshes); ds.bvh_nodes = to_device(ns.bvh_nodes, ns.n_bvh_nodes);
    ds.vertices = to_device(ns.vertices, 3 * (size_t)ns.n_vertices); ds.indices = to_device(ns.indices, ns.n_indices);
    VdRay* d_rays = to_device(rays.data(), rays.size());
    VdHit* d_hits = nullptr;
    REQUIRE(ds.tlas_nodes && ds.instances && ds.meshes && ds.bvh_nodes && ds.vertices && ds.indices && d_rays);
    REQUIRE(hipMalloc(reinterpret_cast<void**>(&d_hits), rays.size() * sizeof(VdHit)) == hipSuccess);
    std::vector<VdHit> got(rays.size());
    auto fetch = [&]() { return hipMemcpy(got.data(), d_hits, got.size() * sizeof(VdHit), hipMemcpyDeviceToHost) == hipSuccess; };
    {
        gpu.set_option(VD_OPT_TRACE_TIGHT_TLAS, 1);
        voidin::TraceScene scene(gpu, ds);
        gpu.set_option(VD_OPT_TRACE_TIGHT_TLAS, -1);
        REQUIRE(scene.wide());
        VdTraceAccelInfoWide info = scene.info_wide();
        REQUIRE(info.tight_tlas == 2 && info.n_tlas_nodes == 2 * inst.size() && info.tight_fallback_instances == 0 && info.refits_since_build == 0);
        REQUIRE(info.d_tlas_nodes != ds.tlas_nodes && info.triangle_bytes == 36ull * (idx.size() / 3));
        const VdTlasNodeWide* tree = info.d_tlas_nodes;
        scene.trace(d_rays, (uint32_t)rays.size(), d_hits);
        REQUIRE(fetch() && std::memcmp(got.data(), want.data(), want.size() * sizeof(VdHit)) == 0);
        bool threw = false;
        try { (void)scene.info(); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG && std::strstr(e.what(), "info_wide") != nullptr; }
        REQUIRE(threw);

        // the instances move by a third of their spacing: refit, same tree, the records of a fresh top level over the moved scene
        std::vector<voidin::Instance> moved(inst.size());
        place(moved, side, 0.5f);
        REQUIRE(hipMemcpy(d_inst, moved.data(), moved.size() * sizeof(voidin::Instance), hipMemcpyHostToDevice) == hipSuccess);
        scene.refit();
        info = scene.info_wide();
        REQUIRE(info.tight_tlas == 2 && info.refits_since_build == 1 && info.d_tlas_nodes == tree);
        voidin::TlasWide wide2 = voidin::TlasWide::empty();
        wide2.build_fast(gpu, moved.data(), moved.size(), pool.mesh_info_cpu.data(), pool.mesh_info_cpu.size());
        const std::vector<VdHit> want2 = voidin::traverse_tlas(gpu, wide_scene(wide2, moved.data()), rays);
        REQUIRE(std::memcmp(want2.data(), want.data(), want.size() * sizeof(VdHit)) != 0);
        scene.trace(d_rays, (uint32_t)rays.size(), d_hits);
        REQUIRE(fetch() && std::memcmp(got.data(), want2.data(), want2.size() * sizeof(VdHit)) == 0);
        scene.update();
        REQUIRE(scene.info_wide().refits_since_build == 0 && scene.info_wide().tight_tlas == 2);
        scene.trace(d_rays, (uint32_t)rays.size(), d_hits);
        REQUIRE(fetch() && std::memcmp(got.data(), want2.data(), want2.size() * sizeof(VdHit)) == 0);
    }
    std::printf("trace_wide_prepared_mirror_test OK: %zu rays, %zu hits, prepared, refitted, rebuilt: the records of the plain wide walk\n", rays.size(), hits);
    return 0;
}
