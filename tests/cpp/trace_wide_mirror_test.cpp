// The wide top level of the C++ mirror (include/voidin.hpp): Tlas::build_fast, TlasWide::build / build_fast and the
// traverse_tlas overload for VdTraceSceneWide.  A grid of DISJOINT instances: no two can tie in distance, so a ray's record
// does not depend on the top level's shape - the exact narrow tree, the narrow LBVH, the exact wide tree and the wide LBVH
// must all give the same bytes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/voidin.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    voidin::Gpu gpu(0);
    // an octahedron of radius 0.4
    std::vector<voidin::Vec3> v = {{.4f, 0, 0}, {-.4f, 0, 0}, {0, .4f, 0}, {0, -.4f, 0}, {0, 0, .4f}, {0, 0, -.4f}};
    std::vector<uint32_t> idx = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    voidin::MeshPool pool(gpu);
    REQUIRE(pool.add({v.data(), v.size(), idx.data(), idx.size()}) == 0);

    const int side = 9;                                  // 81 instances, 1.5 apart
    std::vector<voidin::Instance> inst(side * side);
    for (int k = 0; k < side * side; ++k) {
        voidin::Instance& I = inst[k];
        std::memset(&I, 0, sizeof(I));
        for (int d = 0; d < 4; ++d) I.transform[5 * d] = I.inv_transform[5 * d] = 1.0f;
        const float x = 1.5f * (float)(k % side), y = 1.5f * (float)(k / side);
        I.transform[12] = x; I.transform[13] = y; I.inv_transform[12] = -x; I.inv_transform[13] = -y;
    }
    std::vector<VdRay> rays;
    for (int k = 0; k < side * side; ++k)
        for (int j = 0; j < 4; ++j) {                    // three rays into every instance, one between two of them
            VdRay r{};
            r.eye[0] = 1.5f * (float)(k % side) + (j == 3 ? 0.75f : 0.017f + 0.05f * (float)j); r.eye[1] = 1.5f * (float)(k / side) + (j == 3 ? 0.75f : 0.031f);
            r.eye[2] = 10.0f;
            r.dir[0] = 0.003f; r.dir[1] = 0.002f; r.dir[2] = -1.0f;      // no zero component: 1 / dir stays finite in the slab test (intersections.wgsl:13-23)
            rays.push_back(r);
        }

    pool.generate_tlas(inst);                            // the exact narrow tree
    const std::vector<VdHit> want = voidin::traverse_tlas(gpu, pool.trace_scene(inst), rays);
    size_t hits = 0;
    for (const VdHit& h : want) hits += h.hit;
    REQUIRE(hits == 3u * side * side);

    pool.tlas.build_fast(gpu, inst.data(), inst.size(), pool.mesh_info_cpu.data(), pool.mesh_info_cpu.size());
    REQUIRE(pool.tlas.nodes.size() == 2 * inst.size() + 1);
    const std::vector<VdHit> fast = voidin::traverse_tlas(gpu, pool.trace_scene(inst), rays);
    REQUIRE(std::memcmp(fast.data(), want.data(), want.size() * sizeof(VdHit)) == 0);

    const VdTraceScene ns = pool.trace_scene(inst);
    for (int lbvh = 0; lbvh < 2; ++lbvh) {
        voidin::TlasWide wide = voidin::TlasWide::empty();
        if (lbvh) wide.build_fast(gpu, inst.data(), inst.size(), pool.mesh_info_cpu.data(), pool.mesh_info_cpu.size());
        else wide.build(gpu, inst.data(), inst.size(), pool.mesh_info_cpu.data(), pool.mesh_info_cpu.size());
        VdTraceSceneWide ws{};
        ws.tlas_nodes = wide.nodes.data(); ws.n_tlas_nodes = (uint32_t)wide.nodes.size();
        ws.instances = ns.instances; ws.n_instances = ns.n_instances; ws.meshes = ns.meshes; ws.n_meshes = ns.n_meshes;
        ws.bvh_nodes = ns.bvh_nodes; ws.n_bvh_nodes = ns.n_bvh_nodes; ws.vertices = ns.vertices; ws.n_vertices = ns.n_vertices;
        ws.indices = ns.indices; ws.n_indices = ns.n_indices;
        const std::vector<VdHit> got = voidin::traverse_tlas(gpu, ws, rays);
        REQUIRE(std::memcmp(got.data(), want.data(), want.size() * sizeof(VdHit)) == 0);
    }
    std::printf("trace_wide_mirror_test OK: %zu rays, %zu hits, four top levels, the same records\n", rays.size(), hits);
    return 0;
}
