// blas_refit_mirror_test.cpp — MeshPool::update_vertices / Bvh::refit of the C++ mirror (include/voidin.hpp):
// a mesh of the pool deforms, its BLAS is refitted in place and its MeshInfo bounds follow.
//   * scaled by 2 (exact in f32, so every SAH comparison falls the same way): the topology of a fresh `add` of the
//     deformed mesh coincides, and the refitted boxes must equal the fresh build's bit for bit;
//   * bent (the fresh build may split differently): every refitted box must be the exact bounds of its subtree, and
//     where the fresh topology does coincide the boxes are compared as well;
//   * the refit identity: refitting a fresh build with its own vertices changes no byte.
// Build: hipcc --offload-arch=gfx950 -I include tests/cpp/blas_refit_mirror_test.cpp -L... -lvoidin_hip
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/voidin.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint64_t rng_state = 0x5EED0077ull;
static float frand() {   // splitmix64 -> [0,1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}

using Nodes = std::vector<voidin::BvhNode>;

static bool same_topology(const voidin::BvhNode* a, const voidin::BvhNode* b, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (a[k].left_first != b[k].left_first || a[k].count != b[k].count) return false;
    return true;
}

// every box the exact bounds of its subtree, from (+1e30, -1e30) (blas.rs:184-204); no NaN or zero in these meshes
static bool boxes_are_exact(const voidin::BvhNode* nodes, size_t n, const voidin::Vec3* v, const uint32_t* idx) {
    std::vector<float> mn(3 * n, 1e30f), mx(3 * n, -1e30f);
    std::vector<char> live(n, 0);
    live[0] = 1;
    for (size_t k = 0; k < n; ++k)
        if (live[k] && nodes[k].count == 0) live[nodes[k].left_first] = live[nodes[k].left_first + 1] = 1;
    for (size_t k = n; k-- > 0;) {
        if (!live[k]) continue;
        if (nodes[k].count) {
            for (uint32_t t = nodes[k].left_first; t < nodes[k].left_first + nodes[k].count; ++t)
                for (int c = 0; c < 3; ++c) {
                    const float p[3] = {v[idx[3 * t + c]].x, v[idx[3 * t + c]].y, v[idx[3 * t + c]].z};
                    for (int q = 0; q < 3; ++q) { mn[3 * k + q] = std::fmin(mn[3 * k + q], p[q]); mx[3 * k + q] = std::fmax(mx[3 * k + q], p[q]); }
                }
        } else {
            const size_t l = nodes[k].left_first;
            for (int q = 0; q < 3; ++q) { mn[3 * k + q] = std::fmin(mn[3 * l + q], mn[3 * l + 3 + q]); mx[3 * k + q] = std::fmax(mx[3 * l + q], mx[3 * l + 3 + q]); }
        }
        if (std::memcmp(nodes[k].min, &mn[3 * k], 12) || std::memcmp(nodes[k].max, &mx[3 * k], 12)) return false;
    }
    return true;
}

int main() {
    voidin::Gpu gpu(0);
    std::vector<voidin::Vec3> plane_v = {{-.5f, 0, -.5f}, {-.5f, 0, .5f}, {.5f, 0, .5f}, {.5f, 0, -.5f}};
    std::vector<uint32_t> plane_i = {0, 1, 2, 0, 2, 3};
    std::vector<voidin::Vec3> soup_v; std::vector<uint32_t> soup_i;
    for (int t = 0; t < 900; ++t) {
        voidin::Vec3 b{frand() * 9 - 5.5f, frand() * 9 - 5.5f, frand() * 9 + 0.5f};
        soup_v.push_back(b);
        soup_v.push_back({b.x + frand() + 0.01f, b.y + frand() + 0.01f, b.z + frand()});
        soup_v.push_back({b.x + frand() + 0.01f, b.y + frand() + 0.01f, b.z + frand()});
        for (int c = 0; c < 3; ++c) soup_i.push_back((uint32_t)(3 * t + c));
    }
    soup_v.push_back({40.f, -50.f, 60.f});           // a vertex no triangle refers to: MeshInfo bounds see it, the root box does not

    for (int bent = 0; bent < 2; ++bent) {
        voidin::MeshPool pool(gpu);
        std::vector<uint32_t> pi = plane_i, si = soup_i, pi2 = plane_i;
        REQUIRE(pool.add({plane_v.data(), plane_v.size(), pi.data(), pi.size()}) == 0);
        REQUIRE(pool.add({soup_v.data(), soup_v.size(), si.data(), si.size()}) == 1);
        REQUIRE(pool.add({plane_v.data(), plane_v.size(), pi2.data(), pi2.size()}) == 2);
        const Nodes before = pool.bvh_nodes;
        const std::vector<voidin::MeshInfo> info_before = pool.mesh_info_cpu;
        const std::vector<uint32_t> indices_before = pool.indices;

        std::vector<voidin::Vec3> moved = soup_v;
        for (auto& p : moved) {
            if (bent) p = {p.x + 0.8f * std::sin(0.9f * p.y), p.y * 1.3f + 0.4f * std::cos(0.7f * p.z), p.z + 0.5f * std::sin(1.1f * p.x)};
            else p = {p.x * 2.f, p.y * 2.f, p.z * 2.f};
        }
        pool.update_vertices(1, moved.data(), moved.size());

        const voidin::MeshInfo& info = pool.mesh_info_cpu[1];
        const size_t b0 = info.bvh_index, b1 = pool.mesh_info_cpu[2].bvh_index, n = b1 - b0;
        REQUIRE(pool.bvh_nodes.size() == before.size() && pool.indices == indices_before);
        REQUIRE(same_topology(pool.bvh_nodes.data(), before.data(), before.size()));
        REQUIRE(std::memcmp(pool.bvh_nodes.data(), before.data(), b0 * sizeof(voidin::BvhNode)) == 0);                  // the plane in front
        REQUIRE(std::memcmp(pool.bvh_nodes.data() + b1, before.data() + b1, (before.size() - b1) * sizeof(voidin::BvhNode)) == 0);   // and behind
        REQUIRE(std::memcmp(pool.bvh_nodes.data() + b0, before.data() + b0, n * sizeof(voidin::BvhNode)) != 0);
        REQUIRE(std::memcmp(&pool.bvh_nodes[b0 + 1], &before[b0 + 1], sizeof(voidin::BvhNode)) == 0);                   // the reserved slot
        REQUIRE(std::memcmp(&pool.vertices[info.vertex_offset], moved.data(), moved.size() * sizeof(voidin::Vec3)) == 0);
        REQUIRE(boxes_are_exact(pool.bvh_nodes.data() + b0, n, moved.data(), pool.indices.data() + info.base_index));

        // a fresh add of the deformed mesh
        voidin::MeshPool fresh(gpu);
        std::vector<uint32_t> fi = soup_i;
        REQUIRE(fresh.add({moved.data(), moved.size(), fi.data(), fi.size()}) == 0);
        REQUIRE(std::memcmp(info.min, fresh.mesh_info_cpu[0].min, 12) == 0 && std::memcmp(info.max, fresh.mesh_info_cpu[0].max, 12) == 0);
        REQUIRE(info.max[0] == moved.back().x && info.min[1] == moved.back().y && info.max[0] > pool.bvh_nodes[b0].max[0]);   // the unreferenced vertex counts
        REQUIRE(info.index_count == info_before[1].index_count && info.base_index == info_before[1].base_index &&
                info.vertex_offset == info_before[1].vertex_offset && info.bvh_index == info_before[1].bvh_index);
        const bool coincides = fresh.bvh_nodes.size() == n && same_topology(fresh.bvh_nodes.data(), pool.bvh_nodes.data() + b0, n) &&
                               std::memcmp(fresh.indices.data(), pool.indices.data() + info.base_index, fi.size() * 4) == 0;
        if (!bent) REQUIRE(coincides);               // a scale by 2 is exact: the builder decides as before
        if (coincides) REQUIRE(std::memcmp(fresh.bvh_nodes.data(), pool.bvh_nodes.data() + b0, n * sizeof(voidin::BvhNode)) == 0);
        // the refit identity on the fresh build, through MeshPool and through Bvh::refit
        const Nodes fresh_nodes = fresh.bvh_nodes;
        fresh.update_vertices(0, moved.data(), moved.size());
        REQUIRE(std::memcmp(fresh.bvh_nodes.data(), fresh_nodes.data(), fresh_nodes.size() * sizeof(voidin::BvhNode)) == 0);
        voidin::Bvh bvh{fresh_nodes};
        for (auto& nd : bvh.nodes) { nd.min[0] -= 1.f; nd.max[2] += 1.f; }
        bvh.nodes[1] = fresh_nodes[1];
        bvh.refit(gpu, moved.data(), moved.size(), reinterpret_cast<const voidin::UVec3*>(fresh.indices.data()), fresh.indices.size() / 3);
        REQUIRE(std::memcmp(bvh.nodes.data(), fresh_nodes.data(), fresh_nodes.size() * sizeof(voidin::BvhNode)) == 0);
        std::printf("%s: %zu nodes refitted, fresh topology %s\n", bent ? "bent" : "scaled", n, coincides ? "coincides" : "differs");

        bool threw = false;
        try { pool.update_vertices(1, moved.data(), moved.size() - 1); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
        REQUIRE(threw);
        threw = false;
        try { pool.update_vertices(7, moved.data(), moved.size()); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
        REQUIRE(threw);
    }
    std::printf("blas_refit_mirror_test OK\n");
    return 0;
}
