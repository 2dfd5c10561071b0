// blas_lbvh_mirror_test.cpp — BvhBuilder::build_fast / MeshPool::add_fast / MeshPool::rebuild_fast of the C++ mirror
// (include/voidin.hpp): a mesh of the pool is re-triangulated, its LBVH bottom level is rebuilt in place.
//   * add_fast keeps max(2, 2 T) node slots for the mesh, zero nodes behind its tree;
//   * after rebuild_fast with other positions and other indices the mesh's nodes, indices and bounds equal those of a fresh
//     build_fast / add_fast of the new mesh, the slots behind the new tree are zero nodes again;
//   * the neighbours' MeshInfo rows, nodes, indices and vertices, and every offset, are untouched.
// Build: hipcc --offload-arch=gfx950 -I include tests/cpp/blas_lbvh_mirror_test.cpp -L... -lvoidin_hip
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/voidin.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint64_t rng_state = 0x5EED0099ull;
static float frand() {   // splitmix64 -> [0,1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}

static bool zero_nodes(const voidin::BvhNode* n, size_t count) {
    const voidin::BvhNode z{};
    for (size_t k = 0; k < count; ++k) if (std::memcmp(&n[k], &z, sizeof z)) return false;
    return true;
}

int main() {
    voidin::Gpu gpu(0);
    std::vector<voidin::Vec3> plane_v = {{-.5f, 0, -.5f}, {-.5f, 0, .5f}, {.5f, 0, .5f}, {.5f, 0, -.5f}};
    std::vector<uint32_t> plane_i = {0, 1, 2, 0, 2, 3};
    // a grid of G x G quads over shared vertices: two triangulations of the same vertex and triangle counts
    const int G = 24;
    std::vector<voidin::Vec3> grid_v;
    for (int y = 0; y <= G; ++y)
        for (int x = 0; x <= G; ++x) grid_v.push_back({(float)x * 0.25f, 0.3f * std::sin(0.7f * x) * std::cos(0.5f * y) + 0.05f * frand(), (float)y * 0.25f});
    auto triangulate = [&](bool other) {
        std::vector<uint32_t> idx;
        for (int y = 0; y < G; ++y)
            for (int x = 0; x < G; ++x) {
                const uint32_t a = (uint32_t)(y * (G + 1) + x), b = a + 1, c = a + (uint32_t)(G + 1), d = c + 1;
                if (other) { const uint32_t t[6] = {a, b, d, a, d, c}; idx.insert(idx.end(), t, t + 6); }      // the other diagonal
                else { const uint32_t t[6] = {a, b, c, b, d, c}; idx.insert(idx.end(), t, t + 6); }
            }
        return idx;
    };
    const std::vector<uint32_t> grid_i = triangulate(false), grid_i2 = triangulate(true);
    const size_t T = grid_i.size() / 3;
    std::vector<voidin::Vec3> moved = grid_v;
    for (auto& p : moved) p = {p.x + 0.1f * std::sin(1.3f * p.z), p.y * 1.5f, p.z + 0.2f};

    voidin::MeshPool pool(gpu);
    std::vector<uint32_t> pi = plane_i, gi = grid_i, pi2 = plane_i;
    REQUIRE(pool.add({plane_v.data(), plane_v.size(), pi.data(), pi.size()}) == 0);
    REQUIRE(pool.add_fast({grid_v.data(), grid_v.size(), gi.data(), gi.size()}) == 1);
    REQUIRE(pool.add({plane_v.data(), plane_v.size(), pi2.data(), pi2.size()}) == 2);
    const voidin::MeshInfo info0 = pool.mesh_info_cpu[1];
    const size_t b0 = info0.bvh_index, b1 = pool.mesh_info_cpu[2].bvh_index;
    REQUIRE(b1 - b0 == 2 * T);                                            // the full 2 T slots

    // add_fast == build_fast, then zero nodes
    std::vector<uint32_t> fi = grid_i;
    voidin::Bvh first = voidin::BvhBuilder(gpu, grid_v.data(), grid_v.size(), reinterpret_cast<voidin::UVec3*>(fi.data()), T).build_fast();
    REQUIRE(first.nodes.size() >= 4 && first.nodes.size() <= 2 * T && first.nodes[0].count == 0 && first.nodes[0].left_first == 2);
    REQUIRE(std::memcmp(pool.bvh_nodes.data() + b0, first.nodes.data(), first.nodes.size() * sizeof(voidin::BvhNode)) == 0);
    REQUIRE(zero_nodes(pool.bvh_nodes.data() + b0 + first.nodes.size(), 2 * T - first.nodes.size()));
    REQUIRE(std::memcmp(pool.indices.data() + info0.base_index, fi.data(), fi.size() * 4) == 0 && fi == gi && fi != grid_i);   // permuted, in the caller's slice too

    const std::vector<voidin::BvhNode> nodes_before = pool.bvh_nodes;
    const std::vector<voidin::MeshInfo> info_before = pool.mesh_info_cpu;
    const std::vector<uint32_t> indices_before = pool.indices;
    const std::vector<voidin::Vec3> vertices_before = pool.vertices;

    pool.rebuild_fast(1, moved.data(), moved.size(), grid_i2.data(), grid_i2.size());

    // a fresh build of the new mesh
    std::vector<uint32_t> ri = grid_i2;
    voidin::Bvh fresh = voidin::BvhBuilder(gpu, moved.data(), moved.size(), reinterpret_cast<voidin::UVec3*>(ri.data()), T).build_fast();
    REQUIRE(pool.bvh_nodes.size() == nodes_before.size() && pool.indices.size() == indices_before.size() && pool.vertices.size() == vertices_before.size());
    REQUIRE(std::memcmp(pool.bvh_nodes.data() + b0, fresh.nodes.data(), fresh.nodes.size() * sizeof(voidin::BvhNode)) == 0);
    REQUIRE(zero_nodes(pool.bvh_nodes.data() + b0 + fresh.nodes.size(), 2 * T - fresh.nodes.size()));
    REQUIRE(std::memcmp(pool.indices.data() + info0.base_index, ri.data(), ri.size() * 4) == 0);
    REQUIRE(std::memcmp(&pool.vertices[(size_t)info0.vertex_offset], moved.data(), moved.size() * sizeof(voidin::Vec3)) == 0);
    REQUIRE(std::memcmp(pool.bvh_nodes.data() + b0, nodes_before.data() + b0, (b1 - b0) * sizeof(voidin::BvhNode)) != 0);
    // ... and through a fresh pool: the MeshInfo bounds
    voidin::MeshPool other(gpu);
    std::vector<uint32_t> oi = grid_i2;
    REQUIRE(other.add_fast({moved.data(), moved.size(), oi.data(), oi.size()}) == 0);
    const voidin::MeshInfo& info = pool.mesh_info_cpu[1];
    REQUIRE(std::memcmp(info.min, other.mesh_info_cpu[0].min, 12) == 0 && std::memcmp(info.max, other.mesh_info_cpu[0].max, 12) == 0);
    REQUIRE(std::memcmp(info.min, info_before[1].min, 12) != 0);
    REQUIRE(info.index_count == info_before[1].index_count && info.base_index == info_before[1].base_index &&
            info.vertex_offset == info_before[1].vertex_offset && info.bvh_index == info_before[1].bvh_index);
    // the neighbours
    REQUIRE(std::memcmp(&pool.mesh_info_cpu[0], &info_before[0], sizeof(voidin::MeshInfo)) == 0);
    REQUIRE(std::memcmp(&pool.mesh_info_cpu[2], &info_before[2], sizeof(voidin::MeshInfo)) == 0);
    REQUIRE(std::memcmp(pool.bvh_nodes.data(), nodes_before.data(), b0 * sizeof(voidin::BvhNode)) == 0);
    REQUIRE(std::memcmp(pool.bvh_nodes.data() + b1, nodes_before.data() + b1, (nodes_before.size() - b1) * sizeof(voidin::BvhNode)) == 0);
    for (size_t k = 0; k < indices_before.size(); ++k)
        if (k < info0.base_index || k >= info0.base_index + info0.index_count) REQUIRE(pool.indices[k] == indices_before[k]);
    for (size_t k = 0; k < vertices_before.size(); ++k)
        if (k < (size_t)info0.vertex_offset || k >= (size_t)info0.vertex_offset + moved.size())
            REQUIRE(std::memcmp(&pool.vertices[k], &vertices_before[k], sizeof(voidin::Vec3)) == 0);
    std::printf("rebuilt: %zu -> %zu nodes of %zu slots\n", first.nodes.size(), fresh.nodes.size(), 2 * T);

    bool threw = false;
    try { pool.rebuild_fast(1, moved.data(), moved.size() - 1, grid_i2.data(), grid_i2.size()); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw);
    threw = false;
    try { pool.rebuild_fast(1, moved.data(), moved.size(), grid_i2.data(), grid_i2.size() - 3); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw);
    threw = false;
    try { pool.rebuild_fast(9, moved.data(), moved.size(), grid_i2.data(), grid_i2.size()); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw);
    threw = false;                                                        // mesh 0 came through add(): it holds its 2 nodes, not 2 T slots
    try { pool.rebuild_fast(0, plane_v.data(), plane_v.size(), plane_i.data(), plane_i.size()); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw);
    REQUIRE(pool.bvh_nodes.size() == nodes_before.size());
    std::printf("blas_lbvh_mirror_test OK\n");
    return 0;
}
