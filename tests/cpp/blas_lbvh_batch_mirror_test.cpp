// blas_lbvh_batch_mirror_test.cpp — MeshPool::add_many_fast / rebuild_many_fast of the C++ mirror (include/voidin.hpp): many
// meshes through ONE batched LBVH build (vd_bvh_build_lbvh_batch).
//   * add_many_fast of five meshes leaves the pool - vertices, indices, nodes, MeshInfo rows - that five add_fast calls leave,
//     and permutes the callers' index slices as add_fast does;
//   * rebuild_many_fast of three of them leaves what three rebuild_fast calls leave;
//   * a batch with an index >= n_vert throws VD_ERR_INVALID_ARG and the pool is unchanged, in both calls.
// Build: hipcc --offload-arch=gfx950 -I include tests/cpp/blas_lbvh_batch_mirror_test.cpp -L... -lvoidin_hip
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/voidin.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint64_t rng_state = 0x5EED0123ull;
static float frand() {   // splitmix64 -> [0,1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}

struct Mesh { std::vector<voidin::Vec3> v; std::vector<uint32_t> i; };

// a grid of gx x gy quads over shared vertices, one of the two diagonals per quad
static Mesh grid(int gx, int gy, bool other, float phase) {
    Mesh m;
    for (int y = 0; y <= gy; ++y)
        for (int x = 0; x <= gx; ++x) m.v.push_back({(float)x * 0.25f + phase, 0.3f * std::sin(0.7f * x + phase) * std::cos(0.5f * y) + 0.05f * frand(), (float)y * 0.25f});
    for (int y = 0; y < gy; ++y)
        for (int x = 0; x < gx; ++x) {
            const uint32_t a = (uint32_t)(y * (gx + 1) + x), b = a + 1, c = a + (uint32_t)(gx + 1), d = c + 1;
            if (other) { const uint32_t t[6] = {a, b, d, a, d, c}; m.i.insert(m.i.end(), t, t + 6); }
            else { const uint32_t t[6] = {a, b, c, b, d, c}; m.i.insert(m.i.end(), t, t + 6); }
        }
    return m;
}

static bool same_pool(const voidin::MeshPool& a, const voidin::MeshPool& b) {
    return a.vertices.size() == b.vertices.size() && a.indices == b.indices && a.bvh_nodes.size() == b.bvh_nodes.size() &&
           a.mesh_info_cpu.size() == b.mesh_info_cpu.size() &&
           std::memcmp(a.vertices.data(), b.vertices.data(), a.vertices.size() * sizeof(voidin::Vec3)) == 0 &&
           std::memcmp(a.bvh_nodes.data(), b.bvh_nodes.data(), a.bvh_nodes.size() * sizeof(voidin::BvhNode)) == 0 &&
           std::memcmp(a.mesh_info_cpu.data(), b.mesh_info_cpu.data(), a.mesh_info_cpu.size() * sizeof(voidin::MeshInfo)) == 0;
}

int main() {
    voidin::Gpu gpu(0);
    // one triangle, a quad, and three grids: 1, 2, 70, 1 152 and 300 triangles
    std::vector<Mesh> src;
    src.push_back(Mesh{{{0, 0, 0}, {1, 0, 0}, {0, 1, 0}}, {0, 1, 2}});
    src.push_back(Mesh{{{-.5f, 0, -.5f}, {-.5f, 0, .5f}, {.5f, 0, .5f}, {.5f, 0, -.5f}}, {0, 1, 2, 0, 2, 3}});
    src.push_back(grid(7, 5, false, 0.0f));
    src.push_back(grid(24, 24, false, 1.0f));
    src.push_back(grid(15, 10, true, 2.0f));

    std::vector<Mesh> one = src, many = src;                // the calls permute the callers' index slices
    voidin::MeshPool a(gpu), b(gpu);
    for (size_t m = 0; m < one.size(); ++m) REQUIRE(a.add_fast({one[m].v.data(), one[m].v.size(), one[m].i.data(), one[m].i.size()}) == m);
    std::vector<voidin::MeshRef> refs;
    for (Mesh& m : many) refs.push_back({m.v.data(), m.v.size(), m.i.data(), m.i.size()});
    REQUIRE(b.add_many_fast(refs.data(), refs.size()) == 0);
    REQUIRE(same_pool(a, b));
    for (size_t m = 0; m < src.size(); ++m) REQUIRE(many[m].i == one[m].i);
    REQUIRE(many[3].i != src[3].i);                          // ... and they were permuted
    REQUIRE(b.add_many_fast(refs.data(), 0) == 5 && same_pool(a, b));
    std::printf("added: %zu meshes, %zu nodes\n", b.mesh_info_cpu.size(), b.bvh_nodes.size());

    // other triangulations and other positions for meshes 4, 2 and 3
    std::vector<Mesh> next = {grid(15, 10, false, 2.5f), grid(7, 5, true, 0.5f), grid(24, 24, true, 1.5f)};
    const uint32_t ids[3] = {4, 2, 3};
    for (int k = 0; k < 3; ++k) a.rebuild_fast(ids[k], next[k].v.data(), next[k].v.size(), next[k].i.data(), next[k].i.size());
    std::vector<voidin::MeshPool::MeshRebuild> jobs;
    for (int k = 0; k < 3; ++k) jobs.push_back({ids[k], next[k].v.data(), next[k].v.size(), next[k].i.data(), next[k].i.size()});
    const std::vector<voidin::BvhNode> nodes_before = b.bvh_nodes;
    b.rebuild_many_fast(jobs.data(), jobs.size());
    REQUIRE(same_pool(a, b));
    REQUIRE(std::memcmp(nodes_before.data(), b.bvh_nodes.data(), nodes_before.size() * sizeof(voidin::BvhNode)) != 0);
    std::printf("rebuilt: 3 meshes\n");

    // a bad index anywhere in a batch: VD_ERR_INVALID_ARG, the pool as it was
    voidin::MeshPool before(gpu);
    before.vertices = b.vertices; before.indices = b.indices; before.bvh_nodes = b.bvh_nodes; before.mesh_info_cpu = b.mesh_info_cpu;
    std::vector<Mesh> bad = src;
    bad[2].i[7] = (uint32_t)bad[2].v.size();
    std::vector<voidin::MeshRef> bad_refs;
    for (Mesh& m : bad) bad_refs.push_back({m.v.data(), m.v.size(), m.i.data(), m.i.size()});
    bool threw = false;
    try { b.add_many_fast(bad_refs.data(), bad_refs.size()); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw && same_pool(before, b));
    std::vector<uint32_t> bad_idx = next[1].i;
    bad_idx[4] = 0xffffffffu;
    jobs[1].indices = bad_idx.data();
    threw = false;
    try { b.rebuild_many_fast(jobs.data(), jobs.size()); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw && same_pool(before, b));
    jobs[1].indices = next[1].i.data();
    jobs[2].n_positions -= 1;                                // a count that differs: refused before anything is built
    threw = false;
    try { b.rebuild_many_fast(jobs.data(), jobs.size()); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw && same_pool(before, b));
    std::printf("blas_lbvh_batch_mirror_test OK\n");
    return 0;
}
