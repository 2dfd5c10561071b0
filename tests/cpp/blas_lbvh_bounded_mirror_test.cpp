// blas_lbvh_bounded_mirror_test.cpp — VD_OPT_BLAS_LBVH_MAX_DEPTH through the C++ mirror (include/voidin.hpp): Gpu::set_option, then
// MeshPool::add_fast of a real mesh gives a tree that a walk with a 24-entry stack can take.
//   * without the option the mesh's LBVH is deeper than 23 (that is what the option is for; the helmet: 24);
//   * with the option at 23, max_depth <= 23, and the indices are the same permutation (only the topology changes);
//   * a few hundred rays walked by a literal push-both-children walk over a 24-entry array that gives up on overflow find the
//     distances of Bvh::traverse_iter bit for bit;
//   * a bound that cannot hold the mesh is refused with VD_ERR_INVALID_ARG, and the pool is what it was.
// The mesh comes from a file (argv[1]): u32 n_vertices, u32 n_indices, the positions (3 floats each), the indices.
// Build: hipcc --offload-arch=gfx950 -I include tests/cpp/blas_lbvh_bounded_mirror_test.cpp -L... -lvoidin_hip
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/voidin.hpp"

#pragma clang fp contract(off)

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint64_t rng_state = 0x5EED0123ull;
static float frand() {   // splitmix64 -> [0,1)
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}

using voidin::BvhNode;
using voidin::Vec3;

static Vec3 sub(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static float dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// the slab test of the walk, without a limit: does the ray enter the box in front of its origin?
static bool enters(Vec3 o, Vec3 d, const float* mn, const float* mx) {
    const float a[3] = {(mn[0] - o.x) / d.x, (mn[1] - o.y) / d.y, (mn[2] - o.z) / d.z};
    const float b[3] = {(mx[0] - o.x) / d.x, (mx[1] - o.y) / d.y, (mx[2] - o.z) / d.z};
    float tmin = -INFINITY, tmax = INFINITY;
    for (int q = 0; q < 3; ++q) { tmin = std::fmax(tmin, std::fmin(a[q], b[q])); tmax = std::fmin(tmax, std::fmax(a[q], b[q])); }
    return tmax >= tmin && tmax > 0.0f;
}
// Moeller-Trumbore in the operation order of the library's triangle test (vd_traverse_iter): t, or -1 for a miss
static float hit_triangle(Vec3 o, Vec3 d, Vec3 v0, Vec3 v1, Vec3 v2) {
    const float eps = 0.0001f;
    const Vec3 e1 = sub(v1, v0), e2 = sub(v2, v0), h = cross(d, e2);
    const float a = dot(e1, h);
    if (-eps < a && a < eps) return -1.0f;
    const float f = 1.0f / a;
    const Vec3 s = sub(o, v0);
    const float u = f * dot(s, h);
    if (!(0.0f <= u && u <= 1.0f)) return -1.0f;
    const Vec3 q = cross(s, e1);
    const float v = f * dot(d, q);
    if (v < 0.0f || u + v > 1.0f) return -1.0f;
    const float t = f * dot(e2, q);
    return t > eps ? t : -1.0f;
}

static unsigned depth_of(const BvhNode* n, uint32_t k) {
    return n[k].count ? 0u : 1u + std::max(depth_of(n, n[k].left_first), depth_of(n, n[k].left_first + 1));
}

// The shader's walk in its plainest form: pop a node; a leaf tests its triangles; an interior node whose box the ray enters pushes BOTH
// children.  24 entries, and an overflow ends the program (exit status 1).  -> closest t, or -1; *deepest = most entries held.
static float walk24(const BvhNode* nodes, const Vec3* verts, const uint32_t* idx, Vec3 o, Vec3 d, unsigned* deepest) {
    uint32_t stack[24];
    unsigned head = 0;
    stack[head++] = 0;
    float best = -1.0f;
    while (head) {
        const BvhNode& n = nodes[stack[--head]];
        if (!enters(o, d, n.min, n.max)) continue;
        if (n.count) {
            for (uint32_t k = 0; k < n.count; ++k) {
                const uint32_t* t = idx + 3 * (size_t)(n.left_first + k);
                const float x = hit_triangle(o, d, verts[t[0]], verts[t[1]], verts[t[2]]);
                if (x >= 0.0f && (best < 0.0f || x < best)) best = x;
            }
            continue;
        }
        if (head + 2 > 24) { std::printf("FAILED: the 24-entry stack overflowed\n"); std::exit(1); }
        stack[head++] = n.left_first;
        stack[head++] = n.left_first + 1;
        if (head > *deepest) *deepest = head;
    }
    return best;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 2);
    std::FILE* f = std::fopen(argv[1], "rb");
    REQUIRE(f);
    uint32_t head[2] = {0, 0};
    REQUIRE(std::fread(head, 4, 2, f) == 2 && head[0] > 0 && head[1] >= 12 && head[1] % 3 == 0);
    std::vector<Vec3> verts(head[0]);
    std::vector<uint32_t> indices(head[1]);
    REQUIRE(std::fread(verts.data(), sizeof(Vec3), verts.size(), f) == verts.size());
    REQUIRE(std::fread(indices.data(), 4, indices.size(), f) == indices.size());
    std::fclose(f);
    const size_t T = indices.size() / 3;

    voidin::Gpu gpu(0);
    // unbounded: the default
    std::vector<uint32_t> ui = indices;
    voidin::Bvh unbounded = voidin::BvhBuilder(gpu, verts.data(), verts.size(), reinterpret_cast<voidin::UVec3*>(ui.data()), T).build_fast();
    const unsigned depth0 = depth_of(unbounded.nodes.data(), 0);
    REQUIRE(depth0 > 23);                                                 // this mesh needs the option

    gpu.set_option(VD_OPT_BLAS_LBVH_MAX_DEPTH, 23);
    voidin::MeshPool pool(gpu);
    std::vector<uint32_t> pi = indices;
    REQUIRE(pool.add_fast({verts.data(), verts.size(), pi.data(), pi.size()}) == 0);
    const voidin::MeshInfo info = pool.mesh_info_cpu[0];
    const BvhNode* nodes = pool.bvh_nodes.data() + info.bvh_index;
    const unsigned depth = depth_of(nodes, 0);
    REQUIRE(depth <= 23);
    REQUIRE(pi == ui);                                                    // order is not the topology's business
    std::vector<uint32_t> bi = indices;
    voidin::Bvh bounded = voidin::BvhBuilder(gpu, verts.data(), verts.size(), reinterpret_cast<voidin::UVec3*>(bi.data()), T).build_fast();
    REQUIRE(std::memcmp(bounded.nodes.data(), nodes, bounded.nodes.size() * sizeof(BvhNode)) == 0 && bi == pi);
    REQUIRE(bounded.nodes.size() != unbounded.nodes.size() ||
            std::memcmp(bounded.nodes.data(), unbounded.nodes.data(), bounded.nodes.size() * sizeof(BvhNode)) != 0);
    std::printf("max_depth: %u unbounded, %u under the bound of 23\n", depth0, depth);

    // rays from a sphere around the mesh at points inside its box
    const float* mn = nodes[0].min; const float* mx = nodes[0].max;
    const Vec3 c = {0.5f * (mn[0] + mx[0]), 0.5f * (mn[1] + mx[1]), 0.5f * (mn[2] + mx[2])};
    const float R = 2.0f * std::sqrt((mx[0] - mn[0]) * (mx[0] - mn[0]) + (mx[1] - mn[1]) * (mx[1] - mn[1]) + (mx[2] - mn[2]) * (mx[2] - mn[2]));
    std::vector<VdRay> rays(400);
    for (VdRay& r : rays) {
        Vec3 p;
        float len;
        do { p = {2.0f * frand() - 1.0f, 2.0f * frand() - 1.0f, 2.0f * frand() - 1.0f}; len = std::sqrt(dot(p, p)); } while (len < 0.1f || len > 1.0f);
        const Vec3 o = {c.x + R * p.x / len, c.y + R * p.y / len, c.z + R * p.z / len};
        const Vec3 to = {mn[0] + frand() * (mx[0] - mn[0]), mn[1] + frand() * (mx[1] - mn[1]), mn[2] + frand() * (mx[2] - mn[2])};
        Vec3 d = sub(to, o);
        const float dl = std::sqrt(dot(d, d));
        std::memset(&r, 0, sizeof r);
        r.eye[0] = o.x; r.eye[1] = o.y; r.eye[2] = o.z;
        r.dir[0] = d.x / dl; r.dir[1] = d.y / dl; r.dir[2] = d.z / dl;
    }
    const std::vector<voidin::Dist> want = bounded.traverse_iter(gpu, verts.data(), verts.size(), reinterpret_cast<const voidin::UVec3*>(bi.data()), T, rays);
    unsigned deepest = 0, hits = 0;
    for (size_t k = 0; k < rays.size(); ++k) {
        const Vec3 o = {rays[k].eye[0], rays[k].eye[1], rays[k].eye[2]}, d = {rays[k].dir[0], rays[k].dir[1], rays[k].dir[2]};
        const float t = walk24(nodes, verts.data(), bi.data(), o, d, &deepest);
        const bool same = want[k].is_hit() ? std::memcmp(&t, &want[k].t, 4) == 0 : t < 0.0f;
        if (!same) std::printf("ray %zu: the walk found %.9g, traverse_iter %s %.9g\n", k, t, want[k].is_hit() ? "Hit" : "Miss", want[k].t);
        REQUIRE(same);
        hits += want[k].is_hit();
    }
    REQUIRE(hits > rays.size() / 8 && deepest <= 24);
    std::printf("walked: %zu rays, %u hits, %u of 24 stack entries used\n", rays.size(), hits, deepest);

    // a bound that cannot hold the mesh
    unsigned need = 0;
    while (((size_t)2 << need) < T) ++need;                                // the smallest D with T <= 2^(D+1)
    gpu.set_option(VD_OPT_BLAS_LBVH_MAX_DEPTH, (int64_t)need - 1);
    const std::vector<BvhNode> nodes_before = pool.bvh_nodes;
    bool threw = false;
    std::vector<uint32_t> ri = indices;
    try { pool.add_fast({verts.data(), verts.size(), ri.data(), ri.size()}); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw && pool.mesh_info_cpu.size() == 1 && pool.bvh_nodes.size() == nodes_before.size());
    gpu.set_option(VD_OPT_BLAS_LBVH_MAX_DEPTH, -1);
    std::vector<uint32_t> di = indices;
    voidin::Bvh again = voidin::BvhBuilder(gpu, verts.data(), verts.size(), reinterpret_cast<voidin::UVec3*>(di.data()), T).build_fast();
    REQUIRE(again.nodes.size() == unbounded.nodes.size() &&
            std::memcmp(again.nodes.data(), unbounded.nodes.data(), again.nodes.size() * sizeof(BvhNode)) == 0);
    std::printf("blas_lbvh_bounded_mirror_test OK\n");
    return 0;
}
