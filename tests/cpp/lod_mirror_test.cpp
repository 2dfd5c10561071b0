// lod_mirror_test.cpp — level-of-detail selection through the C++ mirror (include/voidin.hpp):
//   pass::EmitDraws::record_lod and record_batched_lod on a scene the Python test writes, results to a file it compares
//   byte for byte with the ctypes path and with tests/lod_cases.py (tests/test_cpp_lod.py) - this program holds no expected
//   draw lists of its own; and MeshPool::add_lods, whose group it checks here against the rows the pool recorded.
//   in : u32 n_group, n_mesh, n_inst, pad | camera (320 B) | VdLodParams (16 B) | groups | meshes | instances
//   out: u32 n_list, n_batched | list | n_mesh commands | n_batched ids
// Build: hipcc --offload-arch=gfx950 -I include tests/cpp/lod_mirror_test.cpp -L... -lvoidin_hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/voidin.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static_assert(sizeof(voidin::LodGroup) == 64 && sizeof(voidin::LodParams) == 16, "the header's layouts");

static void* alloc_filled(size_t bytes, int fill) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    if (hipMemset(p, fill, bytes) != hipSuccess) { (void)hipFree(p); return nullptr; }
    return p;
}

template <typename T> static T* upload(const std::vector<T>& v) {
    T* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T) + 16) != hipSuccess) return nullptr;
    if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

// a grid of q x q quads over [-h, h]^2 at height z: 2 q^2 triangles
static void grid(int q, float h, float z, std::vector<voidin::Vec3>& v, std::vector<uint32_t>& idx) {
    for (int y = 0; y <= q; ++y)
        for (int x = 0; x <= q; ++x) v.push_back({-h + 2 * h * x / q, -h + 2 * h * y / q, z});
    for (int y = 0; y < q; ++y)
        for (int x = 0; x < q; ++x) {
            const uint32_t a = (uint32_t)(y * (q + 1) + x), b = a + 1, c = a + (uint32_t)q + 1, d = c + 1;
            const uint32_t t[6] = {a, b, c, b, d, c};
            idx.insert(idx.end(), t, t + 6);
        }
}

static int pool_groups(voidin::Gpu& gpu) {
    voidin::MeshPool pool(gpu);
    std::vector<voidin::Vec3> plane = {{-.5f, 0, -.5f}, {-.5f, 0, .5f}, {.5f, 0, .5f}, {.5f, 0, -.5f}};
    std::vector<uint32_t> plane_i = {0, 1, 2, 0, 2, 3};
    REQUIRE(pool.add({plane.data(), plane.size(), plane_i.data(), plane_i.size()}) == 0);      // a mesh in front: first_row != 0
    std::vector<voidin::Vec3> v[3]; std::vector<uint32_t> idx[3];
    grid(8, 2.0f, 0.25f, v[0], idx[0]); grid(3, 1.5f, 0.0f, v[1], idx[1]); grid(1, 1.0f, 0.0f, v[2], idx[2]);
    voidin::MeshRef lods[3];
    for (int k = 0; k < 3; ++k) lods[k] = {v[k].data(), v[k].size(), idx[k].data(), idx[k].size()};
    const float sw[2] = {40.0f, 9.0f};
    const voidin::LodGroup g = pool.add_lods(lods, 3, sw);
    REQUIRE(g.first_row == 1 && g.n_lods == 3 && pool.mesh_info_cpu.size() == 4);
    REQUIRE(g.switch_size[0] == 40.0f && g.switch_size[1] == 9.0f);
    for (int k = 2; k < 7; ++k) REQUIRE(g.switch_size[k] == 0.0f);
    REQUIRE(std::memcmp(g.min, pool.mesh_info_cpu[1].min, 12) == 0 && std::memcmp(g.max, pool.mesh_info_cpu[1].max, 12) == 0);   // level 0's box
    REQUIRE(g.min[0] == -2.0f && g.max[1] == 2.0f && g.min[2] == 0.25f);
    uint32_t base = 6, vtx = 4;
    for (int k = 0; k < 3; ++k) {                        // consecutive rows with the index ranges MeshPool::add would give
        const voidin::MeshInfo& m = pool.mesh_info_cpu[1 + k];
        REQUIRE(m.index_count == idx[k].size() && m.base_index == base && m.vertex_offset == (int32_t)vtx);
        base += m.index_count; vtx += (uint32_t)v[k].size();
    }
    bool threw = false;
    try { pool.add_lods(lods, 0, sw); } catch (const voidin::Error& e) { threw = e.code == VD_ERR_INVALID_ARG; }
    REQUIRE(threw && pool.mesh_info_cpu.size() == 4);
    return 0;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 3);
    std::FILE* f = std::fopen(argv[1], "rb");
    REQUIRE(f);
    uint32_t head[4];
    REQUIRE(std::fread(head, 4, 4, f) == 4);
    const uint32_t n_group = head[0], n_mesh = head[1], n = head[2];
    voidin::CameraUniform camera;
    voidin::LodParams params;
    REQUIRE(std::fread(&camera, sizeof(camera), 1, f) == 1 && std::fread(&params, sizeof(params), 1, f) == 1);
    std::vector<voidin::LodGroup> groups(n_group);
    std::vector<voidin::MeshInfo> meshes(n_mesh);
    std::vector<voidin::Instance> inst(n);
    REQUIRE(std::fread(groups.data(), sizeof(voidin::LodGroup), n_group, f) == n_group);
    REQUIRE(std::fread(meshes.data(), sizeof(voidin::MeshInfo), n_mesh, f) == n_mesh);
    REQUIRE(std::fread(inst.data(), sizeof(voidin::Instance), n, f) == n);
    std::fclose(f);

    voidin::Gpu gpu(0);
    try {
        if (pool_groups(gpu)) return 1;
    } catch (const voidin::Error& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    voidin::pass::EmitDraws emit(gpu);
    voidin::LodGroup* d_groups = upload(groups);
    voidin::MeshInfo* d_meshes = upload(meshes);
    voidin::Instance* d_inst = upload(inst);
    auto* d_list = static_cast<voidin::DrawIndexedIndirect*>(alloc_filled((size_t)n * 20 + 16, 0xAB));
    auto* d_cmds = static_cast<voidin::DrawIndexedIndirect*>(alloc_filled((size_t)n_mesh * 20 + 16, 0xAB));
    auto* d_ids = static_cast<uint32_t*>(alloc_filled((size_t)n * 4 + 16, 0xAB));
    auto* d_counts = static_cast<uint32_t*>(alloc_filled(16, 0xFF));
    REQUIRE(d_groups && d_meshes && d_inst && d_list && d_cmds && d_ids && d_counts);

    voidin::World world{&camera, d_meshes, n_mesh, d_inst, n};
    voidin::ProfilerCommandEncoder encoder;          // the context's own stream
    const voidin::pass::EmitDrawsLodResource lod{d_groups, n_group, params};
    try {
        emit.record_lod(world, encoder, lod, {d_list, d_counts + 0, false});
        emit.record_batched_lod(world, encoder, lod, {d_cmds, d_ids, d_counts + 1});
        gpu.synchronize();
    } catch (const voidin::Error& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    uint32_t counts[2];
    REQUIRE(hipMemcpy(counts, d_counts, 8, hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(counts[0] <= n && counts[1] <= n);
    std::vector<voidin::DrawIndexedIndirect> list(counts[0]), cmds(n_mesh);
    std::vector<uint32_t> ids(counts[1]);
    if (counts[0]) REQUIRE(hipMemcpy(list.data(), d_list, (size_t)counts[0] * 20, hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(hipMemcpy(cmds.data(), d_cmds, (size_t)n_mesh * 20, hipMemcpyDeviceToHost) == hipSuccess);
    if (counts[1]) REQUIRE(hipMemcpy(ids.data(), d_ids, (size_t)counts[1] * 4, hipMemcpyDeviceToHost) == hipSuccess);
    std::FILE* o = std::fopen(argv[2], "wb");
    REQUIRE(o);
    REQUIRE(std::fwrite(counts, 4, 2, o) == 2);
    REQUIRE(std::fwrite(list.data(), 20, list.size(), o) == list.size());
    REQUIRE(std::fwrite(cmds.data(), 20, cmds.size(), o) == cmds.size());
    REQUIRE(std::fwrite(ids.data(), 4, ids.size(), o) == ids.size());
    std::fclose(o);
    (void)hipFree(d_counts); (void)hipFree(d_ids); (void)hipFree(d_cmds); (void)hipFree(d_list);
    (void)hipFree(d_inst); (void)hipFree(d_meshes); (void)hipFree(d_groups);
    std::printf("lod mirror ok: %u listed, %u batched of %u\n", counts[0], counts[1], n);
    return 0;
}
