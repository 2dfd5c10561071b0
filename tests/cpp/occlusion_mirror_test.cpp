// occlusion_mirror_test.cpp — one frame of two-pass occlusion culling through the C++ mirror (include/voidin.hpp):
//   pass::EmitDraws::record_early -> HizPyramid::build -> pass::EmitDraws::record_late, then record_hiz,
// with the visibility bits owned by an OcclusionState.  The scene comes from a file the Python test writes and the
// results go to a file it compares with the oracle (tests/test_gpu_cull_occlusion.py), so this program holds no
// expected values of its own.
//   in : u32 n_mesh, n_inst, width, height | camera (320 B) | meshes | instances | depth (width * height f32) | P words
//   out: u32 n_early, n_late, n_hiz | early list | late list | hiz list | visibility words after the late call
// Build: hipcc --offload-arch=gfx950 -I include tests/cpp/occlusion_mirror_test.cpp -L... -lvoidin_hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../include/voidin.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static void* alloc_zeroed(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, bytes) != hipSuccess) { (void)hipFree(p); return nullptr; }
    return p;
}
static void free_device(void* p) { (void)hipFree(p); }

template <typename T> static T* upload(const std::vector<T>& v) {
    T* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T) + 16) != hipSuccess) return nullptr;
    if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 3);
    std::FILE* f = std::fopen(argv[1], "rb");
    REQUIRE(f);
    uint32_t head[4];
    REQUIRE(std::fread(head, 4, 4, f) == 4);
    const uint32_t n_mesh = head[0], n = head[1], width = head[2], height = head[3];
    voidin::CameraUniform camera;
    REQUIRE(std::fread(&camera, sizeof(camera), 1, f) == 1);
    std::vector<voidin::MeshInfo> meshes(n_mesh);
    std::vector<voidin::Instance> inst(n);
    std::vector<float> depth((size_t)width * height);
    std::vector<uint64_t> prev((n + 63) / 64);
    REQUIRE(std::fread(meshes.data(), sizeof(voidin::MeshInfo), n_mesh, f) == n_mesh);
    REQUIRE(std::fread(inst.data(), sizeof(voidin::Instance), n, f) == n);
    REQUIRE(std::fread(depth.data(), 4, depth.size(), f) == depth.size());
    REQUIRE(std::fread(prev.data(), 8, prev.size(), f) == prev.size());
    std::fclose(f);

    voidin::Gpu gpu(0);
    voidin::pass::EmitDraws emit(gpu);
    voidin::HizPyramid pyramid(gpu, width, height);
    voidin::OcclusionState state(n, alloc_zeroed, free_device);
    REQUIRE(state.words() == prev.size() && state.bytes() == prev.size() * 8);
    {   // allocated zeroed
        std::vector<uint64_t> z(prev.size(), 1);
        REQUIRE(hipMemcpy(z.data(), state.visible(), state.bytes(), hipMemcpyDeviceToHost) == hipSuccess);
        for (uint64_t w : z) REQUIRE(w == 0);
    }
    REQUIRE(hipMemcpy(state.visible(), prev.data(), state.bytes(), hipMemcpyHostToDevice) == hipSuccess);

    voidin::MeshInfo* d_meshes = upload(meshes);
    voidin::Instance* d_inst = upload(inst);
    float* d_depth = upload(depth);
    float* d_pyr = static_cast<float*>(alloc_zeroed(pyramid.bytes()));
    voidin::DrawIndexedIndirect* d_list[3];
    for (auto& d : d_list) d = static_cast<voidin::DrawIndexedIndirect*>(alloc_zeroed((size_t)n * 20 + 16));
    uint32_t* d_counts = static_cast<uint32_t*>(alloc_zeroed(16));
    REQUIRE(d_meshes && d_inst && d_depth && d_pyr && d_list[0] && d_list[1] && d_list[2] && d_counts);

    voidin::World world{&camera, d_meshes, n_mesh, d_inst, n};
    voidin::ProfilerCommandEncoder encoder;          // the context's own stream
    try {
        emit.record_early(world, encoder, state.visible(), {d_list[0], d_counts + 0, false});
        pyramid.build(d_depth, d_pyr);
        emit.record_late(world, encoder, d_pyr, width, height, state.visible(), {d_list[1], d_counts + 1, false});
        emit.record_hiz(world, encoder, d_pyr, width, height, {d_list[2], d_counts + 2, false});
        gpu.synchronize();
    } catch (const voidin::Error& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    uint32_t counts[3];
    REQUIRE(hipMemcpy(counts, d_counts, 12, hipMemcpyDeviceToHost) == hipSuccess);
    std::FILE* o = std::fopen(argv[2], "wb");
    REQUIRE(o);
    REQUIRE(std::fwrite(counts, 4, 3, o) == 3);
    for (int k = 0; k < 3; ++k) {
        REQUIRE(counts[k] <= n);
        std::vector<voidin::DrawIndexedIndirect> list(counts[k]);
        if (counts[k]) REQUIRE(hipMemcpy(list.data(), d_list[k], (size_t)counts[k] * 20, hipMemcpyDeviceToHost) == hipSuccess);
        REQUIRE(std::fwrite(list.data(), 20, counts[k], o) == counts[k]);
    }
    std::vector<uint64_t> vis(prev.size());
    REQUIRE(hipMemcpy(vis.data(), state.visible(), state.bytes(), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(std::fwrite(vis.data(), 8, vis.size(), o) == vis.size());
    std::fclose(o);
    for (auto d : d_list) free_device(d);
    free_device(d_counts); free_device(d_pyr); free_device(d_depth); free_device(d_inst); free_device(d_meshes);
    std::printf("occlusion mirror ok: early %u, late %u, hiz %u of %u\n", counts[0], counts[1], counts[2], n);
    return 0;
}
