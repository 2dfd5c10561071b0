// The lighting pass through the C++ mirror (include/voidin.hpp, include/voidin_lighting.h): lighting, shade_gbuffer and
// TraceScene::shade_gbuffer - the composed calls against the two calls they are made of, shadow_gbuffer and lighting.
// The scene, the camera and the 4 x 1 image are gbuffer_trace_mirror_test.cpp's: a pinhole at (0, 0, 5) looking down -z, two
// octahedra under pixels 1 and 3 (materials 7 and 255), nothing under pixels 0 and 2.  The G-buffer is traced (gbuffer_trace), so
// this is the whole chain scene + camera + lights -> lit image.  Two lights: one above the middle between the octahedra, which reaches
// both and stands in front of both hit faces, and one far to the left with a short radius, which reaches neither.
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

// the image: one row of 256 bytes, prefilled with 0xC3; -> false when a byte beyond the four pixels changed
static bool read_back(const VdColorTarget& t, float* rgba16) {
    unsigned char row[256];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(row, t.rgba, 256, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (size_t b = 64; b < 256; ++b) if (row[b] != 0xC3) return false;
    std::memcpy(rgba16, row, 64);
    return true;
}

int main() {
    static_assert(sizeof(VdFlatMaterial) == 32 && sizeof(VdColorTarget) == 24 && VD_LIGHTING_MATERIALS == 256u, "the lighting records");
    voidin::Gpu gpu(0);
    std::vector<voidin::Vec3> v = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
    std::vector<uint32_t> idx = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    voidin::MeshPool pool(gpu);
    REQUIRE(pool.add({v.data(), v.size(), idx.data(), idx.size()}) == 0);
    const float centre[2][3] = {{-1.05f, 0.1f, 0.0f}, {3.95f, -0.1f, 0.0f}};
    const uint32_t material[2] = {7u, 0x1ffu};
    std::vector<voidin::Instance> inst(2);
    for (int k = 0; k < 2; ++k) {
        std::memset(&inst[k], 0, sizeof(inst[k]));
        for (int d = 0; d < 4; ++d) inst[k].transform[5 * d] = inst[k].inv_transform[5 * d] = 1.0f;
        for (int c = 0; c < 3; ++c) { inst[k].transform[12 + c] = centre[k][c]; inst[k].inv_transform[12 + c] = -centre[k][c]; }
        inst[k].material = material[k];
    }
    pool.generate_tlas(inst);
    const VdTraceScene scene = pool.trace_scene(inst);
    VdTraceScene ds = scene;
    ds.tlas_nodes = to_device(scene.tlas_nodes, scene.n_tlas_nodes); ds.instances = to_device(scene.instances, scene.n_instances);
    ds.meshes = to_device(scene.meshes, scene.n_meshes); ds.bvh_nodes = to_device(scene.bvh_nodes, scene.n_bvh_nodes);
    ds.vertices = to_device(scene.vertices, 3 * (size_t)scene.n_vertices); ds.indices = to_device(scene.indices, scene.n_indices);
    REQUIRE(ds.tlas_nodes && ds.instances && ds.meshes && ds.bvh_nodes && ds.vertices && ds.indices);

    VdCameraUniform camera;
    std::memset(&camera, 0, sizeof(camera));
    camera.view_position[2] = 5.0f; camera.view_position[3] = 1.0f;
    camera.clip_to_world[0] = 0.125f; camera.clip_to_world[5] = 0.125f; camera.clip_to_world[10] = 5.0f; camera.clip_to_world[11] = 1.0f; camera.clip_to_world[14] = -0.125f;
    for (int d = 0; d < 4; ++d) camera.view[5 * d] = 1.0f;
    camera.projection[0] = camera.projection[5] = 1.0f; camera.projection[11] = -1.0f; camera.projection[14] = 0.125f; camera.projection[15] = 5.0f;

    // the G-buffer from primary rays (the triangle's normal facing the eye: no vertex attributes)
    std::vector<unsigned char> fill(256, 0xC3);
    VdGBufferTarget images;
    std::memset(&images, 0, sizeof(images));
    images.depth = reinterpret_cast<float*>(to_device(fill.data(), 256)); images.depth_pitch = 256;
    images.normal_uv = reinterpret_cast<uint32_t*>(to_device(fill.data(), 256)); images.normal_uv_pitch = 256;
    images.material = to_device(fill.data(), 256); images.material_pitch = 255;
    images.width = 4; images.height = 1;
    REQUIRE(images.depth && images.normal_uv && images.material);
    voidin::TraceScene prepared(gpu, ds);
    voidin::gbuffer_trace(gpu, ds, nullptr, nullptr, camera, images);
    const VdGBuffer gb = voidin::gbuffer_of(images);
    unsigned char mat[4];
    REQUIRE(hipDeviceSynchronize() == hipSuccess && hipMemcpy(mat, images.material, 4, hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(mat[0] == 0 && mat[1] == 7 && mat[2] == 0 && mat[3] == 255);

    // the material table: every row its own values
    std::vector<VdFlatMaterial> table(VD_LIGHTING_MATERIALS);
    for (unsigned m = 0; m < VD_LIGHTING_MATERIALS; ++m) {
        const float f = (float)(m + 1) / 512.0f;
        table[m] = VdFlatMaterial{{f, 0.5f * f, 0.25f}, 0.75f, {0.125f * f, 0.0625f, 0.03125f * f}, 0xABCD0000u + m};
    }
    const VdFlatMaterial* d_table = to_device(table.data(), table.size());
    const VdLight lights[2] = {{{1.25f, 0.0f, 4.0f}, 20.0f, {1.0f, 0.5f, 0.25f}, 0u}, {{-40.0f, 0.0f, 0.0f}, 2.0f, {1.0f, 1.0f, 1.0f}, 0u}};
    const VdLight* d_lights = to_device(lights, 2);
    VdColorTarget target;
    target.rgba = reinterpret_cast<float*>(to_device(fill.data(), 256)); target.pitch = 256; target.width = 4; target.height = 1;
    uint32_t* d_occ = nullptr; uint32_t* d_inr = nullptr;
    REQUIRE(d_table && d_lights && target.rgba && hipMalloc(reinterpret_cast<void**>(&d_occ), 16) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&d_inr), 16) == hipSuccess);

    // no lights: the base colours, bit for bit
    float base[16], want[16], got[16];
    voidin::lighting(gpu, camera, gb, nullptr, 0, nullptr, nullptr, d_table, target);
    REQUIRE(read_back(target, base));
    for (int k = 0; k < 4; ++k) {
        if (k % 2 == 0) { REQUIRE(base[4 * k] == 1.0f && base[4 * k + 1] == 0.0f && base[4 * k + 2] == 1.0f && base[4 * k + 3] == 1.0f); continue; }
        const VdFlatMaterial& M = table[mat[k]];
        for (int c = 0; c < 3; ++c) { const volatile float p = M.albedo[c] * 0.3f; REQUIRE(base[4 * k + c] == p + M.emissive[c]); }
        REQUIRE(base[4 * k + 3] == 1.0f);
    }

    // the two calls
    const VdShadowGBufferInfo pass = voidin::shadow_gbuffer(gpu, ds, camera, gb, d_lights, 2, d_occ, d_inr);
    uint32_t inr[4];
    REQUIRE(hipMemcpy(inr, d_inr, 16, hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(pass.n_points == 2 && pass.n_rays == 2 && inr[0] == 0u && inr[1] == 1u && inr[2] == 0u && inr[3] == 1u);
    voidin::lighting(gpu, camera, gb, d_lights, 2, d_occ, d_inr, d_table, target);
    REQUIRE(read_back(target, want));
    for (int k = 0; k < 4; ++k) {
        if (k % 2 == 0) { REQUIRE(std::memcmp(want + 4 * k, base + 4 * k, 16) == 0); continue; }
        for (int c = 0; c < 3; ++c) REQUIRE(std::isfinite(want[4 * k + c]) && want[4 * k + c] > base[4 * k + c]);      // the light faces both hit faces
        REQUIRE(want[4 * k + 3] == 1.0f);
    }

    // the composed calls give the same bytes and report what the pass reported
    for (int form = 0; form < 2; ++form) {
        REQUIRE(hipMemset(target.rgba, 0xC3, 256) == hipSuccess);
        const VdShadowGBufferInfo info = form ? prepared.shade_gbuffer(camera, gb, d_lights, 2, d_table, target) : voidin::shade_gbuffer(gpu, ds, camera, gb, d_lights, 2, d_table, target);
        REQUIRE(read_back(target, got));
        REQUIRE(std::memcmp(got, want, sizeof(got)) == 0 && std::memcmp(&info, &pass, sizeof(info)) == 0);
    }
    // ... and without lights they are the step alone
    REQUIRE(hipMemset(target.rgba, 0xC3, 256) == hipSuccess);
    const VdShadowGBufferInfo none = voidin::shade_gbuffer(gpu, ds, camera, gb, nullptr, 0, d_table, target);
    REQUIRE(read_back(target, got));
    REQUIRE(std::memcmp(got, base, sizeof(got)) == 0 && none.n_points == 0 && none.words_per_point == 0);
    std::printf("lighting_mirror_test OK: two of four pixels lit; the composed calls give the bytes of shadow_gbuffer + lighting\n");
    return 0;
}
