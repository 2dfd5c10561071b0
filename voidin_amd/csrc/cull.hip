// cull.hip — per-instance frustum cull, indirect-draw emission and ordered compaction for
// gfx950 (CDNA4, wave64).
//
// Replaces the `emit_draws` compute pass (reference: shaders/emit_draws.wgsl:13-64,
// shaders/utils/math.wgsl:67-73, dispatched by crates/app/src/pass/visibility.rs:233-254).
//
// Data movement (HBM-bound, no MFMA — fp32 compares and index work):
//   * instances are a 144-byte AoS (not a power of two).  A wave streams 64 consecutive
//     instances = 9216 contiguous bytes as 9 fully coalesced, nontemporal 16-B-per-lane loads,
//     parks them in a wave-private LDS slab, and every lane then reads back its own instance's
//     transform (4 x ds_read_b128 at a 144-B stride: 36-dword stride is conflict-free for b128)
//     and mesh id; the next round's loads are already in flight (register prefetch);
//   * emit path (reference format): the 20-byte commands of a wave (1280 contiguous bytes) go
//     through the same slab and leave as 16-B-per-lane stores;
//   * compact path, large inputs (split form), two launches: pass 1 `cull_mask_tiled_kernel`
//     writes only one ballot bit + a compact mesh id per instance and the survivors of every
//     1024-instance tile, so the read stream runs at ~6.5 TB/s (it is `cull_tile`, the one tile
//     skeleton, with `TiledPolicy`; the several-views and the occlusion pass 1 are the same
//     skeleton with `ViewsPolicy` / `OccPolicy`, and the LOD pass 1, `cull_mask_lod_kernel`, with `LodPolicy`, which
//     takes its box from a group table and stores the mesh-table ROW it picks as the instance's id); pass 2 `expand_mask_u8_kernel` /
//     `expand_mask_kernel`: workgroup c sums the tile counts before its 8192-instance chunk and
//     expands the chunk to out[offset[c]...): no ticket, no look-back, no wait on another
//     workgroup, every load issued before the first store.
//     (Storing the 20-byte commands from inside the read stream costs ~3x per byte: DESIGN.md §3.1);
//   * masks that pass 1 of the same call did not write carry no tile counts: for them
//     `mask_scan_kernel` (survivors per chunk, scanned by the last workgroup to arrive) runs in
//     front of the expansion - vd_expand_mask_dev and the dist.hip steps (all-gathered masks, the
//     occlusion path's second mask among them) - and of vd_mask_to_indices_dev;
//   * compact path, small inputs (fused form): `cull_compact_kernel<ROUNDS>`, one launch, a
//     decoupled look-back over 8-byte {epoch,status,value} granules ranks the tiles while
//     per-round (mesh id | visible) words wait in LDS;
//   * multi-GPU: the same pass 1 / pass 2 pair with the bitmask all-gathered in between
//     (vd_cull_mask_dev / vd_expand_mask_dev, voidin_amd/dist.py).
// Every float expression of the visibility test is written ONCE, below MeshRec: every kernel calls those.
#include "vd_common.hpp"

#include <math.h>

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kInstBytes = 144;
constexpr int kSlabBytes = kWave * kInstBytes;  // 9216
constexpr int kChunksPerLane = kSlabBytes / (kWave * 16);  // 9



typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct CullCamera {   // the slice of CameraUniform the shader reads (shared.wgsl:13-24)
    float view[16];
    float frustum[4];
    float znear, zfar;
};
// Occlusion extension (include/voidin_abi.h, "Occlusion culling"): the projection terms and the depth pyramid (hiz.hip)
struct OccProj { float p00, p11, p20, p21, p22, p32; };
struct HizView { const float* base; unsigned width, height, n_levels; unsigned off[17]; };

struct MeshRec { float mnx, mny, mnz; unsigned index_count; float mxx, mxy, mxz; unsigned base_index; int vertex_offset; };

__device__ __forceinline__ MeshRec load_mesh(const VdMeshInfo* __restrict__ meshes, unsigned mid) {
    const uint4* p = reinterpret_cast<const uint4*>(meshes + mid);
    const uint4 a = p[0], b = p[1];
    MeshRec m;
    m.mnx = __uint_as_float(a.x); m.mny = __uint_as_float(a.y); m.mnz = __uint_as_float(a.z); m.index_count = a.w;
    m.mxx = __uint_as_float(b.x); m.mxy = __uint_as_float(b.y); m.mxz = __uint_as_float(b.z); m.base_index = b.w;
    m.vertex_offset = meshes[mid].vertex_offset;
    return m;
}

struct LaneInst { float4 T0, T1, T2, T3; unsigned mesh; };   // T = transform columns

__device__ __forceinline__ float len3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// ------------------------------------------------------------------------------------------
// The visibility test: emit_draws.wgsl:13-33 with the evaluation order of SURVEY.md §8a C2', and the occlusion
// extension on the same view-space centre.  ONE definition of every expression: with
// -ffp-contract=off the order written here is the contract with the oracle, for every kernel below.
// ------------------------------------------------------------------------------------------
struct MeshCentre { float x, y, z; };
struct ViewCentre { float c[3]; float max_scale; };

// center = (mesh.max + mesh.min) / 2
__device__ __forceinline__ MeshCentre mesh_centre(const MeshRec& m) {
    return MeshCentre{(m.mxx + m.mnx) / 2.0f, (m.mxy + m.mny) / 2.0f, (m.mxz + m.mnz) / 2.0f};
}

// extract_scale (math.wgsl:67-73) and max_scale
__device__ __forceinline__ float max_scale(const float4 T0, const float4 T1, const float4 T2) {
    const float sx = len3(T0.x, T0.y, T0.z), sy = len3(T1.x, T1.y, T1.z), sz = len3(T2.x, T2.y, T2.z);
    return fmaxf(fmaxf(fabsf(sx), fabsf(sy)), fabsf(sz));
}

// Rows 0..2 of (view * transform) * vec4(centre, 1): the view-space centre, c[].
__device__ __forceinline__ void view_rows(const float* V, const MeshCentre c0, const float4 T0, const float4 T1, const float4 T2, const float4 T3,
                                          float (&c)[3]) {
    // column j = ((V.c0*Tj.x + V.c1*Tj.y) + V.c2*Tj.z) + V.c3*Tj.w
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float v0 = V[r], v1 = V[4 + r], v2 = V[8 + r], v3 = V[12 + r];
        const float m0 = ((v0 * T0.x + v1 * T0.y) + v2 * T0.z) + v3 * T0.w;
        const float m1 = ((v0 * T1.x + v1 * T1.y) + v2 * T1.z) + v3 * T1.w;
        const float m2 = ((v0 * T2.x + v1 * T2.y) + v2 * T2.z) + v3 * T2.w;
        const float m3 = ((v0 * T3.x + v1 * T3.y) + v2 * T3.z) + v3 * T3.w;
        // (VT * vec4(center, 1)).r
        c[r] = ((m0 * c0.x + m1 * c0.y) + m2 * c0.z) + m3 * 1.0f;
    }
}

// What both tests start from.  mesh_centre and max_scale do not depend on the camera: a kernel with several cameras computes
// them once per instance and calls the first form per camera; the second form is the whole of it for one camera.
__device__ __forceinline__ ViewCentre view_centre(const float* V, const MeshCentre c0, const LaneInst& li, float max_scale) {
    ViewCentre vc;
    view_rows(V, c0, li.T0, li.T1, li.T2, li.T3, vc.c);
    vc.max_scale = max_scale;
    return vc;
}
__device__ __forceinline__ ViewCentre view_centre(const float* V, const MeshRec& m, const LaneInst& li) {
    ViewCentre vc;
    view_rows(V, mesh_centre(m), li.T0, li.T1, li.T2, li.T3, vc.c);
    vc.max_scale = max_scale(li.T0, li.T1, li.T2);
    return vc;
}

__device__ __forceinline__ bool frustum_visible(const CullCamera& cam, const MeshRec& m, const ViewCentre& vc) {
    const float* c = vc.c;
    // radius: object-space min/max against the view-space centre — bug-compatible (C2)
    const float d0 = len3(m.mnx - c[0], m.mny - c[1], m.mnz - c[2]);
    const float d1 = len3(m.mxx - c[0], m.mxy - c[1], m.mxz - c[2]);
    const float radius = fmaxf(d0, d1) * vc.max_scale;
    if (c[2] * cam.frustum[1] - fabsf(c[0]) * cam.frustum[0] < -radius) return false;
    if (c[2] * cam.frustum[3] - fabsf(c[1]) * cam.frustum[2] < -radius) return false;
    if (c[2] + radius > cam.znear && c[2] - radius > cam.zfar) return false;
    return true;
}

// a TRUE bounding radius (the frustum test's is bug-compatible): the occlusion test's and the LOD metric's r
__device__ __forceinline__ float sphere_radius(const MeshRec& m, const ViewCentre& vc) {
    return (len3(m.mxx - m.mnx, m.mxy - m.mny, m.mxz - m.mnz) * 0.5f) * vc.max_scale;
}

// does the bounding sphere lie behind the depth pyramid?  (no reference counterpart: definition in include/voidin_abi.h)
__device__ __forceinline__ bool sphere_occluded(const OccProj& P, const float znear, const HizView& hz, const MeshRec& m, const ViewCentre& vc) {
    const float* c = vc.c;
    const float r = sphere_radius(m, vc);
    const float d = -c[2];
    const float dn = d - r;
    if (!(dn > znear)) return false;
    const float rr = r * r, dd = d * d, rd = r * d;
    const float tx = sqrtf((c[0] * c[0] + dd) - rr), ty = sqrtf((c[1] * c[1] + dd) - rr);
    const float dxm = d * tx + c[0] * r, dxp = d * tx - c[0] * r, dym = d * ty + c[1] * r, dyp = d * ty - c[1] * r;
    if (!(dxm > 0.0f && dxp > 0.0f && dym > 0.0f && dyp > 0.0f)) return false;
    const float sx0 = (c[0] * tx - rd) / dxm, sx1 = (c[0] * tx + rd) / dxp;
    const float sy0 = (c[1] * ty - rd) / dym, sy1 = (c[1] * ty + rd) / dyp;
    const float nxa = P.p00 * sx0 - P.p20, nxb = P.p00 * sx1 - P.p20, nya = P.p11 * sy0 - P.p21, nyb = P.p11 * sy1 - P.p21;
    const float nx_lo = fminf(nxa, nxb), nx_hi = fmaxf(nxa, nxb), ny_lo = fminf(nya, nyb), ny_hi = fmaxf(nya, nyb);
    const float W = (float)hz.width, H = (float)hz.height;
    const float u0 = (nx_lo * 0.5f + 0.5f) * W - 0.5f, u1 = (nx_hi * 0.5f + 0.5f) * W + 0.5f;
    const float v0 = (0.5f - ny_hi * 0.5f) * H - 0.5f, v1 = (0.5f - ny_lo * 0.5f) * H + 0.5f;
    if (!(u1 >= 0.0f && v1 >= 0.0f && u0 < W && v0 < H)) return false;
    const unsigned x0 = (unsigned)floorf(fmaxf(u0, 0.0f)), x1 = (unsigned)floorf(fminf(u1, W - 1.0f));
    const unsigned y0 = (unsigned)floorf(fmaxf(v0, 0.0f)), y1 = (unsigned)floorf(fminf(v1, H - 1.0f));
    const unsigned span = max(x1 - x0, y1 - y0);
    const unsigned lvl = min(span ? 32u - (unsigned)__clz((int)span) : 0u, hz.n_levels - 1u);
    const float* t = hz.base + hz.off[lvl];
    const unsigned lw = ((hz.width - 1u) >> lvl) + 1u;
    const unsigned ax = x0 >> lvl, bx = x1 >> lvl, ay = y0 >> lvl, by = y1 >> lvl;
    const float h0 = fminf(t[(size_t)ay * lw + ax], t[(size_t)ay * lw + bx]);
    const float h1 = fminf(t[(size_t)by * lw + ax], t[(size_t)by * lw + bx]);
    const float hmin = fminf(h0, h1);
    const float depth = (P.p32 - P.p22 * dn) / dn;
    return depth < hmin;
}

__device__ __forceinline__ bool is_visible(const CullCamera& cam, const MeshRec& m, const LaneInst& li) {
    return frustum_visible(cam, m, view_centre(cam.view, m, li));
}

// LOD selection (no reference counterpart: definition in include/voidin_abi.h, "Level of detail").  One row of the group
// table is 64 bytes: the box the tests above use, the first row of the group in the mesh table, and the thresholds.
struct LodParams { float scale, min_distance, min_size; };
struct LodRec { MeshRec box; unsigned first_row, n_lods; float switch_size[VD_LOD_MAX - 1]; };

__device__ __forceinline__ LodRec load_group(const VdLodGroup* __restrict__ groups, unsigned g) {
    const uint4* p = reinterpret_cast<const uint4*>(groups + g);
    const uint4 a = p[0], b = p[1], c = p[2], d = p[3];     // four independent 16-byte loads
    LodRec G;
    G.box.mnx = __uint_as_float(a.x); G.box.mny = __uint_as_float(a.y); G.box.mnz = __uint_as_float(a.z); G.first_row = a.w;
    G.box.mxx = __uint_as_float(b.x); G.box.mxy = __uint_as_float(b.y); G.box.mxz = __uint_as_float(b.z); G.n_lods = b.w;
    G.box.index_count = 0u; G.box.base_index = 0u; G.box.vertex_offset = 0;
    G.switch_size[0] = __uint_as_float(c.x); G.switch_size[1] = __uint_as_float(c.y); G.switch_size[2] = __uint_as_float(c.z);
    G.switch_size[3] = __uint_as_float(c.w); G.switch_size[4] = __uint_as_float(d.x); G.switch_size[5] = __uint_as_float(d.y);
    G.switch_size[6] = __uint_as_float(d.z);
    return G;
}

// size = the projected radius (pixels for scale = projection[5] * viewport_height / 2); a NaN distance gives min_distance
__device__ __forceinline__ float lod_size(const LodParams& P, const MeshRec& m, const ViewCentre& vc) {
    const float r = sphere_radius(m, vc);
    const float d = -vc.c[2];
    const float dist = fmaxf(d, P.min_distance);
    return (r * P.scale) / dist;
}

// the row of the mesh table: a COUNT of the thresholds above `size` (defined for unsorted ones; NaN counts none), every
// index clamped so that any table is defined
__device__ __forceinline__ unsigned lod_row(const LodRec& G, float size, unsigned n_mesh) {
    const unsigned nl = min(max(G.n_lods, 1u), (unsigned)VD_LOD_MAX);
    unsigned lod = 0u;
#pragma unroll
    for (unsigned k = 0; k + 1u < (unsigned)VD_LOD_MAX; ++k) lod += (k + 1u < nl && size < G.switch_size[k]) ? 1u : 0u;
    const unsigned first = min(G.first_row, n_mesh - 1u);
    return first + min(lod, n_mesh - 1u - first);           // == min(first + lod, n_mesh - 1) without the overflow
}

// Stream the 64 instances starting at `first` into this wave's LDS slab (coalesced 16 B per
// lane), then return this lane's transform + mesh id.  `n_valid` = instances in range (<= 64).
template <bool NT>
__device__ __forceinline__ void slab_fill(const VdInstance* __restrict__ inst, size_t first,
                                          unsigned n_valid, unsigned lane, u32x4 (&regs)[kChunksPerLane]) {
    const u32x4* src = reinterpret_cast<const u32x4*>(inst + first);
    const unsigned n_chunks = n_valid * (kInstBytes / 16);
#pragma unroll
    for (int j = 0; j < kChunksPerLane; ++j) {
        const unsigned c = j * kWave + lane;
        if (c < n_chunks) regs[j] = NT ? __builtin_nontemporal_load(src + c) : src[c];
        else regs[j] = u32x4{0u, 0u, 0u, 0u};
    }
}

__device__ __forceinline__ void slab_store(char* slab, unsigned lane, const u32x4 (&regs)[kChunksPerLane]) {
    u32x4* dst = reinterpret_cast<u32x4*>(slab);
#pragma unroll
    for (int j = 0; j < kChunksPerLane; ++j) dst[j * kWave + lane] = regs[j];
}

__device__ __forceinline__ LaneInst slab_read(const char* slab, unsigned lane) {
    const float4* p = reinterpret_cast<const float4*>(slab + lane * kInstBytes);
    LaneInst li;
    li.T0 = p[0]; li.T1 = p[1]; li.T2 = p[2]; li.T3 = p[3];
    li.mesh = *reinterpret_cast<const unsigned*>(slab + lane * kInstBytes + 128);
    return li;
}

// ------------------------------------------------------------------------------------------
// C1: emit_draws — every slot written (reference format).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock, 4) void emit_draws_kernel(CullCamera cam, const VdMeshInfo* __restrict__ meshes,
                                                            unsigned n_mesh, const VdInstance* __restrict__ inst,
                                                            unsigned n_inst, VdDrawIndexedIndirect* __restrict__ out,
                                                               unsigned n_wave_tiles, unsigned first_instance) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    char* slab = smem + wave * kSlabBytes;
    const unsigned waves_total = gridDim.x * kWavesPerBlock;
    u32x4 regs[kChunksPerLane];

    unsigned wt = blockIdx.x * kWavesPerBlock + wave;
    if (wt < n_wave_tiles) {
        const size_t f0 = (size_t)wt * kWave;
        slab_fill<true>(inst, f0, min(64u, n_inst - (unsigned)f0), lane, regs);
    }
    for (; wt < n_wave_tiles; wt += waves_total) {
        const size_t first = (size_t)wt * kWave;
        const unsigned n_valid = min(64u, n_inst - (unsigned)first);
        slab_store(slab, lane, regs);
        // prefetch the next wave-tile while this one is processed
        const unsigned wn = wt + waves_total;
        if (wn < n_wave_tiles) {
            const size_t fn = (size_t)wn * kWave;
            slab_fill<true>(inst, fn, min(64u, n_inst - (unsigned)fn), lane, regs);
        }
        vd_wave_lds_sync();
        const LaneInst li = slab_read(slab, lane);
        vd_wave_lds_sync();

        const unsigned mid = min(li.mesh, n_mesh - 1u);
        const MeshRec m = load_mesh(meshes, mid);
        const bool vis = is_visible(cam, m, li);

        // emit_draws.wgsl:55-63 — stage the wave's 64 commands (1280 B) and store 16 B per lane
        unsigned* cmd = reinterpret_cast<unsigned*>(slab) + lane * 5u;
        cmd[0] = m.index_count;
        cmd[1] = vis ? 1u : 0u;
        cmd[2] = m.base_index;
        cmd[3] = (unsigned)m.vertex_offset;
        cmd[4] = first_instance + (unsigned)first + lane;
        vd_wave_lds_sync();
        const unsigned n_bytes = n_valid * 20u;
        char* gdst = reinterpret_cast<char*>(out) + first * 20u;  // 1280-B multiples: 16-B aligned
        const uint4* s4 = reinterpret_cast<const uint4*>(slab);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned c = k * kWave + lane;
            const unsigned b = c * 16u;
            if (k == 1 && lane >= 16u) break;
            if (b + 16u <= n_bytes) {
                *reinterpret_cast<uint4*>(gdst + b) = s4[c];
            } else if (b < n_bytes) {  // ragged tail: 20-B records end on a 4-B boundary
                const unsigned* s1 = reinterpret_cast<const unsigned*>(slab + b);
                for (unsigned w = 0; b + 4u * w < n_bytes; ++w) reinterpret_cast<unsigned*>(gdst + b)[w] = s1[w];
            }
        }
        vd_wave_lds_sync();
    }
}

// ------------------------------------------------------------------------------------------
// C1 + C3 fused: cull and emit survivors only, ascending instance order, single pass (used below
// VdCtx::split_min = 2 Mi instances; larger inputs run the split form: cull_mask_tiled_kernel + expand_mask_kernel).
// ------------------------------------------------------------------------------------------
template <int ROUNDS>
__global__ __launch_bounds__(kBlock, 3)
void cull_compact_kernel(CullCamera cam, const VdMeshInfo* __restrict__ meshes, unsigned n_mesh,
                         const VdInstance* __restrict__ inst, unsigned n_inst, VdDrawIndexedIndirect* __restrict__ out,
                         unsigned* __restrict__ out_count, vd_u64* tile_state, vd_u64* ticket_counter,
                         unsigned n_tiles, unsigned first_instance, unsigned* fault_host) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // dynamic LDS: per-wave slabs, then per-round records (mesh id | visible << 31), then scalars
    unsigned* s_rec = reinterpret_cast<unsigned*>(smem + kWavesPerBlock * kSlabBytes);   // [ROUNDS][kBlock]
    unsigned* s_misc = s_rec + ROUNDS * kBlock;   // [0] ticket, [1] epoch / tile_excl, [2..5] wave totals
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    char* slab = smem + wave * kSlabBytes;

    if (threadIdx.x == 0) s_misc[0] = vd_take_ticket(ticket_counter, n_tiles, &s_misc[1]);
    __syncthreads();
    const unsigned tile = s_misc[0], epoch = s_misc[1];
    __syncthreads();
    if (tile >= n_tiles) return;                  // (the ticket word was not at {epoch, 0} when the launch began: never expected)
#ifdef VD_TUNING
    if (ticket_counter[1] == (vd_u64)tile + 1ull) return;   // tests/test_gpu_scan_fault.py: this workgroup "dies" before it publishes anything
#endif
    // The count is written by the LAST tile; until then it holds the error value, stored by the FIRST tile before anything can
    // depend on it (the fence completes the store before this tile's granule - which every other tile's prefix waits for - goes
    // out): a launch that loses its last workgroup leaves the sentinel, not the previous call's count.
    if (tile == 0u && threadIdx.x == 0) { __hip_atomic_store(out_count, VD_SCAN_STUCK, VD_RLX_AGENT); __threadfence(); }
    const size_t tile_first = (size_t)tile * (kBlock * ROUNDS);
    // wave-contiguous ranges keep the output order (wave, round, lane) == instance order
    const size_t wave_first = tile_first + (size_t)wave * (kWave * ROUNDS);
    auto valid_at = [&](size_t f) -> unsigned { return f < n_inst ? (unsigned)min((size_t)64, (size_t)n_inst - f) : 0u; };

    unsigned wave_total = 0;
    u32x4 regs[kChunksPerLane];
    slab_fill<true>(inst, wave_first, valid_at(wave_first), lane, regs);
#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
        const size_t first = wave_first + (size_t)r * kWave;
        const unsigned n_valid = valid_at(first);
        slab_store(slab, lane, regs);
        if (r + 1 < ROUNDS) slab_fill<true>(inst, first + kWave, valid_at(first + kWave), lane, regs);
        vd_wave_lds_sync();
        const LaneInst li = slab_read(slab, lane);
        vd_wave_lds_sync();
        const unsigned mid = min(li.mesh, n_mesh - 1u);
        const MeshRec m = load_mesh(meshes, mid);
        const bool vis = lane < n_valid && is_visible(cam, m, li);
        s_rec[r * kBlock + threadIdx.x] = mid | (vis ? 0x80000000u : 0u);
        wave_total += (unsigned)__popcll(__ballot(vis));
    }

    if (lane == 0) s_misc[2 + wave] = wave_total;
    __syncthreads();
    if (wave == 0) {
        unsigned tile_total = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) tile_total += s_misc[2 + w];
        const unsigned excl = vd_lookback(tile_state, epoch, tile, tile_total);
        if (lane == 0) {
            s_misc[1] = excl;
            if (tile == n_tiles - 1u) *out_count = vd_scan_final_count(tile_state, epoch, excl, tile_total, fault_host);
        }
    }
    __syncthreads();
    unsigned base = s_misc[1];
    if (base == VD_SCAN_STUCK) return;            // a predecessor never published its total: no list (the count says so)
    for (unsigned w = 0; w < wave; ++w) base += s_misc[2 + w];

#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned rec = s_rec[r * kBlock + threadIdx.x];
        const bool vis = (rec >> 31) != 0u;
        const unsigned long long mask = __ballot(vis);
        if (vis) {
            const unsigned mid = rec & 0x7fffffffu;
            const uint4* mp = reinterpret_cast<const uint4*>(meshes + mid);
            unsigned* o = reinterpret_cast<unsigned*>(out + (base + vd_mbcnt(mask)));
            o[0] = mp[0].w;                         // index_count
            o[1] = 1u;
            o[2] = mp[1].w;                         // base_index
            o[3] = (unsigned)meshes[mid].vertex_offset;
            o[4] = first_instance + (unsigned)(wave_first + (size_t)r * kWave) + lane;
        }
        base += (unsigned)__popcll(mask);
    }
}

template <int ROUNDS>
constexpr int compact_lds_bytes() { return kWavesPerBlock * kSlabBytes + ROUNDS * kBlock * 4 + 32; }

// ------------------------------------------------------------------------------------------
// Multi-GPU wire format: cull -> one bit per instance; expand bits -> ordered draw list.
// ------------------------------------------------------------------------------------------
// (vd_cull_mask_dev: the mask alone; the split single-GPU path uses cull_mask_tiled_kernel below)
__global__ __launch_bounds__(kBlock, 3) void cull_mask_kernel(CullCamera cam, const VdMeshInfo* __restrict__ meshes,
                                                               unsigned n_mesh, const VdInstance* __restrict__ inst,
                                                               unsigned n_inst, vd_u64* __restrict__ mask, unsigned n_wave_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    char* slab = smem + wave * kSlabBytes;
    const unsigned waves_total = gridDim.x * kWavesPerBlock;
    u32x4 regs[kChunksPerLane];
    unsigned wt = blockIdx.x * kWavesPerBlock + wave;
    if (wt < n_wave_tiles) {
        const size_t f0 = (size_t)wt * kWave;
        slab_fill<true>(inst, f0, min(64u, n_inst - (unsigned)f0), lane, regs);
    }
    for (; wt < n_wave_tiles; wt += waves_total) {
        const size_t first = (size_t)wt * kWave;
        const unsigned n_valid = min(64u, n_inst - (unsigned)first);
        slab_store(slab, lane, regs);
        const unsigned wn = wt + waves_total;
        if (wn < n_wave_tiles) {
            const size_t fn = (size_t)wn * kWave;
            slab_fill<true>(inst, fn, min(64u, n_inst - (unsigned)fn), lane, regs);
        }
        vd_wave_lds_sync();
        const LaneInst li = slab_read(slab, lane);
        vd_wave_lds_sync();
        const unsigned mid = min(li.mesh, n_mesh - 1u);
        const MeshRec m = load_mesh(meshes, mid);
        const bool vis = lane < n_valid && is_visible(cam, m, li);
        const unsigned long long b = __ballot(vis);
        if (lane == 0) mask[wt] = b;
    }
}

// ------------------------------------------------------------------------------------------
// Occlusion extension (no reference counterpart — definition in include/voidin_abi.h,
// "Occlusion culling"; pyramid built by hiz.hip).  mask_out = mask_in minus the instances whose bounding sphere lies
// behind the depth pyramid.  Words of mask_in that are 0 cost nothing: their 9 KB of instances are not read, which
// is the common case in the second pass of the two-pass scheme.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock, 3) void occlusion_mask_kernel(CullCamera cam, OccProj proj, HizView hz, const VdMeshInfo* __restrict__ meshes,
                                                                   unsigned n_mesh, const VdInstance* __restrict__ inst, unsigned n_inst,
                                                                   const vd_u64* __restrict__ mask_in, vd_u64* __restrict__ mask_out,
                                                                   unsigned n_wave_tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    char* slab = smem + wave * kSlabBytes;
    const unsigned waves_total = gridDim.x * kWavesPerBlock;
    u32x4 regs[kChunksPerLane];
    for (unsigned wt = blockIdx.x * kWavesPerBlock + wave; wt < n_wave_tiles; wt += waves_total) {
        const vd_u64 in = mask_in[wt];                       // wave-uniform
        if (in == 0ull) {
            if (lane == 0) mask_out[wt] = 0ull;
            continue;
        }
        const size_t first = (size_t)wt * kWave;
        const unsigned n_valid = min(64u, n_inst - (unsigned)first);
        slab_fill<false>(inst, first, n_valid, lane, regs);
        slab_store(slab, lane, regs);
        vd_wave_lds_sync();
        const LaneInst li = slab_read(slab, lane);
        vd_wave_lds_sync();
        bool keep = false;
        if (lane < n_valid && ((in >> lane) & 1ull)) {
            const MeshRec m = load_mesh(meshes, min(li.mesh, n_mesh - 1u));
            keep = !sphere_occluded(proj, cam.znear, hz, m, view_centre(cam.view, m, li));
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) mask_out[wt] = b;
    }
}

// ------------------------------------------------------------------------------------------
// Pass 1 of the two-launch forms: ONE tile skeleton (cull_tile), three kernels that differ in a policy.
// A wave owns kMaskRounds CONSECUTIVE rounds (1024 instances), keeps their mesh ids and ballot words on chip and flushes
// them once per tile as wide stores, so the read stream is interrupted by one 1-KB store per 147 KB read instead of a
// 64-B store per 9 KB.  With the flush goes the number of the tile's survivors, tile_count[t]: a plain store, ordered
// before pass 2 by the kernel boundary.  The expansion sums these to place its chunk (expand_mask_u8_kernel<.., true>).
// No atomics, no fences, no wait on another workgroup.
// ------------------------------------------------------------------------------------------
constexpr int kMaskRounds = 16;

// The id table's part of a tile: the tile's rows as the table holds them now, and - after the rounds - the store of every
// row that differs, or of the whole ragged last tile.  Mesh assignment is static in practice (only transforms animate:
// shaders/compute_update.wgsl), and a row that already matches is not written again - a store interleaved with the read
// stream costs ~3x its bytes, a load does not.  Always correct: any row that differs (first frame,
// reallocated scratch, edited instances) is rewritten.
template <typename IdT> struct TileIds {
    static constexpr int kBytes = kMaskRounds * kWave * (int)sizeof(IdT);
    static constexpr int kRows = kBytes / (kWave * 16);
    u32x4 old_ids[kRows];
    bool full_tile;
    __device__ __forceinline__ void load(const IdT* __restrict__ ids_out, size_t tile_first, unsigned n_inst, unsigned lane) {
        full_tile = tile_first + (size_t)kWave * kMaskRounds <= (size_t)n_inst;
        if (full_tile) {
#pragma unroll
            for (int r = 0; r < kRows; ++r)
                old_ids[r] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(ids_out) + tile_first * sizeof(IdT) + (size_t)r * kWave * 16 + lane * 16u);
        }
    }
    __device__ __forceinline__ void flush(IdT* __restrict__ ids_out, const IdT* s_ids, size_t tile_first, unsigned n_inst, unsigned lane) const {
        const size_t id_base = tile_first * sizeof(IdT);                 // bytes; tile_first % 1024 == 0 -> 16-B aligned
        const size_t id_end = min((size_t)n_inst, tile_first + (size_t)kWave * kMaskRounds) * sizeof(IdT);
        char* gids = reinterpret_cast<char*>(ids_out);
        if (full_tile) {
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const unsigned b0 = (unsigned)r * kWave * 16u + lane * 16u;
                const u32x4 nv = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(s_ids) + b0);
                const bool diff = nv.x != old_ids[r].x || nv.y != old_ids[r].y || nv.z != old_ids[r].z || nv.w != old_ids[r].w;
                if (__any(diff)) *reinterpret_cast<u32x4*>(gids + id_base + b0) = nv;
            }
        } else {
            for (unsigned b0 = lane * 16u; b0 < (unsigned)kBytes; b0 += kWave * 16u) {
                if (id_base + b0 + 16u <= id_end) {
                    *reinterpret_cast<u32x4*>(gids + id_base + b0) = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(s_ids) + b0);
                } else {
                    for (unsigned q = 0; q < 16u && id_base + b0 + q < id_end; ++q) gids[id_base + b0 + q] = reinterpret_cast<const char*>(s_ids)[b0 + q];
                }
            }
        }
    }
};

// Where a policy's box comes from.  Every form but the LOD one takes it from the mesh table: the clamped mesh id - which
// is also the id the table stores - and that mesh's record.  (LodSource, further down, reads a row of the group table.)
struct MeshBox { unsigned mid; MeshRec m; };
struct MeshSource {
    const VdMeshInfo* __restrict__ meshes; unsigned n_mesh;
    __device__ __forceinline__ MeshBox fetch(const LaneInst& li) const {
        const unsigned mid = min(li.mesh, n_mesh - 1u);
        return MeshBox{mid, load_mesh(meshes, mid)};
    }
};

// One wave's tile t.  The policy supplies the box and the id to store: its `src` fetches the record this lane's instance
// is tested with, and round - called once per round, `live` = the instance exists - keeps the ballot word(s) it decides
// on in its own registers and returns the id the table stores for the instance; flush(t), after the last round, stores
// the words and their survivor count(s).  Everything else of a tile is here: the instance stream through the
// wave-private slab (the next round's loads in flight while this one is tested) and the id table.
template <typename IdT, typename Policy>
__device__ __forceinline__ void cull_tile(const VdInstance* __restrict__ inst, unsigned n_inst, IdT* __restrict__ ids_out, unsigned t, Policy& policy) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    char* slab = smem + wave * (kSlabBytes + TileIds<IdT>::kBytes);
    IdT* s_ids = reinterpret_cast<IdT*>(slab + kSlabBytes);
    auto valid_at = [&](size_t f) -> unsigned { return f < n_inst ? (unsigned)min((size_t)64, (size_t)n_inst - f) : 0u; };
    const size_t tile_first = (size_t)t * (kWave * kMaskRounds);
    u32x4 regs[kChunksPerLane];
    slab_fill<true>(inst, tile_first, valid_at(tile_first), lane, regs);
    TileIds<IdT> tile_ids;
    tile_ids.load(ids_out, tile_first, n_inst, lane);
#pragma unroll 1
    for (int r = 0; r < kMaskRounds; ++r) {
        const size_t first = tile_first + (size_t)r * kWave;
        const unsigned n_valid = valid_at(first);
        slab_store(slab, lane, regs);
        if (r + 1 < kMaskRounds) slab_fill<true>(inst, first + kWave, valid_at(first + kWave), lane, regs);
        vd_wave_lds_sync();
        const LaneInst li = slab_read(slab, lane);
        vd_wave_lds_sync();
        const auto box = policy.src.fetch(li);
        s_ids[r * kWave + lane] = (IdT)policy.round(r, lane < n_valid, box, li);
    }
    vd_wave_lds_sync();
    policy.flush(t);
    tile_ids.flush(ids_out, s_ids, tile_first, n_inst, lane);
    vd_wave_lds_sync();
}

// The survivors of a tile from its 16 ballot words, one per lane of a 16-lane group (lanes that hold none pass 0): summed
// over the group, stored by the lane `leader` names.
__device__ __forceinline__ void store_tile_count(unsigned* __restrict__ dst, vd_u64 my_word, bool leader) {
    unsigned survivors = (unsigned)__popcll(my_word);
#pragma unroll
    for (int off = kMaskRounds / 2; off > 0; off >>= 1) survivors += __shfl_xor(survivors, off);
    if (leader) *dst = survivors;
}

// One camera: one ballot word per round, round r's in lane r.
struct TiledPolicy {
    const CullCamera& cam; const MeshSource src;
    vd_u64* __restrict__ mask; unsigned* __restrict__ tile_count; unsigned n_inst;
    const unsigned lane = threadIdx.x & 63u;
    vd_u64 my_word = 0;
    __device__ __forceinline__ unsigned round(int r, bool live, const MeshBox& box, const LaneInst& li) {
        const vd_u64 b = __ballot(live && is_visible(cam, box.m, li));
        if (lane == (unsigned)r) my_word = b;
        return box.mid;
    }
    __device__ __forceinline__ void flush(unsigned t) {
        const size_t w0 = (size_t)t * kMaskRounds, n_words = ((size_t)n_inst + 63) / 64;
        if (lane < (unsigned)kMaskRounds && w0 + lane < n_words) mask[w0 + lane] = my_word;
        store_tile_count(tile_count + t, my_word, lane == 0u);           // my_word is 0 in lanes >= kMaskRounds
    }
};

template <typename IdT>
__global__ __launch_bounds__(kBlock, 3) void cull_mask_tiled_kernel(CullCamera cam, const VdMeshInfo* __restrict__ meshes,
                                                                     unsigned n_mesh, const VdInstance* __restrict__ inst,
                                                                     unsigned n_inst, vd_u64* __restrict__ mask,
                                                                     IdT* __restrict__ ids_out, unsigned* __restrict__ tile_count,
                                                                     unsigned n_tiles) {
    for (unsigned t = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * kWavesPerBlock) {
        TiledPolicy policy{cam, MeshSource{meshes, n_mesh}, mask, tile_count, n_inst};
        cull_tile(inst, n_inst, ids_out, t, policy);
    }
}

// Several cameras in ONE read of the instances (vd_cull_compact_views*): the camera-independent part of the test
// (mesh_centre, max_scale) once per instance, the rest once per camera while the instance is in registers.  The test costs ~250 vector
// instructions per view and instance, under 15 % of the vector budget at the HBM rate, so a further view is
// close to free until the vector unit fills up.
//   * ONE instantiation per id width serves every view count: the view loop is a run-time loop (not unrolled), and its
//     22 camera dwords are fetched by scalar loads from the kernel-argument segment at a wave-uniform offset (eight
//     cameras are 176 dwords: more than the scalar registers of a wave, and nothing a lane should hold);
//   * the 16 ballot words of view v live in the lanes 16 (v & 3) .. + 15 of one of two 64-bit registers (v >> 2): no LDS
//     beyond the single-view kernel's, hence the same occupancy; the flush is one 8-byte store per lane and register;
//   * per tile: n_views x 16 mask words (view v's mask = mask + v * mask_stride), n_views survivor counts
//     (tile_count + v * count_stride) and the mesh ids ONCE.
constexpr int kMaxViews = VD_MAX_VIEWS;
static_assert(kMaxViews * kMaskRounds == 2 * kWave, "two ballot registers per lane hold every (view, round) word of a tile");
struct ViewCameras { CullCamera cam[kMaxViews]; };

struct ViewsPolicy {
    const ViewCameras& cams; unsigned n_views; const MeshSource src;
    vd_u64* __restrict__ mask; size_t mask_stride; unsigned* __restrict__ tile_count; unsigned count_stride; unsigned n_inst;
    const unsigned lane = threadIdx.x & 63u;
    vd_u64 word_lo = 0, word_hi = 0;      // lane l: the ballot of view (l >> 4) [+ 4] in round l & 15
    __device__ __forceinline__ unsigned round(int r, bool live, const MeshBox& box, const LaneInst& li) {
        const MeshRec& m = box.m;
        const MeshCentre c0 = mesh_centre(m);
        const float ms = max_scale(li.T0, li.T1, li.T2);
#pragma unroll 1
        for (unsigned v = 0; v < n_views; ++v) {
            const CullCamera& cam = cams.cam[v];
            const vd_u64 b = __ballot(live && frustum_visible(cam, m, view_centre(cam.view, c0, li, ms)));
            const unsigned slot = (v & 3u) * (unsigned)kMaskRounds + (unsigned)r;
            if (lane == slot) { if (v < 4u) word_lo = b; else word_hi = b; }
        }
        return box.mid;
    }
    // every lane stores its word of each register into its view's mask; the survivors of a view are the bits of its 16 lanes
    __device__ __forceinline__ void flush(unsigned t) {
        const size_t w0 = (size_t)t * kMaskRounds, n_words = ((size_t)n_inst + 63) / 64;
        const unsigned slot_view = lane >> 4, slot_round = lane & 15u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned v = (unsigned)h * 4u + slot_view;
            const vd_u64 my_word = h ? word_hi : word_lo;                // 0 where no view wrote it
            if (v < n_views && w0 + slot_round < n_words) mask[(size_t)v * mask_stride + w0 + slot_round] = my_word;
            store_tile_count(tile_count + (size_t)v * count_stride + t, my_word, slot_round == 0u && v < n_views);
        }
    }
};

template <typename IdT>
__global__ __launch_bounds__(kBlock, 3) void cull_mask_views_kernel(ViewCameras cams, unsigned n_views, const VdMeshInfo* __restrict__ meshes,
                                                                     unsigned n_mesh, const VdInstance* __restrict__ inst,
                                                                     unsigned n_inst, vd_u64* __restrict__ mask, size_t mask_stride,
                                                                     IdT* __restrict__ ids_out, unsigned* __restrict__ tile_count,
                                                                     unsigned count_stride, unsigned n_tiles) {
    for (unsigned t = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * kWavesPerBlock) {
        ViewsPolicy policy{cams, n_views, MeshSource{meshes, n_mesh}, mask, mask_stride, tile_count, count_stride, n_inst};
        cull_tile(inst, n_inst, ids_out, t, policy);
    }
}

// The occlusion-culled draw lists (vd_cull_compact_hiz*, vd_cull_early_dev, vd_cull_late_dev; extension, no reference
// counterpart): the frustum test AND - where a pyramid is bound - the occlusion test evaluated while the instance is in
// registers, so the list of unoccluded instances costs one read of the instances instead of two (vd_cull_mask_dev, then
// vd_occlusion_mask_dev).  With F = frustum_visible, V = F and not sphere_occluded, P = the caller's visible-last-frame bits:
//   HIZ,  no PREV (hiz):    list = V
//   PREV, no HIZ  (early):  list = F & P
//   HIZ and PREV  (late):   list = V & ~P, and V itself goes to visible_out (which may be the buffer P came from: a wave
//                           reads its tile's 16 words of P before it stores anything, and no other wave touches them)
// One view_centre feeds both tests.  Instances that fail the frustum test do not fetch pyramid texels, and a round none of
// whose instances passes skips the occlusion test altogether.  The pyramid is read through the ordinary cached path: only
// the instance stream is nontemporal.
template <bool HIZ, bool PREV>
struct OccPolicy {
    const CullCamera& cam; const OccProj& proj; const HizView& hz; const MeshSource src;
    vd_u64* __restrict__ mask; vd_u64* visible_out; unsigned* __restrict__ tile_count;
    const unsigned lane = threadIdx.x & 63u;
    bool my_slot;                         // lane r holds the words of round r
    unsigned p_lo = 0u, p_hi = 0u;
    vd_u64 list_word = 0, vis_word = 0;
    // this tile's 16 words of P, before anything of the tile is written (visible_out may be the same buffer)
    __device__ __forceinline__ void begin(unsigned t, unsigned n_inst, const vd_u64* prev) {
        const size_t w0 = (size_t)t * kMaskRounds, n_words = ((size_t)n_inst + 63) / 64;
        my_slot = lane < (unsigned)kMaskRounds && w0 + lane < n_words;
        if (PREV && my_slot) { const vd_u64 p = prev[w0 + lane]; p_lo = (unsigned)p; p_hi = (unsigned)(p >> 32); }
    }
    __device__ __forceinline__ unsigned round(int r, bool live, const MeshBox& box, const LaneInst& li) {
        const MeshRec& m = box.m;
        const ViewCentre vc = view_centre(cam.view, m, li);
        bool keep = live && frustum_visible(cam, m, vc);
        if (HIZ) {
            if (__ballot(keep) != 0ull) {                              // wave-uniform: a round wholly outside the frustum fetches no texel
                if (keep) keep = !sphere_occluded(proj, cam.znear, hz, m, vc);
            }
        }
        vd_u64 b = __ballot(keep);
        if (PREV) {
            const vd_u64 p = (vd_u64)(unsigned)__builtin_amdgcn_readlane((int)p_lo, r) |
                             ((vd_u64)(unsigned)__builtin_amdgcn_readlane((int)p_hi, r) << 32);
            if (HIZ) { if (lane == (unsigned)r) vis_word = b; b &= ~p; }
            else b &= p;
        }
        if (lane == (unsigned)r) list_word = b;
        return box.mid;
    }
    __device__ __forceinline__ void flush(unsigned t) {
        const size_t w0 = (size_t)t * kMaskRounds;
        if (my_slot) {
            mask[w0 + lane] = list_word;
            if (HIZ && PREV) visible_out[w0 + lane] = vis_word;
        }
        store_tile_count(tile_count + t, list_word, lane == 0u);         // list_word is 0 in lanes >= kMaskRounds
    }
};

template <typename IdT, bool HIZ, bool PREV>
__global__ __launch_bounds__(kBlock, 3) void cull_mask_occ_kernel(CullCamera cam, OccProj proj, HizView hz, const VdMeshInfo* __restrict__ meshes,
                                                                   unsigned n_mesh, const VdInstance* __restrict__ inst, unsigned n_inst,
                                                                   vd_u64* __restrict__ mask, const vd_u64* prev, vd_u64* visible_out,
                                                                   IdT* __restrict__ ids_out, unsigned* __restrict__ tile_count,
                                                                   unsigned n_tiles) {
    for (unsigned t = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * kWavesPerBlock) {
        OccPolicy<HIZ, PREV> policy{cam, proj, hz, MeshSource{meshes, n_mesh}, mask, visible_out, tile_count};
        policy.begin(t, n_inst, prev);
        // (t is the same in every lane of the wave.  The early forms say so: the tile's addresses then live in scalar registers,
        // which the 4-byte-id one, at the 168-register ceiling of three waves per SIMD, needs to stay free of spills.  The forms
        // that read the pyramid measured 0.2-0.6 % slower with it: profiles/cull_pass1_refactor.md, section 3)
        cull_tile(inst, n_inst, ids_out, HIZ ? t : (unsigned)__builtin_amdgcn_readfirstlane((int)t), policy);
    }
}

// Per-instance LOD selection written into the same id table (vd_cull_compact_lod*, vd_cull_batch_lod_dev, vd_lod_ids_dev;
// extension, no reference counterpart - definition in include/voidin_abi.h, "Level of detail").  The box comes from the
// instance's GROUP (one 64-byte row, four 16-byte loads, nothing that depends on another load), one view_centre feeds the
// frustum test and the size metric, and the id the table stores is the ROW of the mesh table the metric picks: the
// expansion and the counting sort read that table as before and never learn that a row is a level of detail.
//   MASK = false (vd_lod_ids_dev): the rows alone, for every instance - no visibility test, no mask, no counts.
struct LodSource {
    const VdLodGroup* __restrict__ groups; unsigned n_group;
    __device__ __forceinline__ LodRec fetch(const LaneInst& li) const { return load_group(groups, min(li.mesh, n_group - 1u)); }
};

template <bool MASK>
struct LodPolicy {
    const CullCamera& cam; const LodParams& P; const LodSource src; unsigned n_mesh;
    vd_u64* __restrict__ mask; unsigned* __restrict__ tile_count; unsigned n_inst;
    const unsigned lane = threadIdx.x & 63u;
    vd_u64 my_word = 0;
    __device__ __forceinline__ unsigned round(int r, bool live, const LodRec& G, const LaneInst& li) {
        const ViewCentre vc = view_centre(cam.view, G.box, li);
        const float size = lod_size(P, G.box, vc);
        const unsigned row = lod_row(G, size, n_mesh);       // the thresholds are dead before the frustum test needs registers
        if (MASK) {
            const bool drawn = frustum_visible(cam, G.box, vc) && !(size < P.min_size);
            const vd_u64 b = __ballot(live && drawn);
            if (lane == (unsigned)r) my_word = b;
        }
        return row;
    }
    __device__ __forceinline__ void flush(unsigned t) {
        if (!MASK) return;
        const size_t w0 = (size_t)t * kMaskRounds, n_words = ((size_t)n_inst + 63) / 64;
        if (lane < (unsigned)kMaskRounds && w0 + lane < n_words) mask[w0 + lane] = my_word;
        store_tile_count(tile_count + t, my_word, lane == 0u);           // my_word is 0 in lanes >= kMaskRounds
    }
};

template <typename IdT, bool MASK>
__global__ __launch_bounds__(kBlock, 3) void cull_mask_lod_kernel(CullCamera cam, LodParams P, const VdLodGroup* __restrict__ groups,
                                                                   unsigned n_group, unsigned n_mesh, const VdInstance* __restrict__ inst,
                                                                   unsigned n_inst, vd_u64* __restrict__ mask, IdT* __restrict__ ids_out,
                                                                   unsigned* __restrict__ tile_count, unsigned n_tiles) {
    for (unsigned t = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * kWavesPerBlock) {
        LodPolicy<MASK> policy{cam, P, LodSource{groups, n_group}, n_mesh, mask, tile_count, n_inst};
        // (t is wave-uniform; saying so keeps the tile's addresses in scalar registers, as in cull_mask_occ_kernel's early form)
        cull_tile(inst, n_inst, ids_out, (unsigned)__builtin_amdgcn_readfirstlane((int)t), policy);
    }
}

constexpr int kExpandGroup = 4;                      // mask words staged and stored as one contiguous run
constexpr int kExpandWords = 32;                     // mask words (64 instances each) per wave
constexpr int kChunkWords = kWavesPerBlock * kExpandWords;   // per workgroup: 128 words = 8192 instances

// Pass 2a for masks without pass 1's tile counts (vd_expand_mask_dev, vd_mask_to_indices_dev, the dist.hip steps; the
// single-GPU vd_cull_compact* does not launch it): survivors per 8192-instance chunk, then (last workgroup to finish) their
// exclusive scan in place and the total.  Keeping the scan out of pass 2b leaves that kernel without tickets, look-back or
// any other load that depends on another workgroup: under a saturated store stream every dependent load costs
// microseconds (on gfx950 loads and stores share vmcnt and the same queue), and 2b had four of them in a chain.
//
// Hand-off between workgroups without fences (an agent-scope release writes back the whole L2 of the XCD, ~100 ns per
// workgroup while the previous frame's command list is still dirty in it) and without a data race: a chunk's count
// travels as ONE naturally aligned 8-byte {launch epoch, count} word, written by one agent-scope atomic store and
// read by agent-scope atomic loads - the datum is its own flag, as in the look-back granules of vd_common.hpp.  The
// arrival counter only ELECTS the workgroup that scans; that workgroup accepts an entry when its tag is this
// launch's epoch (and polls the few that are still in flight), so nothing is inferred from the order of accesses to
// different addresses.  The epoch word is read at the start of every workgroup and advanced by the elected one after
// everybody has arrived, i.e. it is stable for the whole launch; launches on one stream are ordered by the stream.
constexpr int kScanBlock = 1024;                     // 16 waves: the last workgroup's scan is one round trip even at 80 M
struct ScanState { unsigned done, epoch, pad[2]; };  // followed by one vd_u64 entry per chunk: {epoch : 32 | value : 32}
__global__ __launch_bounds__(kScanBlock) void mask_scan_kernel(const vd_u64* __restrict__ mask, unsigned n_words, unsigned n_chunks,
                                                           vd_u64* chunk_entry, ScanState* state,
                                                           unsigned* __restrict__ out_count) {
    constexpr int kScanWaves = kScanBlock / kWave;
    __shared__ unsigned s_last, s_wave_sum[kScanWaves];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned ep = __hip_atomic_load(&state->epoch, VD_RLX_AGENT);
    const vd_u64 tag = (vd_u64)ep << 32;
    for (unsigned c = blockIdx.x * kScanWaves + wave; c < n_chunks; c += gridDim.x * kScanWaves) {
        const unsigned w = c * kChunkWords + lane;
        unsigned v = (w < n_words ? (unsigned)__popcll(mask[w]) : 0u) + (w + 64u < n_words ? (unsigned)__popcll(mask[w + 64u]) : 0u);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) __hip_atomic_store(&chunk_entry[c], tag | v, VD_RLX_AGENT);   // write-through: the datum is its own flag
    }
    // not needed for correctness (entries are self-validating): arriving only after this workgroup's stores have
    // completed means the elected workgroup almost never has to poll
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&state->done, 1u, VD_RLX_AGENT) == gridDim.x - 1u;
    __syncthreads();
    if (!s_last) return;
    // thread t scans the contiguous range [t*per, (t+1)*per): all its loads are independent (one round trip) and
    // read at agent scope (other XCDs wrote the counts)
    const unsigned per = (n_chunks + kScanBlock - 1) / kScanBlock;
    const unsigned begin = min(threadIdx.x * per, n_chunks), end = min(begin + per, n_chunks);
    // Bounded like every other cross-workgroup wait of the library: if the header and the entries ever disagree (a
    // launch on this context faulted mid-kernel, a stray write hit the state) the count becomes the sentinel 0xffffffff
    // - which the expansion pass and every consumer of *out_count treat as "no list" (it exceeds any instance count) -
    // instead of a stream that never finishes.
    bool stuck = false;
    auto entry = [&](unsigned c) -> unsigned {
        vd_u64 e = __hip_atomic_load(&chunk_entry[c], VD_RLX_AGENT);
        unsigned spins = 0;
        while ((e >> 32) != (vd_u64)ep) {                    // still in flight: its writer has arrived, the store lands shortly
            if (++spins > (1u << 22)) { stuck = true; return 0u; }
            __builtin_amdgcn_s_sleep(1);
            e = __hip_atomic_load(&chunk_entry[c], VD_RLX_AGENT);
        }
        return (unsigned)e;
    };
    unsigned sum = 0;
    for (unsigned c = begin; c < end; ++c) sum += entry(c);
    const bool any_stuck = __syncthreads_or(stuck ? 1 : 0) != 0;
    unsigned incl = sum;                                   // inclusive scan of the per-thread sums
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned t = __shfl_up(incl, off);
        if (lane >= (unsigned)off) incl += t;
    }
    if (lane == kWave - 1u) s_wave_sum[wave] = incl;
    __syncthreads();
    unsigned run = incl - sum;
    for (unsigned w = 0; w < wave; ++w) run += s_wave_sum[w];
    for (unsigned c = begin; c < end; ++c) {
        if (any_stuck) { chunk_entry[c] = tag | 0xffffffffu; continue; }   // pass 2b leaves such a chunk alone
        const unsigned v = entry(c);
        chunk_entry[c] = tag | run;                        // read by pass 2b, a later launch on this stream
        run += v;
    }
    if (threadIdx.x == kScanBlock - 1u) {
        *out_count = any_stuck ? 0xffffffffu : run;
        __hip_atomic_store(&state->done, 0u, VD_RLX_AGENT);        // re-armed for the next launch on this stream
        __hip_atomic_store(&state->epoch, ep + 1u, VD_RLX_AGENT);  // every workgroup of this launch has read it (all arrived)
    }
}

constexpr int kChunkTiles = kChunkWords / kMaskRounds;      // a chunk of pass 2 is 8 tiles of pass 1

// Second source of a chunk's offset (single-GPU step: the mask is pass 1's own, one shard): this thread's share of
// tile_count[0, n_before), the survivors of all tiles before the chunk.  At most ~10 independent 16-byte loads per thread
// at 10 M instances (4 per batch in flight), issued ahead of the kernel's mask / id loads and its first store - a load
// miss behind a write-saturated L2 costs microseconds.  The block-wide sum goes through LDS at the barrier the
// kernel has anyway.  The table is 16-byte aligned and padded to a multiple of 4 entries; entries at or past n_before
// may hold anything and are left out.
__device__ __forceinline__ unsigned tile_prefix_partial(const unsigned* __restrict__ tile_count, unsigned n_before) {
    constexpr unsigned kBatch = 4;
    unsigned sum = 0;
    for (unsigned i0 = threadIdx.x * 4u; i0 < n_before; i0 += kBatch * kBlock * 4u) {
        u32x4 v[kBatch];
#pragma unroll
        for (unsigned k = 0; k < kBatch; ++k) {
            const unsigned i = i0 + k * kBlock * 4u;
            v[k] = *reinterpret_cast<const u32x4*>(tile_count + (i < n_before ? i : i0));   // unconditional: no branch between the loads
        }
#pragma unroll
        for (unsigned k = 0; k < kBatch; ++k) {
            const unsigned i = i0 + k * kBlock * 4u;
            sum += (i < n_before ? v[k].x : 0u) + (i + 1u < n_before ? v[k].y : 0u) + (i + 2u < n_before ? v[k].z : 0u) +
                   (i + 3u < n_before ? v[k].w : 0u);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    return sum;                                           // the wave's share
}

// Pass 2b: workgroup c expands the 128 mask words of chunk c to out[chunk_offset[c] ...); word w belongs to shard
// w / wps and holds the instances shard*shard_size + 64*(w % wps) + bit.  Every load is issued before the first
// store (one round trip per workgroup).
//   TILES = false: chunk_offset[c] = chunk_entry[c], written by mask_scan_kernel (any mask: vd_expand_mask_dev, dist.hip).
//   TILES = true:  chunk_offset[c] = sum of pass 1's tile_count[] over the tiles before the chunk; no scan launch, no
//                  cross-workgroup wait and hence no "gave up" state.  The last workgroup also writes *out_count.
// General form (any id width, any shard size); expand_mask_u8_kernel below is the tuned common case.
//   TAB:  the mesh table fits the LDS copy (no global loads in the store loop).
template <typename IdT, bool TAB, bool TILES>
__global__ __launch_bounds__(kBlock) void expand_mask_kernel(const vd_u64* __restrict__ mask, unsigned n_words, unsigned wps,
                                                             unsigned shard_size, unsigned n_total, unsigned first_instance,
                                                             const IdT* __restrict__ mesh_ids,
                                                             const VdMeshInfo* __restrict__ meshes, unsigned n_mesh,
                                                             VdDrawIndexedIndirect* __restrict__ out,
                                                             const vd_u64* __restrict__ chunk_entry,
                                                             const unsigned* __restrict__ tile_count, unsigned* __restrict__ out_count) {
    constexpr int kGroups = kExpandWords / kExpandGroup;
    __shared__ unsigned s_prefix[kWavesPerBlock];
    constexpr unsigned kTab = TAB ? 512 : 1;              // mesh tables up to 512 entries are served from LDS
    __shared__ unsigned s_tab[kTab][3];                   // {index_count, base_index, vertex_offset}
    constexpr int kStageBytes = kExpandGroup * 1280 + 32;
    __shared__ __attribute__((aligned(16))) char s_stage[kWavesPerBlock][kStageBytes];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned chunk = blockIdx.x;
    const unsigned cw0 = chunk * kChunkWords;
    const unsigned w0 = __builtin_amdgcn_readfirstlane(cw0 + wave * kExpandWords);   // wave-uniform: scalar index math
    unsigned base = 0;
    if (TILES) {
        const unsigned part = tile_prefix_partial(tile_count, chunk * kChunkTiles);
        if (lane == 0) s_prefix[wave] = part;
    } else {
        base = (unsigned)chunk_entry[chunk];
        if (base == 0xffffffffu) return;                   // the scan gave up (mask_scan_kernel): no list
    }
    // survivors of the chunk's earlier waves: lane l looks at words cw0 + l and cw0 + 64 + l
    unsigned before = 0;
    if (lane < wave * kExpandWords && cw0 + lane < n_words) before = (unsigned)__popcll(mask[cw0 + lane]);
    if (lane + 64u < wave * kExpandWords && cw0 + 64u + lane < n_words) before += (unsigned)__popcll(mask[cw0 + 64u + lane]);
    // lane l < 32 holds mask word w0 + l
    vd_u64 my_word = 0;
    if (lane < (unsigned)kExpandWords && w0 + lane < n_words) my_word = mask[w0 + lane];
    // first instance of each word of group g (one division per group)
    auto group_first = [&](unsigned wg, unsigned (&f)[kExpandGroup]) {
        unsigned shard = wg / wps, r = wg - shard * wps;
#pragma unroll
        for (int q = 0; q < kExpandGroup; ++q) {
            f[q] = shard * shard_size + 64u * r;
            if (++r >= wps) { r = 0u; ++shard; }
        }
    };
    unsigned ids[kExpandWords];
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const unsigned wg = w0 + g * kExpandGroup;
        unsigned f[kExpandGroup];
        group_first(wg, f);
#pragma unroll
        for (int q = 0; q < kExpandGroup; ++q) {
            const unsigned idx = f[q] + lane;
            ids[g * kExpandGroup + q] = (wg + q < n_words && idx < n_total) ? (unsigned)mesh_ids[idx] : 0u;
        }
    }
    if (TAB)
        for (unsigned i = threadIdx.x; i < n_mesh; i += kBlock) {
            s_tab[i][0] = meshes[i].index_count; s_tab[i][1] = meshes[i].base_index; s_tab[i][2] = (unsigned)meshes[i].vertex_offset;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    base += before;
    __syncthreads();
    if (TILES) {
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) base += s_prefix[w];
        if (chunk == gridDim.x - 1u && wave == kWavesPerBlock - 1u) {   // the total: everything before this wave + its own words
            unsigned mine = (unsigned)__popcll(my_word);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
            if (lane == 0) *out_count = base + mine;
        }
    }
    // survivors of kExpandGroup mask words are staged in LDS at the destination's 16-B phase and leave as
    // 16-B-per-lane stores in one contiguous run (this kernel is write-dominated: 20 B out per ~1 B in)
    char* stage = s_stage[wave];
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const unsigned wg = w0 + g * kExpandGroup;
        vd_u64 m[kExpandGroup];
        unsigned cnt = 0;
#pragma unroll
        for (int q = 0; q < kExpandGroup; ++q) {
            const int k = g * kExpandGroup + q;
            const unsigned lo = __shfl((unsigned)my_word, k), hi = __shfl((unsigned)(my_word >> 32), k);
            m[q] = ((vd_u64)hi << 32) | lo;
            cnt += (unsigned)__popcll(m[q]);
        }
        if (cnt == 0u) continue;
        char* gbase = reinterpret_cast<char*>(out + base);
        const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(gbase) & 15u);
        unsigned run = 0;
        unsigned first[kExpandGroup];
        group_first(wg, first);
#pragma unroll
        for (int q = 0; q < kExpandGroup; ++q) {
            unsigned mid = ids[g * kExpandGroup + q];
            if ((m[q] >> lane) & 1ull) {
                mid = min(mid, n_mesh - 1u);
                unsigned* o = reinterpret_cast<unsigned*>(stage + shift + 20u * (run + vd_mbcnt(m[q])));
                if (TAB) { o[0] = s_tab[mid][0]; o[2] = s_tab[mid][1]; o[3] = s_tab[mid][2]; }
                else { o[0] = meshes[mid].index_count; o[2] = meshes[mid].base_index; o[3] = (unsigned)meshes[mid].vertex_offset; }
                o[1] = 1u;
                o[4] = first_instance + first[q] + lane;
            }
            run += (unsigned)__popcll(m[q]);
        }
        vd_wave_lds_sync();
        const unsigned total = shift + 20u * cnt;
        char* g16 = gbase - shift;
        for (unsigned b0 = lane * 16u; b0 < total; b0 += kWave * 16u) {
            if (b0 >= shift && b0 + 16u <= total) {
                *reinterpret_cast<u32x4*>(g16 + b0) = *reinterpret_cast<const u32x4*>(stage + b0);
            } else {
                const unsigned lo_b = b0 > shift ? b0 : shift, hi_b = b0 + 16u < total ? b0 + 16u : total;
                for (unsigned b = lo_b; b < hi_b; b += 4u)
                    *reinterpret_cast<unsigned*>(g16 + b) = *reinterpret_cast<const unsigned*>(stage + b);
            }
        }
        vd_wave_lds_sync();
        base += cnt;
    }
}

// Pass 2b, fast path: 1-byte ids, mesh table <= 256 entries, every group of 4 mask words inside one shard and the id
// table 4-byte aligned.  This kernel is bound by instruction issue (a wave64 instruction takes 4 cycles), not by LDS
// or store bandwidth, so the per-survivor instruction count is what is tuned here:
//   * all index math that is uniform across the wave runs on the scalar unit (w0 through readfirstlane, shard walk
//     by increments instead of a division per word);
//   * the mask word is the exec mask of the survivor branch (inverse ballot), no per-lane bit test;
//   * a group's 256 ids are one dword per lane, redistributed with ds_bpermute;
//   * the LDS mesh table holds ready-made {index_count, 1, base_index, vertex_offset} rows: one ds_read_b128;
//   * DIRECT: a command leaves as one 16-byte + one 4-byte store at a 20-byte lane stride (L2 merges the lines);
//     otherwise it is staged in LDS at the destination's 16-B phase and leaves in 16-B-per-lane runs.
// The dword that holds the last valid id may extend past n_total: an aligned dword that contains one valid byte
// never crosses a page, and the extra bytes belong to instances whose mask bit is 0.
template <bool DIRECT, bool TILES>
__global__ __launch_bounds__(kBlock) void expand_mask_u8_kernel(const vd_u64* __restrict__ mask, unsigned n_words, unsigned wps,
                                                                unsigned shard_size, unsigned n_total, unsigned first_instance,
                                                                const unsigned char* __restrict__ mesh_ids,
                                                                const VdMeshInfo* __restrict__ meshes, unsigned n_mesh,
                                                                VdDrawIndexedIndirect* __restrict__ out,
                                                                const vd_u64* __restrict__ chunk_entry,
                                                                const unsigned* __restrict__ tile_count, unsigned* __restrict__ out_count) {
    constexpr int kGroups = kExpandWords / kExpandGroup;
    __shared__ unsigned s_prefix[kWavesPerBlock];
    __shared__ __attribute__((aligned(16))) unsigned s_tab[256][4];
    constexpr int kStageBytes = DIRECT ? 16 : kExpandGroup * 1280 + 32;
    __shared__ __attribute__((aligned(16))) char s_stage[kWavesPerBlock][kStageBytes];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned chunk = blockIdx.x;
    const unsigned cw0 = chunk * kChunkWords;
    const unsigned w0 = cw0 + wave * kExpandWords;
    unsigned base = 0;
    if (TILES) {
        const unsigned part = tile_prefix_partial(tile_count, chunk * kChunkTiles);
        if (lane == 0) s_prefix[wave] = part;
    } else {
        base = (unsigned)chunk_entry[chunk];
        if (base == 0xffffffffu) return;                   // the scan gave up (mask_scan_kernel): no list
    }
    // survivors of the chunk's earlier waves: lane l looks at words cw0 + l and cw0 + 64 + l
    unsigned before = 0;
    if (lane < wave * kExpandWords && cw0 + lane < n_words) before = (unsigned)__popcll(mask[cw0 + lane]);
    if (lane + 64u < wave * kExpandWords && cw0 + 64u + lane < n_words) before += (unsigned)__popcll(mask[cw0 + 64u + lane]);
    vd_u64 my_word = 0;                                   // lane l < 32 holds mask word w0 + l
    if (lane < (unsigned)kExpandWords && w0 + lane < n_words) my_word = mask[w0 + lane];
    // ids: lanes 16q..16q+15 of register g hold the 64 ids of the group's word q, four per lane (one dword); the
    // shard walk advances by increments (wps >= 4), one division per wave
    unsigned ids[kGroups];
    {
        const unsigned wl = w0 + (lane >> 4);
        unsigned shard = wl / wps, r = wl - shard * wps;
#pragma unroll
        for (int g = 0; g < kGroups; ++g) {
            const unsigned i0 = shard * shard_size + 64u * r + 4u * (lane & 15u);
            ids[g] = (wl + g * kExpandGroup < n_words && i0 < n_total) ? *reinterpret_cast<const unsigned*>(mesh_ids + i0) : 0u;
            r += kExpandGroup;
            if (r >= wps) { r -= wps; ++shard; }
        }
    }
    unsigned s_shard = w0 / wps, s_r = w0 - s_shard * wps;   // scalar walk over the wave's words
    unsigned word_first = s_shard * shard_size + 64u * s_r;
    // staged form: touch the mask words and ids of chunk c + 8 PF.  Workgroups are dealt to the 8 XCDs round-robin, so
    // that chunk will be expanded on this XCD and finds its inputs in this L2: behind a write-saturated L2 a load MISS
    // waits for an eviction (tens of microseconds), and these misses are nobody's critical path.
    constexpr unsigned PF = DIRECT ? 0u : 32u;
    unsigned pf = 0;
    if (PF > 0) {
        const unsigned pw = (chunk + 8u * PF) * kChunkWords + (threadIdx.x >> 1);
        if (pw < n_words) {
            const unsigned ps = pw / wps;
            const unsigned pi = ps * shard_size + 64u * (pw - ps * wps) + 32u * (threadIdx.x & 1u);
            if (pi + 32u <= n_total) {
                const u32x4 a = *reinterpret_cast<const u32x4*>(mesh_ids + pi), b = *reinterpret_cast<const u32x4*>(mesh_ids + pi + 16u);
                pf = a.x ^ a.w ^ b.x ^ b.w;
            }
            if ((threadIdx.x & 1u) == 0u) pf ^= (unsigned)mask[pw];
        }
    }
    if (threadIdx.x < n_mesh) {
        const VdMeshInfo mi = meshes[threadIdx.x];
        s_tab[threadIdx.x][0] = mi.index_count; s_tab[threadIdx.x][1] = 1u;
        s_tab[threadIdx.x][2] = mi.base_index;  s_tab[threadIdx.x][3] = (unsigned)mi.vertex_offset;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    base = __builtin_amdgcn_readfirstlane(base + before);
    __syncthreads();
    if (TILES) {
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) base += s_prefix[w];
        base = __builtin_amdgcn_readfirstlane(base);
        if (chunk == gridDim.x - 1u && wave == kWavesPerBlock - 1u) {   // the total: everything before this wave + its own words
            unsigned mine = (unsigned)__popcll(my_word);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
            if (lane == 0) *out_count = base + mine;
        }
    }
    const unsigned max_mid = n_mesh - 1u;
    const unsigned inst_lane = first_instance + lane;
    const unsigned id_shift = 8u * (lane & 3u);
    char* stage = s_stage[wave];
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        vd_u64 m[kExpandGroup];
        unsigned cnt = 0;
#pragma unroll
        for (int q = 0; q < kExpandGroup; ++q) {
            const int k = g * kExpandGroup + q;
            const unsigned lo = __builtin_amdgcn_readlane((unsigned)my_word, k), hi = __builtin_amdgcn_readlane((unsigned)(my_word >> 32), k);
            m[q] = ((vd_u64)hi << 32) | lo;
            cnt += (unsigned)__popcll(m[q]);
        }
        unsigned wf[kExpandGroup];                         // first instance of each word of the group
#pragma unroll
        for (int q = 0; q < kExpandGroup; ++q) {
            wf[q] = word_first;
            if (++s_r >= wps) { s_r = 0u; ++s_shard; }
            word_first = s_shard * shard_size + 64u * s_r;
        }
        if (cnt == 0u) continue;
        if (DIRECT) {
            unsigned run = base;
#pragma unroll
            for (int q = 0; q < kExpandGroup; ++q) {
                const unsigned v = (unsigned)__shfl((int)ids[g], q * 16 + (int)(lane >> 2));
                const unsigned mid = min((v >> id_shift) & 0xffu, max_mid);
                if (__builtin_amdgcn_inverse_ballot_w64(m[q])) {
                    unsigned* o = reinterpret_cast<unsigned*>(out + (run + vd_mbcnt(m[q])));
                    typedef u32x4 __attribute__((aligned(4))) u32x4_a4;
                    *reinterpret_cast<u32x4_a4*>(o) = *reinterpret_cast<const u32x4*>(s_tab[mid]);
                    o[4] = inst_lane + wf[q];
                }
                run += (unsigned)__popcll(m[q]);
            }
        } else {
            char* gbase = reinterpret_cast<char*>(out + base);
            const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(gbase) & 15u);
            unsigned run = 0;
#pragma unroll
            for (int q = 0; q < kExpandGroup; ++q) {
                const unsigned v = (unsigned)__shfl((int)ids[g], q * 16 + (int)(lane >> 2));
                const unsigned mid = min((v >> id_shift) & 0xffu, max_mid);
                if (__builtin_amdgcn_inverse_ballot_w64(m[q])) {
                    unsigned* o = reinterpret_cast<unsigned*>(stage + shift + 20u * (run + vd_mbcnt(m[q])));
                    const u32x4 c = *reinterpret_cast<const u32x4*>(s_tab[mid]);
                    o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w;
                    o[4] = inst_lane + wf[q];
                }
                run += (unsigned)__popcll(m[q]);
            }
            vd_wave_lds_sync();
            const unsigned total = shift + 20u * cnt;
            char* g16 = gbase - shift;
            for (unsigned b0 = lane * 16u; b0 < total; b0 += kWave * 16u) {
                if (b0 >= shift && b0 + 16u <= total) {
                    *reinterpret_cast<u32x4*>(g16 + b0) = *reinterpret_cast<const u32x4*>(stage + b0);
                } else {
                    const unsigned lo_b = b0 > shift ? b0 : shift, hi_b = b0 + 16u < total ? b0 + 16u : total;
                    for (unsigned b = lo_b; b < hi_b; b += 4u)
                        *reinterpret_cast<unsigned*>(g16 + b) = *reinterpret_cast<const unsigned*>(stage + b);
                }
            }
            vd_wave_lds_sync();
        }
        base += cnt;
    }
    if (PF > 0 && pf == 0x9e3779b9u && n_mesh == 0u) out[0].instance_count = pf;   // never true: keeps the prefetch loads
}

// Reference-format emission (C1: every slot written, shaders/emit_draws.wgsl:49-63) from pass 1's bits and ids: the
// split form of vd_cull_emit for large inputs.  A lane owns 4 consecutive instances = 80 contiguous bytes = five
// aligned 16-byte stores; no scan is needed (slot = instance index).
template <typename IdT>
__global__ __launch_bounds__(kBlock) void emit_from_mask_kernel(const vd_u64* __restrict__ mask, const IdT* __restrict__ mesh_ids,
                                                               const VdMeshInfo* __restrict__ meshes, unsigned n_mesh,
                                                               unsigned n_inst, unsigned first_instance,
                                                               VdDrawIndexedIndirect* __restrict__ out) {
    constexpr unsigned kTab = 512;
    __shared__ __attribute__((aligned(16))) unsigned s_tab[kTab][4];
    const bool tab = n_mesh <= kTab;
    if (tab)
        for (unsigned i = threadIdx.x; i < n_mesh; i += kBlock) {
            s_tab[i][0] = meshes[i].index_count; s_tab[i][1] = 0u;
            s_tab[i][2] = meshes[i].base_index;  s_tab[i][3] = (unsigned)meshes[i].vertex_offset;
        }
    __syncthreads();
    const unsigned n_quads = (n_inst + 3u) / 4u;
    for (unsigned q = blockIdx.x * kBlock + threadIdx.x; q < n_quads; q += gridDim.x * kBlock) {
        const unsigned i0 = q * 4u;
        const unsigned bits = (unsigned)(mask[i0 >> 6] >> (i0 & 63u)) & 15u;
        unsigned mid[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) mid[k] = i0 + k < n_inst ? min((unsigned)mesh_ids[i0 + k], n_mesh - 1u) : 0u;
        unsigned w[20];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u32x4 c;
            if (tab) c = *reinterpret_cast<const u32x4*>(s_tab[mid[k]]);
            else { c.x = meshes[mid[k]].index_count; c.z = meshes[mid[k]].base_index; c.w = (unsigned)meshes[mid[k]].vertex_offset; }
            w[5 * k] = c.x; w[5 * k + 1] = (bits >> k) & 1u; w[5 * k + 2] = c.z; w[5 * k + 3] = c.w; w[5 * k + 4] = first_instance + i0 + k;
        }
        unsigned* o = reinterpret_cast<unsigned*>(out + i0);
        if (i0 + 4u <= n_inst) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                u32x4 v; v.x = w[4 * k]; v.y = w[4 * k + 1]; v.z = w[4 * k + 2]; v.w = w[4 * k + 3];
                *reinterpret_cast<u32x4*>(o + 4 * k) = v;
            }
        } else {
            for (unsigned k = 0; k < 5u * (n_inst - i0); ++k) o[k] = w[k];
        }
    }
}

// The same for 1-byte ids and a table of <= 256 meshes, with the access pattern of expand_mask_u8_kernel's direct
// form (a lane per instance: one 16-byte + one 4-byte store at a 20-byte lane stride, ids as one dword per lane
// redistributed with ds_bpermute), which runs at the store ceiling of the part.
__global__ __launch_bounds__(kBlock) void emit_all_u8_kernel(const vd_u64* __restrict__ mask, unsigned n_words, unsigned n_inst,
                                                             unsigned first_instance, const unsigned char* __restrict__ mesh_ids,
                                                             const VdMeshInfo* __restrict__ meshes, unsigned n_mesh,
                                                             VdDrawIndexedIndirect* __restrict__ out) {
    constexpr int kGroups = kExpandWords / kExpandGroup;
    __shared__ __attribute__((aligned(16))) unsigned s_tab[256][4];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned w0 = (blockIdx.x * kWavesPerBlock + wave) * kExpandWords;
    vd_u64 my_word = 0;                                   // lane l < 32 holds mask word w0 + l
    if (lane < (unsigned)kExpandWords && w0 + lane < n_words) my_word = mask[w0 + lane];
    unsigned ids[kGroups];
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        const unsigned i0 = 64u * (w0 + g * kExpandGroup + (lane >> 4)) + 4u * (lane & 15u);
        ids[g] = i0 < n_inst ? *reinterpret_cast<const unsigned*>(mesh_ids + i0) : 0u;   // aligned dword with >= 1 valid byte
    }
    if (threadIdx.x < n_mesh) {
        const VdMeshInfo mi = meshes[threadIdx.x];
        s_tab[threadIdx.x][0] = mi.index_count; s_tab[threadIdx.x][1] = 0u;
        s_tab[threadIdx.x][2] = mi.base_index;  s_tab[threadIdx.x][3] = (unsigned)mi.vertex_offset;
    }
    __syncthreads();
    const unsigned max_mid = n_mesh - 1u;
    const unsigned id_shift = 8u * (lane & 3u);
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
#pragma unroll
        for (int q = 0; q < kExpandGroup; ++q) {
            const int k = g * kExpandGroup + q;
            const unsigned lo = __builtin_amdgcn_readlane((unsigned)my_word, k), hi = __builtin_amdgcn_readlane((unsigned)(my_word >> 32), k);
            const vd_u64 m = ((vd_u64)hi << 32) | lo;
            const unsigned v = (unsigned)__shfl((int)ids[g], q * 16 + (int)(lane >> 2));
            const unsigned mid = min((v >> id_shift) & 0xffu, max_mid);
            const unsigned i = 64u * (w0 + (unsigned)k) + lane;
            if (i < n_inst) {
                u32x4 c = *reinterpret_cast<const u32x4*>(s_tab[mid]);
                c.y = (unsigned)(m >> lane) & 1u;
                unsigned* o = reinterpret_cast<unsigned*>(out + i);
                typedef u32x4 __attribute__((aligned(4))) u32x4_a4;
                *reinterpret_cast<u32x4_a4*>(o) = c;
                o[4] = first_instance + i;
            }
        }
    }
}

// Indices-only wire format: the set bits of a shard mask as an ascending list of global instance
// indices (4 B per survivor on the wire instead of 1 bit per instance: smaller below 1 survivor in 32), and the
// commands rebuilt from such a list.  Workgroup c owns mask chunk c as in pass 2b; no inter-workgroup dependency.
__global__ __launch_bounds__(kBlock) void mask_to_indices_kernel(const vd_u64* __restrict__ mask, unsigned n_words, unsigned first_instance,
                                                                 unsigned* __restrict__ out, const vd_u64* __restrict__ chunk_entry) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned cw0 = blockIdx.x * kChunkWords;
    const unsigned w0 = cw0 + wave * kExpandWords;
    unsigned base = (unsigned)chunk_entry[blockIdx.x];
    if (base == 0xffffffffu) return;                       // the scan gave up (mask_scan_kernel): no list
    unsigned before = 0;
    if (lane < wave * kExpandWords && cw0 + lane < n_words) before = (unsigned)__popcll(mask[cw0 + lane]);
    if (lane + 64u < wave * kExpandWords && cw0 + 64u + lane < n_words) before += (unsigned)__popcll(mask[cw0 + 64u + lane]);
    vd_u64 my_word = 0;                                   // lane l < 32 holds mask word w0 + l
    if (lane < (unsigned)kExpandWords && w0 + lane < n_words) my_word = mask[w0 + lane];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    base = __builtin_amdgcn_readfirstlane(base + before);
    const unsigned inst_lane = first_instance + 64u * w0 + lane;
#pragma unroll
    for (int k = 0; k < kExpandWords; ++k) {
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)my_word, k), hi = __builtin_amdgcn_readlane((unsigned)(my_word >> 32), k);
        const vd_u64 m = ((vd_u64)hi << 32) | lo;
        if (__builtin_amdgcn_inverse_ballot_w64(m)) out[base + vd_mbcnt(m)] = inst_lane + 64u * (unsigned)k;
        base += (unsigned)__popcll(m);
    }
}

template <typename IdT>
__global__ __launch_bounds__(kBlock) void indices_to_draws_kernel(const unsigned* __restrict__ indices, unsigned n_indices,
                                                                  const IdT* __restrict__ mesh_ids, unsigned n_total,
                                                                  const VdMeshInfo* __restrict__ meshes, unsigned n_mesh,
                                                                  VdDrawIndexedIndirect* __restrict__ out) {
    constexpr unsigned kTab = 512;
    __shared__ __attribute__((aligned(16))) unsigned s_tab[kTab][4];     // ready-made {index_count, 1, base_index, vertex_offset}
    const bool tab = n_mesh <= kTab;
    if (tab)
        for (unsigned i = threadIdx.x; i < n_mesh; i += kBlock) {
            s_tab[i][0] = meshes[i].index_count; s_tab[i][1] = 1u;
            s_tab[i][2] = meshes[i].base_index;  s_tab[i][3] = (unsigned)meshes[i].vertex_offset;
        }
    __syncthreads();
    for (unsigned k = blockIdx.x * kBlock + threadIdx.x; k < n_indices; k += gridDim.x * kBlock) {
        const unsigned i = indices[k];
        const unsigned mid = min((unsigned)mesh_ids[min(i, n_total - 1u)], n_mesh - 1u);
        u32x4 c;
        if (tab) c = *reinterpret_cast<const u32x4*>(s_tab[mid]);
        else { c.x = meshes[mid].index_count; c.y = 1u; c.z = meshes[mid].base_index; c.w = (unsigned)meshes[mid].vertex_offset; }
        unsigned* o = reinterpret_cast<unsigned*>(out + k);
        typedef u32x4 __attribute__((aligned(4))) u32x4_a4;
        *reinterpret_cast<u32x4_a4*>(o) = c;
        o[4] = i;
    }
}

// Host side of pass 2 (shared by vd_cull_compact* and vd_expand_mask_dev).
// Pass 2a (vd_expand_mask_dev, vd_mask_to_indices_dev; not vd_cull_compact*): per-chunk survivor counts -> exclusive
// offsets (ctx->expand_state) and the total (*d_out_count).
static int launch_mask_scan(VdCtx* ctx, const vd_u64* d_mask, unsigned n_words, unsigned* d_out_count, vd_u64** out_entries) {
    const unsigned n_chunks = (n_words + kChunkWords - 1) / kChunkWords;
    const size_t need = sizeof(ScanState) + (size_t)n_chunks * 8;
    if (need > ctx->expand_state_bytes || !ctx->expand_state) {
        int rc = vd_ensure(ctx, &ctx->expand_state, &ctx->expand_state_bytes, need);
        if (rc) return rc;
        // entries zeroed = tagged with epoch 0; the first launch runs in epoch 1
        VD_HIP_CHECK(ctx, hipMemsetAsync(ctx->expand_state, 0, ctx->expand_state_bytes, ctx->stream));
        VD_HIP_CHECK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reinterpret_cast<char*>(ctx->expand_state) + offsetof(ScanState, epoch)), 1, 1, ctx->stream));
    }
    ScanState* state = reinterpret_cast<ScanState*>(ctx->expand_state);
    vd_u64* entries = reinterpret_cast<vd_u64*>(reinterpret_cast<char*>(ctx->expand_state) + sizeof(ScanState));
    unsigned sblocks = (n_chunks + 15u) / 16u;                                // one wave per chunk, grid-stride beyond 2 per CU
    if (sblocks > (unsigned)ctx->num_cus * 2u) sblocks = (unsigned)ctx->num_cus * 2u;
    hipLaunchKernelGGL(mask_scan_kernel, dim3(sblocks), dim3(kScanBlock), 0, ctx->stream, d_mask, n_words, n_chunks, entries, state,
                       d_out_count);
    *out_entries = entries;
    return VD_OK;
}

// Pass 2b behind it.  d_tile_count = pass 1's survivors per tile of THIS mask as one shard (launch_mask_pass): then the
// expansion places its chunks from that table and no scan is launched.  Null (a mask that pass 1 of this call did not
// write: vd_expand_mask_dev): mask_scan_kernel first.
static int launch_expand(VdCtx* ctx, const vd_u64* d_mask, unsigned n_words, unsigned wps, unsigned shard_size,
                         unsigned n_total, unsigned first_instance, const void* d_ids, unsigned id_bytes,
                         const VdMeshInfo* d_meshes, unsigned n_mesh, VdDrawIndexedIndirect* d_out, unsigned* d_out_count,
                         const unsigned* d_tile_count = nullptr) {
    const unsigned n_chunks = (n_words + kChunkWords - 1) / kChunkWords;
    vd_u64* offsets = nullptr;
    if (!d_tile_count) {
        int rc_scan = launch_mask_scan(ctx, d_mask, n_words, d_out_count, &offsets);
        if (rc_scan) return rc_scan;
    }
    const bool one_shard = wps >= n_words;
    const bool tab = n_mesh <= 512u;
    // fast path: 1-byte ids that can be fetched as aligned dwords (every word's first instance is a multiple of 4)
    const bool fast = id_bytes == 1u && n_mesh <= 256u && (one_shard || (shard_size % 4u == 0u && wps >= (unsigned)kExpandGroup)) &&
                      (reinterpret_cast<uintptr_t>(d_ids) & 3u) == 0u;
    if (fast) {
        // up to ~250 MB of commands (the Infinity Cache absorbs them) the direct form is at the write ceiling; past
        // that the L2 merges fewer of its 4-byte pieces in time and the LDS-staged 16-byte runs win
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, d_mask, n_words, wps, shard_size, n_total, first_instance,
                               reinterpret_cast<const unsigned char*>(d_ids), d_meshes, n_mesh, d_out, offsets, d_tile_count, d_out_count);
        };
        const bool direct = n_total <= (12u << 20);
        if (d_tile_count) { if (direct) launch(expand_mask_u8_kernel<true, true>); else launch(expand_mask_u8_kernel<false, true>); }
        else { if (direct) launch(expand_mask_u8_kernel<true, false>); else launch(expand_mask_u8_kernel<false, false>); }
        return VD_OK;
    }
    vd_dispatch_id(id_bytes, [&](auto id) {
        using IdT = decltype(id);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, d_mask, n_words, wps, shard_size, n_total, first_instance,
                               reinterpret_cast<const IdT*>(d_ids), d_meshes, n_mesh, d_out, offsets, d_tile_count, d_out_count);
        };
        if (d_tile_count) { if (tab) launch(expand_mask_kernel<IdT, true, true>); else launch(expand_mask_kernel<IdT, false, true>); }
        else { if (tab) launch(expand_mask_kernel<IdT, true, false>); else launch(expand_mask_kernel<IdT, false, false>); }
    });
    return VD_OK;
}

// Zero-fill out[count..n) so the unchanged multi_draw_indexed_indirect(buf, 0, N) consumer
// (visibility.rs:188-192) sees instance_count = 0 in the tail.  The tail starts on a 4-byte boundary (count x 20 B): up to
// three single dwords bring it to a 16-byte one, the body leaves as nontemporal 16-byte stores (the `dist small` cloud pads
// 126 MB per step), the last few dwords singly again.  A count beyond n is the scan's error value (VD_SCAN_STUCK: no list was
// written): then the WHOLE buffer is zeroed, so the consumer draws nothing instead of a mix of this frame's and the last
// frame's commands.
__global__ __launch_bounds__(kBlock) void pad_tail_kernel(VdDrawIndexedIndirect* __restrict__ out,
                                                          const unsigned* __restrict__ count, unsigned n) {
    const unsigned c = *count;
    const size_t begin = (c > n ? (size_t)0 : (size_t)c) * 5u, end = (size_t)n * 5u;
    unsigned* o = reinterpret_cast<unsigned*>(out);
    if (begin >= end) return;
    const size_t gid = (size_t)blockIdx.x * kBlock + threadIdx.x, gsz = (size_t)gridDim.x * kBlock;
    const size_t mis = (reinterpret_cast<uintptr_t>(o + begin) >> 2) & 3u;            // dwords past a 16-byte boundary
    const size_t head = min(end - begin, (4u - mis) & 3u);
    const size_t quads = (end - begin - head) >> 2;
    const size_t tail_first = begin + head + quads * 4u;
    if (gid < head) o[begin + gid] = 0u;
    if (gid < end - tail_first) o[tail_first + gid] = 0u;
    u32x4* q = reinterpret_cast<u32x4*>(o + begin + head);
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (size_t i = gid; i < quads; i += gsz) __builtin_nontemporal_store(z, q + i);
}

// ------------------------------------------------------------------------------------------
// C3 alone: ordered compaction of an existing command buffer (pure function of C1's output).
// ------------------------------------------------------------------------------------------
constexpr int kCompactPerThread = 8;
constexpr int kCompactTile = kBlock * kCompactPerThread;

__global__ __launch_bounds__(kBlock) void compact_draws_kernel(const VdDrawIndexedIndirect* __restrict__ in, unsigned n,
                                                               VdDrawIndexedIndirect* __restrict__ out,
                                                               unsigned* __restrict__ out_count, vd_u64* tile_state,
                                                               vd_u64* ticket_counter, unsigned n_tiles, unsigned* fault_host) {
    __shared__ unsigned s_ticket, s_epoch, s_wave_total[kWavesPerBlock], s_tile_excl;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_ticket = vd_take_ticket(ticket_counter, n_tiles, &s_epoch);
    __syncthreads();
    const unsigned tile = s_ticket, epoch = s_epoch;
    if (tile >= n_tiles) return;                  // (the ticket word was not at {epoch, 0} when the launch began: never expected)
    if (tile == 0u && threadIdx.x == 0) { __hip_atomic_store(out_count, VD_SCAN_STUCK, VD_RLX_AGENT); __threadfence(); }   // see cull_compact_kernel
    const size_t wave_first = (size_t)tile * kCompactTile + (size_t)wave * (kWave * kCompactPerThread);
    unsigned long long masks[kCompactPerThread];
    unsigned wave_total = 0;
    const unsigned* in32 = reinterpret_cast<const unsigned*>(in);
#pragma unroll
    for (int r = 0; r < kCompactPerThread; ++r) {
        const size_t i = wave_first + (size_t)r * kWave + lane;
        const bool keep = i < n && in32[i * 5u + 1u] == 1u;
        masks[r] = __ballot(keep);
        wave_total += (unsigned)__popcll(masks[r]);
    }
    if (lane == 0) s_wave_total[wave] = wave_total;
    __syncthreads();
    if (wave == 0) {
        unsigned tile_total = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) tile_total += s_wave_total[w];
        const unsigned excl = vd_lookback(tile_state, epoch, tile, tile_total);
        if (lane == 0) {
            s_tile_excl = excl;
            if (tile == n_tiles - 1u) *out_count = vd_scan_final_count(tile_state, epoch, excl, tile_total, fault_host);
        }
    }
    __syncthreads();
    unsigned base = s_tile_excl;
    if (base == VD_SCAN_STUCK) return;
    for (unsigned w = 0; w < wave; ++w) base += s_wave_total[w];
    unsigned* out32 = reinterpret_cast<unsigned*>(out);
#pragma unroll
    for (int r = 0; r < kCompactPerThread; ++r) {
        const unsigned long long mask = masks[r];
        if ((mask >> lane) & 1ull) {
            const size_t i = wave_first + (size_t)r * kWave + lane;
            const size_t d = (size_t)(base + vd_mbcnt(mask)) * 5u;
#pragma unroll
            for (int k = 0; k < 5; ++k) out32[d + k] = in32[i * 5u + k];
        }
        base += (unsigned)__popcll(mask);
    }
}

// compute_update.wgsl:10-28 — FOUR lanes per listed instance, one matrix column (16 B) each, so a wave's load is 16
// contiguous 64-byte pieces instead of 64 pieces of 16 bytes in 64 different lines (10 M instances with
// fix_inverse: 0.685 -> 0.571 ms; transform only: 0.630 -> 0.604 ms - a read-modify-write stream over 144-byte records).  rotz * transform acts on each column
// separately; inv_transform * rotz(-angle) needs all four columns, which the quad trades through DPP.  Same operation
// order as the oracle's mat_mul_cm (products by the rotation's zeros and ones included: they matter for inf / NaN);
// (c, s) for both signs come from the host.
struct RotZ { float c_pos, s_pos, c_neg, s_neg; };
template <int SRC> __device__ __forceinline__ float quad_bcast(float v) {          // value of lane SRC of this lane's quad
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), SRC * 0x55, 0xf, 0xf, true));
}
__global__ __launch_bounds__(256) void compute_update_kernel(const unsigned* __restrict__ indices, unsigned n_indices,
                                                             VdInstance* __restrict__ inst, unsigned n_inst, RotZ rz, int fix_inverse) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x, k = t >> 2, col = t & 3u;
    const unsigned idx = k < n_indices ? indices[k] : 0xffffffffu;
    const bool live = idx < n_inst;                         // out-of-range ids are dropped; the whole quad agrees
    float4* t4 = reinterpret_cast<float4*>(inst[live ? idx : 0u].transform);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) v = t4[col];
    const float t14 = quad_bcast<3>(v.z);                   // transform[3][2]
    const bool pos = t14 > -15.0f;
    const float c = pos ? rz.c_pos : rz.c_neg, s = pos ? rz.s_pos : rz.s_neg;
    // column j of R * T, R = columns (c, s, 0, 0), (-s, c, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)
    float4 o;
    o.x = ((c * v.x + -s * v.y) + 0.0f * v.z) + 0.0f * v.w;
    o.y = ((s * v.x + c * v.y) + 0.0f * v.z) + 0.0f * v.w;
    o.z = ((0.0f * v.x + 0.0f * v.y) + 1.0f * v.z) + 0.0f * v.w;
    o.w = ((0.0f * v.x + 0.0f * v.y) + 0.0f * v.z) + 1.0f * v.w;
    if (live) t4[col] = o;
    if (fix_inverse) {
        float4* i4 = reinterpret_cast<float4*>(inst[live ? idx : 0u].inv_transform);
        float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live) w = i4[col];
        // all four columns of inv_transform: I0 .. I3
        const float4 I0 = make_float4(quad_bcast<0>(w.x), quad_bcast<0>(w.y), quad_bcast<0>(w.z), quad_bcast<0>(w.w));
        const float4 I1 = make_float4(quad_bcast<1>(w.x), quad_bcast<1>(w.y), quad_bcast<1>(w.z), quad_bcast<1>(w.w));
        const float4 I2 = make_float4(quad_bcast<2>(w.x), quad_bcast<2>(w.y), quad_bcast<2>(w.z), quad_bcast<2>(w.w));
        const float4 I3 = make_float4(quad_bcast<3>(w.x), quad_bcast<3>(w.y), quad_bcast<3>(w.z), quad_bcast<3>(w.w));
        // column `col` of rotz(-angle): (c, -s, 0, 0), (s, c, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)
        const float b0 = col == 0u ? c : (col == 1u ? s : 0.0f);
        const float b1 = col == 0u ? -s : (col == 1u ? c : 0.0f);
        const float b2 = col == 2u ? 1.0f : 0.0f, b3 = col == 3u ? 1.0f : 0.0f;
        float4 r;
        r.x = ((I0.x * b0 + I1.x * b1) + I2.x * b2) + I3.x * b3;
        r.y = ((I0.y * b0 + I1.y * b1) + I2.y * b2) + I3.y * b3;
        r.z = ((I0.z * b0 + I1.z * b1) + I2.z * b2) + I3.z * b3;
        r.w = ((I0.w * b0 + I1.w * b1) + I2.w * b2) + I3.w * b3;
        if (live) i4[col] = r;
    }
}

CullCamera make_cam(const VdCameraUniform* c) {
    CullCamera k;
    memcpy(k.view, c->view, sizeof(k.view));
    memcpy(k.frustum, c->frustum, sizeof(k.frustum));
    k.znear = c->znear;
    k.zfar = c->zfar;
    return k;
}

OccProj make_proj(const VdCameraUniform* c) {
    const float* P = c->projection;
    return OccProj{P[0], P[5], P[8], P[9], P[10], P[14]};
}

HizView make_hiz(const float* d_pyramid, unsigned width, unsigned height, const VdHizLayout& L) {
    HizView hz;
    hz.base = d_pyramid; hz.width = width; hz.height = height; hz.n_levels = L.n_levels;
    for (int k = 0; k < 17; ++k) hz.off[k] = L.level_offset[k];
    return hz;
}

// The launch geometry of pass 1 for ids of id_bytes bytes: a wave per 1024-instance tile, grid-stride beyond 3 workgroups
// per CU, and the dynamic LDS of a workgroup (slabs + the tile's ids).
struct Pass1Grid { unsigned n_mt, mb, lds_bytes; };
Pass1Grid pass1_grid(const VdCtx* ctx, unsigned n_inst, unsigned id_bytes) {
    Pass1Grid g;
    g.n_mt = (n_inst + kWave * kMaskRounds - 1) / (kWave * kMaskRounds);
    g.mb = vd_blocks(ctx, g.n_mt, kWavesPerBlock, 3u);
    g.lds_bytes = kWavesPerBlock * (kSlabBytes + kMaskRounds * kWave * id_bytes);
    return g;
}

// Pass 1 for n_views cameras over n_inst instances: the id width, the tile and launch geometry, and where its outputs lie
// in the arena - [id table | n_views masks | n_views count tables], the id table at offset 0 whatever n_views is.
// ctx->scratch keeps its older order, [mask | id table | counts] (kMaskFirst).  Not for the 240 bytes it saves: with the
// common order there, single-view pass 1 timed alone measured about 1.5 % slower (profiles/cull_host_layer.md, 4b).
// What the expansion relies on holds in both: the id table dword-aligned (16 bytes for full tiles: tiles are 1024 ids),
// every mask 256-byte aligned, every count table 16-byte aligned and padded to whole groups of 4 entries
// (tile_prefix_partial).
struct Pass1Plan : Pass1Grid {
    unsigned id_bytes, n_words;           // id width by n_mesh; mask words
    size_t ids_off, mask_off, counts_off, need;     // bytes
    size_t mask_stride, count_stride;               // words between two views' masks / entries between their count tables
};

enum Pass1Layout { kIdsFirst, kMaskFirst };     // the common order / ctx->scratch's
Pass1Plan pass1_plan(const VdCtx* ctx, unsigned n_inst, unsigned n_mesh, unsigned n_views, Pass1Layout layout) {
    Pass1Plan p;
    p.id_bytes = vd_id_bytes(n_mesh);
    static_cast<Pass1Grid&>(p) = pass1_grid(ctx, n_inst, p.id_bytes);
    p.n_words = (n_inst + 63u) / 64u;
    const size_t ids_bytes = (size_t)n_inst * p.id_bytes, mask_bytes = ((size_t)p.n_words * 8 + 255) & ~(size_t)255;
    p.mask_stride = mask_bytes / 8;
    p.count_stride = ((size_t)p.n_mt + 3) & ~(size_t)3;
    if (layout == kMaskFirst) {
        p.mask_off = 0;
        p.ids_off = n_views * mask_bytes;
        p.counts_off = (p.ids_off + ids_bytes + 15) & ~(size_t)15;
    } else {
        p.ids_off = 0;
        p.mask_off = (ids_bytes + 255) & ~(size_t)255;
        p.counts_off = p.mask_off + n_views * mask_bytes;
    }
    p.need = p.counts_off + n_views * p.count_stride * 4 + 512;
    return p;
}

// Pass 1 of every split form, in order: plan, arena, the call's timer, `launch(IdT(), plan, r)` with the id type of the
// plan's width (the callable launches ONE kernel with p.mb workgroups and p.lds_bytes of LDS, writing r.ids / r.mask /
// r.counts), the stage boundary.  The only caller of pass1_plan.
template <typename F>
VdPass1 run_pass1(VdCtx* ctx, void** arena, size_t* arena_bytes, Pass1Layout layout, unsigned n_inst, unsigned n_mesh, unsigned n_views, F&& launch) {
    const Pass1Plan p = pass1_plan(ctx, n_inst, n_mesh, n_views, layout);
    VdPass1 r = {};
    r.rc = vd_ensure(ctx, arena, arena_bytes, p.need);
    if (r.rc) return r;
    char* base = reinterpret_cast<char*>(*arena);
    r.ids = base + p.ids_off;
    r.mask = reinterpret_cast<vd_u64*>(base + p.mask_off);
    r.counts = reinterpret_cast<unsigned*>(base + p.counts_off);
    r.id_bytes = p.id_bytes; r.n_words = p.n_words; r.n_mt = p.n_mt;
    r.mask_stride = p.mask_stride; r.count_stride = p.count_stride;
    vd_time_begin(ctx);
    vd_dispatch_id(p.id_bytes, [&](auto id) { launch(id, p, r); });
    vd_time_mid(ctx);
    return r;
}

LodParams make_lod(const VdLodParams* p) { return LodParams{p->scale, p->min_distance, p->min_size}; }

void launch_pad_tail(VdCtx* ctx, VdDrawIndexedIndirect* d_out, const unsigned* d_count, unsigned n_inst) {
    hipLaunchKernelGGL(pad_tail_kernel, dim3((unsigned)ctx->num_cus * 4u), dim3(kBlock), 0, ctx->stream, d_out, d_count, n_inst);
}

// Refusals that a host-pointer form and its _dev form (or two _dev forms) word alike, each set of words once: the text
// behind the entry point's name, or null when the arguments pass.
int fail_named(VdCtx* ctx, const char* name, const char* text) {
    snprintf(ctx->err, sizeof(ctx->err), "%s: %s", name, text);
    return VD_ERR_INVALID_ARG;
}
const char kNoCamMeshes[] = "null camera/meshes or n_mesh == 0";
const char kNoCamMeshesCount[] = "null camera/meshes/count or n_mesh == 0";
const char kNoInstOut[] = "null instances/out";
const char kNoLodMeshesCount[] = "null meshes/count";
const char* hiz_refusal(const VdCameraUniform* camera, uint32_t width, uint32_t height, VdHizLayout* L) {
    if (vd_hiz_layout(width, height, L)) return "bad pyramid size";
    if (!(camera->projection[11] == -1.0f && camera->projection[15] == 0.0f))
        return "projection is not a right-handed perspective matrix (projection[11] == -1, [15] == 0)";
    return nullptr;
}
const char* views_refusal(const void* cameras, const void* meshes, uint32_t n_mesh, const void* counts, uint32_t n_views, uint64_t out_stride,
                          uint32_t n_inst) {
    if (!cameras || !meshes || n_mesh == 0 || !counts) return "null cameras/meshes/counts or n_mesh == 0";
    if (n_views == 0 || n_views > (uint32_t)VD_MAX_VIEWS) return "n_views must be 1..VD_MAX_VIEWS";
    if (out_stride < n_inst) return "out_stride < n_inst";
    return nullptr;
}

// The tail of every list form behind pass 1: the expansion of n_views masks, each placed from its own tile counts, into
// d_out + v * out_stride; the call's timer; the pads; the launch check.  first_instance != 0: a shard's list.
int finish_lists(VdCtx* ctx, const VdPass1& r, unsigned n_views, const VdMeshInfo* d_meshes, unsigned n_mesh, unsigned n_inst,
                 unsigned first_instance, VdDrawIndexedIndirect* d_out, size_t out_stride, unsigned* d_out_counts, int pad_tail) {
    for (unsigned v = 0; v < n_views; ++v) {
        int rc = launch_expand(ctx, r.mask + (size_t)v * r.mask_stride, r.n_words, r.n_words, n_inst, n_inst, first_instance, r.ids, r.id_bytes,
                               d_meshes, n_mesh, d_out + (size_t)v * out_stride, d_out_counts + v, r.counts + (size_t)v * r.count_stride);
        if (rc) return rc;
    }
    vd_time_end(ctx);
    if (pad_tail)
        for (unsigned v = 0; v < n_views; ++v) launch_pad_tail(ctx, d_out + (size_t)v * out_stride, d_out_counts + v, n_inst);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

}  // namespace

extern "C" {

int vd_cull_emit_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                     const VdInstance* d_instances, uint32_t n_inst, VdDrawIndexedIndirect* d_out) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    return vd_cull_emit_shard_dev(ctx, camera, d_meshes, n_mesh, d_instances, n_inst, 0u, d_out);
}

// Pass 1 of the split forms: instances -> one bit + a compact mesh id each, and the survivors of every 1024-instance
// tile (padded to whole 16-byte groups; the emit path ignores them), in ctx->scratch.  Declared in vd_common.hpp (hidden
// visibility): batch.hip runs the same pass.
VdPass1 launch_mask_pass(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                         const VdInstance* d_instances, uint32_t n_inst) {
    return run_pass1(ctx, &ctx->scratch, &ctx->scratch_bytes, kMaskFirst, n_inst, n_mesh, 1u, [&](auto id, const Pass1Plan& p, const VdPass1& o) {
        using IdT = decltype(id);
        hipLaunchKernelGGL(cull_mask_tiled_kernel<IdT>, dim3(p.mb), dim3(kBlock), p.lds_bytes, ctx->stream, make_cam(camera), d_meshes, n_mesh,
                           d_instances, n_inst, o.mask, reinterpret_cast<IdT*>(o.ids), o.counts, p.n_mt);
    });
}

int vd_cull_emit_shard_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                           const VdInstance* d_instances, uint32_t n_inst, uint32_t first_instance,
                           VdDrawIndexedIndirect* d_out) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !d_meshes || n_mesh == 0) return fail_named(ctx, "vd_cull_emit", kNoCamMeshes);
    if (n_inst == 0) return VD_OK;
    if (!d_instances || !d_out) return fail_named(ctx, "vd_cull_emit", kNoInstOut);
    if (ctx->option(VD_OPT_CULL_VARIANT, 0) <= 0 && n_inst >= ctx->split_min) {
        // split form, as for the compacted list: the 20-byte stores leave the read stream
        const VdPass1 r = launch_mask_pass(ctx, camera, d_meshes, n_mesh, d_instances, n_inst);
        if (r.rc) return r.rc;
        if (r.id_bytes == 1u) {
            hipLaunchKernelGGL(emit_all_u8_kernel, dim3((r.n_words + kChunkWords - 1) / kChunkWords), dim3(kBlock), 0, ctx->stream, r.mask,
                               r.n_words, n_inst, first_instance, reinterpret_cast<const unsigned char*>(r.ids), d_meshes, n_mesh, d_out);
        } else {
            const unsigned eb = vd_blocks(ctx, (n_inst + 3u) / 4u, kBlock, 16u);
            auto launch = [&](auto kernel, auto ids) {
                hipLaunchKernelGGL(kernel, dim3(eb), dim3(kBlock), 0, ctx->stream, r.mask, ids, d_meshes, n_mesh, n_inst, first_instance, d_out);
            };
            if (r.id_bytes == 2u) launch(emit_from_mask_kernel<unsigned short>, reinterpret_cast<const unsigned short*>(r.ids));
            else launch(emit_from_mask_kernel<unsigned>, reinterpret_cast<const unsigned*>(r.ids));
        }
        vd_time_end(ctx);
        VD_HIP_CHECK(ctx, hipGetLastError());
        return VD_OK;
    }
    const unsigned n_wave_tiles = (n_inst + kWave - 1) / kWave;
    const unsigned blocks = vd_blocks(ctx, n_wave_tiles, kWavesPerBlock, 4u);   // 4 x 36 KB LDS slabs per CU
    vd_time_begin(ctx);
    hipLaunchKernelGGL(emit_draws_kernel, dim3(blocks), dim3(kBlock), kWavesPerBlock * kSlabBytes, ctx->stream,
                       make_cam(camera), d_meshes, n_mesh, d_instances, n_inst, d_out, n_wave_tiles, first_instance);
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_cull_compact_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                        const VdInstance* d_instances, uint32_t n_inst, VdDrawIndexedIndirect* d_out,
                        uint32_t* d_out_count, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    return vd_cull_compact_shard_dev(ctx, camera, d_meshes, n_mesh, d_instances, n_inst, 0u, d_out, d_out_count, pad_tail);
}

int vd_cull_compact_shard_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                              const VdInstance* d_instances, uint32_t n_inst, uint32_t first_instance,
                              VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !d_meshes || n_mesh == 0 || !d_out_count) return fail_named(ctx, "vd_cull_compact", kNoCamMeshesCount);
    if (n_inst == 0) {
        VD_HIP_CHECK(ctx, hipMemsetAsync(d_out_count, 0, 4, ctx->stream));
        return VD_OK;
    }
    if (!d_instances || !d_out) return fail_named(ctx, "vd_cull_compact", kNoInstOut);
    const int variant = (int)ctx->option(VD_OPT_CULL_VARIANT, 0);
    vd_u64* ticket; vd_u64* states;
    int rc = vd_scan_check_fault(ctx);       // an EARLIER launch's scan gave up: said once, here
    if (rc) return rc;
    if (variant <= 0 && n_inst >= ctx->split_min) {
        // Split form (default for large inputs): pass 1 streams the instances and writes only one bit
        // + a compact mesh id per instance (reads run at ~6.4 TB/s when no 20-byte commands are stored
        // in the same kernel) and the survivors per tile; pass 2 expands the bits into the ordered
        // command list, placing each chunk from the tile counts: two launches, no scan kernel.  Mixing
        // the command stores into the read stream costs more than the 1-5 B/instance round trip
        // (A/B: profiles/).
        const VdPass1 r = launch_mask_pass(ctx, camera, d_meshes, n_mesh, d_instances, n_inst);
        if (r.rc) return r.rc;
        return finish_lists(ctx, r, 1u, d_meshes, n_mesh, n_inst, first_instance, d_out, 0, d_out_count, pad_tail);
    }
#define VD_LAUNCH_COMPACT(R)                                                                                     \
    do {                                                                                                         \
        const unsigned n_tiles = (n_inst + kBlock * (R) - 1) / (kBlock * (R));                                   \
        rc = vd_scan_scratch(ctx, n_tiles, &ticket, &states, true);                                              \
        if (rc) return rc;                                                                                       \
        hipLaunchKernelGGL((cull_compact_kernel<R>), dim3(n_tiles), dim3(kBlock), (compact_lds_bytes<R>()),      \
                           ctx->stream, make_cam(camera), d_meshes, n_mesh, d_instances, n_inst, d_out,          \
                           d_out_count, states, ticket, n_tiles, first_instance, vd_scan_fault_word(ctx));       \
    } while (0)
    // fused form: tile size grows with n so that ticket + two barriers + look-back amortise while
    // small inputs still spread over the chip (a 100 k-instance scene in 1024-instance tiles is 98
    // workgroups on 256 CUs; thresholds from profiles/r04_ab_cull_small.log).  variant > 0 forces a
    // tile size (tools/ab_cull.py).
    const int rounds = variant > 0 ? variant : (n_inst >= (4u << 20) ? 32 : (n_inst >= (5u << 18) ? 16 : (n_inst >= 600000u ? 8 : (n_inst >= 192000u ? 4 : (n_inst >= 48000u ? 2 : 1)))));
    switch (rounds) {
        case 1: VD_LAUNCH_COMPACT(1); break;
        case 2: VD_LAUNCH_COMPACT(2); break;
        case 4: VD_LAUNCH_COMPACT(4); break;
        case 8: VD_LAUNCH_COMPACT(8); break;
        case 16: VD_LAUNCH_COMPACT(16); break;
        default: VD_LAUNCH_COMPACT(32); break;
    }
#undef VD_LAUNCH_COMPACT
    vd_time_end(ctx);
    if (pad_tail) launch_pad_tail(ctx, d_out, d_out_count, n_inst);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// K views of one scene: ONE pass over the instances (cull_mask_views_kernel) writes K masks, K tile-count tables and the
// id table; then the unchanged expansion runs once per view, placed from that view's table.  Always the split form:
// K + 1 launches (2K + 1 with pad_tail), whatever the size.  Own arena (ctx->views_scratch), laid out
// [id table | K masks | K count tables]: the id table sits at offset 0 whatever K is, so a renderer that varies its view
// count keeps the table's rows warm, and single-view calls (ctx->scratch) in between leave it alone.  Whatever the arena
// holds - fresh, regrown, or laid out for another size - pass 1 rewrites every id row that differs from this call's.
int vd_cull_compact_views_dev(VdCtx* ctx, const VdCameraUniform* cameras, uint32_t n_views, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                              const VdInstance* d_instances, uint32_t n_inst, VdDrawIndexedIndirect* d_out, uint64_t out_stride,
                              uint32_t* d_out_counts, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (const char* no = views_refusal(cameras, d_meshes, n_mesh, d_out_counts, n_views, out_stride, n_inst)) return fail_named(ctx, "vd_cull_compact_views", no);
    if (n_inst == 0) {
        VD_HIP_CHECK(ctx, hipMemsetAsync(d_out_counts, 0, 4 * (size_t)n_views, ctx->stream));
        return VD_OK;
    }
    if (!d_instances || !d_out) return fail_named(ctx, "vd_cull_compact_views", kNoInstOut);
    if (n_views == 1) return vd_cull_compact_dev(ctx, cameras, d_meshes, n_mesh, d_instances, n_inst, d_out, d_out_counts, pad_tail);
    ViewCameras cams;
    memset(&cams, 0, sizeof(cams));
    for (uint32_t v = 0; v < n_views; ++v) cams.cam[v] = make_cam(cameras + v);
    const VdPass1 r = run_pass1(ctx, &ctx->views_scratch, &ctx->views_scratch_bytes, kIdsFirst, n_inst, n_mesh, n_views,
                                [&](auto id, const Pass1Plan& p, const VdPass1& o) {
        using IdT = decltype(id);
        hipLaunchKernelGGL(cull_mask_views_kernel<IdT>, dim3(p.mb), dim3(kBlock), p.lds_bytes, ctx->stream, cams, n_views, d_meshes, n_mesh,
                           d_instances, n_inst, o.mask, p.mask_stride, reinterpret_cast<IdT*>(o.ids), o.counts, (unsigned)p.count_stride, p.n_mt);
    });
    if (r.rc) return r.rc;
    return finish_lists(ctx, r, n_views, d_meshes, n_mesh, n_inst, 0u, d_out, out_stride, d_out_counts, pad_tail);
}

// Occlusion-culled draw lists: ONE pass over the instances (cull_mask_occ_kernel: frustum test, occlusion test against the
// pyramid and / or the visible-last-frame bits) writes the list's mask, its tile counts and the id table; then the
// unchanged expansion, placed from the tile counts.  Always the two-launch form (three with pad_tail), whatever the size:
// no scan kernel, no wait between workgroups.  Own arena (ctx->occ_scratch), laid out [id table | mask | tile counts]: the
// three entry points share the id table, so after vd_cull_early_dev the late call finds every row equal and stores none,
// and vd_cull_compact* / vd_cull_compact_views* calls in between (ctx->scratch, ctx->views_scratch) leave it alone.
enum OccMode { kOccHiz = 0, kOccEarly = 1, kOccLate = 2 };
static int cull_occ_list(VdCtx* ctx, OccMode mode, const char* name, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                         const VdInstance* d_instances, uint32_t n_inst, const float* d_pyramid, uint32_t width, uint32_t height,
                         const uint64_t* d_prev, uint64_t* d_visible_out, VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail) {
    if (!ctx) return VD_ERR_INVALID_ARG;
    const bool hiz = mode != kOccEarly, prev = mode != kOccHiz;
    char msg[256];
#define VD_OCC_FAIL(text) do { snprintf(msg, sizeof(msg), "%s: %s", name, text); VD_FAIL(ctx, VD_ERR_INVALID_ARG, msg); } while (0)
    if (!camera || !d_meshes || n_mesh == 0 || !d_out_count) VD_OCC_FAIL(kNoCamMeshesCount);
    VdHizLayout L = {};
    if (hiz) {
        if (!d_pyramid) VD_OCC_FAIL("null pyramid");
        if (const char* no = hiz_refusal(camera, width, height, &L)) VD_OCC_FAIL(no);
    }
    if (n_inst == 0) {
        VD_HIP_CHECK(ctx, hipMemsetAsync(d_out_count, 0, 4, ctx->stream));
        return VD_OK;
    }
    if (!d_instances || !d_out) VD_OCC_FAIL(kNoInstOut);
    if (prev && !d_prev) VD_OCC_FAIL("null visibility mask");
    if (mode == kOccLate && !d_visible_out) VD_OCC_FAIL("null visibility mask (out)");
#undef VD_OCC_FAIL
    OccProj proj = {};
    HizView hz = {};
    if (hiz) { proj = make_proj(camera); hz = make_hiz(d_pyramid, width, height, L); }
    const VdPass1 r = run_pass1(ctx, &ctx->occ_scratch, &ctx->occ_scratch_bytes, kIdsFirst, n_inst, n_mesh, 1u, [&](auto id, const Pass1Plan& p, const VdPass1& o) {
        using IdT = decltype(id);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(p.mb), dim3(kBlock), p.lds_bytes, ctx->stream, make_cam(camera), proj, hz, d_meshes, n_mesh, d_instances,
                               n_inst, o.mask, reinterpret_cast<const vd_u64*>(d_prev), reinterpret_cast<vd_u64*>(d_visible_out),
                               reinterpret_cast<IdT*>(o.ids), o.counts, p.n_mt);
        };
        if (mode == kOccHiz) launch(cull_mask_occ_kernel<IdT, true, false>);
        else if (mode == kOccEarly) launch(cull_mask_occ_kernel<IdT, false, true>);
        else launch(cull_mask_occ_kernel<IdT, true, true>);
    });
    if (r.rc) return r.rc;
    return finish_lists(ctx, r, 1u, d_meshes, n_mesh, n_inst, 0u, d_out, 0, d_out_count, pad_tail);
}

int vd_cull_compact_hiz_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                            const VdInstance* d_instances, uint32_t n_inst, const float* d_pyramid, uint32_t width, uint32_t height,
                            VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    return cull_occ_list(ctx, kOccHiz, "vd_cull_compact_hiz", camera, d_meshes, n_mesh, d_instances, n_inst, d_pyramid, width, height,
                         nullptr, nullptr, d_out, d_out_count, pad_tail);
}

int vd_cull_early_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                      const VdInstance* d_instances, uint32_t n_inst, const uint64_t* d_prev_visible,
                      VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    return cull_occ_list(ctx, kOccEarly, "vd_cull_early", camera, d_meshes, n_mesh, d_instances, n_inst, nullptr, 0u, 0u,
                         d_prev_visible, nullptr, d_out, d_out_count, pad_tail);
}

int vd_cull_late_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                     const VdInstance* d_instances, uint32_t n_inst, const float* d_pyramid, uint32_t width, uint32_t height,
                     const uint64_t* d_prev_visible, uint64_t* d_visible_out, VdDrawIndexedIndirect* d_out, uint32_t* d_out_count,
                     int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    return cull_occ_list(ctx, kOccLate, "vd_cull_late", camera, d_meshes, n_mesh, d_instances, n_inst, d_pyramid, width, height,
                         d_prev_visible, d_visible_out, d_out, d_out_count, pad_tail);
}

// ---- level of detail (extension: include/voidin_abi.h, "Level of detail") ----------------------------------------------
// What every LOD entry point refuses in the same words (`name` = the entry point).  Declared in vd_common.hpp (hidden
// visibility): batch.hip checks its arguments with it.
int vd_lod_check(VdCtx* ctx, const char* name, const VdCameraUniform* camera, const VdLodParams* params, const VdLodGroup* groups,
                 uint32_t n_group, uint32_t n_mesh) {
    const char* what = nullptr;
    if (!camera || !params || !groups) what = "null camera/params/groups";
    else if (n_group == 0 || n_mesh == 0) what = "n_group == 0 or n_mesh == 0";
    else if (!(isfinite(params->scale) && params->scale >= 0.0f)) what = "params.scale must be finite and >= 0";
    else if (!(isfinite(params->min_distance) && params->min_distance > 0.0f)) what = "params.min_distance must be finite and > 0";
    else if (!(isfinite(params->min_size) && params->min_size >= 0.0f)) what = "params.min_size must be finite and >= 0";
    return what ? fail_named(ctx, name, what) : VD_OK;
}

// Pass 1 of the LOD forms into ctx->scratch, laid out as launch_mask_pass lays it out (the two share the arena: whatever
// the other left in the id table - another width included - every row that differs from this call's is rewritten).  The
// id width follows the number of ROWS, n_mesh.
VdPass1 launch_lod_pass(VdCtx* ctx, const VdCameraUniform* camera, const VdLodParams* params, const VdLodGroup* d_groups, uint32_t n_group,
                        uint32_t n_mesh, const VdInstance* d_instances, uint32_t n_inst) {
    return run_pass1(ctx, &ctx->scratch, &ctx->scratch_bytes, kMaskFirst, n_inst, n_mesh, 1u, [&](auto id, const Pass1Plan& p, const VdPass1& o) {
        using IdT = decltype(id);
        hipLaunchKernelGGL((cull_mask_lod_kernel<IdT, true>), dim3(p.mb), dim3(kBlock), p.lds_bytes, ctx->stream, make_cam(camera), make_lod(params),
                           d_groups, n_group, n_mesh, d_instances, n_inst, o.mask, reinterpret_cast<IdT*>(o.ids), o.counts, p.n_mt);
    });
}

// The ids alone, of the caller's width, into the caller's table: the same kernel without a mask and without counts, on
// pass 1's launch geometry for that width.  No arena, one launch.
int vd_lod_ids_dev(VdCtx* ctx, const VdCameraUniform* camera, VdLodParams params, const VdLodGroup* d_groups, uint32_t n_group,
                   uint32_t n_mesh, const VdInstance* d_instances, uint32_t n_inst, void* d_out_ids, uint32_t id_bytes) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    int rc = vd_lod_check(ctx, "vd_lod_ids", camera, &params, d_groups, n_group, n_mesh);
    if (rc) return rc;
    if (id_bytes != 1u && id_bytes != 2u && id_bytes != 4u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_lod_ids: id_bytes must be 1, 2 or 4");
    if (id_bytes < vd_id_bytes(n_mesh)) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_lod_ids: ids of id_bytes bytes cannot hold n_mesh - 1");
    if (n_inst == 0) return VD_OK;
    if (!d_instances || !d_out_ids) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_lod_ids: null instances/ids");
    if (reinterpret_cast<uintptr_t>(d_out_ids) & 15u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_lod_ids: the id table must be 16-byte aligned");
    const Pass1Grid g = pass1_grid(ctx, n_inst, id_bytes);
    vd_time_begin(ctx);
    vd_dispatch_id(id_bytes, [&](auto id) {
        using IdT = decltype(id);
        hipLaunchKernelGGL((cull_mask_lod_kernel<IdT, false>), dim3(g.mb), dim3(kBlock), g.lds_bytes, ctx->stream, make_cam(camera), make_lod(&params),
                           d_groups, n_group, n_mesh, d_instances, n_inst, (vd_u64*)nullptr, reinterpret_cast<IdT*>(d_out_ids), (unsigned*)nullptr,
                           g.n_mt);
    });
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// Always the two-launch form (three with pad_tail), at every size, like the views and the occlusion forms: pass 1 above,
// then the unchanged expansion placed from the tile counts, reading d_meshes by the rows pass 1 chose.
int vd_cull_compact_lod_dev(VdCtx* ctx, const VdCameraUniform* camera, VdLodParams params, const VdLodGroup* d_groups, uint32_t n_group,
                            const VdMeshInfo* d_meshes, uint32_t n_mesh, const VdInstance* d_instances, uint32_t n_inst,
                            VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    int rc = vd_lod_check(ctx, "vd_cull_compact_lod", camera, &params, d_groups, n_group, n_mesh);
    if (rc) return rc;
    if (!d_meshes || !d_out_count) return fail_named(ctx, "vd_cull_compact_lod", kNoLodMeshesCount);
    if (n_inst == 0) {
        VD_HIP_CHECK(ctx, hipMemsetAsync(d_out_count, 0, 4, ctx->stream));
        return VD_OK;
    }
    if (!d_instances || !d_out) return fail_named(ctx, "vd_cull_compact_lod", kNoInstOut);
    const VdPass1 r = launch_lod_pass(ctx, camera, &params, d_groups, n_group, n_mesh, d_instances, n_inst);
    if (r.rc) return r.rc;
    return finish_lists(ctx, r, 1u, d_meshes, n_mesh, n_inst, 0u, d_out, 0, d_out_count, pad_tail);
}

int vd_cull_mask_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                     const VdInstance* d_instances, uint32_t n_inst, uint64_t* d_mask) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !d_meshes || n_mesh == 0) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_cull_mask: null camera/meshes or n_mesh == 0");
    if (n_inst == 0) return VD_OK;
    if (!d_instances || !d_mask) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_cull_mask: null instances/mask");
    const unsigned n_wave_tiles = (n_inst + kWave - 1) / kWave;
    const unsigned blocks = vd_blocks(ctx, n_wave_tiles, kWavesPerBlock, 4u);
    vd_time_begin(ctx);
    hipLaunchKernelGGL(cull_mask_kernel, dim3(blocks), dim3(kBlock), kWavesPerBlock * kSlabBytes, ctx->stream, make_cam(camera),
                       d_meshes, n_mesh, d_instances, n_inst, reinterpret_cast<vd_u64*>(d_mask), n_wave_tiles);
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_occlusion_mask_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                          const VdInstance* d_instances, uint32_t n_inst, const float* d_pyramid, uint32_t width, uint32_t height,
                          const uint64_t* d_mask_in, uint64_t* d_mask_out) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !d_meshes || n_mesh == 0 || !d_pyramid) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_occlusion_mask: null camera/meshes/pyramid or n_mesh == 0");
    VdHizLayout L;
    if (const char* no = hiz_refusal(camera, width, height, &L)) return fail_named(ctx, "vd_occlusion_mask", no);
    if (n_inst == 0) return VD_OK;
    if (!d_instances || !d_mask_in || !d_mask_out) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_occlusion_mask: null instances/masks");
    const unsigned n_wave_tiles = (n_inst + kWave - 1) / kWave;
    const unsigned blocks = vd_blocks(ctx, n_wave_tiles, kWavesPerBlock, 8u);
    vd_time_begin(ctx);
    hipLaunchKernelGGL(occlusion_mask_kernel, dim3(blocks), dim3(kBlock), kWavesPerBlock * kSlabBytes, ctx->stream, make_cam(camera),
                       make_proj(camera), make_hiz(d_pyramid, width, height, L), d_meshes, n_mesh,
                       d_instances, n_inst, reinterpret_cast<const vd_u64*>(d_mask_in), reinterpret_cast<vd_u64*>(d_mask_out), n_wave_tiles);
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_expand_mask_dev(VdCtx* ctx, const uint64_t* d_mask, uint32_t n_total, uint32_t shard_size, const void* d_mesh_ids,
                       uint32_t id_bytes, const VdMeshInfo* d_meshes, uint32_t n_mesh, VdDrawIndexedIndirect* d_out,
                       uint32_t* d_out_count) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_out_count || !d_meshes || n_mesh == 0) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_expand_mask: null count/meshes");
    if (n_total == 0) {
        VD_HIP_CHECK(ctx, hipMemsetAsync(d_out_count, 0, 4, ctx->stream));
        return VD_OK;
    }
    if (!d_mask || !d_mesh_ids || !d_out || shard_size == 0) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_expand_mask: null mask/ids/out or shard_size == 0");
    if (id_bytes != 1u && id_bytes != 2u && id_bytes != 4u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_expand_mask: id_bytes must be 1, 2 or 4");
    const unsigned n_shards = (n_total + shard_size - 1) / shard_size;
    const unsigned wps = (shard_size + 63u) / 64u;
    const unsigned n_words = n_shards * wps;   // padding bits (beyond a shard's / the scene's end) are 0 by construction
    vd_time_begin(ctx);
    int rc = launch_expand(ctx, reinterpret_cast<const vd_u64*>(d_mask), n_words, wps, shard_size, n_total, 0u, d_mesh_ids,
                           id_bytes, d_meshes, n_mesh, d_out, d_out_count);
    if (rc) return rc;
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_mask_to_indices_dev(VdCtx* ctx, const uint64_t* d_mask, uint32_t n_inst, uint32_t first_instance, uint32_t* d_out_indices,
                           uint32_t* d_out_count) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_out_count) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_mask_to_indices: null count");
    if (n_inst == 0) {
        VD_HIP_CHECK(ctx, hipMemsetAsync(d_out_count, 0, 4, ctx->stream));
        return VD_OK;
    }
    if (!d_mask || !d_out_indices) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_mask_to_indices: null mask/out");
    const unsigned n_words = (n_inst + 63u) / 64u;
    vd_time_begin(ctx);
    vd_u64* offsets;
    int rc = launch_mask_scan(ctx, reinterpret_cast<const vd_u64*>(d_mask), n_words, d_out_count, &offsets);
    if (rc) return rc;
    hipLaunchKernelGGL(mask_to_indices_kernel, dim3((n_words + kChunkWords - 1) / kChunkWords), dim3(kBlock), 0, ctx->stream,
                       reinterpret_cast<const vd_u64*>(d_mask), n_words, first_instance, d_out_indices, offsets);
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_indices_to_draws_dev(VdCtx* ctx, const uint32_t* d_indices, uint32_t n_indices, const void* d_mesh_ids, uint32_t id_bytes,
                            uint32_t n_total, const VdMeshInfo* d_meshes, uint32_t n_mesh, VdDrawIndexedIndirect* d_out) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_meshes || n_mesh == 0) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_indices_to_draws: null meshes or n_mesh == 0");
    if (n_indices == 0) return VD_OK;
    if (!d_indices || !d_mesh_ids || !d_out || n_total == 0) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_indices_to_draws: null indices/ids/out or n_total == 0");
    if (id_bytes != 1u && id_bytes != 2u && id_bytes != 4u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_indices_to_draws: id_bytes must be 1, 2 or 4");
    const unsigned blocks = vd_blocks(ctx, n_indices, kBlock, 16u);
    vd_time_begin(ctx);
    vd_dispatch_id(id_bytes, [&](auto id) {
        using IdT = decltype(id);
        hipLaunchKernelGGL(indices_to_draws_kernel<IdT>, dim3(blocks), dim3(kBlock), 0, ctx->stream, d_indices, n_indices,
                           reinterpret_cast<const IdT*>(d_mesh_ids), n_total, d_meshes, n_mesh, d_out);
    });
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_compact_draws_dev(VdCtx* ctx, const VdDrawIndexedIndirect* d_in, uint32_t n, VdDrawIndexedIndirect* d_out,
                         uint32_t* d_out_count) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_out_count) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_compact_draws: null count");
    if (n == 0) {
        VD_HIP_CHECK(ctx, hipMemsetAsync(d_out_count, 0, 4, ctx->stream));
        return VD_OK;
    }
    if (!d_in || !d_out) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_compact_draws: null in/out");
    const unsigned n_tiles = (n + kCompactTile - 1) / kCompactTile;
    vd_u64* ticket; vd_u64* states;
    int rc = vd_scan_check_fault(ctx);
    if (rc) return rc;
    rc = vd_scan_scratch(ctx, n_tiles, &ticket, &states, true);
    if (rc) return rc;
    hipLaunchKernelGGL(compact_draws_kernel, dim3(n_tiles), dim3(kBlock), 0, ctx->stream, d_in, n, d_out, d_out_count,
                       states, ticket, n_tiles, vd_scan_fault_word(ctx));
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_compute_update_dev(VdCtx* ctx, const uint32_t* d_indices, uint32_t n_indices, VdInstance* d_instances,
                          uint32_t n_instances, float time, float dt, int fix_inverse) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (n_indices == 0) return VD_OK;
    if (!d_indices || !d_instances) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_compute_update: null indices/instances");
    const float speed = 2.0f * sinf(time * 0.5f);          // compute_update.wgsl:20
    const float a_pos = (speed * 1.0f) * dt, a_neg = (speed * -1.0f) * dt;
    RotZ rz{cosf(a_pos), sinf(a_pos), cosf(a_neg), sinf(a_neg)};
    vd_time_begin(ctx);
    hipLaunchKernelGGL(compute_update_kernel, dim3((unsigned)(((size_t)n_indices * 4u + 255u) / 256u)), dim3(256), 0, ctx->stream, d_indices, n_indices,
                       d_instances, n_instances, rz, fix_inverse);
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// ---- host-pointer variants: one staged round trip through ctx-owned device buffers (declared in vd_common.hpp, hidden
// visibility: batch.hip stages the same way) --------------------------------------------------------------------------
int vd_stage(VdCtx* ctx, const VdInstance* instances, uint32_t n_inst, size_t header, VdBlob* blobs, unsigned n_blobs, size_t out_bytes,
             VdStaged* s) {
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    size_t aux_bytes = header;
    for (unsigned b = 0; b < n_blobs; ++b) {           // (dev holds the blob's offset until the arena exists)
        aux_bytes = (aux_bytes + blobs[b].align - 1) & ~(blobs[b].align - 1);
        blobs[b].dev = reinterpret_cast<void*>(aux_bytes);
        aux_bytes += blobs[b].bytes;
    }
    int rc = vd_ensure(ctx, &ctx->stage_in, &ctx->stage_in_bytes, (size_t)n_inst * sizeof(VdInstance));
    if (rc) return rc;
    rc = vd_ensure(ctx, &ctx->stage_aux, &ctx->stage_aux_bytes, aux_bytes);
    if (rc) return rc;
    rc = vd_ensure(ctx, &ctx->stage_out, &ctx->stage_out_bytes, out_bytes);
    if (rc) return rc;
    s->inst = reinterpret_cast<VdInstance*>(ctx->stage_in);
    s->counts = reinterpret_cast<uint32_t*>(ctx->stage_aux);
    s->out = reinterpret_cast<VdDrawIndexedIndirect*>(ctx->stage_out);
    if (n_inst) VD_HIP_CHECK(ctx, hipMemcpyAsync(s->inst, instances, (size_t)n_inst * sizeof(VdInstance), hipMemcpyHostToDevice, ctx->stream));
    for (unsigned b = 0; b < n_blobs; ++b) {
        blobs[b].dev = reinterpret_cast<char*>(ctx->stage_aux) + reinterpret_cast<size_t>(blobs[b].dev);
        VD_HIP_CHECK(ctx, hipMemcpyAsync(blobs[b].dev, blobs[b].host, blobs[b].bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    return VD_OK;
}

int vd_fetch_lists(VdCtx* ctx, const char* name, bool scan, const VdStaged* s, uint32_t n_views, uint32_t n_inst, int pad_tail,
                   VdDrawIndexedIndirect* out, uint64_t out_stride, uint32_t* out_counts) {
    if (out_counts) {
        VD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->host_pinned, s->counts, 4 * (size_t)n_views, hipMemcpyDeviceToHost, ctx->stream));
        VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (uint32_t v = 0; v < n_views; ++v) {
        uint32_t c = n_inst;
        if (out_counts) {
            c = ctx->host_pinned[v];
            // scan: a cross-workgroup wait of the fused form's scan timed out (vd_common.hpp) - the fault word is up and the count
            // is 0, or the launch lost its LAST workgroup and the count still holds the value the first one pre-stored,
            // VD_SCAN_STUCK.  No list was written either way; whatever state the launch left, start over.
            if (scan && (c > n_inst || ctx->host_pinned[kScanFaultWord] != 0u)) {
                ctx->host_pinned[kScanFaultWord] = 0u;
                if (ctx->scan_state) (void)hipMemsetAsync(ctx->scan_state, 0, ctx->scan_state_bytes, ctx->stream);
                snprintf(ctx->err, sizeof(ctx->err), "%s: the compaction scan gave up waiting for a workgroup", name);
                return VD_ERR_HIP;
            }
            if (c > n_inst) {
                snprintf(ctx->err, sizeof(ctx->err), "%s: the expansion wrote no count", name);
                return VD_ERR_HIP;
            }
            out_counts[v] = c;
        }
        const size_t n_copy = pad_tail ? n_inst : c;
        if (n_copy)
            VD_HIP_CHECK(ctx, hipMemcpyAsync(out + (size_t)v * out_stride, s->out + (size_t)v * n_inst, n_copy * sizeof(VdDrawIndexedIndirect),
                                             hipMemcpyDeviceToHost, ctx->stream));
    }
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VD_OK;
}

int vd_cull_emit(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* meshes, uint32_t n_mesh,
                 const VdInstance* instances, uint32_t n_inst, VdDrawIndexedIndirect* out) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !meshes || n_mesh == 0) return fail_named(ctx, "vd_cull_emit", kNoCamMeshes);
    if (n_inst == 0) return VD_OK;
    if (!instances || !out) return fail_named(ctx, "vd_cull_emit", kNoInstOut);
    VdBlob m = {meshes, (size_t)n_mesh * sizeof(VdMeshInfo), 16, nullptr};
    VdStaged s;
    int rc = vd_stage(ctx, instances, n_inst, 16, &m, 1, (size_t)n_inst * sizeof(VdDrawIndexedIndirect) + 16, &s);
    if (rc) return rc;
    rc = vd_cull_emit_dev(ctx, camera, reinterpret_cast<VdMeshInfo*>(m.dev), n_mesh, s.inst, n_inst, s.out);
    if (rc) return rc;
    return vd_fetch_lists(ctx, "vd_cull_emit", false, &s, 1u, n_inst, 0, out, 0, nullptr);   // no count: all n_inst commands
}

int vd_cull_compact(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* meshes, uint32_t n_mesh,
                    const VdInstance* instances, uint32_t n_inst, VdDrawIndexedIndirect* out, uint32_t* out_count,
                    int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !meshes || n_mesh == 0 || !out_count) return fail_named(ctx, "vd_cull_compact", kNoCamMeshesCount);
    *out_count = 0;
    if (n_inst == 0) return VD_OK;
    if (!instances || !out) return fail_named(ctx, "vd_cull_compact", kNoInstOut);
    VdBlob m = {meshes, (size_t)n_mesh * sizeof(VdMeshInfo), 16, nullptr};
    VdStaged s;
    int rc = vd_stage(ctx, instances, n_inst, 16, &m, 1, (size_t)n_inst * sizeof(VdDrawIndexedIndirect) + 16, &s);
    if (rc) return rc;
    rc = vd_cull_compact_dev(ctx, camera, reinterpret_cast<VdMeshInfo*>(m.dev), n_mesh, s.inst, n_inst, s.out, s.counts, pad_tail);
    if (rc) return rc;
    return vd_fetch_lists(ctx, "vd_cull_compact", true, &s, 1u, n_inst, pad_tail, out, 0, out_count);
}

// n_views lists of n_inst commands; a 64-byte header takes the counts.  n_views == 1 below the split size runs the fused
// form, whose scan can give up (vd_cull_compact).
int vd_cull_compact_views(VdCtx* ctx, const VdCameraUniform* cameras, uint32_t n_views, const VdMeshInfo* meshes, uint32_t n_mesh,
                          const VdInstance* instances, uint32_t n_inst, VdDrawIndexedIndirect* out, uint64_t out_stride,
                          uint32_t* out_counts, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (const char* no = views_refusal(cameras, meshes, n_mesh, out_counts, n_views, out_stride, n_inst)) return fail_named(ctx, "vd_cull_compact_views", no);
    if (n_inst > 0 && (!instances || !out)) return fail_named(ctx, "vd_cull_compact_views", kNoInstOut);
    for (uint32_t v = 0; v < n_views; ++v) out_counts[v] = 0;      // (a refused call writes nothing)
    if (n_inst == 0) return VD_OK;
    VdBlob m = {meshes, (size_t)n_mesh * sizeof(VdMeshInfo), 16, nullptr};
    VdStaged s;
    int rc = vd_stage(ctx, instances, n_inst, 64, &m, 1, (size_t)n_views * n_inst * sizeof(VdDrawIndexedIndirect) + 16, &s);
    if (rc) return rc;
    rc = vd_cull_compact_views_dev(ctx, cameras, n_views, reinterpret_cast<VdMeshInfo*>(m.dev), n_mesh, s.inst, n_inst, s.out, n_inst, s.counts, pad_tail);
    if (rc) return rc;
    return vd_fetch_lists(ctx, "vd_cull_compact_views", true, &s, n_views, n_inst, pad_tail, out, out_stride, out_counts);
}

// behind the 16-byte header: the meshes, then the pyramid on a 256-byte boundary
int vd_cull_compact_hiz(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* meshes, uint32_t n_mesh,
                        const VdInstance* instances, uint32_t n_inst, const float* pyramid, uint32_t width, uint32_t height,
                        VdDrawIndexedIndirect* out, uint32_t* out_count, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !meshes || n_mesh == 0 || !out_count || !pyramid)
        VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_cull_compact_hiz: null camera/meshes/count/pyramid or n_mesh == 0");
    VdHizLayout L;
    if (const char* no = hiz_refusal(camera, width, height, &L)) return fail_named(ctx, "vd_cull_compact_hiz", no);
    if (n_inst > 0 && (!instances || !out)) return fail_named(ctx, "vd_cull_compact_hiz", kNoInstOut);
    *out_count = 0;                                                  // (a refused call writes nothing)
    if (n_inst == 0) return VD_OK;
    VdBlob b[2] = {{meshes, (size_t)n_mesh * sizeof(VdMeshInfo), 16, nullptr}, {pyramid, (size_t)L.total_texels * sizeof(float), 256, nullptr}};
    VdStaged s;
    int rc = vd_stage(ctx, instances, n_inst, 16, b, 2, (size_t)n_inst * sizeof(VdDrawIndexedIndirect) + 16, &s);
    if (rc) return rc;
    rc = vd_cull_compact_hiz_dev(ctx, camera, reinterpret_cast<VdMeshInfo*>(b[0].dev), n_mesh, s.inst, n_inst, reinterpret_cast<float*>(b[1].dev), width,
                                 height, s.out, s.counts, pad_tail);
    if (rc) return rc;
    return vd_fetch_lists(ctx, "vd_cull_compact_hiz", false, &s, 1u, n_inst, pad_tail, out, 0, out_count);
}

// behind the 64-byte header: the groups, then the meshes.  The group table is on the host here, so it is validated (the
// _dev forms clamp instead).
int vd_cull_compact_lod(VdCtx* ctx, const VdCameraUniform* camera, VdLodParams params, const VdLodGroup* groups, uint32_t n_group,
                        const VdMeshInfo* meshes, uint32_t n_mesh, const VdInstance* instances, uint32_t n_inst,
                        VdDrawIndexedIndirect* out, uint32_t* out_count, int pad_tail) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    int rc = vd_lod_check(ctx, "vd_cull_compact_lod", camera, &params, groups, n_group, n_mesh);
    if (rc) return rc;
    if (!meshes || !out_count) return fail_named(ctx, "vd_cull_compact_lod", kNoLodMeshesCount);
    for (uint32_t g = 0; g < n_group; ++g) {
        const uint32_t nl = groups[g].n_lods;
        if (nl < 1u || nl > VD_LOD_MAX || (uint64_t)groups[g].first_row + nl > (uint64_t)n_mesh) {
            snprintf(ctx->err, sizeof(ctx->err), "vd_cull_compact_lod: group %u: n_lods must be 1..VD_LOD_MAX and first_row + n_lods <= n_mesh", g);
            return VD_ERR_INVALID_ARG;
        }
    }
    if (n_inst > 0 && (!instances || !out)) return fail_named(ctx, "vd_cull_compact_lod", kNoInstOut);
    *out_count = 0;                                                  // (a refused call writes nothing)
    if (n_inst == 0) return VD_OK;
    VdBlob b[2] = {{groups, (size_t)n_group * sizeof(VdLodGroup), 16, nullptr}, {meshes, (size_t)n_mesh * sizeof(VdMeshInfo), 16, nullptr}};
    VdStaged s;
    rc = vd_stage(ctx, instances, n_inst, 64, b, 2, (size_t)n_inst * sizeof(VdDrawIndexedIndirect) + 16, &s);
    if (rc) return rc;
    rc = vd_cull_compact_lod_dev(ctx, camera, params, reinterpret_cast<VdLodGroup*>(b[0].dev), n_group, reinterpret_cast<VdMeshInfo*>(b[1].dev), n_mesh,
                                 s.inst, n_inst, s.out, s.counts, pad_tail);
    if (rc) return rc;
    return vd_fetch_lists(ctx, "vd_cull_compact_lod", false, &s, 1u, n_inst, pad_tail, out, 0, out_count);
}

#ifdef VD_TUNING
// Tuning / test hook (libvoidin_hip_tuning.so only): the workgroup that draws ticket `tile` of the next fused
// cull + compaction launches leaves before it publishes anything - what a workgroup lost to a fault looks like to the
// others.  tile < 0 clears it.  tests/test_gpu_scan_fault.py.
int vd_debug_scan_fault(VdCtx* ctx, int tile) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx) return VD_ERR_INVALID_ARG;
    vd_u64* ticket; vd_u64* states;
    int rc = vd_scan_scratch(ctx, 1u << 16, &ticket, &states, false);   // makes sure the arena exists (and is large enough for the test's launches)
    if (rc) return rc;
    const vd_u64 v = tile < 0 ? 0ull : (vd_u64)tile + 1ull;
    VD_HIP_CHECK(ctx, hipMemcpyAsync(ticket + 1, &v, 8, hipMemcpyHostToDevice, ctx->stream));
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VD_OK;
}
#endif

}  // extern "C"
