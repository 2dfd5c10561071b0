// shadow.hip — the shadow pass for many point lights (include/voidin_shadow.h): the loop of src/bin/raytraced_shadows.wgsl:87-115
// over P points and L lights in one call.  Every (point, light) pair is tested on the device, only the pairs in range become
// rays, the any-hit walk of trace.hip answers them through its exported entry points, and one bit per pair comes back.
//
// Cells.  A cell is (light, tile of kTilePoints points), numbered light-major: cell = light * n_tiles + tile - the rays of one
// light are neighbours and converge on one point.  ONE WAVE owns a tile (kPerLane points per lane, point = tile * kTilePoints +
// k * 64 + lane), so the rank of a pair inside its cell is ballots and popcounts of that wave alone: no LDS, no barrier, and
// nothing is handed over inside a launch - no atomic anywhere.  Hand-offs happen between launches:
//
//   shadow_count_kernel   count[cell] = the cell's pairs in range (plain stores)
//   shadow_scan_kernel    one workgroup: the exclusive scan of the counts in cell order, the total behind them
//   -- the offsets come back to the host: it sizes the scratch with them and cuts the chunks --
//   per chunk (a run of whole cells of at most max_chunk_rays rays, at least one cell):
//     shadow_write_kernel the test again, each ray of the chunk at offset[cell] - offset[first cell] + rank, two 16-byte stores
//     vd_trace_any*_dev   the walk over the chunk's rays
//     shadow_fold_kernel  the test again; the lane that owns a point ORs hit[offset + rank] into the point's word in a register
//                         and stores it.  One lane owns a (point, word) in a launch, so a word whose lights two chunks share is
//                         a read-modify-write ACROSS launches; the chunk that holds the word's first light writes without reading,
//                         which is why the result does not depend on what the buffers held.
//
// The three tile kernels share one skeleton (ShadowTile) and one copy of the range test (shadow_in_range); the scan itself, the pair
// limit and the arena helper are vd_shade.hpp's, shared with the passes built on this one.
#include "vd_shade.hpp"
#include "../../include/voidin_shadow.h"

namespace {

constexpr unsigned kPerLane = 8u;                       // points per lane
constexpr unsigned kTilePoints = 64u * kPerLane;        // points per tile = per wave
constexpr unsigned kTileWaves = 4u;                     // waves (tiles) per workgroup
constexpr unsigned kDefaultChunkRays = 4u << 20;

// raytraced_shadows.wgsl:90-92: `if dist - light.radius > 0. { continue; }` - negated, so that a NaN is in range
__device__ __forceinline__ bool shadow_in_range(float dx, float dy, float dz, float radius) {
    const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
    return !((dist - radius) > 0.0f);
}

// The lights whose cell of `tile` lies in the cell range [c0, c1): [first, end)
struct LightRun { unsigned first, end; };
__device__ __forceinline__ LightRun shadow_light_run(unsigned c0, unsigned c1, unsigned tile, unsigned n_tiles) {
    LightRun r;
    r.first = c0 > tile ? (c0 - tile + n_tiles - 1u) / n_tiles : 0u;
    r.end = c1 > tile ? (c1 - tile + n_tiles - 1u) / n_tiles : 0u;
    return r;
}

// The tile skeleton: this wave's tile, its points in registers, and the loop over a run of lights.
struct ShadowTile {
    unsigned tile, lane, valid;                         // valid: bit k = point k of this lane exists
    float px[kPerLane], py[kPerLane], pz[kPerLane];

    // false: this wave has no tile among [tile0, tile_end)
    __device__ __forceinline__ bool load(const float* __restrict__ pos, unsigned n_points, unsigned tile0, unsigned tile_end) {
        tile = tile0 + blockIdx.x * kTileWaves + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (tile >= tile_end) return false;
        lane = vd_lane();
        valid = 0u;
#pragma unroll
        for (unsigned k = 0; k < kPerLane; ++k) {
            const unsigned p = point(k);
            const bool ok = p < n_points;
            px[k] = ok ? pos[3u * (size_t)p] : 0.0f; py[k] = ok ? pos[3u * (size_t)p + 1u] : 0.0f; pz[k] = ok ? pos[3u * (size_t)p + 2u] : 0.0f;
            valid |= ok ? 1u << k : 0u;
        }
        return true;
    }
    __device__ __forceinline__ unsigned point(unsigned k) const { return tile * kTilePoints + k * 64u + lane; }

    // f(light index, the light, m): m[k] = the lanes whose point k is in range of it
    template <typename F>
    __device__ __forceinline__ void for_lights(const VdLight* __restrict__ lights, LightRun run, F&& f) const {
        for (unsigned l = run.first; l < run.end; ++l) {
            const VdLight L = lights[l];                // uniform across the wave: scalar loads
            unsigned long long m[kPerLane];
#pragma unroll
            for (unsigned k = 0; k < kPerLane; ++k)
                m[k] = __ballot(((valid >> k) & 1u) != 0u && shadow_in_range(L.position[0] - px[k], L.position[1] - py[k], L.position[2] - pz[k], L.radius));
            f(l, L, m);
        }
    }
};

__global__ __launch_bounds__(64 * kTileWaves) void shadow_count_kernel(const float* __restrict__ pos, unsigned n_points, const VdLight* __restrict__ lights,
                                                                         unsigned n_lights, unsigned n_tiles, unsigned* __restrict__ count) {
    ShadowTile t;
    if (!t.load(pos, n_points, 0u, n_tiles)) return;
    t.for_lights(lights, LightRun{0u, n_lights}, [&](unsigned l, const VdLight&, const unsigned long long (&m)[kPerLane]) {
        unsigned c = 0u;
#pragma unroll
        for (unsigned k = 0; k < kPerLane; ++k) c += (unsigned)__popcll(m[k]);
        if (t.lane == 0u) count[(size_t)l * n_tiles + t.tile] = c;
    });
}

// offsets[i] = count[0] + ... + count[i - 1] for i in [0, n]: ONE workgroup (vd_block_scan).
__global__ __launch_bounds__(kScanThreads) void shadow_scan_kernel(const unsigned* __restrict__ count, unsigned n, unsigned* __restrict__ offsets) {
    const unsigned total = vd_block_scan(count, n, offsets);
    if (threadIdx.x == 0u) offsets[n] = total;
}

// What the per-chunk kernels are told: the chunk's cells [c0, c1), the ray offset of c0, and the tiles those cells touch.
struct ShadowChunk { unsigned c0, c1, base, n, tile0, tile_end; };      // n: the chunk's rays - no index at or above it is touched

__global__ __launch_bounds__(64 * kTileWaves) void shadow_write_kernel(const float* __restrict__ pos, const float* __restrict__ nor, unsigned n_points,
                                                                         const VdLight* __restrict__ lights, unsigned n_tiles, const unsigned* __restrict__ offsets,
                                                                         ShadowChunk ch, float t_max, float4* __restrict__ rays) {
    ShadowTile t;
    if (!t.load(pos, n_points, ch.tile0, ch.tile_end)) return;
    float ex[kPerLane], ey[kPerLane], ez[kPerLane];     // the origins: vd_shadow_rays_dev's pos + nor * 0.0001
#pragma unroll
    for (unsigned k = 0; k < kPerLane; ++k) {
        const unsigned p = t.point(k);
        const bool ok = ((t.valid >> k) & 1u) != 0u;
        ex[k] = t.px[k] + (ok ? nor[3u * (size_t)p] : 0.0f) * 0.0001f;
        ey[k] = t.py[k] + (ok ? nor[3u * (size_t)p + 1u] : 0.0f) * 0.0001f;
        ez[k] = t.pz[k] + (ok ? nor[3u * (size_t)p + 2u] : 0.0f) * 0.0001f;
    }
    t.for_lights(lights, shadow_light_run(ch.c0, ch.c1, t.tile, n_tiles), [&](unsigned l, const VdLight& L, const unsigned long long (&m)[kPerLane]) {
        unsigned at = offsets[(size_t)l * n_tiles + t.tile] - ch.base;
#pragma unroll
        for (unsigned k = 0; k < kPerLane; ++k) {
            const unsigned i = at + vd_mbcnt(m[k]);
            if (((m[k] >> t.lane) & 1ull) && i < ch.n) {
                float4* r = rays + 2u * (size_t)i;
                r[0] = make_float4(ex[k], ey[k], ez[k], 0.0f);
                r[1] = make_float4(L.position[0] - t.px[k], L.position[1] - t.py[k], L.position[2] - t.pz[k], t_max);
            }
            at += (unsigned)__popcll(m[k]);
        }
    });
}

__global__ __launch_bounds__(64 * kTileWaves) void shadow_fold_kernel(const float* __restrict__ pos, unsigned n_points, const VdLight* __restrict__ lights,
                                                                        unsigned n_tiles, const unsigned* __restrict__ offsets, ShadowChunk ch,
                                                                        const unsigned* __restrict__ hit, unsigned words, unsigned* occluded, unsigned* in_range) {
    ShadowTile t;
    if (!t.load(pos, n_points, ch.tile0, ch.tile_end)) return;
    const LightRun run = shadow_light_run(ch.c0, ch.c1, t.tile, n_tiles);
    unsigned occ[kPerLane], inr[kPerLane];
#pragma unroll
    for (unsigned k = 0; k < kPerLane; ++k) occ[k] = inr[k] = 0u;
    t.for_lights(lights, run, [&](unsigned l, const VdLight&, const unsigned long long (&m)[kPerLane]) {
        unsigned at = offsets[(size_t)l * n_tiles + t.tile] - ch.base;
        const unsigned bit = 1u << (l & 31u);
#pragma unroll
        for (unsigned k = 0; k < kPerLane; ++k) {
            const unsigned i = at + vd_mbcnt(m[k]);
            if (((m[k] >> t.lane) & 1ull) && i < ch.n) {
                inr[k] |= bit;
                occ[k] |= hit[i] != 0u ? bit : 0u;
            }
            at += (unsigned)__popcll(m[k]);
        }
        if ((l & 31u) != 31u && l + 1u != run.end) return;
        // the word is complete as far as this launch goes; an earlier chunk wrote its lower lights unless its first light is ours
        const unsigned w = l >> 5;
        const bool fresh = w * 32u >= run.first;
#pragma unroll
        for (unsigned k = 0; k < kPerLane; ++k) {
            if ((t.valid >> k) & 1u) {
                const size_t a = (size_t)t.point(k) * words + w;
                occluded[a] = (fresh ? 0u : occluded[a]) | occ[k];
                if (in_range) in_range[a] = (fresh ? 0u : in_range[a]) | inr[k];
            }
            occ[k] = inr[k] = 0u;
        }
    });
}

// Both forms: exactly one of scene / accel is given (the entry points have checked that it is not null).
int shadow_pass(VdCtx* ctx, const char* name, const VdTraceScene* scene, const VdTraceAccel* accel, const float* d_pos, const float* d_nor, uint32_t n_points,
                const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays, uint32_t* d_occluded, uint32_t* d_in_range, VdShadowPassInfo* out_info) {
    if (out_info) memset(out_info, 0, sizeof(*out_info));
    if (n_points == 0 || n_lights == 0) return VD_OK;
    if (!d_pos || !d_nor || !d_lights || !d_occluded) return vd_fail_arg(ctx, name, "null pointer");
    if (n_lights > VD_SHADOW_MAX_LIGHTS) return vd_fail_arg(ctx, name, "more than VD_SHADOW_MAX_LIGHTS lights");
    if ((uint64_t)n_points * n_lights > kMaxPairs) return vd_fail_arg(ctx, name, "n_points * n_lights exceeds 0xf0000000");
    // what the walk refuses it refuses now, before anything is launched: a call without rays checks the scene and does nothing else
    int rc = scene ? vd_trace_any_dev(ctx, scene, nullptr, 0u, nullptr) : vd_trace_any_prepared_dev(ctx, accel, nullptr, 0u, nullptr);
    if (rc) return rc;
    const unsigned words = (n_lights + 31u) / 32u;
    const unsigned n_tiles = (n_points + kTilePoints - 1u) / kTilePoints;
    const unsigned n_cells = n_tiles * n_lights;                       // <= kMaxPairs / 512 + 1024
    const unsigned max_rays = max_chunk_rays ? max_chunk_rays : kDefaultChunkRays;

    // counts and offsets; the offsets come back through the pinned staging
    unsigned* d_count = nullptr; unsigned* d_off = nullptr;
    size_t tables = 0;                                                 // where the tables end
    rc = vd_carve(ctx, &ctx->shadow, [&](Arena& a) { d_count = a.take<unsigned>(n_cells); d_off = a.take<unsigned>((size_t)n_cells + 1u); tables = a.off; });
    if (rc || (rc = vd_ensure_host(ctx, ((size_t)n_cells + 1u) * 4u))) return rc;
    const unsigned tile_blocks = (n_tiles + kTileWaves - 1u) / kTileWaves;
    hipLaunchKernelGGL(shadow_count_kernel, dim3(tile_blocks), dim3(64 * kTileWaves), 0, ctx->stream, d_pos, n_points, d_lights, n_lights, n_tiles, d_count);
    hipLaunchKernelGGL(shadow_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d_count, n_cells, d_off);
    VD_HIP_CHECK(ctx, hipGetLastError());
    unsigned* off = static_cast<unsigned*>(ctx->host_stage);
    VD_HIP_CHECK(ctx, hipMemcpyAsync(off, d_off, ((size_t)n_cells + 1u) * 4u, hipMemcpyDeviceToHost, ctx->stream));
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));

    // the chunks: greedy runs of whole cells; the largest one sizes the scratch
    auto chunk_end = [&](unsigned c0) {
        unsigned c1 = c0 + 1u;
        while (c1 < n_cells && off[c1 + 1u] - off[c0] <= max_rays) ++c1;
        return c1;
    };
    unsigned largest = 0u, n_chunks = 0u;
    for (unsigned c0 = 0; c0 < n_cells; ++n_chunks) {
        const unsigned c1 = chunk_end(c0);
        if (off[c1] - off[c0] > largest) largest = off[c1] - off[c0];
        c0 = c1;
    }
    VdRay* d_rays = nullptr; unsigned* d_hit = nullptr;
    if (largest) {
        Arena a{static_cast<char*>(ctx->shadow.state), tables};
        a.take<VdRay>(largest); a.take<unsigned>(largest);
        // growing moves the tables: the stream is idle and the host holds the offsets, so the counts may go and the offsets are put back
        if (a.off > ctx->shadow.bytes) {
            if ((rc = vd_ensure(ctx, &ctx->shadow.state, &ctx->shadow.bytes, a.off))) return rc;
            a = Arena{static_cast<char*>(ctx->shadow.state), 0};
            d_count = a.take<unsigned>(n_cells);
            d_off = a.take<unsigned>((size_t)n_cells + 1u);
            VD_HIP_CHECK(ctx, hipMemcpyAsync(d_off, off, ((size_t)n_cells + 1u) * 4u, hipMemcpyHostToDevice, ctx->stream));
        } else {
            a = Arena{static_cast<char*>(ctx->shadow.state), tables};
        }
        d_rays = a.take<VdRay>(largest); d_hit = a.take<unsigned>(largest);
    }
    const float t_max = ctx->option(VD_OPT_TRACE_RAY_RANGE, 0) == 1 ? 1.0f : 0.0f;      // as vd_shadow_rays_dev sets the pad words
    const unsigned total = off[n_cells];
    for (unsigned c0 = 0; c0 < n_cells;) {
        // (`off` stays valid across the walk: of the library only the BLAS builders size the pinned staging)
        const unsigned c1 = chunk_end(c0), n = off[c1] - off[c0];
        ShadowChunk ch{c0, c1, off[c0], n, 0u, n_tiles};
        if (c0 / n_tiles == (c1 - 1u) / n_tiles) { ch.tile0 = c0 % n_tiles; ch.tile_end = (c1 - 1u) % n_tiles + 1u; }      // within one light: its tiles only
        const unsigned blocks = (ch.tile_end - ch.tile0 + kTileWaves - 1u) / kTileWaves;
        if (n) {
            hipLaunchKernelGGL(shadow_write_kernel, dim3(blocks), dim3(64 * kTileWaves), 0, ctx->stream, d_pos, d_nor, n_points, d_lights, n_tiles, d_off, ch,
                               t_max, reinterpret_cast<float4*>(d_rays));
            VD_HIP_CHECK(ctx, hipGetLastError());
            rc = scene ? vd_trace_any_dev(ctx, scene, d_rays, n, d_hit) : vd_trace_any_prepared_dev(ctx, accel, d_rays, n, d_hit);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(shadow_fold_kernel, dim3(blocks), dim3(64 * kTileWaves), 0, ctx->stream, d_pos, n_points, d_lights, n_tiles, d_off, ch, d_hit, words,
                           d_occluded, d_in_range);
        VD_HIP_CHECK(ctx, hipGetLastError());
        c0 = c1;
    }
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (out_info) { out_info->n_rays = total; out_info->n_chunks = n_chunks; out_info->words_per_point = words; }
    return VD_OK;
}

}  // namespace

extern "C" {

int vd_shadow_pass_dev(VdCtx* ctx, const VdTraceScene* d_scene, const float* d_positions, const float* d_normals, uint32_t n_points, const VdLight* d_lights,
                       uint32_t n_lights, uint32_t max_chunk_rays, uint32_t* d_occluded, uint32_t* d_in_range, VdShadowPassInfo* out_info) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_scene) return vd_fail_arg(ctx, "vd_shadow_pass", "null scene");
    return shadow_pass(ctx, "vd_shadow_pass", d_scene, nullptr, d_positions, d_normals, n_points, d_lights, n_lights, max_chunk_rays, d_occluded, d_in_range,
                       out_info);
}

int vd_shadow_pass_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const float* d_positions, const float* d_normals, uint32_t n_points,
                                const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays, uint32_t* d_occluded, uint32_t* d_in_range,
                                VdShadowPassInfo* out_info) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!accel) return vd_fail_arg(ctx, "vd_shadow_pass_prepared", "null accel");
    return shadow_pass(ctx, "vd_shadow_pass_prepared", nullptr, accel, d_positions, d_normals, n_points, d_lights, n_lights, max_chunk_rays, d_occluded,
                       d_in_range, out_info);
}

}  // extern "C"
