// gbuffer.hip — the shadow pass straight from the G-buffer (include/voidin_gbuffer.h): lines 62-89 of
// src/bin/raytraced_shadows.wgsl for a whole image - which pixels receive, their world position from the depth image, their
// normal from the octahedral word - as an ordered compaction, the pass of shadow.hip over the points through its exported entry
// points, and the bits back per pixel.
//
// Tiles.  A tile is kTilePixels consecutive pixels i = y * width + x, and ONE WAVE owns it (kPerLane pixels per lane, pixel =
// tile * kTilePixels + k * 64 + lane: a wave's load of one k is 64 neighbours of a row, or the end of one and the start of the
// next).  The rank of a receiver inside its tile is ballots and popcounts of that wave alone - no LDS, no barrier, no atomic -
// and the tiles are put in order between launches, as shadow.hip does with its cells:
//
//   gbuffer_count_kernel    count[tile] = the tile's receivers; reads the material byte alone
//   gbuffer_scan_kernel     one workgroup: the exclusive scan of the counts, the total behind them and into *n_points
//   gbuffer_write_kernel    the material test again; each receiver decoded and stored at offset[tile] + rank
//   -- vd_shadow_gbuffer*_dev: the count comes back to the host, which sizes the arena; vd_shadow_pass*_dev over the points --
//   gbuffer_scatter_kernel  the material test again; the W words of every pixel: its point's, or zero.  The 64 W words of one k
//                           are one contiguous run, stored 64 words at a time (lane j of a step owns word j of the run and
//                           fetches its pixel's rank from the lane that holds it), so every store is a full 256-byte line.
//
// What a pixel IS - receiver or not, its world position, its normal - is stated once, in vd_shade.hpp, for this file and for the step
// that shades the pixels afterwards; so are the view of the three images, their checks and the scan.
#include "vd_shade.hpp"
#include "../../include/voidin_gbuffer.h"

namespace {

constexpr unsigned kPerLane = 8u;                       // pixels per lane
constexpr unsigned kTilePixels = 64u * kPerLane;        // pixels per tile = per wave
constexpr unsigned kTileWaves = 4u;                     // waves (tiles) per workgroup

// The tile skeleton: this wave's tile and which of its pixels receive.
struct GBufferTile {
    unsigned tile, lane;
    unsigned x[kPerLane], y[kPerLane];
    unsigned long long m[kPerLane];                     // m[k] = the lanes whose pixel k is a receiver
    unsigned total;                                     // receivers of the tile

    // false: this wave has no tile
    __device__ __forceinline__ bool load(const Images& im, unsigned n_tiles) {
        tile = blockIdx.x * kTileWaves + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (tile >= n_tiles) return false;
        lane = vd_lane();
        unsigned mat[kPerLane];
#pragma unroll
        for (unsigned k = 0; k < kPerLane; ++k) {
            const unsigned i = pixel(k);
            y[k] = i / im.width; x[k] = i - y[k] * im.width;
            mat[k] = i < im.n_pixels ? *im.material_at(x[k], y[k]) : VD_GBUFFER_NO_MATERIAL;
        }
        total = 0u;
#pragma unroll
        for (unsigned k = 0; k < kPerLane; ++k) { m[k] = __ballot(receives_light(mat[k])); total += (unsigned)__popcll(m[k]); }
        return true;
    }
    __device__ __forceinline__ unsigned pixel(unsigned k) const { return tile * kTilePixels + k * 64u + lane; }
    __device__ __forceinline__ bool receives(unsigned k) const { return ((m[k] >> lane) & 1ull) != 0ull; }
};

__global__ __launch_bounds__(64 * kTileWaves) void gbuffer_count_kernel(Images im, unsigned n_tiles, unsigned* __restrict__ count) {
    GBufferTile t;
    if (!t.load(im, n_tiles)) return;
    if (t.lane == 0u) count[t.tile] = t.total;
}

// offsets[i] = count[0] + ... + count[i - 1] for i in [0, n], *total = offsets[n]: ONE workgroup (vd_block_scan).
__global__ __launch_bounds__(kScanThreads) void gbuffer_scan_kernel(const unsigned* __restrict__ count, unsigned n, unsigned* __restrict__ offsets,
                                                                      unsigned* __restrict__ total_out) {
    const unsigned total = vd_block_scan(count, n, offsets);
    if (threadIdx.x == 0u) { offsets[n] = total; *total_out = total; }
}

__global__ __launch_bounds__(64 * kTileWaves) void gbuffer_write_kernel(Images im, Mat4 c2w, unsigned n_tiles, const unsigned* __restrict__ offsets,
                                                                          unsigned cap, V3* __restrict__ positions, V3* __restrict__ normals,
                                                                          unsigned* __restrict__ pixels) {
    GBufferTile t;
    if (!t.load(im, n_tiles)) return;
    if (t.total == 0u) return;
    float depth[kPerLane]; unsigned n32[kPerLane];
#pragma unroll
    for (unsigned k = 0; k < kPerLane; ++k) {           // all loads of the tile in flight before the first is used
        const bool r = t.receives(k);
        depth[k] = r ? *im.depth_at(t.x[k], t.y[k]) : 0.0f;
        n32[k] = r ? *im.normal_uv_at(t.x[k], t.y[k]) : 0u;
    }
    const float fw = (float)im.width, fh = (float)(im.n_pixels / im.width);
    unsigned at = offsets[t.tile];
#pragma unroll
    for (unsigned k = 0; k < kPerLane; ++k) {
        if (t.receives(k)) {
            const V3 p = position_from_depth(c2w, t.x[k], t.y[k], fw, fh, depth[k]);
            const V3 n = decode_octahedral(n32[k]);
            const unsigned i = at + vd_mbcnt(t.m[k]);
            if (i < cap) { positions[i] = p; normals[i] = n; pixels[i] = t.pixel(k); }      // (cap: images that change under the call cannot make it write outside the arrays)
        }
        at += (unsigned)__popcll(t.m[k]);
    }
}

// words: W.  point_occluded / point_in_range: W words for each of n_points points (never read by a tile without receivers, nor at or
// beyond n_points).  in_range may be null.
__global__ __launch_bounds__(64 * kTileWaves) void gbuffer_scatter_kernel(Images im, unsigned n_tiles, const unsigned* __restrict__ offsets, unsigned words, unsigned n_points,
                                                                            const unsigned* __restrict__ point_occluded, const unsigned* __restrict__ point_in_range,
                                                                            unsigned* __restrict__ occluded, unsigned* __restrict__ in_range) {
    GBufferTile t;
    if (!t.load(im, n_tiles)) return;
    unsigned at = offsets[t.tile];
#pragma unroll
    for (unsigned k = 0; k < kPerLane; ++k) {
        const unsigned first = t.tile * kTilePixels + k * 64u;             // the first pixel of this k: wave-uniform
        if (first >= im.n_pixels) break;
        const unsigned rank = at + vd_mbcnt(t.m[k]);
        const unsigned left = im.n_pixels - first;                         // pixels that exist from `first` on
        const unsigned run = (left < 64u ? left : 64u) * words;            // words of this k
        const size_t base = (size_t)first * words;
        for (unsigned j = t.lane; j < run + t.lane; j += 64u) {            // every lane makes every step: the shuffle needs them all
            const unsigned owner = j / words, w = j - owner * words;       // (owner < 64 whenever j < run)
            const unsigned src = owner & 63u;
            const unsigned r = (unsigned)__shfl((int)rank, (int)src);
            const bool recv = ((t.m[k] >> src) & 1ull) != 0ull && r < n_points;
            if (j < run) {
                const size_t from = (size_t)r * words + w;
                occluded[base + j] = recv ? point_occluded[from] : 0u;
                if (in_range) in_range[base + j] = recv ? point_in_range[from] : 0u;
            }
        }
        at += (unsigned)__popcll(t.m[k]);
    }
}

// The tile tables of an image in ctx->gbuffer_tables: counts, offsets (n_tiles + 1), and one word for a count nobody else takes.
struct Tables { unsigned n_tiles, blocks; unsigned* count; unsigned* offsets; unsigned* n_points; };
int gbuffer_tables(VdCtx* ctx, const Images& im, Tables* t) {
    t->n_tiles = (im.n_pixels + kTilePixels - 1u) / kTilePixels;
    t->blocks = (t->n_tiles + kTileWaves - 1u) / kTileWaves;
    return vd_carve(ctx, &ctx->gbuffer_tables, [&](Arena& a) {
        t->count = a.take<unsigned>(t->n_tiles); t->offsets = a.take<unsigned>((size_t)t->n_tiles + 1u); t->n_points = a.take<unsigned>(1);
    });
}

// count -> scan: the offsets of the tiles, the total into *d_n_points.  Enqueues only.
int gbuffer_count(VdCtx* ctx, const Images& im, const Tables& t, unsigned* d_n_points) {
    hipLaunchKernelGGL(gbuffer_count_kernel, dim3(t.blocks), dim3(64 * kTileWaves), 0, ctx->stream, im, t.n_tiles, t.count);
    hipLaunchKernelGGL(gbuffer_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, t.count, t.n_tiles, t.offsets, d_n_points);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// cap: the entries the three arrays take
int gbuffer_write(VdCtx* ctx, const Images& im, const VdCameraUniform* camera, const Tables& t, unsigned cap, float* d_pos, float* d_nor, uint32_t* d_pix) {
    Mat4 c2w;
    memcpy(c2w.m, camera->clip_to_world, sizeof(c2w.m));
    hipLaunchKernelGGL(gbuffer_write_kernel, dim3(t.blocks), dim3(64 * kTileWaves), 0, ctx->stream, im, c2w, t.n_tiles, t.offsets, cap, reinterpret_cast<V3*>(d_pos),
                       reinterpret_cast<V3*>(d_nor), d_pix);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// The count back on the host (blocks).
int gbuffer_fetch_count(VdCtx* ctx, const char* name, const unsigned* d_n_points, const Images& im, uint32_t* out) {
    VD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->host_pinned, d_n_points, 4, hipMemcpyDeviceToHost, ctx->stream));
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *out = ctx->host_pinned[0];
    if (*out > im.n_pixels) { snprintf(ctx->err, sizeof(ctx->err), "%s: the device count exceeds width * height", name); return VD_ERR_HIP; }
    return VD_OK;
}

// Both forms: exactly one of scene / accel is given (the entry points have checked that it is not null).
int shadow_gbuffer(VdCtx* ctx, const char* name, const VdTraceScene* scene, const VdTraceAccel* accel, const VdCameraUniform* camera, const VdGBuffer* gb,
                   const VdLight* d_lights, uint32_t n_lights, uint32_t max_chunk_rays, uint32_t* d_occluded, uint32_t* d_in_range, VdShadowGBufferInfo* out_info) {
    if (out_info) memset(out_info, 0, sizeof(*out_info));
    if (n_lights == 0) return VD_OK;
    if (!gb) return vd_fail_arg(ctx, name, "null pointer");
    if (gb->width == 0 || gb->height == 0) return VD_OK;
    if (!camera || !d_lights || !d_occluded) return vd_fail_arg(ctx, name, "null pointer");
    int rc = vd_check_images(ctx, name, gb);
    if (rc) return rc;
    if (n_lights > VD_SHADOW_MAX_LIGHTS) return vd_fail_arg(ctx, name, "more than VD_SHADOW_MAX_LIGHTS lights");
    if ((uint64_t)gb->width * gb->height * n_lights > kMaxPairs) return vd_fail_arg(ctx, name, "width * height * n_lights exceeds 0xf0000000");
    // what the walk refuses it refuses now, before anything is launched (the pass itself would not look at the scene of a call
    // without receivers): a call without rays checks the scene and does nothing else
    rc = scene ? vd_trace_any_dev(ctx, scene, nullptr, 0u, nullptr) : vd_trace_any_prepared_dev(ctx, accel, nullptr, 0u, nullptr);
    if (rc) return rc;

    const Images im = vd_images<const char>(gb);
    const unsigned words = (n_lights + 31u) / 32u;
    Tables t;
    if ((rc = gbuffer_tables(ctx, im, &t))) return rc;
    if ((rc = gbuffer_count(ctx, im, t, t.n_points))) return rc;
    uint32_t n_points = 0;
    if ((rc = gbuffer_fetch_count(ctx, name, t.n_points, im, &n_points))) return rc;

    float* d_pos = nullptr; float* d_nor = nullptr; uint32_t* d_pix = nullptr; unsigned* d_pocc = nullptr; unsigned* d_pinr = nullptr;
    VdShadowPassInfo pass = {};
    if (n_points) {
        rc = vd_carve(ctx, &ctx->gbuffer_points, [&](Arena& a) {
            d_pos = a.take<float>(3u * (size_t)n_points); d_nor = a.take<float>(3u * (size_t)n_points); d_pix = a.take<uint32_t>(n_points);
            d_pocc = a.take<unsigned>((size_t)n_points * words);
            d_pinr = d_in_range ? a.take<unsigned>((size_t)n_points * words) : nullptr;
        });
        if (rc) return rc;
        if ((rc = gbuffer_write(ctx, im, camera, t, n_points, d_pos, d_nor, d_pix))) return rc;
        rc = scene ? vd_shadow_pass_dev(ctx, scene, d_pos, d_nor, n_points, d_lights, n_lights, max_chunk_rays, d_pocc, d_pinr, &pass)
                   : vd_shadow_pass_prepared_dev(ctx, accel, d_pos, d_nor, n_points, d_lights, n_lights, max_chunk_rays, d_pocc, d_pinr, &pass);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(gbuffer_scatter_kernel, dim3(t.blocks), dim3(64 * kTileWaves), 0, ctx->stream, im, t.n_tiles, t.offsets, words, n_points, d_pocc, d_pinr, d_occluded,
                       d_in_range);
    VD_HIP_CHECK(ctx, hipGetLastError());
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (out_info) { out_info->n_points = n_points; out_info->n_rays = pass.n_rays; out_info->n_chunks = pass.n_chunks; out_info->words_per_point = words; }
    return VD_OK;
}

}  // namespace

extern "C" {

int vd_gbuffer_points_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdGBuffer* gb, float* d_positions, float* d_normals, uint32_t* d_pixels,
                          uint32_t* d_n_points, uint32_t* out_n_points) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    const char* name = "vd_gbuffer_points";
    if (!gb) return vd_fail_arg(ctx, name, "null pointer");
    if (gb->width == 0 || gb->height == 0) { if (out_n_points) *out_n_points = 0; return VD_OK; }
    if (!camera || !d_positions || !d_normals || !d_pixels || !d_n_points) return vd_fail_arg(ctx, name, "null pointer");
    int rc = vd_check_images(ctx, name, gb);
    if (rc) return rc;
    const Images im = vd_images<const char>(gb);
    Tables t;
    if ((rc = gbuffer_tables(ctx, im, &t))) return rc;
    if ((rc = gbuffer_count(ctx, im, t, d_n_points))) return rc;
    if ((rc = gbuffer_write(ctx, im, camera, t, im.n_pixels, d_positions, d_normals, d_pixels))) return rc;
    return out_n_points ? gbuffer_fetch_count(ctx, name, d_n_points, im, out_n_points) : VD_OK;
}

int vd_shadow_gbuffer_dev(VdCtx* ctx, const VdTraceScene* d_scene, const VdCameraUniform* camera, const VdGBuffer* gb, const VdLight* d_lights,
                          uint32_t n_lights, uint32_t max_chunk_rays, uint32_t* d_occluded, uint32_t* d_in_range, VdShadowGBufferInfo* out_info) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_scene) return vd_fail_arg(ctx, "vd_shadow_gbuffer", "null scene");
    return shadow_gbuffer(ctx, "vd_shadow_gbuffer", d_scene, nullptr, camera, gb, d_lights, n_lights, max_chunk_rays, d_occluded, d_in_range, out_info);
}

int vd_shadow_gbuffer_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdCameraUniform* camera, const VdGBuffer* gb, const VdLight* d_lights,
                                   uint32_t n_lights, uint32_t max_chunk_rays, uint32_t* d_occluded, uint32_t* d_in_range, VdShadowGBufferInfo* out_info) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!accel) return vd_fail_arg(ctx, "vd_shadow_gbuffer_prepared", "null accel");
    return shadow_gbuffer(ctx, "vd_shadow_gbuffer_prepared", nullptr, accel, camera, gb, d_lights, n_lights, max_chunk_rays, d_occluded, d_in_range, out_info);
}

}  // extern "C"
