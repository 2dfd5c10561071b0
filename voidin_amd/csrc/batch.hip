// batch.hip — instanced draw lists: one command per MESH and the survivors' instance ids grouped by mesh
// (vd_batch_mask_dev, vd_cull_batch_dev, vd_cull_batch; contract in include/voidin_abi.h, "Instanced draw lists").
//
// The reference emits one single-instance command per instance (shaders/emit_draws.wgsl:13-64) and draws them with
// multi_draw_indexed_indirect(buf, 0, N) (crates/app/src/pass/visibility.rs:188-192).  Here the survivors are sorted by
// mesh - a stable one-digit counting sort over at most VD_BATCH_MAX_MESHES keys - so that the consumer issues n_mesh
// instanced draws and we write 4 bytes per survivor instead of 20.  The sort reads what pass 1 of the two-launch step left
// in scratch (one bit + a 1- or 2-byte clamped mesh id per instance); the 144-byte instances are still read once.
//
//   batch_hist_kernel     every wave owns ONE contiguous range of mask words (64 instances each) and counts its survivors
//                         per mesh in a wave-private LDS table: row `wave` of hist[row][mesh].
//   batch_scan_kernel     per mesh, the exclusive scan down the rows (in place) and the mesh's total.
//   batch_cmds_kernel     ONE workgroup: exclusive scan of the totals over the meshes, the n_mesh commands, the count.
//   batch_scatter_kernel  every wave walks its range again with per-mesh cursors in LDS, starting at
//                         mesh_base[m] + hist[row][m]; a survivor's slot is cursor[mesh] + its rank among the same-mesh
//                         survivors of its 64-instance round.
// The rank comes from ballots over the BITS of the mesh id: after ceil(log2 n_mesh) <= 12 ballots every lane holds the
// set of lanes that share its mesh (peers); rank = popcount(peers below me), and the highest peer advances the cursor by
// popcount(peers).  A fixed 12 steps where a loop over the distinct ids of a round takes up to 64.  No atomics decide a
// position and no workgroup waits on another: the bytes are the same from run to run, and there is no "gave up" state.
//
// Occupancy: the tables are n_mesh words per wave, 16 KB at the limit of 4096 meshes; a workgroup is 4 waves = 64 KB, so two
// workgroups (8 waves) fit the 160 KB of a CU.  The grid is therefore 2 x CUs workgroups = 8 x CUs rows at most - derived
// from the CU count, not from n_inst: the count table (rows x n_mesh words, 32 MB at 4096 meshes on 256 CUs) does not grow
// with the scene, and all workgroups of a launch are resident at once.
#include "vd_common.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kRowsPerCu = 2 * kWavesPerBlock;       // two 64 KB workgroups per CU at n_mesh = 4096
constexpr int kRounds = 4;                           // rounds of a wave whose loads are in flight together
constexpr int kScanBlock = 1024;
constexpr int kScanUnroll = 8;
static_assert(VD_BATCH_MAX_MESHES * 4u * kWavesPerBlock <= 65536u, "four wave-private tables fit one workgroup's 64 KB of LDS");
static_assert(VD_BATCH_MAX_MESHES <= 4u * kScanBlock, "batch_cmds_kernel: four meshes per thread of one workgroup");

// kRounds consecutive rounds of a wave's range: the mask words (wave-uniform loads) and this lane's clamped mesh ids.
// Rounds at or behind w_end read nothing and have no survivors; bits at or behind n_inst in the last word are dropped
// (they are zero by contract; a set one must not become an id or a slot).
template <typename IdT>
__device__ __forceinline__ void load_rounds(const vd_u64* __restrict__ mask, const IdT* __restrict__ ids, unsigned w, unsigned w_end,
                                            unsigned n_inst, unsigned n_words, unsigned n_mesh, unsigned lane,
                                            vd_u64 (&word)[kRounds], unsigned (&mid)[kRounds]) {
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
        const unsigned wk = w + (unsigned)k;
        const bool in = wk < w_end;
        vd_u64 bits = in ? mask[wk] : 0ull;
        if (wk == n_words - 1u && (n_inst & 63u)) bits &= (1ull << (n_inst & 63u)) - 1ull;
        word[k] = bits;
        const size_t i = (size_t)wk * kWave + lane;
        const unsigned id = (in && i < (size_t)n_inst) ? (unsigned)ids[i] : 0u;
        mid[k] = min(id, n_mesh - 1u);
    }
}

template <typename IdT>
__global__ __launch_bounds__(kBlock) void batch_hist_kernel(const vd_u64* __restrict__ mask, const IdT* __restrict__ ids, unsigned n_inst,
                                                             unsigned n_words, unsigned n_mesh, unsigned words_per_row, unsigned rows,
                                                             unsigned* __restrict__ hist) {
    extern __shared__ unsigned s_tab[];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned row = blockIdx.x * kWavesPerBlock + wave;
    if (row >= rows) return;                          // whole waves; the kernel has no workgroup barrier
    unsigned* tab = s_tab + wave * n_mesh;
    for (unsigned m = lane; m < n_mesh; m += kWave) tab[m] = 0u;
    vd_wave_lds_sync();
    const unsigned w_begin = row * words_per_row;
    const unsigned w_end = min(n_words, w_begin + words_per_row);
    for (unsigned w = w_begin; w < w_end; w += kRounds) {
        vd_u64 word[kRounds]; unsigned mid[kRounds];
        load_rounds(mask, ids, w, w_end, n_inst, n_words, n_mesh, lane, word, mid);
#pragma unroll
        for (int k = 0; k < kRounds; ++k)
            if ((word[k] >> lane) & 1ull) __hip_atomic_fetch_add(&tab[mid[k]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);   // LDS, wave-private: a count, not a position
    }
    vd_wave_lds_sync();
    unsigned* out = hist + (size_t)row * n_mesh;
    for (unsigned m = lane; m < n_mesh; m += kWave) out[m] = tab[m];
}

// In place: hist[r][m] becomes the sum of hist[r'][m] over r' < r; totals[m] = the column's sum.  A workgroup takes `cols`
// adjacent meshes (a power of two, 16..64: loads are contiguous across meshes) and cuts the rows into kScanBlock / cols
// segments, one per thread and column: sum the segment, scan the segment sums in LDS, walk the segment again.
__global__ __launch_bounds__(kScanBlock) void batch_scan_kernel(unsigned* __restrict__ hist, unsigned rows, unsigned n_mesh, unsigned cols,
                                                                 unsigned* __restrict__ totals) {
    __shared__ unsigned s_seg[kScanBlock];
    const unsigned t = threadIdx.x, col = t & (cols - 1u), seg = t / cols, segs = kScanBlock / cols;
    const unsigned m = blockIdx.x * cols + col;
    const bool live = m < n_mesh;
    const unsigned len = (rows + segs - 1u) / segs;
    const unsigned r0 = min(rows, seg * len), r1 = min(rows, r0 + len);
    unsigned* column = hist + (live ? m : 0u);
    unsigned sum = 0u;
    for (unsigned r = r0; r < r1; r += kScanUnroll) {
        unsigned v[kScanUnroll];
#pragma unroll
        for (int k = 0; k < kScanUnroll; ++k) v[k] = (live && r + k < r1) ? column[(size_t)(r + k) * n_mesh] : 0u;
#pragma unroll
        for (int k = 0; k < kScanUnroll; ++k) sum += v[k];
    }
    s_seg[t] = sum;                                   // [seg][col]
    __syncthreads();
    if (seg == 0u) {
        unsigned run = 0u;
        for (unsigned s = 0; s < segs; ++s) {
            const unsigned v = s_seg[s * cols + col];
            s_seg[s * cols + col] = run;
            run += v;
        }
        if (live) totals[m] = run;
    }
    __syncthreads();
    unsigned run = s_seg[t];
    for (unsigned r = r0; r < r1; r += kScanUnroll) {
        unsigned v[kScanUnroll];
#pragma unroll
        for (int k = 0; k < kScanUnroll; ++k) v[k] = (live && r + k < r1) ? column[(size_t)(r + k) * n_mesh] : 0u;
#pragma unroll
        for (int k = 0; k < kScanUnroll; ++k) {
            if (live && r + k < r1) column[(size_t)(r + k) * n_mesh] = run;
            run += v[k];
        }
    }
}

// ONE workgroup, four adjacent meshes per thread: mesh_base[m] = sum of totals[k] over k < m, the n_mesh commands and the
// count.  totals == nullptr: an empty scene (all instance counts and bases 0).
__global__ __launch_bounds__(kScanBlock) void batch_cmds_kernel(const unsigned* __restrict__ totals, const VdMeshInfo* __restrict__ meshes,
                                                                 unsigned n_mesh, unsigned* __restrict__ mesh_base,
                                                                 VdDrawIndexedIndirect* __restrict__ cmds, unsigned* __restrict__ count) {
    __shared__ unsigned s_wave[kScanBlock / kWave];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    unsigned c[4], sum = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned m = t * 4u + k;
        c[k] = (totals && m < n_mesh) ? totals[m] : 0u;
        sum += c[k];
    }
    unsigned incl = sum;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned v = __shfl_up(incl, off);
        if (lane >= (unsigned)off) incl += v;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    unsigned before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < kScanBlock / kWave; ++w) {
        const unsigned v = s_wave[w];
        if ((unsigned)w < wave) before += v;
        all += v;
    }
    unsigned excl = before + incl - sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned m = t * 4u + k;
        if (m < n_mesh) {
            const VdMeshInfo mi = meshes[m];
            VdDrawIndexedIndirect d;
            d.vertex_count = mi.index_count; d.instance_count = c[k]; d.base_index = mi.base_index;
            d.vertex_offset = mi.vertex_offset; d.base_instance = excl;
            cmds[m] = d;
            if (mesh_base) mesh_base[m] = excl;
        }
        excl += c[k];
    }
    if (t == 0u) *count = all;
}

template <typename IdT>
__global__ __launch_bounds__(kBlock) void batch_scatter_kernel(const vd_u64* __restrict__ mask, const IdT* __restrict__ ids, unsigned n_inst,
                                                                unsigned n_words, unsigned n_mesh, unsigned id_bits, unsigned words_per_row,
                                                                unsigned rows, const unsigned* __restrict__ row_base,
                                                                const unsigned* __restrict__ mesh_base, unsigned* __restrict__ out_ids) {
    extern __shared__ unsigned s_tab[];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned row = blockIdx.x * kWavesPerBlock + wave;
    if (row >= rows) return;                          // whole waves; the kernel has no workgroup barrier
    unsigned* cursor = s_tab + wave * n_mesh;
    const unsigned* base = row_base + (size_t)row * n_mesh;
    for (unsigned m = lane; m < n_mesh; m += kWave) cursor[m] = mesh_base[m] + base[m];
    vd_wave_lds_sync();
    const vd_u64 below = (1ull << lane) - 1ull;
    const unsigned w_begin = row * words_per_row;
    const unsigned w_end = min(n_words, w_begin + words_per_row);
    for (unsigned w = w_begin; w < w_end; w += kRounds) {
        vd_u64 word[kRounds]; unsigned mid[kRounds];
        load_rounds(mask, ids, w, w_end, n_inst, n_words, n_mesh, lane, word, mid);
#pragma unroll
        for (int k = 0; k < kRounds; ++k) {
            const vd_u64 alive = word[k];             // == the ballot of the survivors of this round
            if (alive == 0ull) continue;              // wave-uniform
            const bool surv = (alive >> lane) & 1ull;
            const unsigned id = mid[k];
            vd_u64 peers = alive;                     // survivors that share this lane's mesh: one ballot per id bit
            for (unsigned b = 0; b < id_bits; ++b) {
                const bool bit = (id >> b) & 1u;
                const vd_u64 ones = __ballot(surv && bit);
                peers &= bit ? ones : ~ones;
            }
            const unsigned rank = (unsigned)__popcll(peers & below);
            const unsigned group = (unsigned)__popcll(peers);
            const bool last = ((peers >> lane) >> 1) == 0ull;
            const unsigned at = surv ? cursor[id] : 0u;
            const unsigned slot = at + rank;
            if (surv && slot < n_inst) out_ids[slot] = (w + (unsigned)k) * kWave + lane;   // (slot < |S| <= n_inst by construction)
            vd_wave_lds_sync();                       // every read of the round's cursors before any is advanced
            if (surv && last) cursor[id] = at + group;
            vd_wave_lds_sync();
        }
    }
}

// rows and words per row for n_words mask words: at most kRowsPerCu rows per CU, every row at least one word
struct RowPlan { unsigned rows, words_per_row; };
RowPlan plan_rows(const VdCtx* ctx, unsigned n_words) {
    const unsigned rows_max = (unsigned)ctx->num_cus * kRowsPerCu;
    RowPlan p;
    p.words_per_row = (n_words + rows_max - 1u) / rows_max;
    p.rows = (n_words + p.words_per_row - 1u) / p.words_per_row;
    return p;
}

// The four launches behind a mask and an id table (n_inst > 0, arguments checked).
int launch_batch(VdCtx* ctx, const vd_u64* d_mask, unsigned n_inst, const void* d_ids, unsigned id_bytes, const VdMeshInfo* d_meshes,
                 unsigned n_mesh, VdDrawIndexedIndirect* d_cmds, unsigned* d_out_ids, unsigned* d_count) {
    const unsigned n_words = (n_inst + 63u) / 64u;
    const RowPlan p = plan_rows(ctx, n_words);
    char* base = reinterpret_cast<char*>(ctx->batch_scratch);
    const size_t col_bytes = ((size_t)n_mesh * 4 + 255) & ~(size_t)255;
    unsigned* totals = reinterpret_cast<unsigned*>(base);
    unsigned* mesh_base = reinterpret_cast<unsigned*>(base + col_bytes);
    unsigned* hist = reinterpret_cast<unsigned*>(base + 2 * col_bytes);
    const unsigned blocks = (p.rows + kWavesPerBlock - 1u) / kWavesPerBlock;
    const unsigned lds = kWavesPerBlock * n_mesh * 4u;
    unsigned id_bits = 0u;
    while ((1u << id_bits) < n_mesh) ++id_bits;
    unsigned cols = 16u;
    while (cols < 64u && cols < n_mesh) cols *= 2u;
    vd_dispatch_id(id_bytes, [&](auto id) {
        using IdT = decltype(id);
        hipLaunchKernelGGL(batch_hist_kernel<IdT>, dim3(blocks), dim3(kBlock), lds, ctx->stream, d_mask, reinterpret_cast<const IdT*>(d_ids),
                           n_inst, n_words, n_mesh, p.words_per_row, p.rows, hist);
        hipLaunchKernelGGL(batch_scan_kernel, dim3((n_mesh + cols - 1u) / cols), dim3(kScanBlock), 0, ctx->stream, hist, p.rows, n_mesh,
                           cols, totals);
        hipLaunchKernelGGL(batch_cmds_kernel, dim3(1), dim3(kScanBlock), 0, ctx->stream, totals, d_meshes, n_mesh, mesh_base, d_cmds,
                           d_count);
        hipLaunchKernelGGL(batch_scatter_kernel<IdT>, dim3(blocks), dim3(kBlock), lds, ctx->stream, d_mask,
                           reinterpret_cast<const IdT*>(d_ids), n_inst, n_words, n_mesh, id_bits, p.words_per_row, p.rows, hist,
                           mesh_base, d_out_ids);
    });
    return VD_OK;
}

// Own arena (ctx->batch_scratch), laid out [totals | mesh bases | count table]: sized by the CU count and n_mesh, never by
// n_inst, and apart from ctx->scratch, where pass 1 keeps the single-view id table warm between calls.
int ensure_batch_scratch(VdCtx* ctx, unsigned n_mesh) {
    const size_t col_bytes = ((size_t)n_mesh * 4 + 255) & ~(size_t)255;
    const size_t need = 2 * col_bytes + (size_t)ctx->num_cus * kRowsPerCu * n_mesh * 4 + 256;
    return vd_ensure(ctx, &ctx->batch_scratch, &ctx->batch_scratch_bytes, need);
}

const char kNoCamMeshesCmdsCount[] = "vd_cull_batch: null camera/meshes/cmds/count";
const char kNoInstIds[] = "vd_cull_batch: null instances/instance-ids";
const char* const kMeshLimitMsg =
    ": n_mesh must be 1..VD_BATCH_MAX_MESHES (4096) - the limit of the one-digit counting sort (a wave-private table of n_mesh "
    "counters in LDS); a second sort digit is future work";

void launch_empty(VdCtx* ctx, const VdMeshInfo* d_meshes, unsigned n_mesh, VdDrawIndexedIndirect* d_cmds, unsigned* d_count) {
    hipLaunchKernelGGL(batch_cmds_kernel, dim3(1), dim3(kScanBlock), 0, ctx->stream, (const unsigned*)nullptr, d_meshes, n_mesh,
                       (unsigned*)nullptr, d_cmds, d_count);
}

}  // namespace

extern "C" {

int vd_batch_mask_dev(VdCtx* ctx, const uint64_t* d_mask, uint32_t n_inst, const void* d_mesh_ids, uint32_t id_bytes,
                      const VdMeshInfo* d_meshes, uint32_t n_mesh, VdDrawIndexedIndirect* d_out_cmds, uint32_t* d_out_instance_ids,
                      uint32_t* d_out_count) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!d_meshes || !d_out_cmds || !d_out_count) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_batch_mask: null meshes/cmds/count");
    if (n_mesh == 0 || n_mesh > VD_BATCH_MAX_MESHES) {
        snprintf(ctx->err, sizeof(ctx->err), "vd_batch_mask%s", kMeshLimitMsg);
        return VD_ERR_INVALID_ARG;
    }
    if (id_bytes != 1u && id_bytes != 2u && id_bytes != 4u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_batch_mask: id_bytes must be 1, 2 or 4");
    if (n_inst > 0 && (!d_mask || !d_mesh_ids || !d_out_instance_ids)) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_batch_mask: null mask/ids/instance-ids");
    if (n_inst == 0) {
        launch_empty(ctx, d_meshes, n_mesh, d_out_cmds, d_out_count);
        VD_HIP_CHECK(ctx, hipGetLastError());
        return VD_OK;
    }
    int rc = ensure_batch_scratch(ctx, n_mesh);
    if (rc) return rc;
    vd_time_begin(ctx);
    rc = launch_batch(ctx, reinterpret_cast<const vd_u64*>(d_mask), n_inst, d_mesh_ids, id_bytes, d_meshes, n_mesh, d_out_cmds,
                      d_out_instance_ids, d_out_count);
    if (rc) return rc;
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_cull_batch_dev(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                      const VdInstance* d_instances, uint32_t n_inst, VdDrawIndexedIndirect* d_out_cmds,
                      uint32_t* d_out_instance_ids, uint32_t* d_out_count) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !d_meshes || !d_out_cmds || !d_out_count) VD_FAIL(ctx, VD_ERR_INVALID_ARG, kNoCamMeshesCmdsCount);
    if (n_mesh == 0 || n_mesh > VD_BATCH_MAX_MESHES) {
        snprintf(ctx->err, sizeof(ctx->err), "vd_cull_batch%s", kMeshLimitMsg);
        return VD_ERR_INVALID_ARG;
    }
    if (n_inst > 0 && (!d_instances || !d_out_instance_ids)) VD_FAIL(ctx, VD_ERR_INVALID_ARG, kNoInstIds);
    if (n_inst == 0) {
        launch_empty(ctx, d_meshes, n_mesh, d_out_cmds, d_out_count);
        VD_HIP_CHECK(ctx, hipGetLastError());
        return VD_OK;
    }
    int rc = ensure_batch_scratch(ctx, n_mesh);
    if (rc) return rc;
    // pass 1, unchanged: bitmask + clamped mesh ids (+ tile counts, not needed here) in ctx->scratch; stage boundary behind it
    const VdPass1 r = launch_mask_pass(ctx, camera, d_meshes, n_mesh, d_instances, n_inst);
    if (r.rc) return r.rc;
    rc = launch_batch(ctx, r.mask, n_inst, r.ids, r.id_bytes, d_meshes, n_mesh, d_out_cmds, d_out_instance_ids, d_out_count);
    if (rc) return rc;
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// The instanced form over ROWS of the mesh table (include/voidin_abi.h, "Level of detail"): pass 1 of the LOD forms, whose
// id table holds the row every instance is drawn with, then the grouping above unchanged - one command per (mesh, LOD).
int vd_cull_batch_lod_dev(VdCtx* ctx, const VdCameraUniform* camera, VdLodParams params, const VdLodGroup* d_groups, uint32_t n_group,
                          const VdMeshInfo* d_meshes, uint32_t n_mesh, const VdInstance* d_instances, uint32_t n_inst,
                          VdDrawIndexedIndirect* d_out_cmds, uint32_t* d_out_instance_ids, uint32_t* d_out_count) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    int rc = vd_lod_check(ctx, "vd_cull_batch_lod", camera, &params, d_groups, n_group, n_mesh);
    if (rc) return rc;
    if (!d_meshes || !d_out_cmds || !d_out_count) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_cull_batch_lod: null meshes/cmds/count");
    if (n_mesh > VD_BATCH_MAX_MESHES) {
        snprintf(ctx->err, sizeof(ctx->err), "vd_cull_batch_lod%s", kMeshLimitMsg);
        return VD_ERR_INVALID_ARG;
    }
    if (n_inst > 0 && (!d_instances || !d_out_instance_ids)) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_cull_batch_lod: null instances/instance-ids");
    if (n_inst == 0) {
        launch_empty(ctx, d_meshes, n_mesh, d_out_cmds, d_out_count);
        VD_HIP_CHECK(ctx, hipGetLastError());
        return VD_OK;
    }
    rc = ensure_batch_scratch(ctx, n_mesh);
    if (rc) return rc;
    const VdPass1 r = launch_lod_pass(ctx, camera, &params, d_groups, n_group, n_mesh, d_instances, n_inst);
    if (r.rc) return r.rc;
    rc = launch_batch(ctx, r.mask, n_inst, r.ids, r.id_bytes, d_meshes, n_mesh, d_out_cmds, d_out_instance_ids, d_out_count);
    if (rc) return rc;
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

// host pointers: staged like vd_cull_compact (vd_stage) - instances; meshes behind a 16-byte header that takes the count;
// the n_mesh commands followed by n_inst id words, which is not the shape vd_fetch_lists copies back
int vd_cull_batch(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* meshes, uint32_t n_mesh, const VdInstance* instances,
                  uint32_t n_inst, VdDrawIndexedIndirect* out_cmds, uint32_t* out_instance_ids, uint32_t* out_count) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera || !meshes || !out_cmds || !out_count) VD_FAIL(ctx, VD_ERR_INVALID_ARG, kNoCamMeshesCmdsCount);
    if (n_mesh == 0 || n_mesh > VD_BATCH_MAX_MESHES) {
        snprintf(ctx->err, sizeof(ctx->err), "vd_cull_batch%s", kMeshLimitMsg);
        return VD_ERR_INVALID_ARG;
    }
    if (n_inst > 0 && (!instances || !out_instance_ids)) VD_FAIL(ctx, VD_ERR_INVALID_ARG, kNoInstIds);
    const size_t ids_off = ((size_t)n_mesh * sizeof(VdDrawIndexedIndirect) + 15) & ~(size_t)15;
    VdBlob m = {meshes, (size_t)n_mesh * sizeof(VdMeshInfo), 16, nullptr};
    VdStaged s;
    int rc = vd_stage(ctx, instances, n_inst, 16, &m, 1, ids_off + (size_t)n_inst * 4 + 16, &s);
    if (rc) return rc;
    uint32_t* d_count = s.counts;
    VdDrawIndexedIndirect* d_cmds = s.out;
    uint32_t* d_ids = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(s.out) + ids_off);
    rc = vd_cull_batch_dev(ctx, camera, reinterpret_cast<VdMeshInfo*>(m.dev), n_mesh, s.inst, n_inst, d_cmds, d_ids, d_count);
    if (rc) return rc;
    VD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->host_pinned, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    VD_HIP_CHECK(ctx, hipMemcpyAsync(out_cmds, d_cmds, (size_t)n_mesh * sizeof(VdDrawIndexedIndirect), hipMemcpyDeviceToHost, ctx->stream));
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t count = ctx->host_pinned[0];
    if (count > n_inst) VD_FAIL(ctx, VD_ERR_HIP, "vd_cull_batch: the device count exceeds n_inst");
    *out_count = count;
    if (count) {
        VD_HIP_CHECK(ctx, hipMemcpyAsync(out_instance_ids, d_ids, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
        VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return VD_OK;
}

}  // extern "C"
