// vd_common.hpp — shared host/device plumbing of libvoidin_hip.so (gfx950 only).
//
// Strict fp32 everywhere: the library is compiled with -ffp-contract=off so that a*b+c is
// never fused (rustc / the reference never contract), with hipcc's default
// correctly-rounded f32 divide/sqrt and f32 denormals kept.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/voidin_abi.h"
#include "vd_plan.hpp"

// TLAS refit: epoch-tagged {parent, sibling} links + arrival words for ONE instance count at a time (tlas.hip: tlas_refit_impl).
// The context has one for vd_tlas_refit*; a VdTraceAccel with a private top level has its own (vd_trace_accel_refit_dev), so
// that the caller's own refits at another n do not start either arena over.
struct VdRefitArena {
    void* state = nullptr; size_t bytes = 0;
    unsigned epoch = 0;                 // tag of the last refit launch (0 = the arena is freshly zeroed)
    unsigned n = 0;                     // instance count the arena's layout was last used with
};

// A self-freeing grow-only device buffer (sized through vd_carve below).  It frees itself where ctx.hip deletes the context
// (vd_ctx_destroy has drained the stream and made the context's device current by then).
struct VdDeviceBuffer {
    void* state = nullptr; size_t bytes = 0;
    VdDeviceBuffer() = default;
    ~VdDeviceBuffer() { if (state) (void)hipFree(state); }
    VdDeviceBuffer(const VdDeviceBuffer&) = delete;
    VdDeviceBuffer& operator=(const VdDeviceBuffer&) = delete;
};

struct VdCtx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;      // stream in use (own or caller's)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_mid = nullptr, ev_aux = nullptr;
    bool timed_mid = false;
    bool timed = false;
    bool timing_enabled = false;        // event pairs around kernels cost a few us of GPU idle each: opt-in
    char err[512] = {0};
    int num_cus = 256;
    unsigned split_min = 2u << 20;      // inputs of at least this many instances run the split form of the cull
                                        // (VD_OPT_CULL_SPLIT_MIN): below, the fused single launch is faster (tools/ab_split_min.py:
                                        // 1 Mi 39 vs 47 us, 2 Mi 65 vs 65, 3 Mi 97 vs 93, 10 M 312 vs 256)
    long long opt[VD_OPT_COUNT_];       // vd_ctx_set_option: -1 = default (set in vd_ctx_create)
    long long option(int o, long long dflt) const { return opt[o] < 0 ? dflt : opt[o]; }

    // grow-only device scratch arenas
    void* scratch = nullptr;     size_t scratch_bytes = 0;     // general purpose
    void* views_scratch = nullptr; size_t views_scratch_bytes = 0;   // vd_cull_compact_views*: id table, K masks, K tile-count tables
    void* occ_scratch = nullptr; size_t occ_scratch_bytes = 0;       // vd_cull_compact_hiz* / vd_cull_early_dev / vd_cull_late_dev: id table, mask, tile counts
    void* batch_scratch = nullptr; size_t batch_scratch_bytes = 0;   // vd_cull_batch* / vd_batch_mask_dev: mesh totals, mesh bases, the [wave][mesh] count table
    void* scan_state = nullptr;  size_t scan_state_bytes = 0;  // look-back granules + ticket word (epoch-tagged)
    void* expand_state = nullptr; size_t expand_state_bytes = 0;  // mask_scan_kernel: done counter + chunk offsets
    void* trace_ovf = nullptr;   size_t trace_ovf_bytes = 0;      // traversal: one bit per ray of the call = "its 128-entry stack overflowed"
    bool trace_ovf_dirty = false;                                 // a call left early (error) and may have left bits set
    void* trace_deep = nullptr;  size_t trace_deep_bytes = 0;     // traversal, second pass over those rays: their list + stack entries beyond 128 (allocated when first needed)
    void* trace_wide = nullptr;  size_t trace_wide_bytes = 0;     // vd_trace_wide*: the per-call records of a wide top level (64 B per node), mesh records, triangles, fan-out
    void* lbvh_state = nullptr;  size_t lbvh_state_bytes = 0;     // vd_tlas_build_lbvh*: leaf boxes, codes, the sort's tables, parent links, arrival words
    void* blas_lbvh_state = nullptr; size_t blas_lbvh_state_bytes = 0;   // vd_bvh_build_lbvh*: triangle boxes, the index copy, the sort's work memory, the radix tree
    VdDeviceBuffer shadow;                                        // vd_shadow_pass*: cell counts and offsets, then the rays and hit flags of one chunk (not `scratch`: the walk's arena)
    VdDeviceBuffer gbuffer_tables, gbuffer_points;                // vd_gbuffer_points_dev / vd_shadow_gbuffer*: tile counts and offsets | points, normals, pixel ids, per-point words.
                                                                  // Two buffers, so that sizing the second by the count the first gave never moves the tables
    VdDeviceBuffer gbuffer_trace;                                 // vd_gbuffer_trace*: the rays and hit records of one image (gbuffer_trace.hip)
    VdDeviceBuffer lighting;                                      // vd_shade_gbuffer*: the two per-pixel bit arrays between the pass and the lighting step (lighting.hip)
    VdRefitArena refit;                                           // vd_tlas_refit*: links + arrival words
    const void* fan_tlas = nullptr; unsigned fan_idle_calls = 0;  // traversal fan-out: top level of the last call that tried it, calls left to run without it
    unsigned fan_nodes = 0, fan_inst = 0;                         // ... and its node / instance counts: the verdict is about THAT scene
    void fan_forget(const void* tlas) { if (tlas == fan_tlas) { fan_tlas = nullptr; fan_idle_calls = 0; } }   // the top level at this address was rebuilt / refitted / released
    // A call that would fan out asks first: true = the last call over this very top level made too few jobs, run as one launch
    // (one of the 15 such calls is used up).  fan_remember: what a call that did fan out found.
    bool fan_rest(const void* tlas, unsigned nodes, unsigned inst) { const bool rest = tlas == fan_tlas && nodes == fan_nodes && inst == fan_inst && fan_idle_calls != 0u; if (rest) --fan_idle_calls; return rest; }
    void fan_remember(const void* tlas, unsigned nodes, unsigned inst, bool few_jobs) { fan_tlas = tlas; fan_nodes = nodes; fan_inst = inst; fan_idle_calls = few_jobs ? 15u : 0u; }
    unsigned long long scan_launches = 0;
    void* dbg_ptr = nullptr; unsigned dbg_count = 0; void* dbg_ptr2 = nullptr;   // tuning hooks
#ifdef VD_TUNING
    bool dbg_fan_wide = false; size_t dbg_fan_at = 0;                                // vd_debug_trace_fan: the last trace call's arena (scratch / trace_wide) and where its fan-out block lay
    unsigned dbg_fan_phases = 0, dbg_fan_waves = 0, dbg_fan_cap = 0;                 // ... its launches (0: no trace call yet), grid and job slots
#endif
    void* stage_in = nullptr;    size_t stage_in_bytes = 0;    // host-pointer API staging
    void* stage_out = nullptr;   size_t stage_out_bytes = 0;
    void* stage_aux = nullptr;   size_t stage_aux_bytes = 0;
    uint32_t* host_pinned = nullptr;                           // 64 u32 of pinned host memory
    unsigned* fault_dev = nullptr;                             // device address of host_pinned[kScanFaultWord] (vd_scan_check_fault)
    void* host_stage = nullptr;  size_t host_stage_bytes = 0;  // grow-only pinned staging (BLAS top tree; vd_shadow_pass*: the cell offsets)
    void* lvl_pinned = nullptr; hipEvent_t ev_lvl[2] = {nullptr, nullptr};   // BLAS level loop: control words of the last two levels (pinned) + their events
    hipStream_t aux_stream = nullptr;                          // copies that overlap a kernel on `stream`
    VdBvhBuildStats bvh_stats = {};                            // vd_bvh_last_build_stats
    bool tlas_chain_lds_opt_in[2] = {false, false};              // tlas_build_kernel<VdTlasNode / VdTlasNodeWide>: dynamic LDS for the slot arrays
    bool mid_lds_opt_in = false;                               // blas_mid_kernel's dynamic-LDS attribute set on this device
    bool tlas_ix_lds_opt_in[2] = {false, false};               // tlas_build_indexed_kernel<VdTlasNode / VdTlasNodeWide>, likewise
};

// Every extern "C" entry point runs on the context's device: allocations, event records and launches otherwise go to
// the calling thread's CURRENT device (another thread, or torch.cuda.set_device(j) after the ctx was made for k).
struct VdDeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit VdDeviceGuard(const VdCtx* ctx) {
        if (!ctx) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != ctx->device) switched = hipSetDevice(ctx->device) == hipSuccess;
    }
    ~VdDeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    VdDeviceGuard(const VdDeviceGuard&) = delete;
    VdDeviceGuard& operator=(const VdDeviceGuard&) = delete;
};

#define VD_HIP_CHECK(ctx, call)                                                              \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s:%d %s -> %s", __FILE__, __LINE__,   \
                     #call, hipGetErrorString(e_));                                          \
            (void)hipGetLastError();   /* reported here: a later launch check must not find it again */ \
            return VD_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

#define VD_FAIL(ctx, code, msg)                                          \
    do {                                                                 \
        snprintf((ctx)->err, sizeof((ctx)->err), "%s", (msg));           \
        return (code);                                                   \
    } while (0)

// "<name>: <what>" -> VD_ERR_INVALID_ARG: what an entry point answers to an argument it refuses.
static inline int vd_fail_arg(VdCtx* ctx, const char* name, const char* what) {
    snprintf(ctx->err, sizeof(ctx->err), "%s: %s", name, what);
    return VD_ERR_INVALID_ARG;
}

// Grow-only arena helper. Never called between a kernel's enqueue and its completion on the
// same buffer without a stream sync (callers sync before growing).
int vd_ensure(VdCtx* ctx, void** buf, size_t* cur, size_t need);
int vd_ensure_host(VdCtx* ctx, size_t need);   // ctx->host_stage: grow-only pinned host memory
// tlas.hip: the agglomerative build of tlas.rs:56-105 over ready leaf boxes (six floats {min xyz, max xyz} per leaf; n <= 32 768)
int vd_tlas_build_from_boxes(VdCtx* ctx, const float* d_boxes, uint32_t n, VdTlasNode* d_nodes);
// tlas.hip: the LBVH build (vd_tlas_build_lbvh*) over ready leaf boxes, into 2n + 1 narrow nodes, with `work` (vd_lbvh_work_bytes(n)
// bytes of device memory, 256-byte aligned) as its work memory.  Enqueues only.  n <= 32 768.
size_t vd_lbvh_work_bytes(uint32_t n);
int vd_tlas_lbvh_from_boxes(VdCtx* ctx, const float* d_boxes, uint32_t n, VdTlasNode* d_nodes, void* work);
// tlas.hip: the first half of that build for any box array (blas_lbvh.hip: triangle boxes) - the codes of the box centres and their
// stable radix sort.  *keys / *vals = the sorted codes and, per sorted position, the index of its box; both lie inside `work`
// (vd_lbvh_sort_bytes(n) bytes, 256-byte aligned).  Enqueues only.  n <= 2^24.
size_t vd_lbvh_sort_bytes(uint32_t n);
int vd_lbvh_sort_boxes(VdCtx* ctx, const float* d_boxes, uint32_t n, void* work, const unsigned** keys, const unsigned** vals);
// tlas.hip: ... and for MANY box arrays side by side in one slot space (blas_lbvh.hip: the batched build).  Segment m owns the slots
// [slot0, slot0 + n_units * kVdLbvhBatchUnit); its first min(d_n_live[m], cap) slots (cap when d_n_live is null) hold boxes, read at
// d_boxes + 6 * slot.  After the call every segment's slots hold its pairs sorted by (code, position in the segment), the absent
// slots behind them; *vals are positions INSIDE the segment.  d_ext (6 words per segment) must hold the neutral elements
// (3 x 0xffffffff, 3 x 0) when the call starts.  The number of launches depends on n_slots alone (<= or > 16 384: the scan in
// parts), never on the counts.  `work`: vd_lbvh_batch_sort_bytes(n_slots) bytes, 256-byte aligned.  Enqueues only.
// (kVdLbvhBatchUnit, kVdLbvhExtentChunk, VdLbvhSeg: vd_plan.hpp)
struct VdLbvhBatchLayout {
    unsigned n_slots, n_chunks;            // n_slots: a multiple of kVdLbvhBatchUnit
    const VdLbvhSeg* d_segs;               // per segment
    const unsigned* d_unit_seg;            // per unit of the slot space: its segment
    const uint2* d_chunks;                 // {segment, first position}: ceil(cap / kVdLbvhExtentChunk) per segment
    unsigned* d_ext;                       // 6 words per segment
};
size_t vd_lbvh_batch_sort_bytes(uint32_t n_slots);
int vd_lbvh_batch_sort_boxes(VdCtx* ctx, const float* d_boxes, const VdLbvhBatchLayout* layout, const unsigned* d_n_live, void* work,
                             const unsigned** keys, const unsigned** vals);
// ... and into 2n + 1 WIDE nodes: n <= VD_TLAS_WIDE_MAX_INSTANCES.
int vd_tlas_lbvh_from_boxes_wide(VdCtx* ctx, const float* d_boxes, uint32_t n, VdTlasNodeWide* d_nodes, void* work);
// tlas.hip: the refit (vd_tlas_refit*) of a top level whose leaves sit at 1..n, from ready leaf boxes (six floats per INSTANCE; leaf
// j takes the box of its instance_idx): new leaf boxes, then bottom-up, topology kept.  `wide`: d_nodes is VdTlasNodeWide.  The links
// and arrival words live in `arena` (grown when needed - then it drains the stream first).  Enqueues only otherwise.
int vd_tlas_refit_from_boxes(VdCtx* ctx, const float* d_boxes, uint32_t n, void* d_nodes, bool wide, VdRefitArena* arena);
// Look-back scan state for n_tiles tiles: *ticket = 64-bit {epoch | ticket} word, *states = granules.
// Zeroed once when (re)allocated; the epoch tags make per-launch clearing unnecessary.
int vd_scan_scratch(VdCtx* ctx, unsigned n_tiles, unsigned long long** ticket, unsigned long long** states, bool start_timer);
// Has a scan of an earlier launch on this context given up (fault word in pinned host memory)?  Reports it ONCE: VD_ERR_HIP
// with a message, after draining the stream and zeroing the scan state; VD_OK otherwise.  Called at the entry of every vd_*
// that launches a look-back scan, so a renderer that only uses the *_dev forms hears about it on its next frame.
int vd_scan_check_fault(VdCtx* ctx);
static inline unsigned* vd_scan_fault_word(VdCtx* ctx) { return ctx->fault_dev; }
// The width of a mesh id by the size of the mesh table - 1, 2 or 4 bytes: the one statement of the rule (pass 1, the sharded
// scene's replicated table, the width check of vd_lod_ids_dev).
static inline unsigned vd_id_bytes(unsigned n_mesh) { return n_mesh <= 256u ? 1u : (n_mesh <= 65536u ? 2u : 4u); }
// Workgroups of a grid-stride launch: ceil(items / per_block), at most per_cu on every CU.
static inline unsigned vd_blocks(const VdCtx* ctx, unsigned items, unsigned per_block, unsigned per_cu) {
    const unsigned blocks = (items + per_block - 1u) / per_block, cap = (unsigned)ctx->num_cus * per_cu;
    return blocks < cap ? blocks : cap;
}

// What pass 1 of a split form leaves behind in its arena (where in the arena: cull.hip, pass1_plan - callers use these
// pointers, never offsets): view v's mask at mask + v * mask_stride, its survivors per 1024-instance tile at
// counts + v * count_stride.  rc != VD_OK: the arena could not be made, nothing was launched.
struct VdPass1 {
    int rc;
    unsigned long long* mask; void* ids; unsigned* counts;
    unsigned id_bytes, n_words, n_mt;          // id width by n_mesh; mask words; 1024-instance tiles
    size_t mask_stride, count_stride;          // words / entries between two views
};
// cull.hip: pass 1 of the single-view forms into ctx->scratch - cull_mask_tiled_kernel, and cull_mask_lod_kernel (the ids are
// rows of the mesh table, their width by n_mesh).  Both start the call's timer and record its stage boundary.  batch.hip
// groups by mesh / by row from the same passes.  Not part of the C ABI.
extern "C" __attribute__((visibility("hidden"))) VdPass1 launch_mask_pass(VdCtx* ctx, const VdCameraUniform* camera, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                                                                          const VdInstance* d_instances, uint32_t n_inst);
extern "C" __attribute__((visibility("hidden"))) VdPass1 launch_lod_pass(VdCtx* ctx, const VdCameraUniform* camera, const VdLodParams* params,
                                                                         const VdLodGroup* d_groups, uint32_t n_group, uint32_t n_mesh,
                                                                         const VdInstance* d_instances, uint32_t n_inst);
// ... and the argument check every LOD entry point shares (`name` prefixes the message).
extern "C" __attribute__((visibility("hidden"))) int vd_lod_check(VdCtx* ctx, const char* name, const VdCameraUniform* camera, const VdLodParams* params,
                                                                  const VdLodGroup* groups, uint32_t n_group, uint32_t n_mesh);

// cull.hip: the staged round trip of the host-pointer forms.  vd_stage drains the stream, sizes ctx->stage_in / stage_aux /
// stage_out and uploads the instances and, behind a header of `header` bytes at the front of stage_aux that takes the
// counts, the blobs in order, each at its alignment (*dev = where it went).  vd_fetch_lists reads n_views counts through
// host_pinned, refuses an implausible one (`scan`: the fused form's scan may have given up - fault word, state reset;
// otherwise "the expansion wrote no count"), and copies pad_tail ? n_inst : count commands per view from s.out + v * n_inst
// to out + v * out_stride.  out_counts == null: a list without a count, n_inst commands (vd_cull_emit).
struct VdBlob { const void* host; size_t bytes, align; void* dev; };
struct VdStaged { VdInstance* inst; uint32_t* counts; VdDrawIndexedIndirect* out; };
extern "C" __attribute__((visibility("hidden"))) int vd_stage(VdCtx* ctx, const VdInstance* instances, uint32_t n_inst, size_t header, VdBlob* blobs,
                                                              unsigned n_blobs, size_t out_bytes, VdStaged* s);
extern "C" __attribute__((visibility("hidden"))) int vd_fetch_lists(VdCtx* ctx, const char* name, bool scan, const VdStaged* s, uint32_t n_views, uint32_t n_inst,
                                                                    int pad_tail, VdDrawIndexedIndirect* out, uint64_t out_stride, uint32_t* out_counts);

// ctx.hip: the staged round trip of the host-pointer forms that are not draw lists (vd_trace*, vd_traverse*, vd_primary_rays,
// vd_tlas_*, vd_bvh_build*, vd_bvh_build_lbvh*, vd_bvh_refit).  vd_stage_blobs drains the stream, sizes ONE arena in
// ctx->stage_in, places every blob at its alignment (*dev) and uploads those that have a host pointer - one without is room for
// a result; vd_fetch_blob copies a blob back and drains again.  vd_fetch_blobs: blob b to hosts[b] where that is not null, ONE
// drain behind them all (the SAH builder's forms: two results per mesh; the LBVH batch: nodes, indices, VdMeshInfo per mesh).
extern "C" __attribute__((visibility("hidden"))) int vd_stage_blobs(VdCtx* ctx, VdBlob* blobs, unsigned n_blobs);
extern "C" __attribute__((visibility("hidden"))) int vd_fetch_blob(VdCtx* ctx, void* host, const VdBlob* blob);
extern "C" __attribute__((visibility("hidden"))) int vd_fetch_blobs(VdCtx* ctx, void* const* hosts, const VdBlob* blobs, unsigned n_blobs);

// Carves 256-byte aligned arrays out of one block of memory, in the order they are taken (base == null: only sizes it).
struct Arena {
    char* base; size_t off;
    template <typename T> T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return p;
    }
};

// Sizes and carves a buffer from ONE statement of its layout: `layout(Arena&)` takes the arrays in order and keeps the pointers.  It
// runs once over a null base (the pointers mean nothing yet), the buffer grows to what that took - draining the stream first when it
// has to move, see vd_ensure - and it runs again over the real base.
template <typename F> static inline int vd_carve(VdCtx* ctx, VdDeviceBuffer* buf, F&& layout) {
    Arena a{nullptr, 0};
    layout(a);
    const int rc = vd_ensure(ctx, &buf->state, &buf->bytes, a.off);
    if (rc) return rc;
    a = Arena{static_cast<char*>(buf->state), 0};
    layout(a);
    return VD_OK;
}

// ctx.hip: the device memory of a plan (vd_bvh_lbvh_plan_dev, vd_bvh_refit_plan_dev) - ONE allocation: the parts in order, each
// 256-byte aligned (*dev = where it went), then `work_bytes` of work memory (*work; may be null when there is none).  The parts
// are zeroed, those with a host pointer uploaded - blocking calls on the null stream - and the null stream is drained; the work
// memory is left as it comes.  A failure frees the allocation: "<who>: device memory" -> VD_ERR_OOM, HIP's own text -> VD_ERR_HIP.
// The caller owns *base and gives it back with vd_plan_free (null: nothing to free) once nothing queued uses the plan.
struct VdPlanPart { const void* host; size_t bytes; void* dev; };
extern "C" __attribute__((visibility("hidden"))) int vd_plan_tables(VdCtx* ctx, const char* who, VdPlanPart* parts, unsigned n_parts, size_t work_bytes,
                                                                    void** base, void** work);
extern "C" __attribute__((visibility("hidden"))) void vd_plan_free(void* base);

// Calls f with a value of the mesh-id type of that width - unsigned char, unsigned short or unsigned: the one place
// where an id width (1, 2 or 4 bytes; checked by the caller) picks a kernel instantiation.
//   vd_dispatch_id(id_bytes, [&](auto id) { using IdT = decltype(id); hipLaunchKernelGGL(some_kernel<IdT>, ...); });
template <typename F> static inline void vd_dispatch_id(unsigned id_bytes, F&& f) {
    if (id_bytes == 1u) f((unsigned char)0);
    else if (id_bytes == 2u) f((unsigned short)0);
    else f(0u);
}

static inline void vd_time_begin(VdCtx* ctx) {
    ctx->timed_mid = false;
    if (ctx->timing_enabled) (void)hipEventRecord(ctx->ev_start, ctx->stream);
}
static inline void vd_time_mid(VdCtx* ctx) {   // boundary between the two passes of a split call
    if (ctx->timing_enabled) { (void)hipEventRecord(ctx->ev_mid, ctx->stream); ctx->timed_mid = true; }
}
static inline void vd_time_end(VdCtx* ctx) {
    if (!ctx->timing_enabled) { ctx->timed = false; return; }
    (void)hipEventRecord(ctx->ev_stop, ctx->stream);
    ctx->timed = true;
}

#ifdef __HIPCC__
// ---- device helpers ------------------------------------------------------------------

// Order-preserving float key (-0 < +0) and Rust's f32::min / f32::max on top of it (glam 0.24 scalar
// Vec3::min/max, crates/bvh/src/blas.rs:190-198, tlas.rs:43,69-70,96-97): a NaN operand is IGNORED - the other
// operand is returned - and -0 < +0 is the tie rule Rust leaves open, which makes bounds
// reductions order-independent and bit-exact against the oracle.  Key reductions (integer atomic min / max) skip
// NaNs through vd_key_lo / vd_key_hi: a NaN maps to the neutral element of the reduction.
__device__ __forceinline__ int vd_key(float f) {
    int i = __float_as_int(f);
    return i ^ ((i >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float vd_unkey(int k) {
    return __int_as_float(k ^ ((k >> 31) & 0x7fffffff));
}
__device__ __forceinline__ int vd_key_lo(float f) { return f != f ? 0x7fffffff : vd_key(f); }        // operand of a min
__device__ __forceinline__ int vd_key_hi(float f) { return f != f ? (int)0x80000000 : vd_key(f); }   // operand of a max
// IEEE minNum / maxNum as gfx950 executes them - one v_min_f32 / v_max_f32: a QUIET NaN operand is ignored, both NaN ->
// NaN, and -0 orders below +0 (the ISA's LT_NEG_ZERO compare).  Exactly the semantics above, without the
// compare-and-select chains (which the compiler turned into six divergent branches per box union: the refit climb went
// from 0.10 to 0.18 ms).  A SIGNALLING NaN is different: in IEEE mode the instruction quiets and RETURNS it, and the
// compiler does not canonicalise the operands of fminf for us (LLVM leaves minnum(sNaN, x) open) - so raw user floats
// pass through vd_quiet once where they are loaded (blas_precompute_kernel); everything arithmetic produces is quiet.
__device__ __forceinline__ float vd_quiet(float x) { return __builtin_canonicalizef(x); }
__device__ __forceinline__ float vd_min_to(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float vd_max_to(float a, float b) { return __builtin_fmaxf(a, b); }

// crates/bvh/src/intersection.rs:16-19
__device__ __forceinline__ float vd_area(float dx, float dy, float dz) {
    return (dx * dy + dx * dz + dy * dz) * 2.0f;
}

__device__ __forceinline__ unsigned vd_lane() { return __lane_id(); }

// count of set bits of `mask` strictly below this lane
__device__ __forceinline__ unsigned vd_mbcnt(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// Compiler-level ordering for same-wave LDS exchange (DS ops of one wave execute in order).
__device__ __forceinline__ void vd_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef unsigned long long vd_u64;
#define VD_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- Karras' binary radix tree over sorted 30-bit codes (tlas.hip: lbvh_tree_kernel, blas_lbvh.hip: blas_lbvh_tree_kernel) ----
// length of the common prefix of the codes at sorted positions i and j (-1 outside the array); equal codes: their positions decide,
// i.e. the keys are the 64-bit words code << 32 | sorted position
// The LOW word of those keys: the sorted position itself (VdLbvhLowIsPosition - nothing is read), or a word per position from an
// array (VdLbvhLowArray: the depth-bounded bottom level, blas_lbvh.hip, whose keys are explicit).  Either way the 64-bit keys are
// distinct and ascending.
struct VdLbvhLowIsPosition { __device__ __forceinline__ unsigned operator()(int i) const { return (unsigned)i; } };
struct VdLbvhLowArray { const unsigned* __restrict__ low; __device__ __forceinline__ unsigned operator()(int i) const { return low[i]; } };
template <typename Low>
__device__ __forceinline__ int vd_lbvh_delta(const unsigned* __restrict__ keys, Low low, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const unsigned a = keys[i], b = keys[j];
    return a != b ? __clz((int)(a ^ b)) : 32 + __clz((int)(low(i) ^ low(j)));
}
__device__ __forceinline__ int vd_lbvh_delta(const unsigned* __restrict__ keys, int n, int i, int j) {
    return vd_lbvh_delta(keys, VdLbvhLowIsPosition{}, n, i, j);
}
// Karras 2012 for interior node i of n - 1: the sorted positions [lo, hi] it covers and its split - the left child covers
// [lo, gamma], the right one [gamma + 1, hi]; a child of one position is that leaf, any other is interior node gamma / gamma + 1.
template <typename Low>
__device__ __forceinline__ void vd_lbvh_range(const unsigned* __restrict__ keys, Low low, int N, int i, int& lo, int& hi, int& gamma) {
    const int d = vd_lbvh_delta(keys, low, N, i, i + 1) - vd_lbvh_delta(keys, low, N, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = vd_lbvh_delta(keys, low, N, i, i - d);
    int lmax = 2;
    while (vd_lbvh_delta(keys, low, N, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1) if (vd_lbvh_delta(keys, low, N, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = vd_lbvh_delta(keys, low, N, i, j);
    int sp = 0;
    for (int t = (l + 1) >> 1; ; t = (t + 1) >> 1) {
        if (vd_lbvh_delta(keys, low, N, i, i + (sp + t) * d) > dnode) sp += t;
        if (t == 1) break;
    }
    gamma = i + sp * d + min(d, 0);
    lo = min(i, j); hi = max(i, j);
}
__device__ __forceinline__ void vd_lbvh_range(const unsigned* __restrict__ keys, int N, int i, int& lo, int& hi, int& gamma) {
    vd_lbvh_range(keys, VdLbvhLowIsPosition{}, N, i, lo, hi, gamma);
}

// boxes in segment m of a batched slot space: the count on the device, read as the capacity when it is above it (or absent)
__device__ __forceinline__ unsigned vd_lbvh_seg_count(const VdLbvhSeg& sg, const unsigned* __restrict__ n_live, unsigned m) {
    return n_live ? min(n_live[m], sg.cap) : sg.cap;
}

// ---- VdMeshInfo.min / max of one mesh inside a launch that serves many (blas_refit.hip, blas_lbvh.hip) --------------------------
// MeshPool::calculate_bounds (crates/pools/src/mesh/mod.rs:22-27): the fold over ALL n_vert vertices from (+inf, -inf), NaN ignored,
// on the order-preserving integer image of the float bits.  One 256-thread block folds kVdVertChunk vertices from `first` on and
// sends six integer atomics to keys6; the block whose arrival completes the mesh (n_chunks of them) writes info->min / max and puts
// keys6 and *done back to their neutral values: nothing is cleared between launches.
// (kVdVertChunk, kVdKeyPosInf, kVdKeyNegInf: vd_plan.hpp)
__device__ __forceinline__ void vd_mesh_bounds_fold(const float* __restrict__ verts, unsigned n_vert, VdMeshInfo* info, unsigned n_chunks, unsigned first,
                                                    int* keys6, unsigned* done) {
    __shared__ int part[6][4];
    int k[6] = {kVdKeyPosInf, kVdKeyPosInf, kVdKeyPosInf, kVdKeyNegInf, kVdKeyNegInf, kVdKeyNegInf};
    const unsigned end = n_vert - first < kVdVertChunk ? n_vert : first + kVdVertChunk;
    for (unsigned v = first + threadIdx.x; v < end; v += 256u) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float p = verts[3u * (size_t)v + q];
            const int lo = vd_key_lo(p), hi = vd_key_hi(p);
            k[q] = lo < k[q] ? lo : k[q]; k[3 + q] = hi > k[3 + q] ? hi : k[3 + q];
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(k[q], off);
            k[q] = q < 3 ? (o < k[q] ? o : k[q]) : (o > k[q] ? o : k[q]);
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int q = 0; q < 6; ++q) part[q][threadIdx.x >> 6] = k[q];
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        int r = part[q][0];
        for (unsigned w = 1; w < 4u; ++w) r = q < 3 ? (part[q][w] < r ? part[q][w] : r) : (part[q][w] > r ? part[q][w] : r);
        if (q < 3) (void)__hip_atomic_fetch_min(&keys6[q], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else (void)__hip_atomic_fetch_max(&keys6[q], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned old = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old + 1u < n_chunks) return;
    __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
    for (int q = 0; q < 3; ++q) {                      // read and re-arm in one atomic each
        info->min[q] = vd_unkey(__hip_atomic_exchange(&keys6[q], kVdKeyPosInf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        info->max[q] = vd_unkey(__hip_atomic_exchange(&keys6[3 + q], kVdKeyNegInf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
}

// ---- single-pass ordered scan across workgroups ("decoupled look-back") ----------------
// tile_state[t] is one naturally aligned 8-byte {epoch:30 | status:2 | value:32} granule written
// by ONE agent-scope store and polled by agent-scope loads (write-through / L1-bypassing on
// gfx950), so the data is its own flag and no fence is needed.  A granule whose epoch is not the
// launch's epoch is INVALID, so nothing has to be zeroed between launches: the 64-bit ticket
// word {epoch:32 | next ticket:32} hands out both, and the workgroup that draws the last ticket
// re-arms it for the next launch ({epoch + 1, 0}) - the state advances ON THE DEVICE, so a launch
// recorded in a HIP graph replays correctly (tests/test_gpu_frame_loop.py).  Tickets come from an
// atomic counter, so every predecessor of a running tile is itself running or finished: no
// residency assumption.
// Every wait is BOUNDED, by the wall clock: a tile whose predecessor does not show up within kScanTimeoutTicks of the
// constant 100 MHz counter (two seconds; an ordinary wait is microseconds) - ONE deadline for both of its waiting loops -
// publishes VD_TILE_POISON and returns VD_SCAN_STUCK, and every later tile that runs into the poison does the same at once.
// Giving up is STICKY for the launch: the tile also stores the launch's epoch + 1 into the arena's stuck word, and the last
// tile looks at that word after its own look-back - a tile that had read the quitter's AGGREGATE before it was poisoned and
// then completed normally would otherwise hide the failure behind its INCLUSIVE.  What the last tile then does is
// the kernel's business (cull.hip: count = 0, no list, the fault word in pinned host memory raised - the next vd_* call on the
// context reports VD_ERR_HIP and zeroes the scan state); a launch that lost its LAST tile keeps the count the first tile
// pre-stored, VD_SCAN_STUCK.
// Arena layout (vd_scan_scratch): u64[0] ticket word, u64[1] tuning hook (vd_debug_scan_fault), u64[2] stuck word,
// u64[3] spare, granules from byte 32: the stuck word of a granule array is tile_state[-2].
enum : unsigned { VD_TILE_AGGREGATE = 1u, VD_TILE_INCLUSIVE = 2u, VD_TILE_POISON = 3u };
constexpr unsigned VD_SCAN_STUCK = 0xffffffffu;
constexpr unsigned long long kScanTimeoutTicks = 200000000ull;     // wall_clock64(): 100 MHz on gfx950 -> 2 s
constexpr int kScanFaultWord = 63;                                 // VdCtx::host_pinned[63]: raised by a launch whose scan gave up

__device__ __forceinline__ vd_u64 vd_tile_pack(unsigned epoch, unsigned status, unsigned value) {
    return ((vd_u64)(epoch & 0x3fffffffu) << 34) | ((vd_u64)status << 32) | value;
}

// ONE lane: draw a ticket.  Returns the ticket; *epoch = this launch's epoch.
__device__ __forceinline__ unsigned vd_take_ticket(vd_u64* ticket_word, unsigned n_tiles, unsigned* epoch) {
    const vd_u64 t = __hip_atomic_fetch_add(ticket_word, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned ticket = (unsigned)t, ep = (unsigned)(t >> 32);
    *epoch = ep;
    if (ticket == n_tiles - 1u)   // every ticket of this launch is out: re-arm for the next one
        __hip_atomic_store(ticket_word, (vd_u64)(ep + 1u) << 32, VD_RLX_AGENT);
    return ticket;
}

__device__ __forceinline__ bool vd_scan_gave_up(vd_u64* tile_state, unsigned epoch) {      // has any tile of this launch given up?
    return __hip_atomic_load(tile_state - 2, VD_RLX_AGENT) == (vd_u64)(epoch & 0x3fffffffu) + 1ull;
}

// Called by ONE full wave of the workgroup. Returns the exclusive prefix of tile `t`
// (sum of `total` over tiles < t) in every lane, after publishing this tile's state - or VD_SCAN_STUCK.
// `first` marks the first tile of a segment (segmented scan): its prefix restarts at 0.
__device__ __forceinline__ unsigned vd_lookback(vd_u64* tile_state, unsigned epoch, unsigned t, unsigned total, bool first = false) {
    const unsigned lane = vd_lane();
    const unsigned ep = epoch & 0x3fffffffu;
    if (t == 0 || first) {
        if (lane == 0) __hip_atomic_store(&tile_state[t], vd_tile_pack(ep, VD_TILE_INCLUSIVE, total), VD_RLX_AGENT);
        return 0u;
    }
    if (lane == 0) __hip_atomic_store(&tile_state[t], vd_tile_pack(ep, VD_TILE_AGGREGATE, total), VD_RLX_AGENT);
    const unsigned long long deadline = wall_clock64() + kScanTimeoutTicks;      // one deadline for both loops below: they expire together
    unsigned exclusive = 0u;
    int look = (int)t - 1;
    bool stuck = false;
    {   // tiles finish roughly in ticket order: wait for the immediate predecessor with ONE lane
        // (one 8-byte poll per iteration instead of a 64-granule window), then sweep the window
        if (lane == 0) {
            vd_u64 s0 = __hip_atomic_load(&tile_state[look], VD_RLX_AGENT);
            unsigned spins = 0;
            while ((unsigned)(s0 >> 34) != ep || ((unsigned)(s0 >> 32) & 3u) == 0u) {
                if ((++spins & 63u) == 0u && wall_clock64() > deadline) { stuck = true; break; }
                __builtin_amdgcn_s_sleep(8);
                s0 = __hip_atomic_load(&tile_state[look], VD_RLX_AGENT);
            }
        }
        stuck = __builtin_amdgcn_readfirstlane((int)stuck) != 0;
    }
    while (!stuck) {
        const int idx = look - (int)lane;
        vd_u64 s = vd_tile_pack(ep, VD_TILE_INCLUSIVE, 0u);   // virtual tiles before 0
        bool mine_stuck = false;
        if (idx >= 0) {
            s = __hip_atomic_load(&tile_state[idx], VD_RLX_AGENT);
            unsigned spins = 0;
            while ((unsigned)(s >> 34) != ep || ((unsigned)(s >> 32) & 3u) == 0u) {   // not written in this launch yet
                if ((++spins & 63u) == 0u && wall_clock64() > deadline) { mine_stuck = true; break; }
                __builtin_amdgcn_s_sleep(1);
                s = __hip_atomic_load(&tile_state[idx], VD_RLX_AGENT);
            }
        }
        const unsigned status = (unsigned)(s >> 32) & 3u;
        const unsigned value = (unsigned)s;
        const unsigned long long incl = __ballot(!mine_stuck && status == VD_TILE_INCLUSIVE);
        // lanes at or before the first INCLUSIVE one (closest predecessors first) contribute
        const unsigned first_incl = incl ? (unsigned)__builtin_ctzll(incl) : 63u;
        if (__ballot(lane <= first_incl && (mine_stuck || status == VD_TILE_POISON))) { stuck = true; break; }   // a predecessor gave up, or never came
        unsigned v = lane <= first_incl ? value : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        exclusive += v;
        if (incl) break;
        look -= 64;
    }
    if (stuck) {
        if (lane == 0) {
            __hip_atomic_store(tile_state - 2, (vd_u64)ep + 1ull, VD_RLX_AGENT);      // sticky for the launch: the last tile reads it
            __hip_atomic_store(&tile_state[t], vd_tile_pack(ep, VD_TILE_POISON, 0u), VD_RLX_AGENT);
        }
        return VD_SCAN_STUCK;
    }
    if (lane == 0) __hip_atomic_store(&tile_state[t], vd_tile_pack(ep, VD_TILE_INCLUSIVE, exclusive + total), VD_RLX_AGENT);
    return exclusive;
}

// What the LAST tile of a launch stores as the count (one lane): the total - or, when some tile of the launch gave up, 0
// (no list was written: nothing to draw) while the fault word in pinned host memory is raised for the host side.
__device__ __forceinline__ unsigned vd_scan_final_count(vd_u64* tile_state, unsigned epoch, unsigned excl, unsigned tile_total, unsigned* fault_host) {
    if (excl != VD_SCAN_STUCK && !vd_scan_gave_up(tile_state, epoch)) return excl + tile_total;
    __hip_atomic_store(fault_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return 0u;
}
#endif  // __HIPCC__
