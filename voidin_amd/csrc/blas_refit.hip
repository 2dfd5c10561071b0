// blas_refit.hip — BLAS refit on gfx950: new boxes for a mesh whose vertices moved, same topology.
//
// Every box BvhBuilder writes is `calculate_bounds` over the vertices of the node's triangles (reference:
// crates/bvh/src/blas.rs:184-204): a fold from (+1e30, -1e30) with f32::min / f32::max, which ignore a NaN operand; the tie
// -0 < +0 is the oracle's (oracle/vd_oracle_math.h).  That min / max is associative and commutative, so an interior box is
// the union of its two children's boxes and refit(build(x), x) == build(x) bit for bit.
//
// A plan (vd_bvh_refit_plan_dev, once per topology, blocking) copies each item's nodes and indices to the host, validates
// what the kernel will walk and derives: a parent link per node, an arrival counter per node, the list of leaves.  The plan
// keeps the items' POINTERS; vertices, and the boxes it rewrites, are read through them at every refit.
//
// The refit (vd_bvh_refit_planned_dev) is ONE launch for all items of the plan and nothing else - no host read, no
// allocation, no memset - so it can be captured into a HIP graph:
//   * a lane takes a leaf, folds its triangles' vertices, stores the box and climbs;
//   * at each parent it bumps the arrival counter: the first arriver leaves, the second reads the sibling's box, stores
//     the union and goes on, up to node 0.  Nobody waits for anybody: no spin, no look-back.  Parent ids come from the
//     plan's own array, where every parent id is smaller than the child's (validated), so a climb ends after at most
//     n_nodes steps whatever the node array holds by then;
//   * the arriver that completes a node puts its counter back to 0: the same plan refits again with nothing cleared.
// Visibility of a box between the two lanes that meet at a parent (any two workgroups, any two XCDs - private L2s, L1s
// that other CUs' stores never refresh): every word of the box is a write-through agent-scope GLOBAL store, the storing
// wave drains its stores (s_waitcnt vmcnt(0)) before the agent-scope counter add, and the lane whose add came second reads
// the sibling's box with agent-scope global loads, which bypass its L1 - the form the TLAS refit climbs with (tlas.hip).
// A plain cached load of the sibling box is what would be wrong here.  VD_OPT_BLAS_REFIT_FENCES = 1 adds an agent-scope
// release fence before the add and an acquire fence after it (an L2 write-back and an L1 invalidate per wave and level):
// same bytes, measured beside the default in profiles/blas_refit.md.
//   * blocks behind the leaf blocks fold ALL n_vert vertices of every item that carries a VdMeshInfo from (+inf, -inf)
//     (MeshPool::calculate_bounds, crates/pools/src/mesh/mod.rs:22-27), 4096 vertices per block, on the order-preserving
//     integer image of the float bits (vd_key: -0 below +0, NaN mapped to the neutral element), integer atomic min / max
//     across blocks; the block whose arrival completes an item writes MeshInfo.min / max and re-arms the item's words.
//
// The host side: vd_bvh_refit_plan_dev is judge and derive (plan_tables: the read-back of an item's nodes and indices, then
// blas_refit_plan.hpp - pure host arithmetic, tested without a GPU by tests/cpp/blas_refit_plan_test.cpp) -> upload (plan_upload:
// vd_plan_tables, ctx.hip - one allocation) -> the plan struct.  vd_bvh_refit stages in the context's one arena (vd_stage_blobs /
// vd_fetch_blob, ctx.hip): the nodes go up and come back.  profiles/blas_lbvh_host_layer.md.
#include "vd_common.hpp"
#include "blas_refit_plan.hpp"

#include <new>
#include <vector>

namespace {

constexpr unsigned kBlock = 256u;                      // (kNoParent, RefitItemDev: blas_refit_plan.hpp, which fills the plan's tables)

}  // namespace

struct VdBvhRefitPlan {
    unsigned n_items = 0, n_leaves = 0, n_chunks = 0;
    void* dev = nullptr;                               // ONE allocation: everything below
    RefitItemDev* d_items = nullptr;
    uint4* d_leaves = nullptr;                         // {item, node, first triangle, triangle count}, ascending node id within an item
    unsigned* d_up = nullptr;                          // per node: parent << 1 | (node is the right child), kNoParent for node 0 / the reserved slot
    unsigned* d_arrivals = nullptr;                    // per node: 0 between refits
    int* d_keys = nullptr;                             // per item: 3 min keys, 3 max keys, at their neutral values between refits
    unsigned* d_done = nullptr;                        // per item: blocks of the MeshInfo fold that arrived; 0 between refits
    uint2* d_chunks = nullptr;                         // per fold block: {item, first vertex}
};

namespace {

// the boxes that change hands inside the launch: GLOBAL (never flat) agent-scope accesses - write-through stores, L1-bypassing loads
typedef __attribute__((address_space(1))) float gfloat;
__device__ __forceinline__ gfloat* box_words(VdBvhNode* n) { return (gfloat*)reinterpret_cast<float*>(n); }      // min xyz at words 0..2, max xyz at 4..6

__device__ __forceinline__ void store_box_agent(VdBvhNode* n, const float* mn, const float* mx) {
    gfloat* w = box_words(n);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        __hip_atomic_store(w + q, mn[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(w + 4 + q, mx[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool kFences>
__device__ __forceinline__ void leaf_climb(const RefitItemDev* __restrict__ items, const uint4 leaf, const unsigned* __restrict__ up,
                                           unsigned* arrivals) {
    const RefitItemDev it = items[leaf.x];
    float mn[3] = {1e30f, 1e30f, 1e30f}, mx[3] = {-1e30f, -1e30f, -1e30f};
    for (unsigned t = 0; t < leaf.w; ++t) {
        const size_t tri = (size_t)leaf.z + t;
        if (tri >= it.n_tri) break;                    // the plan checked the range; a node array edited since must not read outside
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned vi = it.indices[3u * tri + c];
            if (vi >= it.n_vert) continue;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float p = vd_quiet(it.verts[3u * (size_t)vi + q]);      // a signalling NaN is ignored like a quiet one
                mn[q] = vd_min_to(mn[q], p); mx[q] = vd_max_to(mx[q], p);
            }
        }
    }
    unsigned k = leaf.y;
    if (k >= it.n_nodes) return;
    up += it.node_base; arrivals += it.node_base;
    for (;;) {
        store_box_agent(&it.nodes[k], mn, mx);
        const unsigned u = up[k];
        if (u == kNoParent) return;                    // node 0 is done
        const unsigned p = u >> 1, s = (u & 1u) ? k - 1u : k + 1u;
        if (p >= k || s >= it.n_nodes) return;         // cannot happen with the plan's own links: ids strictly fall on the way up
        if (kFences) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // no instruction: the stores stay above the add
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                      // my write-through box has reached memory before the counter says so
        const unsigned old = __hip_atomic_fetch_add(&arrivals[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0u) return;                         // first at this parent: the sibling's climber goes on
        __hip_atomic_store(&arrivals[p], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-armed for the next refit
        if (kFences) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");          // no instruction: the loads stay below the add
        gfloat* w = box_words(&it.nodes[s]);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float a = __hip_atomic_load(w + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float b = __hip_atomic_load(w + 4 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mn[q] = vd_min_to(mn[q], a); mx[q] = vd_max_to(mx[q], b);
        }
        k = p;
    }
}

__device__ __forceinline__ void bounds_fold(const RefitItemDev* __restrict__ items, const uint2 chunk, int* keys, unsigned* done) {
    const RefitItemDev it = items[chunk.x];
    vd_mesh_bounds_fold(it.verts, it.n_vert, it.info, it.n_chunks, chunk.y, keys + 6u * chunk.x, done + chunk.x);      // vd_common.hpp
}

template <bool kFences>
__global__ __launch_bounds__(kBlock) void blas_refit_kernel(const RefitItemDev* __restrict__ items, const uint4* __restrict__ leaves,
                                                            unsigned n_leaves, unsigned leaf_blocks, const unsigned* __restrict__ up,
                                                            unsigned* arrivals, const uint2* __restrict__ chunks, int* keys, unsigned* done) {
    if (blockIdx.x >= leaf_blocks) { bounds_fold(items, chunks[blockIdx.x - leaf_blocks], keys, done); return; }
    const unsigned g = blockIdx.x * kBlock + threadIdx.x;
    if (g < n_leaves) leaf_climb<kFences>(items, leaves[g], up, arrivals);
}

int fail_item(VdCtx* ctx, VdBvhRefitItem* items, uint32_t m, const char* what) {
    items[m].status = VD_ERR_INVALID_ARG;
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "vd_bvh_refit_plan: item %u: %s", m, what);
    return VD_ERR_INVALID_ARG;
}

// judge and derive: every item's nodes and indices are read back (into the caller's two buffers, one item at a time) and go
// through blas_refit_plan.hpp
int plan_tables(VdCtx* ctx, VdBvhRefitItem* items, uint32_t n_items, RefitPlanTables& t, std::vector<VdBvhNode>& nodes, std::vector<unsigned>& idx) {
    t.items.reserve(n_items);
    for (uint32_t m = 0; m < n_items; ++m) {
        const VdBvhRefitItem& it = items[m];
        if (const char* what = refit_judge_item(t, it)) return fail_item(ctx, items, m, what);
        nodes.resize(it.n_nodes);
        idx.resize(3 * (size_t)it.n_tri);
        VD_HIP_CHECK(ctx, hipMemcpy(nodes.data(), it.nodes, sizeof(VdBvhNode) * (size_t)it.n_nodes, hipMemcpyDeviceToHost));
        if (it.n_tri) VD_HIP_CHECK(ctx, hipMemcpy(idx.data(), it.indices, 12 * (size_t)it.n_tri, hipMemcpyDeviceToHost));
        if (const char* what = refit_plan_item(t, m, it, nodes.data(), idx.data())) return fail_item(ctx, items, m, what);
    }
    return VD_OK;
}

// upload: the tables in ONE allocation, and the plan's pointers into it.  Arrival and done counters are not uploaded: they start
// at 0 and come back to 0 after every refit.
static_assert(sizeof(VdPair) == sizeof(uint2) && sizeof(VdQuad) == sizeof(uint4), "chunk and leaf records are uploaded where the kernel reads uint2 / uint4");
int plan_upload(VdCtx* ctx, const RefitPlanTables& t, VdBvhRefitPlan* p) {
    const size_t n = t.items.size();
    const std::vector<int> keys = vd_fold_neutral_keys(n);
    enum { kItems, kLeaves, kUp, kArrivals, kKeys, kDone, kChunks, kParts };
    VdPlanPart part[kParts] = {{t.items.data(), sizeof(RefitItemDev) * n, nullptr},
                               {t.leaves.data(), sizeof(VdQuad) * t.leaves.size(), nullptr},
                               {t.up.data(), 4 * t.up.size(), nullptr},
                               {nullptr, 4 * t.up.size(), nullptr},
                               {keys.data(), 4 * keys.size(), nullptr},
                               {nullptr, 4 * n, nullptr},
                               {t.chunks.data(), sizeof(VdPair) * t.chunks.size(), nullptr}};
    const int rc = vd_plan_tables(ctx, "vd_bvh_refit_plan", part, kParts, 0, &p->dev, nullptr);
    if (rc) return rc;
    p->d_items = static_cast<RefitItemDev*>(part[kItems].dev);
    p->d_leaves = static_cast<uint4*>(part[kLeaves].dev);
    p->d_up = static_cast<unsigned*>(part[kUp].dev);
    p->d_arrivals = static_cast<unsigned*>(part[kArrivals].dev);
    p->d_keys = static_cast<int*>(part[kKeys].dev);
    p->d_done = static_cast<unsigned*>(part[kDone].dev);
    p->d_chunks = static_cast<uint2*>(part[kChunks].dev);
    return VD_OK;
}

}  // namespace

extern "C" {

int vd_bvh_refit_plan_release(VdCtx* ctx, VdBvhRefitPlan* plan) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !plan) return VD_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(ctx->stream);           // a queued refit still reads the plan's arrays
    vd_plan_free(plan->dev);
    delete plan;
    return VD_OK;
}

int vd_bvh_refit_plan_dev(VdCtx* ctx, VdBvhRefitItem* items, uint32_t n_items, VdBvhRefitPlan** out) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !out) return VD_ERR_INVALID_ARG;
    *out = nullptr;
    if (n_items && !items) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_refit_plan: null item array");
    for (uint32_t m = 0; m < n_items; ++m) items[m].status = VD_OK;
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));      // the nodes / indices may come from work still queued
    VdBvhRefitPlan* p = nullptr;
    try {
        std::vector<VdBvhNode> nodes;                  // the read-back buffers live until the plan is uploaded, as they always did: a megabyte
        std::vector<unsigned> idx;                     // freed in between costs every plan call its page faults again (profiles/blas_lbvh_host_layer.md, 5)
        RefitPlanTables t;
        int rc = plan_tables(ctx, items, n_items, t, nodes, idx);
        if (rc) return rc;
        p = new VdBvhRefitPlan();
        p->n_items = n_items; p->n_leaves = (unsigned)t.leaves.size(); p->n_chunks = (unsigned)t.chunks.size();
        if (n_items && (rc = plan_upload(ctx, t, p))) { delete p; return rc; }      // no plan is returned after a refusal
    } catch (const std::bad_alloc&) {
        delete p;
        VD_FAIL(ctx, VD_ERR_OOM, "vd_bvh_refit_plan: host memory");
    }
    *out = p;
    return VD_OK;
}

int vd_bvh_refit_planned_dev(VdCtx* ctx, const VdBvhRefitPlan* plan) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!plan) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_refit_planned: null plan");
    const unsigned leaf_blocks = (plan->n_leaves + kBlock - 1u) / kBlock;
    if (leaf_blocks + plan->n_chunks == 0u) return VD_OK;
    vd_time_begin(ctx);
    if (ctx->option(VD_OPT_BLAS_REFIT_FENCES, 0) != 0)
        hipLaunchKernelGGL(blas_refit_kernel<true>, dim3(leaf_blocks + plan->n_chunks), dim3(kBlock), 0, ctx->stream, plan->d_items, plan->d_leaves,
                           plan->n_leaves, leaf_blocks, plan->d_up, plan->d_arrivals, plan->d_chunks, plan->d_keys, plan->d_done);
    else
        hipLaunchKernelGGL(blas_refit_kernel<false>, dim3(leaf_blocks + plan->n_chunks), dim3(kBlock), 0, ctx->stream, plan->d_items, plan->d_leaves,
                           plan->n_leaves, leaf_blocks, plan->d_up, plan->d_arrivals, plan->d_chunks, plan->d_keys, plan->d_done);
    VD_HIP_CHECK(ctx, hipGetLastError());
    vd_time_end(ctx);
    return VD_OK;
}

int vd_bvh_refit(VdCtx* ctx, const float* verts_xyz, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                 VdBvhNode* nodes_inout, uint32_t n_nodes) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!verts_xyz || !indices || !nodes_inout || n_vert == 0u || n_tri == 0u || n_nodes == 0u)
        VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_refit: null or empty vertices / indices / nodes");
    VdBlob blobs[3] = {{verts_xyz, 12 * (size_t)n_vert, 256, nullptr}, {indices, 12 * (size_t)n_tri, 256, nullptr},
                       {nodes_inout, sizeof(VdBvhNode) * (size_t)n_nodes, 256, nullptr}};      // the nodes go up and come back
    int rc = vd_stage_blobs(ctx, blobs, 3);
    if (rc) return rc;
    VdBvhRefitItem it{};
    it.verts_xyz = static_cast<const float*>(blobs[0].dev); it.indices = static_cast<const uint32_t*>(blobs[1].dev);
    it.nodes = static_cast<VdBvhNode*>(blobs[2].dev); it.mesh_info = nullptr;
    it.n_vert = n_vert; it.n_tri = n_tri; it.n_nodes = n_nodes;
    VdBvhRefitPlan* plan = nullptr;
    if ((rc = vd_bvh_refit_plan_dev(ctx, &it, 1u, &plan))) return rc;
    rc = vd_bvh_refit_planned_dev(ctx, plan);
    if (rc == VD_OK) rc = vd_fetch_blob(ctx, nodes_inout, &blobs[2]);
    (void)vd_bvh_refit_plan_release(ctx, plan);
    return rc;
}

}  // extern "C"
