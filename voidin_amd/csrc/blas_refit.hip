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
#include "vd_common.hpp"

#include <new>
#include <vector>

namespace {

constexpr unsigned kNoParent = 0xffffffffu;
constexpr unsigned kBlock = 256u;
constexpr unsigned kVertChunk = kVdVertChunk;          // vertices per block of the MeshInfo fold (vd_common.hpp: vd_mesh_bounds_fold)
constexpr int kKeyPosInf = kVdKeyPosInf, kKeyNegInf = kVdKeyNegInf;      // the neutral keys of its min / max

struct RefitItemDev {
    const float* verts; const unsigned* indices; VdBvhNode* nodes; VdMeshInfo* info;
    unsigned n_vert, n_tri, n_nodes, node_base;        // node_base: where the item's links / counters start in the plan's arrays
    unsigned n_chunks, _pad[3];
};
static_assert(sizeof(RefitItemDev) == 64, "one item record per cache-line half");

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
    snprintf(ctx->err, sizeof(ctx->err), "vd_bvh_refit_plan: item %u: %s", m, what);
    return VD_ERR_INVALID_ARG;
}

}  // namespace

extern "C" {

int vd_bvh_refit_plan_release(VdCtx* ctx, VdBvhRefitPlan* plan) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !plan) return VD_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(ctx->stream);           // a queued refit still reads the plan's arrays
    if (plan->dev) (void)hipFree(plan->dev);
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
    std::vector<RefitItemDev> h_items(n_items);
    std::vector<uint4> h_leaves;
    std::vector<unsigned> h_up;
    std::vector<uint2> h_chunks;
    std::vector<VdBvhNode> nodes;
    std::vector<unsigned> idx;
    try {
        for (uint32_t m = 0; m < n_items; ++m) {
            const VdBvhRefitItem& it = items[m];
            if (!it.verts_xyz || !it.indices || !it.nodes) return fail_item(ctx, items, m, "null vertices / indices / nodes");
            if (it.n_nodes < 1u) return fail_item(ctx, items, m, "n_nodes < 1");
            if (it.n_nodes > 0x7fffffffu || (size_t)h_up.size() + it.n_nodes > 0xfffffff0u) return fail_item(ctx, items, m, "too many nodes for one plan");
            nodes.resize(it.n_nodes);
            idx.resize(3 * (size_t)it.n_tri);
            VD_HIP_CHECK(ctx, hipMemcpy(nodes.data(), it.nodes, sizeof(VdBvhNode) * (size_t)it.n_nodes, hipMemcpyDeviceToHost));
            if (it.n_tri) VD_HIP_CHECK(ctx, hipMemcpy(idx.data(), it.indices, 12 * (size_t)it.n_tri, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < idx.size(); ++k)
                if (idx[k] >= it.n_vert) return fail_item(ctx, items, m, "an index >= n_vert");
            const size_t base = h_up.size();
            h_up.resize(base + it.n_nodes, kNoParent);
            unsigned* up = h_up.data() + base;
            // children follow their parent (pre-order), so one ascending sweep knows every node's parent before it gets there
            for (unsigned k = 0; k < it.n_nodes; ++k) {
                if (k != 0u && up[k] == kNoParent) {
                    if (k == 1u) continue;             // the reserved slot: whatever it holds, nobody reads or writes it
                    return fail_item(ctx, items, m, "a node other than 0 and the reserved slot 1 has no parent");
                }
                const VdBvhNode& nd = nodes[k];
                if (nd.count == 0u) {
                    const uint64_t l = nd.left_first;
                    if (l <= k || l + 1u >= it.n_nodes) return fail_item(ctx, items, m, "an interior node's children are not both in (own id, n_nodes)");
                    if (up[l] != kNoParent || up[l + 1u] != kNoParent) return fail_item(ctx, items, m, "a node has two parents");
                    up[l] = k << 1; up[l + 1u] = (k << 1) | 1u;
                } else {
                    if ((uint64_t)nd.left_first + nd.count > it.n_tri) return fail_item(ctx, items, m, "a leaf's triangle range leaves [0, n_tri)");
                    if (h_leaves.size() >= 0xfffffff0u) return fail_item(ctx, items, m, "too many leaves for one plan");
                    h_leaves.push_back(make_uint4(m, k, nd.left_first, nd.count));
                }
            }
            RefitItemDev& d = h_items[m];
            d = RefitItemDev{};
            d.verts = it.verts_xyz; d.indices = it.indices; d.nodes = it.nodes; d.info = it.mesh_info;
            d.n_vert = it.n_vert; d.n_tri = it.n_tri; d.n_nodes = it.n_nodes; d.node_base = (unsigned)base;
            if (it.mesh_info) {
                d.n_chunks = it.n_vert ? (unsigned)(((size_t)it.n_vert + kVertChunk - 1u) / kVertChunk) : 1u;      // an empty fold still writes (+inf, -inf)
                for (unsigned c = 0; c < d.n_chunks; ++c) h_chunks.push_back(make_uint2(m, c * kVertChunk));
            }
        }
    } catch (const std::bad_alloc&) {
        VD_FAIL(ctx, VD_ERR_OOM, "vd_bvh_refit_plan: host memory");
    }
    VdBvhRefitPlan* p = new (std::nothrow) VdBvhRefitPlan();
    if (!p) VD_FAIL(ctx, VD_ERR_OOM, "vd_bvh_refit_plan: host memory");
    p->n_items = n_items; p->n_leaves = (unsigned)h_leaves.size(); p->n_chunks = (unsigned)h_chunks.size();
    *out = p;
    if (n_items == 0) return VD_OK;
    auto up256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_items = 0, o_leaves = up256(sizeof(RefitItemDev) * n_items), o_up = o_leaves + up256(16 * h_leaves.size()),
                 o_arr = o_up + up256(4 * h_up.size()), o_keys = o_arr + up256(4 * h_up.size()), o_done = o_keys + up256(24 * (size_t)n_items),
                 o_chunks = o_done + up256(4 * (size_t)n_items), total = o_chunks + up256(8 * h_chunks.size());
    std::vector<int> h_keys(6 * (size_t)n_items);
    for (size_t m = 0; m < n_items; ++m)
        for (int q = 0; q < 6; ++q) h_keys[6 * m + q] = q < 3 ? kKeyPosInf : kKeyNegInf;
    hipError_t e = hipMalloc(&p->dev, total);
    if (e != hipSuccess) { delete p; *out = nullptr; VD_FAIL(ctx, VD_ERR_OOM, "vd_bvh_refit_plan: device memory"); }
    char* base = reinterpret_cast<char*>(p->dev);
    e = hipMemset(base, 0, total);                     // arrival and done counters start at 0 and come back to 0 after every refit
    if (e == hipSuccess) e = hipMemcpy(base + o_items, h_items.data(), sizeof(RefitItemDev) * n_items, hipMemcpyHostToDevice);
    if (e == hipSuccess && !h_leaves.empty()) e = hipMemcpy(base + o_leaves, h_leaves.data(), 16 * h_leaves.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + o_up, h_up.data(), 4 * h_up.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + o_keys, h_keys.data(), 4 * h_keys.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !h_chunks.empty()) e = hipMemcpy(base + o_chunks, h_chunks.data(), 8 * h_chunks.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // the uploads ran on the default stream; the refit runs on the context's
    if (e != hipSuccess) {
        (void)hipFree(p->dev); delete p; *out = nullptr;
        VD_FAIL(ctx, VD_ERR_HIP, hipGetErrorString(e));
    }
    p->d_items = reinterpret_cast<RefitItemDev*>(base + o_items);
    p->d_leaves = reinterpret_cast<uint4*>(base + o_leaves);
    p->d_up = reinterpret_cast<unsigned*>(base + o_up);
    p->d_arrivals = reinterpret_cast<unsigned*>(base + o_arr);
    p->d_keys = reinterpret_cast<int*>(base + o_keys);
    p->d_done = reinterpret_cast<unsigned*>(base + o_done);
    p->d_chunks = reinterpret_cast<uint2*>(base + o_chunks);
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
    const size_t bv = 12 * (size_t)n_vert, bi = 12 * (size_t)n_tri, bn = sizeof(VdBvhNode) * (size_t)n_nodes;
    const size_t o_i = (bv + 255) & ~(size_t)255, o_n = o_i + ((bi + 255) & ~(size_t)255);
    char* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), o_n + bn) != hipSuccess) VD_FAIL(ctx, VD_ERR_OOM, "vd_bvh_refit: staging");
    VdBvhRefitPlan* plan = nullptr;
    int rc = VD_OK;
    hipError_t e = hipMemcpy(d, verts_xyz, bv, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_i, indices, bi, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + o_n, nodes_inout, bn, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        VdBvhRefitItem it{};
        it.verts_xyz = reinterpret_cast<const float*>(d); it.indices = reinterpret_cast<const uint32_t*>(d + o_i);
        it.nodes = reinterpret_cast<VdBvhNode*>(d + o_n); it.mesh_info = nullptr;
        it.n_vert = n_vert; it.n_tri = n_tri; it.n_nodes = n_nodes;
        rc = vd_bvh_refit_plan_dev(ctx, &it, 1u, &plan);
        if (rc == VD_OK) rc = vd_bvh_refit_planned_dev(ctx, plan);
        if (rc == VD_OK) {
            e = hipStreamSynchronize(ctx->stream);
            if (e == hipSuccess) e = hipMemcpy(nodes_inout, d + o_n, bn, hipMemcpyDeviceToHost);
        }
    }
    if (plan) (void)vd_bvh_refit_plan_release(ctx, plan);
    (void)hipFree(d);
    if (rc != VD_OK) return rc;
    if (e != hipSuccess) VD_FAIL(ctx, VD_ERR_HIP, hipGetErrorString(e));
    return VD_OK;
}

}  // extern "C"
