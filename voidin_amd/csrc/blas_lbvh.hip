// blas_lbvh.hip — LBVH bottom level on gfx950 (vd_bvh_build_lbvh*): a BLAS for a mesh whose TRIANGLES change every frame.
//
// NOT the reference's tree (that is blas.hip, the exact emulation of its SAH partition): an LBVH over the triangles' boxes
// in the reference's BvhNode layout and node numbering, so that every consumer of a BLAS takes it as it is.  The tree is a
// function of the input alone; its definition is in include/voidin_abi.h.  The call only enqueues:
//   1. blas_lbvh_boxes_kernel    a box per triangle (three range-checked corners folded from +-1e30), a copy of the index
//                                triples (the permutation is not in place), the count of bad indices;
//   2. vd_lbvh_sort_boxes        tlas.hip's codes of the box centres and their stable radix sort - the top level's own code;
//   3. blas_lbvh_tree_kernel     Karras' radix tree over the sorted codes (vd_lbvh_range): range, split and parent links;
//   4. blas_lbvh_fit_kernel      bottom-up from every EMITTED leaf (a radix node of <= 3 positions under a parent of > 3): the
//                                box, the number of emitted interior nodes and the height of every subtree.  The second child
//                                to arrive at a node goes on, the first leaves: nobody waits (the refit's climb and its fence-free hand-over);
//   5. blas_lbvh_number_kernel   an interior node climbs to the root: its pre-order rank among the interior nodes is its depth
//                                plus the interior counts of the left siblings of the right turns on the way, and the
//                                reference's pair allocation (blas.rs:105-128) puts its children at 2 + 2 * rank.  It writes
//                                its own node and those of its leaf children; the root writes the result;
//   6. blas_lbvh_permute_kernel  the index triples in sorted order.
// Separate launches are the synchronisation between the passes.
#include "vd_common.hpp"

namespace {

constexpr unsigned kNoParent = 0xffffffffu;
constexpr unsigned kBlock = 256u;

struct LbvhWork {
    float* tbox;            // 6 T: triangle boxes, input order
    unsigned* idx;          // 3 T: the index triples as they came
    float* ibox;            // 6 T: box of radix interior node i
    unsigned* lo;           // T: first sorted position of radix interior node i
    unsigned* hi;           // T: last
    unsigned* split;        // T: gamma - the left child ends there
    unsigned* par_int;      // T: parent << 1 | (right child) of radix interior node i; kNoParent for the root
    unsigned* par_leaf;     // T: ... of the radix leaf at sorted position j
    unsigned* meta;         // T: emitted interior nodes in the subtree of i (itself included) << 8 | height of that subtree
    unsigned* arrived;      // T
    void* sort;             // vd_lbvh_sort_bytes(T)
};
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t work_bytes(uint32_t T) { return 2 * up256(24 * (size_t)T) + up256(12 * (size_t)T) + 7 * up256(4 * (size_t)T) + vd_lbvh_sort_bytes(T); }
LbvhWork carve(void* base, uint32_t T) {
    char* p = reinterpret_cast<char*>(base);
    auto take = [&](size_t bytes) { char* q = p; p += up256(bytes); return q; };
    LbvhWork w;
    w.tbox = reinterpret_cast<float*>(take(24 * (size_t)T));
    w.idx = reinterpret_cast<unsigned*>(take(12 * (size_t)T));
    w.ibox = reinterpret_cast<float*>(take(24 * (size_t)T));
    unsigned** words[7] = {&w.lo, &w.hi, &w.split, &w.par_int, &w.par_leaf, &w.meta, &w.arrived};
    for (unsigned** a : words) *a = reinterpret_cast<unsigned*>(take(4 * (size_t)T));
    w.sort = p;
    return w;
}

struct Box3 { float mn[3], mx[3]; };
__device__ __forceinline__ Box3 box_empty() { return Box3{{1e30f, 1e30f, 1e30f}, {-1e30f, -1e30f, -1e30f}}; }
__device__ __forceinline__ void box_add(Box3& a, const float* __restrict__ six) {
#pragma unroll
    for (int q = 0; q < 3; ++q) { a.mn[q] = vd_min_to(a.mn[q], six[q]); a.mx[q] = vd_max_to(a.mx[q], six[q + 3]); }
}
// What changes hands inside the fit launch - a box, a count word - between two lanes on any two CUs, as blas_refit.hip hands
// boxes over: every word a write-through agent-scope GLOBAL (never flat) store, drained (s_waitcnt vmcnt(0)) before the
// agent-scope counter add; the lane whose add came second reads with agent-scope global loads, which bypass its L1.  No fence.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) unsigned guint;
__device__ __forceinline__ void box_store_agent(float* six, const Box3& b) {
    gfloat* w = (gfloat*)six;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        __hip_atomic_store(w + q, b.mn[q], VD_RLX_AGENT);
        __hip_atomic_store(w + 3 + q, b.mx[q], VD_RLX_AGENT);
    }
}
__device__ __forceinline__ void box_add_agent(Box3& a, float* six) {
    gfloat* w = (gfloat*)six;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        a.mn[q] = vd_min_to(a.mn[q], __hip_atomic_load(w + q, VD_RLX_AGENT));
        a.mx[q] = vd_max_to(a.mx[q], __hip_atomic_load(w + 3 + q, VD_RLX_AGENT));
    }
}
__device__ __forceinline__ void node_store(VdBvhNode* nodes, unsigned id, const float* __restrict__ six, unsigned left_first, unsigned count) {
    float4* w = reinterpret_cast<float4*>(nodes + id);
    w[0] = make_float4(six[0], six[1], six[2], __uint_as_float(left_first));
    w[1] = make_float4(six[3], six[4], six[5], __uint_as_float(count));
}

__global__ __launch_bounds__(kBlock) void blas_lbvh_boxes_kernel(const float* __restrict__ verts, unsigned n_vert, const unsigned* __restrict__ indices,
                                                                 unsigned T, float* __restrict__ tbox, unsigned* __restrict__ idx_copy,
                                                                 VdBvhLbvhResult* result) {
    const unsigned t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    Box3 b = box_empty();
    unsigned bad = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned vi = indices[3u * t + c];
        idx_copy[3u * t + c] = vi;
        if (vi >= n_vert) { ++bad; continue; }            // counts as a NaN vertex: ignored by the fold, never read
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float p = vd_quiet(verts[3u * (size_t)vi + q]);
            b.mn[q] = vd_min_to(b.mn[q], p); b.mx[q] = vd_max_to(b.mx[q], p);
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { tbox[6u * t + q] = b.mn[q]; tbox[6u * t + 3 + q] = b.mx[q]; }
    if (bad) atomicAdd(&result->n_bad_indices, bad);
}

__global__ __launch_bounds__(kBlock) void blas_lbvh_tree_kernel(const unsigned* __restrict__ keys, unsigned T, unsigned* __restrict__ rlo,
                                                                unsigned* __restrict__ rhi, unsigned* __restrict__ split, unsigned* __restrict__ par_int,
                                                                unsigned* __restrict__ par_leaf, unsigned* __restrict__ arrived) {
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x), N = (int)T;
    if (i >= N - 1) return;
    int lo, hi, gamma;
    vd_lbvh_range(keys, N, i, lo, hi, gamma);
    rlo[i] = (unsigned)lo; rhi[i] = (unsigned)hi; split[i] = (unsigned)gamma;
    const unsigned me = (unsigned)i << 1;
    if (lo == gamma) par_leaf[gamma] = me; else par_int[gamma] = me;
    if (hi == gamma + 1) par_leaf[gamma + 1] = me | 1u; else par_int[gamma + 1] = me | 1u;
    if (i == 0) par_int[0] = kNoParent;
    arrived[i] = 0u;
}

// One thread per radix leaf (g < T) and per radix interior node (g - T): those that are EMITTED leaves fold their box and climb.
__global__ __launch_bounds__(kBlock) void blas_lbvh_fit_kernel(unsigned T, const unsigned* __restrict__ vals, const float* __restrict__ tbox,
                                                               const unsigned* __restrict__ rlo, const unsigned* __restrict__ rhi,
                                                               const unsigned* __restrict__ split, const unsigned* __restrict__ par_int,
                                                               const unsigned* __restrict__ par_leaf, float* ibox, unsigned* meta, unsigned* arrived) {
    const unsigned g = blockIdx.x * kBlock + threadIdx.x;
    if (T < 2u || g >= 2u * T - 1u) return;
    Box3 b = box_empty();
    unsigned up;
    if (g < T) {                                           // the leaf at sorted position g
        up = par_leaf[g];
        const unsigned p = up >> 1;
        if (rhi[p] - rlo[p] < 3u) return;                  // inside a leaf of 2 or 3: not emitted
        box_add(b, tbox + 6u * (size_t)vals[g]);
    } else {
        const unsigned i = g - T, lo = rlo[i], hi = rhi[i];
        if (hi - lo >= 3u) return;                         // interior
        up = par_int[i];
        if (up != kNoParent) { const unsigned p = up >> 1; if (rhi[p] - rlo[p] < 3u) return; }      // a pair inside a leaf of 3
        for (unsigned j = lo; j <= hi; ++j) box_add(b, tbox + 6u * (size_t)vals[j]);
        box_store_agent(ibox + 6u * (size_t)i, b);
        __hip_atomic_store((guint*)&meta[i], 0u, VD_RLX_AGENT);
        if (up == kNoParent) return;                       // T <= 3: the root is the leaf
    }
    unsigned cnt = 0, hgt = 0;
    for (int step = 0; step < 64; ++step) {                // 62 key bits bound the depth
        const unsigned p = up >> 1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");           // no instruction: the stores stay above the add
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // my write-through box and counts have reached memory before the counter says so
        if (__hip_atomic_fetch_add((guint*)&arrived[p], 1u, VD_RLX_AGENT) == 0u) return;      // the first child to arrive leaves; the second finds both written
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");           // no instruction: the loads stay below the add
        const unsigned gm = split[p];
        const bool sib_leaf = (up & 1u) ? rlo[p] == gm : rhi[p] == gm + 1u;
        const unsigned sib = (up & 1u) ? gm : gm + 1u;     // I am the right child: the sibling ends at gamma; else it starts behind it
        if (sib_leaf) {
            box_add(b, tbox + 6u * (size_t)vals[sib]);
        } else {
            box_add_agent(b, ibox + 6u * (size_t)sib);
            const unsigned m = __hip_atomic_load((guint*)&meta[sib], VD_RLX_AGENT);
            cnt += m >> 8;
            hgt = max(hgt, m & 255u);
        }
        cnt += 1u; hgt += 1u;
        box_store_agent(ibox + 6u * (size_t)p, b);
        __hip_atomic_store((guint*)&meta[p], cnt << 8 | hgt, VD_RLX_AGENT);
        up = par_int[p];
        if (up == kNoParent) return;
    }
}

// interior nodes in the subtree of a child of p: 0 for a leaf child
__device__ __forceinline__ unsigned left_interior(const unsigned* __restrict__ rlo, const unsigned* __restrict__ split, const unsigned* __restrict__ meta, unsigned p) {
    const unsigned gm = split[p];
    return rlo[p] == gm ? 0u : meta[gm] >> 8;
}

__global__ __launch_bounds__(kBlock) void blas_lbvh_number_kernel(unsigned T, const unsigned* __restrict__ vals, const float* __restrict__ tbox,
                                                                  const unsigned* __restrict__ rlo, const unsigned* __restrict__ rhi,
                                                                  const unsigned* __restrict__ split, const unsigned* __restrict__ par_int,
                                                                  const float* __restrict__ ibox, const unsigned* __restrict__ meta,
                                                                  VdBvhNode* __restrict__ nodes, unsigned node_cap, VdBvhLbvhResult* result) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const float zero[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (T <= 3u) {                                         // node 0 is the one leaf
        if (i != 0u) return;
        node_store(nodes, 0u, T == 1u ? tbox : ibox, 0u, T);
        node_store(nodes, 1u, zero, 0u, 0u);
        result->n_nodes = 2u; result->max_depth = 0u;
        return;
    }
    if (i >= T - 1u) return;
    const unsigned lo = rlo[i], hi = rhi[i], gm = split[i];
    if (hi - lo < 3u) return;                              // a leaf, or inside one: its parent writes it
    // pre-order rank among the interior nodes: one for every ancestor, plus the interior nodes of every left sibling passed on a right turn
    unsigned rank = 0, first_step = 0;                     // first_step: what my rank has over my parent's
    unsigned k = i;
    for (int step = 0; step < 64 && k != 0u; ++step) {     // 62 key bits bound the depth
        const unsigned up = par_int[k], p = up >> 1;
        const unsigned add = 1u + ((up & 1u) ? left_interior(rlo, split, meta, p) : 0u);
        if (k == i) first_step = add;
        rank += add;
        k = p;
    }
    const unsigned id = i == 0u ? 0u : 2u + 2u * (rank - first_step) + (par_int[i] & 1u);      // my slot in my parent's pair
    const unsigned lf = 2u + 2u * rank;
    if (lf + 1u >= node_cap || id >= node_cap) return;      // cannot happen: 2 + 2 * interior <= 2 T <= node_cap; nothing is written outside whatever the work memory holds
    node_store(nodes, id, ibox + 6u * (size_t)i, lf, 0u);
    // children that are leaves
    if (lo == gm) node_store(nodes, lf, tbox + 6u * (size_t)vals[gm], gm, 1u);
    else if (rhi[gm] - rlo[gm] < 3u) node_store(nodes, lf, ibox + 6u * (size_t)gm, lo, gm - lo + 1u);
    if (hi == gm + 1u) node_store(nodes, lf + 1u, tbox + 6u * (size_t)vals[hi], hi, 1u);
    else if (rhi[gm + 1u] - rlo[gm + 1u] < 3u) node_store(nodes, lf + 1u, ibox + 6u * (size_t)(gm + 1u), gm + 1u, hi - gm);
    if (i == 0u) {
        node_store(nodes, 1u, zero, 0u, 0u);
        const unsigned m = meta[0];
        result->n_nodes = 2u + 2u * (m >> 8); result->max_depth = m & 255u;
    }
}

__global__ __launch_bounds__(kBlock) void blas_lbvh_permute_kernel(unsigned T, const unsigned* __restrict__ vals, const unsigned* __restrict__ idx_copy,
                                                                   unsigned* __restrict__ indices) {
    const unsigned p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= T) return;
    const size_t s = 3u * (size_t)vals[p];
    indices[3u * p] = idx_copy[s]; indices[3u * p + 1u] = idx_copy[s + 1u]; indices[3u * p + 2u] = idx_copy[s + 2u];
}

int check_args(VdCtx* ctx, const void* verts, const void* indices, uint32_t n_tri, const void* nodes, uint32_t node_cap) {
    if (!verts || !indices || !nodes) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: null vertices / indices / nodes");
    if (n_tri == 0u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: n_tri == 0");
    if (n_tri > VD_BVH_LBVH_MAX_TRIANGLES) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: n_tri > VD_BVH_LBVH_MAX_TRIANGLES");
    if (node_cap < (n_tri < 2u ? 2u : 2u * n_tri)) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: node_cap < max(2, 2 * n_tri)");
    return VD_OK;
}

}  // namespace

extern "C" {

int vd_bvh_build_lbvh_dev(VdCtx* ctx, const float* d_verts_xyz, uint32_t n_vert, uint32_t* d_indices_inout, uint32_t n_tri,
                          VdBvhNode* d_out_nodes, uint32_t node_cap, VdBvhLbvhResult* d_result) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx) return VD_ERR_INVALID_ARG;
    int rc = check_args(ctx, d_verts_xyz, d_indices_inout, n_tri, d_out_nodes, node_cap);
    if (rc) return rc;
    if (!d_result) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh_dev: null result");
    if ((reinterpret_cast<uintptr_t>(d_out_nodes) & 15u) != 0u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh_dev: d_out_nodes is not 16-byte aligned");
    const uint32_t T = n_tri;
    if ((rc = vd_ensure(ctx, &ctx->blas_lbvh_state, &ctx->blas_lbvh_state_bytes, work_bytes(T)))) return rc;
    const LbvhWork w = carve(ctx->blas_lbvh_state, T);
    hipStream_t st = ctx->stream;
    VD_HIP_CHECK(ctx, hipMemsetAsync(d_result, 0, sizeof(VdBvhLbvhResult), st));
    vd_time_begin(ctx);
    const unsigned grid = (T + kBlock - 1u) / kBlock;
    hipLaunchKernelGGL(blas_lbvh_boxes_kernel, dim3(grid), dim3(kBlock), 0, st, d_verts_xyz, n_vert, d_indices_inout, T, w.tbox, w.idx, d_result);
    const unsigned *keys = nullptr, *vals = nullptr;
    if ((rc = vd_lbvh_sort_boxes(ctx, w.tbox, T, w.sort, &keys, &vals))) { vd_time_end(ctx); return rc; }
    if (T >= 2u) {
        hipLaunchKernelGGL(blas_lbvh_tree_kernel, dim3(grid), dim3(kBlock), 0, st, keys, T, w.lo, w.hi, w.split, w.par_int, w.par_leaf, w.arrived);
        hipLaunchKernelGGL(blas_lbvh_fit_kernel, dim3((2u * T + kBlock - 1u) / kBlock), dim3(kBlock), 0, st, T, vals, w.tbox, w.lo, w.hi, w.split,
                           w.par_int, w.par_leaf, w.ibox, w.meta, w.arrived);
    }
    hipLaunchKernelGGL(blas_lbvh_number_kernel, dim3(grid), dim3(kBlock), 0, st, T, vals, w.tbox, w.lo, w.hi, w.split, w.par_int, w.ibox, w.meta,
                       d_out_nodes, node_cap, d_result);
    hipLaunchKernelGGL(blas_lbvh_permute_kernel, dim3(grid), dim3(kBlock), 0, st, T, vals, w.idx, d_indices_inout);
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_bvh_build_lbvh(VdCtx* ctx, const float* verts_xyz, uint32_t n_vert, uint32_t* indices_inout, uint32_t n_tri,
                      VdBvhNode* out_nodes, uint32_t node_cap, uint32_t* out_n_nodes) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx) return VD_ERR_INVALID_ARG;
    int rc = check_args(ctx, verts_xyz, indices_inout, n_tri, out_nodes, node_cap);
    if (rc) return rc;
    if (!out_n_nodes || n_vert == 0u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: null out_n_nodes or no vertices");
    const uint32_t cap = n_tri < 2u ? 2u : 2u * n_tri;
    VdBlob blobs[4] = {{verts_xyz, 12 * (size_t)n_vert, 256, nullptr}, {indices_inout, 12 * (size_t)n_tri, 256, nullptr},
                       {nullptr, sizeof(VdBvhNode) * (size_t)cap, 256, nullptr}, {nullptr, sizeof(VdBvhLbvhResult), 256, nullptr}};
    if ((rc = vd_stage_blobs(ctx, blobs, 4))) return rc;
    rc = vd_bvh_build_lbvh_dev(ctx, static_cast<const float*>(blobs[0].dev), n_vert, static_cast<uint32_t*>(blobs[1].dev), n_tri,
                               static_cast<VdBvhNode*>(blobs[2].dev), cap, static_cast<VdBvhLbvhResult*>(blobs[3].dev));
    if (rc) return rc;
    VdBvhLbvhResult res;
    if ((rc = vd_fetch_blob(ctx, &res, &blobs[3]))) return rc;
    if (res.n_bad_indices != 0u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: an index >= n_vert");
    if (res.n_nodes > cap) VD_FAIL(ctx, VD_ERR_HIP, "vd_bvh_build_lbvh: implausible node count");
    blobs[2].bytes = sizeof(VdBvhNode) * (size_t)res.n_nodes;
    if ((rc = vd_fetch_blob(ctx, out_nodes, &blobs[2]))) return rc;
    if ((rc = vd_fetch_blob(ctx, indices_inout, &blobs[1]))) return rc;
    *out_n_nodes = res.n_nodes;
    return VD_OK;
}

}  // extern "C"
