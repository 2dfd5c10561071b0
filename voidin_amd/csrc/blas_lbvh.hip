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
//
// VD_OPT_BLAS_LBVH_MAX_DEPTH = D >= 1 (voidin_abi.h: the depth-bounded topology) adds two passes behind pass 3, over work memory
// that is taken only then:
//   3b. blas_lbvh_bound_kernel   a sorted position climbs the radix tree twice - once to count its ancestors, which gives every
//                                ancestor's depth, once to find the TOPMOST one whose Karras split breaks d + 1 + needr(larger
//                                child) <= D, its switch node - and writes an explicit 64-bit key: (code, position) under no
//                                switch node, else (the codes' common prefix under the switch node, position - its first position),
//                                the low word behind the positions' common prefix where the codes are all equal;
//   3c. blas_lbvh_tree_kernel    again, over those keys (vd_lbvh_range with the low word from an array): above the switch nodes
//                                the tree is what it was, below one it is the radix tree of the relative positions.
// Passes 4 - 6 run as they are.  D == 0: none of this is launched, allocated or passed.
//
// vd_bvh_lbvh_plan_dev / vd_bvh_build_lbvh_planned_dev build MANY meshes with the same six passes, each run once over one slot space
// in which every mesh owns a run of 256-slot units, through the same per-mesh __device__ bodies; the sort is tlas.hip's segmented
// variant (vd_lbvh_batch_sort_boxes).  Every mesh's triangle count is read from device memory by every pass, so the launches -
// 19 or 23 kernels (21 or 25 for a plan made under VD_OPT_BLAS_LBVH_MAX_DEPTH), no memset, one more kernel for VdMeshInfo bounds - are
// the same whatever the counts are ("the batched build" below).
//
// The host side: vd_bvh_lbvh_plan_dev is judge and derive (blas_lbvh_plan.hpp: pure host arithmetic, tested without a GPU by
// tests/cpp/blas_lbvh_plan_test.cpp) -> upload (plan_upload: vd_plan_tables, ctx.hip - one allocation, tables then work memory)
// -> the plan struct.  The host-pointer forms vd_bvh_build_lbvh and vd_bvh_build_lbvh_batch stage in the context's one arena
// (vd_stage_blobs / vd_fetch_blob(s), ctx.hip); the batch comes back through batch_fetch.  profiles/blas_lbvh_host_layer.md.
#include "vd_common.hpp"
#include "blas_lbvh_plan.hpp"

#include <new>
#include <vector>

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
struct LbvhKeys {           // the depth-bounded build only: the explicit 64-bit key of every sorted position
    unsigned* hi;           // T
    unsigned* low;          // T
};
// The arrays over T positions (a mesh's triangles, a plan's slots) at `base`, each 256-byte aligned, the sort's work memory last.
// base == null: only sizes them.  *sort_at = the bytes in front of the sort's.
LbvhWork carve(void* base, size_t T, LbvhKeys* bounded /* null: the unbounded build's layout */, size_t* sort_at = nullptr) {
    Arena a{reinterpret_cast<char*>(base), 0};
    LbvhWork w;
    w.tbox = a.take<float>(6 * T);
    w.idx = a.take<unsigned>(3 * T);
    w.ibox = a.take<float>(6 * T);
    unsigned** words[7] = {&w.lo, &w.hi, &w.split, &w.par_int, &w.par_leaf, &w.meta, &w.arrived};
    for (unsigned** arr : words) *arr = a.take<unsigned>(T);
    if (bounded) { bounded->hi = a.take<unsigned>(T); bounded->low = a.take<unsigned>(T); }
    w.sort = a.take<char>(0);
    if (sort_at) *sort_at = a.off;
    return w;
}
size_t work_bytes(uint32_t T, bool bounded, size_t sort_bytes /* vd_lbvh_sort_bytes(T), or the batched sort's */) {
    LbvhKeys k;
    size_t sort_at = 0;
    (void)carve(nullptr, T, bounded ? &k : nullptr, &sort_at);
    return sort_at + sort_bytes;
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

// The per-mesh bodies of the six passes: what one thread does for ONE mesh, given that mesh's arrays.  The single-mesh kernels
// call them with the thread's index in the grid, the batched ones (below) with the slot's position inside its mesh.
__device__ __forceinline__ void boxes_body(unsigned t, const float* __restrict__ verts, unsigned n_vert, const unsigned* __restrict__ indices,
                                           float* __restrict__ tbox, unsigned* __restrict__ idx_copy, unsigned* n_bad) {
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
    if (bad) atomicAdd(n_bad, bad);
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_boxes_kernel(const float* __restrict__ verts, unsigned n_vert, const unsigned* __restrict__ indices,
                                                                 unsigned T, float* __restrict__ tbox, unsigned* __restrict__ idx_copy,
                                                                 VdBvhLbvhResult* result) {
    const unsigned t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    boxes_body(t, verts, n_vert, indices, tbox, idx_copy, &result->n_bad_indices);
}

template <typename Low>
__device__ __forceinline__ void tree_body(int i, const unsigned* __restrict__ keys, Low low, unsigned T, unsigned* __restrict__ rlo,
                                          unsigned* __restrict__ rhi, unsigned* __restrict__ split, unsigned* __restrict__ par_int,
                                          unsigned* __restrict__ par_leaf, unsigned* __restrict__ arrived) {
    const int N = (int)T;
    if (i >= N - 1) return;
    int lo, hi, gamma;
    vd_lbvh_range(keys, low, N, i, lo, hi, gamma);
    rlo[i] = (unsigned)lo; rhi[i] = (unsigned)hi; split[i] = (unsigned)gamma;
    const unsigned me = (unsigned)i << 1;
    if (lo == gamma) par_leaf[gamma] = me; else par_int[gamma] = me;
    if (hi == gamma + 1) par_leaf[gamma + 1] = me | 1u; else par_int[gamma + 1] = me | 1u;
    if (i == 0) par_int[0] = kNoParent;
    arrived[i] = 0u;
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_tree_kernel(const unsigned* __restrict__ keys, unsigned T, unsigned* __restrict__ rlo,
                                                                unsigned* __restrict__ rhi, unsigned* __restrict__ split, unsigned* __restrict__ par_int,
                                                                unsigned* __restrict__ par_leaf, unsigned* __restrict__ arrived) {
    tree_body((int)(blockIdx.x * kBlock + threadIdx.x), keys, VdLbvhLowIsPosition{}, T, rlo, rhi, split, par_int, par_leaf, arrived);
}

// ---- the depth bound (VD_OPT_BLAS_LBVH_MAX_DEPTH) --------------------------------------------------------------------------------
// (needr, the depth of the radix tree over the integers 0 .. k - 1 cut off at nodes of <= 3 positions: blas_lbvh_plan.hpp)
// One thread per sorted position p < T of a mesh of T >= 2: the explicit key of that position.  Every ancestor of the radix leaf
// covers > 3 positions or lies inside an emitted leaf; only the former have a split to judge, and those are the emitted interior
// nodes, so the radix depth of one is its depth in the array.  The ancestors BELOW the topmost rule-breaker belong to a subtree that
// the second tree pass replaces: they are looked at for the same test only, and the topmost one wins.
__device__ __forceinline__ void bound_body(unsigned p, unsigned T, unsigned D, const unsigned* __restrict__ keys, const unsigned* __restrict__ rlo,
                                           const unsigned* __restrict__ rhi, const unsigned* __restrict__ split, const unsigned* __restrict__ par_int,
                                           const unsigned* __restrict__ par_leaf, unsigned* __restrict__ key_hi, unsigned* __restrict__ key_low) {
    const unsigned code = keys[p];
    unsigned hw = code, lw = p;
    if (T > 3u) {
        const unsigned first = par_leaf[p] >> 1;
        unsigned len = 1u;                                  // ancestors of the leaf, the root included: 62 key bits bound them
        for (unsigned k = first; k != 0u && len < 64u; ++len) k = par_int[k] >> 1;
        unsigned c = kNoParent, k = first;
        for (unsigned j = 0; j < len; ++j) {               // ancestor j from below is at depth len - 1 - j
            const unsigned lo = rlo[k], hi = rhi[k];
            if (hi - lo >= 3u) {
                const unsigned gm = split[k];
                if (len - j + needr(max(gm - lo + 1u, hi - gm)) > D) c = k;      // depth + 1 + needr(larger child) > D
            }
            k = par_int[k] >> 1;                           // (of the root: not used)
        }
        if (c != kNoParent) {
            const unsigned lo = rlo[c], hi = rhi[c], cl = keys[lo], ch = keys[hi];
            lw = p - lo;
            if (cl != ch) {                                 // the end keys share delta = clz < 32 bits, all of the code
                hw = code & ~(0xffffffffu >> __clz((int)(cl ^ ch)));
            } else {                                       // ... 32 + clz(lo ^ hi): one code, and the positions' common prefix stays
                const unsigned sh = 32u - (unsigned)__clz((int)(lo ^ hi));       // 64 - delta; hi - lo >= 3: lo != hi
                if (sh < 32u) lw |= lo >> sh << sh;
            }
        }
    }
    key_hi[p] = hw; key_low[p] = lw;
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_bound_kernel(unsigned T, unsigned D, const unsigned* __restrict__ keys, const unsigned* __restrict__ rlo,
                                                                 const unsigned* __restrict__ rhi, const unsigned* __restrict__ split,
                                                                 const unsigned* __restrict__ par_int, const unsigned* __restrict__ par_leaf,
                                                                 unsigned* __restrict__ key_hi, unsigned* __restrict__ key_low) {
    const unsigned p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= T) return;
    bound_body(p, T, D, keys, rlo, rhi, split, par_int, par_leaf, key_hi, key_low);
}
// the tree pass over explicit keys: every link, range and arrival word of the first one is written again
__global__ __launch_bounds__(kBlock) void blas_lbvh_tree_keys_kernel(const unsigned* __restrict__ key_hi, const unsigned* __restrict__ key_low, unsigned T,
                                                                     unsigned* __restrict__ rlo, unsigned* __restrict__ rhi, unsigned* __restrict__ split,
                                                                     unsigned* __restrict__ par_int, unsigned* __restrict__ par_leaf, unsigned* __restrict__ arrived) {
    tree_body((int)(blockIdx.x * kBlock + threadIdx.x), key_hi, VdLbvhLowArray{key_low}, T, rlo, rhi, split, par_int, par_leaf, arrived);
}

// One thread per radix leaf (g < T) and per radix interior node (g - T): those that are EMITTED leaves fold their box and climb.
__device__ __forceinline__ void fit_body(unsigned g, unsigned T, const unsigned* __restrict__ vals, const float* __restrict__ tbox,
                                         const unsigned* __restrict__ rlo, const unsigned* __restrict__ rhi,
                                         const unsigned* __restrict__ split, const unsigned* __restrict__ par_int,
                                         const unsigned* __restrict__ par_leaf, float* ibox, unsigned* meta, unsigned* arrived) {
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
__global__ __launch_bounds__(kBlock) void blas_lbvh_fit_kernel(unsigned T, const unsigned* __restrict__ vals, const float* __restrict__ tbox,
                                                               const unsigned* __restrict__ rlo, const unsigned* __restrict__ rhi,
                                                               const unsigned* __restrict__ split, const unsigned* __restrict__ par_int,
                                                               const unsigned* __restrict__ par_leaf, float* ibox, unsigned* meta, unsigned* arrived) {
    fit_body(blockIdx.x * kBlock + threadIdx.x, T, vals, tbox, rlo, rhi, split, par_int, par_leaf, ibox, meta, arrived);
}

// interior nodes in the subtree of a child of p: 0 for a leaf child
__device__ __forceinline__ unsigned left_interior(const unsigned* __restrict__ rlo, const unsigned* __restrict__ split, const unsigned* __restrict__ meta, unsigned p) {
    const unsigned gm = split[p];
    return rlo[p] == gm ? 0u : meta[gm] >> 8;
}

__device__ __forceinline__ void number_body(unsigned i, unsigned T, const unsigned* __restrict__ vals, const float* __restrict__ tbox,
                                            const unsigned* __restrict__ rlo, const unsigned* __restrict__ rhi,
                                            const unsigned* __restrict__ split, const unsigned* __restrict__ par_int,
                                            const float* __restrict__ ibox, const unsigned* __restrict__ meta,
                                            VdBvhNode* __restrict__ nodes, unsigned node_cap, VdBvhLbvhResult* result) {
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
__global__ __launch_bounds__(kBlock) void blas_lbvh_number_kernel(unsigned T, const unsigned* __restrict__ vals, const float* __restrict__ tbox,
                                                                  const unsigned* __restrict__ rlo, const unsigned* __restrict__ rhi,
                                                                  const unsigned* __restrict__ split, const unsigned* __restrict__ par_int,
                                                                  const float* __restrict__ ibox, const unsigned* __restrict__ meta,
                                                                  VdBvhNode* __restrict__ nodes, unsigned node_cap, VdBvhLbvhResult* result) {
    number_body(blockIdx.x * kBlock + threadIdx.x, T, vals, tbox, rlo, rhi, split, par_int, ibox, meta, nodes, node_cap, result);
}

__device__ __forceinline__ void permute_body(unsigned p, const unsigned* __restrict__ vals, const unsigned* __restrict__ idx_copy,
                                             unsigned* __restrict__ indices) {
    const size_t s = 3u * (size_t)vals[p];
    indices[3u * p] = idx_copy[s]; indices[3u * p + 1u] = idx_copy[s + 1u]; indices[3u * p + 2u] = idx_copy[s + 2u];
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_permute_kernel(unsigned T, const unsigned* __restrict__ vals, const unsigned* __restrict__ idx_copy,
                                                                   unsigned* __restrict__ indices) {
    const unsigned p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= T) return;
    permute_body(p, vals, idx_copy, indices);
}

// ---- the batched build (vd_bvh_lbvh_plan_dev / vd_bvh_build_lbvh_planned_dev) ---------------------------------------------------
// All meshes of a plan lie in ONE slot space: item m owns the slots [slot0, slot0 + n_units * 256), n_units = ceil(tri_cap / 256), so
// a 256-thread block (and a unit of the segmented sort, tlas.hip) never spans two meshes and the mesh of a block is one scalar
// load.  Every array of LbvhWork is laid out over the slots; a mesh's part of it starts at slot0 and is what the single build's
// array is for that mesh: positions, radix node ids and vals are mesh-local.  T_m = min(d_n_tri[m], tri_cap) is read on the
// device by every pass; a lane whose position is beyond T_m leaves.  Grids come from the slot count alone.
// (BatchItemDev, a mesh's pointers and sizes: blas_lbvh_plan.hpp, which fills it)
struct BatchSlot { unsigned m, j, T, slot0; };           // the mesh of this thread's slot, its position in it, the mesh's count
__device__ __forceinline__ BatchSlot batch_slot(unsigned unit, const VdLbvhSeg* __restrict__ segs, const unsigned* __restrict__ unit_seg,
                                                const unsigned* __restrict__ n_tri) {
    BatchSlot b;
    b.m = unit_seg[unit];
    const VdLbvhSeg sg = segs[b.m];
    b.slot0 = sg.slot0;
    b.j = unit * kBlock + threadIdx.x - sg.slot0;
    b.T = vd_lbvh_seg_count(sg, n_tri, b.m);
    return b;
}
static_assert(kBlock == kVdLbvhBatchUnit, "a block is a unit of the slot space");

__global__ __launch_bounds__(kBlock) void blas_lbvh_batch_boxes_kernel(const BatchItemDev* __restrict__ items, const VdLbvhSeg* __restrict__ segs,
                                                                       const unsigned* __restrict__ unit_seg, const unsigned* __restrict__ n_tri,
                                                                       float* __restrict__ tbox, unsigned* __restrict__ idx_copy, unsigned* __restrict__ ext,
                                                                       unsigned* n_bad /* per mesh, the plan's: 0 between builds */) {
    const BatchSlot b = batch_slot(blockIdx.x, segs, unit_seg, n_tri);
    if (b.j == 0u) {                                       // the mesh's extent words start from the neutral elements (read by the NEXT launch)
#pragma unroll
        for (int q = 0; q < 3; ++q) { ext[6u * b.m + q] = 0xffffffffu; ext[6u * b.m + 3 + q] = 0u; }
    }
    if (b.j >= b.T) return;
    const BatchItemDev it = items[b.m];
    boxes_body(b.j, it.verts, it.n_vert, it.indices, tbox + 6u * (size_t)b.slot0, idx_copy + 3u * (size_t)b.slot0, n_bad + b.m);
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_batch_tree_kernel(const VdLbvhSeg* __restrict__ segs, const unsigned* __restrict__ unit_seg,
                                                                      const unsigned* __restrict__ n_tri, const unsigned* __restrict__ keys, LbvhWork w) {
    const BatchSlot b = batch_slot(blockIdx.x, segs, unit_seg, n_tri);
    if (b.j + 1u >= b.T) return;                           // interior nodes 0 .. T - 2
    tree_body((int)b.j, keys + b.slot0, VdLbvhLowIsPosition{}, b.T, w.lo + b.slot0, w.hi + b.slot0, w.split + b.slot0, w.par_int + b.slot0,
              w.par_leaf + b.slot0, w.arrived + b.slot0);
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_batch_bound_kernel(const VdLbvhSeg* __restrict__ segs, const unsigned* __restrict__ unit_seg,
                                                                       const unsigned* __restrict__ n_tri, const unsigned* __restrict__ keys, unsigned D,
                                                                       LbvhWork w, LbvhKeys k) {
    const BatchSlot b = batch_slot(blockIdx.x, segs, unit_seg, n_tri);
    if (b.T < 2u || b.j >= b.T) return;
    bound_body(b.j, b.T, D, keys + b.slot0, w.lo + b.slot0, w.hi + b.slot0, w.split + b.slot0, w.par_int + b.slot0, w.par_leaf + b.slot0,
               k.hi + b.slot0, k.low + b.slot0);
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_batch_tree_keys_kernel(const VdLbvhSeg* __restrict__ segs, const unsigned* __restrict__ unit_seg,
                                                                           const unsigned* __restrict__ n_tri, LbvhWork w, LbvhKeys k) {
    const BatchSlot b = batch_slot(blockIdx.x, segs, unit_seg, n_tri);
    if (b.j + 1u >= b.T) return;
    tree_body((int)b.j, k.hi + b.slot0, VdLbvhLowArray{k.low + b.slot0}, b.T, w.lo + b.slot0, w.hi + b.slot0, w.split + b.slot0, w.par_int + b.slot0,
              w.par_leaf + b.slot0, w.arrived + b.slot0);
}
// blocks [0, n_units): the radix leaves; blocks [n_units, 2 n_units): the radix interior nodes
__global__ __launch_bounds__(kBlock) void blas_lbvh_batch_fit_kernel(unsigned n_units, const VdLbvhSeg* __restrict__ segs, const unsigned* __restrict__ unit_seg,
                                                                     const unsigned* __restrict__ n_tri, const unsigned* __restrict__ vals, LbvhWork w) {
    const bool interior = blockIdx.x >= n_units;
    const BatchSlot b = batch_slot(interior ? blockIdx.x - n_units : blockIdx.x, segs, unit_seg, n_tri);
    if (b.T < 2u || b.j + (interior ? 1u : 0u) >= b.T) return;
    fit_body(interior ? b.T + b.j : b.j, b.T, vals + b.slot0, w.tbox + 6u * (size_t)b.slot0, w.lo + b.slot0, w.hi + b.slot0, w.split + b.slot0,
             w.par_int + b.slot0, w.par_leaf + b.slot0, w.ibox + 6u * (size_t)b.slot0, w.meta + b.slot0, w.arrived + b.slot0);
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_batch_number_kernel(const BatchItemDev* __restrict__ items, const VdLbvhSeg* __restrict__ segs,
                                                                        const unsigned* __restrict__ unit_seg, const unsigned* __restrict__ n_tri,
                                                                        const unsigned* __restrict__ vals, LbvhWork w, VdBvhLbvhResult* results) {
    const BatchSlot b = batch_slot(blockIdx.x, segs, unit_seg, n_tri);
    if (b.j >= b.T) return;                                // T == 0: no node, the result stays all zero
    const BatchItemDev it = items[b.m];
    number_body(b.j, b.T, vals + b.slot0, w.tbox + 6u * (size_t)b.slot0, w.lo + b.slot0, w.hi + b.slot0, w.split + b.slot0, w.par_int + b.slot0,
                w.ibox + 6u * (size_t)b.slot0, w.meta + b.slot0, it.nodes, it.node_cap, results + b.m);
}
__global__ __launch_bounds__(kBlock) void blas_lbvh_batch_permute_kernel(const BatchItemDev* __restrict__ items, const VdLbvhSeg* __restrict__ segs,
                                                                         const unsigned* __restrict__ unit_seg, const unsigned* __restrict__ n_tri,
                                                                         const unsigned* __restrict__ vals, const unsigned* __restrict__ idx_copy,
                                                                         unsigned* n_bad, VdBvhLbvhResult* results) {
    const BatchSlot b = batch_slot(blockIdx.x, segs, unit_seg, n_tri);
    if (b.j == 0u) {                                       // every mesh has this slot, whatever T: the rest of its result, and the count re-armed
        results[b.m].n_bad_indices = n_bad[b.m]; n_bad[b.m] = 0u;
        results[b.m]._pad = 0u;
        if (b.T == 0u) { results[b.m].n_nodes = 0u; results[b.m].max_depth = 0u; }      // otherwise: blas_lbvh_batch_number_kernel's, a launch ago
    }
    if (b.j >= b.T) return;
    permute_body(b.j, vals + b.slot0, idx_copy + 3u * (size_t)b.slot0, items[b.m].indices);
}
// VdMeshInfo.min / max of every item that carries one: a block per chunk {item, first vertex} (vd_common.hpp: vd_mesh_bounds_fold)
__global__ __launch_bounds__(kBlock) void blas_lbvh_batch_bounds_kernel(const BatchItemDev* __restrict__ items, const uint2* __restrict__ chunks, int* keys,
                                                                        unsigned* done) {
    const uint2 ch = chunks[blockIdx.x];
    const BatchItemDev it = items[ch.x];
    vd_mesh_bounds_fold(it.verts, it.n_vert, it.info, it.n_chunks, ch.y, keys + 6u * ch.x, done + ch.x);
}

int fail_item(VdCtx* ctx, VdBvhLbvhBatchItem* items, uint32_t m, const char* what) {
    items[m].status = VD_ERR_INVALID_ARG;
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "vd_bvh_lbvh_plan: item %u: %s", m, what);
    return VD_ERR_INVALID_ARG;
}

}  // namespace

struct VdBvhLbvhPlan {
    unsigned n_items = 0, n_slots = 0, n_bound_chunks = 0;
    void* dev = nullptr;                                   // ONE allocation: the tables, then the work memory
    BatchItemDev* d_items = nullptr;
    uint2* d_bound_chunks = nullptr;                       // per block of the MeshInfo fold: {item, first vertex}
    int* d_bound_keys = nullptr;                           // per item: 3 min keys, 3 max keys, neutral between builds
    unsigned* d_bound_done = nullptr;                      // per item: 0 between builds
    unsigned* d_bad = nullptr;                             // per item: indices >= n_vert counted by the boxes pass; 0 between builds
    VdLbvhBatchLayout layout = {};
    LbvhWork w = {};
    unsigned max_depth = 0;                                // VD_OPT_BLAS_LBVH_MAX_DEPTH as it was when the plan was made; 0: unbounded
    LbvhKeys k = {};                                       // ... and the explicit keys, when it is not
};

namespace {

// VD_OPT_BLAS_LBVH_MAX_DEPTH as the builds read it: 0 = unbounded (the default), at most 62
unsigned depth_bound(const VdCtx* ctx) {
    const long long d = ctx->option(VD_OPT_BLAS_LBVH_MAX_DEPTH, 0);
    return (unsigned)(d > 62 ? 62 : d);
}

// The upload of a plan: its tables (blas_lbvh_plan.hpp) and the work memory over its slots in ONE allocation, the plan's pointers
// into it.  What is not uploaded starts as zeros: the extent words are set by the boxes pass, the fold's done counters and the
// bad-index counts start at 0 and come back to 0 after every build.
static_assert(sizeof(VdPair) == sizeof(uint2), "chunk records are uploaded where the kernels read uint2");
int plan_upload(VdCtx* ctx, const LbvhPlanTables& t, VdBvhLbvhPlan* p) {
    const size_t n = t.items.size();
    const std::vector<int> keys = vd_fold_neutral_keys(n);
    enum { kItems, kSegs, kUnitSeg, kExtChunks, kExt, kBoundChunks, kBoundKeys, kBoundDone, kBad, kParts };
    VdPlanPart part[kParts] = {{t.items.data(), sizeof(BatchItemDev) * n, nullptr},
                               {t.segs.data(), sizeof(VdLbvhSeg) * n, nullptr},
                               {t.unit_seg.data(), 4 * t.unit_seg.size(), nullptr},
                               {t.ext_chunks.data(), sizeof(VdPair) * t.ext_chunks.size(), nullptr},
                               {nullptr, 24 * n, nullptr},
                               {t.bound_chunks.data(), sizeof(VdPair) * t.bound_chunks.size(), nullptr},
                               {keys.data(), 4 * keys.size(), nullptr},
                               {nullptr, 4 * n, nullptr},
                               {nullptr, 4 * n, nullptr}};
    const bool bounded = p->max_depth != 0u;
    void* work = nullptr;
    const int rc = vd_plan_tables(ctx, "vd_bvh_lbvh_plan", part, kParts, work_bytes(p->n_slots, bounded, vd_lbvh_batch_sort_bytes(p->n_slots)), &p->dev, &work);
    if (rc) return rc;
    p->d_items = static_cast<BatchItemDev*>(part[kItems].dev);
    p->d_bound_chunks = static_cast<uint2*>(part[kBoundChunks].dev);
    p->d_bound_keys = static_cast<int*>(part[kBoundKeys].dev);
    p->d_bound_done = static_cast<unsigned*>(part[kBoundDone].dev);
    p->d_bad = static_cast<unsigned*>(part[kBad].dev);
    p->layout.d_segs = static_cast<const VdLbvhSeg*>(part[kSegs].dev);
    p->layout.d_unit_seg = static_cast<const unsigned*>(part[kUnitSeg].dev);
    p->layout.d_chunks = static_cast<const uint2*>(part[kExtChunks].dev);
    p->layout.d_ext = static_cast<unsigned*>(part[kExt].dev);
    p->w = carve(work, p->n_slots, bounded ? &p->k : nullptr);      // .sort: vd_lbvh_batch_sort_bytes(n_slots)
    return VD_OK;
}

// The host batch's staging (vd_bvh_build_lbvh_batch): every item's blobs in this order, those of item m from kItemBlobs * m on.
enum { kBlobVerts, kBlobIndices, kBlobNodes /* room for node_cap */, kBlobInfo /* no bytes where the item has no VdMeshInfo */, kItemBlobs };

// ... and its way back, the results being on the host: a bad index or an implausible count in any item and nothing is copied;
// else every item's n_nodes nodes, 3 * T_m indices and VdMeshInfo behind one drain.
int batch_fetch(VdCtx* ctx, VdBvhLbvhBatchItem* items, uint32_t n_items, const uint32_t* n_tri, const VdBvhLbvhResult* results, VdBlob* blobs, void** hosts) {
    int rc = VD_OK;
    for (uint32_t m = 0; m < n_items; ++m)
        if (results[m].n_bad_indices != 0u) { rc = fail_item(ctx, items, m, "an index >= n_vert"); }
        else if (results[m].n_nodes > items[m].node_cap) { rc = VD_ERR_HIP; snprintf(ctx->err, sizeof(ctx->err), "vd_bvh_build_lbvh_batch: implausible node count"); }
    if (rc) return rc;
    for (uint32_t m = 0; m < n_items; ++m) {
        const VdBvhLbvhBatchItem& it = items[m];
        const uint32_t T = n_tri ? (n_tri[m] < it.tri_cap ? n_tri[m] : it.tri_cap) : it.tri_cap;
        VdBlob* b = blobs + kItemBlobs * (size_t)m;
        void** h = hosts + kItemBlobs * (size_t)m;
        b[kBlobNodes].bytes = sizeof(VdBvhNode) * (size_t)results[m].n_nodes; h[kBlobNodes] = it.nodes;
        b[kBlobIndices].bytes = 12 * (size_t)T; h[kBlobIndices] = it.indices_inout;
        h[kBlobInfo] = it.mesh_info;                       // (no bytes where there is none)
    }
    return vd_fetch_blobs(ctx, hosts, blobs, kItemBlobs * n_items);
}

int check_args(VdCtx* ctx, const void* verts, const void* indices, uint32_t n_tri, const void* nodes, uint32_t node_cap) {
    if (!verts || !indices || !nodes) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: null vertices / indices / nodes");
    if (n_tri == 0u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: n_tri == 0");
    if (n_tri > VD_BVH_LBVH_MAX_TRIANGLES) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: n_tri > VD_BVH_LBVH_MAX_TRIANGLES");
    if (node_cap < (n_tri < 2u ? 2u : 2u * n_tri)) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh: node_cap < max(2, 2 * n_tri)");
    const unsigned D = depth_bound(ctx);
    if (D && needr(n_tri) > D) {
        snprintf(ctx->err, sizeof(ctx->err), "vd_bvh_build_lbvh: VD_OPT_BLAS_LBVH_MAX_DEPTH = %u cannot hold %u triangles: the smallest bound that can is %u",
                 D, n_tri, needr(n_tri));
        return VD_ERR_INVALID_ARG;
    }
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
    const unsigned D = depth_bound(ctx);
    if ((rc = vd_ensure(ctx, &ctx->blas_lbvh_state, &ctx->blas_lbvh_state_bytes, work_bytes(T, D != 0u, vd_lbvh_sort_bytes(T))))) return rc;
    LbvhKeys k = {};
    const LbvhWork w = carve(ctx->blas_lbvh_state, T, D ? &k : nullptr);
    hipStream_t st = ctx->stream;
    VD_HIP_CHECK(ctx, hipMemsetAsync(d_result, 0, sizeof(VdBvhLbvhResult), st));
    vd_time_begin(ctx);
    const unsigned grid = (T + kBlock - 1u) / kBlock;
    hipLaunchKernelGGL(blas_lbvh_boxes_kernel, dim3(grid), dim3(kBlock), 0, st, d_verts_xyz, n_vert, d_indices_inout, T, w.tbox, w.idx, d_result);
    const unsigned *keys = nullptr, *vals = nullptr;
    if ((rc = vd_lbvh_sort_boxes(ctx, w.tbox, T, w.sort, &keys, &vals))) { vd_time_end(ctx); return rc; }
    if (T >= 2u) {
        hipLaunchKernelGGL(blas_lbvh_tree_kernel, dim3(grid), dim3(kBlock), 0, st, keys, T, w.lo, w.hi, w.split, w.par_int, w.par_leaf, w.arrived);
        if (D && T > 3u) {                                 // (a mesh of <= 3 triangles is one leaf under any bound)
            hipLaunchKernelGGL(blas_lbvh_bound_kernel, dim3(grid), dim3(kBlock), 0, st, T, D, keys, w.lo, w.hi, w.split, w.par_int, w.par_leaf, k.hi, k.low);
            hipLaunchKernelGGL(blas_lbvh_tree_keys_kernel, dim3(grid), dim3(kBlock), 0, st, k.hi, k.low, T, w.lo, w.hi, w.split, w.par_int, w.par_leaf,
                               w.arrived);
        }
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

int vd_bvh_lbvh_plan_release(VdCtx* ctx, VdBvhLbvhPlan* plan) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !plan) return VD_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(ctx->stream);               // a queued build still uses the plan's memory
    vd_plan_free(plan->dev);
    delete plan;
    return VD_OK;
}

int vd_bvh_lbvh_plan_dev(VdCtx* ctx, VdBvhLbvhBatchItem* items, uint32_t n_items, VdBvhLbvhPlan** out) {
    VdDeviceGuard vd_guard_(ctx);
    if (!out) return VD_ERR_INVALID_ARG;
    *out = nullptr;
    if ((n_items && !items) || n_items > VD_BVH_LBVH_BATCH_MAX_ITEMS) {
        if (ctx) snprintf(ctx->err, sizeof(ctx->err), "vd_bvh_lbvh_plan: null item array, or n_items > VD_BVH_LBVH_BATCH_MAX_ITEMS");
        return VD_ERR_INVALID_ARG;
    }
    const unsigned D = ctx ? depth_bound(ctx) : 0u;        // latched: the plan's memory and launch list follow it, later changes of the option do not
    VdBvhLbvhPlan* p = nullptr;
    try {
        // judge and derive (blas_lbvh_plan.hpp): the items are judged without a context - nothing here touches the device
        LbvhPlanTables t;
        uint32_t failed = 0;
        char buf[kLbvhWhatLen];
        if (const char* what = lbvh_plan_tables(items, n_items, D, t, &failed, buf)) return fail_item(ctx, items, failed, what);
        if (!ctx) return VD_ERR_INVALID_ARG;
        p = new VdBvhLbvhPlan();
        p->n_items = n_items; p->n_slots = (unsigned)t.n_slots; p->n_bound_chunks = (unsigned)t.bound_chunks.size();
        p->max_depth = D;
        p->layout.n_slots = p->n_slots; p->layout.n_chunks = (unsigned)t.ext_chunks.size();
        const int rc = n_items ? plan_upload(ctx, t, p) : VD_OK;
        if (rc) { delete p; return rc; }                   // no plan is returned after a refusal
    } catch (const std::bad_alloc&) {
        delete p;
        if (!ctx) return VD_ERR_OOM;
        VD_FAIL(ctx, VD_ERR_OOM, "vd_bvh_lbvh_plan: host memory");
    }
    *out = p;
    return VD_OK;
}

int vd_bvh_build_lbvh_planned_dev(VdCtx* ctx, const VdBvhLbvhPlan* plan, const uint32_t* d_n_tri, VdBvhLbvhResult* d_results) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!plan || !d_results) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh_planned: null plan / results");
    if (plan->n_items == 0u) return VD_OK;
    const VdLbvhBatchLayout& L = plan->layout;
    const LbvhWork& w = plan->w;
    const unsigned n_units = L.n_slots / kBlock;
    hipStream_t st = ctx->stream;
    // No memset of d_results: every word of a result is stored by a kernel (the last pass completes it and re-arms the plan's
    // bad-index count), so a captured call is kernels only - a memset node of a HIP graph was seen to fill with other bytes than
    // it was given from the second replay on (profiles/blas_lbvh_batch.md).
    vd_time_begin(ctx);
    hipLaunchKernelGGL(blas_lbvh_batch_boxes_kernel, dim3(n_units), dim3(kBlock), 0, st, plan->d_items, L.d_segs, L.d_unit_seg, d_n_tri, w.tbox, w.idx, L.d_ext,
                       plan->d_bad);
    const unsigned *keys = nullptr, *vals = nullptr;
    int rc;
    if ((rc = vd_lbvh_batch_sort_boxes(ctx, w.tbox, &L, d_n_tri, w.sort, &keys, &vals))) { vd_time_end(ctx); return rc; }
    hipLaunchKernelGGL(blas_lbvh_batch_tree_kernel, dim3(n_units), dim3(kBlock), 0, st, L.d_segs, L.d_unit_seg, d_n_tri, keys, w);
    if (plan->max_depth) {
        hipLaunchKernelGGL(blas_lbvh_batch_bound_kernel, dim3(n_units), dim3(kBlock), 0, st, L.d_segs, L.d_unit_seg, d_n_tri, keys, plan->max_depth, w, plan->k);
        hipLaunchKernelGGL(blas_lbvh_batch_tree_keys_kernel, dim3(n_units), dim3(kBlock), 0, st, L.d_segs, L.d_unit_seg, d_n_tri, w, plan->k);
    }
    hipLaunchKernelGGL(blas_lbvh_batch_fit_kernel, dim3(2u * n_units), dim3(kBlock), 0, st, n_units, L.d_segs, L.d_unit_seg, d_n_tri, vals, w);
    hipLaunchKernelGGL(blas_lbvh_batch_number_kernel, dim3(n_units), dim3(kBlock), 0, st, plan->d_items, L.d_segs, L.d_unit_seg, d_n_tri, vals, w, d_results);
    hipLaunchKernelGGL(blas_lbvh_batch_permute_kernel, dim3(n_units), dim3(kBlock), 0, st, plan->d_items, L.d_segs, L.d_unit_seg, d_n_tri, vals, w.idx,
                       plan->d_bad, d_results);
    if (plan->n_bound_chunks)
        hipLaunchKernelGGL(blas_lbvh_batch_bounds_kernel, dim3(plan->n_bound_chunks), dim3(kBlock), 0, st, plan->d_items, plan->d_bound_chunks,
                           plan->d_bound_keys, plan->d_bound_done);
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_bvh_build_lbvh_batch(VdCtx* ctx, VdBvhLbvhBatchItem* items, uint32_t n_items, const uint32_t* n_tri, VdBvhLbvhResult* results) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (n_items && (!items || !results)) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh_batch: null items / results");
    if (n_items > VD_BVH_LBVH_BATCH_MAX_ITEMS) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_bvh_build_lbvh_batch: n_items > VD_BVH_LBVH_BATCH_MAX_ITEMS");
    if (n_items == 0u) return VD_OK;
    std::vector<VdBvhLbvhBatchItem> d_items;               // the items as the device sees them: the staged copies
    std::vector<VdBlob> blobs;                             // kItemBlobs per item, then the counts and the results
    std::vector<void*> hosts;                              // where each blob is fetched to; null: it is not
    try {
        d_items.assign(items, items + n_items);
        blobs.reserve(kItemBlobs * (size_t)n_items + 2);
        for (uint32_t m = 0; m < n_items; ++m) {
            items[m].status = VD_OK;
            const VdBvhLbvhBatchItem& it = items[m];
            if (!it.verts_xyz || !it.indices_inout || !it.nodes) return fail_item(ctx, items, m, "null vertices / indices / nodes");
            if (it.tri_cap == 0u || it.tri_cap > VD_BVH_LBVH_MAX_TRIANGLES) return fail_item(ctx, items, m, "tri_cap == 0 or > VD_BVH_LBVH_MAX_TRIANGLES");
            if (it.node_cap < (it.tri_cap < 2u ? 2u : 2u * it.tri_cap)) return fail_item(ctx, items, m, "node_cap < max(2, 2 * tri_cap)");
            blobs.push_back(VdBlob{it.verts_xyz, 12 * (size_t)it.n_vert, 256, nullptr});
            blobs.push_back(VdBlob{it.indices_inout, 12 * (size_t)it.tri_cap, 256, nullptr});
            blobs.push_back(VdBlob{nullptr, sizeof(VdBvhNode) * (size_t)it.node_cap, 256, nullptr});
            blobs.push_back(VdBlob{it.mesh_info, it.mesh_info ? sizeof(VdMeshInfo) : 0, 256, nullptr});
        }
        blobs.push_back(VdBlob{n_tri, 4 * (size_t)n_items, 256, nullptr});
        blobs.push_back(VdBlob{nullptr, sizeof(VdBvhLbvhResult) * (size_t)n_items, 256, nullptr});
        hosts.assign(blobs.size(), nullptr);
    } catch (const std::bad_alloc&) {
        VD_FAIL(ctx, VD_ERR_OOM, "vd_bvh_build_lbvh_batch: host memory");
    }
    int rc = vd_stage_blobs(ctx, blobs.data(), (unsigned)blobs.size());
    if (rc) return rc;
    const VdBlob* counts = &blobs[kItemBlobs * (size_t)n_items];
    for (uint32_t m = 0; m < n_items; ++m) {
        const VdBlob* b = &blobs[kItemBlobs * (size_t)m];
        d_items[m].verts_xyz = static_cast<const float*>(b[kBlobVerts].dev); d_items[m].indices_inout = static_cast<uint32_t*>(b[kBlobIndices].dev);
        d_items[m].nodes = static_cast<VdBvhNode*>(b[kBlobNodes].dev);
        d_items[m].mesh_info = items[m].mesh_info ? static_cast<VdMeshInfo*>(b[kBlobInfo].dev) : nullptr;
    }
    VdBvhLbvhPlan* plan = nullptr;
    rc = vd_bvh_lbvh_plan_dev(ctx, d_items.data(), n_items, &plan);
    for (uint32_t m = 0; m < n_items; ++m) items[m].status = d_items[m].status;
    if (rc) return rc;
    rc = vd_bvh_build_lbvh_planned_dev(ctx, plan, n_tri ? static_cast<const uint32_t*>(counts[0].dev) : nullptr, static_cast<VdBvhLbvhResult*>(counts[1].dev));
    if (rc == VD_OK) rc = vd_fetch_blob(ctx, results, &counts[1]);
    if (rc == VD_OK) rc = batch_fetch(ctx, items, n_items, n_tri, results, blobs.data(), hosts.data());
    (void)vd_bvh_lbvh_plan_release(ctx, plan);
    return rc;
}

}  // extern "C"
