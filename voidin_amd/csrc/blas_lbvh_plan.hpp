// blas_lbvh_plan.hpp — the pure host part of vd_bvh_lbvh_plan_dev (blas_lbvh.hip): which items a batched LBVH build takes, and the
// slot space it lays them out in.  No HIP and no VdCtx, so a host compiler builds it alone (tests/cpp/blas_lbvh_plan_test.cpp).
// Everything is in the unnamed namespace of the one file that includes it.  The kernels trust these tables without a bounds check.
//
// The slot space: item m owns the slots [slot0, slot0 + n_units * 256), n_units = ceil(tri_cap / 256), one item after the other, so
// that a 256-thread block (and a unit of the segmented sort, tlas.hip) never spans two meshes.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "vd_plan.hpp"

namespace {

// depth of the radix tree over the integers 0 .. k - 1 cut off at nodes of <= 3 positions
VD_HOST_DEVICE unsigned needr(unsigned k) { return k <= 3u ? 0u : 31u - (unsigned)__builtin_clz(k - 1u); }

struct BatchItemDev {
    const float* verts; unsigned* indices; VdBvhNode* nodes; VdMeshInfo* info;
    unsigned n_vert, node_cap, n_chunks /* of the MeshInfo fold */, _pad[5];
};
static_assert(sizeof(BatchItemDev) == 64, "one item record per cache-line half");

struct LbvhPlanTables {
    std::vector<BatchItemDev> items;                  // per item
    std::vector<VdLbvhSeg> segs;                      // per item: its run of slots
    std::vector<unsigned> unit_seg;                   // per 256-slot unit: its item
    std::vector<VdPair> ext_chunks;                   // {item, first position}: one per kVdLbvhExtentChunk of tri_cap
    std::vector<VdPair> bound_chunks;                 // {item, first vertex}: the blocks of the MeshInfo fold
    uint64_t n_slots = 0;
};

constexpr size_t kLbvhWhatLen = 160;

// Is this item one the build can take under the depth bound D (0: unbounded)?  null, or why not (`buf`: kLbvhWhatLen chars).
inline const char* lbvh_judge_item(const VdBvhLbvhBatchItem& it, unsigned D, char* buf) {
    if (!it.verts_xyz || !it.indices_inout || !it.nodes) return "null vertices / indices / nodes";
    if (it.tri_cap == 0u) return "tri_cap == 0";
    if (it.tri_cap > VD_BVH_LBVH_MAX_TRIANGLES) return "tri_cap > VD_BVH_LBVH_MAX_TRIANGLES";
    if (it.node_cap < (it.tri_cap < 2u ? 2u : 2u * it.tri_cap)) return "node_cap < max(2, 2 * tri_cap)";
    if ((reinterpret_cast<uintptr_t>(it.nodes) & 15u) != 0u) return "nodes is not 16-byte aligned";
    if (D && needr(it.tri_cap) > D) {                  // T_m <= tri_cap: every count the device can hold then fits the bound
        snprintf(buf, kLbvhWhatLen, "VD_OPT_BLAS_LBVH_MAX_DEPTH = %u cannot hold tri_cap = %u: the smallest bound that can is %u", D, it.tri_cap,
                 needr(it.tri_cap));
        return buf;
    }
    return nullptr;
}

// Item m (judged) takes the next slots: its segment, units, extent chunks, device record and fold chunks.  null, or why not.
inline const char* lbvh_place_item(LbvhPlanTables& t, uint32_t m, const VdBvhLbvhBatchItem& it) {
    const unsigned n_units = (it.tri_cap + kVdLbvhBatchUnit - 1u) / kVdLbvhBatchUnit;
    if (t.n_slots + (uint64_t)n_units * kVdLbvhBatchUnit > VD_BVH_LBVH_MAX_TRIANGLES)
        return "the capacities, each rounded up to 256, add up to more than VD_BVH_LBVH_MAX_TRIANGLES";
    t.segs.push_back(VdLbvhSeg{(unsigned)t.n_slots, it.tri_cap, n_units, 0u});
    t.unit_seg.insert(t.unit_seg.end(), n_units, m);
    for (unsigned c = 0; c < it.tri_cap; c += kVdLbvhExtentChunk) t.ext_chunks.push_back(VdPair{m, c});
    BatchItemDev d = BatchItemDev{};
    d.verts = it.verts_xyz; d.indices = it.indices_inout; d.nodes = it.nodes; d.info = it.mesh_info;
    d.n_vert = it.n_vert; d.node_cap = it.node_cap;
    if (it.mesh_info) d.n_chunks = vd_fold_chunks(t.bound_chunks, m, it.n_vert);
    t.items.push_back(d);
    t.n_slots += (uint64_t)n_units * kVdLbvhBatchUnit;
    return nullptr;
}

// All items in order, each judged and then placed: every status VD_OK, or the first refused item's VD_ERR_INVALID_ARG with
// *failed = its index and the text to report (null: none was refused).  The tables are of use only then.
inline const char* lbvh_plan_tables(VdBvhLbvhBatchItem* items, uint32_t n_items, unsigned D, LbvhPlanTables& t, uint32_t* failed, char* buf) {
    for (uint32_t m = 0; m < n_items; ++m) items[m].status = VD_OK;
    t.items.reserve(n_items); t.segs.reserve(n_items);
    for (uint32_t m = 0; m < n_items; ++m) {
        const char* what = lbvh_judge_item(items[m], D, buf);
        if (!what) what = lbvh_place_item(t, m, items[m]);
        if (what) { items[m].status = VD_ERR_INVALID_ARG; *failed = m; return what; }
    }
    return nullptr;
}

}  // namespace
