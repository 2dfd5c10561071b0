// blas_refit_plan.hpp — the pure host part of vd_bvh_refit_plan_dev (blas_refit.hip): what the refit kernel will walk, validated
// and derived one item at a time from the item's nodes and indices as host arrays.  No HIP and no VdCtx, so a host compiler
// builds it alone (tests/cpp/blas_refit_plan_test.cpp).  Everything is in the unnamed namespace of the one file that includes
// it.  The kernel trusts these tables: a parent id below every child's is what ends its climb.
#pragma once

#include <stdint.h>

#include <vector>

#include "vd_plan.hpp"

namespace {

constexpr unsigned kNoParent = 0xffffffffu;

struct RefitItemDev {
    const float* verts; const unsigned* indices; VdBvhNode* nodes; VdMeshInfo* info;
    unsigned n_vert, n_tri, n_nodes, node_base;        // node_base: where the item's links / counters start in the plan's arrays
    unsigned n_chunks, _pad[3];
};
static_assert(sizeof(RefitItemDev) == 64, "one item record per cache-line half");

struct RefitPlanTables {
    std::vector<RefitItemDev> items;                   // per item
    std::vector<VdQuad> leaves;                        // {item, node, first triangle, triangle count}, ascending node id within an item
    std::vector<unsigned> up;                          // per node: parent << 1 | (node is the right child), kNoParent for node 0 / the reserved slot
    std::vector<VdPair> chunks;                        // per block of the MeshInfo fold: {item, first vertex}
};

// What is known of an item before its nodes and indices are read: null, or why the plan refuses it.
inline const char* refit_judge_item(const RefitPlanTables& t, const VdBvhRefitItem& it) {
    if (!it.verts_xyz || !it.indices || !it.nodes) return "null vertices / indices / nodes";
    if (it.n_nodes < 1u) return "n_nodes < 1";
    if (it.n_nodes > 0x7fffffffu || (size_t)t.up.size() + it.n_nodes > 0xfffffff0u) return "too many nodes for one plan";
    return nullptr;
}

// Item m (judged), its n_nodes nodes and 3 * n_tri indices on the host: the indices against n_vert, the parent links and the
// leaves in one ascending sweep, the device record, the fold chunks.  null, or why the plan refuses it (the tables are of no
// use then).
inline const char* refit_plan_item(RefitPlanTables& t, uint32_t m, const VdBvhRefitItem& it, const VdBvhNode* nodes, const unsigned* idx) {
    for (size_t k = 0; k < 3 * (size_t)it.n_tri; ++k)
        if (idx[k] >= it.n_vert) return "an index >= n_vert";
    const size_t base = t.up.size();
    t.up.resize(base + it.n_nodes, kNoParent);
    unsigned* up = t.up.data() + base;
    // children follow their parent (pre-order), so one ascending sweep knows every node's parent before it gets there
    for (unsigned k = 0; k < it.n_nodes; ++k) {
        if (k != 0u && up[k] == kNoParent) {
            if (k == 1u) continue;                     // the reserved slot: whatever it holds, nobody reads or writes it
            return "a node other than 0 and the reserved slot 1 has no parent";
        }
        const VdBvhNode& nd = nodes[k];
        if (nd.count == 0u) {
            const uint64_t l = nd.left_first;
            if (l <= k || l + 1u >= it.n_nodes) return "an interior node's children are not both in (own id, n_nodes)";
            if (up[l] != kNoParent || up[l + 1u] != kNoParent) return "a node has two parents";
            up[l] = k << 1; up[l + 1u] = (k << 1) | 1u;
        } else {
            if ((uint64_t)nd.left_first + nd.count > it.n_tri) return "a leaf's triangle range leaves [0, n_tri)";
            if (t.leaves.size() >= 0xfffffff0u) return "too many leaves for one plan";
            t.leaves.push_back(VdQuad{m, k, nd.left_first, nd.count});
        }
    }
    RefitItemDev d = RefitItemDev{};
    d.verts = it.verts_xyz; d.indices = it.indices; d.nodes = it.nodes; d.info = it.mesh_info;
    d.n_vert = it.n_vert; d.n_tri = it.n_tri; d.n_nodes = it.n_nodes; d.node_base = (unsigned)base;
    if (it.mesh_info) d.n_chunks = vd_fold_chunks(t.chunks, m, it.n_vert);
    t.items.push_back(d);
    return nullptr;
}

}  // namespace
