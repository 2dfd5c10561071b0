// The host part of vd_bvh_refit_plan_dev (voidin_amd/csrc/blas_refit_plan.hpp) on hand-made node arrays: the parent links of
// the ascending sweep, the leaf records, the fold chunks and every refusal.  Host code only - no HIP, no library.
//
// The expected values are written out by hand: up[k] = parent << 1 | (k is the right child), kNoParent for node 0 and for the
// reserved slot 1; a leaf record is {item, node, first triangle, triangle count}, in ascending node order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../voidin_amd/csrc/blas_refit_plan.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

// stand for device memory: never dereferenced
alignas(16) static unsigned char g_mem[64];
static const unsigned kNo = 0xffffffffu;

static VdBvhNode leaf(unsigned first, unsigned count) { VdBvhNode n; memset(&n, 0, sizeof(n)); n.left_first = first; n.count = count; return n; }
static VdBvhNode inner(unsigned left) { VdBvhNode n; memset(&n, 0, sizeof(n)); n.left_first = left; n.count = 0u; return n; }
static VdBvhNode junk() { VdBvhNode n; memset(&n, 0xc3, sizeof(n)); return n; }      // the reserved slot: whatever it holds

struct Mesh {
    std::vector<VdBvhNode> nodes;
    uint32_t n_tri, n_vert;
    std::vector<unsigned> idx;       // empty: 0, 1, 2, 0, 1, 2, ...
    bool info;
};
static VdBvhRefitItem item_of(const Mesh& ms) {
    VdBvhRefitItem it;
    memset(&it, 0, sizeof(it));
    it.verts_xyz = reinterpret_cast<const float*>(g_mem); it.indices = reinterpret_cast<const uint32_t*>(g_mem);
    it.nodes = reinterpret_cast<VdBvhNode*>(g_mem); it.mesh_info = ms.info ? reinterpret_cast<VdMeshInfo*>(g_mem + 16) : nullptr;
    it.n_vert = ms.n_vert; it.n_tri = ms.n_tri; it.n_nodes = (uint32_t)ms.nodes.size();
    return it;
}
// the item through both steps; "" when the plan takes it
static std::string add(RefitPlanTables& t, uint32_t m, const Mesh& ms) {
    const VdBvhRefitItem it = item_of(ms);
    if (const char* what = refit_judge_item(t, it)) return what;
    std::vector<unsigned> idx = ms.idx;
    if (idx.empty()) for (size_t k = 0; k < 3 * (size_t)ms.n_tri; ++k) idx.push_back((unsigned)(k % 3));
    // exactly n_nodes nodes and 3 * n_tri indices, in heap blocks of their own: a read past either is the sanitizer's
    std::vector<VdBvhNode> nodes(ms.nodes);
    nodes.shrink_to_fit(); idx.shrink_to_fit();
    const char* what = refit_plan_item(t, m, it, nodes.data(), idx.data());
    return what ? what : "";
}
static bool is(const VdQuad& l, unsigned item, unsigned node, unsigned first, unsigned count) { return l.x == item && l.y == node && l.z == first && l.w == count; }

static void trees() {
    {   // a single leaf, nothing behind it
        RefitPlanTables t;
        CHECK(add(t, 0, Mesh{{leaf(0, 2)}, 2, 3, {}, false}) == "");
        CHECK(t.up == std::vector<unsigned>({kNo}));
        CHECK(t.leaves.size() == 1u && is(t.leaves[0], 0, 0, 0, 2));
        CHECK(t.items.size() == 1u && t.items[0].n_nodes == 1u && t.items[0].n_tri == 2u && t.items[0].n_vert == 3u && t.items[0].node_base == 0u);
        CHECK(t.items[0].n_chunks == 0u && t.items[0].info == nullptr && t.chunks.empty());
    }
    {   // a leaf and the reserved slot
        RefitPlanTables t;
        CHECK(add(t, 0, Mesh{{leaf(0, 3), junk()}, 3, 3, {}, false}) == "");
        CHECK(t.up == std::vector<unsigned>({kNo, kNo}));
        CHECK(t.leaves.size() == 1u && is(t.leaves[0], 0, 0, 0, 3));
    }
    {   // the root over two leaves at 2 and 3
        RefitPlanTables t;
        CHECK(add(t, 0, Mesh{{inner(2), junk(), leaf(0, 1), leaf(1, 3)}, 4, 3, {}, false}) == "");
        CHECK(t.up == std::vector<unsigned>({kNo, kNo, 0u << 1, 0u << 1 | 1u}));
        CHECK(t.leaves.size() == 2u && is(t.leaves[0], 0, 2, 0, 1) && is(t.leaves[1], 0, 3, 1, 3));
    }
    {   // three interior nodes, pre-order: the right subtree (3 -> 6, 7) follows the whole left one (2 -> 4, 5)
        RefitPlanTables t;
        CHECK(add(t, 0, Mesh{{inner(2), junk(), inner(4), inner(6), leaf(0, 1), leaf(1, 1), leaf(2, 2), leaf(4, 1)}, 5, 3, {}, false}) == "");
        CHECK(t.up == std::vector<unsigned>({kNo, kNo, 0, 1, 2u << 1, 2u << 1 | 1u, 3u << 1, 3u << 1 | 1u}));
        CHECK(t.leaves.size() == 4u && is(t.leaves[0], 0, 4, 0, 1) && is(t.leaves[1], 0, 5, 1, 1) && is(t.leaves[2], 0, 6, 2, 2) && is(t.leaves[3], 0, 7, 4, 1));
    }
    {   // two items: the second one's links start behind the first one's, its ids are its own
        RefitPlanTables t;
        CHECK(add(t, 0, Mesh{{inner(2), junk(), leaf(0, 1), leaf(1, 3)}, 4, 3, {}, true}) == "");
        CHECK(add(t, 1, Mesh{{leaf(0, 1), junk()}, 1, 4097, {}, true}) == "");
        CHECK(t.items.size() == 2u && t.items[0].node_base == 0u && t.items[1].node_base == 4u);
        CHECK(t.up == std::vector<unsigned>({kNo, kNo, 0, 1, kNo, kNo}));
        CHECK(t.leaves.size() == 3u && is(t.leaves[0], 0, 2, 0, 1) && is(t.leaves[1], 0, 3, 1, 3) && is(t.leaves[2], 1, 0, 0, 1));
        CHECK(t.items[0].n_chunks == 1u && t.items[1].n_chunks == 2u && t.items[1].info != nullptr);
        CHECK(t.chunks.size() == 3u && t.chunks[0].x == 0u && t.chunks[0].y == 0u && t.chunks[1].x == 1u && t.chunks[1].y == 0u &&
              t.chunks[2].x == 1u && t.chunks[2].y == 4096u);
    }
}

static void refused(const Mesh& ms, const char* text) {
    RefitPlanTables t;
    const std::string what = add(t, 0, ms);
    CHECK(what == text);
    if (what != text) printf("  got \"%s\"\n  for \"%s\"\n", what.c_str(), text);
}

static void refusals() {
    refused(Mesh{{}, 1, 3, {}, false}, "n_nodes < 1");
    {   // null pointers, and the limit of one plan's link array
        RefitPlanTables t;
        VdBvhRefitItem it = item_of(Mesh{{leaf(0, 1)}, 1, 3, {}, false});
        it.indices = nullptr;
        CHECK(std::string(refit_judge_item(t, it)) == "null vertices / indices / nodes");
        it = item_of(Mesh{{leaf(0, 1)}, 1, 3, {}, false});
        it.n_nodes = 0x80000000u;
        CHECK(std::string(refit_judge_item(t, it)) == "too many nodes for one plan");
        it.n_nodes = 0x7fffffffu;
        CHECK(refit_judge_item(t, it) == nullptr);
    }
    refused(Mesh{{inner(0), junk(), leaf(0, 1), leaf(1, 1)}, 2, 3, {}, false}, "an interior node's children are not both in (own id, n_nodes)");
    refused(Mesh{{inner(2), junk(), inner(2), leaf(1, 1)}, 2, 3, {}, false}, "an interior node's children are not both in (own id, n_nodes)");      // its own id
    refused(Mesh{{inner(3), junk(), leaf(0, 1), leaf(1, 1)}, 2, 3, {}, false}, "an interior node's children are not both in (own id, n_nodes)");     // the pair ends at n_nodes
    refused(Mesh{{inner(2), junk(), inner(3), leaf(0, 1), leaf(1, 1)}, 2, 3, {}, false}, "a node has two parents");                                     // 3: of 0 and of 2
    refused(Mesh{{inner(3), junk(), leaf(0, 1), leaf(0, 1), leaf(1, 1)}, 2, 3, {}, false}, "a node other than 0 and the reserved slot 1 has no parent");
    refused(Mesh{{inner(2), junk(), leaf(0, 1), leaf(1, 2)}, 2, 3, {}, false}, "a leaf's triangle range leaves [0, n_tri)");                           // one past n_tri
    refused(Mesh{{leaf(0xffffffffu, 2)}, 2, 3, {}, false}, "a leaf's triangle range leaves [0, n_tri)");                                                // no 32-bit wrap
    refused(Mesh{{leaf(0, 2)}, 2, 3, {0, 1, 2, 2, 3, 0}, false}, "an index >= n_vert");
    {   // ... the largest index that is one passes
        RefitPlanTables t;
        CHECK(add(t, 0, Mesh{{leaf(0, 2)}, 2, 3, {0, 1, 2, 2, 2, 0}, false}) == "");
    }
}

int main() {
    trees();
    refusals();
    if (g_fail) { printf("blas_refit_plan_test: %d checks failed\n", g_fail); return 1; }
    printf("blas_refit_plan_test OK\n");
    return 0;
}
