// The host part of vd_bvh_lbvh_plan_dev (voidin_amd/csrc/blas_lbvh_plan.hpp) on hand-made item lists: which items the batched
// LBVH build takes, and the slot space it lays them out in.  Host code only - no HIP, no library.
//
// The expected values are written out by hand from the rule in the header: item m owns n_units = ceil(tri_cap / 256) units of
// 256 slots behind the items before it; one extent chunk per 2048 of tri_cap; one fold chunk per 4096 vertices of an item that
// carries a VdMeshInfo, and one for none at all.
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../voidin_amd/csrc/blas_lbvh_plan.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

// stand for device memory: never dereferenced
alignas(16) static unsigned char g_mem[64];
static const float* g_verts = reinterpret_cast<const float*>(g_mem);
static uint32_t* g_idx = reinterpret_cast<uint32_t*>(g_mem);
static VdBvhNode* g_nodes = reinterpret_cast<VdBvhNode*>(g_mem);
static VdMeshInfo* g_info = reinterpret_cast<VdMeshInfo*>(g_mem + 16);

static VdBvhLbvhBatchItem item(uint32_t tri_cap, uint32_t n_vert = 100u, bool info = false) {
    VdBvhLbvhBatchItem it;
    memset(&it, 0, sizeof(it));
    it.verts_xyz = g_verts; it.indices_inout = g_idx; it.nodes = g_nodes; it.mesh_info = info ? g_info : nullptr;
    it.n_vert = n_vert; it.tri_cap = tri_cap; it.node_cap = tri_cap < 2u ? 2u : 2u * tri_cap;
    it.status = 0x5a5a;
    return it;
}

struct Planned {
    LbvhPlanTables t;
    std::string what;      // empty: every item was taken
    uint32_t failed = 77u;
};
static Planned plan(std::vector<VdBvhLbvhBatchItem>& items, unsigned D = 0u) {
    Planned p;
    char buf[kLbvhWhatLen] = "";
    const char* what = lbvh_plan_tables(items.data(), (uint32_t)items.size(), D, p.t, &p.failed, buf);
    if (what) p.what = what;
    return p;
}
static bool is(const VdLbvhSeg& s, unsigned slot0, unsigned cap, unsigned n_units) { return s.slot0 == slot0 && s.cap == cap && s.n_units == n_units && s._pad == 0u; }
static bool is(const VdPair& c, unsigned x, unsigned y) { return c.x == x && c.y == y; }

static void layouts() {
    {   // three items: 2, 1 and 3 units
        std::vector<VdBvhLbvhBatchItem> items = {item(300), item(5), item(700)};
        Planned p = plan(items);
        CHECK(p.what.empty() && p.failed == 77u);
        CHECK(items[0].status == VD_OK && items[1].status == VD_OK && items[2].status == VD_OK);
        CHECK(p.t.segs.size() == 3u && is(p.t.segs[0], 0, 300, 2) && is(p.t.segs[1], 512, 5, 1) && is(p.t.segs[2], 768, 700, 3));
        CHECK(p.t.unit_seg == std::vector<unsigned>({0, 0, 1, 2, 2, 2}));
        CHECK(p.t.n_slots == 1536u);
        CHECK(p.t.ext_chunks.size() == 3u && is(p.t.ext_chunks[0], 0, 0) && is(p.t.ext_chunks[1], 1, 0) && is(p.t.ext_chunks[2], 2, 0));
        CHECK(p.t.bound_chunks.empty());
        CHECK(p.t.items.size() == 3u);
        const BatchItemDev& d = p.t.items[2];
        CHECK(d.verts == g_verts && d.indices == g_idx && d.nodes == g_nodes && d.info == nullptr);
        CHECK(d.n_vert == 100u && d.node_cap == 1400u && d.n_chunks == 0u);
        for (unsigned q = 0; q < 5; ++q) CHECK(d._pad[q] == 0u);
    }
    {   // 5000 triangles: 20 units, three extent chunks
        std::vector<VdBvhLbvhBatchItem> items = {item(5000)};
        Planned p = plan(items);
        CHECK(p.what.empty() && is(p.t.segs[0], 0, 5000, 20) && p.t.unit_seg == std::vector<unsigned>(20, 0u) && p.t.n_slots == 5120u);
        CHECK(p.t.ext_chunks.size() == 3u && is(p.t.ext_chunks[0], 0, 0) && is(p.t.ext_chunks[1], 0, 2048) && is(p.t.ext_chunks[2], 0, 4096));
    }
    {   // the unit's edge
        std::vector<VdBvhLbvhBatchItem> items = {item(256), item(257)};
        Planned p = plan(items);
        CHECK(p.what.empty() && is(p.t.segs[0], 0, 256, 1) && is(p.t.segs[1], 256, 257, 2) && p.t.n_slots == 768u);
        CHECK(p.t.unit_seg == std::vector<unsigned>({0, 1, 1}));
    }
}

static void fold_chunks() {
    std::vector<VdBvhLbvhBatchItem> items = {item(4, 0, true), item(4, 4096, true), item(4, 4097, false), item(4, 4097, true)};
    Planned p = plan(items);
    CHECK(p.what.empty());
    CHECK(p.t.items[0].n_chunks == 1u && p.t.items[1].n_chunks == 1u && p.t.items[2].n_chunks == 0u && p.t.items[3].n_chunks == 2u);
    CHECK(p.t.items[0].info == g_info && p.t.items[2].info == nullptr);
    CHECK(p.t.bound_chunks.size() == 4u);
    CHECK(is(p.t.bound_chunks[0], 0, 0) && is(p.t.bound_chunks[1], 1, 0) && is(p.t.bound_chunks[2], 3, 0) && is(p.t.bound_chunks[3], 3, 4096));
    const std::vector<int> keys = vd_fold_neutral_keys(2);
    CHECK(keys == std::vector<int>({0x7f800000, 0x7f800000, 0x7f800000, (int)0x807fffff, (int)0x807fffff, (int)0x807fffff,
                                    0x7f800000, 0x7f800000, 0x7f800000, (int)0x807fffff, (int)0x807fffff, (int)0x807fffff}));
}

// the bad item in the middle of three: refused by index and text, the item before it keeps status 0
static void refused(VdBvhLbvhBatchItem bad, const char* text, unsigned D = 0u) {
    std::vector<VdBvhLbvhBatchItem> items = {item(D ? 16 : 300), bad, item(5)};      // (16: what the bounds used here can hold)
    Planned p = plan(items, D);
    CHECK(p.failed == 1u);
    CHECK(p.what == text);
    if (p.what != text) printf("  got \"%s\"\n  for \"%s\"\n", p.what.c_str(), text);
    CHECK(items[0].status == VD_OK && items[1].status == VD_ERR_INVALID_ARG);
}

static void refusals() {
    VdBvhLbvhBatchItem it = item(700);
    it.verts_xyz = nullptr; refused(it, "null vertices / indices / nodes");
    it = item(700); it.indices_inout = nullptr; refused(it, "null vertices / indices / nodes");
    it = item(700); it.nodes = nullptr; refused(it, "null vertices / indices / nodes");
    it = item(700); it.tri_cap = 0u; refused(it, "tri_cap == 0");
    it = item(700); it.tri_cap = (1u << 24) + 1u; it.node_cap = 0xffffffffu; refused(it, "tri_cap > VD_BVH_LBVH_MAX_TRIANGLES");
    it = item(700); it.node_cap = 2u * 700u - 1u; refused(it, "node_cap < max(2, 2 * tri_cap)");
    it = item(1); it.node_cap = 1u; refused(it, "node_cap < max(2, 2 * tri_cap)");
    it = item(700); it.nodes = reinterpret_cast<VdBvhNode*>(g_mem + 8); refused(it, "nodes is not 16-byte aligned");
    {   // the order of the texts: a null pointer is named before a bad capacity, a bad capacity before the alignment
        it = item(700); it.nodes = nullptr; it.tri_cap = 0u; refused(it, "null vertices / indices / nodes");
        it = item(700); it.nodes = reinterpret_cast<VdBvhNode*>(g_mem + 8); it.node_cap = 3u; refused(it, "node_cap < max(2, 2 * tri_cap)");
    }
    {   // capacities that add up to one unit more than 2^24 slots: refused at the item that crosses the limit
        std::vector<VdBvhLbvhBatchItem> items = {item(1u << 23), item(1u << 23), item(1)};
        Planned p = plan(items);
        CHECK(p.failed == 2u && p.what == "the capacities, each rounded up to 256, add up to more than VD_BVH_LBVH_MAX_TRIANGLES");
        CHECK(items[0].status == VD_OK && items[1].status == VD_OK && items[2].status == VD_ERR_INVALID_ARG);
        std::vector<VdBvhLbvhBatchItem> fits = {item(1u << 23), item(1u << 23)};
        Planned q = plan(fits);
        CHECK(q.what.empty() && q.t.n_slots == (1u << 24));
    }
    {   // the depth bound: 16 triangles need 3 levels under their leaves of <= 3, 17 need 4
        refused(item(17), "VD_OPT_BLAS_LBVH_MAX_DEPTH = 3 cannot hold tri_cap = 17: the smallest bound that can is 4", 3u);
        std::vector<VdBvhLbvhBatchItem> items = {item(16), item(3), item(1)};
        CHECK(plan(items, 3u).what.empty());
        std::vector<VdBvhLbvhBatchItem> free_of_it = {item(17)};
        CHECK(plan(free_of_it, 0u).what.empty() && plan(free_of_it, 4u).what.empty());
        CHECK(needr(1) == 0u && needr(3) == 0u && needr(4) == 1u && needr(5) == 2u && needr(16) == 3u && needr(17) == 4u && needr(1u << 24) == 23u);
    }
}

int main() {
    layouts();
    fold_chunks();
    refusals();
    if (g_fail) { printf("blas_lbvh_plan_test: %d checks failed\n", g_fail); return 1; }
    printf("blas_lbvh_plan_test OK\n");
    return 0;
}
