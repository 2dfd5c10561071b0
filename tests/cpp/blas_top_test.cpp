// The host part of the SAH builder's copy-out (voidin_amd/csrc/blas_top.hpp) on hand-made top trees: top_preorder +
// number_top give every node its final index, place_nodes every mesh its room.  Host code only - no HIP, no library.
//
// The expected values are written out by hand from the rule in include/voidin_abi.h ("vd_bvh_build") and blas.rs:105-128:
// node 0 is the root, node 1 the pad; a pair is taken when an interior is visited in pre-order (left before right); a
// small root takes 2 * sub_interior nodes in one piece when visited.
//
// A top tree here: mesh m's root is tmp node 2m, 2m + 1 its pad slot (kind 3), child pairs follow from 2K on.
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../voidin_amd/csrc/blas_top.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static TopNode leaf() { TopNode t; memset(&t, 0, sizeof(t)); t.kind = 0u; t.count = 3u; return t; }
static TopNode inner(unsigned left) { TopNode t; memset(&t, 0, sizeof(t)); t.kind = 1u; t.left = left; return t; }
static TopNode small_root(unsigned r) { TopNode t; memset(&t, 0, sizeof(t)); t.kind = 2u; t.small = r; return t; }
static TopNode pad() { TopNode t; memset(&t, 0, sizeof(t)); t.kind = 3u; return t; }

static VdBvhNode g_own[4];        // stands for "this mesh has a node array of its own": never dereferenced

struct Numbered {
    std::vector<TopOut> out;
    std::vector<unsigned> root_pair;
    std::vector<BuildMesh> hm;
};

// own[m]: node_cap of mesh m's own array, 0 = packed
static Numbered number(const std::vector<TopNode>& top, const std::vector<unsigned>& sub, const std::vector<uint32_t>& own) {
    const uint32_t K = (uint32_t)own.size();
    Numbered r;
    r.out.assign(top.size(), TopOut{0xdeadu, 0xdeadu, 0xdeadu});
    r.root_pair.assign(sub.size(), 0xdeadu);
    r.hm.resize(K);
    for (uint32_t m = 0; m < K; ++m) r.hm[m] = BuildMesh{nullptr, 3u, nullptr, 1u, own[m] ? g_own : nullptr, own[m], 0xdeadu, 0xdeadu};
    std::vector<unsigned> ord(top.size()), ord_end(K);
    top_preorder(top.data(), K, r.out.data(), ord.data(), ord_end.data());
    number_top(top.data(), sub.data(), K, ord.data(), ord_end.data(), r.out.data(), r.root_pair.data(), r.hm.data());
    // every mesh's final indices are exactly 0 .. pool - 1: the top nodes' own places and the small roots' ranges
    for (uint32_t m = 0; m < K; ++m) {
        std::vector<int> seen(r.hm[m].out_n_nodes, 0);
        bool in_range = true;
        for (size_t v = 0; v < top.size(); ++v) {
            if (r.out[v].mesh != m) continue;
            if (r.out[v].final_index < seen.size()) ++seen[r.out[v].final_index]; else in_range = false;
            if (top[v].kind != 2u) continue;
            for (unsigned j = 0; j < 2u * sub[top[v].small]; ++j)
                if (r.root_pair[top[v].small] + j < seen.size()) ++seen[r.root_pair[top[v].small] + j]; else in_range = false;
        }
        CHECK(in_range);
        for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1);
    }
    return r;
}

static bool is(const TopOut& o, unsigned final_index, unsigned pair, unsigned mesh) { return o.final_index == final_index && o.pair == pair && o.mesh == mesh; }
// a leaf takes no pair: its TopOut::pair is never written and never read
static bool is_leaf(const TopOut& o, unsigned final_index, unsigned mesh) { return o.final_index == final_index && o.mesh == mesh; }

static void single_meshes() {
    {   // one mesh that is a single leaf
        Numbered r = number({leaf(), pad()}, {}, {2});
        CHECK(r.hm[0].out_n_nodes == 2u);
        CHECK(is_leaf(r.out[0], 0, 0) && is(r.out[1], 1, 0, 0));
    }
    {   // one mesh that is one small root of three interiors
        Numbered r = number({small_root(0), pad()}, {3}, {8});
        CHECK(r.hm[0].out_n_nodes == 8u);
        CHECK(is(r.out[0], 0, 2, 0) && is(r.out[1], 1, 0, 0) && r.root_pair[0] == 2u);
    }
    {   // an interior node over a small root (two interiors) and a big leaf
        Numbered r = number({inner(2), pad(), small_root(0), leaf()}, {2}, {8});
        CHECK(r.hm[0].out_n_nodes == 8u);
        CHECK(is(r.out[0], 0, 2, 0) && is(r.out[1], 1, 0, 0) && is(r.out[2], 2, 4, 0) && is_leaf(r.out[3], 3, 0));
        CHECK(r.root_pair[0] == 4u);
    }
    {   // a left-deep chain of four interiors
        Numbered r = number({inner(2), pad(), inner(4), leaf(), inner(6), leaf(), inner(8), leaf(), leaf(), leaf()}, {}, {10});
        CHECK(r.hm[0].out_n_nodes == 10u);
        CHECK(is(r.out[0], 0, 2, 0) && is(r.out[2], 2, 4, 0) && is(r.out[4], 4, 6, 0) && is(r.out[6], 6, 8, 0));
        CHECK(is_leaf(r.out[3], 3, 0) && is_leaf(r.out[5], 5, 0) && is_leaf(r.out[7], 7, 0) && is_leaf(r.out[8], 8, 0) && is_leaf(r.out[9], 9, 0));
    }
    {   // pre-order, not level order: the right child's pair comes after the whole left subtree
        Numbered r = number({inner(2), pad(), inner(4), inner(6), inner(8), leaf(), leaf(), leaf(), small_root(0), leaf()}, {2}, {14});
        CHECK(r.hm[0].out_n_nodes == 14u);
        CHECK(is(r.out[0], 0, 2, 0) && is(r.out[2], 2, 4, 0) && is(r.out[4], 4, 6, 0));
        CHECK(is(r.out[8], 6, 8, 0) && r.root_pair[0] == 8u && is_leaf(r.out[9], 7, 0));       // the small root: nodes 8 .. 11
        CHECK(is(r.out[3], 3, 12, 0) && is_leaf(r.out[5], 5, 0) && is_leaf(r.out[6], 12, 0) && is_leaf(r.out[7], 13, 0));
    }
}

// mesh 0: a small root of one interior (4 nodes); mesh 1: an interior over a small root of two and a leaf (8 nodes);
// mesh 2: a single leaf (2 nodes)
static std::vector<TopNode> two_trees() { return {small_root(0), pad(), inner(4), pad(), small_root(1), leaf()}; }
static std::vector<TopNode> three_trees() { return {small_root(0), pad(), inner(6), pad(), leaf(), pad(), small_root(1), leaf()}; }

static void several_meshes() {
    uint32_t failed = 77u;
    char msg[512] = "untouched";
    {   // two meshes, own arrays: every mesh is numbered from 0
        Numbered r = number(two_trees(), {1, 2}, {4, 8});
        CHECK(r.hm[0].out_n_nodes == 4u && r.hm[1].out_n_nodes == 8u);
        CHECK(is(r.out[0], 0, 2, 0) && is(r.out[1], 1, 0, 0) && r.root_pair[0] == 2u);
        CHECK(is(r.out[2], 0, 2, 1) && is(r.out[3], 1, 0, 1) && is(r.out[4], 2, 4, 1) && is_leaf(r.out[5], 3, 1) && r.root_pair[1] == 4u);
        CHECK(place_nodes(r.hm.data(), 2, 0, 0, &failed, msg, sizeof(msg)));
        CHECK(r.hm[0].out_first == 0u && r.hm[1].out_first == 0u && failed == 77u && !strcmp(msg, "untouched"));
    }
    {   // two meshes, packed from node 11 on, into a buffer that is exactly large enough
        Numbered r = number(two_trees(), {1, 2}, {0, 0});
        CHECK(place_nodes(r.hm.data(), 2, 23, 11, &failed, msg, sizeof(msg)));
        CHECK(r.hm[0].out_first == 11u && r.hm[1].out_first == 15u && failed == 77u);
        CHECK(is(r.out[2], 0, 2, 1) && r.root_pair[1] == 4u);           // packed or not: the numbers inside a mesh are the same
    }
    {   // three meshes, own arrays
        Numbered r = number(three_trees(), {1, 2}, {4, 8, 2});
        CHECK(r.hm[0].out_n_nodes == 4u && r.hm[1].out_n_nodes == 8u && r.hm[2].out_n_nodes == 2u);
        CHECK(is(r.out[2], 0, 2, 1) && is(r.out[6], 2, 4, 1) && is_leaf(r.out[7], 3, 1) && r.root_pair[1] == 4u);
        CHECK(is_leaf(r.out[4], 0, 2) && is(r.out[5], 1, 0, 2));
        CHECK(place_nodes(r.hm.data(), 3, 0, 0, &failed, msg, sizeof(msg)));
        CHECK(r.hm[0].out_first == 0u && r.hm[1].out_first == 0u && r.hm[2].out_first == 0u);
    }
    {   // three meshes, packed from 11 on; and the middle one with its own array: it takes no packed room
        Numbered r = number(three_trees(), {1, 2}, {0, 0, 0});
        CHECK(place_nodes(r.hm.data(), 3, 25, 11, &failed, msg, sizeof(msg)));
        CHECK(r.hm[0].out_first == 11u && r.hm[1].out_first == 15u && r.hm[2].out_first == 23u);
        Numbered q = number(three_trees(), {1, 2}, {0, 8, 0});
        CHECK(place_nodes(q.hm.data(), 3, 17, 11, &failed, msg, sizeof(msg)));
        CHECK(q.hm[0].out_first == 11u && q.hm[1].out_first == 0u && q.hm[2].out_first == 15u && failed == 77u && !strcmp(msg, "untouched"));
    }
}

static void refusals() {
    {   // node_cap one pair short
        uint32_t failed = 77u;
        char msg[512] = "";
        Numbered r = number({inner(2), pad(), small_root(0), leaf()}, {2}, {6});
        CHECK(!place_nodes(r.hm.data(), 1, 0, 0, &failed, msg, sizeof(msg)));
        CHECK(failed == 0u && std::string(msg) == "vd_bvh_build: node_cap too small (mesh 0 of the build needs 8 nodes)");
        Numbered q = number(three_trees(), {1, 2}, {4, 6, 2});
        CHECK(!place_nodes(q.hm.data(), 3, 0, 0, &failed, msg, sizeof(msg)));
        CHECK(failed == 1u && std::string(msg) == "vd_bvh_build: node_cap too small (mesh 1 of the build needs 8 nodes)");
    }
    {   // a packed buffer that is full at the second mesh: one node short of 11 + 4 + 8
        uint32_t failed = 77u;
        char msg[512] = "";
        Numbered r = number(three_trees(), {1, 2}, {0, 0, 0});
        CHECK(!place_nodes(r.hm.data(), 3, 22, 11, &failed, msg, sizeof(msg)));
        CHECK(failed == 1u && r.hm[0].out_first == 11u);
        CHECK(std::string(msg) == "vd_bvh_build_batch: the packed node buffer is full at mesh 1 (or its node indices pass 2^32)");
    }
    {   // node indices are 32-bit: a range that would pass 2^32 is refused whatever the buffer holds
        uint32_t failed = 77u;
        char msg[512] = "";
        Numbered r = number(two_trees(), {1, 2}, {0, 0});
        CHECK(!place_nodes(r.hm.data(), 2, ~0ull, 0xfffffff8u, &failed, msg, sizeof(msg)));
        CHECK(failed == 1u && r.hm[0].out_first == 0xfffffff8u);
    }
}

int main() {
    single_meshes();
    several_meshes();
    refusals();
    if (g_fail) { printf("blas_top_test: %d checks failed\n", g_fail); return 1; }
    printf("blas_top_test OK\n");
    return 0;
}
