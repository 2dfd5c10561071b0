// blas_top.hpp — the pure host part of the SAH builder's copy-out (blas.hip, phase C): the final node numbers of the
// temporary top tree and where every mesh's nodes go.  No HIP and no VdCtx, so a host compiler builds it alone
// (tests/cpp/blas_top_test.cpp).  Everything is in the unnamed namespace of the one file that includes it.
//
// The rule (include/voidin_abi.h "vd_bvh_build", blas.rs:105-128): node 0 is the root and node 1 the never-used pad; a pair
// of nodes is taken when an interior node is VISITED in pre-order (left before right); a small root - a subtree that
// phase B built on its own - takes its 2 * sub_interior nodes in one piece when visited.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/voidin_abi.h"

namespace {

struct TopNode {                      // temporary top-tree node
    float mn[3]; unsigned start;
    float mx[3]; unsigned count;
    unsigned kind;                    // 0 leaf, 1 big interior, 2 small root (3: the pad slot 2m + 1 of mesh m)
    unsigned left;                    // tmp id of the left child (right = left + 1) for kind 1
    unsigned small;                   // index into the small-root list for kind 2
    unsigned pad;
};

struct TopOut { unsigned final_index, pair, mesh; };   // pair = final left_first for interior nodes; mesh: whose node array

// One mesh of a build, host side.  d_out == nullptr: packed - the mesh's nodes follow the previous mesh's in the batch's
// shared node buffer (MeshPool's `bvh_index = bvh_nodes.len()` bookkeeping, mesh/mod.rs:320-345).
struct BuildMesh {
    const float* d_verts; uint32_t n_vert; uint32_t* d_idx; uint32_t n_tri; VdBvhNode* d_out; uint32_t node_cap;
    uint32_t out_n_nodes, out_first;
};

// Pre-order walk of every mesh's tree (root of mesh m = tmp node 2m), one after the other.  Needs the top tree alone, so
// it runs while phase B does; `ord` records the visits of the nodes that take a pair, ord_end[m] where mesh m's end.
// Sets TopOut::mesh of every node, and the pad's entry whole.
inline void top_preorder(const TopNode* top, uint32_t K, TopOut* out, unsigned* ord, unsigned* ord_end) {
    unsigned n_ord = 0;
    std::vector<unsigned> stk;
    for (uint32_t m = 0; m < K; ++m) {
        stk.push_back(2u * m);
        while (!stk.empty()) {
            const unsigned v = stk.back(); stk.pop_back();
            const TopNode& t = top[v];
            out[v].mesh = m;
            if (t.kind == 0u) continue;
            ord[n_ord++] = v;
            if (t.kind == 1u) {
                stk.push_back(t.left + 1);
                stk.push_back(t.left);
            }
        }
        out[2u * m + 1u].mesh = m; out[2u * m + 1u].final_index = 1u; out[2u * m + 1u].pair = 0u;
        ord_end[m] = n_ord;
    }
}

// What depends on phase B - sub[r] = the interior nodes of small root r - enters in one linear pass over the recorded
// pre-order: every visited node's pair, its children's final indices, root_pair[r] = where small root r's nodes start,
// and hm[m].out_n_nodes = the mesh's node count.
inline void number_top(const TopNode* top, const unsigned* sub, uint32_t K, const unsigned* ord, const unsigned* ord_end,
                       TopOut* out, unsigned* root_pair, BuildMesh* hm) {
    unsigned k = 0;
    for (uint32_t m = 0; m < K; ++m) {
        unsigned pool = 2;
        out[2u * m].final_index = 0;
        for (; k < ord_end[m]; ++k) {
            const unsigned v = ord[k];
            const TopNode& t = top[v];
            const unsigned pair = pool;
            out[v].pair = pair;
            if (t.kind == 2u) {
                root_pair[t.small] = pair;
                pool += 2u * sub[t.small];
            } else {
                pool += 2;
                out[t.left].final_index = pair;
                out[t.left + 1].final_index = pair + 1;
            }
        }
        hm[m].out_n_nodes = pool;
    }
}

// Room for every mesh's nodes, in build order: its own array (node_cap), or the next out_n_nodes of the packed buffer
// from packed_first on (hm[m].out_first).  false: mesh *failed does not fit, `msg` says why.
inline bool place_nodes(BuildMesh* hm, uint32_t K, uint64_t packed_cap, uint32_t packed_first, uint32_t* failed, char* msg, size_t msg_len) {
    uint64_t packed_at = packed_first;
    for (uint32_t m = 0; m < K; ++m) {
        const uint32_t pool = hm[m].out_n_nodes;
        hm[m].out_first = 0;
        if (hm[m].d_out) {
            if (pool > hm[m].node_cap) {
                *failed = m;
                snprintf(msg, msg_len, "vd_bvh_build: node_cap too small (mesh %u of the build needs %u nodes)", m, pool);
                return false;
            }
        } else {
            if (packed_at + pool > packed_cap || packed_at + pool > 0xffffffffull) {     // out_first_node / bvh_index are 32-bit
                *failed = m;
                snprintf(msg, msg_len, "vd_bvh_build_batch: the packed node buffer is full at mesh %u (or its node indices pass 2^32)", m);
                return false;
            }
            hm[m].out_first = (uint32_t)packed_at;
            packed_at += pool;
        }
    }
    return true;
}

}  // namespace
