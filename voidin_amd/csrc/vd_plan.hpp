// vd_plan.hpp — what the plan headers (blas_lbvh_plan.hpp, blas_refit_plan.hpp: pure host arithmetic, built by a host compiler
// alone in tests/cpp) share with the device code that trusts their tables.  No HIP and no VdCtx; vd_common.hpp includes it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/voidin_abi.h"

#ifdef __HIPCC__
#define VD_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define VD_HOST_DEVICE inline
#endif

// the batched slot space of tlas.hip's segmented sort (vd_lbvh_batch_sort_boxes, vd_common.hpp)
constexpr unsigned kVdLbvhBatchUnit = 256, kVdLbvhExtentChunk = 2048;
struct VdLbvhSeg { unsigned slot0, cap, n_units, _pad; };

// the MeshInfo fold (vd_common.hpp: vd_mesh_bounds_fold): vertices per block, and the neutral keys of its min / max
constexpr unsigned kVdVertChunk = 4096u;
constexpr int kVdKeyPosInf = 0x7f800000;               // vd_key(+inf): start (and re-armed value) of a min
constexpr int kVdKeyNegInf = (int)0x807fffff;          // vd_key(-inf): of a max

// A plan's tables are uploaded where the kernels read uint2 / uint4; the host arithmetic writes these (same size, asserted
// where they are cast).
struct VdPair { unsigned x, y; };
struct VdQuad { unsigned x, y, z, w; };

// blocks of one mesh's fold, {item, first vertex} each: an empty fold still writes (+inf, -inf)
static inline unsigned vd_fold_chunks(std::vector<VdPair>& chunks, unsigned item, unsigned n_vert) {
    const unsigned n = n_vert ? (unsigned)(((size_t)n_vert + kVdVertChunk - 1u) / kVdVertChunk) : 1u;
    for (unsigned c = 0; c < n; ++c) chunks.push_back(VdPair{item, c * kVdVertChunk});
    return n;
}
// per item: 3 min keys, 3 max keys, as they stand between two launches
static inline std::vector<int> vd_fold_neutral_keys(size_t n_items) {
    std::vector<int> keys(6 * n_items);
    for (size_t k = 0; k < keys.size(); ++k) keys[k] = k % 6 < 3 ? kVdKeyPosInf : kVdKeyNegInf;
    return keys;
}
