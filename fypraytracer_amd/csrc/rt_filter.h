// Query filters (fyprt_set_mesh_query_masks / fyprt_set_query_mask): every mesh carries a 32-bit group mask M[m], a query call one mask
// Q, and a triangle of mesh m is admitted iff (M[m] & Q) != 0.  The five query families (rt_query.h, rt_points.h, rt_boxes.h, rt_triangles.h) run their
// existing rules over the admitted leaf records only; frames, radiance queries, denoisers and edits never look at a mask.
//
// Derived data, built lazily on the context stream by the first filtered query after the table was set or the tree changed:
//   leafMask : one word per leaf record, in leaf order (the order the leaf test walks: no gather depends on the triangle index)
//   nodeMask : one word per node, the OR of leafMask over everything below the node
// k_filter_leaf_masks finds a record's mesh by binary search in the table of the meshes' first triangles (ascending, empty meshes left
// out); k_filter_level ORs the children's words, run over the refit passes' level grouping, levels = 1 first, so every child's word is
// written by an earlier launch.  An import or a regraft leaves a mesh as one sub-tree: excluding it costs one node word.
//
// The visit rule of the filtered lane states (LaneFilter<true>): before a node is fetched — the root and resume entries included — a lane
// whose nodeMask word does not meet Q pops instead; at a leaf a record whose leafMask word does not meet Q is skipped before its test.
// A masked node is no node visit and a masked record no triangle test to the ray counters.  LaneFilter<false> is empty and always
// admits: the unfiltered kernels are the code they were.  The mask is read in the lane's `start`, so a per-record mask array would
// touch no traversal code.
#pragma once
#include <type_traits>
#include "rt_device.h"

namespace rt {

struct QueryFilter { const uint32_t* nodeMask; const uint32_t* leafMask; uint32_t queryMask; };
// A query record with the filter behind it: what the filtered kernels take in place of Q
template <class Q> struct Filtered : Q { QueryFilter flt; };

template <bool FILTER> struct LaneFilter {
    template <class Q> RT_DEV void load(const Q&) {}
    RT_DEV bool node(int32_t) const { return true; }
    RT_DEV bool record(uint32_t) const { return true; }
};
template <> struct LaneFilter<true> {
    const uint32_t* nodeMask = nullptr; const uint32_t* leafMask = nullptr; uint32_t mask = 0u;
    template <class Q> RT_DEV void load(const Q& q) { nodeMask = q.flt.nodeMask; leafMask = q.flt.leafMask; mask = q.flt.queryMask; }
    // `cur` >= 0: an inner reference or a resume entry, both carry the node's byte offset
    RT_DEV bool node(int32_t cur) const { return (nodeMask[((uint32_t)cur & kNodeOffsetMask) >> 6] & mask) != 0u; }
    RT_DEV bool record(uint32_t leafRecord) const { return (leafMask[leafRecord] & mask) != 0u; }
};

// One thread per leaf record: the mask of the mesh that holds the record's triangle.  first[0 .. meshCount): the non-empty meshes' first
// triangles ascending (first[0] == 0: the meshes partition the triangle list), masks[] in the same order.
__global__ __launch_bounds__(256) void k_filter_leaf_masks(const float4* leafTris, uint32_t leafCount, const uint32_t* first, const uint32_t* masks,
                                                           uint32_t meshCount, uint32_t* leafMask) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= leafCount) return;
    const uint32_t tri = (uint32_t)__float_as_int(leafTris[(size_t)i * 3 + 2].y);
    uint32_t lo = 0u, hi = meshCount;                                   // the last k in [lo, hi) with first[k] <= tri
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (first[mid] <= tri) lo = mid; else hi = mid; }
    leafMask[i] = meshCount ? masks[lo] : 0u;
}

// One thread per listed node of one level: the OR of its children's words (leaf records: leafMask; inner children: nodeMask, written by
// the launches of the lower levels).  References in device form; a reference outside the arrays contributes nothing.
__global__ __launch_bounds__(128) void k_filter_level(const float4* nodes, const uint32_t* levelNodes, uint32_t count, uint32_t nodeCount,
                                                      const uint32_t* leafMask, uint32_t leafCount, uint32_t* nodeMask) {
    const uint32_t k = blockIdx.x * 128u + threadIdx.x;
    if (k >= count) return;
    const uint32_t node = levelNodes[k];
    if (node >= nodeCount) return;
    const float4 q0 = nodes[(size_t)node * 4], q1 = nodes[(size_t)node * 4 + 1];
    const uint32_t cnt = ((uint32_t)__float_as_int(q0.w) >> 24) & 7u;
    const int32_t ref[4] = {__float_as_int(q1.x), __float_as_int(q1.y), __float_as_int(q1.z), __float_as_int(q1.w)};
    uint32_t word = 0u;
    for (uint32_t i = 0; i < 4u; ++i) {
        if (i >= cnt) continue;
        if (ref[i] >= 0) {
            const uint32_t child = ((uint32_t)ref[i] & kNodeOffsetMask) >> 6;
            if (child < nodeCount) word |= nodeMask[child];
        } else {
            const uint32_t code = (uint32_t)~ref[i], firstRec = code >> 2, n = (code & 3u) + 1u;
            for (uint32_t j = 0; j < n; ++j) if (firstRec + j < leafCount) word |= leafMask[firstRec + j];
        }
    }
    nodeMask[node] = word;
}

}  // namespace rt
