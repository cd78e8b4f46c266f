// Partial refit: a geometry edit of a few meshes at the cost of what moved (fyprt_update_mesh_vertices, and fyprt_update_transforms with
// tuning key 22 = 1).  The full pass (rt_refit.h, run_refit) rewrites every leaf record and every node; this one walks up from the moved
// triangles:
//   k_tree_links            once per topology, one thread per node: nodeParent[child] for inner children (the root keeps ~0u),
//                           leafParent[j] for every record j of a leaf child, leafOfTri[triangle of record j] = j
//   k_partial_seed          one thread per moved triangle t: leaf record leafOfTri[t] rewritten (refresh_leaf_record), its node marked
//                           dirty; the thread that finds the flag clear appends the node to the list of the node's level
//   k_partial_refit_level   levels 1..L in ascending order (a parent's level exceeds its child's), one thread per listed node: the node
//                           refitted (refit_node), its flag cleared, its parent marked and listed the same way
//   k_partial_refit_tail    the same for the top levels in ONE launch of one workgroup, a barrier between two levels: from the first level
//                           on above which no level can list more than kPartialTail nodes (the host knows min(nodes of the level, moved
//                           triangles)).  The walk is bound by its launches, not by its work (profiles/partial_refit): a 16-triangle
//                           edit takes one launch for all 14 levels of the 1M-triangle hall
// A dirty node reads nodeBox of its clean inner children, so nodeBox must hold every node's exact box: a tree no refit pass has run on
// gets the k_graft_node_boxes pass first, once.  A node's result depends on its children only, never on the order of a list.
// Afterwards every node with a moved triangle below it has the bytes and the nodeBox the full pass writes; every other node and every
// record of an unmoved triangle keeps its bytes.  Flags are cleared by the nodes themselves and the (at most 32) list counts by a
// 128-byte memset: once the links exist, no launch runs over all triangles, all records or all nodes.
// Flags and counts are plain words in global memory, touched inside a launch by agent-scope vector atomics only.
// This header is part of fyprt.hip (it uses the context and its helpers, rt_tree_host.h among them) and is included there once.
#pragma once
#include "rt_refit.h"

namespace rt {

constexpr uint32_t kPartialLevels = 32;         // list counts: [l] = dirty nodes of level l (1..31), [0] = leaf records rewritten
constexpr uint32_t kPartialTail = 256;          // dirty nodes of one level the tail kernel's workgroup takes in one pass
// first list slot of every level: the level grouping's offsets (fyprt_context::levelOffset), the unused tail repeats the node count
struct PartialLevels { uint32_t first[kPartialLevels + 1]; };

__global__ void k_tree_links(const float4* nodes, uint32_t nNodes, int32_t rootRef, const float4* leafTris, uint32_t nLeaf, uint32_t nT,
                             uint32_t* nodeParent, uint32_t* leafParent, uint32_t* leafOfTri) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t child[4] = {rootRef, 0, 0, 0};      // a tree whose root is a leaf code has no nodes: thread 0 links the root's records to ~0u
    uint32_t cnt = 1, self = ~0u;
    if (nNodes) {
        if (k >= nNodes) return;
        const float4* n = nodes + (size_t)k * 4;
        const float4 q1 = n[1];
        cnt = ((uint32_t)__float_as_int(n[0].w) >> 24) & 7u; self = k;
        child[0] = __float_as_int(q1.x); child[1] = __float_as_int(q1.y); child[2] = __float_as_int(q1.z); child[3] = __float_as_int(q1.w);
    } else if (k != 0u || rootRef >= 0) return;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        if (i >= cnt) continue;
        if (child[i] >= 0) {
            const uint32_t ci = (uint32_t)child[i] >> 6;                 // device form: byte offset of the child node (rt_host.h)
            if (ci < nNodes) nodeParent[ci] = self;
        } else {
            const uint32_t code = (uint32_t)~child[i], first = code >> 2, m = (code & 3u) + 1u;
            for (uint32_t j = first; j < first + m && j < nLeaf; ++j) {
                leafParent[j] = self;
                const uint32_t tri = (uint32_t)__float_as_int(leafTris[(size_t)j * 3 + 2].y);
                if (tri < nT) leafOfTri[tri] = j;
            }
        }
    }
}

// Test-and-set of a node's dirty flag; `level` of the node from its meta byte (count | levels << 3, the top byte of the first quad)
RT_DEV bool partial_mark(uint32_t node, uint32_t nNodes, const float4* nodes, uint32_t* dirty, uint32_t& level) {
    level = ~0u;
    if (node >= nNodes || atomicExch(dirty + node, 1u) != 0u) return false;
    level = (uint32_t)__float_as_int(nodes[(size_t)node * 4].w) >> 27;
    return level >= 1u && level < kPartialLevels;
}

// The lanes of a wave that marked a node append it to the list of its level: one atomic per wave and level present (every lane of the
// wave calls this; lanes with nothing to append pass push = false)
RT_DEV void partial_append(bool push, uint32_t node, uint32_t level, uint32_t* lists, uint32_t* counters, const PartialLevels& lv) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long pending = __ballot(push);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(level, leader));
        const bool mine = push && level == l;
        const unsigned long long mask = __ballot(mine);
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(counters + l, (uint32_t)__popcll(mask));
        base = __shfl(base, leader);
        if (mine) {
            const uint32_t slot = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (slot < lv.first[l + 1] - lv.first[l]) lists[lv.first[l] + slot] = node;      // (a node is listed once: the level's segment holds them all)
        }
        pending &= ~mask;
    }
}

__global__ __launch_bounds__(256) void k_partial_seed(uint32_t firstTri, uint32_t triCount, const float4* triPos, float4* leafTris, uint32_t nLeaf,
                                                      const uint32_t* leafOfTri, const uint32_t* leafParent, const float4* nodes, uint32_t nNodes,
                                                      uint32_t* dirty, uint32_t* lists, uint32_t* counters, PartialLevels lv) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t node = ~0u, level = ~0u;
    bool found = false;
    if (k < triCount) {
        const uint32_t j = leafOfTri[firstTri + k];
        if (j < nLeaf) { found = true; refresh_leaf_record(triPos, leafTris, j); node = leafParent[j]; }
    }
    const bool push = found && partial_mark(node, nNodes, nodes, dirty, level);
    const unsigned long long rewritten = __ballot(found);
    if ((threadIdx.x & 63u) == 0u && rewritten) atomicAdd(counters, (uint32_t)__popcll(rewritten));
    partial_append(push, node, level, lists, counters, lv);
}

// Entry k of a level's list (`active`: there is one): the node refitted, its flag cleared, its parent marked and listed.  Every lane of
// a wave calls this together.
RT_DEV void partial_refit_entry(bool active, const uint32_t* list, uint32_t k, float4* nodes, uint32_t nNodes, const float4* leafTris, const float4* triPos, float4* nodeBox,
                                const uint32_t* nodeParent, uint32_t* dirty, uint32_t* lists, uint32_t* counters, const PartialLevels& lv) {
    uint32_t parent = ~0u, level = ~0u;
    if (active) {
        const uint32_t node = list[k];
        if (node < nNodes) {
            refit_node(nodes, node, leafTris, triPos, nodeBox);
            __hip_atomic_store(dirty + node, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // nothing below this level is still running: nobody marks it again
            parent = nodeParent[node];
        }
    }
    const bool push = partial_mark(parent, nNodes, nodes, dirty, level);
    partial_append(push, parent, level, lists, counters, lv);
}

// `list`: the segment of this launch's level, `count`: its counter (complete: every launch that appends to it has ended)
__global__ __launch_bounds__(128) void k_partial_refit_level(float4* nodes, uint32_t nNodes, const uint32_t* list, const uint32_t* count, uint32_t capacity,
                                                             const float4* leafTris, const float4* triPos, float4* nodeBox, const uint32_t* nodeParent,
                                                             uint32_t* dirty, uint32_t* lists, uint32_t* counters, PartialLevels lv) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = *count < capacity ? *count : capacity;
    partial_refit_entry(k < n, list, k, nodes, nNodes, leafTris, triPos, nodeBox, nodeParent, dirty, lists, counters, lv);
}

// Levels [firstLevel, lastLevel] by ONE workgroup.  Between two levels an agent-scope fence and the workgroup's barrier: what the threads
// stored for the level below (nodes, boxes, list entries) is complete and this CU's L1 holds no older copy of it; a level's count is
// final by then (only lower levels append to it) and is read as the atomics left it.  Every trip count is the same for all threads.
__global__ __launch_bounds__(256) void k_partial_refit_tail(float4* nodes, uint32_t nNodes, uint32_t firstLevel, uint32_t lastLevel, const float4* leafTris, const float4* triPos,
                                                            float4* nodeBox, const uint32_t* nodeParent, uint32_t* dirty, uint32_t* lists, uint32_t* counters, PartialLevels lv) {
    if (blockIdx.x != 0u) return;
    for (uint32_t l = firstLevel; l <= lastLevel && l < kPartialLevels; ++l) {
        const uint32_t capacity = lv.first[l + 1] - lv.first[l];
        uint32_t n = __hip_atomic_load(counters + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(n < capacity ? n : capacity));
        for (uint32_t base = 0; base < n; base += blockDim.x)
            partial_refit_entry(base + threadIdx.x < n, lists + lv.first[l], base + threadIdx.x, nodes, nNodes, leafTris, triPos, nodeBox, nodeParent, dirty, lists, counters, lv);
        __threadfence();
        __syncthreads();
    }
}

}  // namespace rt

// ---- host side

// The three maps and the scratch of the walk, (re)built for the tree as it is: 4 bytes per node, leaf record and triangle for the maps,
// 8 bytes per node (lists, flags) + 128 bytes (counts) for the scratch.  Kept until the topology changes (fyprt_context::linksValid).
static int partial_ensure_links(fyprt_context* c) {
    const uint32_t nNodes = (uint32_t)c->hostBvh.nodes.size(), nLeaf = (uint32_t)c->hostBvh.tris.size(), nT = (uint32_t)(c->topoTris.size() / 4);
    if (!c->linksValid) {
        if (c->nodeParent.n != nNodes) { HIPCHK(c, c->nodeParent.alloc(nNodes)); HIPCHK(c, c->partialLists.alloc(nNodes)); HIPCHK(c, c->partialDirty.alloc(nNodes)); }
        if (c->leafParent.n != nLeaf) HIPCHK(c, c->leafParent.alloc(nLeaf));
        if (c->leafOfTri.n != nT) HIPCHK(c, c->leafOfTri.alloc(nT));
        if (c->partialCounters.n != kPartialLevels) HIPCHK(c, c->partialCounters.alloc(kPartialLevels));
        HIPCHK(c, c->partialCountsHost.alloc(kPartialLevels));               // page-locked: the counts' way back does not stall the stream
        if (nNodes) { HIPCHK(c, hipMemsetAsync(c->nodeParent.p, 0xFF, c->nodeParent.bytes(), c->stream)); HIPCHK(c, hipMemsetAsync(c->partialDirty.p, 0, c->partialDirty.bytes(), c->stream)); }
        if (nLeaf) HIPCHK(c, hipMemsetAsync(c->leafParent.p, 0xFF, c->leafParent.bytes(), c->stream));
        if (nT) HIPCHK(c, hipMemsetAsync(c->leafOfTri.p, 0xFF, c->leafOfTri.bytes(), c->stream));
        if (nLeaf) {
            const uint32_t threads = std::max(nNodes, 1u);
            hipLaunchKernelGGL(k_tree_links, dim3((threads + 255u) / 256u), dim3(256), 0, c->stream, (const float4*)c->nodes.p, nNodes, rth::device_ref(c->hostBvh.rootRef),
                               (const float4*)c->leafTris.p, nLeaf, nT, c->nodeParent.p, c->leafParent.p, c->leafOfTri.p);
            HIPCHK(c, hipGetLastError());
        }
        c->linksValid = true;
    }
    return ensure_node_boxes(c);
}

// The walk for the listed meshes (distinct), whose new world vertices the context stream has written or will have written by now:
// per-triangle records of their ranges, their leaf records, every node above them.  Enqueues only; the caller synchronises, then
// completes the edit's statistics with partial_finish_stats.
static int run_partial_refit(fyprt_context* c, const std::vector<uint32_t>& meshes) {
    fyprt_edit_stats& st = c->editStats;
    st = fyprt_edit_stats{1u, 0u, 0u, 0u, 0u}; c->haveEditStats = true;
    uint32_t moved = 0;
    for (uint32_t m : meshes) moved += c->topoMeshes[m].triangle_count;
    if (!moved) return FYPRT_OK;
    TRY(partial_ensure_links(c));
    const uint32_t nNodes = (uint32_t)c->hostBvh.nodes.size(), nLeaf = (uint32_t)c->hostBvh.tris.size();
    PartialLevels lv;
    for (uint32_t l = 0; l <= kPartialLevels; ++l) lv.first[l] = nNodes ? c->levelOffset[std::min<size_t>(l, c->levelOffset.size() - 1u)] : 0u;
    HIPCHK(c, hipMemsetAsync(c->partialCounters.p, 0, c->partialCounters.bytes(), c->stream));
    for (uint32_t m : meshes) {
        const uint32_t first = c->topoMeshes[m].first_triangle, n = c->topoMeshes[m].triangle_count;
        if (!n) continue;
        TRY(launch_refresh_triangles(c, first, n));
        hipLaunchKernelGGL(k_partial_seed, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, first, n, (const float4*)c->triPos.p, c->leafTris.p, nLeaf, (const uint32_t*)c->leafOfTri.p,
                           (const uint32_t*)c->leafParent.p, (const float4*)c->nodes.p, nNodes, c->partialDirty.p, c->partialLists.p, c->partialCounters.p, lv);
    }
    // nodes of one level have disjoint sub-trees: a level lists at most min(its nodes, moved triangles) of them.  The levels from
    // `tail` on, none of which can list more than kPartialTail, go to one workgroup in one launch.
    const uint32_t L = nNodes ? std::min(c->hostBvh.levels, kPartialLevels - 1u) : 0u;
    uint32_t tail = L + 1u;
    while (tail > 1u && std::min(lv.first[tail] - lv.first[tail - 1u], moved) <= kPartialTail) --tail;
    for (uint32_t l = 1; l < tail; ++l) {
        const uint32_t capacity = std::min(lv.first[l + 1] - lv.first[l], moved);
        if (!capacity) continue;
        hipLaunchKernelGGL(k_partial_refit_level, dim3((capacity + 127u) / 128u), dim3(128), 0, c->stream, c->nodes.p, nNodes, (const uint32_t*)(c->partialLists.p + lv.first[l]),
                           (const uint32_t*)(c->partialCounters.p + l), capacity, (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p, (const uint32_t*)c->nodeParent.p,
                           c->partialDirty.p, c->partialLists.p, c->partialCounters.p, lv);
        ++st.level_launches;
    }
    if (tail <= L) {
        hipLaunchKernelGGL(k_partial_refit_tail, dim3(1), dim3(256), 0, c->stream, c->nodes.p, nNodes, tail, L, (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p,
                           (const uint32_t*)c->nodeParent.p, c->partialDirty.p, c->partialLists.p, c->partialCounters.p, lv);
        ++st.level_launches;
    }
    HIPCHK(c, hipGetLastError());
    // the counts come back behind everything else the edit enqueues: partial_finish_stats reads them after the edit's last synchronisation
    HIPCHK(c, hipMemcpyAsync(c->partialCountsHost.p, c->partialCounters.p, c->partialCounters.bytes(), hipMemcpyDeviceToHost, c->stream));
    st.triangles_refreshed = moved; c->partialCountsPending = true;
    return FYPRT_OK;
}

// ... once the context stream is idle again: the counts into the edit's statistics
static void partial_finish_stats(fyprt_context* c) {
    if (!c->partialCountsPending) return;
    c->partialCountsPending = false;
    c->editStats.leaf_records_refreshed = c->partialCountsHost.p[0];
    for (uint32_t l = 1; l < kPartialLevels; ++l) c->editStats.nodes_refit += c->partialCountsHost.p[l];
}

// what the full passes of an edit cover
static void full_edit_stats(fyprt_context* c) {
    fyprt_edit_stats& st = c->editStats;
    st = fyprt_edit_stats{0u, (uint32_t)(c->topoTris.size() / 4), (uint32_t)c->hostBvh.tris.size(), (uint32_t)c->hostBvh.nodes.size(), 0u};
    for_each_level(c->levelOffset, [&](uint32_t, uint32_t, dim3) { ++st.level_launches; });
    c->haveEditStats = true;
}
