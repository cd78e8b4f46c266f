// Surface-area cost of the tree as it is (fyprt_tree_cost; new, no reference counterpart): what an application reads to decide that a
// moved mesh should be regrafted (fyprt_regraft_meshes), and what shows that the regraft helped.  With A, b(Y) and the exact leaf boxes of
// the placement rule (include/fyprt.h; place_area of rt_graft.h: binary32, every operation rounded on its own):
//   root area    (double) A(b(R)); of a leaf-code root its exact leaf box; 0 for an empty tree
//   inner area   sum over inner nodes Y of (double) A(b(Y))
//   leaf area    sum over leaf children (first, n) of n * (double) A(exact box of those n triangles); a leaf-code root is the one leaf child
//   k_tree_cost  one thread per node: its own box from nodeBox (every node's exact box: a tree no refit pass has run on gets the
//                k_graft_node_boxes passes first), its leaf children's boxes from triPos through the leaf records (refit_child_boxes); both
//                sums reduced over the wave by shuffles, over the workgroup's four waves in LDS, always in the same order; one (inner,
//                leaf) pair per workgroup into a partials buffer by ordinary stores, the root's area in front of them.  No atomics: the
//                host adds the pairs in workgroup order, so two calls on the same tree return the same bits
// The host-only restatement adds the same terms node by node.  Summation orders differ between the two, so they agree to a tolerance: at
// most 2^26 non-negative terms (2^24 nodes, four children each), any order within (n - 1) * 2^-53 <= 2^-27 relative of the exact sum, two
// orders within 2^-26 relative of each other.
// This header is part of fyprt.hip (it uses the context and its helpers) and is included there once, after rt_prune.h.
#pragma once
#include "rt_graft.h"

namespace rt {

constexpr uint32_t kCostBlock = 256;

// partials[0] = root area, partials[2 + 2 * block] = (inner, leaf) of the workgroup.  nNodes == 0: the root is a leaf code, thread 0 of
// the one workgroup takes it as the only child of a node that is not there (as k_tree_links does).
__global__ __launch_bounds__(kCostBlock) void k_tree_cost(const float4* nodes, uint32_t nNodes, int32_t rootRef, const float4* leafTris, const float4* triPos, const float4* nodeBox, double* partials) {
    __shared__ double s_part[kCostBlock / 64][2];
    const uint32_t X = blockIdx.x * kCostBlock + threadIdx.x;
    double inner = 0.0, leaf = 0.0;
    if (X < nNodes || (nNodes == 0u && X == 0u && rootRef < 0)) {
        int32_t child[4] = {rootRef, 0, 0, 0};
        uint32_t cnt = 1;
        if (nNodes) {
            const float4* n = nodes + (size_t)X * 4;
            const float4 q1 = n[1];
            cnt = ((uint32_t)__float_as_int(n[0].w) >> 24) & 7u;
            child[0] = __float_as_int(q1.x); child[1] = __float_as_int(q1.y); child[2] = __float_as_int(q1.z); child[3] = __float_as_int(q1.w);
            const float4 l = nodeBox[(size_t)X * 2], h = nodeBox[(size_t)X * 2 + 1];
            RBox own; own.lo[0] = l.x; own.lo[1] = l.y; own.lo[2] = l.z; own.hi[0] = h.x; own.hi[1] = h.y; own.hi[2] = h.z;
            inner = (double)place_area(own);
            if ((int32_t)(X << 6) == rootRef) partials[0] = inner;
        }
        RBox cb[4]; RBox nb;
        refit_child_boxes(cnt, child, leafTris, triPos, nodeBox, cb, nb);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (i < cnt && child[i] < 0) leaf = leaf + (double)(((uint32_t)~child[i] & 3u) + 1u) * (double)place_area(cb[i]);
        if (nNodes == 0u) partials[0] = (double)place_area(cb[0]);
    }
    for (int off = 32; off > 0; off >>= 1) { inner = inner + __shfl_down(inner, off); leaf = leaf + __shfl_down(leaf, off); }
    if ((threadIdx.x & 63u) == 0u) { s_part[threadIdx.x >> 6][0] = inner; s_part[threadIdx.x >> 6][1] = leaf; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        double* out = partials + 2 + 2 * (size_t)blockIdx.x;
        out[0] = (s_part[0][0] + s_part[1][0]) + (s_part[2][0] + s_part[3][0]);
        out[1] = (s_part[0][1] + s_part[1][1]) + (s_part[2][1] + s_part[3][1]);
    }
}

}  // namespace rt

// ---- host side

// The sums of a host-only context, from its topology copy and the vertices: exact boxes bottom-up, then the terms in node order
static void tree_cost_host(const fyprt_context* c, fyprt_tree_cost_sums* out) {
    const rth::SceneBVH& hb = c->hostBvh;
    const std::vector<rth::Node>& hn = hb.nodes;
    const uint32_t n = (uint32_t)hn.size();
    auto leaf_term = [&](int32_t ref) { return (double)(((uint32_t)~ref & 3u) + 1u) * (double)place_area(to_rbox(graft_host_box(c, ref))); };
    if (n == 0) {                                        // a leaf-code root: the one leaf child
        out->root_area = (double)place_area(to_rbox(graft_host_box(c, hb.rootRef)));
        out->leaf_area = leaf_term(hb.rootRef);
        return;
    }
    const std::vector<RBox> box = host_exact_boxes(c);
    for (uint32_t X = 0; X < n; ++X) {
        double leaf = 0.0;
        for (uint32_t i = 0; i < (hn[X].meta & 7u); ++i) if (hn[X].child[i] < 0) leaf = leaf + leaf_term(hn[X].child[i]);
        out->inner_area += (double)place_area(box[X]); out->leaf_area += leaf;
    }
    out->root_area = (double)place_area(box[(size_t)hb.rootRef]);
}

// The call proper, after every check, all streams idle.  The counts come from the host's topology copy, which every edit keeps current.
static int tree_cost(fyprt_context* c, fyprt_tree_cost_sums* out) {
    const rth::SceneBVH& hb = c->hostBvh;
    *out = fyprt_tree_cost_sums{0.0, 0.0, 0.0, (uint32_t)hb.nodes.size(), 0u, (uint32_t)hb.tris.size(), hb.levels};
    if (hb.tris.empty()) return FYPRT_OK;
    for (const rth::Node& n : hb.nodes) for (uint32_t i = 0; i < (n.meta & 7u); ++i) out->leaf_children += n.child[i] < 0 ? 1u : 0u;
    if (hb.nodes.empty()) out->leaf_children = 1u;
    if (c->hostOnly) { tree_cost_host(c, out); return FYPRT_OK; }
    const uint32_t nNodes = out->nodes, blocks = std::max(1u, (nNodes + kCostBlock - 1u) / kCostBlock);
    const size_t words = 2u + 2u * (size_t)blocks;
    if (c->costPartials.n < words) HIPCHK(c, c->costPartials.alloc(std::max(words, 2 * c->costPartials.n)));
    TRY(ensure_node_boxes(c));
    hipLaunchKernelGGL(k_tree_cost, dim3(blocks), dim3(kCostBlock), 0, c->stream, (const float4*)c->nodes.p, nNodes, rth::device_ref(hb.rootRef), (const float4*)c->leafTris.p,
                       (const float4*)c->triPos.p, (const float4*)c->nodeBox.p, c->costPartials.p);
    HIPCHK(c, hipGetLastError());
    std::vector<double> part(words);
    HIPCHK(c, hipMemcpyAsync(part.data(), c->costPartials.p, words * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->root_area = part[0];
    for (uint32_t b = 0; b < blocks; ++b) { out->inner_area += part[2 + 2 * (size_t)b]; out->leaf_area += part[3 + 2 * (size_t)b]; }
    return FYPRT_OK;
}
