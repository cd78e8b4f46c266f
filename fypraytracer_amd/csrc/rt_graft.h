// The acceleration structure of an append (fyprt_append_meshes; the reference's "Import Mesh", Scene::CreateNewMeshInScene,
// Scene.cpp:241-290, which builds the new mesh's BLAS and the small TLAS): a sub-tree over the appended triangles only, grafted
// into the live tree at its root.  Everything the old scene owns keeps its index and its bytes, except the root when it takes the
// sub-tree as one more child.
//   sub-tree     tuning key 12 as for an upload: the host builder over the new meshes, or the device builder (rt_lbvh.h) over the
//                appended triangle range, its leaf records written behind the old ones and its nodes copied behind the old nodes
//   k_graft_rebase        the device-built nodes where they lie: inner references and leaf codes moved from the sub-tree's own
//                         numbering (node 0, leaf record 0) to their place in the arrays
//   k_graft_link          the sub-tree root S and the old root R: S becomes one more child of an R that has a free slot, otherwise
//                         a new two-child node (R, S) behind all others becomes the root; the level counts stay exact
//   k_graft_node_boxes (rt_refit.h, run by ensure_node_boxes) exact node boxes of a tree no refit pass has run on yet (a host-built one): what k_refit_level reads of the
//                         children of the nodes it is run on
//   k_refit_level (rt_refit.h) over the new nodes, lowest level first: one box and quantisation rule on the device whichever builder
//                         made the sub-tree
//   k_graft_place         fyprt_set_append_placement(ctx, 1): the cheapest place for S by the surface-area rule of include/fyprt.h instead
//                         of the root — one thread per old inner node over the partial refit's parent links (rt_partial.h) and nodeBox
//   k_graft_path          the nodes whose children changed (a new pair node, the node that took S, its ancestors; just R / the new root in
//                         mode 0): their meta bytes, then refit_node on each, lowest first, by ONE thread in one launch
// In mode 0 the tree grows by one level about every third append (two more children for a full root's successor, then a new root again); a
// result deeper than the traversal stack allows is rebuilt as an upload builds it (fyprt.hip: fyprt_append_meshes).
// This header is part of fyprt.hip (it uses the context and its helpers, rt_tree_host.h among them) and is included there once.
#pragma once
#include "rt_refit.h"
#include "rt_partial.h"      // partial_ensure_links: the parent links the placement search walks

namespace rt {

// nodes [0, count) of a device-built sub-tree at `nodes`: inner references + nodeBase (a byte offset), leaf codes + leafBase records
__global__ void k_graft_rebase(float4* nodes, uint32_t count, int32_t nodeBase, uint32_t leafBase) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    float4* n = nodes + (size_t)k * 4;
    const uint32_t cnt = ((uint32_t)__float_as_int(n[0].w) >> 24) & 7u;
    const float4 q1 = n[1];
    int32_t child[4] = {__float_as_int(q1.x), __float_as_int(q1.y), __float_as_int(q1.z), __float_as_int(q1.w)};
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        if (i < cnt) child[i] = child[i] >= 0 ? child[i] + nodeBase : ~(int32_t)((uint32_t)~child[i] + (leafBase << 2));
    n[1] = make_float4(__int_as_float(child[0]), __int_as_float(child[1]), __int_as_float(child[2]), __int_as_float(child[3]));
}

// One thread.  fresh = 0: `ref1` becomes child `slot` of `node` (one more child, or a new pair node in place of the child that was
// there), whose meta byte (count | levels << 3) becomes `meta`.  fresh = 1: `node` becomes a new node of the children (ref0, ref1).  Boxes, exponents and planes are k_refit_level's.  References in device form.
__global__ void k_graft_link(float4* nodes, uint32_t node, uint32_t slot, int32_t ref0, int32_t ref1, uint32_t meta, int fresh) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    float4* n = nodes + (size_t)node * 4;
    if (fresh) {
        n[0] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float((int)(meta << 24)));
        n[1] = make_float4(__int_as_float(ref0), __int_as_float(ref1), __int_as_float((int)0x80000000), __int_as_float((int)0x80000000));
        n[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); n[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float4 q0 = n[0], q1 = n[1];
    q0.w = __int_as_float((int)(((uint32_t)__float_as_int(q0.w) & 0x00FFFFFFu) | (meta << 24)));
    const float r = __int_as_float(ref1);
    if (slot == 0u) q1.x = r; else if (slot == 1u) q1.y = r; else if (slot == 2u) q1.z = r; else q1.w = r;
    n[0] = q0; n[1] = q1;
}

// ---- placement by surface-area cost (fyprt_set_append_placement(ctx, 1); the rule: include/fyprt.h).  Plain binary32 expressions, every
// operation rounded on its own (the build sets -ffp-contract=off for host and device alike); the same functions serve the kernel and the
// host-only search.
#define RT_HD __host__ __device__ __forceinline__
RT_HD float place_area(const RBox& b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    const float xy = dx * dy, yz = dy * dz, zx = dz * dx;
    const float s = xy + yz;
    return s + zx;
}
RT_HD float place_union_area(const RBox& a, const RBox& b) {
    RBox u;
    for (int k = 0; k < 3; ++k) { u.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k]; u.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k]; }
    return place_area(u);
}
RT_HD float place_growth(const RBox& y, const RBox& B) { const float u = place_union_area(y, B), a = place_area(y); return u - a; }
// one candidate offered to a thread's best key ((cost bits << 32) | id) and candidate count; costs are >= +0, so their bits order as they do
RT_HD void place_offer(bool feasible, float cost, uint32_t id, unsigned long long& best, uint32_t& found) {
    uint32_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __float_as_uint(cost);
#else
    std::memcpy(&bits, &cost, 4);
#endif
    if (!feasible || (bits & 0x7FFFFFFFu) >= 0x7F800000u) return;
    const unsigned long long key = ((unsigned long long)bits << 32) | id;
    best = key < best ? key : best; ++found;
}
// What the host knows before the search: the appended box, the sub-tree's level count, which kinds the node range still allows, and
// whether the root pair is feasible (its new root levels <= 31)
struct PlaceParams { RBox B; uint32_t subLevels, slotOk, pairOk, rootPairOk, root; };
// The (up to five) candidates at node X and, at the root, the root pair.  acc = P(X), depth = d(X), levelsX / childLevels from the meta
// bytes, cb / nb = the exact boxes of X's children / of X.
RT_HD void place_candidates(const PlaceParams& pp, uint32_t X, uint32_t cnt, uint32_t levelsX, const uint32_t (&childLevels)[4], const RBox (&cb)[4], const RBox& nb,
                            float acc, uint32_t depth, unsigned long long& best, uint32_t& found) {
    const uint32_t h = pp.subLevels;
    if (cnt < 4u) { const uint32_t hX = levelsX > h + 1u ? levelsX : h + 1u; place_offer(pp.slotOk && depth + hX <= 31u, acc, X * 8u + 4u, best, found); }
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {                // (unrolled: the child boxes stay in registers, as in refit_child_boxes)
        if (i >= cnt) continue;
        const uint32_t hN = 1u + (childLevels[i] > h ? childLevels[i] : h), hX = levelsX > hN + 1u ? levelsX : hN + 1u;
        const float u = place_union_area(cb[i], pp.B);
        place_offer(pp.pairOk && depth + hX <= 31u, acc + u, X * 8u + i, best, found);
    }
    if (X == pp.root) place_offer(pp.rootPairOk != 0u, place_union_area(nb, pp.B), 0xFFFFFFFFu, best, found);
}

// One thread per old inner node X: its children's exact boxes, the walk up the parent links for P(X) and d(X), its candidates; the best key
// of a wave by shuffles, then one 64-bit atomicMin (and one add of the candidate count) per wave: out[0] = best key, out[1] = candidates.
__global__ __launch_bounds__(256) void k_graft_place(const float4* nodes, uint32_t nNodes, const float4* leafTris, const float4* triPos, const float4* nodeBox,
                                                     const uint32_t* nodeParent, PlaceParams pp, unsigned long long* out) {
    const uint32_t X = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long best = ~0ull; uint32_t found = 0;
    if (X < nNodes) {
        const float4* n = nodes + (size_t)X * 4;
        const float4 q0 = n[0], q1 = n[1];
        const uint32_t w = (uint32_t)__float_as_int(q0.w), cnt = (w >> 24) & 7u, levelsX = w >> 27;
        const int32_t child[4] = {__float_as_int(q1.x), __float_as_int(q1.y), __float_as_int(q1.z), __float_as_int(q1.w)};
        RBox cb[4]; RBox nb;
        refit_child_boxes(cnt, child, leafTris, triPos, nodeBox, cb, nb);
        uint32_t childLevels[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t ci = (uint32_t)child[i] >> 6;
            if (i < cnt && child[i] >= 0 && ci < nNodes) childLevels[i] = (uint32_t)__float_as_int(nodes[(size_t)ci * 4].w) >> 27;
        }
        float acc = place_growth(nb, pp.B);
        uint32_t depth = 0;
        for (uint32_t p = nodeParent[X]; p < nNodes && depth < 64u; p = nodeParent[p]) {
            const float4 l = nodeBox[(size_t)p * 2], hgh = nodeBox[(size_t)p * 2 + 1];
            RBox y; y.lo[0] = l.x; y.lo[1] = l.y; y.lo[2] = l.z; y.hi[0] = hgh.x; y.hi[1] = hgh.y; y.hi[2] = hgh.z;
            acc = acc + place_growth(y, pp.B);
            ++depth;
        }
        place_candidates(pp, X, cnt, levelsX, childLevels, cb, nb, acc, depth, best, found);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(best, off); const uint32_t f = __shfl_down(found, off);
        best = o < best ? o : best; found += f;
    }
    if ((threadIdx.x & 63u) == 0u && found) { atomicMin(out, best); atomicAdd(out + 1, (unsigned long long)found); }
}

// One thread: the meta bytes (count | levels << 3) of the `count` listed nodes, then their refit in list order, lowest first, each
// reading what the one before wrote: the new pair node, the node that took the sub-tree and its ancestors up to the root.
__global__ void k_graft_path(float4* nodes, const uint32_t* list, const uint32_t* metas, uint32_t count, const float4* leafTris, const float4* triPos, float4* nodeBox) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    for (uint32_t k = 0; k < count; ++k) {
        float4* n = nodes + (size_t)list[k] * 4;
        const float w = n[0].w;
        n[0].w = __int_as_float((int)(((uint32_t)__float_as_int(w) & 0x00FFFFFFu) | (metas[k] << 24)));
    }
    for (uint32_t k = 0; k < count; ++k) refit_node(nodes, list[k], leafTris, triPos, nodeBox);
}

}  // namespace rt

// ---- host side

constexpr int kGraftRebuild = -1001;        // the grafted tree would exceed the traversal stack or the node range: rebuild it

// parent[i] of the tree's inner nodes (the root keeps ~0u)
static void graft_parents(const rth::SceneBVH& hb, std::vector<uint32_t>& parent) {
    parent.assign(hb.nodes.size(), ~0u);
    for (uint32_t i = 0; i < (uint32_t)hb.nodes.size(); ++i)
        for (uint32_t k = 0; k < (hb.nodes[i].meta & 7u); ++k) if (hb.nodes[i].child[k] >= 0) parent[(size_t)hb.nodes[i].child[k]] = i;
}
// The placement search of a host-only context: k_graft_place's arithmetic in its order, node by node.  Exact boxes bottom-up from the
// vertices (the host's copy of the tree holds quantised planes only).  res[0] = the best key, res[1] = the candidates.
static void graft_place_host(const fyprt_context* c, const PlaceParams& pp, std::vector<uint32_t>& parent, unsigned long long (&res)[2]) {
    const std::vector<rth::Node>& hn = c->hostBvh.nodes;
    const uint32_t n = (uint32_t)hn.size();
    graft_parents(c->hostBvh, parent);
    const std::vector<RBox> box = host_exact_boxes(c);
    unsigned long long best = ~0ull; uint32_t found = 0;
    for (uint32_t X = 0; X < n; ++X) {
        const uint32_t cnt = hn[X].meta & 7u;
        RBox cb[4]; uint32_t childLevels[4] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < 4 && i < cnt; ++i) { cb[i] = host_child_box(c, box, hn[X].child[i]); if (hn[X].child[i] >= 0) childLevels[i] = hn[(size_t)hn[X].child[i]].meta >> 3; }
        float acc = place_growth(box[X], pp.B);
        uint32_t depth = 0;
        for (uint32_t p = parent[X]; p != ~0u; p = parent[p]) { acc = acc + place_growth(box[p], pp.B); ++depth; }
        place_candidates(pp, X, cnt, hn[X].meta >> 3, childLevels, cb, box[X], acc, depth, best, found);
    }
    res[0] = best; res[1] = found;
}

// The sub-tree over the appended triangles [firstTri, firstTri + nT) = the meshes `meshes` (first_triangle absolute), built and grafted
// into the tree of c.  The per-triangle records of the range are on the device, the host's topology (c->topoTris) and vertices
// (c->hostVerts, valid for every vertex the range uses) hold the combined scene; `newVerts`: the appended vertices (the Morton grid of a
// device build).  Returns kGraftRebuild, with the tree untouched, when the result would be too deep or too large.
static int graft_append(fyprt_context* c, const fyprt_vertex* newVerts, uint32_t nV, uint32_t firstTri, uint32_t nT, const fyprt_mesh* meshes, uint32_t meshCount) {
    rth::SceneBVH& hb = c->hostBvh;
    const size_t leafBase = hb.tris.size(), nodeBase = hb.nodes.size();
    // 1. the sub-tree: S (relative to the sub-tree), its node count and levels
    bool onDevice = !c->hostOnly && c->tuning[K_BUILDER] != 0 && nT > 4;
    DevBuf<float4> wide; LbvhTree tree; rth::SceneBVH sub;
    if (onDevice) {
        TRY(grow_buffer(c, c->leafTris, (leafBase + nT) * 3));
        const int rc = build_device_lbvh(c, newVerts, nV, firstTri, nT, c->tuning[K_BUILDER] == 2, leafBase, wide, &tree);
        if (rc == kLbvhTooDeep) onDevice = false;
        else if (rc != FYPRT_OK) return rc;
    }
    if (!onDevice) rth::BuildSceneBVH(c->hostVerts.data(), (const uint8_t*)c->topoTris.data(), 16, meshes, meshCount, sub);
    const uint32_t subNodes = onDevice ? tree.nodes : (uint32_t)sub.nodes.size(), subLevels = onDevice ? tree.levels : sub.levels;
    auto rebased = [&](int32_t ref) { return ref >= 0 ? ref + (int32_t)nodeBase : ~(int32_t)((uint32_t)~ref + ((uint32_t)leafBase << 2)); };
    const int32_t S = rebased(onDevice ? 0 : sub.rootRef);
    // 2. where it goes: the root (mode 0, an empty tree, a leaf-code root) or the cheapest place (mode 1)
    const int32_t R = hb.rootRef;
    const bool empty = leafBase == 0, search = c->appendPlacement == 1 && !empty && R >= 0;
    const uint32_t rLevels = (!empty && R >= 0) ? (uint32_t)(hb.nodes[(size_t)R].meta >> 3) : 0u;
    if (!search) c->linksValid = false;        // new nodes, new records, maybe a new root: the partial refit's maps are rebuilt (a search reads them first)
    fyprt_append_placement& rep = c->placement;
    rep = fyprt_append_placement{(uint32_t)c->appendPlacement, 0u, 0u, 0u, 0u, 0u, hb.levels, 0u, 0u};
    enum : uint32_t { kFirst = 0, kSlot = 1, kPair = 2, kRootPair = 3 };
    uint32_t kind = kFirst, X = 0, slot = 0;
    std::vector<uint32_t> parent;               // of the old nodes, when the place may lie below the root
    if (search) {
        PlaceParams pp;
        pp.B = to_rbox(tri_range_box(c, firstTri, nT));
        pp.subLevels = subLevels; pp.root = (uint32_t)R;
        pp.slotOk = nodeBase + subNodes < (size_t)rth::kMaxNodes ? 1u : 0u; pp.pairOk = nodeBase + subNodes + 1u < (size_t)rth::kMaxNodes ? 1u : 0u;
        pp.rootPairOk = pp.pairOk && 1u + std::max(rLevels, subLevels) <= rth::kStackBudget ? 1u : 0u;
        unsigned long long res[2] = {~0ull, 0ull};
        if (c->hostOnly) graft_place_host(c, pp, parent, res);
        else {
            TRY(partial_ensure_links(c));          // parent links and exact boxes of the old tree (the sub-tree is not linked yet)
            if (c->placeOut.n != 2) HIPCHK(c, c->placeOut.alloc(2));
            HIPCHK(c, hipMemsetAsync(c->placeOut.p, 0xFF, 8, c->stream)); HIPCHK(c, hipMemsetAsync(c->placeOut.p + 1, 0, 8, c->stream));
            hipLaunchKernelGGL(k_graft_place, dim3(((uint32_t)nodeBase + 255u) / 256u), dim3(256), 0, c->stream, (const float4*)c->nodes.p, (uint32_t)nodeBase, (const float4*)c->leafTris.p,
                               (const float4*)c->triPos.p, (const float4*)c->nodeBox.p, (const uint32_t*)c->nodeParent.p, pp, c->placeOut.p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(res, c->placeOut.p, 16, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        c->linksValid = false;
        if (res[0] == ~0ull) { c->leafTris.n = leafBase * 3; return kGraftRebuild; }
        const uint32_t id = (uint32_t)res[0];
        rep.cost_bits = (uint32_t)(res[0] >> 32); rep.candidates = (uint32_t)res[1];
        if (id == 0xFFFFFFFFu) kind = kRootPair;
        else { X = id >> 3; kind = (id & 7u) == 4u ? kSlot : kPair; slot = kind == kSlot ? (uint32_t)(hb.nodes[X].meta & 7u) : (id & 7u); }
        if (kind != kRootPair && (X >= nodeBase || slot >= 4u)) return c->fail(FYPRT_EHIP, "fyprt_append_meshes: the placement search returned no node of the tree");
        if (kind != kRootPair && X != (uint32_t)R && parent.empty()) graft_parents(hb, parent);
    } else if (!empty) {
        const bool attach = R >= 0 && (hb.nodes[(size_t)R].meta & 7u) < 4u;
        kind = attach ? kSlot : kRootPair;
        if (attach) { X = (uint32_t)R; slot = hb.nodes[X].meta & 7u; }
        const uint32_t levels = attach ? std::max(rLevels, subLevels + 1u) : 1u + std::max(rLevels, subLevels);
        if (levels > rth::kStackBudget || nodeBase + subNodes + (attach ? 0u : 1u) >= (size_t)rth::kMaxNodes) { c->leafTris.n = leafBase * 3; return kGraftRebuild; }
    }
    const bool fresh = kind == kPair || kind == kRootPair;
    const size_t total = nodeBase + subNodes + (fresh ? 1u : 0u);
    if (kind == kFirst && (subLevels > rth::kStackBudget || total >= (size_t)rth::kMaxNodes)) { c->leafTris.n = leafBase * 3; return kGraftRebuild; }
    // 3. the sub-tree's nodes and leaf records behind the old ones, on the device and in the host's copy
    TRY(grow_buffer(c, c->nodes, total * 4)); TRY(grow_buffer(c, c->nodeBox, total * 2));
    hb.nodes.resize(total); hb.tris.resize(leafBase + nT);
    if (onDevice) {
        hipLaunchKernelGGL(k_refresh_leaf_tris, dim3((nT + 255u) / 256u), dim3(256), 0, c->stream, c->triPos.p, c->leafTris.p + leafBase * 3, nT);
        HIPCHK(c, hipMemcpyAsync(c->nodes.p + nodeBase * 4, wide.p, (size_t)subNodes * 64, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(k_graft_rebase, dim3((subNodes + 255u) / 256u), dim3(256), 0, c->stream, c->nodes.p + nodeBase * 4, subNodes, (int32_t)(nodeBase << rth::kNodeRefShift), (uint32_t)leafBase);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hb.nodes.data() + nodeBase, c->nodes.p + nodeBase * 4, (size_t)subNodes * 64, hipMemcpyDeviceToHost, c->stream));   // topology + meta of the new nodes
        HIPCHK(c, hipStreamSynchronize(c->stream));
        rth::nodes_to_host_form(hb.nodes.data() + nodeBase, subNodes);
    } else {
        for (uint32_t i = 0; i < subNodes; ++i) {
            rth::Node n = sub.nodes[i];
            for (uint32_t k = 0; k < (n.meta & 7u); ++k) n.child[k] = rebased(n.child[k]);
            hb.nodes[nodeBase + i] = n;
        }
        std::copy(sub.tris.begin(), sub.tris.end(), hb.tris.begin() + leafBase);
        if (!c->hostOnly) {
            std::vector<rth::Node> dn(hb.nodes.begin() + nodeBase, hb.nodes.begin() + nodeBase + subNodes);
            rth::nodes_to_device_form(dn.data(), dn.size());
            TRY(grow_buffer(c, c->leafTris, (leafBase + nT) * 3));
            TRY(upload(c, c->nodes.p + nodeBase * 4, dn.data(), dn.size() * 64));
            TRY(upload(c, c->leafTris.p + leafBase * 3, sub.tris.data(), sub.tris.size() * 48));
        } else c->leafTris.n = c->leafTris.cap = (leafBase + nT) * 3;
    }
    // (a tree no refit pass has run on: the exact boxes of the old nodes first, once — the old grouping still describes them)
    TRY(ensure_node_boxes(c));
    // 4. the link, in the host's copy (topology and level counts; on a host-only context the planes too) and on the device.  `path`: the
    // nodes whose children changed, lowest first — the new pair node, the node that took the sub-tree, its ancestors up to the root
    const uint32_t N = (uint32_t)(total - 1);
    std::vector<uint32_t> path;
    if (fresh) {
        rth::Node& n = hb.nodes[N];
        std::memset(&n, 0, sizeof n);
        n.child[0] = kind == kPair ? hb.nodes[X].child[slot] : R; n.child[1] = S; n.child[2] = n.child[3] = INT32_MIN; n.meta = 2u;
        if (!c->hostOnly) hipLaunchKernelGGL(k_graft_link, dim3(1), dim3(64), 0, c->stream, c->nodes.p, N, 0u, rth::device_ref(n.child[0]), rth::device_ref(S), 2u, 1);
        path.push_back(N);
    }
    const bool legacy = c->hostOnly && !search && kind == kSlot;     // mode 0 keeps R's old children on R's own planes, byte for byte
    rth::ChildBox legacyBoxes[4];
    if (legacy) for (uint32_t i = 0; i < slot; ++i) legacyBoxes[i] = graft_plane_box(hb.nodes[X], (int)i);
    if (kind == kSlot || kind == kPair) {
        rth::Node& x = hb.nodes[X];
        x.child[slot] = kind == kPair ? (int32_t)N : S;
        if (kind == kSlot) x.meta = (uint8_t)((x.meta & 0xF8u) | (slot + 1u));
        for (uint32_t p = X; p != ~0u; p = p == (uint32_t)R ? ~0u : parent[p]) path.push_back(p);
        rep.depth = (uint32_t)path.size() - (fresh ? 2u : 1u);
    }
    std::vector<uint32_t> metas(path.size());
    for (size_t k = 0; k < path.size(); ++k) {
        rth::Node& n = hb.nodes[path[k]];
        uint32_t lv = 0;
        for (uint32_t i = 0; i < (n.meta & 7u); ++i) if (n.child[i] >= 0) lv = std::max(lv, (uint32_t)(hb.nodes[(size_t)n.child[i]].meta >> 3));
        n.meta = (uint8_t)((n.meta & 7u) | ((lv + 1u) << 3));
        metas[k] = n.meta;
        if (c->hostOnly) host_requantise(c, path[k], legacyBoxes, legacy ? slot : 0u);     // as the prune does it: the children's boxes from what the tree holds
    }
    if (!c->hostOnly && (kind == kSlot || kind == kPair))
        hipLaunchKernelGGL(k_graft_link, dim3(1), dim3(64), 0, c->stream, c->nodes.p, X, slot, 0, rth::device_ref(hb.nodes[X].child[slot]), (uint32_t)hb.nodes[X].meta, 0);
    // 5. boxes and quantisation of the new nodes, level by level, then of the path in one launch
    if (!c->hostOnly) {
        LevelGroups sub = group_by_level(hb.nodes.data() + nodeBase, subNodes, rth::kStackBudget, kEveryNode);
        std::vector<uint32_t>& list = sub.order;                      // the new nodes by level, then the path, then the path's meta bytes
        for (uint32_t& i : list) i += (uint32_t)nodeBase;
        list.insert(list.end(), path.begin(), path.end()); list.insert(list.end(), metas.begin(), metas.end());
        if (c->graftList.n < list.size()) HIPCHK(c, c->graftList.alloc(std::max(list.size(), 2 * c->graftList.n)));
        TRY(upload(c, c->graftList.p, list.data(), list.size() * 4));
        for_each_level(sub.offsets, [&](uint32_t first, uint32_t count, dim3 grid) {
            hipLaunchKernelGGL(k_refit_level, grid, dim3(kLevelBlock), 0, c->stream, c->nodes.p, (const uint32_t*)(c->graftList.p + first), count, (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p);
        });
        if (!path.empty()) hipLaunchKernelGGL(k_graft_path, dim3(1), dim3(64), 0, c->stream, c->nodes.p, (const uint32_t*)(c->graftList.p + subNodes), (const uint32_t*)(c->graftList.p + subNodes + path.size()),
                                              (uint32_t)path.size(), (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p);
        HIPCHK(c, hipGetLastError());
        c->nodeBoxValid = true; c->hostBvhStale = true;       // the boxes of the new nodes live on the device: an export reads the tree back
    }
    hb.rootRef = kind == kFirst ? S : kind == kRootPair ? (int32_t)N : R;
    hb.levels = hb.rootRef >= 0 ? (uint32_t)(hb.nodes[(size_t)hb.rootRef].meta >> 3) : 0u;
    rep.kind = kind; rep.node = kind == kSlot || kind == kPair ? X : 0u; rep.slot = kind == kSlot || kind == kPair ? slot : 0u; rep.levels_after = hb.levels;
    c->linksValid = false;                     // new nodes, new records, maybe a new root: the partial refit's maps are rebuilt
    // 6. the level grouping, regrouped on the host: 4 bytes per node cross the bus (once the launches above have read the old one)
    if (!c->hostOnly) HIPCHK(c, hipStreamSynchronize(c->stream));
    return upload_level_grouping(c, true);
}

// graft_append, or, where the graft would be too deep or too large, the tree of the whole scene as an upload builds it (`who`: the
// caller's name for its error texts), reported as kind 4.  The host builder reads every vertex: the first `staleVerts` of the host's
// copy come back first if device edits left them behind.  `rebuilt`: NULL, or set when the tree was rebuilt.
static int graft_or_rebuild(fyprt_context* c, const char* who, const fyprt_vertex* newVerts, uint32_t nV, uint32_t firstTri, uint32_t nT, const fyprt_mesh* meshes, uint32_t meshCount,
                            uint32_t staleVerts, bool* rebuilt = nullptr) {
    int rc = graft_append(c, newVerts, nV, firstTri, nT, meshes, meshCount);
    if (rc != kGraftRebuild) return rc;
    TRY(ensure_host_verts(c, staleVerts, true));
    rc = build_scene_tree(c, who, c->hostVerts.data(), c->vertexCount, (const uint8_t*)c->topoTris.data(), 16, c->topoMeshes.data(), (uint32_t)c->topoMeshes.size(), (uint32_t)(c->topoTris.size() / 4));
    c->placement.kind = 4u; c->placement.node = c->placement.slot = c->placement.depth = c->placement.cost_bits = c->placement.candidates = 0u;
    c->placement.levels_after = c->hostBvh.levels;
    if (rebuilt) *rebuilt = true;
    return rc;
}
