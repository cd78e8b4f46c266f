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
//   k_graft_node_boxes    exact node boxes of a tree no refit pass has run on yet (a host-built one): what k_refit_level reads of the
//                         children of the nodes it is run on
//   k_refit_level (rt_refit.h) over the new nodes, lowest level first, then over R / the new root: one box and quantisation rule
//                         on the device whichever builder made the sub-tree
// The tree grows by one level about every third append (two more children for a full root's successor, then a new root again); a
// result deeper than the traversal stack allows is rebuilt as an upload builds it (fyprt.hip: fyprt_append_meshes).
// This header is part of fyprt.hip (it uses the context and its helpers) and is included there once.
#pragma once
#include "rt_refit.h"

extern "C++" {
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

// One thread.  fresh = 0: `ref1` becomes child `slot` of `node`, whose meta byte (count | levels << 3) becomes `meta`.  fresh = 1:
// `node` becomes a new node of the children (ref0, ref1).  Boxes, exponents and planes are k_refit_level's.  References in device form.
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

// nodeBox of the listed nodes of one level (levels = 1 first), nothing else written: the box half of k_refit_level
__global__ __launch_bounds__(128) void k_graft_node_boxes(const float4* nodes, const uint32_t* levelNodes, uint32_t count, const float4* leafTris, const float4* triPos, float4* nodeBox) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint32_t node = levelNodes[k];
    const float4* n = nodes + (size_t)node * 4;
    const float4 q0 = n[0], q1 = n[1];
    const uint32_t cnt = ((uint32_t)__float_as_int(q0.w) >> 24) & 7u;
    const int32_t child[4] = {__float_as_int(q1.x), __float_as_int(q1.y), __float_as_int(q1.z), __float_as_int(q1.w)};
    RBox cb[4]; RBox nb;
    refit_child_boxes(cnt, child, leafTris, triPos, nodeBox, cb, nb);
    nodeBox[(size_t)node * 2] = make_float4(nb.lo[0], nb.lo[1], nb.lo[2], 0.0f);
    nodeBox[(size_t)node * 2 + 1] = make_float4(nb.hi[0], nb.hi[1], nb.hi[2], 0.0f);
}

}  // namespace rt

// ---- host side
constexpr int kGraftRebuild = -1001;        // the grafted tree would exceed the traversal stack or the node range: rebuild it

// Host-only contexts quantise with the builder's own quantiser from what the tree itself holds: a node's box is its exact lower corner
// (the grid origin) and its conservative upper planes; a leaf's box is exact, from the vertices.
static rth::ChildBox graft_plane_box(const rth::Node& n, int i) {       // child i of n, from its planes
    rth::ChildBox b;
    for (int a = 0; a < 3; ++a) {
        const float s = std::ldexp(1.0f, (int)n.ex[a] - 127);
        b.lo[a] = std::fmaf((float)n.qlo[a][i], s, n.origin[a]); b.hi[a] = std::fmaf((float)n.qhi[a][i], s, n.origin[a]);
    }
    return b;
}
static rth::ChildBox graft_host_box(const fyprt_context* c, int32_t ref) {
    rth::ChildBox b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = 3.402823466e+38f; b.hi[a] = -3.402823466e+38f; }
    if (ref >= 0) {
        const rth::Node& n = c->hostBvh.nodes[(size_t)ref];
        for (int i = 0; i < (int)(n.meta & 7u); ++i) { const rth::ChildBox cb = graft_plane_box(n, i); for (int a = 0; a < 3; ++a) b.hi[a] = std::max(b.hi[a], cb.hi[a]); }
        for (int a = 0; a < 3; ++a) b.lo[a] = n.origin[a];
        return b;
    }
    const uint32_t code = (uint32_t)~ref, first = code >> 2, m = (code & 3u) + 1u;
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t* t = &c->topoTris[(size_t)c->hostBvh.tris[first + j].tri * 4];
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) { const float v = c->hostVerts[t[k]].position[a]; b.lo[a] = std::min(b.lo[a], v); b.hi[a] = std::max(b.hi[a], v); }
    }
    return b;
}

// The sub-tree over the appended triangles [firstTri, firstTri + nT) = the meshes `meshes` (first_triangle absolute), built and grafted
// into the tree of c.  The per-triangle records of the range are on the device, the host's topology (c->topoTris) and vertices
// (c->hostVerts, valid for every vertex the range uses) hold the combined scene; `newVerts`: the appended vertices (the Morton grid of a
// device build).  Returns kGraftRebuild, with the tree untouched, when the result would be too deep or too large.
static int graft_append(fyprt_context* c, const fyprt_vertex* newVerts, uint32_t nV, uint32_t firstTri, uint32_t nT, const fyprt_mesh* meshes, uint32_t meshCount) {
    rth::SceneBVH& hb = c->hostBvh;
    const size_t leafBase = hb.tris.size(), nodeBase = hb.nodes.size();
    c->linksValid = false;                     // new nodes, new records, maybe a new root: the partial refit's maps are rebuilt
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
    // 2. where it goes
    const int32_t R = hb.rootRef;
    const bool empty = leafBase == 0, attach = !empty && R >= 0 && (hb.nodes[(size_t)R].meta & 7u) < 4u, newRoot = !empty && !attach;
    const uint32_t rLevels = (!empty && R >= 0) ? (uint32_t)(hb.nodes[(size_t)R].meta >> 3) : 0u;
    const uint32_t levels = empty ? subLevels : attach ? std::max(rLevels, subLevels + 1u) : 1u + std::max(rLevels, subLevels);
    const size_t total = nodeBase + subNodes + (newRoot ? 1u : 0u);
    if (levels > rth::kStackBudget || total >= (size_t)rth::kMaxNodes) { c->leafTris.n = leafBase * 3; return kGraftRebuild; }
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
    if (!c->hostOnly && !c->nodeBoxValid && !empty) {
        for (uint32_t l = 1; l < (uint32_t)c->levelOffset.size() - 1u; ++l) {
            const uint32_t first = c->levelOffset[l], count = c->levelOffset[l + 1] - first;
            if (count) hipLaunchKernelGGL(k_graft_node_boxes, dim3((count + 127u) / 128u), dim3(128), 0, c->stream, (const float4*)c->nodes.p, (const uint32_t*)(c->levelNodes.p + first), count, (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p);
        }
    }
    // 4. the link, in the host's copy (topology and level counts; on a host-only context the planes too) and on the device
    const uint32_t linked = empty ? ~0u : attach ? (uint32_t)R : (uint32_t)(total - 1);        // the node that is refitted last
    if (attach) {
        rth::Node& r = hb.nodes[(size_t)R];
        const uint32_t k = r.meta & 7u;
        if (c->hostOnly) {
            rth::ChildBox boxes[4]; int32_t child[4];
            for (uint32_t i = 0; i < k; ++i) { boxes[i] = graft_plane_box(r, (int)i); child[i] = r.child[i]; }
            boxes[k] = graft_host_box(c, S);
            rth::QuantiseNode(r, boxes, (int)k + 1);
            for (uint32_t i = 0; i < 4; ++i) r.child[i] = i < k ? child[i] : INT32_MIN;
        }
        r.child[k] = S; r.meta = (uint8_t)((k + 1u) | (levels << 3));
        if (!c->hostOnly) hipLaunchKernelGGL(k_graft_link, dim3(1), dim3(64), 0, c->stream, c->nodes.p, (uint32_t)R, k, 0, rth::device_ref(S), (uint32_t)r.meta, 0);
    } else if (newRoot) {
        rth::Node& r = hb.nodes[total - 1];
        std::memset(&r, 0, sizeof r);
        if (c->hostOnly) { const rth::ChildBox boxes[2] = {graft_host_box(c, R), graft_host_box(c, S)}; rth::QuantiseNode(r, boxes, 2); }
        r.child[0] = R; r.child[1] = S; r.child[2] = r.child[3] = INT32_MIN; r.meta = (uint8_t)(2u | (levels << 3));
        if (!c->hostOnly) hipLaunchKernelGGL(k_graft_link, dim3(1), dim3(64), 0, c->stream, c->nodes.p, (uint32_t)(total - 1), 0u, rth::device_ref(R), rth::device_ref(S), (uint32_t)r.meta, 1);
    }
    // 5. boxes and quantisation of the new nodes, then of the linked one
    if (!c->hostOnly) {
        std::vector<uint32_t> byLevel(rth::kStackBudget + 2u, 0u);
        for (uint32_t i = 0; i < subNodes; ++i) byLevel[(hb.nodes[nodeBase + i].meta >> 3) + 1u]++;
        for (size_t l = 1; l < byLevel.size(); ++l) byLevel[l] += byLevel[l - 1];
        std::vector<uint32_t> list(subNodes + 1u), fill(byLevel);
        for (uint32_t i = 0; i < subNodes; ++i) list[fill[hb.nodes[nodeBase + i].meta >> 3]++] = (uint32_t)nodeBase + i;
        list[subNodes] = linked;
        if (c->graftList.n < list.size()) HIPCHK(c, c->graftList.alloc(std::max(list.size(), 2 * c->graftList.n)));
        TRY(upload(c, c->graftList.p, list.data(), list.size() * 4));
        for (size_t l = 1; l + 1 < byLevel.size(); ++l) {
            const uint32_t first = byLevel[l], count = byLevel[l + 1] - first;
            if (count) hipLaunchKernelGGL(k_refit_level, dim3((count + 127u) / 128u), dim3(128), 0, c->stream, c->nodes.p, (const uint32_t*)(c->graftList.p + first), count, (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p);
        }
        if (linked != ~0u) hipLaunchKernelGGL(k_refit_level, dim3(1), dim3(128), 0, c->stream, c->nodes.p, (const uint32_t*)(c->graftList.p + subNodes), 1u, (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p);
        HIPCHK(c, hipGetLastError());
        c->nodeBoxValid = true; c->hostBvhStale = true;       // the boxes of the new nodes live on the device: an export reads the tree back
    }
    hb.rootRef = empty ? S : attach ? R : (int32_t)(total - 1); hb.levels = levels;
    // 6. the level grouping, regrouped on the host: 4 bytes per node cross the bus (once the launches above have read the old one)
    if (!c->hostOnly) HIPCHK(c, hipStreamSynchronize(c->stream));
    return upload_level_grouping(c, true);
}

}  // extern "C++"
