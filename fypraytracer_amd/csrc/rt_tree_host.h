// Host helpers shared by whatever builds or edits the scene's tree (fyprt.hip; rt_graft.h, rt_prune.h, rt_partial.h, rt_treecost.h): the
// sweep over a list of nodes grouped by level and the grouping itself, the host's boxes, the re-quantisation of a node of the host's
// copy, the host's vertices after device edits, the descriptor's tree fields, and the two launches every edit ends with.  Nothing here
// synchronises or copies unless its comment says so.
// This header is part of fyprt.hip (it uses the context and its helpers) and is included there once, ahead of the builders.
#pragma once

// ---- nodes by level
constexpr uint32_t kLevelBlock = 128;           // threads of a workgroup of the per-level kernels: one per listed node
// `launch(first, count, grid)` for every level that lists nodes, lowest level first.  offsets[l] = the first list slot of level l (levels
// count from 1; offsets[0] = offsets[1] = 0) and offsets.back() = the list's length: the levels are 1 .. offsets.size() - 2.
template <class Launch> static void for_each_level(const std::vector<uint32_t>& offsets, Launch&& launch) {
    for (size_t l = 1; l + 1 < offsets.size(); ++l)
        if (const uint32_t count = offsets[l + 1] - offsets[l]) launch(offsets[l], count, dim3((count + kLevelBlock - 1u) / kLevelBlock));
}

// Counting sort by level (meta >> 3) of those of the `count` nodes at `nodes` that `take(i)` accepts: `order` = their indices i, level
// ascending, index ascending within a level; `offsets` as for_each_level reads them, for `levels` levels.  No node's level may exceed
// `levels` (it indexes `offsets`): a tree's levels are bounded by its root's, and builders and graft keep that within rth::kStackBudget
struct LevelGroups { std::vector<uint32_t> offsets, order; };
constexpr auto kEveryNode = [](uint32_t) { return true; };
template <class Take> static LevelGroups group_by_level(const rth::Node* nodes, size_t count, uint32_t levels, Take take) {
    LevelGroups g;
    g.offsets.assign(levels + 2u, 0u);
    for (uint32_t i = 0; i < (uint32_t)count; ++i) if (take(i)) g.offsets[(nodes[i].meta >> 3) + 1u]++;
    for (uint32_t l = 1; l <= levels + 1u; ++l) g.offsets[l] += g.offsets[l - 1];
    g.order.resize(g.offsets.back());
    std::vector<uint32_t> fill(g.offsets);
    for (uint32_t i = 0; i < (uint32_t)count; ++i) if (take(i)) g.order[fill[nodes[i].meta >> 3]++] = i;
    return g;
}

// The nodes of the host's copy of the tree grouped by level (levels = 1 first) for the refit pass: c->levelOffset and, on the device,
// c->levelNodes — 4 bytes per node.  `keep`: the buffer grows within its capacity (an append) instead of being allocated to size.
static int upload_level_grouping(fyprt_context* c, bool keep) {
    LevelGroups g = group_by_level(c->hostBvh.nodes.data(), c->hostBvh.nodes.size(), c->hostBvh.levels, kEveryNode);
    c->levelOffset.swap(g.offsets);
    if (!keep) return alloc_upload(c, c->levelNodes, g.order.data(), g.order.size());
    TRY(grow_buffer(c, c->levelNodes, g.order.size(), false));
    return upload(c, c->levelNodes.p, g.order.data(), c->levelNodes.bytes());
}

// nodeBox of every node of a tree no refit pass has run on (a host-built one), level by level, once: what k_refit_level, the partial
// walk, the placement search and the cost sums read of the children of the nodes they are run on.  The level grouping describes the
// tree the boxes are asked for (a graft asks before it regroups).
static int ensure_node_boxes(fyprt_context* c) {
    if (c->nodeBoxValid || c->hostOnly || c->levelOffset.empty() || !c->levelOffset.back()) return FYPRT_OK;
    for_each_level(c->levelOffset, [&](uint32_t first, uint32_t count, dim3 grid) {
        hipLaunchKernelGGL(k_graft_node_boxes, grid, dim3(kLevelBlock), 0, c->stream, (const float4*)c->nodes.p, (const uint32_t*)(c->levelNodes.p + first), count, (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p);
    });
    HIPCHK(c, hipGetLastError());
    c->nodeBoxValid = true;
    return FYPRT_OK;
}

// ---- boxes on the host
static RBox to_rbox(const rth::ChildBox& b) { RBox r; for (int a = 0; a < 3; ++a) { r.lo[a] = b.lo[a]; r.hi[a] = b.hi[a]; } return r; }
// the exact box of the triangles [firstTri, firstTri + count), from the host's topology and vertices
static void grow_triangle(const fyprt_context* c, rth::HostBox& b, uint32_t t) { for (int k = 0; k < 3; ++k) b.grow(c->hostVerts[c->topoTris[(size_t)t * 4 + k]].position); }
static rth::HostBox tri_range_box(const fyprt_context* c, uint32_t firstTri, uint32_t count) { rth::HostBox b; for (uint32_t t = firstTri; t < firstTri + count; ++t) grow_triangle(c, b, t); return b; }
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
    rth::HostBox b;
    if (ref >= 0) {
        const rth::Node& n = c->hostBvh.nodes[(size_t)ref];
        for (int i = 0; i < (int)(n.meta & 7u); ++i) b.merge(graft_plane_box(n, i));
        for (int a = 0; a < 3; ++a) b.lo[a] = n.origin[a];
        return b;
    }
    const uint32_t code = (uint32_t)~ref, first = code >> 2, m = (code & 3u) + 1u;
    for (uint32_t j = 0; j < m; ++j) grow_triangle(c, b, c->hostBvh.tris[first + j].tri);
    return b;
}
// The exact box of every node of the host's copy, bottom-up from the vertices (the copy holds quantised planes only); host_child_box:
// the box of a child reference from them
static RBox host_child_box(const fyprt_context* c, const std::vector<RBox>& box, int32_t ref) { return ref >= 0 ? box[(size_t)ref] : to_rbox(graft_host_box(c, ref)); }
static std::vector<RBox> host_exact_boxes(const fyprt_context* c) {
    const std::vector<rth::Node>& hn = c->hostBvh.nodes;
    std::vector<RBox> box(hn.size());
    for (uint32_t X : group_by_level(hn.data(), hn.size(), rth::kStackBudget, kEveryNode).order) {
        rth::HostBox nb;
        for (uint32_t i = 0; i < (hn[X].meta & 7u); ++i) nb.merge(host_child_box(c, box, hn[X].child[i]));
        box[X] = to_rbox(nb);
    }
    return box;
}

// Node `node` of the host's copy quantised again by the builder's quantiser, its children's boxes from what the tree holds
// (graft_host_box) but for the first `nFixed`, which are given; child references and meta byte stay.  Host-only contexts.
static void host_requantise(fyprt_context* c, uint32_t node, const rth::ChildBox* fixed = nullptr, uint32_t nFixed = 0) {
    rth::Node& n = c->hostBvh.nodes[node];
    const uint32_t cnt = n.meta & 7u; const uint8_t meta = n.meta;
    rth::ChildBox boxes[4]; int32_t child[4];
    for (uint32_t i = 0; i < 4; ++i) { child[i] = n.child[i]; if (i < cnt) boxes[i] = i < nFixed ? fixed[i] : graft_host_box(c, n.child[i]); }
    rth::QuantiseNode(n, boxes, (int)cnt);
    for (uint32_t i = 0; i < 4; ++i) n.child[i] = i < cnt ? child[i] : INT32_MIN;
    n.meta = meta;
}

// ---- the host's world vertices, which device transform edits leave behind (fyprt_context::hostVertsStale)
// the first `count` of them back in one blocking copy, `drain`: once the context stream is idle
static int ensure_host_verts(fyprt_context* c, uint32_t count, bool drain = false) {
    if (!c->hostVertsStale || c->hostOnly || !count) return FYPRT_OK;
    if (drain) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->hostVerts.data(), c->dverts.p, (size_t)count * sizeof(fyprt_vertex), hipMemcpyDeviceToHost));
    c->hostVertsStale = false;
    return FYPRT_OK;
}
// mesh m's range of them, enqueued on the context stream
static int read_back_mesh_verts(fyprt_context* c, uint32_t m) {
    const uint32_t first = c->meshFirstVertex[m], n = c->meshFirstVertex[m + 1] - first;
    if (n) HIPCHK(c, hipMemcpyAsync(c->hostVerts.data() + first, c->dverts.p + first, (size_t)n * sizeof(fyprt_vertex), hipMemcpyDeviceToHost, c->stream));
    return FYPRT_OK;
}

// ---- the scene descriptor's tree fields, and with them those of the per-triangle records of a scene of T triangles.  Every call that
// builds, grafts, prunes or regrafts ends here, so here the kept primary hits go (fyprt_context::KeptPrimary): another tree visits the
// triangles in another order, and hits at equal distance go by that order.  The query filter's node and leaf words describe the old
// node array and leaf order: the next filtered query builds them again.
static void set_scene_tree(fyprt_context* c) { c->drop_kept_primary(); c->filterValid = false; c->dsc.nodes = c->nodes.p; c->dsc.leafTris = c->leafTris.p; c->dsc.rootRef = rth::device_ref(c->hostBvh.rootRef); }
static void set_scene_triangles(fyprt_context* c, uint32_t T) { set_scene_tree(c); c->dsc.triCount = T; c->dsc.triPos = c->triPos.p; c->dsc.triShade = c->triShade.p; }

// ---- launches on the context stream
// the per-light records of the descriptor's emissive list, by the kernels' own arithmetic
static int launch_light_records(fyprt_context* c) {
    const uint32_t n = c->dsc.emissiveCount;
    if (c->hostOnly || !n) return FYPRT_OK;
    hipLaunchKernelGGL(k_build_light_records, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, c->dsc, c->lightRecs.p);
    HIPCHK(c, hipGetLastError());
    return FYPRT_OK;
}
// the per-triangle records of the triangles [firstTri, firstTri + n) from the device's vertices
static int launch_refresh_triangles(fyprt_context* c, uint32_t firstTri, uint32_t n) {
    if (!n) return FYPRT_OK;
    hipLaunchKernelGGL(k_refresh_triangles, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, c->dverts.p, c->triIdx.p + firstTri, c->triPos.p + (size_t)firstTri * 3, c->triShade.p + (size_t)firstTri * 4, n);
    HIPCHK(c, hipGetLastError());
    return FYPRT_OK;
}
