// Mesh removal on the device (fyprt_remove_meshes; new, no reference counterpart): the import of rt_graft.h in reverse.  The listed
// meshes' triangle ranges and the given vertex ranges leave every array the scene owns, survivors keep their order, and the 4-wide
// tree is pruned bottom-up instead of rebuilt.  Removed records are at most `mesh_count` sorted intervals, so "where does record r go"
// is a search in a small table (start, removed before) kept in LDS, and the destination is the source minus the shift:
//   k_prune_stream        one thread per 16-byte quad of a record stream (triIdx 1 quad, triPos 3, triShade 4, vertices 2), out of
//                         place into a buffer of the same capacity; triIdx also remaps its three vertex indices
//   k_prune_count         } ordered compaction where the survivors are not intervals: leaf records (dead = their triangle is removed;
//   k_emissive_scan       } the triangle index is remapped while scattering and the exclusive count of dead records before each
//   k_prune_scatter       } record is kept for the node pass), the emissive list, and the nodes' alive flags (-> new node indices).
//                         Positions come from a scan, never from atomics: the order is part of the contract (rt_materials.h)
//   k_prune_level         per node of one level (levels = 1 first): every child becomes its replacement — a leaf code (first - dead
//                         records before first, survivors in the range), the replacement of an inner child, or DEAD — and the survivors
//                         are compacted in slot order.  None: the node is dead.  One: the node is dead and replaced by that survivor in
//                         its parent (a splice).  Two or more: the node lives with the new count and levels = 1 + max(inner children)
//   k_prune_move          alive nodes and their boxes to their new index, inner references rebased
//   k_refit_level (rt_refit.h) over the surviving nodes that lost a triangle anywhere below them, lowest level first
// A node that lost nothing keeps every byte but its rebased references.  Removal never deepens the tree, so there is no rebuild.
// The host repeats the node pass on its topology copy (prune_host_tree) from the leaf records' dead counts — 4 bytes per leaf record are
// all that comes back from the device — so its copy of the tree, the refit list and the level grouping need no node read-back.
// This header is part of fyprt.hip (it uses the context and its helpers) and is included there once, after rt_graft.h.
#pragma once
#include <algorithm>
#include <utility>
#include "rt_graft.h"
#include "rt_materials.h"

namespace rt {

constexpr uint32_t kPruneLds = 1024;                  // table entries kept in LDS; a longer table is searched in global memory
constexpr int32_t kPruneDead = (int32_t)0x80000000;   // no survivor below (the unused-slot marker: never a leaf code or a reference)

// Table of K sorted, disjoint removed intervals: tab[i] = (start of interval i, records removed before it), tab[K] = (~0, all removed).
// Returns whether record r is removed; `shift` = records removed before a surviving r.  (host and device: one rule)
__host__ __device__ inline bool prune_lookup(const uint2* tab, uint32_t K, uint32_t r, uint32_t& shift) {
    uint32_t lo = 0, hi = K;                           // number of intervals that start at or before r
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (tab[mid].x <= r) lo = mid + 1u; else hi = mid; }
    shift = 0u;
    if (lo == 0u) return false;
    const uint2 a = tab[lo - 1u]; const uint32_t after = tab[lo].y;
    shift = after;
    return r - a.x < after - a.y;
}
// the table a workgroup searches: its LDS copy when it fits (the caller synchronises), else the global one
RT_DEV const uint2* prune_stage(const uint2* tab, uint32_t K, uint2* s_tab) {
    if (K > kPruneLds) return tab;
    for (uint32_t i = threadIdx.x; i <= K; i += blockDim.x) s_tab[i] = tab[i];
    return s_tab;
}

// quad q of the stream belongs to record q / QUADS; REMAP (triIdx): x, y, z are vertex indices, shifted through the vertex table
template <int QUADS, bool REMAP>
__global__ __launch_bounds__(kBlock) void k_prune_stream(const float4* src, float4* dst, unsigned long long nQuads, const uint2* tab, uint32_t K, const uint2* vtab, uint32_t VK) {
    __shared__ uint2 s_tab[kPruneLds + 1]; __shared__ uint2 s_vtab[REMAP ? kPruneLds + 1 : 1];
    const uint2* t = prune_stage(tab, K, s_tab);
    const uint2* vt = REMAP ? prune_stage(vtab, VK, s_vtab) : nullptr;
    __syncthreads();
    const unsigned long long q = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (q >= nQuads) return;
    uint32_t shift;
    if (prune_lookup(t, K, (uint32_t)(q / QUADS), shift)) return;
    float4 v = src[q];
    if (REMAP) {
        uint32_t s;
        (void)prune_lookup(vt, VK, (uint32_t)__float_as_int(v.x), s); v.x = __int_as_float((int)((uint32_t)__float_as_int(v.x) - s));
        (void)prune_lookup(vt, VK, (uint32_t)__float_as_int(v.y), s); v.y = __int_as_float((int)((uint32_t)__float_as_int(v.y) - s));
        (void)prune_lookup(vt, VK, (uint32_t)__float_as_int(v.z), s); v.z = __int_as_float((int)((uint32_t)__float_as_int(v.z) - s));
    }
    dst[q - (unsigned long long)shift * QUADS] = v;
}

// Entry j of an ordered compaction: does it survive, and (kinds 0, 1) the triangle it names and that triangle's shift.
//   KIND 0  leaf records (src = the 48-byte records)      KIND 1  the emissive list (src = triangle indices)      KIND 2  alive flags
//   KIND 3  leaf records whose triangles stay in the scene (fyprt_regraft_meshes): as kind 0, the triangle index is not remapped
template <int KIND> RT_DEV bool prune_alive(const void* src, uint32_t j, uint32_t n, const uint2* tab, uint32_t K, uint32_t& tri, uint32_t& shift) {
    tri = 0u; shift = 0u;
    if (j >= n) return false;
    if (KIND == 2) return ((const uint32_t*)src)[j] != 0u;
    tri = KIND == 0 || KIND == 3 ? (uint32_t)__float_as_int(((const float4*)src)[(size_t)j * 3 + 2].y) : ((const uint32_t*)src)[j];
    return !prune_lookup(tab, K, tri, shift);
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void k_prune_count(const void* src, uint32_t n, uint32_t perGroup, const uint2* tab, uint32_t K, uint32_t* counts) {
    __shared__ uint2 s_tab[kPruneLds + 1]; __shared__ uint32_t s_count[kBlock / 64];
    const uint2* t = KIND == 2 ? nullptr : prune_stage(tab, K, s_tab);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, begin = blockIdx.x * perGroup;
    uint32_t cnt = 0, tri, shift;
    for (uint32_t tile = 0; tile < perGroup; tile += kBlock)
        cnt += (uint32_t)__popcll(__ballot(prune_alive<KIND>(src, begin + tile + threadIdx.x, n, t, K, tri, shift)));
    if (lane == 0u) s_count[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);
}

// Survivor j goes to position p = survivors before it (the scan's offset of the workgroup + the tiles before + the rank in the tile).
//   KIND 0  out = leaf records: record p = record j with its triangle index shifted; aux[j] = j - p = dead records before j, j in [0, n]
//   KIND 3  the same, every byte of record j kept
//   KIND 1  out[p] = the shifted triangle index                     KIND 2  aux[j] = p for EVERY j < n (a dead node's is never read)
template <int KIND>
__global__ __launch_bounds__(kBlock) void k_prune_scatter(const void* src, uint32_t n, uint32_t perGroup, const uint2* tab, uint32_t K, const uint32_t* offsets, void* out, uint32_t outCount, uint32_t* aux) {
    __shared__ uint2 s_tab[kPruneLds + 1]; __shared__ uint32_t s_count[2][kBlock / 64];
    const uint2* t = KIND == 2 ? nullptr : prune_stage(tab, K, s_tab);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, begin = blockIdx.x * perGroup;
    uint32_t base = offsets[blockIdx.x];
    for (uint32_t tile = 0, par = 0; tile < perGroup; tile += kBlock, par ^= 1u) {
        const uint32_t j = begin + tile + threadIdx.x;
        uint32_t tri, shift;
        const bool alive = prune_alive<KIND>(src, j, n, t, K, tri, shift);
        const unsigned long long mask = __ballot(alive);
        if (lane == 0u) s_count[par][wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t p = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        for (uint32_t k = 0; k < wave; ++k) p += s_count[par][k];
        if (KIND == 0 || KIND == 3) {
            if (j < n) { aux[j] = j - p; if (j + 1u == n) aux[n] = n - p - (alive ? 1u : 0u); }
            if (alive && p < outCount) {
                const float4* r = (const float4*)src + (size_t)j * 3; float4* w = (float4*)out + (size_t)p * 3;
                float4 c2 = r[2]; if (KIND == 0) c2.y = __int_as_float((int)(tri - shift));
                w[0] = r[0]; w[1] = r[1]; w[2] = c2;
            }
        } else if (KIND == 1) {
            if (alive && p < outCount) ((uint32_t*)out)[p] = tri - shift;
        } else if (j < n) aux[j] = p;
        base += (s_count[par][0] + s_count[par][1]) + (s_count[par][2] + s_count[par][3]);
    }
}

// what a child reference of the old tree becomes: a device-form reference / leaf code of the pruned tree (old node numbering), or DEAD
RT_DEV int32_t prune_resolve(int32_t child, const uint32_t* deadBefore, const int32_t* repl) {
    if (child >= 0) return repl[child >> 6];
    const uint32_t code = (uint32_t)~child, first = code >> 2, m = (code & 3u) + 1u;
    const uint32_t d0 = deadBefore[first], dead = deadBefore[first + m] - d0;
    return dead == m ? kPruneDead : ~(int32_t)(((first - d0) << 2) | (m - dead - 1u));
}

// The nodes of one level.  repl[node] = the node itself (device form), its only survivor, or DEAD; alive[node]; a living node's child list
// and meta byte are rewritten in place (the slots are compacted with selects: no register array is indexed dynamically).
__global__ __launch_bounds__(128) void k_prune_level(float4* nodes, const uint32_t* levelNodes, uint32_t count, const uint32_t* deadBefore, int32_t* repl, uint32_t* alive) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint32_t node = levelNodes[k];
    float4* n = nodes + (size_t)node * 4;
    const float4 q0 = n[0], q1 = n[1];
    const uint32_t ex = (uint32_t)__float_as_int(q0.w), cnt = (ex >> 24) & 7u;
    const int32_t child[4] = {__float_as_int(q1.x), __float_as_int(q1.y), __float_as_int(q1.z), __float_as_int(q1.w)};
    int32_t o0 = kPruneDead, o1 = kPruneDead, o2 = kPruneDead, o3 = kPruneDead;
    uint32_t kept = 0, lev = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        if (i >= cnt) continue;
        const int32_t r = prune_resolve(child[i], deadBefore, repl);
        if (r == kPruneDead) continue;
        if (r >= 0) { const uint32_t cl = ((uint32_t)__float_as_int(nodes[(size_t)(r >> 6) * 4].w) >> 27) & 31u; lev = cl > lev ? cl : lev; }
        o0 = kept == 0u ? r : o0; o1 = kept == 1u ? r : o1; o2 = kept == 2u ? r : o2; o3 = kept == 3u ? r : o3;
        ++kept;
    }
    if (kept < 2u) { repl[node] = kept == 1u ? o0 : kPruneDead; alive[node] = 0u; return; }
    repl[node] = (int32_t)(node << 6); alive[node] = 1u;
    n[0] = make_float4(q0.x, q0.y, q0.z, __int_as_float((int)((ex & 0x00FFFFFFu) | ((kept | ((lev + 1u) << 3)) << 24))));
    n[1] = make_float4(__int_as_float(o0), __int_as_float(o1), __int_as_float(o2), __int_as_float(o3));
}

// one thread per quad of a node: alive nodes (and the two quads of their boxes) move to newIndex[node], inner references follow
__global__ __launch_bounds__(kBlock) void k_prune_move(const float4* src, float4* dst, const float4* srcBox, float4* dstBox, const uint32_t* alive, const uint32_t* newIndex, uint32_t nNodes) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x, node = t >> 2, q = t & 3u;
    if (node >= nNodes || alive[node] == 0u) return;
    const uint32_t to = newIndex[node];
    float4 v = src[t];
    if (q == 1u) {
        int32_t c;
        c = __float_as_int(v.x); if (c >= 0) v.x = __int_as_float((int)(newIndex[c >> 6] << 6));
        c = __float_as_int(v.y); if (c >= 0) v.y = __int_as_float((int)(newIndex[c >> 6] << 6));
        c = __float_as_int(v.z); if (c >= 0) v.z = __int_as_float((int)(newIndex[c >> 6] << 6));
        c = __float_as_int(v.w); if (c >= 0) v.w = __int_as_float((int)(newIndex[c >> 6] << 6));
    }
    dst[(size_t)to * 4 + q] = v;
    if (q < 2u) dstBox[(size_t)to * 2 + q] = srcBox[(size_t)node * 2 + q];
}

}  // namespace rt

// ---- host side

// Sorted, merged intervals (first, count) as the kernels' table, and the host's own lookup in it
struct PruneTable {
    std::vector<uint2> tab; uint32_t K = 0, removed = 0;
    void build(std::vector<std::pair<uint32_t, uint32_t>> ranges) {
        std::sort(ranges.begin(), ranges.end());
        tab.clear(); removed = 0;
        for (const auto& r : ranges) {
            if (r.second == 0) continue;
            if (!tab.empty() && tab.back().x + (removed - tab.back().y) == r.first) { removed += r.second; continue; }   // touches the one before: one interval
            tab.push_back(make_uint2(r.first, removed)); removed += r.second;
        }
        K = (uint32_t)tab.size();
        tab.push_back(make_uint2(0xFFFFFFFFu, removed));
    }
    uint32_t before(uint32_t r) const {                 // removed records with an index below r
        uint32_t lo = 0, hi = K;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (tab[mid].x <= r) lo = mid + 1u; else hi = mid; }
        if (lo == 0) return 0;
        return tab[lo - 1].y + std::min(r - tab[lo - 1].x, tab[lo].y - tab[lo - 1].y);
    }
    bool dead(uint32_t r, uint32_t& shift) const { return rt::prune_lookup(tab.data(), K, r, shift); }
};

// The node pass on the host's topology copy, from the leaf records' dead counts (deadBefore, nLeaf + 1 entries).  Leaves hb.nodes (children in
// host form, meta; every other byte of a survivor as it was), hb.rootRef and hb.levels of the pruned tree; `refit` = the new indices of the
// surviving nodes that lost a triangle below them, lowest level first; `refitLevel` = where each level's nodes begin in it.
static void prune_host_tree(rth::SceneBVH& hb, const std::vector<uint32_t>& deadBefore, std::vector<uint32_t>& refit, std::vector<uint32_t>& refitLevel) {
    const size_t nN = hb.nodes.size();
    const std::vector<uint32_t> order = group_by_level(hb.nodes.data(), nN, rth::kStackBudget, kEveryNode).order;
    std::vector<int32_t> repl(nN, rt::kPruneDead); std::vector<uint8_t> alive(nN, 0), lost(nN, 0);
    bool rootLost = false;
    auto resolve = [&](int32_t child, bool& lostAny) -> int32_t {
        if (child >= 0) { lostAny = lostAny || lost[(size_t)child]; return repl[(size_t)child]; }
        const uint32_t code = (uint32_t)~child, f = code >> 2, m = (code & 3u) + 1u, d0 = deadBefore[f], dead = deadBefore[f + m] - d0;
        lostAny = lostAny || dead != 0;
        return dead == m ? rt::kPruneDead : ~(int32_t)(((f - d0) << 2) | (m - dead - 1u));
    };
    for (uint32_t i : order) {
        rth::Node& n = hb.nodes[i];
        int32_t out[4] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
        uint32_t kept = 0, lev = 0; bool lostAny = false;
        for (uint32_t s = 0; s < (n.meta & 7u); ++s) {
            const int32_t r = resolve(n.child[s], lostAny);
            if (r == rt::kPruneDead) continue;
            if (r >= 0) lev = std::max(lev, (uint32_t)(hb.nodes[(size_t)r].meta >> 3));
            out[kept++] = r;
        }
        lost[i] = lostAny;
        if (kept < 2) { repl[i] = kept == 1 ? out[0] : rt::kPruneDead; continue; }
        repl[i] = (int32_t)i; alive[i] = 1;
        for (int s = 0; s < 4; ++s) n.child[s] = out[s];
        n.meta = (uint8_t)(kept | ((lev + 1u) << 3));
    }
    const int32_t root = deadBefore.size() <= 1 ? rt::kPruneDead : resolve(hb.rootRef, rootLost);
    std::vector<uint32_t> newIndex(nN, 0); uint32_t nAlive = 0;
    for (size_t i = 0; i < nN; ++i) { newIndex[i] = nAlive; nAlive += alive[i]; }
    LevelGroups g = group_by_level(hb.nodes.data(), nN, rth::kStackBudget, [&](uint32_t i) { return alive[i] && lost[i]; });
    refitLevel.swap(g.offsets); refit.swap(g.order);
    for (uint32_t& i : refit) i = newIndex[i];
    for (size_t i = 0; i < nN; ++i) {
        if (!alive[i]) continue;
        rth::Node n = hb.nodes[i];
        for (int s = 0; s < 4; ++s) if (n.child[s] >= 0) n.child[s] = (int32_t)newIndex[(size_t)n.child[s]];
        hb.nodes[newIndex[i]] = n;                                   // newIndex[i] <= i: nothing still to be read is overwritten
    }
    hb.nodes.resize(nAlive);
    if (root == rt::kPruneDead) { hb.rootRef = 0; hb.levels = 0; }   // the tree of a scene without triangles
    else if (root < 0) { hb.rootRef = root; hb.levels = 0; }         // the whole scene is one leaf
    else { hb.rootRef = (int32_t)newIndex[(size_t)root]; hb.levels = hb.nodes[(size_t)hb.rootRef].meta >> 3; }
}

// one ordered compaction on the device (count, scan, scatter); `total` = the survivors, one 4-byte read
template <int KIND> static int prune_compact(fyprt_context* c, const void* src, uint32_t n, const uint2* tab, uint32_t K, void* out, uint32_t outCount, uint32_t* aux, DevBuf<uint32_t>& counts, uint32_t* total) {
    *total = 0;
    if (n == 0) return FYPRT_OK;
    const uint32_t groups = std::min<uint32_t>(kEmMaxGroups, (n + kEmMinChunk - 1u) / kEmMinChunk);
    const uint32_t perGroup = (((n + groups - 1u) / groups + kBlock - 1u) / kBlock) * kBlock;
    uint32_t* offsets = counts.p + kEmMaxGroups;
    hipLaunchKernelGGL(k_prune_count<KIND>, dim3(groups), dim3(kBlock), 0, c->stream, src, n, perGroup, tab, K, counts.p);
    hipLaunchKernelGGL(k_emissive_scan, dim3(1), dim3(kBlock), 0, c->stream, (const uint32_t*)counts.p, groups, offsets);
    hipLaunchKernelGGL(k_prune_scatter<KIND>, dim3(groups), dim3(kBlock), 0, c->stream, src, n, perGroup, tab, K, (const uint32_t*)offsets, out, outCount, aux);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(total, offsets + groups, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FYPRT_OK;
}

// one record stream compacted out of place into a buffer of the same capacity, which then replaces the old one
template <int QUADS, bool REMAP, class T> static int prune_stream(fyprt_context* c, DevBuf<T>& b, size_t oldRecords, size_t newRecords, const uint2* tab, uint32_t K, const uint2* vtab, uint32_t VK) {
    const size_t per = (size_t)QUADS * 16u / sizeof(T);
    if (c->hostOnly || b.cap == 0) { b.n = newRecords * per; if (c->hostOnly) b.cap = b.n; return FYPRT_OK; }
    DevBuf<T> nb;
    HIPCHK(c, nb.alloc(b.cap));
    const unsigned long long nQuads = (unsigned long long)oldRecords * QUADS;
    if (nQuads) hipLaunchKernelGGL((k_prune_stream<QUADS, REMAP>), dim3((uint32_t)((nQuads + kBlock - 1u) / kBlock)), dim3(kBlock), 0, c->stream, (const float4*)b.p, (float4*)nb.p, nQuads, tab, K, vtab, VK);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    nb.n = newRecords * per;
    b = std::move(nb);
    return FYPRT_OK;
}

// The tree's part of a removal, shared with fyprt_regraft_meshes (`who`: the caller's name for error texts): the leaf records whose triangle
// lies in `tris` leave the tree, the nodes follow by the prune rule.  `renumber`: the triangles leave the scene as well, so the surviving
// records' triangle indices are remapped (a removal); otherwise survivors keep every byte (a regraft).  `dTab`: the table on the device,
// `counts`: the compactions' counts + offsets.  Leaves the compacted leaf records and node array (old boxes and planes) on the device and
// in the host's copy, and in `refit` / `refitLevel` what prune_refit is to run on once the per-triangle streams are in place.
static int prune_tree(fyprt_context* c, const char* who, const PruneTable& tris, bool renumber, const uint2* dTab, DevBuf<uint32_t>& counts,
                      std::vector<uint32_t>& refit, std::vector<uint32_t>& refitLevel) {
    rth::SceneBVH& hb = c->hostBvh;
    const uint32_t nLeaf = (uint32_t)hb.tris.size(), nNodes = (uint32_t)hb.nodes.size(), T = nLeaf - tris.removed;
    const bool dev = !c->hostOnly;
    c->linksValid = false;                     // nodes and records are renumbered: the partial refit's maps are rebuilt
    DevBuf<uint32_t> deadBeforeDev, alive, newIndex; DevBuf<int32_t> repl;      // the node pass's arrays, freed on every way out
    TRY(ensure_node_boxes(c));                 // (the old grouping describes the tree: what k_refit_level reads of untouched children)
    // 1. leaf records: compacted, their triangle indices remapped; the dead counts go to the node pass here and on the host
    std::vector<uint32_t> deadBefore((size_t)nLeaf + 1u, 0u);
    if (dev) {
        DevBuf<float4> nl;
        HIPCHK(c, nl.alloc(c->leafTris.cap)); HIPCHK(c, deadBeforeDev.alloc((size_t)nLeaf + 1u));
        uint32_t kept = 0;
        if (renumber) TRY(prune_compact<0>(c, c->leafTris.p, nLeaf, dTab, tris.K, nl.p, (uint32_t)(nl.cap / 3), deadBeforeDev.p, counts, &kept));
        else TRY(prune_compact<3>(c, c->leafTris.p, nLeaf, dTab, tris.K, nl.p, (uint32_t)(nl.cap / 3), deadBeforeDev.p, counts, &kept));
        if (nLeaf) HIPCHK(c, hipMemcpy(deadBefore.data(), deadBeforeDev.p, ((size_t)nLeaf + 1u) * 4, hipMemcpyDeviceToHost));
        if (kept != T || deadBefore[nLeaf] != tris.removed) return c->fail(FYPRT_EHIP, std::string(who) + ": the device's leaf records disagree with the host's triangle ranges");
        // 2. the node pass on the old array, level by level, then the alive scan and the move
        if (nNodes) {
            HIPCHK(c, repl.alloc(nNodes)); HIPCHK(c, alive.alloc(nNodes)); HIPCHK(c, newIndex.alloc(nNodes));
            for_each_level(c->levelOffset, [&](uint32_t first, uint32_t count, dim3 grid) {
                hipLaunchKernelGGL(k_prune_level, grid, dim3(kLevelBlock), 0, c->stream, c->nodes.p, (const uint32_t*)(c->levelNodes.p + first), count, (const uint32_t*)deadBeforeDev.p, repl.p, alive.p);
            });
            HIPCHK(c, hipGetLastError());
        }
        nl.n = (size_t)T * 3;
        c->leafTris = std::move(nl);
    } else {
        uint32_t w = 0;
        for (uint32_t j = 0; j < nLeaf; ++j) {
            uint32_t shift; deadBefore[j] = j - w;
            if (tris.dead(hb.tris[j].tri, shift)) continue;
            rth::Tri t = hb.tris[j]; if (renumber) t.tri -= shift; hb.tris[w++] = t;
        }
        deadBefore[nLeaf] = nLeaf - w;
        c->leafTris.n = c->leafTris.cap = (size_t)w * 3;
    }
    prune_host_tree(hb, deadBefore, refit, refitLevel);
    hb.tris.resize(T);
    const uint32_t nNew = (uint32_t)hb.nodes.size();
    if (dev && nNodes) {
        DevBuf<float4> nn, nbx;
        HIPCHK(c, nn.alloc(c->nodes.cap)); HIPCHK(c, nbx.alloc(c->nodeBox.cap));
        uint32_t keptNodes = 0;
        TRY(prune_compact<2>(c, alive.p, nNodes, nullptr, 0u, nullptr, 0u, newIndex.p, counts, &keptNodes));
        if (keptNodes != nNew) return c->fail(FYPRT_EHIP, std::string(who) + ": the device's node pass disagrees with the host's");
        hipLaunchKernelGGL(k_prune_move, dim3((nNodes * 4u + kBlock - 1u) / kBlock), dim3(kBlock), 0, c->stream, (const float4*)c->nodes.p, nn.p, (const float4*)c->nodeBox.p, nbx.p, (const uint32_t*)alive.p, (const uint32_t*)newIndex.p, nNodes);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nn.n = (size_t)nNew * 4; nbx.n = (size_t)nNew * 2;
        c->nodes = std::move(nn); c->nodeBox = std::move(nbx);
    } else if (!dev) { c->nodes.n = c->nodes.cap = (size_t)nNew * 4; c->nodeBox.n = c->nodeBox.cap = (size_t)nNew * 2; }
    return FYPRT_OK;
}

// ... and its last step, once the surviving records' triangles are where the records say: boxes and quantisation of the surviving nodes
// that lost a triangle below them, lowest level first, then the level grouping of the pruned tree.  Complete on return.
static int prune_refit(fyprt_context* c, const std::vector<uint32_t>& refit, const std::vector<uint32_t>& refitLevel) {
    if (!c->hostOnly) {
        DevBuf<uint32_t> refitList;
        if (!refit.empty()) {
            TRY(alloc_upload(c, refitList, refit.data(), refit.size()));
            for_each_level(refitLevel, [&](uint32_t first, uint32_t count, dim3 grid) {
                hipLaunchKernelGGL(k_refit_level, grid, dim3(kLevelBlock), 0, c->stream, c->nodes.p, (const uint32_t*)(refitList.p + first), count, (const float4*)c->leafTris.p, (const float4*)c->triPos.p, c->nodeBox.p);
            });
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(c->stream));                  // the list is scratch of this step
        }
        c->nodeBoxValid = true; c->hostBvhStale = true;               // planes and leaf records live on the device: an export reads them back
    } else for (uint32_t i : refit) host_requantise(c, i);
    return upload_level_grouping(c, true);
}

// The removal proper, after every check: `tris` / `verts` the removed triangle and vertex intervals, `gone[m]` the listed meshes.
static int prune_remove(fyprt_context* c, const PruneTable& tris, const PruneTable& verts, const std::vector<uint8_t>& gone) {
    const uint32_t T0 = (uint32_t)(c->topoTris.size() / 4), V0 = c->vertexCount, M0 = (uint32_t)c->topoMeshes.size();
    const uint32_t T = T0 - tris.removed, V = V0 - verts.removed;
    const bool dev = !c->hostOnly;
    // device scratch of the call, freed on every way out: the two tables, the compactions' counts + offsets
    DevBuf<uint2> dTab, dVtab; DevBuf<uint32_t> counts;
    if (dev) {
        TRY(alloc_upload(c, dTab, tris.tab.data(), tris.tab.size())); TRY(alloc_upload(c, dVtab, verts.tab.data(), verts.tab.size()));
        HIPCHK(c, counts.alloc(2u * kEmMaxGroups + 1u));
    }
    // 1. leaf records and 2. the node pass
    std::vector<uint32_t> refit, refitLevel;
    TRY(prune_tree(c, "fyprt_remove_meshes", tris, true, dTab.p, counts, refit, refitLevel));
    // 3. the per-triangle and per-vertex streams
    TRY((prune_stream<1, true>(c, c->triIdx, T0, T, dTab.p, tris.K, dVtab.p, verts.K)));
    TRY((prune_stream<3, false>(c, c->triPos, T0, T, dTab.p, tris.K, nullptr, 0u)));
    TRY((prune_stream<4, false>(c, c->triShade, T0, T, dTab.p, tris.K, nullptr, 0u)));
    if (verts.removed) {
        TRY((prune_stream<2, false>(c, c->dverts, V0, V, dVtab.p, verts.K, nullptr, 0u)));
        if (!c->meshFirstVertex.empty()) TRY((prune_stream<2, false>(c, c->objVerts, V0, V, dVtab.p, verts.K, nullptr, 0u)));
    }
    // 4. the host's copies of the description
    {
        uint32_t w = 0, shift;
        for (uint32_t t = 0; t < T0; ++t) {
            if (tris.dead(t, shift)) continue;
            uint32_t* d = &c->topoTris[(size_t)w++ * 4]; const uint32_t* s = &c->topoTris[(size_t)t * 4];
            for (int k = 0; k < 3; ++k) { uint32_t vs; (void)verts.dead(s[k], vs); d[k] = s[k] - vs; }
            d[3] = s[3];
        }
        c->topoTris.resize((size_t)T * 4);
        if (verts.removed) {
            w = 0;
            for (uint32_t v = 0; v < V0; ++v) if (!verts.dead(v, shift)) c->hostVerts[w++] = c->hostVerts[v];
            c->hostVerts.resize(V);
        }
        const bool copy = !c->meshFirstVertex.empty();
        std::vector<uint32_t> mfv;
        w = 0;
        for (uint32_t m = 0; m < M0; ++m) {
            if (gone[m]) continue;
            fyprt_mesh me = c->topoMeshes[m];
            me.first_triangle -= tris.before(me.first_triangle);
            if (copy) mfv.push_back(c->meshFirstVertex[m] - verts.before(c->meshFirstVertex[m]));
            if (!c->meshMasks.empty()) c->meshMasks[w] = c->meshMasks[m];      // the query filter's table follows the meshes, in order
            c->topoMeshes[w++] = me;
        }
        c->topoMeshes.resize(w);
        if (!c->meshMasks.empty()) { c->meshMasks.resize(w); c->filterValid = false; if (!w) c->release_query_filter(); }
        if (copy) { mfv.push_back(V); c->meshFirstVertex.swap(mfv); }
        c->vertexCount = V; c->meshCount = w;
    }
    // 5. boxes and quantisation of the surviving nodes that lost a triangle below them, lowest level first
    TRY(prune_refit(c, refit, refitLevel));
    set_scene_triangles(c, T);
    DevScene& d = c->dsc;
    // 6. lights.  The emissive list: the old one, explicit or derived, without the removed triangles, remapped, in order
    const uint32_t nE0 = dev ? d.emissiveCount : (uint32_t)c->hostEmissive.size();
    uint32_t nE = 0;
    const bool hostList = c->hostEmissive.size() == nE0;              // (a device context keeps the copy of a list it was handed only)
    if (hostList) {
        uint32_t w = 0, shift;
        for (uint32_t e : c->hostEmissive) if (!tris.dead(e, shift)) c->hostEmissive[w++] = e - shift;
        c->hostEmissive.resize(w); nE = w;
    }
    if (dev && nE0) {
        DevBuf<uint32_t> ne;
        HIPCHK(c, ne.alloc(c->emissive.cap));
        uint32_t kept = 0;
        TRY(prune_compact<1>(c, c->emissive.p, nE0, dTab.p, tris.K, ne.p, (uint32_t)ne.cap, nullptr, counts, &kept));
        if (hostList && kept != nE) return c->fail(FYPRT_EHIP, "fyprt_remove_meshes: the device's emissive list disagrees with the host's");
        nE = kept; ne.n = nE;
        c->emissive = std::move(ne);
    } else if (!dev) c->emissive.n = c->emissive.cap = nE;
    c->lightRecs.n = (size_t)nE * 3; if (!dev) c->lightRecs.cap = c->lightRecs.n;
    d.emissive = c->emissive.p; d.emissiveCount = nE; d.lightRecs = c->lightRecs.p;
    TRY(launch_light_records(c));
    // ... and the light trees of the meshes that stayed + the TLAS, on the host, with the emitter -> TLAS-leaf table of the shorter list
    TRY(rebuild_light_trees(c, c->hostVerts.data(), nullptr, true));   // (the tables keep their capacity)
    if (dev) HIPCHK(c, sync_all(c));
    return FYPRT_OK;
}
