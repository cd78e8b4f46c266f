// Batched ray queries (fyprt_trace_rays / fyprt_trace_rays_device): the caller's rays traced against the uploaded scene, outside any frame.
//
//   ray record : 2 x float4 (32 B, 16-byte aligned) = origin | tmin, direction | tmax
//   CLOSEST    : one 40-byte Payload per ray (make_hit / make_miss, the record a frame's primary kernel writes)
//   OCCLUDED   : one uint32 per ray, 1 iff any triangle is accepted; traversal stops at the first one
// A triangle is accepted at t when tri_test passes (the reference's Möller–Trumbore with its own t > 1e-4), t > tmin and t < tmax.
// The closest-hit query starts from best = min(tmax, FLT_MAX) and culls boxes against best * 1.000001f: with tmin <= 1e-4 and
// tmax = +inf that is trace_closest step for step, so the record equals the primary kernel's bit for bit (exact-t ties go to the first
// triangle found, as there).  The occlusion query culls against tmax * 1.000001f; its answer does not depend on the visiting order.
// A ray with a non-finite origin / direction component, a NaN bound or !(tmin < tmax) is answered as a miss (0) without traversal
// and counted as a ray with no tests.
//
// Two forms, chosen by the host like the path engine's ray kernels (tuning key 15):
//   persistent      waves that stay, one in-flight ray per lane, idle lanes refilled from the wave's claimed chunk (the guided
//                   self-scheduling of trace_rays_body, tuning keys 4, 5, 9, 10); a refill is two 16-byte loads and three
//                   reciprocals, a finished closest-hit ray one triShade gather (make_hit) and a 40-byte store.
//   one thread      per ray, for small trees where rays are too cheap for the refill machinery to pay.
// The query kind is a template parameter: neither form carries the other kind's branches.  They only call the traversal core of
// rt_device.h (node_step, tri_test, make_hit / make_miss, quorum_of, ray_not_finite); no frame kernel is touched.
// The multi-hit query (fyprt_trace_ray_hits*: the K nearest hits per ray in order) further down, the nearest-point query (rt_points.h)
// and the box-overlap query (rt_boxes.h) have the same two forms: all of them are query_body / query_simple_body, written once below,
// around a per-query lane state L, and every query kernel is one of the three entry points k_query<L>, k_query_counted<L> and
// k_query_simple<L, COUNT> behind them.
#pragma once
#include "rt_paths.h"
#include "rt_filter.h"

namespace rt {

struct QueryRays {
    const float4* rays; void* results; uint32_t count; uint32_t* head;
    uint32_t chunk, refillLanes, staticChunks, minChunk;
};

RT_DEV bool query_invalid(f3 o, f3 d, float tmin, float tmax) { return ray_not_finite(o, d) || !(tmin < tmax); }   // (a NaN bound fails the compare)
RT_DEV float query_start(float tmax) { return tmax < 3.402823466e+38f ? tmax : 3.402823466e+38f; }                   // min(tmax, FLT_MAX), tmax not NaN

// 40 bytes as five 8-byte stores: the results array is only required to be 8-byte aligned
RT_DEV void store_payload(Payload* dst, const Payload& p) {
    float2* q = reinterpret_cast<float2*>(dst);
    q[0] = make_float2(p.hitDistance, p.px); q[1] = make_float2(p.py, p.pz); q[2] = make_float2(p.nx, p.ny);
    q[3] = make_float2(p.nz, p.u); q[4] = make_float2(p.v, __int_as_float(p.objectIndex));
}

template <bool OCCLUDED>
RT_DEV void store_query_result(const DevScene& sc, const QueryRays& q, uint32_t i, f3 o, f3 d, float best, float hu, float hv, int32_t hitTri) {
    if (OCCLUDED) { static_cast<uint32_t*>(q.results)[i] = hitTri >= 0 ? 1u : 0u; return; }
    Hit h; h.t = best; h.u = hu; h.v = hv; h.tri = hitTri;
    store_payload(static_cast<Payload*>(q.results) + i, hitTri < 0 ? make_miss() : make_hit(sc, o, d, h));
}

template <bool COUNT>
RT_DEV void count_query_ray(const DevScene& sc, uint32_t nBox, uint32_t nTri, uint32_t nNode, bool hit) {
    if (!COUNT) return;
    atomicAdd(sc.rayCounter + 0, 1ull); atomicAdd(sc.rayCounter + 1, (unsigned long long)nBox);
    atomicAdd(sc.rayCounter + 2, (unsigned long long)nTri); atomicAdd(sc.rayCounter + 3, hit ? 1ull : 0ull);
    atomicAdd(sc.rayCounter + 4, (unsigned long long)nNode);
}

// ---- the scheduling every query family shares.  A lane state L carries the one record a lane has in flight:
//   L::Query, L::kWaves                        the launch's record type; the waves per SIMD the uncounted persistent kernel is held to
//   L(sc, q, s_stack)                          what a thread keeps for the whole launch (the list queries' LDS planes)
//   start(sc, q, i)                            loads record i and initialises; sc.rootRef, or kExit for a record answered without traversal
//   visit<COUNT>(sc, cur, st, nBox, nNode)     one node visit (node_step / point_node_step)
//   leaf<COUNT>(sc, q, cur, nTri)              one leaf's triangles against the state; true when the record is finished by it
//   finish(sc, q, i)                           stores the answer; whether it counts as a hit
// Five of them, each plain and filtered: RayLane<OCCLUDED, FILTER> here, HitsLaneT<FILTER> further down, PointsLaneT in rt_points.h,
// BoxLaneT in rt_boxes.h, TriLaneT in rt_triangles.h.  The compiler replaces a lane state by its scalars (tools/kernel_resources.py shows the registers of the
// hand-written bodies these replaced, profiles/query/).

// Persistent waves: one in-flight record per lane, idle lanes refilled from the wave's claimed chunk.
template <class L, bool COUNT>
RT_DEV void query_body(const DevScene& sc, const typename L::Query& q, int32_t* s_stack) {
    int32_t* lds = s_stack + threadIdx.x;
    L l(sc, q, s_stack);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t total = q.count;
    // work distribution of trace_rays_body: static chunks per wave, then guided claims from the shared head
    const uint32_t nWaves = gridDim.x * (uint32_t)(kBlock / 64), myWave = blockIdx.x * (uint32_t)(kBlock / 64) + (threadIdx.x >> 6);
    const uint32_t share = (total + nWaves - 1u) / nWaves;
    const uint32_t chunk = q.chunk, want1 = chunk * q.staticChunks;
    const uint32_t first = share < want1 ? (share < 16u ? 16u : share) : want1;
    const uint32_t dynBase = nWaves * first;
    const bool hasDyn = dynBase < total;
    uint32_t task = 0; int32_t cur = kExit; int top = 0;
    uint32_t nBox = 0, nTri = 0, nNode = 0;
    bool active = false;
    bool more = total != 0u;
    uint32_t chunkNext = myWave * first < total ? myWave * first : total;
    uint32_t chunkEnd = (myWave + 1u) * first < total ? (myWave + 1u) * first : total;
    while (true) {
        const unsigned long long idle = __ballot(!active);
        if (more && (uint32_t)__popcll(idle) >= q.refillLanes) {
            if (chunkNext >= chunkEnd && hasDyn) {
                uint32_t base = 0;
                uint32_t size = (total - chunkEnd) / nWaves;
                size = size < q.minChunk ? q.minChunk : (size > chunk ? chunk : size);
                if (lane == 0u) base = dynBase + atomicAdd(q.head, size);
                base = (uint32_t)__shfl((int)base, 0);
                chunkNext = base < total ? base : total;
                chunkEnd = (base + size < total) ? base + size : total;
            }
            const uint32_t slot = chunkNext + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            const uint32_t want = (uint32_t)__popcll(idle), avail = chunkEnd - chunkNext;
            chunkNext += (want < avail) ? want : avail;
            more = chunkNext < chunkEnd || (hasDyn && chunkEnd < total);
            if (!active && slot < chunkEnd) {
                task = slot;
                if (COUNT) { nBox = 0; nTri = 0; nNode = 0; }
                top = 0; lane_push(lds, top, kExit);
                cur = l.start(sc, q, task);
                active = true;
            }
        }
        if (__ballot(active) == 0ull) { if (!more) break; else continue; }
        while (true) {
            bool walk = active && cur >= 0;
            const uint32_t quorum = quorum_of(sc.nodeQuorum, (uint32_t)__popcll(__ballot(active)));
            while (walk) {
                { Stack st; st.lds = lds; st.top = top; cur = l.template visit<COUNT>(sc, cur, st, nBox, nNode); top = st.top; }
                walk = cur >= 0;
                if ((uint32_t)__popcll(__ballot(walk)) < quorum) break;
            }
            if (active && cur < 0 && cur != kExit) cur = l.template leaf<COUNT>(sc, q, cur, nTri) ? kExit : lane_pop(lds, top);
            if (active && cur == kExit) {
                count_query_ray<COUNT>(sc, nBox, nTri, nNode, l.finish(sc, q, task));
                active = false;
            }
            const unsigned long long act = __ballot(active);
            if (act == 0ull) break;
            if (more && (64u - (uint32_t)__popcll(act)) >= q.refillLanes) break;
        }
    }
}

// One thread per record, grid-stride: the interval form of trace_closest around the same lane states.
template <class L, bool COUNT>
RT_DEV void query_simple_body(const DevScene& sc, const typename L::Query& q, int32_t* s_stack) {
    L l(sc, q, s_stack);
    for (uint32_t base = blockIdx.x * (uint32_t)kBlock; base < q.count; base += gridDim.x * (uint32_t)kBlock) {   // (block-uniform trips: the node visit's ballots see whole waves)
        const uint32_t i = base + threadIdx.x;
        if (i >= q.count) continue;
        uint32_t nBox = 0, nTri = 0, nNode = 0;
        Stack st; st.lds = s_stack + threadIdx.x; st.top = 0; st.push(kExit);
        int32_t cur = l.start(sc, q, i);
        while (cur != kExit) {
            bool walk = cur >= 0;
            const uint32_t quorum = quorum_of(sc.nodeQuorum, (uint32_t)__popcll(__ballot(true)));
            while (walk) {
                cur = l.template visit<COUNT>(sc, cur, st, nBox, nNode);
                walk = cur >= 0;
                if ((uint32_t)__popcll(__ballot(walk)) < quorum) break;
            }
            if (cur >= 0 || cur == kExit) continue;
            cur = l.template leaf<COUNT>(sc, q, cur, nTri) ? kExit : st.pop();
        }
        count_query_ray<COUNT>(sc, nBox, nTri, nNode, l.finish(sc, q, i));
    }
}

// The kernels of every query family, by lane state.  s_stack: (stackBudget + 1) entries x kBlock threads and behind them the lane state's
// list planes (maxHits x 16 B or 4 B per thread), sized at launch.
template <class L> __global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(L::kWaves))) void k_query(DevScene sc, typename L::Query q) {
    extern __shared__ int32_t s_stack[];
    query_body<L, false>(sc, q, s_stack);
}
template <class L> __global__ __launch_bounds__(kBlock) void k_query_counted(DevScene sc, typename L::Query q) {   // instrumented: no register cap
    extern __shared__ int32_t s_stack[];
    query_body<L, true>(sc, q, s_stack);
}
template <class L, bool COUNT> __global__ __launch_bounds__(kBlock) void k_query_simple(DevScene sc, typename L::Query q) {
    extern __shared__ int32_t s_stack[];
    query_simple_body<L, COUNT>(sc, q, s_stack);
}

// The closest-hit / occlusion lane state.  FILTER: the query filter's visit rule (rt_filter.h) around the same walk; the record is then
// Filtered<QueryRays>.  Without it the base is empty and the lane is the code it was.
template <bool OCCLUDED, bool FILTER = false> struct RayLane : LaneFilter<FILTER> {
    using Query = typename std::conditional<FILTER, Filtered<QueryRays>, QueryRays>::type;
    static constexpr int kWaves = RT_TRACE_WAVES_N;               // the register budget of the frames' persistent trace kernels (rt_wavefront.h)
    // (the origin lives in pk only: a separate copy of it costs three registers across the loop, and the closest-hit kernel spills)
    f3 d = splat3(0.0f); RayPk pk = make_raypk(d, 1.0f, 1.0f, 1.0f);
    float tmin = 0.0f, best = 0.0f, cut = 0.0f, hu = 0.0f, hv = 0.0f; int32_t hitTri = -1;
    RT_DEV RayLane(const DevScene&, const Query&, int32_t*) {}
    // a refill is two 16-byte loads and three reciprocals
    RT_DEV int32_t start(const DevScene& sc, const Query& q, uint32_t i) {
        this->load(q);
        const float4 r0 = q.rays[(size_t)i * 2], r1 = q.rays[(size_t)i * 2 + 1];
        const f3 o = mk3(r0.x, r0.y, r0.z); d = mk3(r1.x, r1.y, r1.z); tmin = r0.w;
        pk = make_raypk(o, safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
        best = OCCLUDED ? r1.w : query_start(r1.w);
        cut = best * 1.000001f;
        hitTri = -1; hu = 0.0f; hv = 0.0f;
        return (sc.triCount == 0 || query_invalid(o, d, tmin, r1.w)) ? kExit : sc.rootRef;
    }
    template <bool COUNT> RT_DEV int32_t visit(const DevScene& sc, int32_t cur, Stack& st, uint32_t& nBox, uint32_t& nNode) {
        if (FILTER && !this->node(cur)) return st.pop();
        return node_step<COUNT>(sc.nodes, sc.stackBudget, cur, pk, cut, st, nBox, nNode);
    }
    template <bool COUNT> RT_DEV bool leaf(const DevScene& sc, const Query&, int32_t cur, uint32_t& nTri) {
        const uint32_t code = (uint32_t)~cur, firstTri = code >> 2, cnt = (code & 3u) + 1u;
        for (uint32_t k = 0; k < cnt; ++k) {
            float t, u, v; uint32_t id;
            if (FILTER && !this->record(firstTri + k)) continue;
            if (COUNT) nTri += 1;
            if (!tri_test(sc.leafTris + (size_t)(firstTri + k) * 3, mk3(pk.ox, pk.oy, pk.oz), d, t, u, v, id) || !(t > tmin) || !(t < best)) continue;
            hitTri = (int32_t)id;
            if (OCCLUDED) return true;
            best = t; cut = t * 1.000001f; hu = u; hv = v;
        }
        return false;
    }
    RT_DEV bool finish(const DevScene& sc, const Query& q, uint32_t i) {
        store_query_result<OCCLUDED>(sc, q, i, mk3(pk.ox, pk.oy, pk.oz), d, best, hu, hv, hitTri);
        return hitTri >= 0;
    }
};

template <bool FILTER> using ClosestLane = RayLane<false, FILTER>;
template <bool FILTER> using OccludedLane = RayLane<true, FILTER>;

// ============================================================ multi-hit queries (fyprt_trace_ray_hits*): the K nearest hits per ray
// Every accepted hit (the closest-hit query's acceptance rule) has the 64-bit key (bits(t) << 32) | triangle: t > 1e-4, so the bit
// pattern orders as the value (the key construction of k_graft_place).  The answer is the `maxHits` smallest keys above the key of
// `after[i]` (0 without `after`), ascending — a function of the triangles alone, not of the tree or the visiting order.
//   hit record : one float4 (16 B) = t | triangle (bits) | u | v, tri_test's values; unused = -1 | 0xFFFFFFFF | 0 | 0
// The per-lane list is kept sorted in LDS behind the traversal stack, lane-strided like it: a plane of 64-bit keys and a plane of
// (u, v) pairs, maxHits entries x kBlock threads each, read and written as 8-byte quantities (a lane's entries are 8 B apart in a
// plane row: conflict-free for ds_read_b64 / ds_write_b64).  Its length and its worst key live in registers — `worst` is all ones
// while the list is not full, so one 64-bit compare rejects a candidate without touching LDS.  Boxes are culled against
// min(tmax, FLT_MAX) * 1.000001f until the list is full, then against t_worst * 1.000001f: a box entered at exactly t_worst is still
// visited, a tie with a lower triangle index displaces the worst entry.
struct QueryHits {
    const float4* rays; const float4* after; float4* hits; uint32_t* counts; uint32_t count, maxHits; uint32_t* head;
    uint32_t chunk, refillLanes, staticChunks, minChunk;
};
struct HitList {
    unsigned long long* keys; float2* uv;       // &plane[threadIdx.x]; entry s at [s * kBlock]
};
constexpr unsigned long long kNoWorstKey = ~0ull;

RT_DEV HitList hit_list(int32_t* s_stack, int32_t budget, uint32_t maxHits) {
    HitList l;
    l.keys = reinterpret_cast<unsigned long long*>(s_stack + (size_t)(budget + 1) * kBlock) + threadIdx.x;      // (the stack is a multiple of 1 KB: 8-byte aligned)
    l.uv = reinterpret_cast<float2*>(l.keys + (size_t)maxHits * kBlock);
    return l;
}
RT_DEV unsigned long long hit_key(float t, uint32_t tri) { return ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)tri; }
// The ray's start: the key every answer must exceed and whether the ray is to be traced at all (an `after` record with t < 0 is the
// unused record of an earlier pass: the ray is finished)
RT_DEV bool hits_start(const QueryHits& q, uint32_t i, unsigned long long& afterKey) {
    afterKey = 0ull;
    if (!q.after) return true;
    const float4 a = q.after[i];
    if (a.x < 0.0f) return false;
    afterKey = hit_key(a.x, __float_as_uint(a.y));
    return true;
}
// Inserts (key, u, v) with afterKey < key < worst into the sorted list of n <= maxHits entries; a key the list holds already is dropped
// (no visit order may duplicate a hit).  Find the place from the tail, then shift from the tail; a full list loses its last entry.
RT_DEV void hit_insert(const HitList& l, uint32_t maxHits, uint32_t& n, unsigned long long& worst, unsigned long long key, float u, float v) {
    uint32_t pos = n;
    while (pos > 0u) {
        const unsigned long long k = l.keys[(size_t)(pos - 1u) * kBlock];
        if (k == key) return;
        if (k < key) break;
        --pos;
    }
    for (uint32_t j = n < maxHits ? n : maxHits - 1u; j > pos; --j) {
        l.keys[(size_t)j * kBlock] = l.keys[(size_t)(j - 1u) * kBlock];
        l.uv[(size_t)j * kBlock] = l.uv[(size_t)(j - 1u) * kBlock];
    }
    l.keys[(size_t)pos * kBlock] = key; l.uv[(size_t)pos * kBlock] = make_float2(u, v);
    if (n < maxHits) ++n;
    if (n == maxHits) worst = l.keys[(size_t)(maxHits - 1u) * kBlock];
}
// One leaf's triangles against the list; returns the box cut that holds afterwards
template <class F>
RT_DEV float hits_leaf(const DevScene& sc, const HitList& l, uint32_t maxHits, int32_t cur, f3 o, f3 d, float tmin, float hi, unsigned long long afterKey,
                       uint32_t& n, unsigned long long& worst, float cut, uint32_t& nTri, bool count, const F& flt) {
    const uint32_t code = (uint32_t)~cur, firstTri = code >> 2, cnt = (code & 3u) + 1u;
    for (uint32_t k = 0; k < cnt; ++k) {
        float t, u, v; uint32_t id;
        if (!flt.record(firstTri + k)) continue;
        if (count) nTri += 1;
        if (!tri_test(sc.leafTris + (size_t)(firstTri + k) * 3, o, d, t, u, v, id) || !(t > tmin) || !(t < hi)) continue;
        const unsigned long long key = hit_key(t, id);
        if (key <= afterKey || key >= worst) continue;
        hit_insert(l, maxHits, n, worst, key, u, v);
        if (n == maxHits) cut = __uint_as_float((uint32_t)(worst >> 32)) * 1.000001f;
    }
    return cut;
}
// The finished ray's maxHits records as 16-byte stores, then its count
RT_DEV void store_hits(const QueryHits& q, const HitList& l, uint32_t i, uint32_t n) {
    float4* dst = q.hits + (size_t)i * q.maxHits;
    for (uint32_t s = 0; s < q.maxHits; ++s) {
        float4 r = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f);
        if (s < n) {
            const unsigned long long k = l.keys[(size_t)s * kBlock]; const float2 uv = l.uv[(size_t)s * kBlock];
            r = make_float4(__uint_as_float((uint32_t)(k >> 32)), __uint_as_float((uint32_t)k), uv.x, uv.y);
        }
        dst[s] = r;
    }
    if (q.counts) q.counts[i] = n;
}

// The multi-hit lane state: the ray, and the list's length, worst key and `after` key in registers.  FILTER as RayLane's.
template <bool FILTER> struct HitsLaneT : LaneFilter<FILTER> {
    using Query = typename std::conditional<FILTER, Filtered<QueryHits>, QueryHits>::type;
    // 5 waves per SIMD (96 VGPRs, 12 B of scratch as the closest-hit kernel), not the 6 of RT_TRACE_WAVES (80 VGPRs, 20 B: the list's
    // length, its worst key and the `after` key are five more live registers): the list's LDS leaves room for no more than 5 workgroups
    // per CU from a 26-entry stack on (26 x 4 + 16 B per thread = 30 KB), so the sixth wave would be bought for small trees only.
    static constexpr int kWaves = 5;
    const HitList list;
    f3 d = splat3(0.0f); RayPk pk = make_raypk(d, 1.0f, 1.0f, 1.0f);
    float tmin = 0.0f, hi = 0.0f, cut = 0.0f; uint32_t n = 0;
    unsigned long long worst = kNoWorstKey, afterKey = 0ull;
    RT_DEV HitsLaneT(const DevScene& sc, const Query& q, int32_t* s_stack) : list(hit_list(s_stack, sc.stackBudget, q.maxHits)) {}
    RT_DEV int32_t start(const DevScene& sc, const Query& q, uint32_t i) {
        this->load(q);
        const float4 r0 = q.rays[(size_t)i * 2], r1 = q.rays[(size_t)i * 2 + 1];
        const f3 o = mk3(r0.x, r0.y, r0.z); d = mk3(r1.x, r1.y, r1.z); tmin = r0.w;
        pk = make_raypk(o, safe_inv(d.x), safe_inv(d.y), safe_inv(d.z));
        hi = query_start(r1.w);
        cut = hi * 1.000001f;
        n = 0; worst = kNoWorstKey;
        const bool wanted = hits_start(q, i, afterKey);
        return (sc.triCount == 0 || !wanted || query_invalid(o, d, tmin, r1.w)) ? kExit : sc.rootRef;
    }
    template <bool COUNT> RT_DEV int32_t visit(const DevScene& sc, int32_t cur, Stack& st, uint32_t& nBox, uint32_t& nNode) {
        if (FILTER && !this->node(cur)) return st.pop();
        return node_step<COUNT>(sc.nodes, sc.stackBudget, cur, pk, cut, st, nBox, nNode);
    }
    template <bool COUNT> RT_DEV bool leaf(const DevScene& sc, const Query& q, int32_t cur, uint32_t& nTri) {
        cut = hits_leaf(sc, list, q.maxHits, cur, mk3(pk.ox, pk.oy, pk.oz), d, tmin, hi, afterKey, n, worst, cut, nTri, COUNT, static_cast<const LaneFilter<FILTER>&>(*this));
        return false;
    }
    RT_DEV bool finish(const DevScene&, const Query& q, uint32_t i) { store_hits(q, list, i, n); return n != 0u; }
};

// ============================================================ radiance queries (fyprt_render_rays*): the primary pass
// The primary segments are traced by the closest-hit kernels above into the query's own payload records (the frame's primary record
// for the same ray and the default interval).  This kernel, one thread per ray, does what the rest of k_primary does: an invalid ray
// gives (0,0,0,0), a miss inside the interval (sky, 1), an emitter hit (emission, 1); every other ray is appended to the live list, where
// the stages (k_shade<TECH, RaySource>, k_nee_mis<RaySource>) take it from the primary hit as they take a frame's pixel.
__global__ __launch_bounds__(kBlock) void k_render_rays_primary(DevScene sc, RaySource rs, DevFrame fr, DevSettings st, uint32_t count,
                                                                uint32_t* list, uint32_t* listCount) {
    for (uint32_t base = blockIdx.x * (uint32_t)kBlock; base < count; base += gridDim.x * (uint32_t)kBlock) {   // (block-uniform trips: block_append)
        const uint32_t k = base + threadIdx.x;
        bool live = false;
        if (k < count) {
            const float4 r0 = rs.rays[(size_t)k * 2], r1 = rs.rays[(size_t)k * 2 + 1];
            if (query_invalid(xyz(r0), xyz(r1), r0.w, r1.w)) rs.radiance[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            else {
                const Payload pp = fr.payload[k];
                if (pp.hitDistance < 0.0f) finish(rs, fr, k, rgb1(st.sky));
                else {
                    const Mat hm = load_mat(sc, tri_material(sc, pp.objectIndex));
                    if (length(emission(hm)) > 0.0f) finish(rs, fr, k, rgb1(emission(hm))); else live = true;
                }
            }
        }
        const uint32_t slot = block_append(live, listCount);
        if (live) list[slot] = k;
    }
}

}  // namespace rt
