// Box-overlap queries (fyprt_overlap_boxes / fyprt_overlap_boxes_device): the triangles that touch each of the caller's axis-aligned
// boxes, outside any frame — the first query that is a pure set: no distance, no order among children, nothing that ends it early.
//
//   box record : two float4 (32 B, 16-byte aligned) = lo | pad, hi | pad
//   answer     : maxHits uint32 per box, the lowest accepted triangle indices ascending, unused = 0xFFFFFFFF; a count; a total
// A leaf record (v0, e1, e2) is accepted by box_tri below: the separating-axis test of include/fyprt.h (three box axes on the
// untranslated vertices, nine edge axes and the plane on the vertices relative to the box centre), every operation rounded on its own,
// every comparison written positively so that a NaN rejects.  With `after` the index must also be greater than after[i].  The answer
// is the maxHits smallest accepted indices: a function of the leaf records alone.
//
// The traversal (box_node_step, on point_node_step's node fetch, rt_points.h; node_step is not touched) has no order network: every
// surviving child is visited, in slot order.  A child is skipped iff on some axis planeLo - s > hi or planeHi + s < lo with
// s = k * max(|planeLo|, |planeHi|), k = 2^-20 (kPointSlack).  The slack is needed because the decoded planes bound the TRUE vertices
// while box_tri's first step tests the ROUNDED v0 + e1, which lies up to 3 * 2^-24 * max(|V0|, |V1|) outside them (DESIGN.md §4,
// "Box-overlap queries"); it changes only cost, never an answer.  A child box wholly inside the query box is still descended and its
// records tested one by one: the contract is the rounded rule on every record.
//
// Two forms by tuning key 15, as the other queries: persistent waves (query_body of rt_query.h with BoxLaneT, keys 4, 5, 6, 9, 10) and
// one thread per box (query_simple_body), behind rt_query.h's kernel templates.  The per-lane list is one LDS plane of uint32 behind
// the stack, lane-strided like it, kept sorted ascending; its length and its worst entry live in registers.
#pragma once
#include "rt_points.h"

namespace rt {

struct QueryBoxes {
    const float4* boxes; const uint32_t* after; uint32_t* triangles; uint32_t* counts; uint32_t* totals; uint32_t count, maxHits; uint32_t* head;
    uint32_t chunk, refillLanes, staticChunks, minChunk;
};
constexpr uint32_t kNoTriangle = 0xFFFFFFFFu;          // the unused slot, the `after` word of a finished box, the worst entry of a list that is not full

RT_DEV float sel_min(float a, float b) { return a < b ? a : b; }       // selects, not minnum / maxnum: include/fyprt.h's rule
RT_DEV float sel_max(float a, float b) { return a > b ? a : b; }
RT_DEV float min_of3(float a, float b, float c) { return sel_min(sel_min(a, b), c); }
RT_DEV float max_of3(float a, float b, float c) { return sel_max(sel_max(a, b), c); }

// !(lo <= hi) on some axis, or a sum lo + hi or a difference hi - lo that is not finite (x - x is 0 for a finite x only)
RT_DEV bool box_invalid(f3 lo, f3 hi) {
    const f3 s = lo + hi, d = hi - lo;
    const float z = (((s.x - s.x) + (s.y - s.y)) + (s.z - s.z)) + (((d.x - d.x) + (d.y - d.y)) + (d.z - d.z));
    return !(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z) || !(z == 0.0f);
}

// The three axes f x (1,0,0), f x (0,1,0), f x (0,0,1) of one edge direction f against the vertices p0..p2 relative to the box centre
RT_DEV bool box_edge_axes(f3 p0, f3 p1, f3 p2, f3 f, f3 h) {
    const float ax = __builtin_fabsf(f.x), ay = __builtin_fabsf(f.y), az = __builtin_fabsf(f.z);
    float s0 = p0.z * f.y - p0.y * f.z, s1 = p1.z * f.y - p1.y * f.z, s2 = p2.z * f.y - p2.y * f.z;
    float r = h.y * az + h.z * ay;
    if (!(min_of3(s0, s1, s2) <= r && max_of3(s0, s1, s2) >= -r)) return false;
    s0 = p0.x * f.z - p0.z * f.x; s1 = p1.x * f.z - p1.z * f.x; s2 = p2.x * f.z - p2.z * f.x;
    r = h.x * az + h.z * ax;
    if (!(min_of3(s0, s1, s2) <= r && max_of3(s0, s1, s2) >= -r)) return false;
    s0 = p0.y * f.x - p0.x * f.y; s1 = p1.y * f.x - p1.x * f.y; s2 = p2.y * f.x - p2.x * f.y;
    r = h.x * ay + h.y * ax;
    return min_of3(s0, s1, s2) <= r && max_of3(s0, s1, s2) >= -r;
}

// Whether the leaf record's triangle touches [lo, hi] (c, h: the box's centre and half extent), include/fyprt.h's rule
RT_DEV bool box_tri(const float4* tp, f3 lo, f3 hi, f3 c, f3 h, uint32_t& id) {
    const float4 a = tp[0], b = tp[1], cc = tp[2];
    id = (uint32_t)__float_as_int(cc.y);
    const f3 v0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y), e2 = mk3(b.z, b.w, cc.x);
    const f3 v1 = v0 + e1, v2 = v0 + e2;
    if (!(min_of3(v0.x, v1.x, v2.x) <= hi.x && max_of3(v0.x, v1.x, v2.x) >= lo.x)) return false;
    if (!(min_of3(v0.y, v1.y, v2.y) <= hi.y && max_of3(v0.y, v1.y, v2.y) >= lo.y)) return false;
    if (!(min_of3(v0.z, v1.z, v2.z) <= hi.z && max_of3(v0.z, v1.z, v2.z) >= lo.z)) return false;
    const f3 p0 = v0 - c, p1 = v1 - c, p2 = v2 - c;
    if (!box_edge_axes(p0, p1, p2, e1, h)) return false;
    if (!box_edge_axes(p0, p1, p2, e2 - e1, h)) return false;
    if (!box_edge_axes(p0, p1, p2, e2, h)) return false;
    const f3 n = cross(e1, e2);
    const float d = dot(n, p0);
    const float r = (h.x * __builtin_fabsf(n.x) + h.y * __builtin_fabsf(n.y)) + h.z * __builtin_fabsf(n.z);
    return d <= r && d >= -r;
}

// One axis of the child cull: the decoded planes [pl, ph], widened by k * max(|pl|, |ph|), against the box's [lo, hi]
RT_DEV bool box_axis_apart(float pl, float ph, float lo, float hi) {
    const float s = kPointSlack * __builtin_fmaxf(__builtin_fabsf(pl), __builtin_fabsf(ph));
    return (pl - s > hi) || (ph + s < lo);
}
// Whether child i of a node is skipped; the planes are decoded as point_child_key decodes them (q * step exact, then one add)
RT_DEV bool box_child_apart(uint32_t i, f3 lo, f3 hi, const NodeBoxes& nd) {
    return box_axis_apart(ubyte_f(nd.lx, i) * nd.step.x + nd.org.x, ubyte_f(nd.hx, i) * nd.step.x + nd.org.x, lo.x, hi.x) ||
           box_axis_apart(ubyte_f(nd.ly, i) * nd.step.y + nd.org.y, ubyte_f(nd.hy, i) * nd.step.y + nd.org.y, lo.y, hi.y) ||
           box_axis_apart(ubyte_f(nd.lz, i) * nd.step.z + nd.org.z, ubyte_f(nd.hz, i) * nd.step.z + nd.org.z, lo.z, hi.z);
}

// One visit of a 4-wide node for a box: point_node_step's fetch (fetch_node_boxes), stack rule and resume entries around the overlap
// test, without the order network — the surviving child in the lowest slot is visited next, the others are pushed.
// A resume entry carries the slots still owed; the slot descended into is taken out of it before it is pushed, and a resumed visit looks
// at the owed slots only.  So every child of a node is entered at most once however often the node is fetched, every leaf is reached
// once, and a record is tested once: the lane's total needs no memory of what it has counted.
template <bool COUNT>
RT_DEV int32_t box_node_step(const float4* nodes, int32_t budget, int32_t cur, f3 lo, f3 hi, Stack& st, uint32_t& nBox, uint32_t& nNode) {
    const NodeBoxes nd = fetch_node_boxes<COUNT>(nodes, cur, nBox, nNode);
    const uint32_t off = nd.off, allow = nd.allow, levels = nd.levels;
    const uint32_t hit = allow & ((box_child_apart(0, lo, hi, nd) ? 0u : 1u) | (box_child_apart(1, lo, hi, nd) ? 0u : 2u) |
                                  (box_child_apart(2, lo, hi, nd) ? 0u : 4u) | (box_child_apart(3, lo, hi, nd) ? 0u : 8u));
    const int32_t c0 = nd.c0, c1 = nd.c1, c2 = nd.c2, c3 = nd.c3;
    const uint32_t first = hit & (0u - hit), rest = hit & ~first;     // the lowest surviving slot; slot 0 is never in `rest`
    const int32_t next = (first & 1u) ? c0 : (first & 2u) ? c1 : (first & 4u) ? c2 : c3;
    // node_step's stack rule: pushes while pending + 2 + levels <= budget (room for three entries), one resume entry otherwise
#define RT_PUSH3() do { st.lds[st.top * kBlock] = c3; st.top += (rest & 8u) ? 1 : 0; \
                        st.lds[st.top * kBlock] = c2; st.top += (rest & 4u) ? 1 : 0; \
                        st.lds[st.top * kBlock] = c1; st.top += (rest & 2u) ? 1 : 0; } while (0)
    const uint64_t noRoom = __ballot((st.top - 1) + 2 + (int)levels > budget);
    if (noRoom == 0ull) RT_PUSH3();
    else if (((noRoom >> (threadIdx.x & 63u)) & 1ull) == 0ull) RT_PUSH3();
    else if (rest != 0u) st.push(kResumeBase | (int32_t)(off | rest));
#undef RT_PUSH3
    return (hit != 0u) ? next : st.pop();
}

// Inserts `id` (< worst) into the sorted list of n <= maxHits entries; an index the list holds already is dropped (no visit order may
// duplicate a triangle).  Find the place from the tail, then shift from the tail; a full list loses its last entry.
RT_DEV void tri_insert(uint32_t* l, uint32_t maxHits, uint32_t& n, uint32_t& worst, uint32_t id) {
    uint32_t pos = n;
    while (pos > 0u) {
        const uint32_t k = l[(size_t)(pos - 1u) * kBlock];
        if (k == id) return;
        if (k < id) break;
        --pos;
    }
    for (uint32_t j = n < maxHits ? n : maxHits - 1u; j > pos; --j) l[(size_t)j * kBlock] = l[(size_t)(j - 1u) * kBlock];
    l[(size_t)pos * kBlock] = id;
    if (n < maxHits) ++n;
    if (n == maxHits) worst = l[(size_t)(maxHits - 1u) * kBlock];
}

// The box lane state: the box, and the list's length, worst entry, lowest admissible index and the total in registers.  FILTER as
// RayLane's; the total then counts admitted triangles only.
template <bool FILTER> struct BoxLaneT : LaneFilter<FILTER> {
    using Query = typename std::conditional<FILTER, Filtered<QueryBoxes>, QueryBoxes>::type;
    // 5 waves per SIMD (87 VGPRs, no scratch), as the other list queries: held to 6 (80 VGPRs) the kernel spills five registers to 16 B of
    // scratch, and the LDS holds a sixth workgroup per CU only while stack and list together stay within 26 entries (1 KB each)
    static constexpr int kWaves = 5;
    uint32_t* const list;                       // &plane[threadIdx.x]; entry s at [s * kBlock]
    f3 lo = splat3(0.0f), hi = splat3(0.0f);
    uint32_t n = 0, worst = kNoTriangle, low = 0, total = 0;
    RT_DEV BoxLaneT(const DevScene& sc, const Query&, int32_t* s_stack)
        : list(reinterpret_cast<uint32_t*>(s_stack + (size_t)(sc.stackBudget + 1) * kBlock) + threadIdx.x) {}
    RT_DEV int32_t start(const DevScene& sc, const Query& q, uint32_t i) {
        this->load(q);
        const float4 b0 = q.boxes[(size_t)i * 2], b1 = q.boxes[(size_t)i * 2 + 1];
        lo = mk3(b0.x, b0.y, b0.z); hi = mk3(b1.x, b1.y, b1.z);
        n = 0; worst = kNoTriangle; low = 0; total = 0;
        bool wanted = true;
        if (q.after) { const uint32_t a = q.after[i]; wanted = a != kNoTriangle; low = a + 1u; }     // no index lies above all ones: the box is finished
        return (sc.triCount == 0 || !wanted || box_invalid(lo, hi)) ? kExit : sc.rootRef;
    }
    template <bool COUNT> RT_DEV int32_t visit(const DevScene& sc, int32_t cur, Stack& st, uint32_t& nBox, uint32_t& nNode) {
        if (FILTER && !this->node(cur)) return st.pop();
        return box_node_step<COUNT>(sc.nodes, sc.stackBudget, cur, lo, hi, st, nBox, nNode);
    }
    template <bool COUNT> RT_DEV bool leaf(const DevScene& sc, const Query& q, int32_t cur, uint32_t& nTri) {
        const uint32_t code = (uint32_t)~cur, firstTri = code >> 2, cnt = (code & 3u) + 1u;
        const f3 c = (lo + hi) * 0.5f, h = (hi - lo) * 0.5f;          // (six operations per leaf instead of six registers across the walk)
        for (uint32_t k = 0; k < cnt; ++k) {
            uint32_t id;
            if (FILTER && !this->record(firstTri + k)) continue;
            if (COUNT) nTri += 1;
            if (!box_tri(sc.leafTris + (size_t)(firstTri + k) * 3, lo, hi, c, h, id) || id < low) continue;
            total += 1u;                                              // every accepted triangle, also those beyond maxHits
            if (id < worst) tri_insert(list, q.maxHits, n, worst, id);
        }
        return false;                                                 // a set query is never finished early
    }
    RT_DEV bool finish(const DevScene&, const Query& q, uint32_t i) {
        uint32_t* dst = q.triangles + (size_t)i * q.maxHits;
        for (uint32_t s = 0; s < q.maxHits; ++s) dst[s] = s < n ? list[(size_t)s * kBlock] : kNoTriangle;
        if (q.counts) q.counts[i] = n;
        if (q.totals) q.totals[i] = total;
        return n != 0u;
    }
};

}  // namespace rt
