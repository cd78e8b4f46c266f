// Nearest-point queries (fyprt_nearest_points / fyprt_nearest_points_device): the K closest triangles to each of the caller's points,
// outside any frame — the first query that is not asked along a ray.
//
//   point record : one float4 (16 B, 16-byte aligned) = position | max_distance
//   hit record   : one float4 (16 B) = distance2 | triangle (bits) | u | v; unused = -1 | 0xFFFFFFFF | 0 | 0 (the multi-hit record)
// The distance of a point to a leaf record (v0, e1, e2) is point_tri below: Ericson's closest point on a triangle in the operation
// order include/fyprt.h states, every operation rounded on its own, the barycentrics clamped at the end.  A triangle is accepted when
// distance2 <= r2 = min(max_distance^2, FLT_MAX) — a NaN or infinite distance2 (a degenerate record) never is — and, with `after`, when
// its key (bits(distance2) << 32) | triangle is greater than the key of after[i].  distance2 >= +0, so the bit pattern orders as the
// value; the answer is the maxHits smallest keys, ascending: a function of the leaf records alone.
//
// The traversal orders and culls by box distance instead of slab parameter (point_node_step, a sibling of node_step: that one is not
// touched, no frame kernel and no ray query compiles differently).  The cull is conservative against point_tri's ROUNDED arithmetic:
// with the decoded planes lo <= every vertex coordinate <= hi, the per-axis gap g = max(lo - p, p - hi, 0) is shrunk to
// g' = max(g - k * max(|p|, |lo|, |hi|), 0), k = 2^-20, which is no larger than |diff| of ANY triangle below the child on that axis
// ("Nearest-point queries": 14 roundings of 2^-24 * max(...) each at most, 16 allowed for); lb2 = (g'x^2 + g'y^2) + g'z^2
// has point_tri's own operation order, rounding is monotonic, so lb2 <= distance2.  A child is skipped iff lb2 * (1 - k) > bound, the
// bound being r2 until the list is full and the worst entry's distance2 from then on: a child at exactly the bound is still visited,
// a tie with a lower triangle index displaces the worst entry.
//
// Two forms by tuning key 15, as the other queries: persistent waves (query_body of rt_query.h with PointsLaneT, keys 4, 5, 6, 9, 10) and
// one thread per point (query_simple_body), behind rt_query.h's kernel templates.  The per-lane list is the multi-hit query's:
// HitList, hit_insert and store_hits, in LDS behind the stack, 16 B per entry; the query record is QueryHits with one float4 per point.
#pragma once
#include "rt_query.h"

namespace rt {

using QueryPoints = QueryHits;                  // .rays = the point records (ONE float4 per point), everything else as the multi-hit query
constexpr float kPointSlack = 9.5367431640625e-07f;        // k = 2^-20
constexpr float kPointKeep = 0.99999904632568359375f;      // 1 - k, exact in binary32

RT_DEV bool point_invalid(f3 p, float maxDistance) {       // non-finite position, NaN or negative max_distance (-0 is 0)
    const float z = ((p.x - p.x) + (p.y - p.y)) + (p.z - p.z);
    return !(z == 0.0f) || !(maxDistance >= 0.0f);
}
RT_DEV float point_r2(float maxDistance) { const float m = maxDistance * maxDistance; return m < 3.402823466e+38f ? m : 3.402823466e+38f; }
// The point's start: the lowest key an answer may have (0 without `after`, key(after[i]) + 1 with it) and whether the point is to be
// traversed at all: an `after` record with distance2 < 0 is the unused record of an earlier pass, and no key lies above all ones.
// (distance2 = 0 on triangle 0 is the key 0, a valid answer: an exclusive bound as the multi-hit query keeps could not admit it)
RT_DEV bool points_start(const QueryPoints& q, uint32_t i, unsigned long long& lowKey) {
    lowKey = 0ull;
    if (!q.after) return true;
    const float4 a = q.after[i];
    if (a.x < 0.0f) return false;
    lowKey = hit_key(a.x, __float_as_uint(a.y)) + 1ull;
    return lowKey != 0ull;
}

// Squared distance of p to the leaf record's triangle and the barycentrics (u, v) of the closest point, include/fyprt.h's rule
RT_DEV void point_tri(const float4* tp, f3 p, float& dist2, float& u, float& v, uint32_t& id) {
    const float4 a = tp[0], b = tp[1], c = tp[2];
    id = (uint32_t)__float_as_int(c.y);
    const f3 v0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y), e2 = mk3(b.z, b.w, c.x);
    const f3 ap = p - v0;
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    u = 0.0f; v = 0.0f;
    if (!(d1 <= 0.0f && d2 <= 0.0f)) {
        const f3 bp = ap - e1;
        const float d3 = dot(e1, bp), d4 = dot(e2, bp);
        if (d3 >= 0.0f && d4 <= d3) u = 1.0f;
        else {
            const float vc = d1 * d4 - d3 * d2;
            if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) u = d1 / (d1 - d3);
            else {
                const f3 cp = ap - e2;
                const float d5 = dot(e1, cp), d6 = dot(e2, cp);
                if (d6 >= 0.0f && d5 <= d6) v = 1.0f;
                else {
                    const float vb = d5 * d2 - d1 * d6;
                    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) v = d2 / (d2 - d6);
                    else {
                        const float va = d3 * d6 - d5 * d4, ea = d4 - d3, eb = d5 - d6;
                        if (va <= 0.0f && ea >= 0.0f && eb >= 0.0f) { const float w = ea / (ea + eb); u = 1.0f - w; v = w; }
                        else { const float s = (va + vb) + vc, f = 1.0f / s; u = vb * f; v = vc * f; }
                    }
                }
            }
        }
    }
    u = u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u);                     // selects: a NaN stays a NaN
    const float m = 1.0f - u;
    v = v < 0.0f ? 0.0f : (v > m ? m : v);
    const f3 diff = mk3((ap.x - u * e1.x) - v * e2.x, (ap.y - u * e1.y) - v * e2.y, (ap.z - u * e1.z) - v * e2.z);
    dist2 = dot(diff, diff);
}

// A node of the 4-wide tree as the point and box walks see it: fetched whole (64 bytes) and decoded, no test made yet.  `allow`: the
// slots to look at — those of a resume entry, or all four, masked by the node's child count: unused slots (planes qlo 255 / qhi 0) are a
// box like any other to a distance or overlap test.  `levels`: the height the stack rule needs; the planes stay packed, one word per
// axis and side, and are decoded per child as the builders verify them (org + q * step).  Counts the visit and its box tests under COUNT.
struct NodeBoxes {
    uint32_t off, allow, levels; f3 org, step;
    uint32_t lx, ly, lz, hx, hy, hz;
    int32_t c0, c1, c2, c3;
};
template <bool COUNT>
RT_DEV NodeBoxes fetch_node_boxes(const float4* nodes, int32_t cur, uint32_t& nBox, uint32_t& nNode) {
    NodeBoxes nd;
    const bool anyResumed = __ballot(cur >= kResumeBase) != 0ull;
    nd.off = (uint32_t)cur & kNodeOffsetMask;
    nd.allow = 0xFu;
    if (anyResumed) nd.allow = (cur >= kResumeBase) ? ((uint32_t)cur & 0xFu) : 0xFu;
    const float4* n = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(nodes) + nd.off);     // uniform base + 32-bit lane offset
    const float4 q0 = n[0], q1 = n[1], q2 = n[2]; const float2 q3 = *reinterpret_cast<const float2*>(n + 3);
    const uint32_t ex = (uint32_t)__float_as_int(q0.w), cnt = (ex >> 24) & 7u;
    nd.levels = ex >> 27;
    nd.allow &= (1u << cnt) - 1u;
    if (COUNT) { nBox += (uint32_t)__popc(nd.allow); nNode += 1u; }
    nd.org = mk3(q0.x, q0.y, q0.z);
    nd.step = mk3(__int_as_float((int)((ex & 0xFFu) << 23)), __int_as_float((int)(((ex >> 8) & 0xFFu) << 23)), __int_as_float((int)(((ex >> 16) & 0xFFu) << 23)));
    nd.lx = (uint32_t)__float_as_int(q2.x); nd.ly = (uint32_t)__float_as_int(q2.y); nd.lz = (uint32_t)__float_as_int(q2.z);
    nd.hx = (uint32_t)__float_as_int(q2.w); nd.hy = (uint32_t)__float_as_int(q3.x); nd.hz = (uint32_t)__float_as_int(q3.y);
    nd.c0 = __float_as_int(q1.x); nd.c1 = __float_as_int(q1.y); nd.c2 = __float_as_int(q1.z); nd.c3 = __float_as_int(q1.w);
    return nd;
}

// One axis of a child's lower bound: the gap of p to [lo, hi], shrunk by k * max(|p|, |lo|, |hi|)
RT_DEV float point_gap(float p, float lo, float hi) {
    const float g = __builtin_fmaxf(__builtin_fmaxf(lo - p, p - hi), 0.0f);
    const float m = __builtin_fmaxf(__builtin_fabsf(p), __builtin_fmaxf(__builtin_fabsf(lo), __builtin_fabsf(hi)));
    return __builtin_fmaxf(g - kPointSlack * m, 0.0f);
}
// Child i's planes decoded as the builders verify them (Collapser::quantise, refit_node: fma(q, step, origin) with q * step exact, so the
// product and one add), its lower bound lb2, and the high word of its sort key: the bits of max(lb2, kNearClamp) if the child survives
// the cull, the miss word otherwise.  Only the sort key is clamped, never the cull.
RT_DEV uint32_t point_child_key(uint32_t i, f3 p, const NodeBoxes& nd, float bound, uint32_t missHi) {
    const float gx = point_gap(p.x, ubyte_f(nd.lx, i) * nd.step.x + nd.org.x, ubyte_f(nd.hx, i) * nd.step.x + nd.org.x);
    const float gy = point_gap(p.y, ubyte_f(nd.ly, i) * nd.step.y + nd.org.y, ubyte_f(nd.hy, i) * nd.step.y + nd.org.y);
    const float gz = point_gap(p.z, ubyte_f(nd.lz, i) * nd.step.z + nd.org.z, ubyte_f(nd.hz, i) * nd.step.z + nd.org.z);
    const float lb2 = (gx * gx + gy * gy) + gz * gz;
    return (lb2 * kPointKeep > bound) ? missHi : __float_as_uint(__builtin_fmaxf(lb2, kNearClamp));
}

// One visit of a 4-wide node for a point: node_step's order network, stack rule and resume entries around the box-distance test.
template <bool COUNT>
RT_DEV int32_t point_node_step(const float4* nodes, int32_t budget, int32_t cur, f3 p, float bound, Stack& st, uint32_t& nBox, uint32_t& nNode) {
    const NodeBoxes nd = fetch_node_boxes<COUNT>(nodes, cur, nBox, nNode);
    const uint32_t off = nd.off, allow = nd.allow, levels = nd.levels;
    // the four (lower bound, child reference) pairs as 64-bit keys, ordered with v_min_f64 / v_max_f64 as node_step orders its entry
    // distances: the high word is >= 1e-30 (the clamp) and finite (an infinite lb2 exceeds every bound), a positive normal double
    constexpr uint32_t kMissHi = 0x7F900000u;
    uint32_t h0 = point_child_key(0, p, nd, bound, kMissHi), h1 = point_child_key(1, p, nd, bound, kMissHi);
    uint32_t h2 = point_child_key(2, p, nd, bound, kMissHi), h3 = point_child_key(3, p, nd, bound, kMissHi);
    h0 = (allow & 1u) ? h0 : kMissHi; h1 = (allow & 2u) ? h1 : kMissHi; h2 = (allow & 4u) ? h2 : kMissHi; h3 = (allow & 8u) ? h3 : kMissHi;
    const int32_t c0 = nd.c0, c1 = nd.c1, c2 = nd.c2, c3 = nd.c3;
    double d0 = __hiloint2double((int)h0, c0), d1 = __hiloint2double((int)h1, c1), d2 = __hiloint2double((int)h2, c2), d3 = __hiloint2double((int)h3, c3);
    order_keys(d0, d1); order_keys(d2, d3); order_keys(d0, d2); order_keys(d1, d3); order_keys(d1, d2);
    const uint32_t s0h = (uint32_t)__double2hiint(d0), s1h = (uint32_t)__double2hiint(d1), s2h = (uint32_t)__double2hiint(d2), s3h = (uint32_t)__double2hiint(d3);
    const int32_t r0 = __double2loint(d0), r1 = __double2loint(d1), r2 = __double2loint(d2), r3 = __double2loint(d3);
    // node_step's stack rule: far-to-near pushes while pending + 2 + levels <= budget, one resume entry otherwise
#define RT_PUSH3() do { st.lds[st.top * kBlock] = r3; st.top += (s3h < kMissHi) ? 1 : 0; \
                        st.lds[st.top * kBlock] = r2; st.top += (s2h < kMissHi) ? 1 : 0; \
                        st.lds[st.top * kBlock] = r1; st.top += (s1h < kMissHi) ? 1 : 0; } while (0)
    const uint64_t noRoom = __ballot((st.top - 1) + 2 + (int)levels > budget);
    if (noRoom == 0ull) RT_PUSH3();
    else if (((noRoom >> (threadIdx.x & 63u)) & 1ull) == 0ull) RT_PUSH3();
    else if (s1h < kMissHi) {
        const uint32_t hit = (h0 < kMissHi ? 1u : 0u) | (h1 < kMissHi ? 2u : 0u) | (h2 < kMissHi ? 4u : 0u) | (h3 < kMissHi ? 8u : 0u);
        const uint32_t nearest = (c0 == r0) ? 1u : (c1 == r0) ? 2u : (c2 == r0) ? 4u : 8u;
        st.push(kResumeBase | (int32_t)(off | (hit & ~nearest)));
    }
#undef RT_PUSH3
    return (s0h < kMissHi) ? r0 : st.pop();
}

// One leaf's triangles against the list; returns the cull bound that holds afterwards
template <class F>
RT_DEV float points_leaf(const DevScene& sc, const HitList& l, uint32_t maxHits, int32_t cur, f3 p, float r2, unsigned long long lowKey,
                         uint32_t& n, unsigned long long& worst, float bound, uint32_t& nTri, bool count, const F& flt) {
    const uint32_t code = (uint32_t)~cur, firstTri = code >> 2, cnt = (code & 3u) + 1u;
    for (uint32_t k = 0; k < cnt; ++k) {
        float dist2, u, v; uint32_t id;
        if (!flt.record(firstTri + k)) continue;
        if (count) nTri += 1;
        point_tri(sc.leafTris + (size_t)(firstTri + k) * 3, p, dist2, u, v, id);
        if (!(dist2 <= r2)) continue;
        const unsigned long long key = hit_key(dist2, id);
        if (key < lowKey || key >= worst) continue;
        hit_insert(l, maxHits, n, worst, key, u, v);
        if (n == maxHits) bound = __uint_as_float((uint32_t)(worst >> 32));
    }
    return bound;
}

// The point lane state: HitsLaneT with a point in place of the ray, the squared radius in place of the interval.  FILTER as RayLane's:
// a masked sub-tree is never entered, so near an excluded mesh the list still fills from the admitted ones and the cull bound shrinks.
template <bool FILTER> struct PointsLaneT : LaneFilter<FILTER> {
    using Query = typename std::conditional<FILTER, Filtered<QueryPoints>, QueryPoints>::type;
    static constexpr int kWaves = 5;            // as HitsLaneT: the list's LDS leaves room for no more workgroups from a 26-entry stack on
    const HitList list;
    f3 p = splat3(0.0f);
    float r2 = 0.0f, bound = 0.0f; uint32_t n = 0;
    unsigned long long worst = kNoWorstKey, lowKey = 0ull;
    RT_DEV PointsLaneT(const DevScene& sc, const Query& q, int32_t* s_stack) : list(hit_list(s_stack, sc.stackBudget, q.maxHits)) {}
    RT_DEV int32_t start(const DevScene& sc, const Query& q, uint32_t i) {
        this->load(q);
        const float4 r0 = q.rays[i];
        p = mk3(r0.x, r0.y, r0.z);
        r2 = point_r2(r0.w); bound = r2;
        n = 0; worst = kNoWorstKey;
        const bool wanted = points_start(q, i, lowKey);
        return (sc.triCount == 0 || !wanted || point_invalid(p, r0.w)) ? kExit : sc.rootRef;
    }
    template <bool COUNT> RT_DEV int32_t visit(const DevScene& sc, int32_t cur, Stack& st, uint32_t& nBox, uint32_t& nNode) {
        if (FILTER && !this->node(cur)) return st.pop();
        return point_node_step<COUNT>(sc.nodes, sc.stackBudget, cur, p, bound, st, nBox, nNode);
    }
    template <bool COUNT> RT_DEV bool leaf(const DevScene& sc, const Query& q, int32_t cur, uint32_t& nTri) {
        bound = points_leaf(sc, list, q.maxHits, cur, p, r2, lowKey, n, worst, bound, nTri, COUNT, static_cast<const LaneFilter<FILTER>&>(*this));
        return false;
    }
    RT_DEV bool finish(const DevScene&, const Query& q, uint32_t i) { store_hits(q, list, i, n); return n != 0u; }
};

}  // namespace rt
