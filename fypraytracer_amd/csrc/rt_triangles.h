// Triangle-overlap queries (fyprt_overlap_triangles / fyprt_overlap_triangles_device): the scene triangles that cut each of the
// caller's triangles, outside any frame — the narrow phase behind the box query's broad phase, a pure set like it.
//
//   triangle record : three float4 (48 B, 16-byte aligned) = q0 | pad, q1 | pad, q2 | pad
//   answer          : maxHits uint32 per query triangle, the lowest accepted scene-triangle indices ascending, unused = 0xFFFFFFFF; a
//                     count; a total
// A leaf record (v0, e1, e2) is accepted by tri_tri below: the separating-axis test of include/fyprt.h (three coordinate axes on the
// untranslated vertices against the query triangle's bounds, then 17 axes on the vertices relative to q0: the two normals, nine edge
// pairs, six in-plane edge normals), every operation rounded on its own, sel_min / sel_max / min_of3 / max_of3 of rt_boxes.h, every
// comparison written positively so that a NaN rejects.  With `after` the index must also be greater than after[i].  The answer is the
// maxHits smallest accepted indices: a function of the leaf records alone.
//
// The traversal is the box query's, unchanged: box_node_step with the query triangle's bounds [lo, hi] as the box, the same slack
// (kPointSlack).  The cull drops nothing because the coordinate-axis step IS the box rule's step 2 with [lo, hi] as the box: a child is
// skipped only if [lo, hi] is apart from its slack-widened planes on some axis, and then every record below it fails that step on that
// axis ("Triangle-overlap queries").  The list is BoxLaneT's: one LDS plane of uint32 behind the stack, tri_insert.
//
// Two forms by tuning key 15, as the other queries: query_body / query_simple_body of rt_query.h around TriLaneT.
#pragma once
#include "rt_boxes.h"

namespace rt {

struct QueryTriangles {
    const float4* tris; const uint32_t* after; uint32_t* triangles; uint32_t* counts; uint32_t* totals; uint32_t count, maxHits; uint32_t* head;
    uint32_t chunk, refillLanes, staticChunks, minChunk;
};

// A component of q0, q1, q2, f1 = q1 - q0 or f2 = q2 - q0 that is not finite (x - x is 0 for a finite x only)
RT_DEV bool tri_query_invalid(f3 q0, f3 q1, f3 q2, f3 f1, f3 f2) {
    const float a = ((q0.x - q0.x) + (q0.y - q0.y)) + (q0.z - q0.z), b = ((q1.x - q1.x) + (q1.y - q1.y)) + (q1.z - q1.z);
    const float c = ((q2.x - q2.x) + (q2.y - q2.y)) + (q2.z - q2.z), d = ((f1.x - f1.x) + (f1.y - f1.y)) + (f1.z - f1.z);
    const float e = ((f2.x - f2.x) + (f2.y - f2.y)) + (f2.z - f2.z);
    return !((((a + b) + c) + (d + e)) == 0.0f);
}

// One rounded binary32 multiply / add / subtract as one instruction.  Left to itself the compiler pairs the three dot products of an axis
// into packed v_pk_mul_f32 / v_pk_add_f32 and keeps swizzled copies of p_k, f1 and f2 for them: 142 to 156 VGPRs for the one-thread
// kernel, 240 to 332 B of scratch in the persistent kernels at 5 waves per SIMD and 104 to 176 B at 4; as single instructions the same
// operations need 70 to 97 VGPRs over the eight kernels and no scratch ("Triangle-overlap queries", with the compiler
// version).  The bits are the same: each operation is rounded on its own either way.
RT_DEV float tri_mul(float a, float b) { float r; asm("v_mul_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RT_DEV float tri_add(float a, float b) { float r; asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
RT_DEV float tri_sub(float a, float b) { float r; asm("v_sub_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// dot and cross of rt_math.h, operation for operation
RT_DEV float tri_dot(f3 a, f3 b) { return tri_add(tri_add(tri_mul(a.x, b.x), tri_mul(a.y, b.y)), tri_mul(a.z, b.z)); }
RT_DEV f3 tri_cross(f3 a, f3 b) {
    return mk3(tri_sub(tri_mul(a.y, b.z), tri_mul(b.y, a.z)), tri_sub(tri_mul(a.z, b.x), tri_mul(b.z, a.x)), tri_sub(tri_mul(a.x, b.y), tri_mul(b.x, a.y)));
}

// One separating axis: the scene triangle's interval over t_k = dot(a, p_k) against the query triangle's over 0, dot(a, f1), dot(a, f2)
RT_DEV bool tri_axis(f3 a, f3 p0, f3 p1, f3 p2, f3 f1, f3 f2) {
    const float t0 = tri_dot(a, p0), t1 = tri_dot(a, p1), t2 = tri_dot(a, p2), s1 = tri_dot(a, f1), s2 = tri_dot(a, f2);
    return min_of3(t0, t1, t2) <= max_of3(0.0f, s1, s2) && max_of3(t0, t1, t2) >= min_of3(0.0f, s1, s2);
}

// Whether the leaf record's triangle touches the query triangle (q0, q0 + f1, q0 + f2) with bounds [lo, hi], include/fyprt.h's rule
RT_DEV bool tri_tri(const float4* tp, f3 lo, f3 hi, f3 q0, f3 f1, f3 f2, uint32_t& id) {
    const float4 a = tp[0], b = tp[1], cc = tp[2];
    id = (uint32_t)__float_as_int(cc.y);
    const f3 v0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y), e2 = mk3(b.z, b.w, cc.x);
    const f3 v1 = v0 + e1, v2 = v0 + e2;
    if (!(min_of3(v0.x, v1.x, v2.x) <= hi.x && max_of3(v0.x, v1.x, v2.x) >= lo.x)) return false;
    if (!(min_of3(v0.y, v1.y, v2.y) <= hi.y && max_of3(v0.y, v1.y, v2.y) >= lo.y)) return false;
    if (!(min_of3(v0.z, v1.z, v2.z) <= hi.z && max_of3(v0.z, v1.z, v2.z) >= lo.z)) return false;
    const f3 p0 = v0 - q0, p1 = v1 - q0, p2 = v2 - q0;
    const f3 n = tri_cross(e1, e2), m = tri_cross(f1, f2);
    if (!tri_axis(n, p0, p1, p2, f1, f2)) return false;
    if (!tri_axis(m, p0, p1, p2, f1, f2)) return false;
    const f3 g[3] = {e1, e2 - e1, e2}, h[3] = {f1, f2 - f1, f2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) if (!tri_axis(tri_cross(g[i], h[j]), p0, p1, p2, f1, f2)) return false;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) if (!tri_axis(tri_cross(n, g[i]), p0, p1, p2, f1, f2)) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) if (!tri_axis(tri_cross(m, h[j]), p0, p1, p2, f1, f2)) return false;
    return true;
}

// The triangle lane state: the query triangle's bounds for the walk, (q0, f1, f2) for the leaf test, and the list's length, worst entry,
// lowest admissible index and the total in registers.  FILTER as RayLane's; the total then counts admitted triangles only.
template <bool FILTER> struct TriLaneT : LaneFilter<FILTER> {
    using Query = typename std::conditional<FILTER, Filtered<QueryTriangles>, QueryTriangles>::type;
    // 5 waves per SIMD as the other list queries: 85 VGPRs plain and 91 filtered, no scratch.  (q0, f1, f2) are carried across the walk:
    // loading the query triangle again in every leaf instead saves no register here (88 and 94)
    static constexpr int kWaves = 5;
    uint32_t* const list;                       // &plane[threadIdx.x]; entry s at [s * kBlock]
    f3 lo = splat3(0.0f), hi = splat3(0.0f);
    f3 q0 = splat3(0.0f), f1 = splat3(0.0f), f2 = splat3(0.0f);
    uint32_t n = 0, worst = kNoTriangle, low = 0, total = 0;
    RT_DEV TriLaneT(const DevScene& sc, const Query&, int32_t* s_stack)
        : list(reinterpret_cast<uint32_t*>(s_stack + (size_t)(sc.stackBudget + 1) * kBlock) + threadIdx.x) {}
    RT_DEV int32_t start(const DevScene& sc, const Query& q, uint32_t i) {
        this->load(q);
        const float4 t0 = q.tris[(size_t)i * 3], t1 = q.tris[(size_t)i * 3 + 1], t2 = q.tris[(size_t)i * 3 + 2];
        const f3 a = mk3(t0.x, t0.y, t0.z), b = mk3(t1.x, t1.y, t1.z), c = mk3(t2.x, t2.y, t2.z);
        lo = mk3(min_of3(a.x, b.x, c.x), min_of3(a.y, b.y, c.y), min_of3(a.z, b.z, c.z));
        hi = mk3(max_of3(a.x, b.x, c.x), max_of3(a.y, b.y, c.y), max_of3(a.z, b.z, c.z));
        const f3 d1 = b - a, d2 = c - a;
        q0 = a; f1 = d1; f2 = d2;
        n = 0; worst = kNoTriangle; low = 0; total = 0;
        bool wanted = true;
        if (q.after) { const uint32_t w = q.after[i]; wanted = w != kNoTriangle; low = w + 1u; }     // no index lies above all ones: the record is finished
        return (sc.triCount == 0 || !wanted || tri_query_invalid(a, b, c, d1, d2)) ? kExit : sc.rootRef;
    }
    template <bool COUNT> RT_DEV int32_t visit(const DevScene& sc, int32_t cur, Stack& st, uint32_t& nBox, uint32_t& nNode) {
        if (FILTER && !this->node(cur)) return st.pop();
        return box_node_step<COUNT>(sc.nodes, sc.stackBudget, cur, lo, hi, st, nBox, nNode);
    }
    template <bool COUNT> RT_DEV bool leaf(const DevScene& sc, const Query& q, int32_t cur, uint32_t& nTri) {
        const uint32_t code = (uint32_t)~cur, firstTri = code >> 2, cnt = (code & 3u) + 1u;
        for (uint32_t k = 0; k < cnt; ++k) {
            uint32_t id;
            if (FILTER && !this->record(firstTri + k)) continue;
            if (COUNT) nTri += 1;
            if (!tri_tri(sc.leafTris + (size_t)(firstTri + k) * 3, lo, hi, q0, f1, f2, id) || id < low) continue;
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
