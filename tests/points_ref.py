"""Brute-force reference of the nearest-point query (fyprt_nearest_points): the point/triangle rule of include/fyprt.h restated in numpy
float32 over EVERY leaf record of ctx.export_bvh() — no tree — then the accepted triangles of a point sorted by the key
(bits(distance2) << 32) | triangle.  float32 throughout, the device's operation order: every distance2, u and v is the device's bit for
bit.  Also the traversal's cull rule (rt_points.h: point_child_key) restated for one exported node, for the CPU test that holds it to
the triangle arithmetic.  A helper of the nearest-point tests, not a test file."""
import numpy as np

import bruteforce
from bruteforce import F32, FLT_MAX, ONE, ZERO, _dot
from fypraytracer_amd import capi
from multihit_ref import record_diff, records_equal   # noqa: F401  (16-byte records either way)

UNUSED = np.array([(-1.0, 0xFFFFFFFF, 0.0, 0.0)], dtype=capi.POINT_HIT_DTYPE)[0]
SLACK = F32(2.0 ** -20)                # k of the cull rule ("Nearest-point queries")
KEEP = F32(1.0) - SLACK                # 1 - k, exact in binary32
NEAR_CLAMP = F32(1e-30)


def point_tri(p, v0, e1, e2):
    """The header's rule for points (P, 3) x leaf records (T, 3): (distance2, u, v) as (P, T) float32 arrays."""
    with np.errstate(all="ignore"):
        P = [np.asarray(p, F32)[:, k:k + 1] for k in range(3)]
        V0 = [v0[None, :, k] for k in range(3)]
        E1 = [e1[None, :, k] for k in range(3)]
        E2 = [e2[None, :, k] for k in range(3)]
        ap = [P[k] - V0[k] for k in range(3)]
        d1, d2 = _dot(E1, ap), _dot(E2, ap)
        bp = [ap[k] - E1[k] for k in range(3)]
        d3, d4 = _dot(E1, bp), _dot(E2, bp)
        vc = d1 * d4 - d3 * d2
        cp = [ap[k] - E2[k] for k in range(3)]
        d5, d6 = _dot(E1, cp), _dot(E2, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        a, b = d4 - d3, d5 - d6
        w = a / (a + b)
        s = (va + vb) + vc
        f = ONE / s
        conds = [(d1 <= ZERO) & (d2 <= ZERO),
                 (d3 >= ZERO) & (d4 <= d3),
                 (vc <= ZERO) & (d1 >= ZERO) & (d3 <= ZERO),
                 (d6 >= ZERO) & (d5 <= d6),
                 (vb <= ZERO) & (d2 >= ZERO) & (d6 <= ZERO),
                 (va <= ZERO) & (a >= ZERO) & (b >= ZERO)]
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        u = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, ONE - w], vb * f).astype(F32)
        v = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w], vc * f).astype(F32)
        u = np.where(u < ZERO, ZERO, np.where(u > ONE, ONE, u)).astype(F32)          # selects: a NaN stays a NaN
        m = ONE - u
        v = np.where(v < ZERO, ZERO, np.where(v > m, m, v)).astype(F32)
        diff = [(ap[k] - u * E1[k]) - v * E2[k] for k in range(3)]
        dist2 = _dot(diff, diff)
    assert dist2.dtype == F32 and u.dtype == F32 and v.dtype == F32
    return dist2, u, v


def region_of(p, v0, e1, e2):
    """Which branch of the rule answered (0 = vertex A, 1 = B, 2 = edge AB, 3 = C, 4 = edge AC, 5 = edge BC, 6 = interior), (P, T)."""
    with np.errstate(all="ignore"):
        P = [np.asarray(p, F32)[:, k:k + 1] for k in range(3)]
        ap = [P[k] - v0[None, :, k] for k in range(3)]
        E1 = [e1[None, :, k] for k in range(3)]
        E2 = [e2[None, :, k] for k in range(3)]
        d1, d2 = _dot(E1, ap), _dot(E2, ap)
        bp = [ap[k] - E1[k] for k in range(3)]
        d3, d4 = _dot(E1, bp), _dot(E2, bp)
        cp = [ap[k] - E2[k] for k in range(3)]
        d5, d6 = _dot(E1, cp), _dot(E2, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        a, b = d4 - d3, d5 - d6
        conds = [(d1 <= ZERO) & (d2 <= ZERO), (d3 >= ZERO) & (d4 <= d3), (vc <= ZERO) & (d1 >= ZERO) & (d3 <= ZERO),
                 (d6 >= ZERO) & (d5 <= d6), (vb <= ZERO) & (d2 >= ZERO) & (d6 <= ZERO), (va <= ZERO) & (a >= ZERO) & (b >= ZERO)]
        return np.select(conds, [0, 1, 2, 3, 4, 5], 6)


def hit_keys(rec):
    """The 64-bit order key of hit records: (bits(distance2) << 32) | triangle."""
    return (np.ascontiguousarray(rec["distance2"]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rec["triangle"].astype(np.uint64)


def invalid_points(p, max_distance):
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(p).all(axis=1) | ~(max_distance >= ZERO)


def radius2(max_distance):
    with np.errstate(all="ignore"):
        return np.minimum((max_distance * max_distance).astype(F32), FLT_MAX)          # (a NaN max_distance is an invalid point)


def k_nearest(bvh, p, max_distance, k, after=None, batch=128):
    """The k smallest-key accepted triangles per point: (hits (P, k) POINT_HIT_DTYPE, counts (P,) uint32, totals (P,) int64).  Accepted:
    distance2 <= min(max_distance^2, FLT_MAX) and, with `after`, key > key(after[i]); an after[i] with distance2 < 0 finishes the
    point, an invalid point answers nothing.  Unused records are UNUSED; totals counts every accepted triangle, also beyond k."""
    v0, e1, e2, ids = bruteforce.leaf_records(bvh)
    p = np.asarray(p, F32).reshape(-1, 3)
    n = len(p)
    md = np.broadcast_to(np.asarray(max_distance, dtype=F32), (n,))
    r2, bad = radius2(md), invalid_points(p, md)
    hits = np.full((n, k), UNUSED, dtype=capi.POINT_HIT_DTYPE)
    counts = np.zeros(n, dtype=np.uint32)
    totals = np.zeros(n, dtype=np.int64)
    if after is not None:
        after = np.asarray(after).reshape(-1)
        assert after.dtype == capi.POINT_HIT_DTYPE and len(after) == n
        after_key, finished = hit_keys(after), after["distance2"] < 0
    for sl in bruteforce._batches(n, batch):
        dist2, u, v = point_tri(p[sl], v0, e1, e2)
        with np.errstate(invalid="ignore"):
            ok = dist2 <= r2[sl, None]
        for r in range(ok.shape[0]):
            i = sl.start + r
            if bad[i] or (after is not None and finished[i]):
                continue
            m = np.nonzero(ok[r])[0]
            db = np.ascontiguousarray(dist2[r, m], dtype=F32).view(np.uint32)
            tri = ids[m].astype(np.uint32)
            if after is not None:
                keep = ((db.astype(np.uint64) << np.uint64(32)) | tri.astype(np.uint64)) > after_key[i]
                m, db, tri = m[keep], db[keep], tri[keep]
            order = np.lexsort((tri, db))                    # primary key: the bits of distance2; ties: the triangle index
            totals[i] = len(order)
            order = order[:k]
            c = len(order)
            counts[i] = c
            hits["distance2"][i, :c], hits["triangle"][i, :c] = dist2[r, m[order]], tri[order]
            hits["u"][i, :c], hits["v"][i, :c] = u[r, m[order]], v[r, m[order]]
    return hits, counts, totals


def all_within(bvh, p, radius, batch=128):
    """Every triangle within `radius` per point in key order, in triangles_within's shape: (flat records, offsets (P + 1,) int64)."""
    n = len(np.asarray(p).reshape(-1, 3))
    _, _, totals = k_nearest(bvh, p, radius, 1, batch=batch)
    kmax = max(1, int(totals.max(initial=0)))
    hits, counts, _ = k_nearest(bvh, p, radius, kmax, batch=batch)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.int64))]).astype(np.int64)
    flat = np.concatenate([hits[i, :counts[i]] for i in range(n)]) if n else np.empty(0, dtype=capi.POINT_HIT_DTYPE)
    return flat, offsets


# ---- the traversal's cull rule for one exported node
def child_planes(node):
    """Decoded child planes of one exported node as the kernel decodes them: (lo (cnt, 3), hi (cnt, 3)) float32 — q * 2^(e-127) is
    exact, then one add."""
    cnt = int(node["meta"]) & 7
    step = np.ldexp(F32(1.0), node["ex"].astype(np.int32) - 127).astype(F32)
    lo = (node["qlo"][:, :cnt].T.astype(F32) * step[None, :]).astype(F32) + node["origin"][None, :]
    hi = (node["qhi"][:, :cnt].T.astype(F32) * step[None, :]).astype(F32) + node["origin"][None, :]
    return lo.astype(F32), hi.astype(F32)


def child_lower_bounds(node, p):
    """lb2 of the node's children for points (P, 3): (P, cnt) float32, the kernel's operations in its order."""
    lo, hi = child_planes(node)
    p = np.asarray(p, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        g2 = []
        for a in range(3):
            pa, la, ha = p[:, a:a + 1], lo[None, :, a], hi[None, :, a]
            g = np.maximum(np.maximum(la - pa, pa - ha), ZERO)
            m = np.maximum(np.abs(pa), np.maximum(np.abs(la), np.abs(ha)))
            gs = np.maximum(g - SLACK * m, ZERO).astype(F32)
            g2.append(gs * gs)
        lb2 = (g2[0] + g2[1]) + g2[2]
    assert lb2.dtype == F32
    return lb2


def culled(lb2, bound):
    """The skip decision: lb2 * (1 - k) > bound."""
    with np.errstate(all="ignore"):
        return (lb2 * KEEP) > bound


def leaf_records_below(bvh):
    """For every node, per child slot, the indices (into bvh['tris']) of the leaf records below that child: a list of lists of arrays."""
    nodes = bvh["nodes"]
    out = [None] * len(nodes)

    def below(ref):
        if ref < 0:
            code = ~ref
            return np.arange(code >> 2, (code >> 2) + (code & 3) + 1)
        if out[ref] is None:
            cnt = int(nodes[ref]["meta"]) & 7
            out[ref] = [below(int(nodes[ref]["child"][c])) for c in range(cnt)]
        return np.concatenate(out[ref])

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(10000)
    try:
        below(int(bvh["root"]))
    finally:
        sys.setrecursionlimit(old)
    return out
