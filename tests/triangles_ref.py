"""Brute-force reference of the triangle-overlap query (fyprt_overlap_triangles): the separating-axis rule of include/fyprt.h restated
in numpy float32 over EVERY leaf record of ctx.export_bvh() — no tree — then the accepted triangle indices of a query triangle in
ascending order.  float32 throughout, the device's operations (every one rounded on its own), selects for min and max: every decision is
the device's.  The traversal's cull is the box query's with the query triangle's bounds as the box (boxes_ref.children_apart).  A helper
of the triangle-overlap tests, not a test file."""
import numpy as np

import bruteforce
from bruteforce import F32, _cross, _dot
from boxes_ref import NONE, SLACK, _max3, _min3, children_apart, leaf_records_below  # noqa: F401  (the cull with the query bounds, as the box query's)

ZERO = F32(0.0)


def _comp(a):
    """(..., 3) float32 -> the three component arrays."""
    a = np.asarray(a, F32)
    return [a[..., k] for k in range(3)]


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def bounds(q):
    """lo, hi (N, 3) of query triangles (N, 3, 3) by the selects of step 1."""
    q = np.asarray(q, F32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        lo = np.stack([_min3(q[:, 0, k], q[:, 1, k], q[:, 2, k]) for k in range(3)], axis=1)
        hi = np.stack([_max3(q[:, 0, k], q[:, 1, k], q[:, 2, k]) for k in range(3)], axis=1)
    return lo.astype(F32), hi.astype(F32)


def invalid_triangles(q):
    """A non-finite component of q0, q1, q2, f1 = q1 - q0 or f2 = q2 - q0."""
    q = np.asarray(q, F32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        f1, f2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
        return ~(np.isfinite(q).all(axis=(1, 2)) & np.isfinite(f1).all(axis=1) & np.isfinite(f2).all(axis=1))


def _axis(a, P, F1, F2):
    t = [_dot(a, p) for p in P]
    s1, s2 = _dot(a, F1), _dot(a, F2)
    assert t[0].dtype == F32 and s1.dtype == F32
    return (_min3(*t) <= _max3(ZERO, s1, s2)) & (_max3(*t) >= _min3(ZERO, s1, s2))


def rule(Q0, Q1, Q2, V0, E1, E2, steps=False):
    """The header's rule on component lists that broadcast against each other (three float32 arrays per vector).  Returns the
    decision, or with `steps` the four partial decisions (coordinate axes, the two normals, the nine edge pairs, the six in-plane
    edge normals) whose conjunction it is."""
    with np.errstate(all="ignore"):
        V1 = [V0[k] + E1[k] for k in range(3)]
        V2 = [V0[k] + E2[k] for k in range(3)]
        coord = True
        for k in range(3):
            lo, hi = _min3(Q0[k], Q1[k], Q2[k]), _max3(Q0[k], Q1[k], Q2[k])
            coord = coord & (_min3(V0[k], V1[k], V2[k]) <= hi) & (_max3(V0[k], V1[k], V2[k]) >= lo)
        F1, F2 = _sub(Q1, Q0), _sub(Q2, Q0)
        P = [_sub(V, Q0) for V in (V0, V1, V2)]
        assert P[0][0].dtype == F32 and F1[0].dtype == F32
        n, m = _cross(E1, E2), _cross(F1, F2)
        G = (E1, _sub(E2, E1), E2)
        H = (F1, _sub(F2, F1), F2)
        normals = _axis(n, P, F1, F2) & _axis(m, P, F1, F2)
        pairs = True
        for g in G:
            for h in H:
                pairs = pairs & _axis(_cross(g, h), P, F1, F2)
        inplane = True
        for g in G:
            inplane = inplane & _axis(_cross(n, g), P, F1, F2)
        for h in H:
            inplane = inplane & _axis(_cross(m, h), P, F1, F2)
    return (coord, normals, pairs, inplane) if steps else coord & normals & pairs & inplane


def tri_pairs(q, v0, e1, e2, steps=False):
    """Pair i: query triangle q[i] (N, 3, 3) against the record (v0[i], e1[i], e2[i]); (N,) bool (no invalid check)."""
    q = np.asarray(q, F32).reshape(-1, 3, 3)
    return rule(_comp(q[:, 0]), _comp(q[:, 1]), _comp(q[:, 2]), _comp(v0), _comp(e1), _comp(e2), steps)


def tri_tri(q, v0, e1, e2, steps=False):
    """Query triangles (B, 3, 3) x leaf records (T, 3): accepted (B, T) bool, or with `steps` the four partial decisions."""
    q = np.asarray(q, F32).reshape(-1, 3, 3)
    col = lambda a: [c[:, None] for c in _comp(a)]
    row = lambda a: [c[None, :] for c in _comp(a)]
    return rule(col(q[:, 0]), col(q[:, 1]), col(q[:, 2]), row(v0), row(e1), row(e2), steps)


def accepted(bvh, q, batch=128, admitted=None, steps=False):
    """(B, T) bool over the leaf records in exported order, invalid query triangles all False; and the records' triangle indices.
    `admitted`: None or a bool per TRIANGLE INDEX (the query filter).  With `steps` the four partial decisions instead of the one."""
    v0, e1, e2, ids = bruteforce.leaf_records(bvh)
    q = np.asarray(q, F32).reshape(-1, 3, 3)
    parts = [np.zeros((len(q), len(ids)), bool) for _ in range(4 if steps else 1)]
    for sl in bruteforce._batches(len(q), batch):
        res = tri_tri(q[sl], v0, e1, e2, steps)
        for p, r in zip(parts, res if steps else (res,)):
            p[sl] = r
    bad = invalid_triangles(q)
    for p in parts:
        p[bad] = False
        if admitted is not None:
            p[:, ~np.asarray(admitted, bool)[ids]] = False
    return (tuple(parts) if steps else parts[0]), ids.astype(np.uint32)


def k_lowest(bvh, q, k, after=None, ok_ids=None, admitted=None):
    """The k lowest accepted triangle indices per query triangle: (triangles (B, k) uint32, counts, totals), as boxes_ref.k_lowest."""
    ok, ids = ok_ids if ok_ids is not None else accepted(bvh, q, admitted=admitted)
    n = len(ok)
    tris = np.full((n, k), NONE, dtype=np.uint32)
    counts = np.zeros(n, dtype=np.uint32)
    totals = np.zeros(n, dtype=np.uint32)
    if after is not None:
        after = np.asarray(after).reshape(-1)
        assert after.dtype == np.uint32 and len(after) == n
    for i in range(n):
        if after is not None and after[i] == NONE:
            continue
        t = np.sort(ids[ok[i]])
        if after is not None:
            t = t[t > after[i]]
        totals[i] = len(t)
        c = min(k, len(t))
        counts[i] = c
        tris[i, :c] = t[:c]
    return tris, counts, totals


def all_touching(bvh, q, ok_ids=None, admitted=None):
    """Every accepted triangle per query triangle, ascending, in triangles_touching's shape: (flat uint32 indices, offsets int64)."""
    ok, ids = ok_ids if ok_ids is not None else accepted(bvh, q, admitted=admitted)
    parts = [np.sort(ids[row]) for row in ok]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    flat = np.concatenate(parts).astype(np.uint32) if parts else np.empty(0, dtype=np.uint32)
    return flat, offsets


# ---- what the CPU and the GPU tests share: a query set for a scene, and the cull rule held to the decisions
def scene_queries(sc, bvh, n, seed):
    """Random triangles of three sizes in the scene box, the scene's own triangles unmoved and jittered, triangles with a vertex
    bit-equal to a record's v0, zero-area ones."""
    rng = np.random.default_rng(seed)
    pos = sc.world_vertices["position"].astype(np.float64)
    slo, shi = pos.min(axis=0), pos.max(axis=0)
    ext = float((shi - slo).max())
    centre = rng.uniform(slo, shi, size=(n, 1, 3))
    rand = (centre + rng.normal(size=(n, 3, 3)) * ext * rng.choice([0.01, 0.05, 0.2], size=(n, 1, 1))).astype(F32)
    v0, e1, e2, _ = bruteforce.leaf_records(bvh)
    pick = rng.integers(0, len(v0), n // 2)
    own = np.stack([v0[pick], v0[pick] + e1[pick], v0[pick] + e2[pick]], axis=1).astype(F32)
    moved = (own + rng.normal(size=(len(own), 1, 3)) * ext * 0.01).astype(F32)
    shared = (v0[pick][:, None, :] + rng.normal(size=(len(pick), 3, 3)) * ext * 0.03).astype(F32)
    shared[np.arange(len(pick)), rng.integers(0, 3, len(pick))] = v0[pick]
    flat = rand[: n // 4].copy()
    flat[:, 2] = flat[:, 1]                                                   # needles
    flat[::2, 1] = flat[::2, 0]                                               # points
    return np.concatenate([rand, own, moved, shared, flat]).astype(F32)


def check_cull(bvh, q, ok, tag):
    """No child with an accepted record below it is skipped by the box walk's cull on the query triangles' bounds."""
    lo, hi = bounds(q)
    below = leaf_records_below(bvh)
    tested = skipped = 0
    for node, slots in zip(bvh["nodes"], below):
        if slots is None:
            continue
        apart = children_apart(node, lo, hi)
        for c, recs in enumerate(slots):
            wanted = ok[:, recs].any(axis=1)
            assert not (apart[:, c] & wanted).any(), (tag, c, node, np.nonzero(apart[:, c] & wanted)[0][:4])
            tested += len(lo)
            skipped += int(apart[:, c].sum())
    assert tested > 0 and skipped > tested // 4, (tag, skipped, tested)       # the rule is exercised, not vacuous
    return tested
