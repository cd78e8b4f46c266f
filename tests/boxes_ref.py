"""Brute-force reference of the box-overlap query (fyprt_overlap_boxes): the separating-axis rule of include/fyprt.h restated in numpy
float32 over EVERY leaf record of ctx.export_bvh() — no tree — then the accepted triangle indices of a box in ascending order.  float32
throughout, the device's operation order, selects for min and max: every decision is the device's.  Also the traversal's cull rule
(rt_boxes.h: box_child_apart) restated for one exported node, for the CPU test that holds it to the rule.  A helper of the box-overlap
tests, not a test file."""
import numpy as np

import bruteforce
from bruteforce import F32, _cross, _dot
from points_ref import child_planes, leaf_records_below   # noqa: F401  (the decoded planes and the records below a child, as there)

NONE = np.uint32(0xFFFFFFFF)           # an unused slot; as `after`, a finished box
SLACK = F32(2.0 ** -20)                # k of the cull rule ("Box-overlap queries")
HALF = F32(0.5)


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a > b, a, b)


def _min3(a, b, c):
    return _min(_min(a, b), c)


def _max3(a, b, c):
    return _max(_max(a, b), c)


def invalid_boxes(lo, hi):
    """!(lo <= hi) on some axis, or lo + hi or hi - lo not finite."""
    with np.errstate(all="ignore"):
        return ~(lo <= hi).all(axis=1) | ~np.isfinite(lo + hi).all(axis=1) | ~np.isfinite(hi - lo).all(axis=1)


def box_tri(lo, hi, v0, e1, e2, steps=False):
    """The header's rule for boxes (B, 3) x leaf records (T, 3): accepted (B, T) bool.  With `steps`, the three partial decisions
    (box axes, edge axes, plane) instead, each (B, T)."""
    lo, hi = np.asarray(lo, F32).reshape(-1, 3), np.asarray(hi, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        LO = [lo[:, k:k + 1] for k in range(3)]
        HI = [hi[:, k:k + 1] for k in range(3)]
        V0 = [v0[None, :, k] for k in range(3)]
        E1 = [e1[None, :, k] for k in range(3)]
        E2 = [e2[None, :, k] for k in range(3)]
        V1 = [V0[k] + E1[k] for k in range(3)]
        V2 = [V0[k] + E2[k] for k in range(3)]
        axes = np.ones((len(lo), len(v0)), bool)
        for k in range(3):
            axes &= (_min3(V0[k], V1[k], V2[k]) <= HI[k]) & (_max3(V0[k], V1[k], V2[k]) >= LO[k])
        c = [(LO[k] + HI[k]) * HALF for k in range(3)]
        h = [(HI[k] - LO[k]) * HALF for k in range(3)]
        P = [[V[k] - c[k] for k in range(3)] for V in (V0, V1, V2)]
        assert P[0][0].dtype == F32 and h[0].dtype == F32
        edges = np.ones_like(axes)
        for f in (E1, [E2[k] - E1[k] for k in range(3)], E2):
            a = [np.abs(f[k]) for k in range(3)]
            for (i, j, ri, rj) in ((2, 1, 1, 2), (0, 2, 0, 2), (1, 0, 0, 1)):
                # x: s = p.z*f.y - p.y*f.z, r = h.y*|f.z| + h.z*|f.y|; y and z by rotation
                s = [p[i] * f[j] - p[j] * f[i] for p in P]
                r = h[ri] * a[rj] + h[rj] * a[ri]
                edges &= (_min3(*s) <= r) & (_max3(*s) >= -r)
        n = _cross(E1, E2)
        d = _dot(n, P[0])
        r = (h[0] * np.abs(n[0]) + h[1] * np.abs(n[1])) + h[2] * np.abs(n[2])
        assert d.dtype == F32 and r.dtype == F32
        plane = (d <= r) & (d >= -r)
    return (axes, edges, plane) if steps else axes & edges & plane


def accepted(bvh, lo, hi, batch=256):
    """(B, T) bool over the leaf records in exported order, invalid boxes all False; and the records' triangle indices."""
    v0, e1, e2, ids = bruteforce.leaf_records(bvh)
    lo, hi = np.asarray(lo, F32).reshape(-1, 3), np.asarray(hi, F32).reshape(-1, 3)
    ok = np.zeros((len(lo), len(ids)), bool)
    for sl in bruteforce._batches(len(lo), batch):
        ok[sl] = box_tri(lo[sl], hi[sl], v0, e1, e2)
    ok[invalid_boxes(lo, hi)] = False
    return ok, ids.astype(np.uint32)


def k_lowest(bvh, lo, hi, k, after=None, ok_ids=None):
    """The k lowest accepted triangle indices per box: (triangles (B, k) uint32, counts (B,) uint32, totals (B,) uint32).  With
    `after`, only indices greater than after[i]; after[i] == NONE finishes the box.  Unused slots are NONE; totals counts every
    accepted triangle, also beyond k.  `ok_ids`: an earlier result of accepted() for the same boxes."""
    ok, ids = ok_ids if ok_ids is not None else accepted(bvh, lo, hi)
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


def all_in_boxes(bvh, lo, hi, ok_ids=None):
    """Every accepted triangle per box, ascending, in triangles_in_boxes' shape: (flat uint32 indices, offsets (B + 1,) int64)."""
    ok, ids = ok_ids if ok_ids is not None else accepted(bvh, lo, hi)
    parts = [np.sort(ids[row]) for row in ok]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    flat = np.concatenate(parts).astype(np.uint32) if parts else np.empty(0, dtype=np.uint32)
    return flat, offsets


# ---- the traversal's cull rule for one exported node
def children_apart(node, lo, hi, slack=SLACK):
    """The skip decision of the node's children for boxes (B, 3): (B, cnt) bool, the kernel's operations in its order.  `slack`: k; 0
    gives the rule a kernel without slack would apply."""
    plo, phi = child_planes(node)
    lo, hi = np.asarray(lo, F32).reshape(-1, 3), np.asarray(hi, F32).reshape(-1, 3)
    out = np.zeros((len(lo), len(plo)), bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            pl, ph = plo[None, :, a], phi[None, :, a]
            s = F32(slack) * np.maximum(np.abs(pl), np.abs(ph))
            assert s.dtype == F32
            out |= ((pl - s) > hi[:, a:a + 1]) | ((ph + s) < lo[:, a:a + 1])
    return out


def protruding_boxes(bvh, margin=0.01):
    """Boxes that only a cull with slack gets right: wherever a record's ROUNDED vertex v0 + e lies outside a decoded plane of a child
    above it, a box around the record that begins (or ends) exactly on that vertex's coordinate — beyond the plane.  Returns
    (lo, hi, where): `where` lists (node, child slot, leaf record) per box.  Empty for a tree whose planes hold every rounded vertex."""
    v0, e1, e2, _ = bruteforce.leaf_records(bvh)
    v1, v2 = (v0 + e1).astype(F32), (v0 + e2).astype(F32)
    mn, mx = np.minimum(np.minimum(v0, v1), v2), np.maximum(np.maximum(v0, v1), v2)
    los, his, where = [], [], []
    for ni, (node, slots) in enumerate(zip(bvh["nodes"], leaf_records_below(bvh))):
        if slots is None:
            continue
        plo, phi = child_planes(node)
        for c, recs in enumerate(slots):
            for r in recs[((mx[recs] > phi[c]) | (mn[recs] < plo[c])).any(axis=1)]:
                for a in range(3):
                    lo, hi = mn[r] - F32(margin), mx[r] + F32(margin)
                    if mx[r, a] > phi[c, a]:
                        lo[a] = mx[r, a]
                    elif mn[r, a] < plo[c, a]:
                        hi[a] = mn[r, a]
                    else:
                        continue
                    los.append(lo); his.append(hi); where.append((ni, c, int(r)))
    return np.array(los, F32).reshape(-1, 3), np.array(his, F32).reshape(-1, 3), where
