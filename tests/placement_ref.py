"""The placement rule of fyprt_set_append_placement(ctx, 1) (include/fyprt.h) restated in numpy, and the link rule of a placed graft
restated on two exports of the acceleration structure.  Every operation is a binary32 one, rounded on its own (numpy float32 scalars)."""
import numpy as np

F = np.float32
FIRST, SLOT, PAIR, ROOT_PAIR, REBUILT = range(5)
MAX_LEVELS = 31
MAX_NODES = 1 << 24


def area(lo, hi):
    """A(b) = (d.x*d.y + d.y*d.z) + d.z*d.x with d = hi - lo."""
    dx, dy, dz = F(hi[0]) - F(lo[0]), F(hi[1]) - F(lo[1]), F(hi[2]) - F(lo[2])
    return F(F(F(dx * dy) + F(dy * dz)) + F(dz * dx))


def union_area(lo, hi, blo, bhi):
    return area(np.minimum(lo, blo), np.maximum(hi, bhi))


def triangle_corners(pos, triangles, idx):
    """(len(idx), 3, 3) world positions of the listed triangles' vertices."""
    t = triangles[idx]
    return np.stack([pos[t["v0"]], pos[t["v1"]], pos[t["v2"]]], axis=1).astype(np.float32)


def exact_boxes(export, pos, triangles):
    """Exact boxes of an exported tree from the scene's vertices through the leaf records' triangle indices.  Returns (lo, hi) per
    node, parent per node (-1 for the root) and leaf_box(code) -> (lo, hi)."""
    nodes, tris = export["nodes"], export["tris"]
    n = len(nodes)
    lo, hi = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    parent = np.full(n, -1, dtype=np.int64)

    def leaf_box(ref):
        code = ~int(ref)
        first, m = code >> 2, (code & 3) + 1
        p = triangle_corners(pos, triangles, tris["tri"][first:first + m]).reshape(-1, 3)
        return p.min(axis=0), p.max(axis=0)

    for x in sorted(range(n), key=lambda k: int(nodes[k]["meta"]) >> 3):        # children (lower level counts) first
        l, h = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
        for i in range(int(nodes[x]["meta"]) & 7):
            c = int(nodes[x]["child"][i])
            if c >= 0:
                parent[c] = x
                cl, ch = lo[c], hi[c]
            else:
                cl, ch = leaf_box(c)
            l, h = np.minimum(l, cl), np.maximum(h, ch)
        lo[x], hi[x] = l, h
    return lo, hi, parent, leaf_box


def candidates(before_export, scene_vertices, triangles, new_range, sub_levels, sub_nodes=0):
    """Every feasible, finite candidate of the rule as (cost_bits, id), for an inner root; plus the parent array of the old tree."""
    nodes = before_export["nodes"]
    root, n = int(before_export["root"]), len(before_export["nodes"])
    pos = np.asarray(scene_vertices, dtype=np.float32)
    corners = triangle_corners(pos, triangles, np.arange(new_range[0], new_range[1])).reshape(-1, 3)
    blo, bhi = corners.min(axis=0), corners.max(axis=0)
    lo, hi, parent, leaf_box = exact_boxes(before_export, pos, triangles)
    h = int(sub_levels)
    levels = lambda ref: (int(nodes[ref]["meta"]) >> 3) if ref >= 0 else 0
    g = [F(union_area(lo[y], hi[y], blo, bhi) - area(lo[y], hi[y])) for y in range(n)]
    slot_ok, pair_ok = n + sub_nodes < MAX_NODES, n + sub_nodes + 1 < MAX_NODES
    out = []

    def offer(cost, ident):
        if np.isfinite(cost):
            out.append((int(np.float32(cost).view(np.uint32)), ident))

    for x in range(n):
        acc, d, p = g[x], 0, int(parent[x])
        while p >= 0:
            acc, d, p = F(acc + g[p]), d + 1, int(parent[p])
        cnt, lx = int(nodes[x]["meta"]) & 7, levels(x)
        if cnt < 4 and slot_ok and d + max(lx, h + 1) <= MAX_LEVELS:
            offer(acc, x * 8 + 4)
        for i in range(cnt):
            c = int(nodes[x]["child"][i])
            hn = 1 + max(levels(c), h)
            if pair_ok and d + max(lx, hn + 1) <= MAX_LEVELS:
                cl, ch = (lo[c], hi[c]) if c >= 0 else leaf_box(c)
                offer(F(acc + union_area(cl, ch, blo, bhi)), x * 8 + i)
    if pair_ok and 1 + max(levels(root), h) <= MAX_LEVELS:
        offer(union_area(lo[root], hi[root], blo, bhi), 0xFFFFFFFF)
    return out, parent


def place(before_export, scene_vertices, triangles, new_range, sub_levels, sub_nodes=0):
    """The rule.  `scene_vertices`: (V, 3) world positions of the combined scene; `triangles`: its triangle records; `new_range` =
    (first, end) of the appended triangles; `sub_levels`: the level count of the sub-tree's root (0 for a leaf code); `sub_nodes`: its
    node count, which only the node-range rule reads.
    Returns (kind, node, slot, depth, cost_bits, candidates)."""
    if len(before_export["tris"]) == 0:
        return (FIRST, 0, 0, 0, 0, 0)
    if int(before_export["root"]) < 0:
        return (ROOT_PAIR, 0, 0, 0, 0, 0)                       # a leaf-code root: mode 0's rule, no search
    cands, parent = candidates(before_export, scene_vertices, triangles, new_range, sub_levels, sub_nodes)
    if not cands:
        return (REBUILT, 0, 0, 0, 0, 0)
    bits, ident = min(cands)                                    # the 64-bit key (cost bits << 32) | id, as a tuple
    if ident == 0xFFFFFFFF:
        return (ROOT_PAIR, 0, 0, 0, bits, len(cands))
    x, i = ident >> 3, ident & 7
    d, p = 0, int(parent[x])
    while p >= 0:
        d, p = d + 1, int(parent[p])
    if i == 4:
        return (SLOT, x, int(before_export["nodes"][x]["meta"]) & 7, d, bits, len(cands))
    return (PAIR, x, i, d, bits, len(cands))


def report_tuple(pl):
    """The fields of a capi.AppendPlacement that place() returns."""
    return (pl.kind, pl.node, pl.slot, pl.depth, pl.cost_bits, pl.candidates)


def sub_levels(before, after, n_new):
    """Level count of the appended sub-tree's root in `after`: 0 when it is one leaf code (at most four triangles)."""
    return 0 if n_new <= 4 else int(after["nodes"][len(before["nodes"])]["meta"]) >> 3


def check_placed_graft(before, after, n_new, placement):
    """The link rule of a placed graft (kinds 1 and 2; kinds 0 and 3 are append_common.check_graft's): old leaf records byte-equal; old
    nodes off the path byte-equal at the same index; on the path the child lists equal but for the one slot, counts right, levels exact
    on every node; a pair's node N is last and holds (old child, S); S recognised as check_graft recognises it."""
    nb, na = before["nodes"], after["nodes"]
    tb, ta = before["tris"], after["tris"]
    kind, X, slot = int(placement.kind), int(placement.node), int(placement.slot)
    assert kind in (SLOT, PAIR)
    assert len(ta) == len(tb) + n_new and ta[:len(tb)].tobytes() == tb.tobytes()
    assert sorted(ta["tri"][len(tb):].tolist()) == list(range(len(tb), len(tb) + n_new))
    assert after["root"] == before["root"]

    def is_subtree_root(ref):
        if ref >= 0:
            return ref == len(nb)
        code = ~ref
        return code >> 2 == len(tb) and (code & 3) + 1 == n_new

    parent = np.full(len(nb), -1, dtype=np.int64)
    for k in range(len(nb)):
        for i in range(int(nb[k]["meta"]) & 7):
            if nb[k]["child"][i] >= 0:
                parent[int(nb[k]["child"][i])] = k
    path, p = [], X
    while p >= 0:
        path.append(p)
        p = int(parent[p])
    assert path[-1] == before["root"] and len(path) - 1 == placement.depth
    keep = np.ones(len(nb), dtype=bool)
    keep[path] = False
    assert na[:len(nb)][keep].tobytes() == nb[keep].tobytes()
    cnt = int(nb[X]["meta"]) & 7
    for y in path:                                              # child lists and counts
        same = np.ones(4, dtype=bool)
        if y == X:
            same[slot] = False
        assert (na[y]["child"][same] == nb[y]["child"][same]).all()
        assert (int(na[y]["meta"]) & 7) == (int(nb[y]["meta"]) & 7) + (1 if y == X and kind == SLOT else 0)
    if kind == SLOT:
        assert slot == cnt and cnt < 4 and is_subtree_root(int(na[X]["child"][slot]))
    else:
        N = len(na) - 1
        assert slot < cnt and int(na[X]["child"][slot]) == N and N >= len(nb)
        assert (int(na[N]["meta"]) & 7) == 2
        assert int(na[N]["child"][0]) == int(nb[X]["child"][slot]) and is_subtree_root(int(na[N]["child"][1]))
        path = [N] + path
    for y in path:                                              # levels exact: 1 + max over the inner children
        inner = [int(c) for c in na[y]["child"][:int(na[y]["meta"]) & 7] if c >= 0]
        assert (int(na[y]["meta"]) >> 3) == 1 + max([int(na[c]["meta"]) >> 3 for c in inner], default=0)
    assert after["max_stack"] <= MAX_LEVELS


def inner_area_sum(export, pos, triangles):
    """Sum of A(b(Y)) over all inner nodes in float64, from exact boxes."""
    lo, hi, _, _ = exact_boxes(export, np.asarray(pos, dtype=np.float32), triangles)
    d = hi.astype(np.float64) - lo.astype(np.float64)
    return float((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]).sum())
