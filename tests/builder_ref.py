"""The device builders (rt_lbvh.h, build_device_lbvh in fyprt.hip) and the refit rule (rt_refit.h: refit_node) restated in numpy and
plain Python: binary32 where the device uses binary32, double where it uses double, the device's operation order (-ffp-contract=off
holds for every kernel, so each product and sum below is one rounding, as there).  Everything here is a deterministic function of
the triangle positions, so a test compares it with an exported tree EXACTLY: sort key, sorted order, radix / PLOC tree, collapse,
level counts and the bytes of the quantisation.  What is not pinned: the numbers of the wide nodes within a BFS level and of PLOC's
binary nodes (both come from atomic counters); `canonical` removes them.  Not a test file."""
import math

import numpy as np

F = np.float32
LEAF = 0x80000000                   # kRadixLeaf: bit 31 of a binary-tree reference marks a leaf (sorted position in the low bits)
LEAF_LIMIT = 4                      # kLbvhLeaf
STACK_BUDGET = 31                   # rth::kStackBudget: more wide levels and the driver falls back to the host builder
PLOC_BLOCK, PLOC_MAX_RADIUS, PLOC_FORCE_ABOVE = 256, 32, 4096


# ------------------------------------------------------------------------------------------------ k_lbvh_keys
def _expand_bits21(v):
    v = v.astype(np.uint64) & np.uint64(0x1FFFFF)
    for shift, mask in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v


def grid_of(positions):
    """The Morton grid the driver derives from the vertices it is handed: their box."""
    p = np.asarray(positions, dtype=F).reshape(-1, 3)
    return p.min(axis=0), p.max(axis=0)


def morton_cells(tri_pos, grid_lo, grid_hi):
    """The three 21-bit cell coordinates of every triangle's centroid, (n, 3) uint64."""
    p = np.asarray(tri_pos, dtype=F).reshape(-1, 3, 3)
    lo, hi = np.asarray(grid_lo, dtype=F), np.asarray(grid_hi, dtype=F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(hi > lo, F(1.0) / (hi - lo), F(0.0)).astype(F)
    third = F(1.0) / F(3.0)
    c = (((p[:, 0] + p[:, 1]) + p[:, 2]) * third - lo) * inv
    v = c * F(2097152.0)
    v = np.where(v < F(0.0), F(0.0), np.where(v > F(2097151.0), F(2097151.0), v))
    return np.where(np.isnan(v), F(0.0), v).astype(np.uint64)       # the conversion truncates


def morton_keys(tri_pos, grid_lo, grid_hi):
    """k_lbvh_keys: the 63-bit sort key of every triangle, x << 2 | y << 1 | z over the expanded cell coordinates."""
    q = morton_cells(tri_pos, grid_lo, grid_hi)
    return (_expand_bits21(q[:, 0]) << np.uint64(2)) | (_expand_bits21(q[:, 1]) << np.uint64(1)) | _expand_bits21(q[:, 2])


def sorted_order(keys):
    """The device sort is a stable radix sort over all 63 bits: position -> index into the builder's triangle range."""
    return np.argsort(keys, kind="stable")


def leaf_boxes(tri_pos):
    """(n, 6) binary32: lo.xyz, hi.xyz of every triangle (exact)."""
    p = np.asarray(tri_pos, dtype=F).reshape(-1, 3, 3)
    return np.concatenate([p.min(axis=1), p.max(axis=1)], axis=1)


# ------------------------------------------------------------------------------------------------ binary trees
class BinaryTree:
    """The builders' common binary-tree format: per internal node its two children (references: LEAF | sorted position, or an
    internal node's number) and the number of leaves below it; `root` is a reference."""

    def __init__(self, n_leaves):
        self.n_leaves, self.left, self.right, self.span, self.root = n_leaves, [], [], [], 0

    def span_of(self, ref):
        return 1 if ref & LEAF else self.span[ref]

    def nested(self):
        """Nested tuples of sorted positions (node numbers removed), for comparisons between binary trees."""
        out = {}
        stack = [(self.root, False)]
        while stack:
            ref, done = stack.pop()
            if ref & LEAF:
                out[ref] = ref & ~LEAF
            elif done:
                out[ref] = (out[self.left[ref]], out[self.right[ref]])
            else:
                stack += [(ref, True), (self.left[ref], False), (self.right[ref], False)]
        return out[self.root]


def node_boxes(tree, leaf_box):
    """Boxes of the internal nodes, (m, 6) binary32: the union of the children's (min / max: exact in any order)."""
    box = np.zeros((len(tree.left), 6), dtype=F)
    stack = [(tree.root, False)]
    get = lambda r: leaf_box[r & ~LEAF] if r & LEAF else box[r]
    while stack:
        ref, done = stack.pop()
        if ref & LEAF:
            continue
        if not done:
            stack += [(ref, True), (tree.left[ref], False), (tree.right[ref], False)]
            continue
        a, b = get(tree.left[ref]), get(tree.right[ref])
        box[ref, :3], box[ref, 3:] = np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])
    return box


def _clz(x, bits):
    return bits - int(x).bit_length()


def radix_tree(keys):
    """k_lbvh_radix (Karras 2012) over the sorted keys: internal node i covers a range that begins or ends at position i; node 0 is
    the root.  delta = length of the common prefix of two 64-bit keys; equal keys: 64 + clz32(i ^ j); out of range: -1."""
    k = [int(v) for v in keys]
    n = len(k)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        x = k[i] ^ k[j]
        return _clz(x, 64) if x else 64 + _clz(i ^ j, 32)

    t = BinaryTree(n)
    t.first, t.last = [], []
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, s = 0, lmax // 2
        while s >= 1:
            if delta(i, i + (l + s) * d) > dmin:
                l += s
            s //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, s2 = 0, l
        while True:
            s2 = (s2 + 1) >> 1
            if delta(i, i + (s + s2) * d) > dnode:
                s += s2
            if s2 <= 1:
                break
        gamma = i + s * d + (d if d < 0 else 0)
        lo, hi = min(i, j), max(i, j)
        t.left.append(LEAF | gamma if lo == gamma else gamma)
        t.right.append(LEAF | (gamma + 1) if hi == gamma + 1 else gamma + 1)
        t.first.append(lo); t.last.append(hi); t.span.append(hi - lo + 1)
    t.root = 0
    return t


# ------------------------------------------------------------------------------------------------ PLOC
def _area_f32(box):
    """lbvh_area / the PLOC cost: dx * dy + dy * dz + dz * dx in binary32, left to right."""
    dx, dy, dz = box[..., 3] - box[..., 0], box[..., 4] - box[..., 1], box[..., 5] - box[..., 2]
    return (dx * dy + dy * dz) + dz * dx


def ploc_nearest(box, radius):
    """k_ploc_nearest without force for one cluster list, box = (n, 6) binary32 in list order.  Returns (nearest, stats): the chosen
    position per cluster — the smallest cost within `radius` positions; ties: the partner i ^ 1 (i - 1 for an unpaired last), then
    the lowest position — and how many choices went to another 256-block, were ties kept by the partner against a LOWER position
    (what a search that began at the window's start would have taken), or ties among non-partners (lowest taken)."""
    n = len(box)
    i = np.arange(n)
    partner = np.where((i ^ 1) < n, i ^ 1, i - 1)
    cost = np.full((n, 2 * radius + 1), np.inf, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(-radius, radius + 1):
            if d == 0:
                continue
            a, b = max(0, -d), min(n, n - d)                   # clusters [a, b) have position i + d inside the list
            if a >= b:
                continue
            me, o = box[a:b], box[a + d:b + d]
            u = np.concatenate([np.minimum(me[:, :3], o[:, :3]), np.maximum(me[:, 3:], o[:, 3:])], axis=1)
            c = _area_f32(u)
            cost[a:b, d + radius] = np.where(np.isnan(c), np.inf, c)      # `cg < bestCost` is false for NaN: never wins
    m = cost.min(axis=1)
    pcost = cost[i, partner - i + radius]
    lowest = cost.argmin(axis=1) - radius + i                  # argmin: the first = the lowest position
    keep_partner = ~(m < pcost)
    nearest = np.where(keep_partner, partner, lowest)
    at_min = cost == m[:, None]
    ties = at_min.sum(axis=1)
    stats = {"cross_block": int(((nearest // PLOC_BLOCK) != (i // PLOC_BLOCK)).sum()),
             "tie_to_partner": int((keep_partner & (pcost == m) & (lowest < partner) & np.isfinite(m)).sum()),
             "tie_to_lowest": int((~keep_partner & (ties >= 2)).sum())}
    return nearest, stats


def ploc_tree(boxes, radius=16, force_rule=True):
    """build_device_lbvh's PLOC rounds over the leaf boxes in sorted order: k_ploc_nearest, k_ploc_merge (mutual choices merge into
    a new node at the lower position), the order-keeping compaction, and the host's force rule (a round over more than 4096
    clusters that kept more than n - n / 16 of them is followed by one in which everybody takes its partner).
    Returns (tree, node_box, rounds, forced_rounds, stats); node numbers are this function's own (the device's come from an atomic)."""
    radius = min(PLOC_MAX_RADIUS, max(1, int(radius)))
    leaf = np.asarray(boxes, dtype=F)
    n_leaves = len(leaf)
    t = BinaryTree(n_leaves)
    node_box = []
    clusters = [LEAF | j for j in range(n_leaves)]
    cbox = leaf.copy()
    rounds, forced, force = 0, [], False
    stats = {"cross_block": 0, "tie_to_partner": 0, "tie_to_lowest": 0}
    while len(clusters) > 1:
        n = len(clusters)
        if force:
            i = np.arange(n)
            nearest = np.where((i ^ 1) < n, i ^ 1, i - 1)
            forced.append(rounds)
        else:
            nearest, st = ploc_nearest(cbox, radius)
            for k in stats:
                stats[k] += st[k]
        nxt, nbox = [], []
        for i in range(n):
            j = int(nearest[i])
            if int(nearest[j]) != i:
                nxt.append(clusters[i]); nbox.append(cbox[i]); continue
            if i > j:
                continue
            k = len(t.left)
            t.left.append(clusters[i]); t.right.append(clusters[j]); t.span.append(t.span_of(clusters[i]) + t.span_of(clusters[j]))
            b = np.concatenate([np.minimum(cbox[i, :3], cbox[j, :3]), np.maximum(cbox[i, 3:], cbox[j, 3:])])
            node_box.append(b)
            nxt.append(k); nbox.append(b)
        kept = len(nxt)
        assert 0 < kept < n, "PLOC round made no progress"
        force = bool(force_rule and not force and n > PLOC_FORCE_ABOVE and kept > n - n // 16)
        clusters, cbox = nxt, np.array(nbox, dtype=F)
        rounds += 1
    t.root = clusters[0]
    return t, np.array(node_box, dtype=F).reshape(-1, 6), rounds, forced, stats


# ------------------------------------------------------------------------------------------------ k_lbvh_collapse
def collapse(tree, node_box):
    """The BFS collapse into 4-wide nodes.  A wide node starts from a binary node's two children; loop 1 opens the inner child of
    largest area among those of more than 4 triangles, loop 2 splits the would-be leaf (an internal node of at most 4 triangles) of
    largest area; `>` keeps the first of equal areas; the two children take the opened child's place.  A child of at most 4
    triangles becomes a leaf whose records are its triangles left to right; leaf records are laid in slot order, left subtree first.
    Returns a dict: `leaf_positions` (sorted position per leaf record), `tree` (canonical form: per node the tuple of its children
    in slot order, each ("leaf", first, count) or a node), `level_counts` (wide nodes per BFS level), `too_deep` (more than 31
    levels: the driver falls back to the host builder) and `stats` (how often each loop fired, and fired on a tie of equal areas)."""
    area = _area_f32(node_box) if len(node_box) else np.zeros(0, dtype=F)
    left, right, span_of = tree.left, tree.right, tree.span_of
    stats = {"loop1": 0, "loop2": 0, "tie1": 0, "tie2": 0}

    def pick(ch, want_large):
        best, best_area, ties = -1, F(-1.0), 0
        for i, c in enumerate(ch):
            if c & LEAF:
                continue
            if (span_of(c) > LEAF_LIMIT) != want_large:
                continue
            a = area[c]
            if a > best_area:
                best, best_area, ties = i, a, 1
            elif a == best_area:
                ties += 1
        return best, ties

    leaf_positions = np.full(tree.n_leaves, -1, dtype=np.int64)
    nodes, level_counts = [None], []
    cur = [(tree.root, 0, 0)]                                  # binary node, position of its first leaf record, wide node
    while cur:
        level_counts.append(len(cur))
        nxt = []
        for b, first, me in cur:
            ch = [left[b], right[b]]
            for loop, want_large in (("1", True), ("2", False)):
                while len(ch) < 4:
                    best, ties = pick(ch, want_large)
                    if best < 0:
                        break
                    stats["loop" + loop] += 1
                    stats["tie" + loop] += 1 if ties > 1 else 0
                    ch[best:best + 1] = [left[ch[best]], right[ch[best]]]
            kids = []
            for c in ch:
                sp = span_of(c)
                if sp <= LEAF_LIMIT:
                    kids.append(("leaf", first, sp))
                    stack, pos = [c], first
                    while stack:
                        r = stack.pop()
                        if r & LEAF:
                            leaf_positions[pos] = r & ~LEAF; pos += 1
                        else:
                            stack += [right[r], left[r]]
                else:
                    nodes.append(None)
                    kids.append(("node", len(nodes) - 1))
                    nxt.append((c, first, len(nodes) - 1))
                first += sp
            nodes[me] = kids
        cur = nxt
    for k in range(len(nodes) - 1, -1, -1):                    # children have larger numbers: bottom-up, no recursion
        nodes[k] = tuple(c if c[0] == "leaf" else nodes[c[1]] for c in nodes[k])
    assert (leaf_positions >= 0).all()
    return {"leaf_positions": leaf_positions, "tree": nodes[0], "level_counts": level_counts, "too_deep": len(level_counts) > STACK_BUDGET, "stats": stats}


def build_ref(tri_pos, grid_positions, builder, radius=16, force_rule=True):
    """The whole device build of the triangles `tri_pos` (n, 3, 3) over the Morton grid of `grid_positions`: builder 1 = radix tree,
    2 = PLOC.  Returns collapse()'s dict plus `keys`, `order`, `leaf_tris` (index into tri_pos per leaf record), `binary` and, for
    PLOC, `rounds`, `forced` and `ploc_stats`."""
    lo, hi = grid_of(grid_positions)
    keys = morton_keys(tri_pos, lo, hi)
    order = sorted_order(keys)
    lb = leaf_boxes(tri_pos)[order]
    extra = {}
    if builder == 1:
        bt = radix_tree(keys[order])
        nb = node_boxes(bt, lb)
    else:
        bt, nb, rounds, forced, st = ploc_tree(lb, radius, force_rule)
        extra = {"rounds": rounds, "forced": forced, "ploc_stats": st}
    out = collapse(bt, nb)
    out.update(extra, keys=keys, order=order, binary=bt, leaf_tris=order[out["leaf_positions"]])
    return out


# ------------------------------------------------------------------------------------------------ exported trees
def is_leaf(child):
    return child[0] == "leaf"


def canonical(export, root=None, leaf_base=0):
    """The canonical form of an exported tree (Context.export_bvh) from `root` on (default: the export's root): node numbers
    removed, slot order, leaf positions (relative to leaf record `leaf_base`) and shape kept.  A leaf-code root gives that leaf."""
    nodes = export["nodes"]

    def leaf(ref):
        code = ~ref
        return ("leaf", (code >> 2) - leaf_base, (code & 3) + 1)

    root = export["root"] if root is None else root
    if root < 0:
        return leaf(root)
    out, stack = {}, [(int(root), False)]
    while stack:
        idx, done = stack.pop()
        n = nodes[idx]
        kids = [int(c) for c in n["child"][:int(n["meta"]) & 7]]
        if done:
            out[idx] = tuple(leaf(c) if c < 0 else out[c] for c in kids)
        else:
            stack.append((idx, True))
            stack += [(c, False) for c in kids if c >= 0]
    return out[int(root)]


def walk_export(export, root=None):
    """(path, node index) of every node below `root`, parents first; a path is the tuple of slot numbers from the root."""
    nodes = export["nodes"]
    root = export["root"] if root is None else root
    stack = [((), int(root))] if root >= 0 else []
    while stack:
        path, idx = stack.pop()
        yield path, idx
        n = nodes[idx]
        for s in range((int(n["meta"]) & 7) - 1, -1, -1):
            if int(n["child"][s]) >= 0:
                stack.append((path + (s,), int(n["child"][s])))


def first_tree_difference(a, b):
    """None when two canonical trees are equal, else (path, a's entry, b's entry) at the first difference, parents first."""
    stack = [((), a, b)]
    while stack:
        path, x, y = stack.pop()
        if is_leaf(x) or is_leaf(y):
            if x != y:
                return path, (x if is_leaf(x) else "node of %d" % len(x)), (y if is_leaf(y) else "node of %d" % len(y))
            continue
        if len(x) != len(y):
            return path, "node of %d" % len(x), "node of %d" % len(y)
        for s in range(len(x) - 1, -1, -1):
            stack.append((path + (s,), x[s], y[s]))
    return None


def levels_by_path(tree):
    """path -> wide levels of the node there (1 = all children are leaves) of a canonical tree, capped at 31 as the meta byte is."""
    todo, order = [((), tree)], []
    while todo:
        path, node = todo.pop()
        order.append((path, node))
        todo += [(path + (s,), c) for s, c in enumerate(node) if not is_leaf(c)]
    out = {}
    for path, node in reversed(order):
        out[path] = min(31, 1 + max([out[path + (s,)] for s, c in enumerate(node) if not is_leaf(c)], default=0))
    return out


def child_counts(tree):
    """How many nodes of a canonical tree have 2, 3 and 4 children."""
    out, todo = {2: 0, 3: 0, 4: 0}, [tree]
    while todo:
        node = todo.pop()
        out[len(node)] += 1
        todo += [c for c in node if not is_leaf(c)]
    return out


NODE_DTYPE = np.dtype([("origin", "<f4", 3), ("ex", "u1", 3), ("meta", "u1"), ("child", "<i4", 4), ("qlo", "u1", (3, 4)), ("qhi", "u1", (3, 4))])


def export_from_canonical(tree, leaf_tris):
    """A canonical tree in the shape of an export (nodes numbered in BFS order, topology and level counts only), so that the
    functions below serve the reference's own trees as well."""
    levels = levels_by_path(tree)
    queue, recs = [((), tree)], []
    while queue:
        nxt = []
        for path, node in queue:
            recs.append((path, node))
            nxt += [(path + (s,), c) for s, c in enumerate(node) if not is_leaf(c)]
        queue = nxt
    number = {path: k for k, (path, _) in enumerate(recs)}
    nodes = np.zeros(len(recs), dtype=NODE_DTYPE)
    for k, (path, node) in enumerate(recs):
        nodes[k]["meta"] = len(node) | (levels[path] << 3)
        nodes[k]["child"] = [(~((c[1] << 2) | (c[2] - 1)) if is_leaf(c) else number[path + (s,)]) for s, c in enumerate(node)] + [-2 ** 31] * (4 - len(node))
    return {"nodes": nodes, "tris": {"tri": np.asarray(leaf_tris)}, "root": 0}


def exact_child_boxes(export, tri_lo, tri_hi, root=None):
    """node index -> (lo, hi), each (count, 3) binary32: the exact boxes of the node's children, a leaf's from the triangles of its
    leaf records (tri_lo / tri_hi: per triangle id), an inner child's the union of its own children's — refit_child_boxes."""
    nodes, tri = export["nodes"], export["tris"]["tri"]
    order = list(walk_export(export, root))
    own, out = {}, {}
    for _, idx in reversed(order):
        n = nodes[idx]
        lo, hi = [], []
        for s in range(int(n["meta"]) & 7):
            c = int(n["child"][s])
            if c >= 0:
                l, h = own[c]
            else:
                code = ~c
                ids = tri[(code >> 2):(code >> 2) + (code & 3) + 1]
                l, h = tri_lo[ids].min(axis=0), tri_hi[ids].max(axis=0)
            lo.append(l); hi.append(h)
        out[idx] = (np.array(lo, dtype=F), np.array(hi, dtype=F))
        own[idx] = (out[idx][0].min(axis=0), out[idx][1].max(axis=0))
    return out


# ------------------------------------------------------------------------------------------------ refit_node's quantisation
def _plane(q, sf, lo):
    """fmaf((float)q, sf, lo): q <= 255 times a power of two is exact in binary32, so one rounding remains, that of the sum."""
    with np.errstate(over="ignore", invalid="ignore"):
        return F(F(q) * sf) + lo


def quantise_axis_at(e, lo, ext, child_lo, child_hi):
    """One attempt of refit_node's exponent loop on one axis: step 2^(e - 127), node origin `lo` (binary32), node extent `ext`
    (double), the children's bounds on the axis (binary32).  Returns (ok, qlo, qhi, moved_lo, moved_hi): whether the step holds,
    the 4 + 4 plane bytes as the loop leaves them (slots after a failure and unused slots: 255 / 0), and how many steps each
    correction loop moved a plane."""
    s = math.ldexp(1.0, e - 127)
    sf = F(s)
    ok = ext <= 254.0 * s
    qlo, qhi, moved_lo, moved_hi = [255] * 4, [0] * 4, 0, 0
    for i in range(len(child_lo)):
        if not ok:
            break
        cl, ch = child_lo[i], child_hi[i]
        ql = int(math.floor((float(cl) - float(lo)) / s - 0.0625))
        qh = int(math.ceil((float(ch) - float(lo)) / s + 0.0625))
        ql, qh = min(255, max(0, ql)), min(255, max(0, qh))
        while ql > 0 and not (_plane(ql, sf, lo) <= cl):
            ql -= 1; moved_lo += 1
        while qh < 255 and not (_plane(qh, sf, lo) >= ch):
            qh += 1; moved_hi += 1
        ok = bool(_plane(ql, sf, lo) <= cl and _plane(qh, sf, lo) >= ch)
        qlo[i], qhi[i] = ql, qh
    return ok, qlo, qhi, moved_lo, moved_hi


def start_exponent(ext):
    """The smallest biased exponent e with 2^(e - 127) >= ext / 254, clamped to 1..254 (1 for an axis without extent): frexp gives
    ext / 254 = m * 2^ee with m in [0.5, 1), so 2^ee is the next power of two above, unless m == 0.5, when 2^(ee - 1) is it."""
    if not ext > 0.0:
        return 1
    m, ee = math.frexp(ext / 254.0)
    if m == 0.5:
        ee -= 1
    return min(254, max(1, ee + 127))


def extent_is_254_steps(ext):
    """The `m == 0.5` case: the extent is exactly 254 steps of a power of two."""
    return ext > 0.0 and math.frexp(ext / 254.0)[0] == 0.5


def quantise_ref(child_lo, child_hi):
    """refit_node's rule for one node from the exact boxes of its children, (count, 3) binary32 each: origin = the node's own lower
    corner; per axis the exponent starts at start_exponent(extent in double) and is raised until every child's planes hold: lo plane
    = floor(offset / step - 1/16), hi plane = ceil(offset / step + 1/16) in double, clamped to a byte, moved down / up while the
    binary32 plane origin + q * step does not contain the child, and checked once more; it stops at 254 whatever the outcome.
    Returns a dict: origin (3,), ex (3,), qlo and qhi (3, 4) uint8, `raised` (exponent steps above the start value, per axis),
    `moved_lo` / `moved_hi` (correction-loop steps in the attempt that was kept), `exact_254` (axes whose extent is exactly 254 steps)."""
    child_lo, child_hi = np.asarray(child_lo, dtype=F).reshape(-1, 3), np.asarray(child_hi, dtype=F).reshape(-1, 3)
    origin, top = child_lo.min(axis=0), child_hi.max(axis=0)
    out = {"origin": origin, "ex": np.zeros(3, np.uint8), "qlo": np.zeros((3, 4), np.uint8), "qhi": np.zeros((3, 4), np.uint8),
           "raised": [0, 0, 0], "moved_lo": 0, "moved_hi": 0, "exact_254": 0}
    for a in range(3):
        lo = origin[a]
        ext = float(top[a]) - float(lo)
        e0 = e = start_exponent(ext)
        while True:
            ok, qlo, qhi, ml, mh = quantise_axis_at(e, lo, ext, child_lo[:, a], child_hi[:, a])
            if ok or e >= 254:
                break
            e += 1
        out["ex"][a], out["qlo"][a], out["qhi"][a] = e, qlo, qhi
        out["raised"][a] = e - e0
        out["moved_lo"] += ml; out["moved_hi"] += mh
        out["exact_254"] += 1 if extent_is_254_steps(ext) else 0
    return out


def quantisation_differences(export, tri_lo, tri_hi, root=None, stats=None):
    """Every node below `root` against quantise_ref of its exact child boxes: a list of (path, field, exported, reference) for
    origin, ex, qlo and qhi, parents first.  `stats` (a dict) collects the reference's counters over the nodes seen."""
    nodes = export["nodes"]
    boxes = exact_child_boxes(export, tri_lo, tri_hi, root)
    bad = []
    for path, idx in walk_export(export, root):
        ref = quantise_ref(*boxes[idx])
        n = nodes[idx]
        for field in ("origin", "ex", "qlo", "qhi"):
            if n[field].tobytes() != ref[field].tobytes():
                bad.append((path, field, n[field].tolist(), ref[field].tolist()))
        if stats is not None:
            stats["nodes"] = stats.get("nodes", 0) + 1
            stats["raised"] = stats.get("raised", 0) + sum(1 for r in ref["raised"] if r > 0)
            stats["moved_lo"] = stats.get("moved_lo", 0) + ref["moved_lo"]
            stats["moved_hi"] = stats.get("moved_hi", 0) + ref["moved_hi"]
            stats["exact_254"] = stats.get("exact_254", 0) + ref["exact_254"]
    return bad
