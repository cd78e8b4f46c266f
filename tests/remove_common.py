"""Shared helpers of the removal tests (test_remove_cpu.py, test_gpu_remove.py): which meshes each scene loses, and the prune rule of
fyprt_remove_meshes restated in plain Python / numpy on two exports of the acceleration structure."""
import numpy as np

INT32_MIN = -(1 << 31)

# hall_small: 12 wall quads (meshes 0-11), 8 columns (12-19), 4 drapes (20-23; 1800 triangles each, more than one compaction chunk of
# 1024), 4 light meshes (24-27).  One call removes a column from the middle, a drape and a light mesh, so the removed ranges begin and end
# inside a chunk, a tile and a wave.  cornell: the tall box (5 faces) and the right wall.  banana: the mesh the test imported first.
LOSES = {"cornell": (5, 4), "hall_small": (15, 21, 25)}

BRANCHES = ("leaf partly emptied", "leaf dropped", "node dropped", "splice onto a leaf code", "splice onto an inner node",
            "chain of splices", "root replaced")


def removed_triangles(sc, mesh_indices):
    """Bool array over the triangles of `sc` (before the edit): True for those of the listed meshes."""
    dead = np.zeros(len(sc.triangles), dtype=bool)
    for m in mesh_indices:
        first, count, _ = sc.meshes[m]
        dead[first:first + count] = True
    return dead


def check_prune(before, after, removed):
    """The prune rule.  `before` / `after`: export_bvh results around one fyprt_remove_meshes; `removed`: bool per old triangle.
    Leaf records: the expected array byte for byte.  Nodes: for every old node the expected new index, child list in the used slots and
    meta; unused slots as a fresh upload exports them; nodes that lost nothing below them byte for byte but for rebased references.
    Returns the set of BRANCHES met."""
    met = set()
    removed = np.asarray(removed, dtype=bool)
    tb, nb, na = before["tris"], before["nodes"], after["nodes"]
    new_tri = (np.cumsum(~removed) - 1).astype(np.uint32)
    dead_rec = removed[tb["tri"]] if len(tb) else np.zeros(0, dtype=bool)
    expect = tb[~dead_rec].copy()
    expect["tri"] = new_tri[expect["tri"]]
    assert after["tris"].tobytes() == expect.tobytes()
    dead_before = np.concatenate([[0], np.cumsum(dead_rec)]).astype(np.int64)

    n = len(nb)
    levels = (nb["meta"].astype(np.int64) >> 3)
    order = np.argsort(levels, kind="stable")
    repl = [None] * n               # None = dead, else an int: old node index (>= 0) or leaf code of the pruned tree (< 0)
    spliced = np.zeros(n, dtype=bool)
    lost = np.zeros(n, dtype=bool)
    child_new = [None] * n
    meta_new = np.zeros(n, dtype=np.int64)

    def resolve(ref):
        """(replacement or None, lost anything below, came through a splice)"""
        if ref >= 0:
            return repl[ref], bool(lost[ref]), bool(spliced[ref])
        code = ~ref
        first, m = code >> 2, (code & 3) + 1
        d0 = int(dead_before[first]); dead = int(dead_before[first + m]) - d0
        if dead == m:
            met.add(BRANCHES[1])
            return None, True, False
        if dead:
            met.add(BRANCHES[0])
        return ~(((first - d0) << 2) | (m - dead - 1)), dead > 0, False

    new_level = {}
    for i in order:
        i = int(i)
        kept, lev, via_splice = [], 0, False
        for s in range(int(nb[i]["meta"]) & 7):
            r, l, sp = resolve(int(nb[i]["child"][s]))
            lost[i] |= l
            if r is None:
                continue
            if r >= 0:
                lev = max(lev, new_level[r])
            kept.append(r)
            via_splice = sp
        if len(kept) == 0:
            met.add(BRANCHES[2]); repl[i] = None
        elif len(kept) == 1:
            repl[i] = kept[0]; spliced[i] = True
            met.add(BRANCHES[3] if kept[0] < 0 else BRANCHES[4])
            if via_splice:
                met.add(BRANCHES[5])
        else:
            repl[i] = i; child_new[i] = kept; new_level[i] = lev + 1; meta_new[i] = len(kept) | ((lev + 1) << 3)

    alive = np.array([repl[i] == i for i in range(n)], dtype=bool)
    new_index = (np.cumsum(alive) - 1).astype(np.int64)
    assert len(na) == int(alive.sum())
    for i in np.nonzero(alive)[0]:
        i = int(i)
        got, k = na[new_index[i]], len(child_new[i])
        want = [int(new_index[c]) if c >= 0 else c for c in child_new[i]]
        assert got["child"][:k].tolist() == want, (i, got["child"], want)
        assert int(got["meta"]) == meta_new[i], i
        assert (got["child"][k:] == INT32_MIN).all() and (got["qlo"][:, k:] == 255).all() and (got["qhi"][:, k:] == 0).all(), i
        if not lost[i]:
            same = nb[i:i + 1].copy()
            same["child"][0, :k] = want
            assert got.tobytes() == same.tobytes(), i
    if len(tb) == 0:
        root, depth = 0, 0                                           # the tree of a scene without triangles stays that
    else:
        r, _, _ = resolve(int(before["root"]))
        if before["root"] >= 0 and r != before["root"]:
            met.add(BRANCHES[6])
        root, depth = (0, 0) if r is None else (r, 0) if r < 0 else (int(new_index[r]), new_level[r])
    assert after["root"] == root and after["max_stack"] == depth, (after["root"], root, after["max_stack"], depth)
    return met
