"""Shared helpers of the partial-refit tests (test_partial_refit_cpu.py, test_gpu_partial_refit.py): the dirty rule of the partial refit
(fyprt_update_mesh_vertices, fyprt_update_transforms with tuning key 22 = 1) restated in plain Python on an export of the
acceleration structure, and the moves the tests make."""
import numpy as np

# two meshes per scene: a large and a small one whose ways to the root share ancestors (hall_small / cornell: the moves of
# test_gpu_transforms.py; banana: the move of test_gpu_refit.py and one of the two light quads)
MOVES = {"hall_small": [(3, dict(pos=(0.7, 0.0, -0.4), rotation=(0, 25, 0))), (-1, dict(pos=(0.0, -0.3, 0.2), rotation=(10, 0, 5)))],
         "cornell": [(5, dict(pos=(0.2, 0.0, 0.1), rotation=(0, 30, 0))), (7, dict(pos=(0.15, 0.0, -0.1), scale_=(1.1, 0.8, 1.0)))],
         "banana": [(0, dict(pos=(0.3, -3.0, 0.2), rotation=(90, 40, 10), scale_=(1.2, 0.9, 1.0))), (-1, dict(pos=(0.1, 0.05, -0.1)))]}


def mesh_triangles(sc, mesh_indices):
    """The triangle indices of the listed meshes of `sc`, each once."""
    ids = set()
    for m in mesh_indices:
        first, count, _ = sc.meshes[m]
        ids.update(range(first, first + count))
    return sorted(ids)


def node_parents(bvh):
    """parent[i] of every node of an export (-1 for the root), and per node the (first, count) ranges of its leaf-code children."""
    nodes = bvh["nodes"]
    parent = np.full(len(nodes), -1, dtype=np.int64)
    leaves = [[] for _ in range(len(nodes))]
    for i in range(len(nodes)):
        for s in range(int(nodes[i]["meta"]) & 7):
            c = int(nodes[i]["child"][s])
            if c >= 0:
                assert parent[c] == -1 and c != bvh["root"]
                parent[c] = i
            else:
                leaves[i].append(((~c) >> 2, ((~c) & 3) + 1))
    return parent, leaves


def expected_dirty_nodes(bvh, tri_ids):
    """The nodes a partial refit of the triangles `tri_ids` rewrites: the records whose triangle is in the set, the nodes holding those
    records in a leaf-code child, and all their ancestors."""
    tris = bvh["tris"]
    moved = np.zeros(int(tris["tri"].max()) + 1 if len(tris) else 0, dtype=bool)
    ids = np.asarray(sorted(set(int(t) for t in tri_ids)), dtype=np.int64)
    moved[ids[ids < len(moved)]] = True
    rec = moved[tris["tri"]] if len(tris) else np.zeros(0, dtype=bool)
    parent, leaves = node_parents(bvh)
    dirty = set()
    for i, ranges in enumerate(leaves):
        if any(rec[first:first + count].any() for first, count in ranges):
            k = i
            while k >= 0 and k not in dirty:
                dirty.add(k)
                k = int(parent[k])
    return dirty
