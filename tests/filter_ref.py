"""Reference of the query filter (fyprt_set_mesh_query_masks / fyprt_set_query_mask): which exported leaf records a mask table M and
a query mask Q admit, the exported tree reduced to them — on which the existing brute-force references (bruteforce, multihit_ref,
points_ref, boxes_ref) run unchanged — and the OR of the leaf masks below every exported node, computed level by level from the node
array (node_masks) or, independently, from the sets of records below every node (node_masks_by_sets).
A helper of the query filter tests, not a test file."""
import numpy as np


def mesh_of_triangle(meshes, n_triangles):
    """The mesh index of every triangle, from (firstTriangle, triangleCount, ...) per mesh: the meshes partition the triangle list."""
    out = np.full(n_triangles, -1, dtype=np.int64)
    for m, me in enumerate(meshes):
        out[int(me[0]):int(me[0]) + int(me[1])] = m
    assert (out >= 0).all()
    return out


def leaf_masks(bvh, meshes, M):
    """M[mesh of the record's triangle] per exported leaf record, uint32."""
    M = np.asarray(M, dtype=np.uint32)
    assert len(M) == len(meshes)
    ids = bvh["tris"]["tri"].astype(np.int64)
    n_tri = max(int(ids.max(initial=-1)) + 1, max((int(me[0]) + int(me[1]) for me in meshes), default=0))
    return M[mesh_of_triangle(meshes, n_tri)[ids]] if len(ids) else np.zeros(0, dtype=np.uint32)


def admitted(bvh, meshes, M, Q):
    """A bool per exported leaf record: (M[mesh] & Q) != 0."""
    return (leaf_masks(bvh, meshes, M) & np.uint32(Q)) != 0


def filtered(bvh, meshes, M, Q):
    """The exported tree with the admitted leaf records only (nodes and root are dropped: the references read the records alone)."""
    return {"tris": bvh["tris"][admitted(bvh, meshes, M, Q)], "nodes": bvh["nodes"][:0], "root": None}


def node_masks(bvh, leaf_mask):
    """The OR of `leaf_mask` over everything below every exported node, uint32 per node: children before parents by the nodes' level
    (meta >> 3), as the device builds it."""
    nodes = bvh["nodes"]
    out = np.zeros(len(nodes), dtype=np.uint32)
    done = np.zeros(len(nodes), dtype=bool)
    for i in np.argsort(nodes["meta"].astype(np.int64) >> 3, kind="stable"):
        word = np.uint32(0)
        for c in range(int(nodes[i]["meta"]) & 7):
            ref = int(nodes[i]["child"][c])
            if ref >= 0:
                assert done[ref], "a child's level is below its parent's"
                word |= out[ref]
            else:
                code = ~ref
                for r in range(code >> 2, (code >> 2) + (code & 3) + 1):
                    word |= leaf_mask[r]
        out[i], done[i] = word, True
    return out


def node_masks_by_sets(bvh, leaf_mask):
    """The same words from the set of leaf records below every node (points_ref.leaf_records_below); nodes the root does not reach get 0
    and a False in the second result."""
    from points_ref import leaf_records_below
    below = leaf_records_below(bvh) if len(bvh["nodes"]) and bvh["root"] >= 0 else []
    out = np.zeros(len(bvh["nodes"]), dtype=np.uint32)
    reached = np.zeros(len(bvh["nodes"]), dtype=bool)
    for i, slots in enumerate(below):
        if slots is None:
            continue
        reached[i] = True
        for recs in slots:
            out[i] |= np.bitwise_or.reduce(leaf_mask[recs].astype(np.uint32), initial=np.uint32(0))
    return out, reached


def renumbering(meshes, kept):
    """Old triangle index -> new index after the meshes NOT in `kept` (a bool per mesh) are removed, -1 for removed triangles."""
    n_tri = sum(int(me[1]) for me in meshes)
    keep_tri = np.asarray(kept, bool)[mesh_of_triangle(meshes, n_tri)]
    new = np.full(n_tri, -1, dtype=np.int64)
    new[keep_tri] = np.arange(int(keep_tri.sum()))
    return new
