"""Shared helpers of the regraft tests (test_regraft_cpu.py, test_gpu_regraft.py): fyprt_tree_cost restated in numpy on an export, and
the twin of fyprt_regraft_meshes — a second context that removes the listed meshes in one fyprt_remove_meshes and appends them again one
call each in the listed order — with the comparison the header promises: nodes64 byte for byte, tris48 in every byte but triangleIndex,
which maps through the twin's renumbering, and each report equal to the twin's fyprt_last_append_placement."""
import copy
import math

import numpy as np

import placement_ref as pr
from append_common import check_graft
from common import check_bvh_invariants
from remove_common import check_prune, removed_triangles

# fyprt_tree_cost, device against host-only against numpy: the three add the same non-negative binary64 terms in different orders.  At
# most 2^26 terms (2^24 nodes, four children each); any summation order is within (n - 1) * 2^-53 <= 2^-27 relative of the exact sum, so
# two orders differ by at most 2^-26 relative.
COST_RTOL = 2.0 ** -26

PLACEMENT_FIELDS = ("mode", "kind", "node", "slot", "depth", "cost_bits", "levels_before", "levels_after", "candidates")


def placement_tuple(pl):
    return tuple(int(getattr(pl, f)) for f in PLACEMENT_FIELDS)


def tree_cost_ref(export, sc):
    """fyprt_tree_cost of the header from an export and the scene's vertices: A in binary32 (placement_ref.area), every term converted
    to binary64, the sums exact (math.fsum).  Returns (root_area, inner_area, leaf_area, nodes, leaf_children, leaf_records, levels)."""
    nodes, tris = export["nodes"], export["tris"]
    if len(tris) == 0:
        return (0.0, 0.0, 0.0, 0, 0, 0, 0)
    pos = np.asarray(sc.world_vertices["position"], dtype=np.float32)
    lo, hi, _, leaf_box = pr.exact_boxes(export, pos, sc.triangles)
    root = int(export["root"])
    if root < 0:
        a = float(pr.area(*leaf_box(root)))
        return (a, 0.0, ((~root & 3) + 1) * a, 0, 1, len(tris), 0)
    inner = [float(pr.area(lo[y], hi[y])) for y in range(len(nodes))]
    leaf = []
    for y in range(len(nodes)):
        for i in range(int(nodes[y]["meta"]) & 7):
            c = int(nodes[y]["child"][i])
            if c < 0:
                leaf.append(((~c & 3) + 1) * float(pr.area(*leaf_box(c))))
    return (inner[root], math.fsum(inner), math.fsum(leaf), len(nodes), len(leaf), len(tris), int(export["max_stack"]))


def cost_tuple(c):
    return (c.root_area, c.inner_area, c.leaf_area, c.nodes, c.leaf_children, c.leaf_records, c.levels)


def assert_cost_close(got, want):
    """Two cost tuples: the doubles within COST_RTOL relative, the four counts exact."""
    for g, w in zip(got[:3], want[:3]):
        assert abs(g - w) <= COST_RTOL * max(abs(g), abs(w)), (got, want)
    assert tuple(got[3:]) == tuple(want[3:]), (got, want)


def same_export(a, b):
    return a["nodes"].tobytes() == b["nodes"].tobytes() and a["tris"].tobytes() == b["tris"].tobytes() and a["root"] == b["root"] and a["max_stack"] == b["max_stack"]


def canonical(export, new_index=None):
    """An export up to the numbering of its nodes and leaf records: the device builders hand out node indices (and with them leaf record
    ranges) by atomic counters, so two builds of the same tree differ in that numbering and in nothing else.  Depth first from the root in
    slot order: every node's bytes with its child references replaced by 0 (inner) / minus the triangle count (leaf), every leaf's
    records (triangle indices through `new_index` if given)."""
    nodes, tris = export["nodes"], export["tris"]
    out = [np.int64([len(nodes), len(tris), export["max_stack"]]).tobytes()]

    def visit(ref):                                                           # (at most 31 levels deep)
        if ref < 0:
            first, n = (~ref) >> 2, ((~ref) & 3) + 1
            rec = tris[first:first + n].copy()
            if new_index is not None:
                rec["tri"] = new_index[rec["tri"]]
            out.append(rec.tobytes())
            return
        node = nodes[ref:ref + 1].copy()
        k = int(node["meta"][0]) & 7
        child = [int(c) for c in node["child"][0, :k]]
        node["child"][0, :k] = [0 if c >= 0 else -(((~c) & 3) + 1) for c in child]
        out.append(node.tobytes())
        for c in child:
            visit(c)

    if len(tris):
        visit(int(export["root"]))
    return b"".join(out)


def _mesh_slices(sc, m):
    first, count, material = sc.meshes[m]
    tr = sc.mesh_transforms[m]
    a, n = int(tr["vertex_start"]), int(tr["vertex_count"])
    t = sc.triangles[first:first + count].copy()
    for k in ("v0", "v1", "v2"):
        assert len(t) == 0 or ((t[k] >= a) & (t[k] < a + n)).all()           # the mesh's triangles use its own vertex range
        t[k] -= a
    return dict(tris=t, world=sc.world_vertices[a:a + n].copy(), obj=sc.vertices[a:a + n].copy(), material=material, transform=dict(tr))


def _append_slices(sc, s):
    """The mesh `s` (of _mesh_slices) pushed onto the end of the scene's arrays with the world vertices it had, bit for bit."""
    v0, t0 = len(sc.world_vertices), len(sc.triangles)
    t = s["tris"].copy()
    for k in ("v0", "v1", "v2"):
        t[k] += v0
    sc.vertices = np.concatenate([sc.vertices, s["obj"]])
    sc.world_vertices = np.concatenate([sc.world_vertices, s["world"]])
    sc.triangles = np.concatenate([sc.triangles, t])
    sc.meshes.append((t0, len(t), s["material"]))
    sc.mesh_transforms.append({**s["transform"], "vertex_start": v0, "vertex_count": len(s["world"])})
    return len(sc.meshes) - 1


def twin_regraft(twin, sc, meshes):
    """The twin's side on context `twin`, which holds `sc` (left untouched: the twin edits a copy).  Every step is checked against the
    prune rule / the graft rule / the placed-graft rule and the invariants.  Returns (final export, reports as tuples, old triangle ->
    twin triangle, the branches of the prune rule met, the twin's scene)."""
    meshes = [int(m) for m in meshes]
    tw = copy.deepcopy(sc)
    slices = [_mesh_slices(tw, m) for m in meshes]
    ranges = [tw.meshes[m][:2] for m in meshes]
    T = len(tw.triangles)
    dead = removed_triangles(tw, meshes)
    new_index = np.full(T, -1, dtype=np.int64)
    new_index[~dead] = np.arange(int((~dead).sum()))
    before = twin.export_bvh()
    twin.remove_meshes(tw.remove_meshes_from_scene(meshes))
    after = twin.export_bvh()
    met = check_prune(before, after, dead)
    if len(tw.triangles):
        check_bvh_invariants(after, tw, require_wide=False)
    reports = []
    for (first, count), s in zip(ranges, slices):
        t0 = len(tw.triangles)
        new_index[first:first + count] = np.arange(t0, t0 + count)
        before = after
        twin.append_meshes(tw, _append_slices(tw, s))
        after = twin.export_bvh()
        if count == 0:
            reports.append(None)
            continue
        pl = twin.last_append_placement()
        if pl.kind in (pr.SLOT, pr.PAIR) and pl.mode == 1:
            pr.check_placed_graft(before, after, count, pl)
        elif pl.kind != pr.REBUILT:
            check_graft(before, after, count)
        check_bvh_invariants(after, tw, require_wide=False)
        reports.append(placement_tuple(pl))
    assert (new_index >= 0).all()
    return after, reports, new_index.astype(np.uint32), met, tw


def assert_equals_twin(export, reports, twin_export, twin_reports, new_index, exact=True):
    """The header's consequence.  `exact` = False (trees of the device builders, whose node numbering is not reproducible from one build
    to the next): the same up to that numbering (canonical), and the reports without the node index."""
    if exact:
        assert export["nodes"].tobytes() == twin_export["nodes"].tobytes()
        assert export["root"] == twin_export["root"] and export["max_stack"] == twin_export["max_stack"]
        mapped = export["tris"].copy()
        mapped["tri"] = new_index[mapped["tri"]]
        assert mapped.tobytes() == twin_export["tris"].tobytes()
    else:
        assert canonical(export, new_index) == canonical(twin_export)
    assert len(reports) == len(twin_reports)
    for got, want in zip(reports, twin_reports):
        if want is None:                                                      # a mesh without triangles: zero apart from the mode
            assert placement_tuple(got)[1:] == (0,) * 8
        elif exact:
            assert placement_tuple(got) == want, (placement_tuple(got), want)
        else:
            assert placement_tuple(got)[:2] + placement_tuple(got)[3:] == want[:2] + want[3:], (placement_tuple(got), want)


def regraft_against_twin(make, meshes, exact=True):
    """`make()` builds (context, scene) the same way twice; one regrafts `meshes`, the other plays the twin.  Returns (the regrafted
    context, its scene, the reports, the branches of the prune rule the twin met); the twin is closed."""
    ctx, sc = make()
    twin, sc2 = make()
    a, b = ctx.export_bvh(), twin.export_bvh()
    assert same_export(a, b) if exact else canonical(a) == canonical(b)
    reports = ctx.regraft_meshes(meshes)
    export = ctx.export_bvh()
    twin_export, twin_reports, new_index, met, _ = twin_regraft(twin, sc2, meshes)
    twin.close()
    assert_equals_twin(export, reports, twin_export, twin_reports, new_index, exact)
    if len(sc.triangles):
        check_bvh_invariants(export, sc, require_wide=False)
    return ctx, sc, reports, met
