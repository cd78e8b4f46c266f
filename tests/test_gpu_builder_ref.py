"""The device builders (tuning key 12: 1 = radix tree, 2 = PLOC; rt_lbvh.h, build_device_lbvh) and the refit pass (rt_refit.h) against
builder_ref.py, EXACTLY: the leaf-record order, the tree in canonical form (slot order, leaf positions, shape; node numbers come
from atomics and are not compared), every node's level count, and every node's origin, exponents and plane bytes.  No tolerance, no
sampling.  test_gpu_lbvh.py holds the same builders to bars that any valid tree passes; this file pins WHICH tree is built.
The inputs and what each is there for: builder_cases.py; that they reach the mechanisms: test_builder_ref_cpu.py."""
import numpy as np
import pytest

import builder_cases as bc
import builder_ref as br
from append_common import append_patch
from common import check_bvh_invariants
from fypraytracer_amd import capi, scenes

pytestmark = pytest.mark.gpu

BUILD_CASES = [(f, n, b) for f, n in bc.CASES for b in (1, 2)] + [(*bc.TOO_DEEP, 1)]      # the too-deep shape is an ordinary case for the radix tree


def upload(sc, builder):
    ctx = capi.Context(0)
    ctx.resize(16, 16)
    ctx.set_tuning(12, builder)
    ctx.upload_scene(sc)
    return ctx


def tri_boxes(sc):
    lb = br.leaf_boxes(bc.scene_triangles(sc))
    return lb[:, :3], lb[:, 3:]


def assert_tree(export, ref, what, root=None, leaf_base=0, tri_base=0):
    """Leaf order, canonical tree and level counts of the (sub-)tree at `root` against build_ref's result."""
    want = np.asarray(ref["leaf_tris"], dtype=np.int64) + tri_base
    got = export["tris"]["tri"][leaf_base:leaf_base + len(want)].astype(np.int64)
    if not np.array_equal(got, want):
        k = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{what}: leaf record {leaf_base + k} holds triangle {got[k]}, the reference's order has {want[k]} there ({int((got != want).sum())} records differ)")
    diff = br.first_tree_difference(br.canonical(export, root, leaf_base), ref["tree"])
    assert diff is None, f"{what}: node at path {diff[0]} (slots from the root): device {diff[1]}, reference {diff[2]}"
    levels = br.levels_by_path(ref["tree"])
    seen = 0
    for path, idx in br.walk_export(export, root):
        got_levels = int(export["nodes"][idx]["meta"]) >> 3
        assert got_levels == levels[path], f"{what}: node at path {path}: {got_levels} levels recorded, the reference has {levels[path]}"
        seen += 1
    assert seen == sum(ref["level_counts"]) == len(levels)


def assert_quantisation(export, sc, what, root=None):
    """origin, ex, qlo and qhi of every node below `root` against quantise_ref of the node's exact child boxes."""
    bad = br.quantisation_differences(export, *tri_boxes(sc), root=root)
    assert not bad, f"{what}: node at path {bad[0][0]}: {bad[0][1]}: device {bad[0][2]}, reference {bad[0][3]} ({len(bad)} fields differ in all)"


@pytest.mark.parametrize("family,n,builder", BUILD_CASES)
def test_device_build_equals_the_reference(family, n, builder):
    what = f"builder {builder}, {family}, n = {n}"
    ref = bc.reference(family, n, builder)
    assert not ref["too_deep"]
    sc = bc.make_scene(bc.triangles(family, n))
    ctx = upload(sc, builder)
    export = ctx.export_bvh()
    ctx.close()
    assert_tree(export, ref, what)
    assert_quantisation(export, sc, what)
    assert export["root"] == 0 and len(export["nodes"]) == sum(ref["level_counts"]) and export["max_stack"] == len(ref["level_counts"]), what


def test_too_deep_ploc_tree_falls_back_to_the_host_builder():
    """More than 31 wide levels in the reference (test_builder_ref_cpu.py proves it): the driver hands the scene to the host builder,
    whose tree is not the reference's; it must be a valid one."""
    family, n = bc.TOO_DEEP
    assert bc.reference(family, n, 2)["too_deep"]
    sc = bc.make_scene(bc.triangles(family, n))
    ctx = upload(sc, 2)
    export = ctx.export_bvh()
    ctx.close()
    check_bvh_invariants(export, sc, require_wide=False)


@pytest.mark.parametrize("radius,n", bc.RADIUS_CASES)
def test_ploc_search_radius(monkeypatch, radius, n):
    """FYPRT_PLOC_RADIUS is read on every build and clamped to 1..32; the window reaches into the neighbouring 256-block."""
    what = f"builder 2, radius {radius}, soup, n = {n}"
    monkeypatch.setenv("FYPRT_PLOC_RADIUS", str(radius))
    ref = bc.reference("soup", n, 2, radius)
    sc = bc.make_scene(bc.triangles("soup", n))
    ctx = upload(sc, 2)
    export = ctx.export_bvh()
    ctx.close()
    assert_tree(export, ref, what)
    assert_quantisation(export, sc, what)


@pytest.mark.parametrize("builder", [1, 2])
def test_two_builds_of_one_input_differ_in_node_numbers_only(builder):
    family, n = "duplicates", 513
    sc = bc.make_scene(bc.triangles(family, n))
    exports = []
    for _ in range(2):
        ctx = upload(sc, builder)
        exports.append(ctx.export_bvh())
        ctx.close()
    a, b = exports
    assert a["tris"].tobytes() == b["tris"].tobytes()
    assert br.first_tree_difference(br.canonical(a), br.canonical(b)) is None
    by_path = [{path: e["nodes"][idx] for path, idx in br.walk_export(e)} for e in exports]
    for path, node in by_path[0].items():
        other = by_path[1][path]
        assert all(node[f].tobytes() == other[f].tobytes() for f in ("origin", "ex", "meta", "qlo", "qhi")), (builder, path)


@pytest.mark.parametrize("builder", [1, 2])
def test_refit_after_a_transform_edit(builder):
    """update_vertices keeps topology and leaf order; every node's bytes are quantise_ref of the MOVED geometry."""
    family, n = bc.EDIT_CASE
    what = f"builder {builder}, {family}, n = {n}, after update_vertices"
    sc = bc.make_scene(bc.triangles(family, n))
    ctx = upload(sc, builder)
    before = ctx.export_bvh()
    assert_tree(before, bc.reference(family, n, builder), what + " (before)")
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    mgr.set_mesh_transform(sc, 0, pos=(0.3, -0.2, 1.1), rotation=(10.0, 20.0, 30.0), scale_=(1.1, 0.9, 1.3))
    mgr.perform_all_scene_updates(sc)
    assert not np.array_equal(sc.world_vertices["position"], bc.triangles(family, n).reshape(-1, 3))
    ctx.update_vertices(sc)
    after = ctx.export_bvh()
    ctx.close()
    assert np.array_equal(after["tris"]["tri"], before["tris"]["tri"])
    assert after["nodes"]["child"].tobytes() == before["nodes"]["child"].tobytes() and np.array_equal(after["nodes"]["meta"], before["nodes"]["meta"])
    assert_quantisation(after, sc, what)
    assert after["nodes"]["origin"].tobytes() != before["nodes"]["origin"].tobytes()


def subtree_over(export, first_id, count):
    """The node whose leaves hold exactly the triangle ids [first_id, first_id + count)."""
    nodes, tri = export["nodes"], export["tris"]["tri"]
    below = {}
    for _, idx in reversed(list(br.walk_export(export))):
        ids = []
        for c in nodes[idx]["child"][:int(nodes[idx]["meta"]) & 7]:
            c = int(c)
            ids += below[c] if c >= 0 else tri[(~c >> 2):(~c >> 2) + (~c & 3) + 1].tolist()
        below[idx] = ids
    want = list(range(first_id, first_id + count))
    found = [idx for idx, ids in below.items() if sorted(ids) == want]
    assert len(found) == 1, found
    return found[0]


@pytest.mark.parametrize("builder", [1, 2])
def test_appended_subtree_equals_the_reference(builder):
    """append_meshes builds the new triangles with the same builder over the appended vertices' grid and grafts the result: after
    a device-built root of four children the first append makes a root pair, the next two attach to it (2, 3, 4 children)."""
    family, n0 = bc.EDIT_CASE
    sc = bc.make_scene(bc.triangles(family, n0))
    cam = scenes.cornell_camera(16, 16)
    ctx = upload(sc, builder)
    for step, n in enumerate(bc.APPEND_SIZES):
        what = f"builder {builder}, {family}, n = {n0}, append of {n}"
        t0, v0 = len(sc.triangles), len(sc.world_vertices)
        mesh = append_patch(sc, cam, "cornell", n, 0, shift=(0.4 * step - 0.4, 0.1, 0.05 * step))
        ctx.append_meshes(sc, mesh)
        export = ctx.export_bvh()
        new_pos = bc.scene_triangles(sc, t0, n)
        ref = br.build_ref(new_pos, sc.world_vertices["position"][v0:], builder)
        assert not ref["too_deep"]
        sub = subtree_over(export, t0, n)
        assert_tree(export, ref, what, root=sub, leaf_base=t0, tri_base=t0)
        assert_quantisation(export, sc, what)                    # the whole tree: the sub-tree, the root that took it, the old nodes
        assert (int(export["nodes"][export["root"]]["meta"]) & 7) == 2 + step, what
    ctx.close()
