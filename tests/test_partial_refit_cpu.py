"""The partial refit (fyprt_update_mesh_vertices, fyprt_last_edit_stats, tuning key 22) on host-only contexts (capi.Context(-1)): argument
and state errors in the header's order, the tuning key, and the dirty rule restated in partial_refit_common.py on host-built exports.
The device work is checked in test_gpu_partial_refit.py."""
import ctypes as C

import numpy as np
import pytest

from common import SCENES
from fypraytracer_amd import capi
from partial_refit_common import expected_dirty_nodes, mesh_triangles, node_parents

EINVAL, ESTATE = -1, -3


def _call(ctx, meshes, n_vertices, null_meshes=False, null_vertices=False):
    idx = (C.c_uint32 * max(1, len(meshes)))(*meshes)
    v = np.zeros(max(1, n_vertices), dtype=capi.VERTEX_DTYPE)
    return ctx.lib.fyprt_update_mesh_vertices(ctx.h, None if null_meshes else idx, len(meshes), None if null_vertices else v.ctypes.data, n_vertices)


def test_update_mesh_vertices_errors_on_a_host_only_context():
    sc = SCENES["cornell"][0]()
    ctx = capi.Context(-1)
    lib = ctx.lib
    assert lib.fyprt_update_mesh_vertices(None, None, 0, None, 0) == EINVAL               # NULL context
    assert _call(ctx, [0], 4, null_meshes=True) == EINVAL                                 # NULL arrays with a non-zero count come first,
    assert _call(ctx, [0], 4, null_vertices=True) == EINVAL                               # before any state is looked at
    assert _call(ctx, [0], 4) == ESTATE                                                   # before fyprt_upload_scene
    assert b"fyprt_upload_scene" in lib.fyprt_last_error(ctx.h)
    assert _call(ctx, [], 0) == ESTATE                                                    # ... whatever the counts
    ctx.upload_scene(sc)
    before = ctx.export_bvh()
    assert _call(ctx, [0], 4, null_vertices=True) == EINVAL
    assert _call(ctx, [0], 4) == ESTATE                                                   # no mesh vertex ranges (a host-only context cannot take them)
    assert b"fyprt_set_object_vertices" in lib.fyprt_last_error(ctx.h)
    assert _call(ctx, [99], 4) == ESTATE                                                  # state before the mesh indices
    assert _call(ctx, [], 0) == ESTATE
    with pytest.raises(capi.FyprtError):
        ctx.update_mesh_vertices(sc, [0])
    after = ctx.export_bvh()
    assert before["nodes"].tobytes() == after["nodes"].tobytes() and before["tris"].tobytes() == after["tris"].tobytes()
    ctx.close()


def test_last_edit_stats_before_any_edit():
    ctx = capi.Context(-1)
    st = capi.EditStats()
    assert ctx.lib.fyprt_last_edit_stats(None, C.byref(st)) == EINVAL
    assert ctx.lib.fyprt_last_edit_stats(ctx.h, None) == EINVAL
    assert ctx.lib.fyprt_last_edit_stats(ctx.h, C.byref(st)) == ESTATE
    ctx.upload_scene(SCENES["cornell"][0]())
    assert ctx.lib.fyprt_last_edit_stats(ctx.h, C.byref(st)) == ESTATE                    # an upload is no geometry edit
    with pytest.raises(capi.FyprtError, match="geometry edit"):
        ctx.last_edit_stats()
    assert C.sizeof(capi.EditStats) == 20
    ctx.close()


def test_tuning_key_22():
    ctx = capi.Context(-1)
    assert ctx.get_tuning(22) == 0                                                        # the full passes stay the default
    ctx.set_tuning(22, 1)
    assert ctx.get_tuning(22) == 1
    with pytest.raises(capi.FyprtError, match="0..1"):
        ctx.set_tuning(22, 2)
    assert ctx.lib.fyprt_set_tuning(ctx.h, 22, -1) == EINVAL
    assert ctx.get_tuning(22) == 1
    ctx.set_tuning(22, 0)
    assert ctx.get_tuning(22) == 0
    with pytest.raises(capi.FyprtError):                                                  # key 23 stays reserved
        ctx.set_tuning(23, 1)
    ctx.close()


@pytest.fixture(scope="module", params=["cornell", "hall_small"])
def export(request):
    sc = SCENES[request.param][0]()
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    return sc, bvh


def test_all_triangles_dirty_all_nodes(export):
    sc, bvh = export
    assert expected_dirty_nodes(bvh, range(len(sc.triangles))) == set(range(len(bvh["nodes"])))
    assert expected_dirty_nodes(bvh, []) == set()


def test_one_mesh_gives_a_set_closed_under_parent_with_the_root(export):
    sc, bvh = export
    parent, _ = node_parents(bvh)
    assert (parent >= 0).sum() == len(parent) - 1 and parent[bvh["root"]] == -1           # one root, every other node has one parent
    sizes = []
    for m in range(len(sc.meshes)):
        dirty = expected_dirty_nodes(bvh, mesh_triangles(sc, [m]))
        assert bvh["root"] in dirty
        assert all(int(parent[k]) in dirty for k in dirty if k != bvh["root"])
        sizes.append(len(dirty))
    assert min(sizes) < len(bvh["nodes"])                                                  # a single mesh does not dirty the whole tree
    # the set of two meshes is the union of their sets: shared ancestors count once
    a, b = expected_dirty_nodes(bvh, mesh_triangles(sc, [0])), expected_dirty_nodes(bvh, mesh_triangles(sc, [len(sc.meshes) - 1]))
    assert expected_dirty_nodes(bvh, mesh_triangles(sc, [0, len(sc.meshes) - 1])) == a | b and len(a & b) >= 1
