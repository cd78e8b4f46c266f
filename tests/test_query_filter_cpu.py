"""Query filters on host-only contexts (capi.Context(-1)): the life of the mesh mask table — set and get, the header's error order, an
append extends it with all ones, a removal compacts it in order, a failed call leaves it alone, an upload drops it and resets the query
mask, a regraft and the material edits keep it — and tests/filter_ref.py's node words against independent facts on hand-built trees and
on exported ones."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import filter_ref as fr
from append_common import append_patch
from common import SCENES
from fypraytracer_amd import capi

EINVAL, ESTATE = -1, -3
ALL = 0xFFFFFFFF
W, H = 96, 64


def _host(name="hall_small"):
    sc = SCENES[name][0]()
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    return ctx, sc


def _raw_set(ctx, masks, count, handle=True):
    arr = None if masks is None else (C.c_uint32 * max(1, len(masks)))(*masks)
    return ctx.lib.fyprt_set_mesh_query_masks(ctx.h if handle else None, arr, count)


def _table(n, seed=3):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def test_header_and_symbol_list_declare_the_entry_points():
    header = (Path(__file__).resolve().parent.parent / "include" / "fyprt.h").read_text()
    lib = capi.load_library()
    for name in ("fyprt_set_mesh_query_masks", "fyprt_set_query_mask", "fyprt_get_query_filter"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_set_then_get_and_the_defaults():
    ctx, sc = _host()
    assert ctx.query_filter() == (None, ALL, 0)                              # off by default, Q all ones, nothing built
    M = _table(len(sc.meshes))
    ctx.set_mesh_query_masks(M)
    got, q, builds = ctx.query_filter()
    assert got.dtype == np.uint32 and np.array_equal(got, M) and q == ALL and builds == 0     # host-only: nothing to build
    ctx.set_query_mask(0x80000001)
    assert ctx.query_filter()[1] == 0x80000001 and np.array_equal(ctx.query_filter()[0], M)
    ctx.set_mesh_query_masks(M[::-1])                                        # a new table replaces the old one, Q stays
    assert np.array_equal(ctx.query_filter()[0], M[::-1]) and ctx.query_filter()[1] == 0x80000001
    ctx.set_mesh_query_masks(None)
    assert ctx.query_filter() == (None, 0x80000001, 0)
    # the count alone, and every optional out-pointer NULL
    ctx.set_mesh_query_masks(M)
    n = C.c_uint32(77)
    assert ctx.lib.fyprt_get_query_filter(ctx.h, None, C.byref(n), None, None) == 0 and n.value == len(M)
    ctx.close()


def test_error_order_of_the_header():
    ctx, sc = _host()
    nM = len(sc.meshes)
    fresh = capi.Context(-1)                                                  # nothing uploaded
    # 1. NULL context before everything
    assert _raw_set(ctx, [1] * nM, nM, handle=False) == EINVAL and _raw_set(fresh, None, 3, handle=False) == EINVAL
    # 2. NULL array with a count / an array with count 0: before the state check
    assert _raw_set(fresh, None, 3) == EINVAL and _raw_set(fresh, [1], 0) == EINVAL
    assert _raw_set(ctx, None, nM) == EINVAL and _raw_set(ctx, [1] * nM, 0) == EINVAL
    # 3. before fyprt_upload_scene — also the call that switches the filter off, and a count that would be wrong anyway
    assert _raw_set(fresh, [1] * 3, 3) == ESTATE and _raw_set(fresh, None, 0) == ESTATE
    # 4. a count different from the scene's
    assert _raw_set(ctx, [1] * (nM + 1), nM + 1) == EINVAL and _raw_set(ctx, [1] * (nM - 1), nM - 1) == EINVAL
    assert ctx.query_filter()[0] is None                                      # no failed call set anything
    M = _table(nM)
    ctx.set_mesh_query_masks(M)
    assert _raw_set(ctx, [1] * (nM + 1), nM + 1) == EINVAL and _raw_set(ctx, None, nM) == EINVAL
    assert np.array_equal(ctx.query_filter()[0], M)                           # ... nor changed the table that was set
    # the query mask: any state; the getter: NULL context or count
    assert fresh.lib.fyprt_set_query_mask(fresh.h, 5) == 0 and fresh.query_filter() == (None, 5, 0)
    assert ctx.lib.fyprt_set_query_mask(None, 5) == EINVAL
    n = C.c_uint32()
    assert ctx.lib.fyprt_get_query_filter(None, None, C.byref(n), None, None) == EINVAL
    assert ctx.lib.fyprt_get_query_filter(ctx.h, None, None, None, None) == EINVAL
    fresh.close(); ctx.close()


def test_table_follows_appends_and_removals():
    mk_scene, mk_cam = SCENES["hall_small"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    n0 = len(sc.meshes)
    M = _table(n0, seed=5)
    ctx.set_mesh_query_masks(M)
    ctx.set_query_mask(6)
    # an append extends the table with all ones, one per new mesh
    first = append_patch(sc, cam, "hall_small", 5, 0)
    ctx.append_meshes(sc, first)
    append_patch(sc, cam, "hall_small", 1, 0, shift=(0.3, 0.0, 0.0))
    ctx.append_meshes(sc, first + 1)
    want = np.concatenate([M, [ALL, ALL]]).astype(np.uint32)
    assert len(sc.meshes) == n0 + 2 and np.array_equal(ctx.query_filter()[0], want)
    # a failed removal (a mesh listed twice, an index out of range) leaves it unchanged
    idx = (C.c_uint32 * 2)(3, 3)
    assert ctx.lib.fyprt_remove_meshes(ctx.h, idx, 2, None) == EINVAL
    idx = (C.c_uint32 * 1)(n0 + 2)
    assert ctx.lib.fyprt_remove_meshes(ctx.h, idx, 1, None) == EINVAL
    assert np.array_equal(ctx.query_filter()[0], want)
    # a removal takes the removed meshes' entries out, the rest moves down in order
    gone = [2, n0, 7]
    ctx.remove_meshes(sc.remove_meshes_from_scene(gone))
    want = np.delete(want, gone)
    assert len(sc.meshes) == n0 - 1 and np.array_equal(ctx.query_filter()[0], want)
    assert ctx.query_filter()[1] == 6                                         # no edit touches Q
    # with the filter off an append sets no table
    ctx.set_mesh_query_masks(None)
    ctx.append_meshes(sc, append_patch(sc, cam, "hall_small", 4, 0, shift=(0.0, 0.2, 0.0)))
    assert ctx.query_filter()[0] is None
    # an upload drops the table and resets Q
    ctx.set_mesh_query_masks(np.arange(len(sc.meshes), dtype=np.uint32))
    assert ctx.query_filter()[0] is not None
    ctx.upload_scene(sc)
    assert ctx.query_filter() == (None, ALL, 0)
    ctx.close()


def test_table_outlives_regrafts_and_shading_edits():
    ctx, sc = _host()
    M = _table(len(sc.meshes), seed=9)
    ctx.set_mesh_query_masks(M)
    ctx.set_query_mask(9)
    for mode in (0, 1):
        ctx.set_append_placement(mode)
        ctx.regraft_meshes([3, 5])
        assert np.array_equal(ctx.query_filter()[0], M)
    sc.materials[0].roughness = 0.25
    ctx.update_materials(sc)
    ctx.update_materials(sc, [1])
    ctx.append_textures([np.full((2, 2), 0xFF00FF00, dtype=np.uint32)])
    assert np.array_equal(ctx.query_filter()[0], M) and ctx.query_filter()[1] == 9
    v = np.ascontiguousarray(sc.world_vertices)
    assert ctx.lib.fyprt_update_vertices(ctx.h, v.ctypes.data, len(v)) == ESTATE     # a geometry edit needs a device; refused, nothing moves
    assert np.array_equal(ctx.query_filter()[0], M)
    ctx.close()


# ---- filter_ref.node_masks
def _node(children):
    n = np.zeros(1, dtype=capi.BVH_NODE_DTYPE)[0]
    return n, children


def _hand_tree():
    """Seven leaf records in four leaves under three nodes: root 0 -> (node 1, node 2, leaf of record 6); node 1 -> leaves (0, 1) and (2);
    node 2 -> leaf (3, 4, 5).  Records 0-2 belong to mesh 0, 3-5 to mesh 1, 6 to mesh 2."""
    nodes = np.zeros(3, dtype=capi.BVH_NODE_DTYPE)
    leaf = lambda first, n: ~((first << 2) | (n - 1))
    nodes["child"][0] = (1, 2, leaf(6, 1), -2 ** 31); nodes["meta"][0] = 3 | (2 << 3)
    nodes["child"][1] = (leaf(0, 2), leaf(2, 1), -2 ** 31, -2 ** 31); nodes["meta"][1] = 2 | (1 << 3)
    nodes["child"][2] = (leaf(3, 3), -2 ** 31, -2 ** 31, -2 ** 31); nodes["meta"][2] = 1 | (1 << 3)
    tris = np.zeros(7, dtype=capi.BVH_TRI_DTYPE)
    tris["tri"] = [4, 5, 3, 0, 2, 1, 6]                                       # leaf order is not triangle order
    meshes = [(3, 3, 0), (0, 3, 0), (6, 1, 0)]                                # nor is mesh order the order of the first triangles
    return {"nodes": nodes, "tris": tris, "root": 0}, meshes


def test_node_masks_on_a_hand_built_tree():
    bvh, meshes = _hand_tree()
    M = np.array([0x11, 0x206, 0x80000000], dtype=np.uint32)
    lm = fr.leaf_masks(bvh, meshes, M)
    assert lm.tolist() == [0x11] * 3 + [0x206] * 3 + [0x80000000]
    nm = fr.node_masks(bvh, lm)
    assert nm[0] == 0x11 | 0x206 | 0x80000000                                 # the root word is the OR of all
    assert nm[1] == 0x11 and nm[2] == 0x206                                   # a node over one mesh has that mesh's word
    by_sets, reached = fr.node_masks_by_sets(bvh, lm)
    assert reached.all() and np.array_equal(by_sets, nm)
    assert fr.admitted(bvh, meshes, M, 0x10).tolist() == [True] * 3 + [False] * 4
    assert fr.admitted(bvh, meshes, M, 0x80000004).tolist() == [False] * 3 + [True] * 4
    assert not fr.admitted(bvh, meshes, M, 0x40000000).any()
    assert fr.filtered(bvh, meshes, M, 0x200)["tris"]["tri"].tolist() == [0, 2, 1]
    assert fr.renumbering(meshes, [True, False, True]).tolist() == [-1, -1, -1, 0, 1, 2, 3]


@pytest.mark.parametrize("name", ["cornell", "hall_small"])
def test_node_masks_on_exported_trees(name):
    """One bit per mesh (modulo 32): the root word is the OR of all words, a node's word has exactly the bits of the meshes with a
    record below it, and the level order of node_masks agrees with the record sets — also after an append and a regraft."""
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    ctx.append_meshes(sc, append_patch(sc, cam, name, 300, 0))
    ctx.regraft_meshes([1])
    bvh = ctx.export_bvh()
    ctx.close()
    M = (np.uint32(1) << (np.arange(len(sc.meshes), dtype=np.uint32) % 32)).astype(np.uint32)
    lm = fr.leaf_masks(bvh, sc.meshes, M)
    nm = fr.node_masks(bvh, lm)
    by_sets, reached = fr.node_masks_by_sets(bvh, lm)
    assert reached[bvh["root"]] and np.array_equal(nm[reached], by_sets[reached])
    assert nm[bvh["root"]] == np.bitwise_or.reduce(M)
    mesh_of = fr.mesh_of_triangle(sc.meshes, len(sc.triangles))
    from points_ref import leaf_records_below
    below = leaf_records_below(bvh)
    single = 0
    for i in np.nonzero(reached)[0]:
        ms = np.unique(mesh_of[bvh["tris"]["tri"][np.concatenate(below[i])]])
        if len(ms) == 1:
            single += 1
            assert nm[i] == M[ms[0]], i
    assert single > 10                                                        # the appended mesh alone is a sub-tree of many nodes
