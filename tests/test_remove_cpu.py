"""fyprt_remove_meshes on host-only contexts (capi.Context(-1)): everything but the device work.  The prune rule restated on two exports
(remove_common.check_prune), the structural invariants of the pruned tree, light trees and emissive list against a context that uploaded
the reduced scene, the exported tree walked by the oracle against the oracle's reference tracer, appends after removals, edge shapes,
errors, and the Python scene edit.
The host builder makes one sub-tree per mesh, so on these contexts no leaf holds triangles of two meshes: the branch "leaf partly
emptied" needs a device-built tree and is met in test_gpu_remove.py; the other six are met here."""
import ctypes as C

import numpy as np
import pytest

from append_common import add_emitter_material, append_patch, check_graft
from common import SCENES, check_bvh_invariants
from edit_sequences import same_exports as same_light_exports
from fypraytracer_amd import capi
from fypraytracer_amd.scene import Scene
from remove_common import BRANCHES, LOSES, check_prune, removed_triangles

W, H = 128, 80
EINVAL, ESTATE = -1, -3
MET = set()                        # the branches of the prune rule the tests of this module met, in file order


def fresh_host(sc):
    ref = capi.Context(-1)
    ref.upload_scene(sc)
    return ref


def remove(ctx, sc, meshes, **kw):
    """One removal on context and scene, checked against the prune rule and the invariants; returns the branches met."""
    before = ctx.export_bvh()
    dead = removed_triangles(sc, meshes)
    ctx.remove_meshes(sc.remove_meshes_from_scene(meshes), **kw)
    after = ctx.export_bvh()
    met = check_prune(before, after, dead)
    if len(sc.triangles):
        check_bvh_invariants(after, sc, require_wide=False)
    else:
        assert len(after["nodes"]) == len(after["tris"]) == 0 and after["root"] == 0 and after["max_stack"] == 0
    MET.update(met)
    return met


@pytest.mark.parametrize("name", ["cornell", "hall_small"])
def test_prune_rule_invariants_and_lights_equal_an_upload(name):
    sc = SCENES[name][0]()
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    n_em = len(ctx.export_emissive())
    remove(ctx, sc, LOSES[name])                                  # hall_small: a column, a drape and a light mesh in ONE call
    ref = fresh_host(sc)
    same_light_exports(ctx, ref, len(sc.meshes))                  # a derived list: exactly what upload derives
    assert len(ctx.export_emissive()) == (n_em - 8 if name == "hall_small" else n_em)
    ref.close()
    ctx.close()


def test_an_explicit_emissive_list_stays_explicit():
    sc = SCENES["cornell"][0]()
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    t_light = int(sc.meshes[7][0])
    sc.emissive_triangles = np.array([t_light + 1, 12, 3, t_light], dtype=np.uint32)      # not in order, two non-emitters, one of them on the tall box
    ctx.update_materials(sc, emissive_triangles=sc.emissive_triangles)
    assert sc.meshes[5][0] <= 12 < sc.meshes[5][0] + sc.meshes[5][1]
    remove(ctx, sc, LOSES["cornell"])
    gone = 2 + 10                                                                          # the right wall and the tall box lie before the light
    assert sc.emissive_triangles.tolist() == [t_light + 1 - gone, 3, t_light - gone]
    ref = fresh_host(sc)
    ref.update_materials(sc, emissive_triangles=sc.emissive_triangles)
    same_light_exports(ctx, ref, len(sc.meshes))
    ref.close()
    ctx.close()


def test_exported_tree_finds_the_reference_tracers_distances(oracle_built):
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    for step, n in enumerate((5, 300, 4)):
        ctx.append_meshes(sc, append_patch(sc, cam, "cornell", n, 4, shift=(0.3 * step - 0.45, 0.2, 0.05 * step)))
    remove(ctx, sc, (6, 8, 2))                                    # the short box, the 5-triangle patch, the back wall
    walk, ref = Oracle(sc, W, H), Oracle(sc, W, H)
    walk.use_product_bvh(ctx.export_bvh())
    ref.use_reference_tracer()
    d = cam.ray_directions().reshape(-1, 3)
    o = np.asarray(cam.position, dtype=np.float32)
    ta = np.array([walk.trace(o, r)[0]["hitDistance"] for r in d], dtype=np.float32)
    tb = np.array([ref.trace(o, r)[0]["hitDistance"] for r in d], dtype=np.float32)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))             # an exact-t tie changes the triangle, never the distance
    assert (tb < 0).sum() > 50                                                 # the back wall is gone: rays leave the box
    ctx.close()


def test_append_remove_append_still_grafts():
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 300, 4, shift=(-0.4, 0.2, 0.0)))
    remove(ctx, sc, (5,))                                         # an OLD mesh
    before = ctx.export_bvh()
    ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 5, light, shift=(0.3, 0.2, 0.1)))
    after = ctx.export_bvh()
    check_graft(before, after, 5)                                 # one record per triangle still holds: leafBase = the triangle count
    check_bvh_invariants(after, sc, require_wide=False)
    ref = fresh_host(sc)
    same_light_exports(ctx, ref, len(sc.meshes))
    ref.close()
    ctx.close()


def test_edge_shapes():
    mk_scene, mk_cam = SCENES["cornell"]
    # a grafted sub-tree removed whole: the two-child root (R, S) is spliced away and R is the root again
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    first = ctx.export_bvh()
    m = append_patch(sc, cam, "cornell", 300, 4)
    ctx.append_meshes(sc, m)
    grown = ctx.export_bvh()
    assert grown["root"] == len(grown["nodes"]) - 1 and (int(grown["nodes"][-1]["meta"]) & 7) == 2
    met = remove(ctx, sc, (m,))
    assert {"splice onto an inner node", "root replaced", "node dropped"} <= met
    back = ctx.export_bvh()
    assert back["root"] == first["root"] and back["nodes"].tobytes() == first["nodes"].tobytes() and back["tris"].tobytes() == first["tris"].tobytes()
    # three grafts (a new root that takes two more children), a fourth (another new root), then all four leave: a chain of two splices
    ms = []
    for k, n in enumerate((5, 1, 4, 5)):
        ms.append(append_patch(sc, cam, "cornell", n, 4, shift=(0.2 * k - 0.4, 0.1, 0.0)))
        ctx.append_meshes(sc, ms[-1])
    top = ctx.export_bvh()
    assert (int(top["nodes"][top["root"]]["meta"]) & 7) == 2 and top["max_stack"] == first["max_stack"] + 2
    met = remove(ctx, sc, ms)
    assert "chain of splices" in met
    assert ctx.export_bvh()["nodes"].tobytes() == first["nodes"].tobytes()
    # mesh_count == 0 changes nothing
    ctx.remove_meshes({"meshes": [], "vertex_ranges": []})
    assert ctx.export_bvh()["nodes"].tobytes() == first["nodes"].tobytes()
    # all but a one-triangle mesh: the root becomes a leaf code
    one = append_patch(sc, cam, "cornell", 1, 4)
    ctx.append_meshes(sc, one)
    met = remove(ctx, sc, tuple(range(one)))
    b = ctx.export_bvh()
    assert b["root"] == ~0 and len(b["nodes"]) == 0 and len(b["tris"]) == 1 and "splice onto a leaf code" in met
    ref = fresh_host(sc)
    same_light_exports(ctx, ref, 1)
    rb = ref.export_bvh()
    assert rb["root"] == b["root"] and rb["tris"].tobytes() == b["tris"].tobytes()
    ref.close()
    # ... an append onto the leaf-code root, then everything goes: the state of an upload of a scene without triangles
    ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 4, 4, shift=(0.3, 0, 0)))
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    remove(ctx, sc, (0, 1))
    assert len(sc.triangles) == len(sc.world_vertices) == len(sc.meshes) == 0
    ref = fresh_host(sc)
    same_light_exports(ctx, ref, 0)
    a, b = ctx.export_bvh(), ref.export_bvh()
    assert (len(a["nodes"]), len(a["tris"]), a["root"], a["max_stack"]) == (len(b["nodes"]), len(b["tris"]), b["root"], b["max_stack"])
    ref.close()
    ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 5, 4))                 # the empty tree takes a graft
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    ctx.close()


def _raw(ctx, meshes, ranges=None, count=None):
    idx = None if meshes is None else (C.c_uint32 * max(1, len(meshes)))(*meshes)
    vr = None if ranges is None else (C.c_uint32 * max(2, len(ranges)))(*ranges)
    return ctx.lib.fyprt_remove_meshes(ctx.h, idx, len(meshes) if count is None else count, vr)


def test_errors_in_order_and_a_failed_call_changes_nothing():
    sc = SCENES["cornell"][0]()
    ctx = capi.Context(-1)
    nv = len(sc.world_vertices)
    own = lambda m: [sc.mesh_transforms[m]["vertex_start"], sc.mesh_transforms[m]["vertex_count"]]
    assert ctx.lib.fyprt_remove_meshes(None, None, 0, None) == EINVAL                  # a NULL context
    assert _raw(ctx, []) == ESTATE                                                      # before the upload (only the empty call has valid arguments then)
    assert _raw(ctx, [0]) == EINVAL                                                     # ... bad arguments come first
    ctx.upload_scene(sc)
    exports = lambda: (ctx.export_bvh(), ctx.export_lighttrees(len(sc.meshes)), ctx.export_emissive())
    e0 = exports()
    assert _raw(ctx, None, count=2) == EINVAL                                           # NULL mesh_indices with a non-zero count
    assert _raw(ctx, [8]) == EINVAL                                                     # a mesh index out of range
    assert _raw(ctx, [8, 8]) == EINVAL                                                  # ... comes before "listed twice"
    assert _raw(ctx, [3, 5, 3]) == EINVAL                                               # a mesh listed twice
    assert _raw(ctx, [3, 3], [nv, 1, 0, 4]) == EINVAL                                   # ... comes before the vertex ranges
    assert _raw(ctx, [5], [nv - 3, 4]) == EINVAL                                        # a vertex range beyond the vertex count
    assert _raw(ctx, [4, 5], own(4)[:1] + [6] + own(5)) == EINVAL                       # two vertex ranges that overlap
    assert _raw(ctx, [4, 5], [nv, 1] + own(4)) == EINVAL                                # (beyond the count comes before an overlap)
    assert _raw(ctx, [5], own(6)) == EINVAL                                             # a surviving triangle (of mesh 6) uses a removed vertex
    assert _raw(ctx, [5], [own(5)[0], own(5)[1] + 1]) == EINVAL
    e1 = exports()
    for k in ("nodes", "tris"):
        assert e0[0][k].tobytes() == e1[0][k].tobytes()
    assert e0[0]["root"] == e1[0]["root"]
    for k in ("tlas", "blas", "blas_first", "blas_count", "blas_root"):
        assert e0[1][k].tobytes() == e1[1][k].tobytes()
    assert np.array_equal(e0[2], e1[2])
    assert _raw(ctx, [5], own(5)) == 0                                                  # the valid call
    sc.remove_meshes_from_scene([5])
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    # without ranges a context that holds no object-space copy removes no vertex: the orphans stay part of the description
    assert _raw(ctx, [4]) == 0
    orphans = sc.world_vertices.copy()
    sc.remove_meshes_from_scene([4])
    moved = Scene(materials=sc.materials, world_vertices=orphans, vertices=orphans, meshes=sc.meshes, mesh_transforms=sc.mesh_transforms)
    t = sc.triangles.copy()
    for k in ("v0", "v1", "v2"):
        t[k] = np.where(t[k] >= own(4)[0], t[k] + 4, t[k])
    moved.triangles = t
    check_bvh_invariants(ctx.export_bvh(), moved, require_wide=False)
    ctx.close()
    # a scene uploaded with prebuilt light trees
    base = SCENES["cornell"][0]()
    pre = capi.Context(-1)
    pre.upload_scene(base)
    lt = pre.export_lighttrees(len(base.meshes))
    pre.upload_scene(base, light_trees=lt)
    assert _raw(pre, [5]) == ESTATE
    assert _raw(pre, [9]) == EINVAL
    pre.close()


def test_scene_edit_equals_a_scene_built_without_the_meshes():
    mk_scene, mk_cam = SCENES["cornell"]
    cam = mk_cam(W, H)

    def build(skip):
        sc = Scene()
        sc.materials = mk_scene().materials
        light = add_emitter_material(sc)
        for k, n in enumerate((4, 300, 1, 5, 7, 2)):
            if k not in skip:
                append_patch(sc, cam, "cornell", n, light if k in (1, 3, 5) else 4, shift=(0.1 * k, 0, 0))
        sc.init_scene_emissive_triangles()
        return sc

    full, want = build(()), build((1, 4))
    rec = full.remove_meshes_from_scene([4, 1])
    assert rec == {"meshes": [1, 4], "vertex_ranges": [(12, 900), (12 + 900 + 3 + 15, 21)]}
    for k in ("world_vertices", "vertices", "triangles"):
        assert getattr(full, k).tobytes() == getattr(want, k).tobytes(), k
    assert full.meshes == want.meshes and full.mesh_transforms == want.mesh_transforms
    assert full.emissive_triangles.dtype == np.uint32 and np.array_equal(full.emissive_triangles, want.emissive_triangles)
    assert len(want.emissive_triangles) == 5 + 2


def test_every_branch_of_the_prune_rule_was_met():
    """(runs last in this file)  All but "leaf partly emptied", which no host-built tree can show: see the module docstring."""
    assert MET >= set(BRANCHES[1:]), set(BRANCHES) - MET
