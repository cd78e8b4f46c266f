"""fyprt_append_meshes / fyprt_append_textures on host-only contexts (capi.Context(-1)): everything but the device work.  The graft of
the acceleration structure, the light trees and the emissive list of an append against a context that uploaded the combined scene; the
exported tree walked by the oracle against the oracle's reference tracer; the depth fall-back; errors and states; textures."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

from append_common import SIZES, add_emitter_material, append_patch, check_graft
from common import SCENES, check_bvh_invariants
from edit_sequences import same_exports as same_light_exports
from fypraytracer_amd import capi

W, H = 128, 80
EINVAL, ESTATE = -1, -3


def fresh_host(sc):
    ref = capi.Context(-1)
    ref.upload_scene(sc)
    return ref


def test_appends_graft_and_lights_equal_an_upload():
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)                              # in the table before the upload: an append does not touch the materials
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    kinds = []
    for step, n in enumerate(SIZES):
        before = ctx.export_bvh()
        m = append_patch(sc, cam, "cornell", n, light if n == 5 else 4, shift=(0.3 * step - 0.45, 0.2, 0.05 * step))
        ctx.append_meshes(sc, m)
        after = ctx.export_bvh()
        check_bvh_invariants(after, sc, require_wide=False)
        kinds.append(check_graft(before, after, n))
        ref = fresh_host(sc)
        same_light_exports(ctx, ref, len(sc.meshes))
        ref.close()
    assert set(kinds) == {"attach", "new root"}, kinds            # cornell's root is full: a new root first, then it takes children
    assert len(ctx.export_emissive()) == 2 + 5
    ctx.close()


def test_exported_tree_finds_the_reference_tracers_distances(oracle_built):
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    t_old = len(sc.triangles)
    for step, n in enumerate(SIZES):
        ctx.append_meshes(sc, append_patch(sc, cam, "cornell", n, 4, shift=(0.3 * step - 0.45, 0.2, 0.05 * step)))
    walk, ref = Oracle(sc, W, H), Oracle(sc, W, H)
    walk.use_product_bvh(ctx.export_bvh())
    ref.use_reference_tracer()
    d = cam.ray_directions().reshape(-1, 3)
    o = np.asarray(cam.position, dtype=np.float32)
    ta = np.array([walk.trace(o, r)[0]["hitDistance"] for r in d], dtype=np.float32)
    hits = [ref.trace(o, r)[0] for r in d]
    tb = np.array([h["hitDistance"] for h in hits], dtype=np.float32)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))             # an exact-t tie changes the triangle, never the distance
    assert sum(int(h["objectIndex"]) >= t_old for h in hits) > 50             # the camera does see the appended meshes
    ctx.close()


def test_many_small_appends_fall_back_to_a_rebuild():
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    deepest, rebuilt = 0, 0
    for k in range(120):
        before = ctx.export_bvh()
        m = append_patch(sc, cam, "cornell", 1, light if k == 60 else 0, shift=(0.01 * k - 0.6, -0.3, 0.0))
        ctx.append_meshes(sc, m)
        after = ctx.export_bvh()
        assert after["max_stack"] <= 31
        deepest = max(deepest, after["max_stack"])
        if after["max_stack"] < before["max_stack"]:
            rebuilt += 1                                          # the graft never makes a tree shallower: this was the fall-back
    assert rebuilt >= 1 and deepest == 31                         # one level about every third append: 120 appends cannot all be grafted
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    ref = fresh_host(sc)
    same_light_exports(ctx, ref, len(sc.meshes))
    ref.close()
    ctx.close()


def _raw_append(ctx, v, t, ms, ov=None, first=None, stride=None, counts=None):
    """fyprt_append_meshes with the arrays as given (None = NULL); counts = (vertices, triangles, meshes) overrides the arrays' lengths."""
    p = lambda a: None if a is None else a.ctypes.data
    nv, nt, nm = counts if counts else (0 if v is None else len(v), 0 if t is None else len(t), 0 if ms is None else len(ms))
    f = None if first is None else (C.c_uint32 * len(first))(*first)
    return ctx.lib.fyprt_append_meshes(ctx.h, p(v), nv, p(t), nt, capi.TRIANGLE_DTYPE.itemsize if stride is None else stride, p(ms), nm, p(ov), f)


def _tails(sc, first_new_mesh):
    v0, t0 = sc.mesh_transforms[first_new_mesh]["vertex_start"], sc.meshes[first_new_mesh][0]
    return (np.ascontiguousarray(sc.world_vertices[v0:]), np.ascontiguousarray(sc.triangles[t0:]), np.ascontiguousarray(sc.meshes_array()[first_new_mesh:]),
            np.ascontiguousarray(sc.vertices[v0:]), v0, t0)


def test_errors_states_and_the_empty_append():
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = capi.Context(-1)
    base = mk_scene()
    m = append_patch(sc, cam, "cornell", 5, 4)
    append_patch(sc, cam, "cornell", 4, 4, shift=(0.4, 0, 0))
    v, t, ms, ov, v0, t0 = _tails(sc, m)
    nv = len(sc.world_vertices)
    assert ctx.lib.fyprt_append_meshes(None, None, 0, None, 0, 16, None, 0, None, None) == EINVAL        # a NULL context
    assert _raw_append(ctx, None, None, None) == ESTATE                                                    # before the upload (only the empty append has valid arguments then)
    assert _raw_append(ctx, None, t, ms, counts=(len(v), len(t), len(ms))) == EINVAL                       # ... bad arguments come first
    ctx.upload_scene(base)
    exports = lambda: (ctx.export_bvh(), ctx.export_lighttrees(len(base.meshes)), ctx.export_emissive())
    e0 = exports()
    # a NULL array with a non-zero count
    assert _raw_append(ctx, None, t, ms, counts=(len(v), len(t), len(ms))) == EINVAL
    assert _raw_append(ctx, v, None, ms, counts=(len(v), len(t), len(ms))) == EINVAL
    assert _raw_append(ctx, v, t, None, counts=(len(v), len(t), len(ms))) == EINVAL
    assert _raw_append(ctx, v, t, ms, ov=ov, first=None) == EINVAL
    assert _raw_append(ctx, v, t, ms, stride=12) == EINVAL                                                 # stride < 16
    bad = t.copy(); bad["v1"][3] = nv
    assert _raw_append(ctx, v, bad, ms) == EINVAL                                                          # a vertex index >= the combined count
    bad = t.copy(); bad["materialIndex"][2] = len(sc.materials)
    assert _raw_append(ctx, v, bad, ms) == EINVAL                                                          # a material outside the table
    bad = ms.copy(); bad["materialIndex"][1] = -1
    assert _raw_append(ctx, v, t, bad) == EINVAL
    for field, delta in (("firstTriangle", 1), ("triangleCount", -1), ("triangleCount", 1)):              # meshes that do not partition the range in order
        bad = ms.copy(); k = 1 if field == "firstTriangle" else 0
        bad[field][k] = int(bad[field][k]) + delta
        assert _raw_append(ctx, v, t, bad) == EINVAL, (field, delta)
    assert _raw_append(ctx, v, t, ms[::-1].copy()) == EINVAL
    assert _raw_append(ctx, v, t, ms[:1]) == EINVAL
    first = [tr["vertex_start"] for tr in sc.mesh_transforms[m:]] + [nv]
    assert _raw_append(ctx, v, t, ms, ov=ov, first=[first[0] + 1] + first[1:]) == EINVAL                  # mesh_first_vertex not spanning / out of order
    assert _raw_append(ctx, v, t, ms, ov=ov, first=first[:-1] + [nv - 1]) == EINVAL
    assert _raw_append(ctx, v, t, ms, ov=ov, first=[first[0], first[2], first[2]]) == EINVAL              # a triangle outside its mesh's vertex range
    assert _raw_append(ctx, v, t, ms, ov=ov, first=[first[0], nv + 3, nv]) == EINVAL
    # nothing of all that changed the context; nor does the empty append
    assert _raw_append(ctx, None, None, None) == 0
    assert _raw_append(ctx, v, None, None, counts=(len(v), 0, 0)) == 0
    e1 = exports()
    for k in ("nodes", "tris"):
        assert e0[0][k].tobytes() == e1[0][k].tobytes()
    assert e0[0]["root"] == e1[0]["root"]
    for k in ("tlas", "blas", "blas_first", "blas_count", "blas_root"):
        assert e0[1][k].tobytes() == e1[1][k].tobytes()
    assert np.array_equal(e0[2], e1[2])
    # the valid call, with object-space vertices (a host-only context holds no copy: they are checked and ignored)
    assert _raw_append(ctx, v, t, ms, ov=ov, first=first) == 0
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    ctx.close()
    # a scene uploaded with prebuilt light trees
    pre = capi.Context(-1)
    pre.upload_scene(base)
    lt = pre.export_lighttrees(len(base.meshes))
    pre.upload_scene(base, light_trees=lt)
    assert _raw_append(pre, v, t, ms) == ESTATE
    pre.close()


def test_append_textures_then_a_material_points_at_the_new_one():
    mk_scene, _ = SCENES["cornell"]
    sc = mk_scene()
    ctx = capi.Context(-1)
    tex = (np.arange(8 * 4, dtype=np.uint32).reshape(8, 4) * 0x01020304) | 0xFF000000
    with pytest.raises(capi.FyprtError, match="error -3"):
        ctx.append_textures([tex])                                # before the upload
    ctx.upload_scene(sc)
    assert ctx.lib.fyprt_append_textures(None, None, 0) == EINVAL
    assert ctx.lib.fyprt_append_textures(ctx.h, None, 2) == EINVAL
    empty = (capi.Texture * 1)()
    assert ctx.lib.fyprt_append_textures(ctx.h, C.cast(empty, C.POINTER(capi.Texture)), 1) == EINVAL      # NULL pixels, no size
    ctx.append_textures([])
    before = ctx.export_bvh()
    ctx.append_textures([tex, tex[:2, :3].copy()])
    sc.textures = [tex, tex[:2, :3].copy()]
    sc.materials[4] = replace(sc.materials[4], is_use_albedo_map=True, albedo_map_index=1)
    sc.materials[3] = replace(sc.materials[3], emission_power=25.0)
    ctx.update_materials(sc)
    ref = fresh_host(sc)
    same_light_exports(ctx, ref, len(sc.meshes))
    ba, bb = ctx.export_bvh(), ref.export_bvh()
    for k in ("nodes", "tris"):
        assert ba[k].tobytes() == before[k].tobytes() == bb[k].tobytes(), k
    ref.close()
    ctx.close()
