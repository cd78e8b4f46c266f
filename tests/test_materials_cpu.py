"""fyprt_update_materials / fyprt_export_emissive on host-only contexts (device -1): after every edit of a chain the light trees and the
emissive list equal those of a fresh context that uploads the edited scene; an explicit emissive list is taken as given; every error
case of the contract answers its code, EINVAL before ESTATE.  The device side of the call is tests/test_gpu_materials.py."""
import ctypes as C
import re
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

from common import struct_equal
from fypraytracer_amd import capi, scenes
from fypraytracer_amd.scene import Material

ROOT = Path(__file__).resolve().parent.parent
EINVAL, ESTATE = -1, -3


def test_header_and_symbol_list_declare_the_new_entry_points():
    header = (ROOT / "include" / "fyprt.h").read_text()
    declared = set(re.findall(r"\b(fyprt_[a-z_0-9]+)\s*\(", header))
    lib = capi.load_library()
    for name in ("fyprt_update_materials", "fyprt_export_emissive"):
        assert name in declared and name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)


def same_lights(a, b, n_meshes):
    la, lb = a.export_lighttrees(n_meshes), b.export_lighttrees(n_meshes)
    for k in ("tlas", "blas"):
        assert len(la[k]) == len(lb[k]) and struct_equal(la[k], lb[k]).all(), k
    assert la["tlas_root"] == lb["tlas_root"]
    for k in ("blas_first", "blas_count", "blas_root"):
        assert np.array_equal(la[k], lb[k]), k
    assert np.array_equal(a.export_emissive(), b.export_emissive())
    return la


def derived_list(sc):
    """np.flatnonzero of the per-material flag gathered through the triangles' material index."""
    flag = np.array([bool((np.asarray(m.emission_color, np.float32) * np.float32(m.emission_power)).any()) for m in sc.materials])
    return np.flatnonzero(flag[sc.triangles["materialIndex"]]).astype(np.uint32)


def hall_edit_chain(sc):
    """The edits of the chain, each as (name, function applying it to the scene and returning the reassigned meshes).  hall_small: meshes
    0-11 walls, 12-19 columns, 20-23 drapes, 24-27 lights; materials 0-11 palette, 12-15 lights."""
    mgr = sc.manager()
    saved = {}

    def power(sc):
        sc.materials[13] = replace(sc.materials[13], emission_power=sc.materials[13].emission_power * 0.5 + 3.0)
        mgr.material_edited(13)
        return []

    def palette(sc):
        sc.materials[2] = replace(sc.materials[2], emission_color=(1.0, 0.6, 0.3), emission_power=2.5)      # columns and drapes become emitters
        mgr.material_edited(2)
        return []

    def reassign(sc):
        mgr.set_mesh_material(sc, 22, 14)           # a drape to a light material
        mgr.set_mesh_material(sc, 25, 5)            # a light mesh to a palette material
        return [22, 25]

    def off(sc):
        for i, m in enumerate(sc.materials):
            saved[i] = m
            sc.materials[i] = replace(m, emission_power=0.0)
            mgr.material_edited(i)
        return []

    def on(sc):
        for i, m in saved.items():
            sc.materials[i] = m
            mgr.material_edited(i)
        return []

    return [("power", power), ("palette", palette), ("reassign", reassign), ("off", off), ("on", on)]


def test_edit_chain_equals_fresh_uploads():
    sc = scenes.hall_scene_small()
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    a = capi.Context(-1)
    a.upload_scene(sc)
    assert np.array_equal(a.export_emissive(), derived_list(sc)) and len(a.export_emissive()) == 32
    for name, edit in hall_edit_chain(sc):
        meshes = edit(sc)
        assert mgr.perform_all_scene_updates(sc) is True
        a.update_materials(sc, meshes)
        b = capi.Context(-1)
        b.upload_scene(sc)
        lt = same_lights(a, b, len(sc.meshes))
        want = derived_list(sc)
        assert np.array_equal(a.export_emissive(), want), name
        if name == "off":
            assert len(want) == 0 and len(lt["tlas"]) == 0 and len(lt["blas"]) == 0
        if name == "palette":
            assert len(want) > 1000                  # the columns and drapes of that material
        b.close()
    assert capi.live_device_bytes() == 0
    a.close()


def test_created_material_and_fast_path_leave_lights_alone():
    sc = scenes.cornell_box()
    a = capi.Context(-1)
    a.upload_scene(sc)
    before = a.export_lighttrees(len(sc.meshes))
    sc.materials[1] = replace(sc.materials[1], albedo=(0.3, 0.9, 0.1), roughness=0.4)
    sc.materials.append(Material(albedo=(0.5, 0.5, 0.5)))                 # "Create New Material"
    a.update_materials(sc)
    after = a.export_lighttrees(len(sc.meshes))
    for k in ("tlas", "blas"):
        assert before[k].tobytes() == after[k].tobytes()
    assert np.array_equal(a.export_emissive(), sc.emissive_triangles)
    sc.manager().set_mesh_material(sc, 3, 5)                              # the new material is usable
    sc.manager().perform_all_scene_updates(sc)
    a.update_materials(sc, [3])
    b = capi.Context(-1)
    b.upload_scene(sc)
    same_lights(a, b, len(sc.meshes))
    a.close(); b.close()


def test_explicit_emissive_list_is_taken_as_given():
    sc = scenes.cornell_box()
    a = capi.Context(-1)
    a.upload_scene(sc)
    given = np.array([31, 4, 30, 4], dtype=np.uint32)                     # any order, repeats, non-emissive triangles
    a.update_materials(sc, emissive_triangles=given)
    assert np.array_equal(a.export_emissive(), given)
    a.update_materials(sc, emissive_triangles=np.zeros(0, dtype=np.uint32))
    assert len(a.export_emissive()) == 0
    a.update_materials(sc)                                                # NULL: derived again
    assert np.array_equal(a.export_emissive(), sc.emissive_triangles)
    a.close()


def _call(ctx, mats, n_mats, idx, mat, n_mesh, em, n_em, handle=True):
    lib = ctx.lib
    return lib.fyprt_update_materials(ctx.h if handle else None, mats, n_mats, idx, mat, n_mesh, em, n_em)


def test_error_cases_in_the_contracts_order():
    sc = scenes.cornell_box()
    m = np.ascontiguousarray(sc.materials_array())
    mp, n = m.ctypes.data, len(m)
    u32, i32 = C.c_uint32, C.c_int32
    one, mat0 = (u32 * 1)(0), (i32 * 1)(0)
    nT, nM = len(sc.triangles), len(sc.meshes)
    fresh = capi.Context(-1)                                              # nothing uploaded: EINVAL cases still win over ESTATE
    assert _call(fresh, mp, n, None, None, 0, None, 0, handle=False) == EINVAL
    assert _call(fresh, None, n, None, None, 0, None, 0) == EINVAL
    assert _call(fresh, mp, n, None, mat0, 1, None, 0) == EINVAL and _call(fresh, mp, n, one, None, 1, None, 0) == EINVAL
    assert _call(fresh, mp, n, one, mat0, 1, None, 0) == EINVAL            # no mesh yet: index out of range
    assert _call(fresh, mp, n, None, None, 0, None, 0) == ESTATE           # before fyprt_upload_scene
    n_out = u32()
    assert fresh.lib.fyprt_export_emissive(fresh.h, None, C.byref(n_out)) == ESTATE and fresh.lib.fyprt_export_emissive(None, None, C.byref(n_out)) == EINVAL
    fresh.close()
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    assert _call(ctx, mp, n - 1, None, None, 0, None, 0) == EINVAL         # the table must not shrink
    assert b"shrink" in ctx.lib.fyprt_last_error(ctx.h)
    assert _call(ctx, mp, n, (u32 * 1)(nM), mat0, 1, None, 0) == EINVAL    # mesh index out of range
    assert _call(ctx, mp, n, one, (i32 * 1)(-1), 1, None, 0) == EINVAL and _call(ctx, mp, n, one, (i32 * 1)(n), 1, None, 0) == EINVAL
    assert _call(ctx, mp, n, None, None, 0, (u32 * 2)(0, nT), 2) == EINVAL  # emissive triangle index out of range
    # order: a shrunken table is reported before a bad mesh index, a bad mesh index before a bad material index, that before the list
    assert _call(ctx, mp, n - 1, (u32 * 1)(nM), mat0, 1, None, 0) == EINVAL and b"shrink" in ctx.lib.fyprt_last_error(ctx.h)
    assert _call(ctx, mp, n, (u32 * 1)(nM), (i32 * 1)(-1), 1, None, 0) == EINVAL and b"mesh index" in ctx.lib.fyprt_last_error(ctx.h)
    assert _call(ctx, mp, n, one, (i32 * 1)(n), 1, (u32 * 1)(nT), 1) == EINVAL and b"material index" in ctx.lib.fyprt_last_error(ctx.h)
    assert _call(ctx, mp, n, one, mat0, 1, None, 0) == 0                   # and the good call passes
    # nothing of the refused calls was applied
    ref = capi.Context(-1)
    ref.upload_scene(sc)
    same_lights(ctx, ref, nM)
    # a scene uploaded with prebuilt light trees is refused (EINVAL cases first)
    pre = capi.Context(-1)
    pre.upload_scene(sc, light_trees=ref.export_lighttrees(nM))
    assert _call(pre, mp, n - 1, None, None, 0, None, 0) == EINVAL
    assert _call(pre, mp, n, None, None, 0, None, 0) == ESTATE and b"prebuilt" in pre.lib.fyprt_last_error(pre.h)
    for c in (ctx, ref, pre):
        c.close()
