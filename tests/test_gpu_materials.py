"""fyprt_update_materials on the device: a material edit (table, mesh reassignment, emissive list, light records, light trees) must leave
the context in exactly the state a fyprt_upload_scene of the edited scene reaches — frames, reservoirs, exports — without touching the
acceleration structure.  Every comparison is bit-exact; the yardstick is a second context that re-uploads.
  A  equals a re-upload, with ReSTIR history carried across the edit (cornell, hall_small, banana)
  B  the ordered compaction of the emissive list at its wave / tile / workgroup boundaries, and past the workgroup cap
  C  after a device transform edit (the host's vertex copy of a mesh that was no light when it moved is stale)
  D  the fast path (no emission moved)      E  state and error codes      F  a two-band group      G  the C++ facade"""
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for, struct_equal
from edit_sequences import same_exports
from fypraytracer_amd import capi
from fypraytracer_amd.scene import Material, Scene

pytestmark = pytest.mark.gpu

W, H = 128, 80
TECHS = (capi.RESTIR_DI, capi.RESTIR_GI, capi.NEE, capi.LIGHT_SOURCE_SAMPLING, capi.BRDF_SAMPLING)


def _ctx(sc, cam):
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    return ctx


def same_frames(a, b, techs=TECHS, seed0=10):
    for tech in techs:
        st = settings_for(tech)
        for f in range(2):
            st.rand_seed = seed0 + f
            a.render(st)
            b.render(st)
            (ia, aa), (ib, ab) = a.readback(), b.readback()
            assert np.array_equal(ia, ib) and bits_equal(aa, ab).all(), (tech, f)
            for buf in (capi.BUF_DI, capi.BUF_DI_PREV):
                assert struct_equal(a.read_buffer(buf), b.read_buffer(buf)).all(), (tech, f, buf)
            assert a.frame_index == b.frame_index


# ---- the edits: each returns the reassigned meshes
def cornell_second_light(sc):
    sc.materials[3] = replace(sc.materials[3], emission_power=25.0)
    sc.manager().material_edited(3)
    sc.manager().set_mesh_material(sc, 3, 3)                 # the red wall becomes a light: one light becomes two
    return [3]


def hall_palette_emits(sc):
    sc.materials[2] = replace(sc.materials[2], emission_color=(1.0, 0.6, 0.3), emission_power=2.5)      # columns and drapes become emitters
    sc.manager().material_edited(2)
    return []


def hall_reassign(sc):
    sc.manager().set_mesh_material(sc, 22, 14)               # a drape to a light material
    sc.manager().set_mesh_material(sc, 25, 5)                # a light mesh to a palette material
    return [22, 25]


def banana_map_off(sc):
    sc.materials[0] = replace(sc.materials[0], is_use_albedo_map=False)
    sc.manager().material_edited(0)
    return []


def banana_map_on(sc):
    sc.materials[0] = replace(sc.materials[0], is_use_albedo_map=True)
    sc.manager().material_edited(0)
    return []


@pytest.mark.parametrize("name,edits", [("cornell", [cornell_second_light]), ("hall_small", [hall_palette_emits, hall_reassign]),
                                        ("banana", [banana_map_off, banana_map_on])])
def test_a_update_equals_reupload_with_history(name, edits):
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    a, b = _ctx(sc, cam), _ctx(sc, cam)
    st = settings_for(capi.RESTIR_DI)
    for f in range(2):                                       # history the edit must carry identically
        st.rand_seed = f + 1
        a.render(st)
        b.render(st)
    for step, edit in enumerate(edits):
        before = a.export_bvh()
        meshes = edit(sc)
        assert mgr.perform_all_scene_updates(sc) is True
        a.update_materials(sc, meshes)
        b.upload_scene(sc)
        ba, bb = a.export_bvh(), b.export_bvh()
        for k in ("nodes", "tris"):
            assert ba[k].tobytes() == before[k].tobytes() and ba[k].tobytes() == bb[k].tobytes(), k
        same_exports(a, b, len(sc.meshes))
        same_frames(a, b, seed0=10 + 20 * step)
    if name == "cornell":
        assert len(a.export_emissive()) == 4
    a.close()
    b.close()


# ---- B
GRID_MESHES = (1, 63, 64, 65, 127, 255, 256, 257, 1023, 1025, 2049)


def strip_scene(mesh_sizes, per_row=128):
    """A flat grid of small triangles at y = 0, cut into consecutive meshes of the given sizes, one material per mesh."""
    sc = Scene()
    sc.materials = [Material(albedo=(0.8, 0.8, 0.8)) for _ in mesh_sizes]
    first = 0
    for m, n in enumerate(mesh_sizes):
        j = np.arange(first, first + n)
        x, z = (j % per_row).astype(np.float32) * 0.01, (j // per_row).astype(np.float32) * 0.01
        p = np.zeros((n, 3, 3), dtype=np.float32)
        p[:, :, 0], p[:, :, 2] = x[:, None], z[:, None]
        p[:, 1, 0] += 0.008
        p[:, 2, 2] += 0.008
        nrm = np.tile(np.array([0, 1, 0], dtype=np.float32), (n * 3, 1))
        sc.add_new_mesh_to_scene(p.reshape(-1, 3), nrm, np.zeros((n * 3, 2), dtype=np.float32), np.arange(n * 3, dtype=np.uint32).reshape(-1, 3), material_index=m)
        first += n
    return sc


def set_emitters(sc, flags):
    for m, on in enumerate(flags):
        sc.materials[m] = replace(sc.materials[m], emission_color=(1.0, 1.0, 1.0), emission_power=3.0 if on else 0.0)
    return np.flatnonzero(np.asarray(flags, dtype=bool)[sc.triangles["materialIndex"]]).astype(np.uint32)


def test_b_compaction_boundaries():
    sc = strip_scene(GRID_MESHES)
    nM = len(GRID_MESHES)
    ctx = capi.Context(0)
    ctx.upload_scene(sc)
    assert len(ctx.export_emissive()) == 0
    alt = [m % 2 == 0 for m in range(nM)]
    patterns = {"alternate": alt, "inverse": [not f for f in alt], "all": [True] * nM, "none": [False] * nM,
                "first": [m == 0 for m in range(nM)], "last": [m == nM - 1 for m in range(nM)]}
    for order in (("alternate", "inverse", "all", "none", "first", "last"), ("last", "all", "first", "none", "inverse", "alternate", "all")):
        for name in order:
            want = set_emitters(sc, patterns[name])
            ctx.update_materials(sc)
            got = ctx.export_emissive()
            assert np.array_equal(got, want), (name, len(got), len(want))
    ref = capi.Context(-1)                                   # and the light trees follow (all emissive at this point)
    ref.upload_scene(sc)
    la, lb = ctx.export_lighttrees(nM), ref.export_lighttrees(nM)
    assert struct_equal(la["blas"], lb["blas"]).all() and struct_equal(la["tlas"], lb["tlas"]).all()
    ctx.close()
    ref.close()


def test_b_compaction_past_the_workgroup_cap():
    """More than 1024 x 1024 triangles: the number of workgroups is capped and every workgroup owns more than four tiles."""
    sizes = (300_001, 449_999, 310_000)                      # 1 060 000 triangles
    sc = strip_scene(sizes, per_row=1024)
    # the light trees hang on the MESH's material, the list on the triangles': a fourth, dark material for the meshes keeps the host
    # from building light trees over a million emitters, which is not what is tested here
    sc.materials.append(Material(albedo=(0.5, 0.5, 0.5)))
    sc.meshes = [(f, n, 3) for f, n, _ in sc.meshes]
    ctx = capi.Context(0)
    ctx.set_tuning(12, 1)                                    # device builder: the tree is not what is tested here
    ctx.upload_scene(sc)
    for flags in ((True, False, True, False), (False, True, False, False), (True, True, True, False)):
        want = set_emitters(sc, flags)
        ctx.update_materials(sc)
        assert np.array_equal(ctx.export_emissive(), want), flags
    ctx.close()


# ---- C
@pytest.mark.parametrize("name,mesh,material", [("cornell", 6, 4), ("hall_small", 13, 2)])
def test_c_after_a_device_transform(name, mesh, material):
    mk_scene, mk_cam = SCENES[name]
    cam = mk_cam(W, H)
    sa, sb = mk_scene(), mk_scene()
    assert sa.meshes[mesh][2] == material
    sb.materials[material] = replace(sb.materials[material], emission_color=(0.9, 1.0, 0.7), emission_power=6.0)
    a, b = _ctx(sa, cam), _ctx(sb, cam)                      # b: the edited materials at the original positions
    for c, s in ((a, sa), (b, sb)):
        c.set_object_vertices(s)
        s.manager().set_mesh_transform(s, mesh, pos=(0.3, 0.1, -0.2), rotation=(0, 20, 0))
        c.update_transforms(s, [mesh])                       # in a the mesh is no light while it moves
    a.update_materials(sb)
    same_exports(a, b, len(sa.meshes))
    same_frames(a, b, techs=(capi.NEE, capi.RESTIR_DI))
    a.close()
    b.close()


# ---- D
def test_d_fast_path_leaves_lights_alone():
    mk_scene, mk_cam = SCENES["hall_small"]
    sc, cam = mk_scene(), mk_cam(W, H)
    a, b = _ctx(sc, cam), _ctx(sc, cam)
    lt0, em0 = a.export_lighttrees(len(sc.meshes)), a.export_emissive()
    sc.materials[4] = replace(sc.materials[4], albedo=(0.2, 0.9, 0.4), roughness=0.35)
    sc.materials[7] = replace(sc.materials[7], metallic=1.0)
    a.update_materials(sc)
    b.upload_scene(sc)
    lt1 = a.export_lighttrees(len(sc.meshes))
    for k in ("tlas", "blas", "blas_first", "blas_count", "blas_root"):
        assert lt0[k].tobytes() == lt1[k].tobytes(), k
    assert np.array_equal(em0, a.export_emissive())
    same_frames(a, b, techs=(capi.RESTIR_DI, capi.NEE, capi.BRDF_SAMPLING))
    a.close()
    b.close()


# ---- E
def test_e_state_and_no_light():
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    a, b = _ctx(sc, cam), _ctx(sc, cam)
    st = settings_for(capi.BRDF_SAMPLING)
    a.render(st)
    a.denoise_temporal()
    a.read_buffer(capi.BUF_TEMPORAL)
    sc.materials[1] = replace(sc.materials[1], albedo=(0.1, 0.2, 0.9))
    a.update_materials(sc)
    with pytest.raises(capi.FyprtError, match="error -3"):
        a.denoise()
    with pytest.raises(capi.FyprtError, match="error -3"):
        a.read_buffer(capi.BUF_TEMPORAL)
    a.render(st)
    a.denoise()
    # every emitter off
    sc.materials[3] = replace(sc.materials[3], emission_power=0.0)
    a.update_materials(sc)
    b.upload_scene(sc)
    assert len(a.export_emissive()) == 0
    for tech in (capi.NEE, capi.RESTIR_DI):
        for c in (a, b):
            with pytest.raises(capi.FyprtError, match="error -4"):
                c.render(settings_for(tech))
    for c in (a, b):
        c.resize(W, H)                                       # a rendered before, b did not: both from zero
    same_frames(a, b, techs=(capi.BRDF_SAMPLING,))
    # radiance queries see the edited scene
    sc.materials[3] = replace(sc.materials[3], emission_power=15.0, emission_color=(1.0, 0.8, 0.6))
    a.update_materials(sc)
    b.upload_scene(sc)
    d = cam.ray_directions().reshape(-1, 3)
    o = np.tile(np.asarray(cam.position, dtype=np.float32), (len(d), 1))
    for tech in (capi.NEE, capi.BRDF_SAMPLING):
        ra, rb = a.render_rays(o, d, settings_for(tech), frame_index=3), b.render_rays(o, d, settings_for(tech), frame_index=3)
        assert bits_equal(ra, rb).all() and (ra[:, :3] > 0).any(), tech
    a.close()
    b.close()


# ---- F
def test_f_group_members_updated_between_frames():
    mk_scene, mk_cam = SCENES["cornell"]
    cam = mk_cam(W, H)
    bounds = [0, 40, H]

    def run(members):
        sc = mk_scene()
        ctxs = [_ctx(sc, cam) for _ in range(members)]
        grp = capi.Group(ctxs, bounds, halo_mode=1) if members > 1 else None
        st = settings_for(capi.RESTIR_DI)
        outs = []
        for f in range(4):
            if f == 2:
                meshes = cornell_second_light(sc)
                sc.manager().perform_all_scene_updates(sc)
                if grp:
                    grp.synchronize()
                for c in ctxs:
                    c.update_materials(sc, meshes)
            st.rand_seed = f + 1
            if grp:
                grp.render(st)
                grp.synchronize()
                acc = np.zeros((H, W, 4), np.float32)
                for c, (r0, r1) in zip(ctxs, zip(bounds, bounds[1:])):
                    c.set_rows(r0, r1, 0)
                    acc[r0:r1] = c.readback()[1][r0:r1]
            else:
                ctxs[0].render(st)
                acc = ctxs[0].readback()[1]
            outs.append(acc)
        if grp:
            grp.close()
        for c in ctxs:
            c.close()
        return outs

    single, banded = run(1), run(2)
    for f in (2, 3):
        assert bits_equal(single[f], banded[f]).all(), f


# ---- G
def test_g_facade_updates_materials_without_a_second_upload():
    exe = Path(capi.__file__).resolve().parent / "host" / "material_edit"
    assert exe.exists(), "host/build.sh builds it"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split(":", 1) for l in out.stdout.splitlines() if ":" in l)
    for tech in ("NEE", "ReSTIR DI"):
        assert int(lines[f"{tech} scene uploads (A)"]) == 1
        assert int(lines[f"{tech} material updates (A)"]) >= 1
        assert lines[f"{tech} images identical"].strip() == "yes"
