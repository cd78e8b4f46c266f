"""fyprt_append_meshes / fyprt_append_textures on the device: an import (vertices, triangles, meshes or textures pushed onto the end of the
scene) must leave the context in the state a fyprt_upload_scene of the combined scene reaches, except for the acceleration structure,
which takes a sub-tree over the new triangles at its root.  Every comparison is bit-exact; the yardsticks are the oracle walking the
exported tree and a second context that uploads the combined scene.
  A  frames after an append equal the oracle on the exported tree, history carried (3 scenes x the three builders); the graft's bytes
  B  a sequence of edits mirrored on the oracle      C  lights equal a fresh upload      D  ray queries
  E  textures      F  denoiser state      G  device memory      H  a two-band group      I  the C++ facade"""
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

from append_common import SIZES, add_emitter_material, append_patch, check_graft
from common import SCENES, bits_equal, check_bvh_invariants, settings_for, struct_equal
from edit_sequences import same_exports
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

W, H = 128, 80
TECHS = (capi.BRUTE_FORCE, capi.NEE, capi.RESTIR_DI, capi.RESTIR_GI)
# which scene gets which append: size and whether it emits
APPEND = {"cornell": (300, True), "hall_small": (300, False), "banana": (5, True)}


def _ctx(sc, cam, key12=0):
    ctx = capi.Context(0)
    ctx.set_tuning(12, key12)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    return ctx


def _oracle(sc, cam, bvh, adopt=None):
    from oraclelib import Oracle
    orc = Oracle(sc, W, H)
    orc.set_camera(cam)
    if adopt is not None:
        orc.adopt_frame(adopt)
        adopt.close()
    orc.use_product_bvh(bvh)
    return orc


def _frames_equal(ctx, orc, tech, seeds, tag):
    st = settings_for(tech)
    for seed in seeds:
        st.rand_seed = seed
        ctx.render(st)
        orc.render(st)
        img, acc = ctx.readback()
        assert bits_equal(acc, orc.accum()).all() and np.array_equal(img, orc.image()), (tag, tech, seed)
        if tech == capi.RESTIR_DI:
            for buf in (capi.BUF_DI, capi.BUF_DI_PREV):
                assert struct_equal(ctx.read_buffer(buf), orc.read_buffer(buf)).all(), (tag, seed, buf)


# ---- A
@pytest.mark.parametrize("key12", [0, 1, 2])
@pytest.mark.parametrize("name", ["cornell", "hall_small", "banana"])
def test_a_frames_after_an_append_equal_the_oracle(oracle_built, name, key12):
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    n, emits = APPEND[name]
    mat = add_emitter_material(sc) if emits else 0
    ctx = _ctx(sc, cam, key12)
    orc = _oracle(sc, cam, ctx.export_bvh())
    _frames_equal(ctx, orc, capi.RESTIR_DI, (1, 2), "before")                # history the append must carry
    before = ctx.export_bvh()
    n_em = len(ctx.export_emissive())
    m = append_patch(sc, cam, name, n, mat)
    ctx.append_meshes(sc, m)
    after = ctx.export_bvh()
    check_bvh_invariants(after, sc, require_wide=False)
    check_graft(before, after, n)
    assert len(ctx.export_emissive()) == n_em + (n if emits else 0)
    orc = _oracle(sc, cam, after, adopt=orc)
    for k, tech in enumerate(TECHS):
        _frames_equal(ctx, orc, tech, (10 + 2 * k, 11 + 2 * k), "after")
    orc.close()
    ctx.close()


@pytest.mark.parametrize("key12", [0, 2])
def test_a_graft_after_a_device_transform(key12):
    """The host's copy of the tree and of the vertices is stale after fyprt_update_transforms: the graft works on the device's."""
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam, key12)
    ctx.set_object_vertices(sc)
    sc.manager().perform_all_scene_updates(sc)
    sc.manager().set_mesh_transform(sc, 5, pos=(0.2, 0.0, 0.1), rotation=(0, 30, 0))
    sc.manager().perform_all_scene_updates(sc)
    ctx.update_transforms(sc, [5])
    for step, n in enumerate(SIZES):
        before = ctx.export_bvh()
        ctx.append_meshes(sc, append_patch(sc, cam, "cornell", n, 4, shift=(0.3 * step - 0.45, 0.2, 0.05 * step)))
        after = ctx.export_bvh()
        check_bvh_invariants(after, sc, require_wide=False)
        check_graft(before, after, n)
    ctx.close()


# ---- B
def test_b_sequence_of_edits_mirrored_on_the_oracle(oracle_built):
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    ctx = _ctx(sc, cam)
    ctx.set_object_vertices(sc)
    orc = _oracle(sc, cam, ctx.export_bvh())
    _frames_equal(ctx, orc, capi.RESTIR_DI, (1, 2), "upload")
    m = append_patch(sc, cam, "cornell", 40, 4)
    ctx.append_meshes(sc, m)                                                 # with object vertices: the context holds them
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (3, 4), "append")
    mgr.set_mesh_transform(sc, m, pos=(0.1, 0.3, 1.0), rotation=(10, 25, 0))
    mgr.set_mesh_transform(sc, 6, pos=(-0.1, 0.0, 0.2))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_transforms(sc, [m, 6])
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (5, 6), "transforms")
    mgr.set_mesh_material(sc, m, light)
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_materials(sc, [m])
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (7, 8), "materials")
    _frames_equal(ctx, orc, capi.NEE, (9,), "materials")
    m2 = append_patch(sc, cam, "cornell", 7, light, shift=(-0.5, -0.3, 0.1))
    ctx.append_meshes(sc, m2)
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (10, 11), "second append")
    _frames_equal(ctx, orc, capi.NEE, (12,), "second append")
    mgr.set_mesh_transform(sc, m2, pos=(-0.4, -0.2, 0.9))                     # ... and the second import moves too
    mgr.perform_all_scene_updates(sc)
    ctx.update_transforms(sc, [m2])
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (13,), "last")
    orc.close()
    ctx.close()


# ---- C
@pytest.mark.parametrize("name,n", [("cornell", 5), ("hall_small", 300)])
def test_c_emissive_append_equals_an_upload_in_its_lights(name, n):
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    a = _ctx(sc, cam)
    a.append_meshes(sc, append_patch(sc, cam, name, n, light))
    a.append_meshes(sc, append_patch(sc, cam, name, 4, 0, shift=(0.1, 0.1, 0.0)))    # no emitter: the lights stay
    b = _ctx(sc, cam)
    same_exports(a, b, len(sc.meshes))
    a.close()
    b.close()


# ---- D
@pytest.mark.parametrize("key12", [0, 2])
def test_d_ray_queries_on_the_grafted_tree(oracle_built, key12):
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam, key12)
    t_old = len(sc.triangles)
    for step, n in enumerate(SIZES):
        ctx.append_meshes(sc, append_patch(sc, cam, "cornell", n, 4, shift=(0.3 * step - 0.45, 0.2, 0.05 * step)))
    d = cam.ray_directions().reshape(-1, 3)
    o = np.tile(np.asarray(cam.position, dtype=np.float32), (len(d), 1))
    got = ctx.trace_rays(o, d)
    occ = ctx.trace_rays(o, d, occluded=True)
    orc = Oracle(sc, 8, 8)
    orc.use_product_bvh(ctx.export_bvh())
    ref = np.zeros(len(d), dtype=capi.PAYLOAD_DTYPE)
    for i in range(len(d)):
        ref[i] = orc.trace(o[i], d[i])[0]
    orc.close()
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))
    assert np.array_equal(occ, ref["objectIndex"] >= 0)
    assert (ref["objectIndex"] >= t_old).sum() > 50                          # the camera sees the appended meshes
    fresh = _ctx(sc, cam, key12)
    assert np.array_equal(fresh.trace_rays(o, d)["hitDistance"].view(np.uint32), got["hitDistance"].view(np.uint32))
    fresh.close()
    ctx.close()


# ---- E
def _texture(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 24, (h, w), dtype=np.uint32) | np.uint32(0xFF000000)).astype(np.uint32)


def test_e_texture_append_then_material_edit_equals_a_reupload():
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    a, b = _ctx(sc, cam), _ctx(sc, cam)
    st = settings_for(capi.RESTIR_DI)
    for f in range(2):
        st.rand_seed = f + 1
        a.render(st)
        b.render(st)
    before = a.export_bvh()
    texs = [_texture(16, 24, 1), _texture(7, 5, 2)]
    a.append_textures(texs)
    sc.textures = texs
    sc.materials[0] = replace(sc.materials[0], is_use_albedo_map=True, albedo_map_index=1)
    sc.materials[4] = replace(sc.materials[4], is_use_albedo_map=True, albedo_map_index=0)
    a.update_materials(sc)
    b.upload_scene(sc)
    ba, bb = a.export_bvh(), b.export_bvh()
    for k in ("nodes", "tris"):
        assert ba[k].tobytes() == before[k].tobytes() == bb[k].tobytes(), k
    same_exports(a, b, len(sc.meshes))
    for tech in (capi.RESTIR_DI, capi.BRDF_SAMPLING, capi.NEE):
        st = settings_for(tech)
        for f in range(2):
            st.rand_seed = 10 + f
            a.render(st)
            b.render(st)
            (ia, aa), (ib, ab) = a.readback(), b.readback()
            assert np.array_equal(ia, ib) and bits_equal(aa, ab).all(), (tech, f)
    a.close()
    b.close()


def test_e_plain_texture_append_keeps_the_frame_denoisable():
    mk_scene, mk_cam = SCENES["banana"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam)
    ctx.render(settings_for(capi.BRDF_SAMPLING))
    img0, rad0 = ctx.denoise()
    ctx.denoise_temporal()
    ctx.append_textures([_texture(9, 9, 3)])
    img1, rad1 = ctx.denoise()
    assert np.array_equal(img0, img1) and bits_equal(rad0, rad1).all()
    ctx.read_buffer(capi.BUF_TEMPORAL)                                       # the history is still there
    # a material that already points at the new slot shaded as solid colour so far: that append is a material edit
    sc.materials[1] = replace(sc.materials[1], is_use_albedo_map=True, albedo_map_index=2)
    ctx.update_materials(sc)
    ctx.render(settings_for(capi.BRDF_SAMPLING))
    ctx.denoise()
    ctx.append_textures([_texture(4, 4, 4)])
    with pytest.raises(capi.FyprtError, match="error -3"):
        ctx.denoise()
    ctx.close()


# ---- F
def test_f_denoiser_state_after_an_append():
    mk_scene, mk_cam = SCENES["cornell"]
    sa, sb, cam = mk_scene(), mk_scene(), mk_cam(W, H)
    a, b = _ctx(sa, cam), _ctx(sb, cam)
    a.denoise_temporal_set_motion(True)
    b.denoise_temporal_set_motion(True)
    st = settings_for(capi.BRDF_SAMPLING)
    a.render(st)
    b.render(st)
    a.denoise()
    a.denoise_temporal()                                                     # a holds a history, b does not
    a.read_buffer(capi.BUF_TEMPORAL)
    for c, s in ((a, sa), (b, sb)):
        c.append_meshes(s, append_patch(s, cam, "cornell", 40, 4))
    for call in (a.denoise, a.denoise_temporal, lambda: a.read_buffer(capi.BUF_TEMPORAL)):
        with pytest.raises(capi.FyprtError, match="error -3"):
            call()
    st.rand_seed = 2
    a.render(st)
    b.render(st)
    (ia, ra), (ib, rb) = a.denoise_temporal(), b.denoise_temporal()          # a's call behaves as a first call: b's is one
    assert np.array_equal(ia, ib) and bits_equal(ra, rb).all()
    assert struct_equal(a.read_buffer(capi.BUF_TEMPORAL), b.read_buffer(capi.BUF_TEMPORAL)).all()
    a.close()
    b.close()


# ---- G
@pytest.mark.parametrize("key12", [0, 2])
def test_g_device_memory(key12):
    start = capi.live_device_bytes()
    mk_scene, mk_cam = SCENES["hall_small"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam, key12)
    uploaded = capi.live_device_bytes()
    ctx.append_meshes(sc, append_patch(sc, cam, "hall_small", 300, 0))
    large = capi.live_device_bytes()
    assert large > uploaded                                                  # the arrays were full: their capacity doubled
    ctx.append_meshes(sc, append_patch(sc, cam, "hall_small", 5, 0, shift=(0.0, 1.5, 0.0)))
    assert capi.live_device_bytes() == large                                 # the capacity holds
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    ctx.close()
    assert capi.live_device_bytes() == start


# ---- H
def test_h_group_members_append_between_frames():
    mk_scene, mk_cam = SCENES["cornell"]
    cam = mk_cam(W, H)
    bounds = [0, 40, H]

    def run(members):
        sc = mk_scene()
        light = add_emitter_material(sc)
        ctxs = [_ctx(sc, cam) for _ in range(members)]
        grp = capi.Group(ctxs, bounds, halo_mode=1) if members > 1 else None
        st = settings_for(capi.RESTIR_DI)
        outs = []
        for f in range(4):
            if f == 2:
                m = append_patch(sc, cam, "cornell", 40, light)
                if grp:
                    grp.synchronize()
                for c in ctxs:
                    c.append_meshes(sc, m)
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


# ---- I
def test_i_facade_appends_without_a_second_upload():
    """host/mesh_import: a texture and a mesh imported through the C++ facade next to a fresh renderer on the grown scene.  The two trees
    differ, so the frames may differ where two triangles are hit at exactly the same distance: the bar is test_gpu_refit.py's for a
    differently built tree (the oracle on the two exported trees of this scene gives 1.0 for both techniques)."""
    exe = Path(capi.__file__).resolve().parent / "host" / "mesh_import"
    assert exe.exists(), "host/build.sh builds it"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = dict(l.split(":", 1) for l in out.stdout.splitlines() if ":" in l)
    for tech in ("cosine", "NEE"):
        assert int(lines[f"{tech} scene uploads (A)"]) == 1
        assert int(lines[f"{tech} scene appends (A)"]) == 1
        assert float(lines[f"{tech} identical pixels"]) > 0.97
    assert out.returncode == 0, out.stdout + out.stderr
