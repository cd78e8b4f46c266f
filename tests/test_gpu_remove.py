"""fyprt_remove_meshes on the device: a deletion must leave the context in the state a fyprt_upload_scene of the reduced scene reaches,
except for the acceleration structure, which is the old tree pruned bottom-up (remove_common.check_prune restates the rule).  Every
comparison is bit-exact; the yardsticks are the oracle walking the exported tree and a second context that uploads the reduced scene.
  A  frames after a removal equal the oracle on the exported tree, history carried (3 scenes x the three builders); the prune's bytes
  B  a sequence of edits mirrored on the oracle      C  lights equal a fresh upload      D  ray queries
  F  denoiser state      G  device memory      H  a two-band group      I  the C++ facade"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from append_common import add_emitter_material, append_patch, check_graft
from common import SCENES, bits_equal, check_bvh_invariants, settings_for, struct_equal
from edit_sequences import same_exports
from fypraytracer_amd import capi
from remove_common import BRANCHES, LOSES, check_prune, removed_triangles

pytestmark = pytest.mark.gpu

W, H = 128, 80
TECHS = (capi.BRUTE_FORCE, capi.NEE, capi.RESTIR_DI, capi.RESTIR_GI)
MET = set()                        # the branches of the prune rule the tests of this module met, in file order


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


def remove(ctx, sc, meshes, **kw):
    """One removal on context and scene, checked against the prune rule and the invariants; returns the branches met."""
    before = ctx.export_bvh()
    dead = removed_triangles(sc, meshes)
    ctx.remove_meshes(sc.remove_meshes_from_scene(meshes), **kw)
    after = ctx.export_bvh()
    met = check_prune(before, after, dead)
    if len(sc.triangles):
        check_bvh_invariants(after, sc, require_wide=False)
    MET.update(met)
    return met


# ---- A
@pytest.mark.parametrize("key12", [0, 1, 2])
@pytest.mark.parametrize("name", ["cornell", "hall_small", "banana"])
def test_a_frames_after_a_removal_equal_the_oracle(oracle_built, name, key12):
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam, key12)
    if name == "banana":                                                     # it removes a mesh it imported first
        light = add_emitter_material(sc)
        ctx.upload_scene(sc)
        loses = (append_patch(sc, cam, name, 5, light),)
        ctx.append_meshes(sc, loses[0])
    else:
        loses = LOSES[name]
    orc = _oracle(sc, cam, ctx.export_bvh())
    _frames_equal(ctx, orc, capi.RESTIR_DI, (1, 2), "before")                # history the removal must carry
    n_em = len(ctx.export_emissive())
    em_gone = int(np.isin(sc.init_scene_emissive_triangles(), np.nonzero(removed_triangles(sc, loses))[0]).sum())
    remove(ctx, sc, loses)
    assert len(ctx.export_emissive()) == n_em - em_gone
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    for k, tech in enumerate(TECHS):
        _frames_equal(ctx, orc, tech, (10 + 2 * k, 11 + 2 * k), "after")
    orc.close()
    ctx.close()


@pytest.mark.parametrize("key12", [0, 2])
def test_a_edge_shapes_on_the_device(key12):
    """Grafts spliced away again (a chain of two splices, the root replaced), the root as a leaf code, the empty scene; every state
    traced against a fresh context on the reduced scene."""
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam, key12)
    d = cam.ray_directions().reshape(-1, 3)
    o = np.tile(np.asarray(cam.position, dtype=np.float32), (len(d), 1))

    def same_distances():
        fresh = _ctx(sc, cam, key12)
        assert np.array_equal(fresh.trace_rays(o, d)["hitDistance"].view(np.uint32), ctx.trace_rays(o, d)["hitDistance"].view(np.uint32))
        same_exports(ctx, fresh, len(sc.meshes))
        fresh.close()

    first = ctx.export_bvh()
    ms = []
    for k, n in enumerate((300, 1, 4, 5)):                                   # a new root that takes two more children, then another new root
        ms.append(append_patch(sc, cam, "cornell", n, 4, shift=(0.2 * k - 0.4, 0.1, 0.0)))
        ctx.append_meshes(sc, ms[-1])
    met = remove(ctx, sc, ms)
    assert {"chain of splices", "root replaced", "splice onto an inner node", "node dropped"} <= met
    back = ctx.export_bvh()
    assert back["root"] == first["root"] and len(back["nodes"]) == len(first["nodes"]) and back["tris"].tobytes() == first["tris"].tobytes()
    same_distances()
    one = append_patch(sc, cam, "cornell", 1, 4)
    ctx.append_meshes(sc, one)
    met = remove(ctx, sc, tuple(range(one)))                                 # all but a one-triangle mesh: the root becomes a leaf code
    b = ctx.export_bvh()
    assert b["root"] == ~0 and len(b["nodes"]) == 0 and len(b["tris"]) == 1
    same_distances()
    before = ctx.export_bvh()
    ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 300, 4, shift=(0.3, 0, 0)))
    check_graft(before, ctx.export_bvh(), 300)
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    same_distances()
    remove(ctx, sc, (0, 1))                                                  # everything
    b = ctx.export_bvh()
    assert (len(b["nodes"]), len(b["tris"]), b["root"], b["max_stack"]) == (0, 0, 0, 0)
    assert (ctx.trace_rays(o, d)["objectIndex"] < 0).all()
    ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 40, 4))           # the empty tree takes a graft
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    same_distances()
    ctx.close()


def test_a_more_intervals_than_the_lds_table():
    """The interval tables stay in LDS up to 1024 intervals (rt_prune.h: kPruneLds); beyond that the kernels search the global copy.
    2100 one-triangle meshes lose every other one: 1050 triangle intervals and 1050 vertex intervals."""
    from append_common import patch
    from fypraytracer_amd.scene import Scene
    mk_scene, mk_cam = SCENES["cornell"]
    cam = mk_cam(W, H)
    sc = Scene()
    sc.materials = mk_scene().materials
    p, nrm, uv, idx = patch(2100, 1.6)
    for k in range(2100):
        sc.add_new_mesh_to_scene(p[3 * k:3 * k + 3], nrm[:3], uv[:3], idx[:1], pos=(0.0, 0.0, 0.5), material_index=3 if k % 7 == 0 else k % 3)
    sc.init_scene_emissive_triangles()
    d = cam.ray_directions().reshape(-1, 3)
    o = np.tile(np.asarray(cam.position, dtype=np.float32), (len(d), 1))
    for key12 in (0, 2):
        s2 = Scene(materials=sc.materials, world_vertices=sc.world_vertices.copy(), vertices=sc.vertices.copy(), triangles=sc.triangles.copy(),
                   meshes=list(sc.meshes), mesh_transforms=[dict(t) for t in sc.mesh_transforms], emissive_triangles=sc.emissive_triangles.copy())
        ctx = _ctx(s2, cam, key12)
        remove(ctx, s2, range(0, 2100, 2))
        fresh = _ctx(s2, cam, key12)
        same_exports(ctx, fresh, len(s2.meshes))
        got = ctx.trace_rays(o, d)
        assert np.array_equal(fresh.trace_rays(o, d)["hitDistance"].view(np.uint32), got["hitDistance"].view(np.uint32))
        assert (got["objectIndex"] >= 0).sum() > 500
        fresh.close()
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
    m = append_patch(sc, cam, "cornell", 40, light)
    ctx.append_meshes(sc, m)                                                 # with object vertices: the context holds them
    remove(ctx, sc, (5,))                                                    # an OLD mesh (the tall box); the ranges given are its own
    m -= 1
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (3, 4), "removal")
    _frames_equal(ctx, orc, capi.NEE, (5,), "removal")
    mgr.set_mesh_transform(sc, m, pos=(0.1, 0.3, 1.0), rotation=(10, 25, 0))
    mgr.set_mesh_transform(sc, 5, pos=(-0.1, 0.0, 0.2))                      # the short box, mesh 6 before
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_transforms(sc, [m, 5])                                        # the compacted object copy and mesh_first_vertex
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (6, 7), "transforms")
    a, n = sc.mesh_transforms[5]["vertex_start"], sc.mesh_transforms[5]["vertex_count"]
    sc.world_vertices["position"][a:a + n] += np.float32(0.05)               # the vertex remap of triIdx: moved reduced vertices
    ctx.update_vertices(sc)
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (8, 9), "vertices")
    remove(ctx, sc, (m,), with_vertex_ranges=False)                          # the imported mesh; its own range from the copy the context holds
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (10, 11), "second removal")
    m2 = append_patch(sc, cam, "cornell", 7, light, shift=(-0.5, -0.3, 0.1))
    ctx.append_meshes(sc, m2)
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    mgr.set_mesh_transform(sc, m2, pos=(-0.4, -0.2, 0.9))
    mgr.perform_all_scene_updates(sc)
    ctx.update_transforms(sc, [m2])
    orc = _oracle(sc, cam, ctx.export_bvh(), adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (12, 13), "append again")
    _frames_equal(ctx, orc, capi.NEE, (14,), "append again")
    orc.close()
    ctx.close()


# ---- C
@pytest.mark.parametrize("name,loses", [("hall_small", (25,)), ("cornell", (5,)), ("hall_small", (3, 13, 22))])
def test_c_lights_equal_an_upload(name, loses):
    """Removing an emitter; removing only non-emitters in front of the emitters (a pure index shift)."""
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    a = _ctx(sc, cam)
    remove(a, sc, loses)
    b = _ctx(sc, cam)
    same_exports(a, b, len(sc.meshes))
    a.close()
    b.close()


def test_c_no_emitter_left():
    mk_scene, mk_cam = SCENES["hall_small"]
    sc, cam = mk_scene(), mk_cam(W, H)
    a = _ctx(sc, cam)
    remove(a, sc, (24, 25, 26, 27))
    assert len(a.export_emissive()) == 0
    b = _ctx(sc, cam)
    same_exports(a, b, len(sc.meshes))
    b.close()
    for tech in (capi.RESTIR_DI, capi.NEE):
        with pytest.raises(capi.FyprtError, match="error -4"):
            a.render(settings_for(tech))
    a.render(settings_for(capi.BRDF_SAMPLING))
    a.close()


# ---- D
@pytest.mark.parametrize("key12", [0, 2])
def test_d_ray_queries_on_the_pruned_tree(oracle_built, key12):
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam, key12)
    for step, n in enumerate((5, 300, 4)):
        ctx.append_meshes(sc, append_patch(sc, cam, "cornell", n, 4, shift=(0.3 * step - 0.45, 0.2, 0.05 * step)))
    remove(ctx, sc, (6, 8, 2))                                               # the short box, the 5-triangle patch, the back wall
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
    assert (ref["objectIndex"] < 0).sum() > 50 and (ref["objectIndex"] >= 18).sum() > 50      # rays leave through the missing wall, others see the 300-patch
    fresh = _ctx(sc, cam, key12)
    assert np.array_equal(fresh.trace_rays(o, d)["hitDistance"].view(np.uint32), got["hitDistance"].view(np.uint32))
    fresh.close()
    ctx.close()


# ---- F
def test_f_denoiser_state_after_a_removal():
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
        c.remove_meshes(s.remove_meshes_from_scene([6]))
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
    m = append_patch(sc, cam, "hall_small", 300, 0)
    ctx.append_meshes(sc, m)
    grown = capi.live_device_bytes()
    remove(ctx, sc, (m,))
    after = capi.live_device_bytes()
    assert after <= grown                                                    # the capacities are kept, the call's scratch is gone
    remove(ctx, sc, LOSES["hall_small"])
    assert capi.live_device_bytes() <= after
    ctx.append_meshes(sc, append_patch(sc, cam, "hall_small", 300, 0))
    assert capi.live_device_bytes() <= after                                 # an append of the removed size fits without growing
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    ctx.close()
    assert capi.live_device_bytes() == start


# ---- H
def test_h_group_members_remove_between_frames():
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
                rec = sc.remove_meshes_from_scene([5, 2])
                if grp:
                    grp.synchronize()
                for c in ctxs:
                    c.remove_meshes(rec)
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
def test_i_facade_removes_without_a_second_upload():
    """host/mesh_remove: a mesh removed through the C++ facade next to a fresh renderer on the reduced scene.  The two trees differ, so the
    frames may differ where two triangles are hit at exactly the same distance: the bar is test I's of test_gpu_append.py for a
    differently built tree.  Checked before relying on it: the oracle on the two exported trees of this scene (the harness's Cornell
    with the 12 x 12 sheet, the left wall removed; pruned tree against freshly built one) gives 1.0 for both techniques."""
    exe = Path(capi.__file__).resolve().parent / "host" / "mesh_remove"
    assert exe.exists(), "host/build.sh builds it"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = dict(l.split(":", 1) for l in out.stdout.splitlines() if ":" in l)
    for tech in ("cosine", "NEE"):
        assert int(lines[f"{tech} scene uploads (A)"]) == 1
        assert int(lines[f"{tech} scene removals (A)"]) == 1
        assert float(lines[f"{tech} identical pixels"]) > 0.97
    assert out.returncode == 0, out.stdout + out.stderr


def test_every_branch_of_the_prune_rule_was_met():
    """(runs last in this file)  The device builders mix the meshes' triangles in their leaves: "leaf partly emptied" is met here."""
    assert MET >= set(BRANCHES), set(BRANCHES) - MET
