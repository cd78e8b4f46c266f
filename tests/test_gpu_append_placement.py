"""fyprt_set_append_placement(ctx, 1) on the device: the search kernel's choice against the placement rule restated in numpy
(placement_ref.place) and against a host-only context, the link and the path's refit on two exports, and the state after a placed
append checked as test_gpu_append.py checks a graft at the root: the oracle walking the exported tree, and a context that uploads the
combined scene.  Every comparison is bit-exact.
  1 the report and the link, three builders      2 the path's refit equals a full refit      3 frames, ray queries, radiance queries
  4 after a device transform edit and a partial refit      5 device memory      6 the C++ facade"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import placement_ref as pr
from append_common import add_emitter_material, append_patch, check_graft
from common import SCENES, bits_equal, check_bvh_invariants, settings_for, struct_equal
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

W, H = 128, 80
# the positions of test_append_placement_cpu.py: by the numpy rule a pair at cornell's root node and a slot two levels down; pairs three
# levels down in hall_small
SHIFTS = {"cornell": ((0.0, 0.0, 0.0), (0.3, -0.7, 0.8)), "hall_small": ((0.0, 0.0, 0.0), (-4.0, 0.5, -3.0))}


def _ctx(sc, cam, key12=0, mode=1, device=0):
    ctx = capi.Context(device)
    if device >= 0:
        ctx.set_tuning(12, key12)
        ctx.resize(W, H)
    ctx.upload_scene(sc)
    if device >= 0:
        ctx.set_camera(cam)
    ctx.set_append_placement(mode)
    return ctx


def _placed_append(ctx, sc, cam, name, n, material, shift):
    """One mode-1 append checked against the numpy rule on the scene's current vertices, the link rule and the invariants."""
    before = ctx.export_bvh()
    t0 = len(sc.triangles)
    m = append_patch(sc, cam, name, n, material, shift=shift)
    ctx.append_meshes(sc, m)
    after = ctx.export_bvh()
    pl = ctx.last_append_placement()
    want = pr.place(before, sc.world_vertices["position"], sc.triangles, (t0, t0 + n), pr.sub_levels(before, after, n))
    assert pr.report_tuple(pl) == want, (pr.report_tuple(pl), want)
    assert pl.mode == 1 and pl.levels_before == before["max_stack"] and pl.levels_after == after["max_stack"]
    if pl.kind in (pr.SLOT, pr.PAIR):
        pr.check_placed_graft(before, after, n, pl)
    else:
        check_graft(before, after, n)
    check_bvh_invariants(after, sc, require_wide=False)
    return before, after, pl, m


# ---- 1
@pytest.mark.parametrize("key12", [0, 1, 2])
@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 300])
@pytest.mark.parametrize("name", ["cornell", "hall_small"])
def test_1_report_equals_the_numpy_rule_and_the_host(name, n, k, key12):
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam, key12)
    _, _, pl, _ = _placed_append(ctx, sc, cam, name, n, 0, SHIFTS[name][k])
    ctx.close()
    if key12 != 0:
        return                                               # a device-built tree is another tree than the host-only context's: no common case
    sh = mk_scene()
    host = _ctx(sh, cam, device=-1)
    host.append_meshes(sh, append_patch(sh, cam, name, n, 0, shift=SHIFTS[name][k]))
    ph = host.last_append_placement()
    host.close()
    assert pl.cost_bits == ph.cost_bits and (pl.kind, pl.node, pl.slot, pl.depth) == (ph.kind, ph.node, ph.slot, ph.depth)


# ---- 2
@pytest.mark.parametrize("name,n,k", [("cornell", 5, 1), ("cornell", 300, 0), ("hall_small", 1, 1), ("hall_small", 300, 0)])
def test_2_the_paths_refit_equals_a_full_refit(name, n, k):
    """The full pass rewrites every node from its children: after it the tree must hold the bytes the placed graft left."""
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = _ctx(sc, cam)
    ctx.update_vertices(sc)                                  # unchanged vertices: every node now carries the refit pass's bytes
    _placed_append(ctx, sc, cam, name, n, 0, SHIFTS[name][k])
    placed = ctx.export_bvh()
    ctx.update_vertices(sc)
    full = ctx.export_bvh()
    assert placed["root"] == full["root"] and placed["max_stack"] == full["max_stack"]
    assert placed["nodes"].tobytes() == full["nodes"].tobytes() and placed["tris"].tobytes() == full["tris"].tobytes()
    ctx.close()


# ---- 3
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


def _same_lights(a, b, n_meshes):
    la, lb = a.export_lighttrees(n_meshes), b.export_lighttrees(n_meshes)
    for key in ("tlas", "blas"):
        assert len(la[key]) == len(lb[key]) and struct_equal(la[key], lb[key]).all(), key
    assert la["tlas_root"] == lb["tlas_root"]
    for key in ("blas_first", "blas_count", "blas_root"):
        assert np.array_equal(la[key], lb[key]), key
    assert np.array_equal(a.export_emissive(), b.export_emissive())


@pytest.mark.parametrize("name,k,key12", [("cornell", 1, 0), ("cornell", 0, 2), ("hall_small", 1, 0), ("hall_small", 0, 1)])
def test_3_frames_after_a_placed_append_equal_the_oracle(oracle_built, name, k, key12):
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    ctx = _ctx(sc, cam, key12)
    orc = _oracle(sc, cam, ctx.export_bvh())
    _frames_equal(ctx, orc, capi.RESTIR_DI, (1, 2), "before")                # history the append must carry
    _, after, pl, _ = _placed_append(ctx, sc, cam, name, 300, light, SHIFTS[name][k])
    assert pl.kind in (pr.SLOT, pr.PAIR)
    orc = _oracle(sc, cam, after, adopt=orc)
    _frames_equal(ctx, orc, capi.RESTIR_DI, (10, 11), "after")
    _frames_equal(ctx, orc, capi.NEE, (12, 13), "after")
    orc.close()
    fresh = _ctx(sc, cam, key12, mode=0)
    _same_lights(ctx, fresh, len(sc.meshes))
    fresh.close()
    ctx.close()


def _camera_rays(cam):
    """(origins, directions) of the frame's pixels in row-major order, directions from the oracle's camera."""
    from fypraytracer_amd import scenes
    from oraclelib import Oracle
    orc = Oracle(scenes.cornell_box(), W, H)                  # (only its camera is used)
    orc.set_camera(cam)
    out3 = np.zeros(3, np.float32)
    d = np.zeros((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            orc.lib.orc_ray_direction(orc.h, x, y, out3.ctypes.data_as(C.c_void_p))
            d[y, x] = out3
    orc.close()
    d = d.reshape(-1, 3)
    return np.broadcast_to(np.asarray(cam.position, np.float32), d.shape).copy(), d


@pytest.mark.parametrize("key12", [0, 2])
def test_3_ray_and_radiance_queries_on_the_placed_tree(oracle_built, key12):
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    ctx = _ctx(sc, cam, key12)
    t_old = len(sc.triangles)
    kinds = set()
    for step, (n, shift) in enumerate(((1, SHIFTS["cornell"][1]), (300, SHIFTS["cornell"][0]), (5, (0.5, 0.6, -0.3)))):
        kinds.add(_placed_append(ctx, sc, cam, "cornell", n, light if n == 5 else 4, shift)[2].kind)
    assert {pr.SLOT, pr.PAIR} <= kinds
    o, d = _camera_rays(cam)
    got = ctx.trace_rays(o, d)
    occ = ctx.trace_rays(o, d, occluded=True)
    bvh = ctx.export_bvh()
    orc = Oracle(sc, 8, 8)
    orc.use_product_bvh(bvh)
    ref = np.zeros(len(d), dtype=capi.PAYLOAD_DTYPE)
    for i in range(len(d)):
        ref[i] = orc.trace(o[i], d[i])[0]
    orc.close()
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))
    assert np.array_equal(occ, ref["objectIndex"] >= 0)
    assert (ref["objectIndex"] >= t_old).sum() > 50                          # the camera sees the appended meshes
    fresh = _ctx(sc, cam, key12, mode=0)
    assert np.array_equal(fresh.trace_rays(o, d)["hitDistance"].view(np.uint32), got["hitDistance"].view(np.uint32))
    fresh.close()
    # a radiance query of the frame's own camera rays reproduces the frame, and the frame equals the oracle on the exported tree
    orc = _oracle(sc, cam, bvh)
    for tech in (capi.NEE, capi.BRDF_SAMPLING):
        st = settings_for(tech, to_accumulate=0)
        ctx.reset_frame_index()
        ctx.render(st)
        orc.reset_frame_index()
        orc.render(st)
        acc = ctx.readback()[1]
        assert bits_equal(acc, orc.accum()).all(), tech
        rad = ctx.render_rays(o, d, st, frame_index=1)
        assert bits_equal(np.float32(0) + rad, acc.reshape(-1, 4)).all(), tech
    orc.close()
    ctx.close()


# ---- 4
@pytest.mark.parametrize("key12", [0, 2])
def test_4_after_a_transform_edit_and_a_partial_refit(key12):
    """The host's copies of tree and vertices are stale after device edits: the search reads the device's boxes.  Two contexts make
    the same placed appends; then one takes the full passes and one the partial refit."""
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    a, b = _ctx(sc, cam, key12), _ctx(sc, cam, key12)
    for c in (a, b):
        c.set_object_vertices(sc)
    mgr.set_mesh_transform(sc, 5, pos=(0.2, 0.0, 0.1), rotation=(0, 30, 0))
    mgr.perform_all_scene_updates(sc)
    for c in (a, b):
        c.update_transforms(sc, [5])                         # a device transform edit (the full passes)
    _, _, _, m1 = _placed_append(a, sc, cam, "cornell", 5, 4, SHIFTS["cornell"][1])
    b.append_meshes(sc, m1)
    mgr.set_mesh_transform(sc, 6, pos=(-0.1, 0.0, 0.2))
    mgr.perform_all_scene_updates(sc)
    for c in (a, b):
        c.update_mesh_vertices(sc, [6])                      # a partial refit: nodeBox follows on the way up only
        assert c.last_edit_stats().partial == 1
    _, _, pl, m2 = _placed_append(a, sc, cam, "cornell", 300, 4, (0.5, 0.6, -0.3))
    b.append_meshes(sc, m2)
    assert pr.report_tuple(b.last_append_placement()) == pr.report_tuple(pl)
    # a later edit of an old mesh and of the placed one: partial on b, the full passes on a
    mgr.set_mesh_transform(sc, 5, pos=(0.1, 0.0, 0.0), rotation=(0, 10, 0))
    mgr.set_mesh_transform(sc, m2, pos=tuple(float(v) + 0.05 for v in sc.mesh_transforms[m2]["pos"]))
    mgr.perform_all_scene_updates(sc)
    a.update_transforms(sc, [5, m2])
    b.update_mesh_vertices(sc, [5, m2])
    assert a.last_edit_stats().partial == 0 and b.last_edit_stats().partial == 1
    ea, eb = a.export_bvh(), b.export_bvh()
    assert ea["root"] == eb["root"] and ea["nodes"].tobytes() == eb["nodes"].tobytes() and ea["tris"].tobytes() == eb["tris"].tobytes()
    check_bvh_invariants(eb, sc, require_wide=False)
    a.close()
    b.close()


# ---- 5
def test_5_device_memory():
    """Over mode 0 a placed append holds the partial refit's maps and scratch for the tree it searched (include/fyprt.h:
    fyprt_update_mesh_vertices), 8 more bytes of refit list per extra node of the path, and the search's two result words, once."""
    start = capi.live_device_bytes()
    mk_scene, mk_cam = SCENES["hall_small"]
    cam = mk_cam(W, H)
    held = {}
    for mode in (0, 1):
        sc = mk_scene()
        ctx = _ctx(sc, cam, 0, mode)
        base = capi.live_device_bytes()
        extra = []
        for n, shift in ((300, SHIFTS["hall_small"][0]), (1, SHIFTS["hall_small"][1])):
            before = ctx.export_bvh()
            ctx.append_meshes(sc, append_patch(sc, cam, "hall_small", n, 0, shift=shift))
            pl = ctx.last_append_placement()
            path = pl.depth + 1 + (1 if pl.kind == pr.PAIR else 0) if pl.kind in (pr.SLOT, pr.PAIR) else 1
            maps = 4 * (len(before["nodes"]) + len(before["tris"]) + len(sc.triangles)) + 8 * len(before["nodes"]) + 128
            extra.append((capi.live_device_bytes() - base, maps, path))
        held[mode] = extra
        ctx.close()
        assert capi.live_device_bytes() == start
    print("device bytes over the upload, per append (bytes, maps of the searched tree, path):", held)
    list_growth = 8 * (held[1][0][2] - held[0][0][2])        # the refit list is sized by the first (larger) append and kept
    for step in (0, 1):
        assert held[1][step][0] - held[0][step][0] == held[1][step][1] + 16 + list_growth, step


# ---- 6
def test_6_facade_import_in_mode_1():
    """host/mesh_import with Renderer::SetAppendPlacement(1): the import still goes through fyprt_append_meshes, the library reports the
    mode, and the frame equals a fresh renderer's up to exact-t ties (test_gpu_append.py's bar)."""
    exe = Path(capi.__file__).resolve().parent / "host" / "mesh_import"
    assert exe.exists(), "host/build.sh builds it"
    out = subprocess.run([str(exe), str(W), str(H), "1"], capture_output=True, text=True, timeout=120)
    lines = dict(l.split(":", 1) for l in out.stdout.splitlines() if ":" in l)
    for tech in ("cosine", "NEE"):
        assert int(lines[f"{tech} scene uploads (A)"]) == 1 and int(lines[f"{tech} scene appends (A)"]) == 1
        assert int(lines[f"{tech} placement mode"]) == 1 and int(lines[f"{tech} placement kind"]) in (pr.SLOT, pr.PAIR, pr.ROOT_PAIR)
        assert float(lines[f"{tech} identical pixels"]) > 0.97
    assert out.returncode == 0, out.stdout + out.stderr
