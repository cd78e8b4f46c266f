"""The partial refit on the device: fyprt_update_mesh_vertices and fyprt_update_transforms with tuning key 22 = 1 against the full passes
(fyprt_update_vertices; fyprt_update_transforms with key 22 = 0), which tests/test_gpu_refit.py and test_gpu_transforms.py check against
the oracle.  On a tree a full refit has run on the two leave byte-identical exports; on any tree the partial one rewrites exactly the
nodes of partial_refit_common.expected_dirty_nodes and the leaf records of the moved triangles, and every frame agrees with the oracle
walking the exported tree.
The device builders (tuning key 12 = 1, 2) number their nodes in the order their workgroups arrive, so two contexts do not build the same
array twice.  Where a test compares the two paths on such a tree, ONE context takes both, one after the other (class Twin): the full
path first, then a full refit back to the old vertices, which leaves the very bytes the first edit started from, then the partial path,
each from zeroed frame state and one frame of the old geometry.  On host-built trees two contexts run side by side."""
import types
import ctypes as C

import numpy as np
import pytest

from append_common import add_emitter_material, append_patch
from common import SCENES, bits_equal, check_bvh_invariants, settings_for, struct_equal
from fypraytracer_amd import capi
from fypraytracer_amd.scene import Material, Scene
from partial_refit_common import MOVES, expected_dirty_nodes, mesh_triangles

pytestmark = pytest.mark.gpu

W, H = 128, 80
EINVAL, ESTATE = -1, -3
CALLS = ("update_mesh_vertices", "update_transforms")


def _scene(name):
    mk_scene, mk_cam = SCENES[name]
    sc = mk_scene()
    sc.manager().perform_all_scene_updates(sc)               # the reference's first call (queues start non-empty)
    return sc, sc.manager(), mk_cam(W, H)


def _ctx(sc, cam, key12=0, refit_first=False):
    ctx = capi.Context(0)
    ctx.set_tuning(12, key12)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    ctx.set_object_vertices(sc)
    if refit_first:
        ctx.update_vertices(sc)                              # unmoved vertices: a full refit has written every node
    return ctx


def _move(sc, mgr, moves):
    moved = []
    for mesh, tr in moves:
        m = mesh % len(sc.meshes)
        mgr.set_mesh_transform(sc, m, **tr)
        moved.append(m)
    assert mgr.perform_all_scene_updates(sc) is True
    return moved


def _partial(ctx, sc, meshes, call="update_mesh_vertices"):
    if call == "update_mesh_vertices":
        ctx.update_mesh_vertices(sc, meshes)
    else:
        ctx.set_tuning(22, 1)
        ctx.update_transforms(sc, meshes)
        ctx.set_tuning(22, 0)
    return ctx.last_edit_stats()


def _same_bvh(ba, bb):
    assert ba["root"] == bb["root"] and ba["max_stack"] == bb["max_stack"]
    assert ba["nodes"].tobytes() == bb["nodes"].tobytes() and ba["tris"].tobytes() == bb["tris"].tobytes()


def _same_trees(a, b):
    ba, bb = a.export_bvh(), b.export_bvh()
    _same_bvh(ba, bb)
    return bb


def _observe(ctx, n_meshes, techs, first_seed):
    """Everything of the context's state an edit can reach: the exports and, bit for bit, two frames of every technique."""
    out = {"bvh": ctx.export_bvh(), "lights": ctx.export_lighttrees(n_meshes), "emissive": ctx.export_emissive(), "frames": []}
    for tech in techs:
        st = settings_for(tech)
        for f in range(2):
            st.rand_seed = first_seed + f
            ctx.render(st)
            out["frames"].append((tech, f) + ctx.readback())
        if tech == capi.RESTIR_DI:
            out["frames"].append((tech, "reservoirs", ctx.read_buffer(capi.BUF_DI), ctx.read_buffer(capi.BUF_DI_PREV)))
    return out


def _same_outcome(x, y, tag=""):
    _same_bvh(x["bvh"], y["bvh"])
    la, lb = x["lights"], y["lights"]
    for k in ("tlas", "blas"):
        assert len(la[k]) == len(lb[k]) and struct_equal(la[k], lb[k]).all(), (tag, k)
    assert la["tlas_root"] == lb["tlas_root"]
    for k in ("blas_first", "blas_count", "blas_root"):
        assert np.array_equal(la[k], lb[k]), (tag, k)
    assert np.array_equal(x["emissive"], y["emissive"])
    assert len(x["frames"]) == len(y["frames"])
    for fa, fb in zip(x["frames"], y["frames"]):
        assert fa[:2] == fb[:2]
        if fa[1] == "reservoirs":
            assert struct_equal(fa[2], fb[2]).all() and struct_equal(fa[3], fb[3]).all(), (tag, fa[:2])
        else:
            assert np.array_equal(fa[2], fb[2]) and bits_equal(fa[3], fb[3]).all(), (tag, fa[:2])


def _full_stats(st, bvh, sc):
    assert (st.partial, st.triangles_refreshed, st.leaf_records_refreshed, st.nodes_refit) == (0, len(sc.triangles), len(bvh["tris"]), len(bvh["nodes"]))
    assert st.level_launches == (bvh["max_stack"] if len(bvh["nodes"]) else 0)


def _partial_stats(st, before, sc, meshes):
    tris = mesh_triangles(sc, meshes)
    want = expected_dirty_nodes(before, tris)
    print(f"partial refit: {len(tris)} of {len(sc.triangles)} triangles, {st.nodes_refit} of {len(before['nodes'])} nodes (expected {len(want)}), {st.level_launches} level launches")
    assert (st.partial, st.triangles_refreshed, st.leaf_records_refreshed) == (1, len(tris), len(tris))
    assert st.nodes_refit == len(want)
    assert st.level_launches <= before["max_stack"]
    return want


class Twin:
    """Context A takes the full path, context B the partial one; on a device-built tree B is A (see the module's text).  Both start with
    one full refit of the unmoved vertices, so that a full refit has written every node."""

    def __init__(self, sc, cam, key12=0):
        self.sc, self.a = sc, _ctx(sc, cam, key12, refit_first=True)
        self.b = self.a if key12 else _ctx(sc, cam, key12, refit_first=True)
        self.seed = 2

    def both(self):
        return (self.a,) if self.b is self.a else (self.a, self.b)

    def edit(self, mgr, moves, call="update_mesh_vertices", techs=(capi.RESTIR_DI,), full=None, partial=None, listed=None, warm=capi.RESTIR_DI, tag=""):
        """The moves applied to the scene, then to A by the full path and to B by the partial one (`full` / `partial`: the calls to make
        instead of update_vertices / `call`), each from zeroed frame state + one `warm` frame of the old geometry: history the edit
        must survive identically.  Compares the outcomes and B's statistics with the dirty rule; returns (export before, export after, stats)."""
        sc, a, b = self.sc, self.a, self.b
        old = types.SimpleNamespace(world_vertices=sc.world_vertices.copy())
        before = _same_trees(a, b)
        moved = _move(sc, mgr, moves)
        listed = moved if listed is None else listed

        def prepare(c):
            c.resize(W, H)
            c.render(settings_for(warm))

        prepare(a)
        (full or (lambda c: c.update_vertices(sc)))(a)
        _full_stats(a.last_edit_stats(), before, sc)
        want = _observe(a, len(sc.meshes), techs, self.seed)
        if b is a:
            a.update_vertices(old)                           # back: a full refit writes every node from the vertices alone
            _same_bvh(a.export_bvh(), before)
        prepare(b)
        if partial:
            partial(b)
            st = b.last_edit_stats()
        else:
            st = _partial(b, sc, listed, call)
        got = _observe(b, len(sc.meshes), techs, self.seed)
        _same_outcome(want, got, tag)
        _partial_stats(st, before, sc, listed)
        check_bvh_invariants(got["bvh"], sc, require_wide=False)
        self.seed += 2
        return before, got["bvh"], st

    def close(self):
        for c in self.both():
            c.close()


# ---- 1
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("key12", [0, 1, 2])
@pytest.mark.parametrize("name", ["cornell", "hall_small", "banana"])
def test_1_equals_the_full_path(name, key12, call):
    sc, mgr, cam = _scene(name)
    tw = Twin(sc, cam, key12)
    before, _, st = tw.edit(mgr, MOVES[name], call, techs=(capi.RESTIR_DI, capi.NEE, capi.BRDF_SAMPLING))
    moved = [m % len(sc.meshes) for m, _ in MOVES[name]]
    per_mesh = [expected_dirty_nodes(before, mesh_triangles(sc, [m])) for m in moved]
    assert len(per_mesh[0] & per_mesh[1]) >= 1 and st.nodes_refit < len(per_mesh[0]) + len(per_mesh[1])     # shared ancestors: listed once
    tw.close()


# ---- 2
@pytest.mark.parametrize("name", ["cornell", "hall_small"])
def test_2_untouched_bytes_and_the_oracle(oracle_built, name):
    from oraclelib import Oracle
    sc, mgr, cam = _scene(name)
    a, b = _ctx(sc, cam), _ctx(sc, cam)                      # host-built trees no refit pass has run on
    b.render(settings_for(capi.COSINE_WEIGHTED_SAMPLING))
    before = b.export_bvh()
    moved = _move(sc, mgr, MOVES[name])
    st = _partial(b, sc, moved)
    after = b.export_bvh()
    dirty = _partial_stats(st, before, sc, moved)
    clean = np.ones(len(before["nodes"]), dtype=bool)
    clean[sorted(dirty)] = False
    assert 0 < clean.sum() < len(clean)
    assert after["nodes"][clean].tobytes() == before["nodes"][clean].tobytes()
    unmoved = ~np.isin(before["tris"]["tri"], mesh_triangles(sc, moved))
    assert np.array_equal(after["tris"]["tri"], before["tris"]["tri"])
    assert after["tris"][unmoved].tobytes() == before["tris"][unmoved].tobytes()
    # the dirty nodes carry what the full refit writes (it reads exact child boxes, as the partial one does from nodeBox)
    a.update_vertices(sc)
    full = a.export_bvh()
    assert after["nodes"][~clean].tobytes() == full["nodes"][~clean].tobytes() and after["tris"].tobytes() == full["tris"].tobytes()
    a.close()
    check_bvh_invariants(after, sc, require_wide=False)
    for tech in (capi.BRUTE_FORCE, capi.RESTIR_DI):
        b.reset_frame_index()
        orc = Oracle(sc, W, H)
        orc.set_camera(cam)
        orc.use_product_bvh(after)
        s2 = settings_for(tech)
        for f in range(2):
            s2.rand_seed = f + 1
            b.render(s2)
            orc.render(s2)
        img, acc = b.readback()
        assert bits_equal(acc, orc.accum()).all() and np.array_equal(img, orc.image()), tech
        orc.close()
    b.close()


# ---- 3
def test_3_the_empty_list_changes_nothing():
    sc, mgr, cam = _scene("cornell")
    b = _ctx(sc, cam)
    b.render(settings_for(capi.NEE))
    before = b.export_bvh()
    grown = capi.live_device_bytes()
    b.update_mesh_vertices(sc, [])
    with pytest.raises(capi.FyprtError, match="geometry edit"):
        b.last_edit_stats()                                  # nothing happened: not even an edit to report
    after = b.export_bvh()
    assert before["nodes"].tobytes() == after["nodes"].tobytes() and before["tris"].tobytes() == after["tris"].tobytes()
    assert capi.live_device_bytes() == grown
    b.denoise()                                              # the rendered frame is still the context's frame
    b.close()


@pytest.mark.parametrize("call", CALLS)
def test_3_every_mesh_listed(call):
    sc, mgr, cam = _scene("cornell")
    tw = Twin(sc, cam)
    everything = list(range(len(sc.meshes)))
    before, _, st = tw.edit(mgr, MOVES["cornell"], call, listed=everything)
    assert st.nodes_refit == len(before["nodes"]) and 1 <= st.level_launches <= before["max_stack"]
    tw.close()


def test_3_a_root_that_is_a_leaf_code():
    sc = Scene()
    sc.materials = [Material(albedo=(0.8, 0.7, 0.6), roughness=0.7)]
    q = np.array([[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2]], np.float32)
    sc.add_new_mesh_to_scene(q, np.tile(np.array([0, 1, 0], np.float32), (4, 1)), np.zeros((4, 2), np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32), material_index=0)
    sc.init_scene_emissive_triangles()
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    cam = SCENES["cornell"][1](W, H)
    cam.set_position((0.0, 1.0, 3.0))
    tw = Twin(sc, cam)
    for k, call in enumerate(CALLS):
        before, _, st = tw.edit(mgr, [(0, dict(pos=(0.3 + k, -0.2, 0.1), rotation=(5, 20, 0)))], call, techs=(capi.BRUTE_FORCE, capi.COSINE_WEIGHTED_SAMPLING),
                                 warm=capi.COSINE_WEIGHTED_SAMPLING)              # (no emitter in this scene: no ReSTIR)
        assert before["root"] < 0 and len(before["nodes"]) == 0 and len(before["tris"]) == 2
        assert (st.partial, st.triangles_refreshed, st.leaf_records_refreshed, st.nodes_refit, st.level_launches) == (1, 2, 2, 0, 0)
    tw.close()


@pytest.mark.parametrize("key12", [1, 2])
def test_3_a_leaf_that_holds_two_meshes(key12):
    sc, mgr, cam = _scene("hall_small")
    tw = Twin(sc, cam, key12)
    tree = tw.b.export_bvh()
    mesh_of_tri = np.zeros(len(sc.triangles), dtype=np.int64)
    for m, (first, count, _) in enumerate(sc.meshes):
        mesh_of_tri[first:first + count] = m
    pair = None
    for n in tree["nodes"]:
        for s in range(int(n["meta"]) & 7):
            c = int(n["child"][s])
            if c < 0 and pair is None:
                ms = sorted(set(mesh_of_tri[tree["tris"]["tri"][(~c) >> 2:((~c) >> 2) + ((~c) & 3) + 1]].tolist()))
                pair = ms[:2] if len(ms) >= 2 else None
    assert pair is not None, "the device-built hall_small tree has no leaf over two meshes"
    mover = pair[0]
    before, after, _ = tw.edit(mgr, [(mover, dict(pos=tuple(float(v) + 0.04 for v in sc.mesh_transforms[mover]["pos"])))])
    unmoved = ~np.isin(before["tris"]["tri"], mesh_triangles(sc, [mover]))
    assert after["tris"][unmoved].tobytes() == before["tris"][unmoved].tobytes()          # the other mesh's records in the shared leaf
    tw.close()


def test_3_the_same_mesh_twice_then_another():
    sc, mgr, cam = _scene("hall_small")
    tw = Twin(sc, cam)
    edits = [(13, dict(pos=(0.3, 0.0, 0.1))), (13, dict(pos=(0.5, 0.0, -0.2), rotation=(0, 15, 0))), (21, dict(pos=(0.0, 0.1, 0.3)))]
    for k, e in enumerate(edits):
        tw.edit(mgr, [e], CALLS[k % 2], tag=k)              # flags left set by the edit before would shorten this one's lists
    tw.close()


def test_3_update_transforms_with_a_mesh_listed_twice():
    sc, mgr, cam = _scene("hall_small")
    tw = Twin(sc, cam)
    first = sc.mesh_matrix(14)
    moves = [(14, dict(pos=(0.4, 0.0, 0.2), rotation=(0, 40, 0))), (2, dict(pos=(0.0, 0.05, 0.0)))]

    def transforms(key22):
        def run(c):
            mats = [first, sc.mesh_matrix(2), sc.mesh_matrix(14)]        # mesh 14 twice: its last matrix holds
            c.set_tuning(22, key22)
            c.update_transforms(sc, [14, 2, 14], mats)
            c.set_tuning(22, 0)
        return run

    _, _, st = tw.edit(mgr, moves, full=transforms(0), partial=transforms(1), techs=(capi.RESTIR_DI, capi.NEE))
    assert st.triangles_refreshed == sc.meshes[14][1] + sc.meshes[2][1]                   # distinct triangles: mesh 14 counts once
    tw.close()


@pytest.mark.parametrize("call", CALLS)
def test_3_an_emissive_mesh_moved(call):
    sc, mgr, cam = _scene("hall_small")
    tw = Twin(sc, cam)
    light = len(sc.meshes) - 2
    assert sc.materials[sc.meshes[light][2]].emission_power > 0
    # the light records feed ReSTIR DI's candidates, the light trees NEE
    tw.edit(mgr, [(light, dict(pos=(0.4, -0.5, 0.3), rotation=(0, 0, 20))), (20, dict(pos=(0.1, 0.0, 0.0)))], call, techs=(capi.RESTIR_DI, capi.NEE))
    tw.close()


# ---- 4
@pytest.mark.parametrize("key12", [0, 2])
def test_4_links_are_rebuilt_after_append_and_remove(key12):
    name = "hall_small"
    sc, mgr, cam = _scene(name)
    light = add_emitter_material(sc)
    tw = Twin(sc, cam, key12)
    tw.edit(mgr, [(3, dict(pos=(0.2, 0.0, 0.0)))], tag="links of the uploaded tree")
    new = append_patch(sc, cam, name, 300, light)
    for c in tw.both():
        c.append_meshes(sc, new)
    tw.edit(mgr, [(13, dict(pos=(0.3, 0.0, 0.1))), (new, dict(pos=tuple(float(v) + 0.1 for v in sc.mesh_transforms[new]["pos"])))], tag="after an append")
    rec = sc.remove_meshes_from_scene([15])
    for c in tw.both():
        c.remove_meshes(rec)
    tw.edit(mgr, [(12, dict(pos=(-0.2, 0.0, 0.1))), (len(sc.meshes) - 1, dict(rotation=(0, 70, 0)))], "update_transforms", tag="after a removal")
    for c in tw.both():
        c.update_vertices(sc)                                # one full refit each: the same tree, byte for byte
    _same_trees(tw.a, tw.b)
    tw.close()


# ---- 5
def test_5_temporal_denoiser_with_object_motion():
    sc, mgr, cam = _scene("cornell")
    a, b = _ctx(sc, cam, refit_first=True), _ctx(sc, cam, refit_first=True)
    st = settings_for(capi.NEE, to_accumulate=0)
    for c in (a, b):
        c.denoise_temporal_set_motion(True)
        c.render(st)
        c.denoise_temporal()
    moved = _move(sc, mgr, MOVES["cornell"])
    a.update_transforms(sc, moved)                           # key 22 = 0: the full passes
    b.update_mesh_vertices(sc, moved)
    assert b.last_edit_stats().partial == 1 and a.last_edit_stats().partial == 0
    for k in range(2):
        st.rand_seed = 5 + k
        outs = []
        for c in (a, b):
            c.render(st)
            outs.append(c.denoise_temporal() + (c.read_buffer(capi.BUF_TEMPORAL),))
        assert np.array_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1]).all(), k
        ta, tb = outs[0][2], outs[1][2]
        assert struct_equal(ta, tb).all(), k
        if k == 0:                                            # a second edit while the history is live
            moved = _move(sc, mgr, [(6, dict(pos=(-0.1, 0.0, 0.1)))])
            a.update_transforms(sc, moved)
            b.update_mesh_vertices(sc, moved)
    a.close(); b.close()


# ---- 6
def test_6_device_memory():
    start = capi.live_device_bytes()
    sc, mgr, cam = _scene("hall_small")
    b = _ctx(sc, cam)
    bvh = b.export_bvh()
    base = capi.live_device_bytes()
    moved = _move(sc, mgr, [(13, dict(pos=(0.3, 0.0, 0.1)))])
    _partial(b, sc, moved)
    n_nodes, n_leaf, n_tri = len(bvh["nodes"]), len(bvh["tris"]), len(sc.triangles)
    maps = 4 * (n_nodes + n_leaf + n_tri)                    # node -> parent, record -> node, triangle -> record
    scratch = 8 * n_nodes + 128                              # per-level lists + a flag per node, 32 list counts (include/fyprt.h)
    assert capi.live_device_bytes() - base == maps + scratch
    moved = _move(sc, mgr, [(20, dict(pos=(0.0, 0.1, 0.0)))])
    _partial(b, sc, moved, "update_transforms")
    assert capi.live_device_bytes() - base == maps + scratch
    b.close()
    assert capi.live_device_bytes() == start


# ---- 7
def test_7_errors_in_order_change_nothing():
    sc, mgr, cam = _scene("cornell")
    ctx = capi.Context(0)
    lib = ctx.lib
    n0 = int(sc.mesh_transforms[0]["vertex_count"])
    v = np.ascontiguousarray(sc.world_vertices)

    def call(meshes, count, null_meshes=False, null_vertices=False):
        idx = (C.c_uint32 * max(1, len(meshes)))(*meshes)
        return lib.fyprt_update_mesh_vertices(ctx.h, None if null_meshes else idx, len(meshes), None if null_vertices else v.ctypes.data, count)

    assert lib.fyprt_update_mesh_vertices(None, None, 0, None, 0) == EINVAL
    assert call([0], n0, null_meshes=True) == EINVAL and call([0], n0, null_vertices=True) == EINVAL
    assert call([0], n0) == ESTATE and b"fyprt_upload_scene" in lib.fyprt_last_error(ctx.h)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    before = ctx.export_bvh()

    def unchanged():
        after = ctx.export_bvh()
        assert before["nodes"].tobytes() == after["nodes"].tobytes() and before["tris"].tobytes() == after["tris"].tobytes()
        assert lib.fyprt_last_edit_stats(ctx.h, C.byref(capi.EditStats())) == ESTATE

    assert call([99], n0) == ESTATE and b"fyprt_set_object_vertices" in lib.fyprt_last_error(ctx.h)     # the state before the indices
    unchanged()
    ref = capi.Context(-1)
    ref.upload_scene(sc)
    lt = ref.export_lighttrees(len(sc.meshes))
    ref.close()
    ctx.upload_scene(sc, light_trees=lt)
    ctx.set_object_vertices(sc)
    assert call([0], n0) == ESTATE and b"prebuilt" in lib.fyprt_last_error(ctx.h)
    ctx.upload_scene(sc)
    ctx.set_object_vertices(sc)
    before = ctx.export_bvh()
    assert call([len(sc.meshes)], n0) == EINVAL and b"out of range" in lib.fyprt_last_error(ctx.h)
    unchanged()
    assert call([0, len(sc.meshes)], n0 + 1) == EINVAL and b"out of range" in lib.fyprt_last_error(ctx.h)   # ... before the duplicate and the sum
    assert call([0, 0], 2 * n0 + 1) == EINVAL and b"twice" in lib.fyprt_last_error(ctx.h)
    unchanged()
    assert call([0], n0 + 1) == EINVAL and b"sum" in lib.fyprt_last_error(ctx.h)
    assert call([], 1) == EINVAL
    unchanged()
    assert call([], 0) == 0
    unchanged()
    ctx.render(settings_for(capi.NEE))                       # the context is as it was
    assert call([0], n0) == 0 and ctx.last_edit_stats().partial == 1
    ctx.close()
