"""Box-overlap queries on the GPU (fyprt_overlap_boxes / fyprt_overlap_boxes_device, rt_boxes.h: BoxLaneT behind rt_query.h's kernel templates).
Every comparison is bit for bit against tests/boxes_ref.py (every leaf record of ctx.export_bvh() tested, no tree): indices, unused
slots, counts and totals.
  * the stack of coplanar layers: slabs of no thickness exactly on a layer, boxes across several layers, the whole scene; K from 1 to
    32, both kernels of tuning key 15;
  * hall_small under the three builders: small boxes where the camera sees surfaces, uniform boxes in twice the scene box, point boxes
    on vertices, boxes with faces on the decoded planes of the exported tree, the whole scene;
  * stack budget extremes; continuation against all_in_boxes; invalid boxes, empty and misaligned calls; counters on hand-countable
    trees; the persistent kernel's claims; the geometry of the last edit; frames untouched; the torch path; device memory."""

import numpy as np
import pytest

import boxes_ref as br
import multihit_ref as mh
from append_common import append_patch
from common import SCENES, bits_equal, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
KMAX = capi.OVERLAP_MAX_HITS


def _ctx(sc, key15=0, counting=False, builder=0):
    ctx = capi.Context(0)
    ctx.set_tuning(15, key15)
    ctx.set_tuning(12, builder)
    ctx.upload_scene(sc)
    ctx.set_ray_counting(counting)
    return ctx


def _truncate(ref, k):
    """The answer for max_hits = k from a reference computed with a larger K: the k lowest indices are a prefix of the K lowest."""
    tris, _, totals = ref
    return np.ascontiguousarray(tris[:, :k]), np.minimum(totals, k).astype(np.uint32), totals


def _assert_equal(got, want, tag):
    (gt, gc, gn), (wt, wc, wn) = got[:3], want[:3]
    assert gt.shape == wt.shape and gt.dtype == np.uint32 and gc.dtype == np.uint32 and gn.dtype == np.uint32
    bad = np.nonzero((gt != wt).any(axis=1))[0]
    assert len(bad) == 0, (tag, len(bad), bad[:8], gt[bad[:2]], wt[bad[:2]])
    assert np.array_equal(gc, wc), (tag, np.nonzero(gc != wc)[0][:8])
    assert np.array_equal(gn, wn), (tag, np.nonzero(gn != wn)[0][:8], gn[gn != wn][:8], wn[gn != wn][:8])


def _same_leaf_records(a, b):
    ka, kb = np.argsort(a["tris"]["tri"]), np.argsort(b["tris"]["tri"])
    return all(np.array_equal(a["tris"][f][ka].view(np.uint32), b["tris"][f][kb].view(np.uint32)) for f in ("v0", "e1", "e2", "tri"))


def _scene_box(sc):
    p = sc.world_vertices["position"].astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


def _uniform_boxes(sc, n, seed, scale=2.0, sizes=(0.02, 0.1, 0.3)):
    lo, hi = _scene_box(sc)
    rng = np.random.default_rng(seed)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * scale
    c = rng.uniform(mid - half, mid + half, size=(n, 3))
    h = (hi - lo)[None, :] * rng.choice(sizes, size=(n, 1)) * rng.uniform(0.2, 1.0, size=(n, 3))
    return (c - h).astype(F32), (c + h).astype(F32)


def _plane_boxes(bvh, n, seed):
    """Boxes that end exactly on a decoded child plane from outside, or begin on it, per axis at random; and the child's own box."""
    rng = np.random.default_rng(seed)
    lo, hi = [], []
    for node in bvh["nodes"][rng.integers(0, len(bvh["nodes"]), n // 2)]:
        blo, bhi = br.child_planes(node)
        c = int(rng.integers(0, len(blo)))
        d = (bhi[c] - blo[c]) * F32(0.5) + F32(0.01)
        side = rng.integers(0, 2, 3) == 1
        lo += [np.where(side, blo[c] - d, bhi[c]).astype(F32), blo[c]]
        hi += [np.where(side, blo[c], bhi[c] + d).astype(F32), bhi[c]]
    return np.array(lo, F32), np.array(hi, F32)


# ---- the layers scene: 15 quads in 12 planes y = -0.25 j, three of them twice
def _layers_boxes():
    rng = np.random.default_rng(29)
    n = 160
    x, z = rng.uniform(-1.5, 1.5, (2, n)), rng.uniform(-1.5, 1.5, (2, n))
    fx, fz = np.sort(x, axis=0), np.sort(z, axis=0)
    small = rng.integers(0, 2, n) == 1                                        # half of them with a footprint that meets one triangle of a quad, or two
    fx[1, small], fz[1, small] = fx[0, small] + 0.02, fz[0, small] + 0.02
    j = rng.integers(0, 12, n)
    y = (F32(-0.25) * j.astype(F32)).astype(F32)
    slab = (np.stack([fx[0], y, fz[0]], 1), np.stack([fx[1], y, fz[1]], 1))   # no thickness, exactly on a layer
    span = rng.integers(1, 12, n)                                             # from layer j down across `span` layers, both ends on a layer
    y2 = (F32(-0.25) * np.minimum(j + span, 11).astype(F32)).astype(F32)
    across = (np.stack([fx[0], y2, fz[0]], 1), np.stack([fx[1], y, fz[1]], 1))
    off = rng.uniform(0.01, 0.24, n)                                          # between layers: ends on none
    loose = (np.stack([fx[0], y2 - off, fz[0]], 1), np.stack([fx[1], y + off, fz[1]], 1))
    whole = (np.array([(-2, -3, -2)] * 20, F32), np.array([(2, 1, 2)] * 20, F32))
    lo = np.concatenate([s[0] for s in (slab, across, loose, whole)]).astype(F32)
    hi = np.concatenate([s[1] for s in (slab, across, loose, whole)]).astype(F32)
    return lo, hi


LAYER_KS = (1, 2, 7, 8, 9, 31, 32)


@pytest.fixture(scope="module")
def layers():
    sc = mh.layers_scene()
    lo, hi = _layers_boxes()
    ctx = _ctx(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    ref = br.k_lowest(bvh, lo, hi, KMAX)
    totals = ref[2]
    assert len(bvh["tris"]) == 30 and len(lo) == 500 and totals.max() == 30
    for k in LAYER_KS:
        assert (totals < k).any(), k
        if k <= 30:                                                           # (the scene has 30 triangles: no total reaches 31)
            assert (totals == k).any() and (totals > k).any() == (k < 30), k
    return sc, lo, hi, bvh, ref


@pytest.mark.parametrize("key15", [1, 2])
def test_layers_every_k_both_kernels(layers, key15):
    sc, lo, hi, bvh, ref = layers
    ctx = _ctx(sc, key15)
    for k in LAYER_KS:
        _assert_equal(ctx.overlap_boxes(lo, hi, max_hits=k), _truncate(ref, k), (key15, k))
    ctx.close()


# ---- hall_small: five box sets
@pytest.fixture(scope="module")
def hall_small():
    sc = SCENES["hall_small"][0]()
    cam = SCENES["hall_small"][1](48, 32)
    ctx = _ctx(sc)
    bvh = ctx.export_bvh()
    d = cam.ray_directions().reshape(-1, 3).astype(F32)[::2]
    o = np.broadcast_to(np.asarray(cam.position, F32), d.shape)
    pay = ctx.trace_rays(o, d)
    ctx.close()
    hit = pay["objectIndex"] >= 0
    assert hit.sum() > 500
    rng = np.random.default_rng(37)
    surf = pay["worldPosition"][hit].astype(F32)[:600]
    r = rng.uniform(0.005, 0.15, size=(len(surf), 3)).astype(F32)
    verts = sc.world_vertices["position"][rng.integers(0, len(sc.world_vertices), 300)].astype(F32)
    slo, shi = _scene_box(sc)
    sets = {"surface": ((surf - r).astype(F32), (surf + r).astype(F32)), "uniform": _uniform_boxes(sc, 700, 39),
            "vertices": (verts, verts), "planes": _plane_boxes(bvh, 400, 41),
            "whole": (np.tile((slo - 1).astype(F32), (4, 1)), np.tile((shi + 1).astype(F32), (4, 1)))}
    lo = np.concatenate([s[0] for s in sets.values()]).astype(F32)
    hi = np.concatenate([s[1] for s in sets.values()]).astype(F32)
    assert 1900 <= len(lo) <= 2100 and not br.invalid_boxes(lo, hi).any()
    ok_ids = br.accepted(bvh, lo, hi)
    ref = br.k_lowest(bvh, lo, hi, KMAX, ok_ids=ok_ids)
    totals = ref[2]
    assert (totals == 0).sum() > 200 and (totals[-4:] == len(sc.triangles)).all() and ((totals > 0) & (totals < 8)).any() and ((totals > 32) & (totals < 1000)).any()
    first = sum(len(sets[k][0]) for k in ("surface", "uniform"))
    assert (totals[first:first + 300] > 0).mean() > 0.5                      # a point box on a vertex accepts the records whose v0 it is, at least
    return sc, lo, hi, bvh, ref, ok_ids


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_hall_small_equals_bruteforce(hall_small, builder):
    sc, lo, hi, bvh, ref = hall_small[:5]
    for key15 in (1, 2):
        ctx = _ctx(sc, key15, builder=builder)
        assert _same_leaf_records(ctx.export_bvh(), bvh)                      # the reference is a function of the leaf records alone
        for k in (1, 8, 32):
            _assert_equal(ctx.overlap_boxes(lo, hi, max_hits=k), _truncate(ref, k), (builder, key15, k))
        ctx.close()


@pytest.mark.parametrize("budget", [1, 31])
def test_stack_budget_extremes(hall_small, budget):
    """Tuning key 8 at its ends: the smallest budget (raised to the tree's level count) makes the node visit push resume entries, which
    fetch a node again — no index twice, no record counted twice; the largest, with K = 32, is the 64 KB workgroup."""
    sc, lo, hi, bvh, ref = hall_small[:5]
    for key15 in (1, 2):
        ctx = capi.Context(0)
        ctx.set_tuning(15, key15)
        ctx.set_tuning(8, budget)
        ctx.upload_scene(sc)
        assert (ctx.get_tuning(8) == 31) == (budget == 31)
        _assert_equal(ctx.overlap_boxes(lo, hi, max_hits=32), ref, (budget, key15))
        if budget == 1:                                                       # resume entries were pushed: nodes were fetched again
            ctx.set_ray_counting(True)
            visits = ctx.overlap_boxes(lo[-4:], hi[-4:], max_hits=32, with_stats=True)[3].node_visits
            assert visits > 4 * len(bvh["nodes"]), (visits, len(bvh["nodes"]))
        ctx.close()


def test_continuation_lists_every_triangle_once(layers, hall_small):
    for name, (sc, lo, hi, bvh) in (("layers", layers[:4]), ("hall", hall_small[:4])):
        if name == "hall":
            few = np.nonzero(hall_small[4][2] <= 120)[0][::4]                 # boxes that a few passes finish
            lo, hi = lo[few], hi[few]
        want, want_off = br.all_in_boxes(bvh, lo, hi)
        assert np.diff(want_off).max() > 9 and (np.diff(want_off) == 0).any(), name
        for key15 in (1, 2):
            ctx = _ctx(sc, key15, counting=True)
            got, off = ctx.triangles_in_boxes(lo, hi, max_hits=3 if name == "layers" else 8)
            assert got.dtype == np.uint32 and np.array_equal(off, want_off), (name, key15)
            assert np.array_equal(got, want), (name, key15)
            if name == "layers":
                # a pass's unused slots passed back in: finished boxes, zero records, total 0, and they count no tests
                tris, counts, totals = ctx.overlap_boxes(lo, hi, max_hits=8)
                done = counts < 8
                assert done.any() and (~done).any() and (tris[done, 7] == br.NONE).all()
                t2, c2, n2, st = ctx.overlap_boxes(lo[done], hi[done], max_hits=8, after=tris[done, 7], with_stats=True)
                assert (c2 == 0).all() and (n2 == 0).all() and (t2 == br.NONE).all()
                assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (int(done.sum()), 0, 0, 0, 0)
                more = ~done
                got3 = ctx.overlap_boxes(lo[more], hi[more], max_hits=8, after=tris[more, 7])
                _assert_equal(got3, br.k_lowest(bvh, lo[more], hi[more], 8, after=tris[more, 7]), "after")
                assert np.array_equal(got3[2], totals[more] - 8)              # what is still to come
            ctx.close()


def test_invalid_boxes_empty_and_misaligned_calls():
    sc = SCENES["cornell"][0]()
    ctx = _ctx(sc)
    nan, inf = F32(np.nan), F32(np.inf)
    lo = np.array([(nan, -9, -9), (-9, -9, -9), (-inf, -9, -9), (-3e38, -9, -9), (2, -9, -9), (-9, -9, -9)], F32)
    hi = np.array([(9, 9, 9), (9, nan, 9), (9, 9, 9), (3e38, 9, 9), (1, 9, 9), (9, 9, inf)], F32)
    assert br.invalid_boxes(lo, hi).all()
    everything = ctx.overlap_boxes(np.full((1, 3), -9, F32), np.full((1, 3), 9, F32), max_hits=2)
    assert everything[1][0] == 2 and everything[2][0] == len(sc.triangles)     # the valid version answers
    for key15 in (1, 2):
        ctx.set_tuning(15, key15)
        for k in (1, 32):
            tris, counts, totals = ctx.overlap_boxes(lo, hi, max_hits=k)
            assert (counts == 0).all() and (totals == 0).all() and (tris == br.NONE).all(), (key15, k)
        ctx.set_ray_counting(True)
        st = ctx.overlap_boxes(lo, hi, max_hits=3, with_stats=True)[3]
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (len(lo), 0, 0, 0, 0)
        ctx.set_ray_counting(False)
        # NULL hit_counts and totals: the indices alone; the pads are ignored
        rr = np.zeros(2, dtype=capi.BOX_DTYPE)
        rr["lo"], rr["hi"], rr["pad0"], rr["pad1"] = -9, 9, 0xDEADBEEF, 0x7FC00000
        out = np.zeros((2, 3), dtype=np.uint32)
        assert ctx.lib.fyprt_overlap_boxes(ctx.h, rr.ctypes.data, None, 2, 3, out.ctypes.data, None, None, None) == 0
        assert out.tolist() == [[0, 1, 2]] * 2
    # count 0: OK, nothing launched
    e = np.zeros(0, dtype=capi.BOX_DTYPE)
    assert ctx.lib.fyprt_overlap_boxes(ctx.h, e.ctypes.data, None, 0, 4, None, None, None, None) == 0
    assert ctx.lib.fyprt_overlap_boxes_device(ctx.h, None, None, 0, 4, None, None, None) == 0
    tris, counts, totals = ctx.overlap_boxes(np.zeros((0, 3)), np.zeros((0, 3)), max_hits=5)
    assert tris.shape == (0, 5) and counts.shape == (0,) and totals.shape == (0,)
    rec, off = ctx.triangles_in_boxes(np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(rec) == 0 and off.tolist() == [0]
    # misaligned device pointers (device memory of the context: its image buffer, 16-byte aligned; refused before any launch)
    ctx.resize(16, 16)
    img = ctx.image_device_ptr()
    dev = ctx.lib.fyprt_overlap_boxes_device
    assert dev(ctx.h, img + 8, None, 1, 1, img + 64, img + 128, img + 192) == -1
    assert dev(ctx.h, img, img + 66, 1, 1, img + 64, img + 128, img + 192) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 65, img + 128, img + 192) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 64, img + 130, img + 192) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 64, img + 128, img + 193) == -1
    assert dev(ctx.h, img, None, 1, 0, img + 64, None, None) == -1 and dev(ctx.h, img, None, 1, 33, img + 64, None, None) == -1
    ctx.close()


def test_counters_on_hand_countable_trees():
    from fypraytracer_amd.scene import Material, Scene
    from fypraytracer_amd.scenes import _quad
    one = Scene()
    one.materials = [Material(albedo=(1, 1, 1), emission_color=(1, 1, 1), emission_power=5.0)]
    one.add_new_mesh_to_scene(*_quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0)), material_index=0)
    one.init_scene_emissive_triangles()
    for key15 in (1, 2):
        # a one-leaf tree: the root reference is the leaf of both triangles — no node visit, two triangle tests
        ctx = _ctx(one, key15, counting=True)
        bvh = ctx.export_bvh()
        assert len(bvh["nodes"]) == 0 and bvh["root"] < 0 and len(bvh["tris"]) == 2
        lo, hi = np.array([[-0.5, -0.5, -0.5]], F32), np.array([[0.5, 0.5, 0.5]], F32)
        got = ctx.overlap_boxes(lo, hi, max_hits=2, with_stats=True)
        st = got[3]
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (1, 0, 2, 1, 0)
        _assert_equal(got, br.k_lowest(bvh, lo, hi, 2), "one leaf")
        assert got[0][0].tolist() == [0, 1]
        got = ctx.overlap_boxes(lo + 2, hi + 2, max_hits=2, with_stats=True)
        st = got[3]
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (1, 0, 2, 0, 0) and got[1][0] == 0 and got[2][0] == 0
        ctx.close()
        # cornell: a box far from everything visits the root, tests its children's boxes and nothing else; a box around everything
        # visits every node, tests every child box and every record
        ctx = _ctx(SCENES["cornell"][0](), key15, counting=True)
        bvh = ctx.export_bvh()
        root_children = int(bvh["nodes"][bvh["root"]]["meta"]) & 7
        far = ctx.overlap_boxes(np.array([[50, 60, -70]], F32), np.array([[51, 61, -69]], F32), max_hits=8, with_stats=True)
        st = far[3]
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (1, root_children, 0, 0, 1) and far[1][0] == 0
        every = ctx.overlap_boxes(np.full((1, 3), -9, F32), np.full((1, 3), 9, F32), max_hits=8, with_stats=True)
        st = every[3]
        children = sum(int(n["meta"]) & 7 for n in bvh["nodes"])
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (1, children, len(bvh["tris"]), 1, len(bvh["nodes"]))
        assert every[2][0] == len(bvh["tris"]) and every[0][0].tolist() == list(range(8))
        ctx.close()


def test_persistent_kernel_claims_and_counters():
    """Small static chunks (key 4 = 16 boxes per claim, key 9 = 1 static chunk per wave) leave most boxes to the claims from the shared
    head; two consecutive calls (the head is reset per call), counted and not, give the same answers."""
    sc = SCENES["banana_standin"][0]()
    lo, hi = _uniform_boxes(sc, 3000, 73, scale=1.0, sizes=(0.05, 0.15))
    ctx = _ctx(sc, key15=1, counting=True)
    want = br.k_lowest(ctx.export_bvh(), lo, hi, 4)
    assert (want[2] > 4).any() and (want[2] == 0).any()
    for key, value in ((4, 16), (9, 1)):
        ctx.set_tuning(key, value)
    counted = []
    for _ in range(2):
        got = ctx.overlap_boxes(lo, hi, max_hits=4, with_stats=True)
        _assert_equal(got, want, "counted")
        st = got[3]
        assert st.rays == len(lo) == st.part_rays[0] and st.hits == int((got[1] > 0).sum()) == st.part_hits[0]
        assert st.launches == 1 and st.kernel_ms > 0.0 and st.tri_tests >= int(want[2].sum()) and st.node_visits > 0 and st.box_tests > st.node_visits
        counted.append((st.box_tests, st.tri_tests, st.node_visits))
    assert counted[0] == counted[1]
    ctx.set_ray_counting(False)
    for _ in range(2):
        _assert_equal(ctx.overlap_boxes(lo, hi, max_hits=4), want, "uncounted")
    ctx.close()


def test_queries_see_current_geometry():
    """After update_vertices, update_transforms, append_meshes, regraft_meshes and remove_meshes: brute force on the re-exported tree."""
    mk_scene, mk_cam = SCENES["hall_small"]
    sc = mk_scene()
    cam = mk_cam(64, 64)
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    ctx = _ctx(sc)
    ctx.set_object_vertices(sc)
    lo, hi = _uniform_boxes(sc, 400, 53, scale=1.0)
    v = sc.world_vertices["position"][::60].astype(F32)
    lo, hi = np.concatenate([lo, v]), np.concatenate([hi, v])

    def check(tag):
        got = ctx.overlap_boxes(lo, hi, max_hits=8)
        bvh = ctx.export_bvh()
        assert len(bvh["tris"]) == len(sc.triangles)
        _assert_equal(got, br.k_lowest(bvh, lo, hi, 8), tag)
        return got
    before = check("before")
    mgr.set_mesh_transform(sc, 3, pos=(0.7, 0.0, -0.4), rotation=(0, 25, 0))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_vertices(sc)
    moved = check("update_vertices")
    assert not np.array_equal(moved[0], before[0])                            # the edit is visible to the query
    mgr.set_mesh_transform(sc, 5, pos=(-0.5, 0.2, 0.3))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_transforms(sc, [5])
    check("update_transforms")
    new = append_patch(sc, cam, "hall_small", 300, 0)
    ctx.append_meshes(sc, new)
    grown = check("append_meshes")
    centre = sc.world_vertices["position"][-1].astype(F32)
    d = F32(0.05)
    near = ctx.overlap_boxes((centre - d)[None], (centre + d)[None], max_hits=32)
    assert near[1][0] > 0 and (near[0][0, :near[1][0]] >= len(sc.triangles) - 300).any()
    ctx.regraft_meshes([3, new])
    assert np.array_equal(check("regraft_meshes")[0], grown[0])               # nothing but the tree moved
    ctx.remove_meshes(sc.remove_meshes_from_scene([new]))
    check("remove_meshes")
    ctx.close()


def test_queries_leave_frames_and_other_queries_untouched(hall_small):
    sc, W, H = hall_small[0], 96, 64
    cam = SCENES["hall_small"][1](W, H)
    lo, hi = hall_small[1][::4], hall_small[2][::4]
    pts = ((lo + hi) * F32(0.5)).astype(F32)
    runs = []
    for with_query in (False, True):
        ctx = _ctx(sc)
        ctx.resize(W, H)
        ctx.set_camera(cam)
        st = settings_for(capi.RESTIR_DI)
        for f in range(3):
            st.rand_seed = f + 1
            ctx.render(st)
            if with_query:
                ctx.overlap_boxes(lo, hi, max_hits=32)
                ctx.triangles_in_boxes(lo[:150], hi[:150], max_hits=32)
        img, acc = ctx.readback()
        runs.append((ctx.frame_index, img, acc, ctx.read_buffer(capi.BUF_PAYLOAD)))
        if with_query:
            # the other list queries' staging is their own: their answers before and after a box query are the same bytes
            near = ctx.nearest_points(pts, max_hits=4)
            ctx.overlap_boxes(lo, hi, max_hits=7)
            again = ctx.nearest_points(pts, max_hits=4)
            assert near[0].tobytes() == again[0].tobytes() and np.array_equal(near[1], again[1])
        ctx.close()
    (ia, imga, acca, pa), (ib, imgb, accb, pb) = runs
    assert ia == ib
    assert np.array_equal(imga, imgb) and bits_equal(acca, accb).all() and pa.tobytes() == pb.tobytes()


def test_device_memory_returns_after_close(layers):
    sc, lo, hi = layers[:3]
    base = capi.live_device_bytes()
    ctx = _ctx(sc)
    loaded = capi.live_device_bytes()
    ctx.overlap_boxes(lo, hi, max_hits=32, after=np.zeros(len(lo), dtype=np.uint32))
    n = len(lo)
    staged = capi.live_device_bytes() - loaded
    assert staged >= n * (32 + 4 + 32 * 4 + 4 + 4) + 64                      # boxes, after, indices, totals, counts, counters: all counted
    ctx.overlap_boxes(lo[:100], hi[:100], max_hits=2)
    assert capi.live_device_bytes() - loaded == staged                       # the staging is kept, a smaller call allocates nothing
    ctx.close()
    assert capi.live_device_bytes() == base


def test_torch_path_equals_host_entry():
    """Run in a fresh process that initialises torch's CUDA before the library is loaded (see test_gpu_query's torch test)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_boxes as t; t._torch_path_checks(); print('torch path ok')"
            % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_path_checks():
    """Boxes produced by torch ops, indices consumed by torch ops, no synchronisation by the caller; two back-to-back device calls at
    different K (two LDS sizes), then a continuation pass from the first call's last slots."""
    import torch
    sc = SCENES["hall_small"][0]()
    lo, hi = _uniform_boxes(sc, 4096, 63, scale=1.0)
    ctx = _ctx(sc, key15=1)
    want2, want32 = ctx.overlap_boxes(lo, hi, max_hits=2), ctx.overlap_boxes(lo, hi, max_hits=32)
    want_next = ctx.overlap_boxes(lo, hi, max_hits=3, after=want2[0][:, 1].copy())
    for _ in range(2):
        lt, ht = torch.from_numpy(lo).to("cuda:0", non_blocking=True), torch.from_numpy(hi).to("cuda:0", non_blocking=True)
        big = torch.randn(2048, 2048, device="cuda:0") @ torch.randn(2048, 2048, device="cuda:0")   # (an unordered query would read unwritten boxes)
        pad = torch.zeros((len(lo), 1), device="cuda:0")
        boxes = torch.cat([lt, pad, ht, pad], 1).contiguous()
        t2, c2, n2 = ctx.overlap_boxes_tensor(boxes, 2)
        t32, c32, n32 = ctx.overlap_boxes_tensor(boxes, 32)
        tn, cn, nn = ctx.overlap_boxes_tensor(boxes, 3, after=t2[:, 1].contiguous())
        total = (c2 + c32).sum()                                              # consumed by torch ops without a synchronisation
        for (t, c, n), (wt, wc, wn) in (((t2, c2, n2), want2), ((t32, c32, n32), want32), ((tn, cn, nn), want_next)):
            assert t.dtype == torch.int32 and c.dtype == torch.int32 and n.dtype == torch.int32 and tuple(t.shape) == wt.shape
            assert np.array_equal(t.cpu().numpy().view(np.uint32), wt)
            assert np.array_equal(c.cpu().numpy().view(np.uint32), wc) and np.array_equal(n.cpu().numpy().view(np.uint32), wn)
        assert int(total) == int(want2[1].sum()) + int(want32[1].sum())
        del boxes, big, lt, ht
    with pytest.raises(ValueError):
        ctx.overlap_boxes_tensor(torch.zeros(4, 6, device="cuda:0"), 4)
    with pytest.raises(ValueError):
        ctx.overlap_boxes_tensor(torch.zeros(4, 8, device="cuda:0"), 4, after=torch.zeros(3, dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError):
        ctx.overlap_boxes_tensor(torch.zeros(4, 8, device="cuda:0"), 4, after=torch.zeros(4, 4, device="cuda:0"))
    ctx.close()


@pytest.mark.parametrize("key15", [1, 2])
def test_boxes_on_rounded_vertices_outside_the_planes(key15):
    """banana: boxes that begin exactly on a record's rounded vertex where that vertex lies outside a decoded plane above the record
    (boxes_ref.protruding_boxes, shown by test_boxes_cpu to lose records under a cull without slack)."""
    sc = SCENES["banana"][0]()
    ctx = _ctx(sc, key15)
    bvh = ctx.export_bvh()
    lo, hi, where = br.protruding_boxes(bvh)
    assert len(where) >= 10
    ok_ids = br.accepted(bvh, lo, hi)
    assert sum(bool(ok_ids[0][i, r]) for i, (_, _, r) in enumerate(where)) >= 10
    _assert_equal(ctx.overlap_boxes(lo, hi, max_hits=32), br.k_lowest(bvh, lo, hi, 32, ok_ids=ok_ids), key15)
    ctx.close()
