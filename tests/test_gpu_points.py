"""Nearest-point queries on the GPU (fyprt_nearest_points / fyprt_nearest_points_device, rt_points.h: PointsLaneT behind rt_query.h's
kernel templates).  Every comparison is bit for bit against tests/points_ref.py (every leaf record of ctx.export_bvh() measured, no
tree): records, unused slots and counts.
  * the stack of coplanar layers, where every point has exact ties, K = 1..8, both kernels of tuning key 15;
  * hall_small under the three builders: points jittered off the surfaces the camera sees, uniform points in twice the scene box, points
    exactly on vertices and on the decoded box planes of the exported tree;
  * stack budget extremes; finite radii; continuation against all_within; invalid points, empty and misaligned calls; counters on
    hand-countable cases; the persistent kernel's claims; the geometry of the last edit; frames untouched; the torch path; device memory."""

import numpy as np
import pytest

import multihit_ref as mh
import points_ref as pr
from append_common import append_patch
from common import SCENES, bits_equal, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32


def _ctx(sc, key15=0, counting=False, builder=0):
    ctx = capi.Context(0)
    ctx.set_tuning(15, key15)
    ctx.set_tuning(12, builder)
    ctx.upload_scene(sc)
    ctx.set_ray_counting(counting)
    return ctx


def _truncate(ref, k):
    """The answer for max_hits = k from a reference computed with a larger K: the k smallest keys are a prefix of the K smallest."""
    hits, _, totals = ref
    return np.ascontiguousarray(hits[:, :k]), np.minimum(totals, k).astype(np.uint32)


def _assert_equal(got, want, tag):
    (gh, gc), (wh, wc) = got, want
    assert gh.shape == wh.shape and gc.dtype == np.uint32
    bad = pr.record_diff(gh, wh)
    assert len(bad) == 0, (tag, len(bad), bad[:8], gh[bad[:2]], wh[bad[:2]])
    assert np.array_equal(gc, wc), (tag, np.nonzero(gc != wc)[0][:8])


def _same_leaf_records(a, b):
    ka, kb = np.argsort(a["tris"]["tri"]), np.argsort(b["tris"]["tri"])
    return all(np.array_equal(a["tris"][f][ka].view(np.uint32), b["tris"][f][kb].view(np.uint32)) for f in ("v0", "e1", "e2", "tri"))


def _box(sc):
    p = sc.world_vertices["position"].astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


def _uniform(sc, n, seed, scale=2.0):
    lo, hi = _box(sc)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * scale
    return np.random.default_rng(seed).uniform(mid - half, mid + half, size=(n, 3)).astype(F32)


def _plane_points(sc, bvh, n, seed):
    """Points exactly on vertices, and on decoded box planes / corners of the exported tree's nodes."""
    rng = np.random.default_rng(seed)
    pos = sc.world_vertices["position"]
    out = [pos[rng.integers(0, len(pos), n // 2)].astype(F32)]
    pts = []
    for node in bvh["nodes"][rng.integers(0, len(bvh["nodes"]), n // 4)]:
        blo, bhi = pr.child_planes(node)
        c = int(rng.integers(0, len(blo)))
        corner = np.where(rng.integers(0, 2, 3) == 1, bhi[c], blo[c]).astype(F32)
        face = rng.uniform(blo[c], bhi[c]).astype(F32)
        a = int(rng.integers(0, 3))
        face[a] = (blo[c] if rng.integers(0, 2) else bhi[c])[a]
        pts += [corner, face]
    return np.concatenate(out + [np.array(pts, F32)])


# ---- the layers scene: coplanar copies, so the distance to a copied quad is tied between two triangle indices for EVERY point
@pytest.fixture(scope="module")
def layers():
    sc = mh.layers_scene()
    rng = np.random.default_rng(23)
    p = np.stack([rng.uniform(-1.6, 1.6, 500), rng.uniform(-3.2, 0.6, 500), rng.uniform(-1.6, 1.6, 500)], 1).astype(F32)
    p[:60, 1] = F32(-0.25) * rng.integers(0, 12, 60).astype(F32)             # some exactly on a layer: distance2 = +0
    ctx = _ctx(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    return sc, p, bvh, pr.k_nearest(bvh, p, np.inf, 9)


def test_layers_every_k_both_kernels(layers):
    sc, p, bvh, ref = layers
    full, _, totals = ref
    assert len(bvh["tris"]) == 30 and (totals == 30).all()
    db = np.ascontiguousarray(full["distance2"]).view(np.uint32)
    straddles = [int(((db[:, k - 1] == db[:, k]) & (full["triangle"][:, k - 1] < full["triangle"][:, k])).sum()) for k in range(1, 9)]
    assert all(s > 0 for s in straddles), straddles                            # a tied pair straddles every K-th place somewhere
    assert (full["distance2"][:, 0] == 0).any()
    for key15 in (1, 2):
        ctx = _ctx(sc, key15)
        for k in range(1, 9):
            _assert_equal(ctx.nearest_points(p, max_hits=k), _truncate(ref, k), (key15, k))
        ctx.close()


# ---- hall_small: three point sets
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
    rng = np.random.default_rng(31)
    surf = pay["worldPosition"][hit].astype(F32)
    surf = (surf + rng.normal(scale=0.02, size=surf.shape)).astype(F32)       # jittered off the surface
    sets = {"surface": surf[:700], "uniform": _uniform(sc, 700, 33), "planes": _plane_points(sc, bvh, 600, 35)}
    p = np.concatenate(list(sets.values()))
    ref = pr.k_nearest(bvh, p, np.inf, 8)
    return sc, p, bvh, ref, {k: len(v) for k, v in sets.items()}


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_hall_small_equals_bruteforce(hall_small, builder):
    sc, p, bvh, ref, sizes = hall_small
    assert (ref[0]["distance2"][-sizes["planes"]:, 0] == 0).sum() >= sizes["planes"] // 2          # the vertex points lie on the scene
    for key15 in (1, 2):
        ctx = _ctx(sc, key15, builder=builder)
        assert _same_leaf_records(ctx.export_bvh(), bvh)                      # the reference is a function of the leaf records alone
        for k in (1, 4, 8):
            _assert_equal(ctx.nearest_points(p, max_hits=k), _truncate(ref, k), (builder, key15, k))
        ctx.close()


@pytest.mark.parametrize("budget", [1, 31])
def test_stack_budget_extremes(hall_small, budget):
    """Tuning key 8 at its ends: the smallest budget (raised to the tree's level count) makes the node visit push resume entries, which
    visit a node again; the largest, with K = 8, is the 64 KB workgroup."""
    sc, p, bvh, ref = hall_small[:4]
    for key15 in (1, 2):
        ctx = capi.Context(0)
        ctx.set_tuning(15, key15)
        ctx.set_tuning(8, budget)
        ctx.upload_scene(sc)
        assert (ctx.get_tuning(8) == 31) == (budget == 31)
        for k in (8, 3):
            _assert_equal(ctx.nearest_points(p, max_hits=k), _truncate(ref, k), (budget, key15, k))
        ctx.close()


@pytest.mark.parametrize("key15", [1, 2])
def test_finite_max_distance(hall_small, key15):
    sc, p, bvh, ref = hall_small[:4]
    p = p[::3]
    d2 = ref[0]["distance2"][::3]
    root = np.sqrt(d2[:, 2]).astype(F32)                                       # the third-nearest distance
    exact = (root * root).astype(F32) == d2[:, 2]                              # ... where its square gives distance2 back exactly
    assert exact.sum() > 20
    cases = {
        "at": np.where(exact, root, F32(0.5)).astype(F32),
        "below": np.nextafter(root, F32(0)),
        "small": np.full(len(p), 0.05, F32),
        "zero": np.zeros(len(p), F32),
        "mixed": np.random.default_rng(3).uniform(0.0, 3.0, len(p)).astype(F32),
    }
    ctx = _ctx(sc, key15)
    for label, md in cases.items():
        want = pr.k_nearest(bvh, p, md, 4)
        _assert_equal(ctx.nearest_points(p, md, max_hits=4), want[:2], label)
        if label == "at":
            r2 = (md * md).astype(F32)
            assert ((want[0]["distance2"] == r2[:, None]).any(axis=1) & exact).sum() > 20     # records exactly at the radius
        if label in ("small", "zero"):
            assert (want[1] == 0).any() and (want[1] > 0).any()               # some points answer nothing; the points on vertices do
    ctx.close()


def test_continuation_enumerates_every_triangle_within_a_radius(layers, hall_small):
    lp = layers[1][:200]
    hp = np.concatenate([hall_small[1][:150], hall_small[1][-150:]])
    for name, sc, p, bvh, radius in (("layers", layers[0], lp, layers[2], F32(0.6)), ("hall", hall_small[0], hp, hall_small[2], F32(0.5))):
        want, want_off = pr.all_within(bvh, p, radius)
        assert np.diff(want_off).max() > 6 and (np.diff(want_off) == 0).any(), name
        for key15 in (1, 2):
            ctx = _ctx(sc, key15, counting=True)
            got, off = ctx.triangles_within(p, radius, max_hits=3)
            assert np.array_equal(off, want_off), (name, key15)
            assert pr.records_equal(got, want), (name, key15, pr.record_diff(got, want)[:8])
            if name == "layers":
                keys = pr.hit_keys(got)
                tied = 0
                for i in range(len(p)):
                    k = keys[off[i]:off[i + 1]].astype(object)
                    assert (np.diff(k) > 0).all()                             # every triangle once
                    tied += int((np.diff(got["distance2"][off[i]:off[i + 1]].view(np.uint32).astype(np.int64)) == 0).sum())
                assert tied > 50
                # a pass's unused records passed back in: finished points, zero hits, and they count no tests
                hits, counts = ctx.nearest_points(p, radius, max_hits=8)
                done = counts < 8
                assert done.any() and (~done).any() and (hits[done, 7] == pr.UNUSED).all()
                h2, c2, st = ctx.nearest_points(p[done], radius, max_hits=8, after=hits[done, 7], with_stats=True)
                assert (c2 == 0).all() and (h2 == pr.UNUSED).all()
                assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (int(done.sum()), 0, 0, 0, 0)
                more = ~done
                h3, c3 = ctx.nearest_points(p[more], radius, max_hits=8, after=hits[more, 7])
                w3 = pr.k_nearest(bvh, p[more], radius, 8, after=hits[more, 7])
                _assert_equal((h3, c3), w3[:2], "after")
            ctx.close()


def test_invalid_points_empty_and_misaligned_calls():
    sc = SCENES["cornell"][0]()
    ctx = _ctx(sc)
    nan, inf = F32(np.nan), F32(np.inf)
    p = np.array([(nan, 0, 0), (0, inf, 0), (0, 0, -inf), (0, 0, 0), (0, 0, 0)], F32)
    md = np.array([1, 1, inf, nan, -1.0], F32)
    assert ctx.nearest_points(np.zeros((1, 3), F32), max_hits=2)[1][0] == 2    # the valid version answers
    for key15 in (1, 2):
        ctx.set_tuning(15, key15)
        for k in (1, 8):
            hits, counts = ctx.nearest_points(p, md, max_hits=k)
            assert (counts == 0).all() and (hits == pr.UNUSED).all(), (key15, k)
        ctx.set_ray_counting(True)
        st = ctx.nearest_points(p, md, max_hits=3, with_stats=True)[2]
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (len(p), 0, 0, 0, 0)
        ctx.set_ray_counting(False)
        # max_distance -0 is 0 and +inf is everything
        hits, counts = ctx.nearest_points(np.zeros((2, 3), F32), np.array([-0.0, inf], F32), max_hits=2)
        _assert_equal((hits, counts), pr.k_nearest(ctx.export_bvh(), np.zeros((2, 3), F32), np.array([-0.0, inf], F32), 2)[:2], "signed zero")
        assert counts.tolist() == [0, 2]
        # a NULL hit_counts: the records alone
        rr = np.zeros(2, dtype=capi.POINT_DTYPE)
        rr["max_distance"] = inf
        out = np.zeros((2, 3), dtype=capi.POINT_HIT_DTYPE)
        assert ctx.lib.fyprt_nearest_points(ctx.h, rr.ctypes.data, None, 2, 3, out.ctypes.data, None, None) == 0
        assert pr.records_equal(out, ctx.nearest_points(rr["position"], max_hits=3)[0]) and out["distance2"][0, 0] >= 0
    # count 0: OK, nothing launched
    e = np.zeros(0, dtype=capi.POINT_DTYPE)
    assert ctx.lib.fyprt_nearest_points(ctx.h, e.ctypes.data, None, 0, 4, None, None, None) == 0
    assert ctx.lib.fyprt_nearest_points_device(ctx.h, None, None, 0, 4, None, None) == 0
    hits, counts = ctx.nearest_points(np.zeros((0, 3)), max_hits=5)
    assert hits.shape == (0, 5) and counts.shape == (0,)
    rec, off = ctx.triangles_within(np.zeros((0, 3)), 1.0)
    assert len(rec) == 0 and off.tolist() == [0]
    # misaligned device pointers (device memory of the context: its image buffer, 16-byte aligned; refused before any launch)
    ctx.resize(16, 16)
    img = ctx.image_device_ptr()
    dev = ctx.lib.fyprt_nearest_points_device
    assert dev(ctx.h, img + 4, None, 1, 1, img + 64, img + 128) == -1
    assert dev(ctx.h, img, img + 72, 1, 1, img + 64, img + 128) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 72, img + 128) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 64, img + 130) == -1
    assert dev(ctx.h, img, None, 1, 0, img + 64, None) == -1 and dev(ctx.h, img, None, 1, 9, img + 64, None) == -1
    ctx.close()


def test_counters_on_hand_countable_cases():
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
        hits, counts, st = ctx.nearest_points(np.array([[0.25, 2.0, 0.5]], F32), max_hits=2, with_stats=True)
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (1, 0, 2, 1, 0)
        _assert_equal((hits, counts), pr.k_nearest(bvh, np.array([[0.25, 2.0, 0.5]], F32), np.inf, 2)[:2], "one leaf")
        assert counts[0] == 2 and hits["distance2"][0, 0] == 4.0 and sorted(hits["triangle"][0].tolist()) == [0, 1]
        _, counts, st = ctx.nearest_points(np.array([[0.25, 2.0, 0.5]], F32), 1.0, max_hits=2, with_stats=True)
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (1, 0, 2, 0, 0) and counts[0] == 0
        ctx.close()
        # cornell: a point far from everything with a small radius visits the root, tests its children's boxes and nothing else;
        # without a radius and with K = 8 < 32 triangles, the counters are those of the restated cull on the exported tree at least
        ctx = _ctx(SCENES["cornell"][0](), key15, counting=True)
        bvh = ctx.export_bvh()
        root_children = int(bvh["nodes"][bvh["root"]]["meta"]) & 7
        _, counts, st = ctx.nearest_points(np.array([[50.0, 60.0, -70.0]], F32), 1.0, max_hits=8, with_stats=True)
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (1, root_children, 0, 0, 1) and counts[0] == 0
        # three such points and one on a vertex: the totals add up
        pts = np.array([[50, 60, -70], [-40, 0, 0], [0, 90, 0], [1, 1, 1]], F32)
        _, counts, st = ctx.nearest_points(pts, 1e-3, max_hits=8, with_stats=True)
        assert st.rays == 4 and st.hits == 1 == int((counts > 0).sum()) and st.node_visits >= 4 and st.tri_tests >= int(counts.sum())
        ctx.close()


def test_persistent_kernel_claims_and_counters():
    """Small static chunks (key 4 = 16 points per claim, key 9 = 1 static chunk per wave, key 10 = 16) leave most points to the claims from
    the shared head; two consecutive calls (the head is reset per call), counted and not, give the same records."""
    sc = SCENES["banana_standin"][0]()
    p = _uniform(sc, 5000, 71, scale=1.2)
    ctx = _ctx(sc, key15=1, counting=True)
    want = pr.k_nearest(ctx.export_bvh(), p, np.inf, 4)
    for key, value in ((4, 16), (9, 1), (10, 16)):
        ctx.set_tuning(key, value)
    counted = []
    for _ in range(2):
        hits, counts, st = ctx.nearest_points(p, max_hits=4, with_stats=True)
        _assert_equal((hits, counts), want[:2], "counted")
        assert st.rays == len(p) == st.part_rays[0] and st.hits == int((counts > 0).sum()) == st.part_hits[0]
        assert st.launches == 1 and st.kernel_ms > 0.0 and st.tri_tests > 0 and st.node_visits > 0 and st.box_tests > st.node_visits
        counted.append((st.box_tests, st.tri_tests, st.node_visits))
    assert counted[0] == counted[1]
    ctx.set_ray_counting(False)
    for _ in range(2):
        _assert_equal(ctx.nearest_points(p, max_hits=4), want[:2], "uncounted")
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
    p = np.concatenate([_uniform(sc, 500, 51, scale=1.0), sc.world_vertices["position"][::40].astype(F32)])

    def check(tag):
        got = ctx.nearest_points(p, max_hits=4)
        bvh = ctx.export_bvh()
        assert len(bvh["tris"]) == len(sc.triangles)
        _assert_equal(got, pr.k_nearest(bvh, p, np.inf, 4)[:2], tag)
        return got
    before = check("before")
    mgr.set_mesh_transform(sc, 3, pos=(0.7, 0.0, -0.4), rotation=(0, 25, 0))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_vertices(sc)
    moved = check("update_vertices")
    assert not pr.records_equal(moved[0], before[0])                          # the edit is visible to the query
    mgr.set_mesh_transform(sc, 5, pos=(-0.5, 0.2, 0.3))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_transforms(sc, [5])
    check("update_transforms")
    new = append_patch(sc, cam, "hall_small", 300, 0)
    ctx.append_meshes(sc, new)
    grown = check("append_meshes")
    centre = sc.world_vertices["position"][-1].astype(F32)
    near = ctx.nearest_points(centre[None], max_hits=1)
    assert near[0]["triangle"][0, 0] >= len(sc.triangles) - 300 and near[0]["distance2"][0, 0] == 0
    ctx.regraft_meshes([3, new])
    assert pr.records_equal(check("regraft_meshes")[0], grown[0])             # nothing but the tree moved
    ctx.remove_meshes(sc.remove_meshes_from_scene([new]))
    check("remove_meshes")
    assert ctx.nearest_points(centre[None], max_hits=1)[0]["distance2"][0, 0] > 0
    ctx.close()


def test_queries_leave_frames_untouched(hall_small):
    sc, W, H = hall_small[0], 96, 64
    cam = SCENES["hall_small"][1](W, H)
    p = hall_small[1][::3]
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
                ctx.nearest_points(p, max_hits=8)
                ctx.triangles_within(p[:200], 0.3, max_hits=2)
        img, acc = ctx.readback()
        runs.append((ctx.frame_index, img, acc, ctx.read_buffer(capi.BUF_PAYLOAD)))
        ctx.close()
    (ia, imga, acca, pa), (ib, imgb, accb, pb) = runs
    assert ia == ib
    assert np.array_equal(imga, imgb) and bits_equal(acca, accb).all() and pa.tobytes() == pb.tobytes()


def test_device_memory_returns_after_close(layers):
    sc, p = layers[:2]
    base = capi.live_device_bytes()
    ctx = _ctx(sc)
    loaded = capi.live_device_bytes()
    ctx.nearest_points(p, max_hits=8, after=np.zeros(len(p), dtype=capi.POINT_HIT_DTYPE))
    n = len(p)
    staged = capi.live_device_bytes() - loaded
    assert staged >= n * (16 + 16 + 8 * 16 + 4) + 64                         # points, after, records, counts, counters: all counted
    ctx.nearest_points(p[:100], max_hits=2)
    assert capi.live_device_bytes() - loaded == staged                       # the staging is kept, a smaller call allocates nothing
    ctx.close()
    assert capi.live_device_bytes() == base


def test_torch_path_equals_host_entry():
    """Run in a fresh process that initialises torch's CUDA before the library is loaded (see test_gpu_query's torch test)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_points as t; t._torch_path_checks(); print('torch path ok')"
            % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_path_checks():
    """Points produced by torch ops, records consumed by torch ops, no synchronisation by the caller; two back-to-back device calls at
    different K (two LDS sizes), then a continuation pass from the first call's last records."""
    import torch
    sc = SCENES["hall_small"][0]()
    p = _uniform(sc, 4096, 61, scale=1.0)
    ctx = _ctx(sc, key15=1)
    want2, want8 = ctx.nearest_points(p, 4.0, max_hits=2), ctx.nearest_points(p, 4.0, max_hits=8)
    want_next = ctx.nearest_points(p, 4.0, max_hits=3, after=want2[0][:, 1].copy())
    for _ in range(2):
        pt = torch.from_numpy(p).to("cuda:0", non_blocking=True)
        big = torch.randn(2048, 2048, device="cuda:0") @ torch.randn(2048, 2048, device="cuda:0")   # (an unordered query would read unwritten points)
        pts = torch.cat([pt, torch.full((len(p), 1), 4.0, device="cuda:0")], 1).contiguous()
        h2, c2 = ctx.nearest_points_tensor(pts, 2)
        h8, c8 = ctx.nearest_points_tensor(pts, 8)
        hn, cn = ctx.nearest_points_tensor(pts, 3, after=h2[:, 1].contiguous())
        total = (c2 + c8).sum()                                               # consumed by torch ops without a synchronisation
        for (h, c), (wh, wc) in (((h2, c2), want2), ((h8, c8), want8), ((hn, cn), want_next)):
            assert h.dtype == torch.float32 and c.dtype == torch.int32 and tuple(h.shape) == wh.shape + (4,)
            got = np.ascontiguousarray(h.cpu().numpy()).view(capi.POINT_HIT_DTYPE).reshape(wh.shape)
            assert pr.records_equal(got, wh) and np.array_equal(c.cpu().numpy().astype(np.uint32), wc)
        assert int(total) == int(want2[1].sum()) + int(want8[1].sum())
        del pts, big, pt
    with pytest.raises(ValueError):
        ctx.nearest_points_tensor(torch.zeros(4, 3, device="cuda:0"), 4)
    with pytest.raises(ValueError):
        ctx.nearest_points_tensor(torch.zeros(4, 4, device="cuda:0"), 4, after=torch.zeros(3, 4, device="cuda:0"))
    ctx.close()
