"""Multi-hit queries on the GPU (fyprt_trace_ray_hits / fyprt_trace_ray_hits_device, rt_query.h: HitsLaneT behind its kernel templates).
Every comparison is bit for bit against tests/multihit_ref.py (every leaf record of ctx.export_bvh() tested, no tree): records, unused
slots and counts.
  * a stack of coplanar layers with exact-t ties, K = 1..8, both kernels of tuning key 15, with its own coverage asserted;
  * hall_small under the three builders, rays inside the scene and rays crossing all of it; K = 1 against the closest-hit query;
  * intervals; continuation passes (trace_all_hits) and finished rays; the persistent kernel's claims and the ray counters;
  * the geometry of the last edit; invalid rays, empty and misaligned calls; frames untouched; the torch path; device memory."""

import numpy as np
import pytest

import bruteforce
import multihit_ref as mh
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
    bad = mh.record_diff(gh, wh)
    assert len(bad) == 0, (tag, bad[:8], gh[bad[:2]], wh[bad[:2]])
    assert np.array_equal(gc, wc), (tag, np.nonzero(gc != wc)[0][:8])


def _same_leaf_records(a, b):
    ka, kb = np.argsort(a["tris"]["tri"]), np.argsort(b["tris"]["tri"])
    return all(np.array_equal(a["tris"][f][ka].view(np.uint32), b["tris"][f][kb].view(np.uint32)) for f in ("v0", "e1", "e2", "tri"))


# ---- the layers scene: coplanar copies give exact-t ties between different triangle indices
@pytest.fixture(scope="module")
def layers():
    sc = mh.layers_scene()
    o, d = mh.layers_rays(600)
    ctx = _ctx(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    return sc, o, d, bvh, mh.k_nearest(bvh, o, d, 0.0, np.inf, 16)            # 15 quads: 16 records hold every hit of any ray


def test_layers_every_k_both_kernels(layers):
    sc, o, d, bvh, ref = layers
    full, _, totals = ref
    assert totals.max() < 16
    tb = np.ascontiguousarray(full["t"]).view(np.uint32)
    straddles = 0
    for k in range(1, 9):
        # the coverage this test exists for: a missing case fails it
        assert (totals > k).any() and (totals == k).any() and (totals < k).any() and (totals == 0).any(), k
        straddles += int(((totals > k) & (tb[:, k - 1] == tb[:, k]) & (full["triangle"][:, k - 1] != full["triangle"][:, k])).sum())
    assert ((totals < 8) & (totals > 0)).any()
    assert straddles > 0                                                       # a tied pair straddles the K-th place
    for key15 in (1, 2):
        ctx = _ctx(sc, key15)
        for k in range(1, 9):
            _assert_equal(ctx.trace_ray_hits(o, d, max_hits=k), _truncate(ref, k), (key15, k))
        ctx.close()


# ---- hall_small: rays inside the scene and the same rays from three scene diagonals back, crossing all of it
@pytest.fixture(scope="module")
def hall_small():
    sc = SCENES["hall_small"][0]()
    o, d = bruteforce.random_rays(sc, 1500, seed=7)
    p = sc.world_vertices["position"]
    diag = F32(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    o = np.concatenate([o, (o - F32(3) * diag * d).astype(F32)])
    d = np.concatenate([d, d])
    ctx = _ctx(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    ref = mh.k_nearest(bvh, o, d, 0.0, np.inf, 8)
    assert (ref[2] > 4).any() and (ref[2] == 0).any() and np.median(ref[2][1500:]) >= 2             # K = 4 cuts lists short, the crossing rays cross
    return sc, o, d, bvh, ref, bruteforce.closest(bvh, o, d)


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_hall_small_equals_bruteforce(hall_small, builder):
    sc, o, d, bvh, ref, (best, _, ties) = hall_small
    for key15 in (1, 2):
        ctx = _ctx(sc, key15, builder=builder)
        assert _same_leaf_records(ctx.export_bvh(), bvh)                      # the reference is a function of the leaf records alone
        for k in (1, 4, 8):
            got = ctx.trace_ray_hits(o, d, max_hits=k)
            _assert_equal(got, _truncate(ref, k), (builder, key15, k))
            if k == 1:
                pay = ctx.trace_rays(o, d)
                hit = got[1] > 0
                assert np.array_equal(hit, pay["objectIndex"] >= 0) and np.array_equal(hit, best >= 0)
                assert np.array_equal(got[0]["t"][hit, 0].view(np.uint32), np.ascontiguousarray(pay["hitDistance"][hit]).view(np.uint32))
                assert all(int(got[0]["triangle"][i, 0]) in ties[i] for i in np.nonzero(hit)[0])
        ctx.close()


@pytest.mark.parametrize("budget", [1, 31])
def test_stack_budget_extremes(hall_small, budget):
    """Tuning key 8 at its ends: the smallest budget (raised to the tree's level count) makes node_step push resume entries, which visit
    a node again; the largest, with K = 8, is the 64 KB workgroup (32 stack entries x 4 B + 8 list entries x 16 B per thread)."""
    sc, o, d, bvh, ref = hall_small[:5]
    for key15 in (1, 2):
        ctx = capi.Context(0)
        ctx.set_tuning(15, key15)
        ctx.set_tuning(8, budget)
        ctx.upload_scene(sc)
        assert (ctx.get_tuning(8) == 31) == (budget == 31)
        for k in (8, 3):
            _assert_equal(ctx.trace_ray_hits(o, d, max_hits=k), _truncate(ref, k), (budget, key15, k))
        ctx.close()


@pytest.mark.parametrize("key15", [1, 2])
def test_intervals_equal_bruteforce(key15):
    """The interval cases of test_gpu_query.test_intervals_equal_bruteforce at K = 4."""
    sc = SCENES["hall_small"][0]()
    ctx = _ctx(sc, key15)
    bvh = ctx.export_bvh()
    o, d = bruteforce.random_rays(sc, 1200, seed=21)
    first = ctx.trace_rays(o, d)
    hit = first["objectIndex"] >= 0
    o, d, t0 = o[hit], d[hit], first["hitDistance"][hit].astype(F32)
    n = len(o)
    rng = np.random.default_rng(5)
    below = np.nextafter(t0, F32(0))
    above = np.nextafter(t0, F32(np.inf))
    cases = {
        "skip nearest": (t0, np.full(n, np.inf, F32)),                          # tmin = the nearest hit: t > tmin skips it
        "tmax below": (np.zeros(n, F32), below),
        "tmax at": (np.zeros(n, F32), t0),                                       # strict t < tmax: the nearest surface is excluded
        "tmax above": (np.zeros(n, F32), above),
        "window": ((t0 * F32(0.5)).astype(F32), (t0 * F32(3.0) + F32(0.5)).astype(F32)),
        "random": (rng.uniform(0, 3, n).astype(F32), rng.uniform(0.5, 12, n).astype(F32)),
    }
    for label, (lo, hi) in cases.items():
        want = mh.k_nearest(bvh, o, d, lo, hi, 4)
        _assert_equal(ctx.trace_ray_hits(o, d, lo, hi, max_hits=4), want[:2], label)
        if label == "tmax above":
            assert (want[1] >= 1).all()
        if label in ("tmax below", "tmax at"):
            assert (want[1] == 0).all()
    ctx.close()


def test_continuation_enumerates_every_hit_once(layers, hall_small):
    crossing = (hall_small[0], hall_small[1][1500:], hall_small[2][1500:], hall_small[3])        # the rays from outside the scene
    for name, (sc, o, d, bvh) in (("layers", layers[:4]), ("crossing", crossing)):
        want, want_off = mh.all_hits(bvh, o, d, 0.0, np.inf)
        for key15 in (1, 2):
            ctx = _ctx(sc, key15, counting=True)
            got, off = ctx.trace_all_hits(o, d, max_hits=3)
            assert np.array_equal(off, want_off), (name, key15)
            assert mh.records_equal(got, want), (name, key15, mh.record_diff(got, want)[:8])
            if name == "layers":
                # the tied pairs appear exactly once each: both triangles of a pair, at one t, adjacent and in index order
                keys = mh.hit_keys(got)
                tied = 0
                for i in range(len(o)):
                    k = keys[off[i]:off[i + 1]].astype(object)
                    assert (np.diff(k) > 0).all()
                    tied += int((np.diff(got["t"][off[i]:off[i + 1]].view(np.uint32).astype(np.int64)) == 0).sum())
                assert tied > 100
                # a pass's unused records passed back in: finished rays, zero hits, and they count no tests
                hits, counts = ctx.trace_ray_hits(o, d, max_hits=8)
                done = counts < 8
                assert done.any() and (hits[done, 7] == mh.UNUSED).all()
                h2, c2, st = ctx.trace_ray_hits(o[done], d[done], max_hits=8, after=hits[done, 7], with_stats=True)
                assert (c2 == 0).all() and (h2 == mh.UNUSED).all()
                assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (int(done.sum()), 0, 0, 0, 0)
                # ... while the full rays go on where they stopped
                more = ~done
                h3, c3 = ctx.trace_ray_hits(o[more], d[more], max_hits=8, after=hits[more, 7])
                w3 = mh.k_nearest(bvh, o[more], d[more], 0.0, np.inf, 8, after=hits[more, 7])
                _assert_equal((h3, c3), w3[:2], "after")
                assert (c3 > 0).any()
            ctx.close()


def test_persistent_kernel_claims_and_counters(hall_small):
    """Small static chunks (key 4 = 16 rays per claim, key 9 = 1 static chunk per wave, key 10 = 16) leave most rays to the claims from the
    shared head; two consecutive calls (the head is reset per call), counted and not, give the same records."""
    sc, _, _, bvh = hall_small[:4]
    o, d = bruteforce.random_rays(sc, 6000, seed=71)
    want = mh.k_nearest(bvh, o, d, 0.0, np.inf, 4)
    ctx = _ctx(sc, key15=1, counting=True)
    for key, value in ((4, 16), (9, 1), (10, 16)):
        ctx.set_tuning(key, value)
    counted = []
    for _ in range(2):
        hits, counts, st = ctx.trace_ray_hits(o, d, max_hits=4, with_stats=True)
        _assert_equal((hits, counts), want[:2], "counted")
        assert st.rays == len(o) == st.part_rays[0] and st.hits == int((counts > 0).sum()) == st.part_hits[0]
        assert st.launches == 1 and st.kernel_ms > 0.0 and st.tri_tests > 0 and st.node_visits > 0 and st.box_tests > st.node_visits
        counted.append((st.box_tests, st.tri_tests, st.node_visits))
    assert counted[0] == counted[1]
    ctx.set_ray_counting(False)
    for _ in range(2):
        _assert_equal(ctx.trace_ray_hits(o, d, max_hits=4), want[:2], "uncounted")
    ctx.close()


def test_queries_see_current_geometry():
    mk_scene, mk_cam = SCENES["hall_small"]
    sc = mk_scene()
    cam = mk_cam(64, 64)
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    ctx = _ctx(sc)
    ctx.set_object_vertices(sc)
    o, d = bruteforce.random_rays(sc, 1200, seed=51)
    before = ctx.trace_ray_hits(o, d, max_hits=4)
    _assert_equal(before, mh.k_nearest(ctx.export_bvh(), o, d, 0.0, np.inf, 4)[:2], "before")
    mgr.set_mesh_transform(sc, 3, pos=(0.7, 0.0, -0.4), rotation=(0, 25, 0))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_transforms(sc, [3])
    moved = ctx.trace_ray_hits(o, d, max_hits=4)
    _assert_equal(moved, mh.k_nearest(ctx.export_bvh(), o, d, 0.0, np.inf, 4)[:2], "update_transforms")
    assert not mh.records_equal(moved[0], before[0])                          # the edit is visible to the query
    first = append_patch(sc, cam, "hall_small", 300, 0)
    ctx.append_meshes(sc, first)
    grown = ctx.trace_ray_hits(o, d, max_hits=4)
    bvh = ctx.export_bvh()
    assert len(bvh["tris"]) == len(sc.triangles)
    _assert_equal(grown, mh.k_nearest(bvh, o, d, 0.0, np.inf, 4)[:2], "append_meshes")
    # rays at the patch: from the camera, where it was placed
    dirs = cam.ray_directions().reshape(-1, 3).astype(F32)[::7]
    oc = np.broadcast_to(np.asarray(cam.position, F32), dirs.shape)
    at_patch = ctx.trace_ray_hits(oc, dirs, max_hits=4)
    _assert_equal(at_patch, mh.k_nearest(bvh, oc, dirs, 0.0, np.inf, 4)[:2], "patch")
    assert (at_patch[0]["triangle"][at_patch[0]["t"] > 0] >= len(sc.triangles) - 300).any()
    ctx.close()


def test_invalid_rays_empty_and_misaligned_calls():
    sc = SCENES["cornell"][0]()
    ctx = _ctx(sc)
    cam = SCENES["cornell"][1](8, 8)
    c = np.asarray(cam.position, F32)
    good_d = np.asarray(cam.ray_directions().reshape(-1, 3)[27], F32)
    nan, inf = F32(np.nan), F32(np.inf)
    rays = [  # (origin, direction, tmin, tmax)
        ((nan, 0, 0), good_d, 0, inf), (c, (good_d[0], nan, good_d[2]), 0, inf), ((inf, 0, 0), good_d, 0, inf), (c, (0, 0, -inf), 0, inf),
        (c, good_d, nan, inf), (c, good_d, 0, nan), (c, good_d, 2.0, 2.0), (c, good_d, 3.0, 1.0), (c, (0, 0, 0), 0, inf),
    ]
    o = np.array([r[0] for r in rays], F32)
    d = np.array([r[1] for r in rays], F32)
    lo = np.array([r[2] for r in rays], F32)
    hi = np.array([r[3] for r in rays], F32)
    assert ctx.trace_ray_hits(c[None], good_d[None], max_hits=2)[1][0] >= 1     # the valid version of the ray hits
    for key15 in (1, 2):
        ctx.set_tuning(15, key15)
        for k in (1, 8):
            hits, counts = ctx.trace_ray_hits(o, d, lo, hi, max_hits=k)
            assert (counts == 0).all() and (hits == mh.UNUSED).all(), (key15, k)
        ctx.set_ray_counting(True)                                            # the invalid ones (all but the zero direction): rays without tests
        st = ctx.trace_ray_hits(o[:-1], d[:-1], lo[:-1], hi[:-1], max_hits=3, with_stats=True)[2]
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (len(o) - 1, 0, 0, 0, 0)
        ctx.set_ray_counting(False)
        # a NULL hit_counts: the records alone
        rr = np.zeros(2, dtype=capi.RAY_DTYPE)
        rr["origin"], rr["direction"], rr["tmax"] = c, good_d, np.inf
        out = np.zeros((2, 3), dtype=capi.RAY_HIT_DTYPE)
        assert ctx.lib.fyprt_trace_ray_hits(ctx.h, rr.ctypes.data, None, 2, 3, out.ctypes.data, None, None) == 0
        want = ctx.trace_ray_hits(rr["origin"], rr["direction"], max_hits=3)[0]
        assert mh.records_equal(out, want) and out["t"][0, 0] > 0
    # count 0: OK, nothing launched
    e = np.zeros(0, dtype=capi.RAY_DTYPE)
    assert ctx.lib.fyprt_trace_ray_hits(ctx.h, e.ctypes.data, None, 0, 4, None, None, None) == 0
    assert ctx.lib.fyprt_trace_ray_hits_device(ctx.h, None, None, 0, 4, None, None) == 0
    hits, counts = ctx.trace_ray_hits(np.zeros((0, 3)), np.zeros((0, 3)), max_hits=5)
    assert hits.shape == (0, 5) and counts.shape == (0,)
    rec, off = ctx.trace_all_hits(np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(rec) == 0 and off.tolist() == [0]
    # misaligned device pointers (device memory of the context: its image buffer, 16-byte aligned; refused before any launch)
    ctx.resize(16, 16)
    img = ctx.image_device_ptr()
    dev = ctx.lib.fyprt_trace_ray_hits_device
    assert dev(ctx.h, img + 4, None, 1, 1, img + 64, img + 128) == -1
    assert dev(ctx.h, img, img + 72, 1, 1, img + 64, img + 128) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 72, img + 128) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 64, img + 130) == -1
    assert dev(ctx.h, img, None, 1, 0, img + 64, None) == -1 and dev(ctx.h, img, None, 1, 9, img + 64, None) == -1
    ctx.close()


def test_queries_leave_frames_untouched(hall_small):
    sc, W, H = hall_small[0], 96, 64
    cam = SCENES["hall_small"][1](W, H)
    o, d = hall_small[1][::3], hall_small[2][::3]
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
                ctx.trace_ray_hits(o, d, max_hits=8)
                ctx.trace_all_hits(o[:200], d[:200], max_hits=2)
        img, acc = ctx.readback()
        runs.append((ctx.frame_index, img, acc, ctx.read_buffer(capi.BUF_PAYLOAD)))
        ctx.close()
    (ia, imga, acca, pa), (ib, imgb, accb, pb) = runs
    assert ia == ib
    assert np.array_equal(imga, imgb) and bits_equal(acca, accb).all() and pa.tobytes() == pb.tobytes()


def test_device_memory_returns_after_close(layers):
    sc, o, d = layers[:3]
    base = capi.live_device_bytes()
    ctx = _ctx(sc)
    loaded = capi.live_device_bytes()
    ctx.trace_ray_hits(o, d, max_hits=8, after=np.zeros(len(o), dtype=capi.RAY_HIT_DTYPE))
    n = len(o)
    staged = capi.live_device_bytes() - loaded
    assert staged >= n * (32 + 16 + 8 * 16 + 4) + 64                         # rays, after, records, counts, counters: all counted
    ctx.trace_ray_hits(o[:100], d[:100], max_hits=2)
    assert capi.live_device_bytes() - loaded == staged                       # the staging is kept, a smaller call allocates nothing
    ctx.close()
    assert capi.live_device_bytes() == base


def test_torch_path_equals_host_entry():
    """Run in a fresh process that initialises torch's CUDA before the library is loaded (see test_gpu_query's torch test)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_multihit as t; t._torch_path_checks(); print('torch path ok')"
            % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_path_checks():
    """Rays produced by torch ops, records consumed by torch ops, no synchronisation by the caller; two back-to-back device calls at
    different K (two LDS sizes: the occupancy entry is asked again), then a continuation pass from the first call's last records."""
    import torch
    sc = SCENES["hall_small"][0]()
    o, d = bruteforce.random_rays(sc, 4096, seed=61)
    ctx = _ctx(sc, key15=1)
    want2, want8 = ctx.trace_ray_hits(o, d, max_hits=2), ctx.trace_ray_hits(o, d, max_hits=8)
    want_next = ctx.trace_ray_hits(o, d, max_hits=3, after=want2[0][:, 1].copy())
    for _ in range(2):
        ot = torch.from_numpy(o).to("cuda:0", non_blocking=True)
        dt = torch.from_numpy(d).to("cuda:0", non_blocking=True)
        big = torch.randn(2048, 2048, device="cuda:0") @ torch.randn(2048, 2048, device="cuda:0")   # (an unordered query would read unwritten rays)
        rays = torch.cat([ot, torch.zeros(len(o), 1, device="cuda:0"), dt, torch.full((len(o), 1), float("inf"), device="cuda:0")], 1).contiguous()
        h2, c2 = ctx.trace_ray_hits_tensor(rays, 2)
        h8, c8 = ctx.trace_ray_hits_tensor(rays, 8)
        hn, cn = ctx.trace_ray_hits_tensor(rays, 3, after=h2[:, 1].contiguous())
        total = (c2 + c8).sum()                                               # consumed by torch ops without a synchronisation
        for (h, c), (wh, wc) in (((h2, c2), want2), ((h8, c8), want8), ((hn, cn), want_next)):
            assert h.dtype == torch.float32 and c.dtype == torch.int32 and tuple(h.shape) == wh.shape + (4,)
            got = np.ascontiguousarray(h.cpu().numpy()).view(capi.RAY_HIT_DTYPE).reshape(wh.shape)
            assert mh.records_equal(got, wh) and np.array_equal(c.cpu().numpy().astype(np.uint32), wc)
        assert int(total) == int(want2[1].sum()) + int(want8[1].sum())
        del rays, big, ot, dt
    with pytest.raises(ValueError):
        ctx.trace_ray_hits_tensor(torch.zeros(4, 7, device="cuda:0"), 4)
    with pytest.raises(ValueError):
        ctx.trace_ray_hits_tensor(torch.zeros(4, 8, device="cuda:0"), 4, after=torch.zeros(3, 4, device="cuda:0"))
    ctx.close()
