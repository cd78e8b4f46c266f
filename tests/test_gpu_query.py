"""Batched ray queries on the GPU (fyprt_trace_rays / fyprt_trace_rays_device, rt_query.h):
  * default interval: the whole 40-byte record equals the oracle's twin of the product traversal (Oracle.trace on ctx.export_bvh()),
    for both kernels of tuning key 15, and counted queries count exactly what the oracle counts;
  * intervals and occlusion: the nearest / any accepted triangle equals tests/bruteforce.py (every leaf record tested, no tree);
  * invalid rays, empty and misaligned calls; the geometry of the last transform edit / device-built tree;
  * camera rays of the 1M-triangle bench hall at 1920x1080 equal the payload a ReSTIR DI Part 1 writes, bit for bit;
  * the torch path is ordered against torch's stream on the device, and queries leave frames untouched."""
import numpy as np
import pytest

import bruteforce
from common import SCENES, bits_equal, settings_for
from edit_sequences import _scene_bvh
from fypraytracer_amd import capi, scenes

pytestmark = pytest.mark.gpu

F32 = np.float32


def _ctx(sc, key15=0, counting=False):
    ctx = capi.Context(0)
    ctx.set_tuning(15, key15)
    ctx.upload_scene(sc)
    ctx.set_ray_counting(counting)
    return ctx


def _oracle_trace(orc, o, d):
    """Oracle.trace per ray: the payloads and the summed (rays, box tests, triangle tests, hits, node visits)."""
    pay = np.zeros(len(o), dtype=capi.PAYLOAD_DTYPE)
    cnt = np.zeros(5, dtype=np.int64)
    for i in range(len(o)):
        p, c = orc.trace(o[i], d[i])
        pay[i] = p
        cnt += (1, c["box_tests"], c["tri_tests"], int(p["objectIndex"] >= 0), c["node_visits"])
    return pay, tuple(int(x) for x in cnt)


def _record_diff(a, b):
    """Indices of the 40-byte records that differ in any bit."""
    a8, b8 = np.ascontiguousarray(a).view(np.uint8).reshape(-1, 40), np.ascontiguousarray(b).view(np.uint8).reshape(-1, 40)
    assert a8.shape == b8.shape
    return np.nonzero((a8 != b8).any(axis=1))[0]


def _records_equal(a, b):
    return len(_record_diff(a, b)) == 0


def _camera_like_rays(sc, cam_fn, n, seed):
    """Half random rays through the scene, half rays from the scene's camera position through random viewport points."""
    o, d = bruteforce.random_rays(sc, n, seed)
    cam = cam_fn(64, 64)
    dirs = cam.ray_directions().reshape(-1, 3).astype(F32)
    pick = np.random.default_rng(seed + 1).integers(0, len(dirs), n // 2)
    o[: n // 2] = np.asarray(cam.position, dtype=F32)
    d[: n // 2] = dirs[pick]
    return o, d


@pytest.mark.parametrize("name", ["cornell", "hall_small", "banana"])
def test_default_interval_equals_oracle(oracle_built, name):
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES[name]
    sc = mk_scene()
    o, d = _camera_like_rays(sc, mk_cam, 3000, seed=len(name))
    ref = None
    for key15 in (1, 2):
        ctx = _ctx(sc, key15, counting=True)
        if ref is None:
            orc = Oracle(sc, 8, 8)
            orc.use_product_bvh(ctx.export_bvh())
            ref, ref_counts = _oracle_trace(orc, o, d)
            orc.close()
            assert (ref["objectIndex"] >= 0).sum() > len(o) // 4
        got, st = ctx.trace_rays(o, d, with_stats=True)
        assert _records_equal(got, ref), (key15, _record_diff(got, ref)[:10])
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == ref_counts, key15
        assert (st.part_rays[0], st.part_box_tests[0], st.part_tri_tests[0], st.part_hits[0], st.part_node_visits[0]) == ref_counts
        assert st.launches == 1 and st.kernel_ms > 0.0
        ctx.set_ray_counting(False)
        assert _records_equal(ctx.trace_rays(o, d), ref)                 # the production (uncounted) kernels give the same records
        ctx.close()


def _last_frame_ms(ctx):
    import ctypes as C
    ms = C.c_float()
    ctx._check(ctx.lib.fyprt_last_frame_ms(ctx.h, C.byref(ms)))
    return ms.value


def test_query_leaves_counted_frames_untouched():
    mk_scene, mk_cam = SCENES["hall_small"]
    sc, W, H = mk_scene(), 96, 64
    cam = mk_cam(W, H)
    o, d = bruteforce.random_rays(sc, 5000, seed=3)
    runs = []
    for with_query in (False, True):
        ctx = _ctx(sc, counting=True)
        ctx.resize(W, H)
        ctx.set_camera(cam)
        st = settings_for(capi.RESTIR_DI)
        stats = []
        for f in range(3):
            st.rand_seed = f + 1
            stats.append(ctx.render(st))
            if with_query:
                # the frame's timings as the library keeps them, read before and after the queries on the same context
                timings = [ctx.frame_timings(k) for k in range(f + 1)], _last_frame_ms(ctx)
                q = ctx.trace_rays(o, d, with_stats=True)[1]
                assert (q.rays, q.part_rays[0], q.launches) == (len(o), len(o), 1)    # the query's own counters, not the frame's
                ctx.trace_rays(o, d, tmax=2.0, occluded=True)
                assert ([ctx.frame_timings(k) for k in range(f + 1)], _last_frame_ms(ctx)) == timings
        fields = [(s.rays, s.box_tests, s.tri_tests, s.hits, s.node_visits, tuple(s.part_rays), tuple(s.part_node_visits), s.launches) for s in stats]
        img, acc = ctx.readback()
        runs.append((fields, ctx.frame_index, img, acc, ctx.read_buffer(capi.BUF_PAYLOAD)))
        ctx.close()
    (fa, ia, imga, acca, pa), (fb, ib, imgb, accb, pb) = runs
    assert fa == fb and ia == ib
    assert np.array_equal(imga, imgb) and bits_equal(acca, accb).all() and _records_equal(pa, pb)


def test_persistent_kernel_dynamic_claims(oracle_built):
    """Small static chunks (key 4 = 16 rays per claim, key 9 = 1 static chunk per wave) leave most rays to the claims from the shared
    head; two consecutive queries on one context (the head is reset per query), counted and not, give the oracle's records."""
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES["hall_small"]
    sc = mk_scene()
    o, d = _camera_like_rays(sc, mk_cam, 6000, seed=71)
    ctx = _ctx(sc, key15=1, counting=True)
    for key, value in ((4, 16), (9, 1), (10, 16)):
        ctx.set_tuning(key, value)
    orc = Oracle(sc, 8, 8)
    orc.use_product_bvh(ctx.export_bvh())
    ref, ref_counts = _oracle_trace(orc, o, d)
    orc.close()
    for _ in range(2):
        got, st = ctx.trace_rays(o, d, with_stats=True)
        assert _records_equal(got, ref), _record_diff(got, ref)[:10]
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == ref_counts
    ctx.set_ray_counting(False)
    for _ in range(2):
        assert _records_equal(ctx.trace_rays(o, d), ref)
        lo = np.full(len(o), 0.05, F32)
        assert np.array_equal(ctx.trace_rays(o, d, lo, 3.0, occluded=True), bruteforce.occluded(ctx.export_bvh(), o, d, lo, 3.0))
    ctx.close()


@pytest.mark.parametrize("key15", [1, 2])
def test_intervals_equal_bruteforce(key15):
    sc = SCENES["hall_small"][0]()
    ctx = _ctx(sc, key15)
    bvh = ctx.export_bvh()
    o, d = _camera_like_rays(sc, SCENES["hall_small"][1], 2000, seed=21)
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
        got = ctx.trace_rays(o, d, tmin=lo, tmax=hi)
        best, _, ties = bruteforce.closest(bvh, o, d, lo, hi)
        bad = bruteforce.check_closest(got, best, ties)
        assert bad == [], (label, bad[:5])
    ctx.close()


@pytest.mark.parametrize("key15", [1, 2])
def test_occlusion_equals_bruteforce(key15):
    sc = SCENES["hall_small"][0]()
    ctx = _ctx(sc, key15)
    bvh = ctx.export_bvh()
    rng = np.random.default_rng(17 + key15)
    o, d = _camera_like_rays(sc, SCENES["hall_small"][1], 6000, seed=31)
    first = ctx.trace_rays(o, d)
    hit = first["objectIndex"] >= 0
    p = first["worldPosition"][hit].astype(F32)
    # (a) shadow segments from hit points to random points on random emissive triangles, tmax = 0.999 (direction = the whole segment)
    em = sc.init_scene_emissive_triangles()
    pos = sc.world_vertices["position"]
    tri = sc.triangles[em[rng.integers(0, len(em), len(p))]]
    r1, r2 = rng.random(len(p), dtype=F32), rng.random(len(p), dtype=F32)
    s = np.sqrt(r1)
    q = ((1 - s)[:, None] * pos[tri["v0"]] + ((1 - r2) * s)[:, None] * pos[tri["v1"]] + (r2 * s)[:, None] * pos[tri["v2"]]).astype(F32)
    seg_o, seg_d = p, (q - p).astype(F32)
    seg_lo, seg_hi = np.full(len(p), 1e-3, F32), np.full(len(p), 0.999, F32)
    # (b) tmax exactly a surface's hit distance (strict <), with and without a positive tmin
    t0 = first["hitDistance"][hit].astype(F32)
    b_lo = np.where(rng.random(len(t0)) < 0.5, F32(0), (t0 * rng.uniform(0, 0.9, len(t0))).astype(F32)).astype(F32)
    # (c) random segments with tmin > 0
    c_o, c_d = bruteforce.random_rays(sc, 4000, seed=41)
    c_lo = rng.uniform(0.01, 2.0, len(c_o)).astype(F32)
    c_hi = (c_lo + rng.uniform(0.0, 4.0, len(c_o))).astype(F32)
    O = np.concatenate([seg_o, o[hit], c_o])
    D = np.concatenate([seg_d, d[hit], c_d])
    LO = np.concatenate([seg_lo, b_lo, c_lo])
    HI = np.concatenate([seg_hi, t0, c_hi])
    assert len(O) >= 10000
    got = ctx.trace_rays(O, D, tmin=LO, tmax=HI, occluded=True)
    ref = bruteforce.occluded(bvh, O, D, LO, HI)
    assert got.dtype == bool and np.array_equal(got, ref), np.nonzero(got != ref)[0][:10]
    assert 0 < ref.sum() < len(ref)
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
    assert ctx.trace_rays(c[None], good_d[None])["objectIndex"][0] >= 0            # the valid version of the ray hits
    for key15 in (1, 2):
        ctx.set_tuning(15, key15)
        got = ctx.trace_rays(o, d, lo, hi)
        assert (got["hitDistance"] == -1).all() and (got["objectIndex"] == -1).all(), key15
        assert not ctx.trace_rays(o, d, lo, hi, occluded=True).any(), key15
        ctx.set_ray_counting(True)                                            # the invalid ones (all but the zero direction): rays without tests
        st = ctx.trace_rays(o[:-1], d[:-1], lo[:-1], hi[:-1], with_stats=True)[1]
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (len(o) - 1, 0, 0, 0, 0)
        ctx.set_ray_counting(False)
    # count 0: OK, nothing launched
    e = np.zeros(0, dtype=capi.RAY_DTYPE)
    assert ctx.lib.fyprt_trace_rays(ctx.h, capi.QUERY_CLOSEST, e.ctypes.data, 0, None, None) == 0
    assert ctx.lib.fyprt_trace_rays_device(ctx.h, capi.QUERY_OCCLUDED, None, 0, None) == 0
    assert len(ctx.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    # misaligned device pointers (device memory of the context: its image buffer, 16-byte aligned; refused before any launch)
    ctx.resize(16, 16)
    img = ctx.image_device_ptr()
    assert ctx.lib.fyprt_trace_rays_device(ctx.h, capi.QUERY_CLOSEST, img + 4, 1, img + 64) == -1
    assert ctx.lib.fyprt_trace_rays_device(ctx.h, capi.QUERY_CLOSEST, img, 1, img + 36) == -1
    ctx.close()


def test_queries_see_current_geometry(oracle_built):
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES["hall_small"]
    sc = mk_scene()
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    ctx = _ctx(sc)
    ctx.set_object_vertices(sc)
    o, d = _camera_like_rays(sc, mk_cam, 1500, seed=51)
    before = ctx.trace_rays(o, d)
    mgr.set_mesh_transform(sc, 3, pos=(0.7, 0.0, -0.4), rotation=(0, 25, 0))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_transforms(sc, [3])
    got = ctx.trace_rays(o, d)
    best, _, ties = bruteforce.closest(_scene_bvh(sc), o, d)
    assert bruteforce.check_closest(got, best, ties) == []
    assert not _records_equal(got, before)                                   # the edit is visible to the query
    lo = np.full(len(o), 0.05, F32)
    assert np.array_equal(ctx.trace_rays(o, d, lo, 3.0, occluded=True), bruteforce.occluded(_scene_bvh(sc), o, d, lo, 3.0))
    ctx.close()
    for builder in (1, 2):                                                   # device LBVH / PLOC trees
        ctx = capi.Context(0)
        ctx.set_tuning(12, builder)
        ctx.upload_scene(sc)
        orc = Oracle(sc, 8, 8)
        orc.use_product_bvh(ctx.export_bvh())
        ref, _ = _oracle_trace(orc, o, d)
        assert _records_equal(ctx.trace_rays(o, d), ref), builder
        orc.close()
        ctx.close()


@pytest.fixture(scope="module")
def hall():
    return scenes.hall_scene()


def test_camera_rays_equal_restir_part1_payload_1080p(oracle_built, hall):
    """The bench hall (1M triangles, persistent kernel) at 1920x1080: camera rays of rows [0, 64) and every 17th row, directions from the
    oracle's camera, equal the payload ReSTIR DI Part 1 writes for those pixels bit for bit."""
    from oraclelib import Oracle
    import ctypes as C
    W, H = 1920, 1080
    cam = scenes.hall_camera(W, H)
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(hall)
    ctx.set_camera(cam)
    ctx.render_part(settings_for(capi.RESTIR_DI), 1)
    frame = ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    rows = sorted(set(range(64)) | set(range(0, H, 17)))
    orc = Oracle(scenes.hall_scene_small(), W, H)                             # (only its camera is used: ray directions)
    orc.set_camera(cam)
    out3 = np.zeros(3, F32)
    d = np.zeros((len(rows), W, 3), F32)
    for k, y in enumerate(rows):
        for x in range(W):
            orc.lib.orc_ray_direction(orc.h, x, y, out3.ctypes.data_as(C.c_void_p))
            d[k, x] = out3
    orc.close()
    o = np.broadcast_to(np.asarray(cam.position, F32), d.shape).reshape(-1, 3)
    got = ctx.trace_rays(o, d.reshape(-1, 3))
    assert _records_equal(got, frame[rows].reshape(-1))
    assert (got["objectIndex"] >= 0).mean() > 0.5
    ctx.close()


def test_torch_path_is_ordered_and_leaves_frames_untouched():
    """Run in a fresh process that initialises torch's CUDA before the library is loaded, as bench.py does.  Then the library binds to
    torch's HIP runtime (the same SONAME).  In a process where the library came first, as in this test process, torch loads a second
    runtime and finds no GPU."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_query as t; t._torch_path_checks(); print('torch path ok')"
            % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_path_checks():
    """Rays produced by torch ops, results consumed by torch ops, no synchronisation by the caller; queries interleaved with asynchronous
    frames change nothing of them (a second context renders the same frames without queries)."""
    import torch
    mk_scene, mk_cam = SCENES["hall_small"]
    sc, W, H = mk_scene(), 128, 72
    cam = mk_cam(W, H)
    o, d = _camera_like_rays(sc, mk_cam, 4096, seed=61)
    ctxs = []
    for _ in range(2):
        c = capi.Context(0)
        c.resize(W, H)
        c.upload_scene(sc)
        c.set_camera(cam)
        ctxs.append(c)
    a, b = ctxs
    hip = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(hip) == 1, hip                                                 # one HIP runtime: the context stream is one of torch's
    want = a.trace_rays(o, d)
    want_occ = a.trace_rays(o, d, tmin=0.01, tmax=2.5, occluded=True)
    st = settings_for(capi.RESTIR_DI)
    results = []
    for f in range(3):
        st.rand_seed = f + 1
        a.render_async(st)
        b.render_async(st)
        # rays produced by torch ops on torch's stream (a big op first, so that an unordered query would read unwritten memory)
        ot = torch.from_numpy(o).to("cuda:0", non_blocking=True)
        dt = torch.from_numpy(d).to("cuda:0", non_blocking=True)
        big = torch.randn(4096, 4096, device="cuda:0") @ torch.randn(4096, 4096, device="cuda:0")
        rays = torch.cat([ot, torch.zeros(len(o), 1, device="cuda:0"), dt, torch.full((len(o), 1), float("inf"), device="cuda:0")], 1).contiguous()
        out = a.trace_rays_tensor(rays)
        hd = out[:, 0] * 1.0                                                  # consumed by torch ops without a synchronisation
        obj = out[:, 9].contiguous().view(torch.int32) + 0
        seg = rays.clone()
        seg[:, 3], seg[:, 7] = 0.01, 2.5
        occ = a.trace_rays_tensor(seg, occluded=True) * 1
        results.append((hd, obj, out, occ))
        del rays, seg, big, ot, dt
    for hd, obj, out, occ in results:
        got = np.ascontiguousarray(out.cpu().numpy()).view(capi.PAYLOAD_DTYPE).reshape(-1)
        assert _records_equal(got, want)
        assert np.array_equal(hd.cpu().numpy().view(np.uint32), want["hitDistance"].view(np.uint32))
        assert np.array_equal(obj.cpu().numpy(), want["objectIndex"])
        assert occ.dtype == torch.int32 and np.array_equal(occ.cpu().numpy().astype(bool), want_occ)
    (ia, aa), (ib, ab) = a.readback(), b.readback()
    assert np.array_equal(ia, ib) and bits_equal(aa, ab).all() and a.frame_index == b.frame_index
    with pytest.raises(ValueError):
        a.trace_rays_tensor(torch.zeros(4, 7, device="cuda:0"))
    a.close()
    b.close()
