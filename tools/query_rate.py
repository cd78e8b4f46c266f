#!/usr/bin/env python3
"""Rate of the batched ray queries (fyprt_trace_rays) on fixed ray sets of the bench hall (1M triangles, 1920x1080), GPU.
  (a) camera rays, row-major, closest hit                 (b) cosine-hemisphere bounce rays from the camera hits, closest hit
  (c) shadow segments from each hit to a seeded random point on a random emissive triangle, tmax = 0.999 x distance, occlusion
  (d) set (a) on hall_small (11 k triangles: the one-thread-per-ray side of tuning key 15)
One JSON line per set: rays, median hipEvent ms of the query launch over --calls calls after warm-up, Mrays/s, node visits per ray
(one counted call).  The same run times ReSTIR DI Part 1 stand-alone (fyprt_render_part(..., 1)), which traces the camera rays of (a)
and does its reservoir work on top.
  usage: python tools/query_rate.py [--calls 20] [--out FILE.jsonl]
With --hits K [K ...]: the multi-hit query (fyprt_trace_ray_hits) instead, on sets (a), (b) and (c) (the shadow segments as rays with
their tmax): per set one line for FYPRT_QUERY_CLOSEST and one per K, timed in the same run on the same rays — median, minimum and
maximum hipEvent ms over --calls calls after warm-up, Mrays/s, records (hits) per second, and the ratio to the closest-hit query.
Written to profiles/query/hits_rate.jsonl unless --out names another file.
  usage: python tools/query_rate.py --hits 1 2 4 8 [--calls 20] [--out FILE.jsonl]
With --points K [K ...]: the nearest-point query (fyprt_nearest_points) on three sets of 1920x1080 points — (a) the camera hits pushed
1 % of the scene diameter along the normal, (b) uniform in the scene box, (c) uniform in a box three diameters wide: per set and K the
median, minimum and maximum hipEvent ms, Mpoints/s, node visits, box and triangle tests per point (one counted call), and the ratio
to the closest-hit query of the camera rays, timed in the same run.  Written to profiles/query/points_rate.jsonl unless --out names
another file.
  usage: python tools/query_rate.py --points 1 4 8 [--calls 20] [--out FILE.jsonl]
With --boxes K [K ...]: the box-overlap query (fyprt_overlap_boxes) on three sets of 1920x1080 boxes centred on the camera hits, with
half extents of 0.1 %, 0.5 % and 2 % of the scene diameter: per set and K the median, minimum and maximum hipEvent ms, Mboxes/s, node
visits, box and triangle tests and accepted triangles per box (one counted call), and the ratio to the closest-hit query of the camera
rays, timed in the same run.  Written to profiles/query/boxes_rate.jsonl unless --out names another file.  --key15 V sets tuning key 15
(1: persistent waves, 2: one thread per box) and --mask-table a mesh mask table of all ones (the filtered kernels, every triangle
admitted) before anything is timed; both are noted in every row.  (FYPRT_LIB names another build of the library: A/B runs.)
  usage: python tools/query_rate.py --boxes 1 8 32 [--key15 V] [--mask-table] [--calls 20] [--out FILE.jsonl]
With --triangles K [K ...]: the triangle-overlap query (fyprt_overlap_triangles).  The query triangles are the triangles of the bench
hall's largest mesh (at most 262 144 of them) under three offsets: (a) where the mesh lies, (b) moved by half its size along its longest
axis, (c) moved two scene diameters away, clear of everything.  Per set and K the median, minimum and maximum hipEvent ms, Mtriangles/s,
node visits, box and triangle tests and accepted triangles per query (one counted call); and, from the same process on the same
triangles' bounding boxes at the same K, the box-overlap query's figures and the ratio of the two medians.  --key15 and --mask-table as
for --boxes.  Written to profiles/query/triangles_rate.jsonl unless --out names another file.
  usage: python tools/query_rate.py --triangles 1 8 32 [--key15 V] [--mask-table] [--calls 20] [--out FILE.jsonl]
With --triangles-summary FILE [FILE ...]: no GPU; the files of several --triangles processes folded into one line per (key 15, mask
table, set, K) — the median of the processes' medians for both queries, every process's median, their ratio and the counters — written
to profiles/query/triangles_rate_summary.jsonl unless --out names another file, and printed as a table.
  usage: python tools/query_rate.py --triangles-summary profiles/query/triangles_rate_key*_run*.jsonl
With --filter: the query filter (fyprt_set_mesh_query_masks / fyprt_set_query_mask) on the bench hall.  Two contexts hold the scene, one
with a mesh mask table and one without; per case the four families (closest hit, hits K = 4, nearest points, boxes K = 8) are timed on
the same records, the two contexts' calls alternating: (1) a table and a query mask of all ones — the price of the checks; (2) one
column excluded, nearest points at K = 1 placed on that column's own surface — the snap case; (3) only that column admitted, with the
camera rays and whole-scene boxes.  Per row the median, minimum and maximum hipEvent ms of both launches, their ratio, and node visits
and triangle tests per record of both (one counted call each).  Written to profiles/query/filter_rate.jsonl unless --out names
another file.
  usage: python tools/query_rate.py --filter [--calls 20] [--out FILE.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch  # noqa: E402  (torch's HIP runtime is initialised before the library's, as bench.py does: Part 1 is timed with torch events)

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from common import settings_for  # noqa: E402
from fypraytracer_amd import capi, scenes  # noqa: E402

F32 = np.float32


def rate(ctx, name, scene, o, d, calls, tmin=0.0, tmax=np.inf, occluded=False):
    for _ in range(3):
        ctx.trace_rays(o, d, tmin, tmax, occluded=occluded)
    ms = [ctx.trace_rays(o, d, tmin, tmax, occluded=occluded, with_stats=True)[1].kernel_ms for _ in range(calls)]
    ctx.set_ray_counting(True)
    res, st = ctx.trace_rays(o, d, tmin, tmax, occluded=occluded, with_stats=True)
    ctx.set_ray_counting(False)
    med = statistics.median(ms)
    hits = int(res.sum()) if occluded else int((res["objectIndex"] >= 0).sum())
    return {"set": name, "scene": scene, "query": "occluded" if occluded else "closest", "rays": len(o), "ms_median": round(med, 4),
            "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": calls, "mrays_per_s": round(len(o) / med / 1e3, 1),
            "node_visits_per_ray": round(st.node_visits / st.rays, 3), "box_tests_per_ray": round(st.box_tests / st.rays, 3),
            "tri_tests_per_ray": round(st.tri_tests / st.rays, 3), "hit_fraction": round(hits / len(o), 4)}, res


def part1_ms(ctx, calls):
    """ReSTIR DI Part 1 alone (fyprt_render_part(..., 1) runs on the context stream): device-event time of its launches."""
    st = settings_for(capi.RESTIR_DI)
    stream = torch.cuda.ExternalStream(ctx.stream())
    ms = []
    for f in range(calls + 3):
        st.rand_seed = f + 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.render_part(st, 1)
        e1.record(stream)
        ctx.synchronize()
        if f >= 3:
            ms.append(e0.elapsed_time(e1))
        ctx.render_part(st, 2)
        ctx.synchronize()
    return statistics.median(ms), min(ms), max(ms)


def query_ms_torch_events(ctx, o, d, calls):
    """The camera query of (a) timed like Part 1 (torch events on the context stream around fyprt_trace_rays_device): checks that this
    way of timing agrees with the library's own hipEvents (kernel_ms of the host entry)."""
    rays = torch.from_numpy(np.concatenate([o, np.zeros((len(o), 1), F32), d, np.full((len(o), 1), np.inf, F32)], 1)).cuda()
    out = torch.empty((len(o), 10), dtype=torch.float32, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream())
    torch.cuda.synchronize()
    ms = []
    for f in range(calls + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx._check(ctx.lib.fyprt_trace_rays_device(ctx.h, capi.QUERY_CLOSEST, rays.data_ptr(), len(o), out.data_ptr()))
        e1.record(stream)
        ctx.synchronize()
        if f >= 3:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def camera_rays(cam):
    d = cam.ray_directions().reshape(-1, 3).astype(F32)           # row-major, row 0 first (the frame's pixel order)
    o = np.broadcast_to(np.asarray(cam.position, F32), d.shape).copy()
    return o, d


def hall_ray_sets(hall, d, rng, camera_hits):
    """The sets (b) and (c) derived from the camera hits of (a): (bounce origins, bounce directions), (shadow directions, tmax)."""
    res = camera_hits
    hit = res["objectIndex"] >= 0
    p = res["worldPosition"][hit].astype(F32)
    n = res["worldNormal"][hit].astype(F32)
    n = np.where((np.einsum("ij,ij->i", n, d[hit]) > 0)[:, None], -n, n).astype(F32)   # facing the camera ray
    # (b) cosine-weighted hemisphere about the shading normal
    u1, u2 = rng.random(len(p)), rng.random(len(p))
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    t = np.cross(n, np.where(np.abs(n[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]]))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    bd = (t * (r * np.cos(phi))[:, None] + b * (r * np.sin(phi))[:, None] + n * np.sqrt(1 - u1)[:, None]).astype(F32)
    # (c) shadow segments to a random point of a random emissive triangle
    em = hall.init_scene_emissive_triangles()
    pos = hall.world_vertices["position"]
    tri = hall.triangles[em[rng.integers(0, len(em), len(p))]]
    r1, r2 = rng.random(len(p)), rng.random(len(p))
    s = np.sqrt(r1)
    q = (1 - s)[:, None] * pos[tri["v0"]] + ((1 - r2) * s)[:, None] * pos[tri["v1"]] + (r2 * s)[:, None] * pos[tri["v2"]]
    v = q - p
    dist = np.linalg.norm(v, axis=1)
    return p, bd, (v / dist[:, None]).astype(F32), (0.999 * dist).astype(F32)


def hits_rate(ctx, name, o, d, tmax, ks, calls):
    """One ray set: the closest-hit query, then the multi-hit query per K, each warmed up and timed over `calls` calls."""
    rows = []

    def timed(fn):
        for _ in range(3):
            fn()
        ms = [fn().kernel_ms for _ in range(calls)]
        return statistics.median(ms), min(ms), max(ms)
    med0, lo0, hi0 = timed(lambda: ctx.trace_rays(o, d, 0.0, tmax, with_stats=True)[1])
    rows.append({"set": name, "scene": "hall_1M", "query": "closest", "rays": len(o), "ms_median": round(med0, 4), "ms_min": round(lo0, 4),
                 "ms_max": round(hi0, 4), "calls": calls, "mrays_per_s": round(len(o) / med0 / 1e3, 1)})
    for k in ks:
        med, lo, hi = timed(lambda: ctx.trace_ray_hits(o, d, 0.0, tmax, max_hits=k, with_stats=True)[2])
        counts = ctx.trace_ray_hits(o, d, 0.0, tmax, max_hits=k)[1]
        records = int(counts.sum())
        rows.append({"set": name, "scene": "hall_1M", "query": "hits", "max_hits": k, "rays": len(o), "ms_median": round(med, 4),
                     "ms_min": round(lo, 4), "ms_max": round(hi, 4), "calls": calls, "mrays_per_s": round(len(o) / med / 1e3, 1),
                     "records": records, "mhits_per_s": round(records / med / 1e3, 1), "records_per_ray": round(records / len(o), 3),
                     "ms_over_closest": round(med / med0, 3)})
    return rows


def main_hits(a):
    W, H = 1920, 1080
    rng = np.random.default_rng(2024)
    hall, cam = scenes.hall_scene(), scenes.hall_camera(W, H)
    ctx = capi.Context(0)
    ctx.upload_scene(hall)
    o, d = camera_rays(cam)
    p, bd, sd, smax = hall_ray_sets(hall, d, rng, ctx.trace_rays(o, d))
    rows = hits_rate(ctx, "a_camera", o, d, np.inf, a.hits, a.calls)
    rows += hits_rate(ctx, "b_bounce", p, bd, np.inf, a.hits, a.calls)
    rows += hits_rate(ctx, "c_shadow", p, sd, smax, a.hits, a.calls)
    ctx.close()
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    out = Path(a.out) if a.out else ROOT / "profiles" / "query" / "hits_rate.jsonl"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


def points_rate(ctx, name, p, ks, calls, med0):
    """One point set: the nearest-point query per K, warmed up and timed over `calls` calls, then one counted call."""
    rows = []
    for k in ks:
        for _ in range(3):
            ctx.nearest_points(p, max_hits=k)
        ms = [ctx.nearest_points(p, max_hits=k, with_stats=True)[2].kernel_ms for _ in range(calls)]
        ctx.set_ray_counting(True)
        st = ctx.nearest_points(p, max_hits=k, with_stats=True)[2]
        ctx.set_ray_counting(False)
        med = statistics.median(ms)
        rows.append({"set": name, "scene": "hall_1M", "query": "points", "max_hits": k, "points": len(p), "ms_median": round(med, 4),
                     "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": calls, "mpoints_per_s": round(len(p) / med / 1e3, 1),
                     "node_visits_per_point": round(st.node_visits / st.rays, 3), "box_tests_per_point": round(st.box_tests / st.rays, 3),
                     "tri_tests_per_point": round(st.tri_tests / st.rays, 3), "ms_over_closest": round(med / med0, 3)})
    return rows


def main_points(a):
    """Three sets of W x H points on the 1M hall: (a) the camera hits pushed 1 % of the scene diameter along the normal, (b) uniform in
    the scene box, (c) uniform in a box three diameters wide; the closest-hit query of the camera rays is timed in the same run."""
    W, H = 1920, 1080
    n = W * H
    rng = np.random.default_rng(2024)
    hall, cam = scenes.hall_scene(), scenes.hall_camera(W, H)
    ctx = capi.Context(0)
    ctx.upload_scene(hall)
    o, d = camera_rays(cam)
    for _ in range(3):
        ctx.trace_rays(o, d)
    ms0 = [ctx.trace_rays(o, d, with_stats=True)[1].kernel_ms for _ in range(a.calls)]
    med0 = statistics.median(ms0)
    rows = [{"set": "a_camera", "scene": "hall_1M", "query": "closest", "rays": n, "ms_median": round(med0, 4), "ms_min": round(min(ms0), 4),
             "ms_max": round(max(ms0), 4), "calls": a.calls, "mrays_per_s": round(n / med0 / 1e3, 1)}]
    res = ctx.trace_rays(o, d)
    pos = hall.world_vertices["position"].astype(np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    diam = float(np.linalg.norm(hi - lo))
    hit = res["objectIndex"] >= 0
    nrm = res["worldNormal"].astype(F32)
    nrm = np.where((np.einsum("ij,ij->i", nrm, d) > 0)[:, None], -nrm, nrm)
    near = np.where(hit[:, None], res["worldPosition"] + F32(0.01 * diam) * nrm, o + F32(0.5 * diam) * d).astype(F32)   # (a miss: a point half a diameter out)
    box = rng.uniform(lo, hi, size=(n, 3)).astype(F32)
    mid = (lo + hi) / 2
    wide = rng.uniform(mid - 1.5 * diam, mid + 1.5 * diam, size=(n, 3)).astype(F32)
    for name, p in (("a_near_surface", near), ("b_scene_box", box), ("c_wide_box", wide)):
        rows += points_rate(ctx, name, p, a.points, a.calls, med0)
    ctx.close()
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    out = Path(a.out) if a.out else ROOT / "profiles" / "query" / "points_rate.jsonl"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


def boxes_rate(ctx, name, lo, hi, ks, calls, med0):
    """One box set: the box-overlap query per K, warmed up and timed over `calls` calls, then one counted call."""
    rows = []
    for k in ks:
        for _ in range(3):
            ctx.overlap_boxes(lo, hi, max_hits=k)
        ms = [ctx.overlap_boxes(lo, hi, max_hits=k, with_stats=True)[3].kernel_ms for _ in range(calls)]
        ctx.set_ray_counting(True)
        _, counts, totals, st = ctx.overlap_boxes(lo, hi, max_hits=k, with_stats=True)
        ctx.set_ray_counting(False)
        med = statistics.median(ms)
        rows.append({"set": name, "scene": "hall_1M", "query": "boxes", "max_hits": k, "boxes": len(lo), "ms_median": round(med, 4),
                     "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": calls, "mboxes_per_s": round(len(lo) / med / 1e3, 1),
                     "node_visits_per_box": round(st.node_visits / st.rays, 3), "box_tests_per_box": round(st.box_tests / st.rays, 3),
                     "tri_tests_per_box": round(st.tri_tests / st.rays, 3), "accepted_per_box": round(float(totals.mean()), 3),
                     "records_per_box": round(float(counts.mean()), 3), "ms_over_closest": round(med / med0, 3)})
    return rows


def main_boxes(a):
    """Three sets of W x H boxes on the 1M hall, centred on the camera hits (a miss: half a diameter out along the ray), with half
    extents of 0.1 %, 0.5 % and 2 % of the scene diameter; the closest-hit query of the camera rays is timed in the same run."""
    W, H = 1920, 1080
    n = W * H
    hall, cam = scenes.hall_scene(), scenes.hall_camera(W, H)
    ctx = capi.Context(0)
    ctx.upload_scene(hall)
    if a.key15:
        ctx.set_tuning(15, a.key15)
    if a.mask_table:
        ctx.set_mesh_query_masks(np.full(len(hall.meshes), 0xFFFFFFFF, dtype=np.uint32))
    o, d = camera_rays(cam)
    for _ in range(3):
        ctx.trace_rays(o, d)
    ms0 = [ctx.trace_rays(o, d, with_stats=True)[1].kernel_ms for _ in range(a.calls)]
    med0 = statistics.median(ms0)
    rows = [{"set": "a_camera", "scene": "hall_1M", "query": "closest", "rays": n, "ms_median": round(med0, 4), "ms_min": round(min(ms0), 4),
             "ms_max": round(max(ms0), 4), "calls": a.calls, "mrays_per_s": round(n / med0 / 1e3, 1)}]
    res = ctx.trace_rays(o, d)
    pos = hall.world_vertices["position"].astype(np.float64)
    diam = float(np.linalg.norm(pos.max(axis=0) - pos.min(axis=0)))
    hit = res["objectIndex"] >= 0
    centre = np.where(hit[:, None], res["worldPosition"], o + F32(0.5 * diam) * d).astype(F32)
    for name, frac in (("a_small_0.1pct", 0.001), ("b_medium_0.5pct", 0.005), ("c_large_2pct", 0.02)):
        h = F32(frac * diam)
        rows += boxes_rate(ctx, name, (centre - h).astype(F32), (centre + h).astype(F32), a.boxes, a.calls, med0)
    ctx.close()
    lines = [json.dumps({**r, "key15": a.key15, "mask_table": a.mask_table}) for r in rows]
    print("\n".join(lines), flush=True)
    out = Path(a.out) if a.out else ROOT / "profiles" / "query" / "boxes_rate.jsonl"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


def main_triangles(a):
    """The triangles of the hall's largest mesh under three offsets against the hall, and the box query on their bounding boxes."""
    hall = scenes.hall_scene()
    ctx = capi.Context(0)
    ctx.upload_scene(hall)
    if a.key15:
        ctx.set_tuning(15, a.key15)
    if a.mask_table:
        ctx.set_mesh_query_masks(np.full(len(hall.meshes), 0xFFFFFFFF, dtype=np.uint32))
    mesh = int(np.argmax([m[1] for m in hall.meshes]))
    first, count = int(hall.meshes[mesh][0]), min(int(hall.meshes[mesh][1]), 1 << 18)
    t = hall.triangles[first:first + count]
    pos = hall.world_vertices["position"]
    q = np.stack([pos[t["v0"]], pos[t["v1"]], pos[t["v2"]]], axis=1).astype(F32)
    allpos = pos.astype(np.float64)
    diam = float(np.linalg.norm(allpos.max(axis=0) - allpos.min(axis=0)))
    size = q.reshape(-1, 3).max(axis=0).astype(np.float64) - q.reshape(-1, 3).min(axis=0).astype(np.float64)
    half = np.zeros(3)
    half[int(np.argmax(size))] = 0.5 * size.max()
    rows = []
    for name, shift in (("a_in_place", np.zeros(3)), ("b_half_size", half), ("c_clear", np.array([0.0, 2.0 * diam, 0.0]))):
        qs = (q + shift.astype(F32)).astype(F32)
        lo, hi = qs.min(axis=1), qs.max(axis=1)
        for k in a.triangles:
            for _ in range(3):
                ctx.overlap_triangles(qs, max_hits=k)
                ctx.overlap_boxes(lo, hi, max_hits=k)
            ms = [ctx.overlap_triangles(qs, max_hits=k, with_stats=True)[3].kernel_ms for _ in range(a.calls)]
            msb = [ctx.overlap_boxes(lo, hi, max_hits=k, with_stats=True)[3].kernel_ms for _ in range(a.calls)]
            ctx.set_ray_counting(True)
            _, counts, totals, st = ctx.overlap_triangles(qs, max_hits=k, with_stats=True)
            _, _, btotals, sb = ctx.overlap_boxes(lo, hi, max_hits=k, with_stats=True)
            ctx.set_ray_counting(False)
            med, medb = statistics.median(ms), statistics.median(msb)
            rows.append({"set": name, "scene": "hall_1M", "query": "triangles", "mesh": mesh, "max_hits": k, "triangles": len(qs),
                         "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "calls": a.calls,
                         "mtriangles_per_s": round(len(qs) / med / 1e3, 1), "node_visits_per_query": round(st.node_visits / st.rays, 3),
                         "box_tests_per_query": round(st.box_tests / st.rays, 3), "tri_tests_per_query": round(st.tri_tests / st.rays, 3),
                         "accepted_per_query": round(float(totals.mean()), 3), "records_per_query": round(float(counts.mean()), 3),
                         "boxes_ms_median": round(medb, 4), "boxes_ms_min": round(min(msb), 4), "boxes_ms_max": round(max(msb), 4),
                         "boxes_tri_tests_per_query": round(sb.tri_tests / sb.rays, 3), "boxes_accepted_per_query": round(float(btotals.mean()), 3),
                         "ms_over_boxes": round(med / medb, 3)})
    ctx.close()
    lines = [json.dumps({**r, "key15": a.key15, "mask_table": a.mask_table}) for r in rows]
    print("\n".join(lines), flush=True)
    out = Path(a.out) if a.out else ROOT / "profiles" / "query" / "triangles_rate.jsonl"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


def main_triangles_summary(a):
    rows = [json.loads(l) for f in a.triangles_summary for l in Path(f).read_text().splitlines() if l.strip()]
    keys = sorted({(r["key15"], r["mask_table"], r["set"], r["max_hits"]) for r in rows})
    out = []
    for key15, mask, name, k in keys:
        rs = [r for r in rows if (r["key15"], r["mask_table"], r["set"], r["max_hits"]) == (key15, mask, name, k)]
        t, b = [r["ms_median"] for r in rs], [r["boxes_ms_median"] for r in rs]
        mt, mb = statistics.median(t), statistics.median(b)
        out.append({"set": name, "key15": key15, "mask_table": mask, "max_hits": k, "processes": len(rs), "triangles": rs[0]["triangles"],
                    "ms_median_of_medians": round(mt, 4), "ms_runs": t, "boxes_ms_median_of_medians": round(mb, 4), "boxes_ms_runs": b,
                    "ms_over_boxes": round(mt / mb, 3), "tri_tests_per_query": rs[0]["tri_tests_per_query"],
                    "node_visits_per_query": rs[0]["node_visits_per_query"], "accepted_per_query": rs[0]["accepted_per_query"],
                    "boxes_accepted_per_query": rs[0]["boxes_accepted_per_query"]})
    dest = Path(a.out) if a.out else ROOT / "profiles" / "query" / "triangles_rate_summary.jsonl"
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text("\n".join(json.dumps(r) for r in out) + "\n")
    print("| key 15 | mask table | set | K = 1 | K = 8 | K = 32 |\n|---|---|---|---|---|---|")
    for key15, mask, name in sorted({k[:3] for k in keys}):
        cells = []
        for k in (1, 8, 32):
            r = [x for x in out if (x["key15"], x["mask_table"], x["set"], x["max_hits"]) == (key15, mask, name, k)]
            cells.append(f"{r[0]['ms_median_of_medians']:.3f} / {r[0]['boxes_ms_median_of_medians']:.3f} ({r[0]['ms_over_boxes']:.2f})" if r else "-")
        print(f"| {key15} | {'yes' if mask else 'no'} | {name} | " + " | ".join(cells) + " |")


def filter_rows(plain, filt, case, families, calls):
    """The families of one case on both contexts: `families` maps a name to (records, call(ctx, with_stats) -> FrameStats)."""
    rows = []
    for name, (n, call) in families.items():
        for _ in range(3):
            call(plain), call(filt)
        ms = {"unfiltered": [], "filtered": []}
        for _ in range(calls):                                        # alternating: both see the same neighbours on the machine
            ms["unfiltered"].append(call(plain).kernel_ms)
            ms["filtered"].append(call(filt).kernel_ms)
        row = {"case": case, "scene": "hall_1M", "query": name, "records": n, "calls": calls}
        for which, ctx in (("unfiltered", plain), ("filtered", filt)):
            ctx.set_ray_counting(True)
            st = call(ctx)
            ctx.set_ray_counting(False)
            row.update({f"ms_median_{which}": round(statistics.median(ms[which]), 4), f"ms_min_{which}": round(min(ms[which]), 4),
                        f"ms_max_{which}": round(max(ms[which]), 4), f"node_visits_per_record_{which}": round(st.node_visits / st.rays, 3),
                        f"tri_tests_per_record_{which}": round(st.tri_tests / st.rays, 3), f"hit_fraction_{which}": round(st.hits / st.rays, 4)})
        row["filtered_over_unfiltered"] = round(row["ms_median_filtered"] / row["ms_median_unfiltered"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main_filter(a):
    W, H = 1920, 1080
    rng = np.random.default_rng(2024)
    hall, cam = scenes.hall_scene(), scenes.hall_camera(W, H)
    plain, filt = capi.Context(0), capi.Context(0)
    plain.upload_scene(hall)
    filt.upload_scene(hall)
    o, d = camera_rays(cam)
    res = plain.trace_rays(o, d)
    pos = hall.world_vertices["position"].astype(np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    diam = float(np.linalg.norm(hi - lo))
    hit = res["objectIndex"] >= 0
    centre = np.where(hit[:, None], res["worldPosition"], o + F32(0.5 * diam) * d).astype(F32)
    h = F32(0.005 * diam)
    blo, bhi = (centre - h).astype(F32), (centre + h).astype(F32)
    # the column the camera sees most of: meshes 12 .. 75 are the columns (scenes.hall_scene)
    first = np.array([m[0] for m in hall.meshes])
    mesh_of_hit = np.searchsorted(first, res["objectIndex"][hit], side="right") - 1
    seen = np.bincount(mesh_of_hit, minlength=len(hall.meshes))[12:76]
    column = 12 + int(seen.argmax())
    t0, nt = hall.meshes[column][0], hall.meshes[column][1]
    # points on the column's own surface: uniform barycentrics on its triangles, drawn with replacement
    tri = hall.triangles[t0 + rng.integers(0, nt, 1 << 18)]
    r1, r2 = rng.random(len(tri)), rng.random(len(tri))
    sq = np.sqrt(r1)
    wp = hall.world_vertices["position"]
    on_column = ((1 - sq)[:, None] * wp[tri["v0"]] + ((1 - r2) * sq)[:, None] * wp[tri["v1"]] + (r2 * sq)[:, None] * wp[tri["v2"]]).astype(F32)
    whole = 64
    wlo, whi = np.tile((lo - 1).astype(F32), (whole, 1)), np.tile((hi + 1).astype(F32), (whole, 1))

    def families(points, k_points, boxes):
        return {"closest": (len(o), lambda c: c.trace_rays(o, d, with_stats=True)[1]),
                "hits_k4": (len(o), lambda c: c.trace_ray_hits(o, d, max_hits=4, with_stats=True)[2]),
                f"points_k{k_points}": (len(points), lambda c: c.nearest_points(points, max_hits=k_points, with_stats=True)[2]),
                "boxes_k8": (len(boxes[0]), lambda c: c.overlap_boxes(boxes[0], boxes[1], max_hits=8, with_stats=True)[3])}
    nM = len(hall.meshes)
    rows = []
    filt.set_mesh_query_masks(np.full(nM, 0xFFFFFFFF, dtype=np.uint32))
    rows += filter_rows(plain, filt, "1_all_ones", families(centre, 4, (blo, bhi)), a.calls)
    M = np.ones(nM, dtype=np.uint32)
    M[column] = 0
    filt.set_mesh_query_masks(M)
    rows += filter_rows(plain, filt, "2_column_excluded", families(on_column, 1, (blo, bhi)), a.calls)
    M = np.zeros(nM, dtype=np.uint32)
    M[column] = 1
    filt.set_mesh_query_masks(M)
    rows += filter_rows(plain, filt, "3_column_alone", families(centre, 1, (wlo, whi)), a.calls)
    for r in rows:
        r["column_mesh"], r["column_triangles"], r["filter_builds"] = column, int(nt), int(filt.query_filter()[2])
    plain.close()
    filt.close()
    lines = [json.dumps(r) for r in rows]
    out = Path(a.out) if a.out else ROOT / "profiles" / "query" / "filter_rate.jsonl"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hits", type=int, nargs="+", default=None, metavar="K", help="time the multi-hit query at these max_hits instead")
    ap.add_argument("--points", type=int, nargs="+", default=None, metavar="K", help="time the nearest-point query at these max_hits instead")
    ap.add_argument("--boxes", type=int, nargs="+", default=None, metavar="K", help="time the box-overlap query at these max_hits instead")
    ap.add_argument("--triangles", type=int, nargs="+", default=None, metavar="K", help="time the triangle-overlap query at these max_hits instead")
    ap.add_argument("--triangles-summary", nargs="+", default=None, metavar="FILE", help="fold the files of several --triangles processes into one summary (no GPU)")
    ap.add_argument("--key15", type=int, default=0, metavar="V", help="with --boxes / --triangles: tuning key 15 (0: the library's choice)")
    ap.add_argument("--mask-table", action="store_true", help="with --boxes / --triangles: a mesh mask table of all ones, so that the filtered kernels run")
    ap.add_argument("--filter", action="store_true", help="time the four families with and without a query filter instead")
    a = ap.parse_args()
    if a.boxes and not all(1 <= k <= capi.OVERLAP_MAX_HITS for k in a.boxes):
        raise SystemExit(f"--boxes takes values in 1..{capi.OVERLAP_MAX_HITS}")
    if a.triangles and not all(1 <= k <= capi.OVERLAP_MAX_HITS for k in a.triangles):
        raise SystemExit(f"--triangles takes values in 1..{capi.OVERLAP_MAX_HITS}")
    if a.hits and not all(1 <= k <= capi.QUERY_MAX_HITS for k in a.hits):
        raise SystemExit(f"--hits takes values in 1..{capi.QUERY_MAX_HITS}")
    if a.points and not all(1 <= k <= capi.QUERY_MAX_HITS for k in a.points):
        raise SystemExit(f"--points takes values in 1..{capi.QUERY_MAX_HITS}")
    if a.triangles_summary:
        return main_triangles_summary(a)
    if not torch.cuda.is_available():
        raise SystemExit("query_rate.py needs an MI355X")
    torch.cuda.set_device(0)
    if a.filter:
        return main_filter(a)
    if a.hits:
        return main_hits(a)
    if a.points:
        return main_points(a)
    if a.boxes:
        return main_boxes(a)
    if a.triangles:
        return main_triangles(a)
    W, H = 1920, 1080
    rows = []
    rng = np.random.default_rng(2024)
    hall, cam = scenes.hall_scene(), scenes.hall_camera(W, H)
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(hall)
    ctx.set_camera(cam)
    o, d = camera_rays(cam)
    ra, res = rate(ctx, "a_camera", "hall_1M", o, d, a.calls)
    rows.append(ra)
    p, bd, sd, smax = hall_ray_sets(hall, d, rng, res)
    rows.append(rate(ctx, "b_bounce", "hall_1M", p, bd, a.calls)[0])
    rows.append(rate(ctx, "c_shadow", "hall_1M", p, sd, a.calls, tmax=smax, occluded=True)[0])
    p1 = part1_ms(ctx, a.calls)
    rows.append({"set": "restir_di_part1", "scene": "hall_1M", "rays": W * H, "ms_median": round(p1[0], 4), "ms_min": round(p1[1], 4),
                 "ms_max": round(p1[2], 4), "calls": a.calls, "camera_query_over_part1": round(ra["ms_median"] / p1[0], 3),
                 "timing": "torch events on the context stream", "camera_query_ms_same_timing": round(query_ms_torch_events(ctx, o, d, a.calls), 4)})
    ctx.close()
    # (d) the camera rays of (a) on hall_small (one thread per ray under the default tuning key 15)
    small = capi.Context(0)
    small.upload_scene(scenes.hall_scene_small())
    rows.append(rate(small, "d_camera_small", "hall_small", o, d, a.calls)[0])
    small.close()
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
