#!/usr/bin/env python3
"""What a mesh import costs on the 1M-triangle hall, and what the grafted tree costs afterwards: fyprt_append_meshes next to
fyprt_upload_scene of the same combined scene, in the same process, for a banana-sized import (the banana fixture's mesh) and a
100 000-triangle sheet, with the host builder (tuning key 12 = 0) and the device PLOC builder (2).  Per case:
  * wall time of the append (context A, which holds the hall) and of the upload of the combined scene (context B);
  * ReSTIR DI frame time (median wall time of blocking frames) and node visits per ray (one counted frame) on A's grafted tree and on
    B's freshly built one, same camera, same settings.
With --sequence K: K small imports scattered over the hall, one after the other, for every placement mode of --placement
(fyprt_set_append_placement: 0 at the root, 1 at the cheapest place by surface-area cost).  Per import: wall time of the append, where it
went, the tree's levels, node visits per ray and ReSTIR DI frame time; at the end the same for a fresh upload of the combined scene.
  usage: mesh_import_rate.py [--frames 9] [--width 1280 --height 720] [--out profiles/mesh_import/import_rate.jsonl]
         mesh_import_rate.py --sequence 30 --placement 0 1 [--import-triangles 2000] [--builder 0] [--out profiles/mesh_import/placement_rate.jsonl]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402


def banana_mesh():
    sc = scenes.banana_scene()
    tr = sc.mesh_transforms[0]
    a, n = tr["vertex_start"], tr["vertex_count"]
    first, count, _ = sc.meshes[0]
    t = sc.triangles[first:first + count]
    idx = np.stack([t["v0"], t["v1"], t["v2"]], -1).astype(np.uint32) - np.uint32(a)
    v = sc.vertices[a:a + n]
    return v["position"].copy(), v["normal"].copy(), v["uv"].copy(), idx


def sheet_mesh(triangles, size):
    n = int(np.ceil(np.sqrt(triangles / 2)))
    g = np.arange(n + 1, dtype=np.float32) / np.float32(n) - np.float32(0.5)
    x, y = np.meshgrid(g * np.float32(size), g * np.float32(size))
    pos = np.stack([x, y, np.float32(0.03 * size) * np.sin(9.0 * x / size + 5.0 * y / size)], -1).reshape(-1, 3).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (len(pos), 1))
    uv = np.stack([x / np.float32(size) + 0.5, y / np.float32(size) + 0.5], -1).reshape(-1, 2).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    a = (j * (n + 1) + i).reshape(-1)
    idx = np.concatenate([np.stack([a, a + 1, a + n + 2], -1), np.stack([a, a + n + 2, a + n + 1], -1)]).astype(np.uint32)
    return pos, nrm, uv, idx[:triangles]


def frames(ctx, st, n):
    ms = []
    for f in range(n + 2):                                   # two to warm up
        st.rand_seed = f + 1
        t = time.perf_counter()
        ctx.render(st)
        if f >= 2:
            ms.append((time.perf_counter() - t) * 1e3)
    ctx.set_ray_counting(True)
    stats = ctx.render(st)
    ctx.set_ray_counting(False)
    return float(np.median(ms)), stats.node_visits / max(1, stats.rays)


def sequence(args, st, cam):
    """K imports scattered over the hall, per placement mode; then a fresh upload of the combined scene."""
    W, H = args.width, args.height
    rng = np.random.default_rng(11)
    lo, hi = np.array([-18.0, 1.0, -8.0]), np.array([18.0, 13.0, 8.0])       # inside the hall's walls
    centres = rng.uniform(lo, hi, size=(args.sequence, 3))
    turns = rng.uniform(0.0, 180.0, size=(args.sequence, 3))
    mesh = sheet_mesh(args.import_triangles, 1.5)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    sc = None
    for mode in args.placement:
        sc = scenes.hall_scene()
        ctx = capi.Context(0)
        ctx.set_tuning(12, args.builder)
        ctx.resize(W, H)
        ctx.set_camera(cam)
        ctx.upload_scene(sc)
        placed = hasattr(ctx.lib, "fyprt_set_append_placement")           # (an older build loaded through FYPRT_LIB for an A/B run has mode 0 only)
        if placed:
            ctx.set_append_placement(mode)
        elif mode != 0:
            raise SystemExit("this library has no placement modes")
        for k in range(args.sequence):
            m = sc.add_new_mesh_to_scene(*mesh, pos=tuple(float(v) for v in centres[k]), rotation=tuple(float(v) for v in turns[k]), material_index=0)
            t = time.perf_counter(); ctx.append_meshes(sc, m); t_append = time.perf_counter() - t
            pl = ctx.last_append_placement() if placed else None
            ms, visits = frames(ctx, st, args.frames)
            emit({"scene": "hall", "sequence": args.sequence, "placement": mode, "library": args.label, "builder_key12": args.builder, "import": k + 1,
                  "triangles_imported": int(sc.meshes[m][1]), "append_meshes_wall_ms": round(t_append * 1e3, 2),
                  "kind": int(pl.kind) if pl else None, "depth": int(pl.depth) if pl else None, "candidates": int(pl.candidates) if pl else None,
                  "levels_after": int(ctx.export_bvh()["max_stack"]), "frame": f"ReSTIR DI {W}x{H}", "frame_ms": round(ms, 3), "node_visits_per_ray": round(visits, 2)})
        ctx.close()
    fresh = capi.Context(0)
    fresh.set_tuning(12, args.builder)
    fresh.resize(W, H)
    fresh.set_camera(cam)
    t = time.perf_counter(); fresh.upload_scene(sc); t_upload = time.perf_counter() - t
    ms, visits = frames(fresh, st, args.frames)
    emit({"scene": "hall", "sequence": args.sequence, "placement": "fresh upload", "library": args.label, "builder_key12": args.builder, "import": args.sequence, "upload_scene_wall_ms": round(t_upload * 1e3, 1),
          "levels_after": int(fresh.export_bvh()["max_stack"]), "frame": f"ReSTIR DI {W}x{H}", "frame_ms": round(ms, 3), "node_visits_per_ray": round(visits, 2)})
    fresh.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sequence", type=int, default=0, help="K scattered imports instead of the two single imports")
    ap.add_argument("--placement", type=int, nargs="+", choices=(0, 1), default=[0], help="placement modes of the sequence")
    ap.add_argument("--import-triangles", type=int, default=2000)
    ap.add_argument("--builder", type=int, choices=(0, 1, 2), default=0, help="tuning key 12 of the sequence")
    ap.add_argument("--label", default="this commit", help="what the sequence's records call the library (an A/B run through FYPRT_LIB)")
    args = ap.parse_args()
    W, H = args.width, args.height
    cam = scenes.hall_camera(W, H)
    if args.sequence:
        lines = sequence(args, capi.Settings(technique=capi.RESTIR_DI, use_temporal_reuse=1, use_spatial_reuse=1, sky_color=(0.1, 0.2, 0.3)), cam)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as f:                     # appended: an A/B run adds its records to the same file
                f.write("\n".join(lines) + "\n")
        return
    centre = np.asarray(cam.position, np.float64) + 8.0 * np.asarray(cam.forward, np.float64)
    imports = {"banana": (banana_mesh(), dict(rotation=(90, 0, 0), scale_=(1, 1, 1))), "sheet_100k": (sheet_mesh(100_000, 4.0), dict(rotation=(0, 90, 0), scale_=(1, 1, 1)))}
    st = capi.Settings(technique=capi.RESTIR_DI, use_temporal_reuse=1, use_spatial_reuse=1, sky_color=(0.1, 0.2, 0.3))
    lines = []
    for key12 in (0, 2):
        for name, (mesh, place) in imports.items():
            sc = scenes.hall_scene()
            a, b = capi.Context(0), capi.Context(0)
            for c in (a, b):
                c.set_tuning(12, key12)
                c.resize(W, H)
                c.set_camera(cam)
            a.upload_scene(sc)
            m = sc.add_new_mesh_to_scene(*mesh, pos=tuple(float(v) for v in centre), material_index=0, **place)
            t = time.perf_counter(); a.append_meshes(sc, m); t_append = time.perf_counter() - t
            t = time.perf_counter(); b.upload_scene(sc); t_upload = time.perf_counter() - t
            ta, tb = a.export_bvh(), b.export_bvh()
            fa, va = frames(a, st, args.frames)
            fb, vb = frames(b, st, args.frames)
            rec = {"scene": "hall", "import": name, "builder_key12": key12, "triangles_before": int(sc.meshes[m][0]), "triangles_imported": int(sc.meshes[m][1]),
                   "append_meshes_wall_ms": round(t_append * 1e3, 2), "upload_scene_wall_ms": round(t_upload * 1e3, 1), "upload_over_append": round(t_upload / t_append, 1),
                   "frame": f"ReSTIR DI {W}x{H}", "frame_ms_after_append": round(fa, 3), "frame_ms_after_upload": round(fb, 3),
                   "node_visits_per_ray_after_append": round(va, 2), "node_visits_per_ray_after_upload": round(vb, 2),
                   "levels_after_append": int(ta["max_stack"]), "levels_after_upload": int(tb["max_stack"]), "nodes_after_append": int(len(ta["nodes"])), "nodes_after_upload": int(len(tb["nodes"]))}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            a.close()
            b.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
