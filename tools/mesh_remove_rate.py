#!/usr/bin/env python3
"""What a mesh removal costs on the 1M-triangle hall, and what the pruned tree costs afterwards: fyprt_remove_meshes next to
fyprt_upload_scene of the same reduced scene (the only way a host had before), in the same process, with the host builder (tuning key
12 = 0) and the device PLOC builder (2).  Cases: one column, one drape, one light mesh, and a 100 000-triangle sheet imported first
(fyprt_append_meshes) and then removed.  Per case:
  * wall time of the removal (context A, which holds the hall) and of the upload of the reduced scene (context B); both calls block
    until the device is done.  A removal on a small scene runs first, so that the kernels' code objects are loaded;
  * ReSTIR DI frame time (median wall time of blocking frames) and node visits per ray (one counted frame) on A's pruned tree and on
    B's freshly built one, same camera, same settings.
  Every case is set up and timed `repeats` times from scratch (a removal cannot be undone); the wall times are the medians, with all
  samples beside them, and the frame figures are the last repeat's.
  usage: mesh_remove_rate.py [--frames 9] [--repeats 3] [--width 1280 --height 720] [--small] [--out profiles/mesh_remove/remove_rate.jsonl]
  (--small: the 13k-triangle hall, to try the tool itself)"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from fypraytracer_amd import capi, scenes  # noqa: E402
from mesh_import_rate import frames, sheet_mesh  # noqa: E402


def one_case(args, mk, cam, centre, st, key12, name, mesh_index, t_removes, t_uploads):
    W, H = args.width, args.height
    sc = mk()
    a, b = capi.Context(0), capi.Context(0)
    for c in (a, b):
        c.set_tuning(12, key12)
        c.resize(W, H)
        c.set_camera(cam)
    a.upload_scene(sc)
    if mesh_index is None:
        mesh_index = sc.add_new_mesh_to_scene(*sheet_mesh(2_000 if args.small else 100_000, 4.0), pos=tuple(float(v) for v in centre), rotation=(0, 90, 0), material_index=0)
        a.append_meshes(sc, mesh_index)
    before, removed = len(sc.triangles), int(sc.meshes[mesh_index][1])
    nodes_before = len(a.export_bvh()["nodes"])
    rec = sc.remove_meshes_from_scene([mesh_index])
    t = time.perf_counter(); a.remove_meshes(rec); t_remove = time.perf_counter() - t
    t = time.perf_counter(); b.upload_scene(sc); t_upload = time.perf_counter() - t
    ta, tb = a.export_bvh(), b.export_bvh()
    fa, va = frames(a, st, args.frames)
    fb, vb = frames(b, st, args.frames)
    t_removes.append(t_remove * 1e3)
    t_uploads.append(t_upload * 1e3)
    a.close()
    b.close()
    return {"scene": "hall_small" if args.small else "hall", "removed": name, "builder_key12": key12, "triangles_before": before, "triangles_removed": removed,
            "frame": f"ReSTIR DI {W}x{H}", "frame_ms_after_remove": round(fa, 3), "frame_ms_after_upload": round(fb, 3),
            "node_visits_per_ray_after_remove": round(va, 2), "node_visits_per_ray_after_upload": round(vb, 2),
            "levels_after_remove": int(ta["max_stack"]), "levels_after_upload": int(tb["max_stack"]),
            "nodes_before": int(nodes_before), "nodes_after_remove": int(len(ta["nodes"])), "nodes_after_upload": int(len(tb["nodes"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cam = scenes.hall_camera(args.width, args.height)
    centre = np.asarray(cam.position, np.float64) + 8.0 * np.asarray(cam.forward, np.float64)
    mk = scenes.hall_scene_small if args.small else scenes.hall_scene
    probe = mk()
    n_col = sum(1 for _, c, _ in probe.meshes if c == probe.meshes[12][1])                    # 12 wall quads, then the columns, the drapes, the light meshes
    n_light = sum(1 for _, _, mi in probe.meshes if mi >= 12)
    cases = {"column": 12 + n_col // 2, "drape": 12 + n_col + 1, "light_mesh": len(probe.meshes) - n_light + 1, "sheet_100k": None}
    del probe
    st = capi.Settings(technique=capi.RESTIR_DI, use_temporal_reuse=1, use_spatial_reuse=1, sky_color=(0.1, 0.2, 0.3))
    warm_sc = scenes.cornell_box()
    warm = capi.Context(0)
    warm.upload_scene(warm_sc)
    warm.remove_meshes(warm_sc.remove_meshes_from_scene([5]))
    warm.close()
    lines = []
    for key12 in (0, 2):
        for name, case_index in cases.items():
            t_removes, t_uploads = [], []
            for _ in range(args.repeats):
                out = one_case(args, mk, cam, centre, st, key12, name, case_index, t_removes, t_uploads)
            out["remove_meshes_wall_ms"], out["upload_scene_wall_ms"] = round(float(np.median(t_removes)), 2), round(float(np.median(t_uploads)), 1)
            out["upload_over_remove"] = round(float(np.median(t_uploads)) / float(np.median(t_removes)), 1)
            out["remove_meshes_wall_ms_samples"], out["upload_scene_wall_ms_samples"] = [round(v, 2) for v in t_removes], [round(v, 1) for v in t_uploads]
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
