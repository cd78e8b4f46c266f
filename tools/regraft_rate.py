#!/usr/bin/env python3
"""What a regraft costs on the 1M-triangle hall, and what it buys: one column, one drape and one light mesh are each moved by several
scene diameters with fyprt_update_transforms (which refits boxes only), then fyprt_regraft_meshes puts the mesh where it lies now.  Next to
it fyprt_upload_scene of the same moved scene, the only repair a host had before, with the host builder (tuning key 12 = 0) and the device
PLOC builder (2).  Per case:
  * wall time of regraft_meshes (context A, which holds the hall) and of the upload of the moved scene (context B); both calls block
    until the device is done.  Each is repeated `repeats` times on the same contexts — a regraft of a mesh that was just regrafted prunes
    and grafts the same records again — and the medians are reported with all samples beside them.  A regraft on a small scene runs
    first, so that the kernels' code objects are loaded;
  * fyprt_tree_cost, the ReSTIR DI frame time (median wall time of blocking frames) and node visits per ray (one counted frame) on three
    trees: A's refit-only tree, A's regrafted tree and B's freshly built one; same camera, same settings.
  usage: regraft_rate.py [--frames 9] [--repeats 5] [--diameters 3] [--placement 1] [--width 1280 --height 720] [--small]
                         [--out profiles/regraft/regraft_rate.jsonl]
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
from mesh_import_rate import frames  # noqa: E402


def cost_fields(c, tag):
    sah = (c.inner_area + c.leaf_area) / c.root_area if c.root_area > 0 else 0.0
    return {f"sah_{tag}": round(sah, 3), f"inner_area_{tag}": round(c.inner_area, 1), f"leaf_area_{tag}": round(c.leaf_area, 1),
            f"nodes_{tag}": int(c.nodes), f"levels_{tag}": int(c.levels)}


def one_case(args, mk, cam, st, key12, name, mesh_index):
    W, H = args.width, args.height
    sc = mk()
    a, b = capi.Context(0), capi.Context(0)
    for c in (a, b):
        c.set_tuning(12, key12)
        c.resize(W, H)
        c.set_camera(cam)
    a.set_append_placement(args.placement)
    a.upload_scene(sc)
    a.set_object_vertices(sc)
    pos = sc.world_vertices["position"]
    diameter = float(np.linalg.norm(pos.max(axis=0).astype(np.float64) - pos.min(axis=0).astype(np.float64)))
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    p = sc.mesh_transforms[mesh_index]["pos"]
    mgr.set_mesh_transform(sc, mesh_index, pos=(float(p[0]) + args.diameters * diameter, float(p[1]), float(p[2])))
    mgr.perform_all_scene_updates(sc)
    a.update_transforms(sc, [mesh_index])
    out = {"scene": "hall_small" if args.small else "hall", "moved": name, "builder_key12": key12, "placement_mode": args.placement,
           "triangles": len(sc.triangles), "triangles_moved": int(sc.meshes[mesh_index][1]), "moved_by_scene_diameters": args.diameters,
           "frame": f"ReSTIR DI {W}x{H}"}
    out.update(cost_fields(a.tree_cost(), "refit_only"))
    f, v = frames(a, st, args.frames)
    out["frame_ms_refit_only"], out["node_visits_per_ray_refit_only"] = round(f, 3), round(v, 2)
    t_regraft, t_upload = [], []
    for _ in range(args.repeats):
        t = time.perf_counter(); report, = a.regraft_meshes([mesh_index]); t_regraft.append((time.perf_counter() - t) * 1e3)
    out["placement_kind"], out["placement_depth"] = int(report.kind), int(report.depth)
    out.update(cost_fields(a.tree_cost(), "regrafted"))
    f, v = frames(a, st, args.frames)
    out["frame_ms_regrafted"], out["node_visits_per_ray_regrafted"] = round(f, 3), round(v, 2)
    for _ in range(args.repeats):
        t = time.perf_counter(); b.upload_scene(sc); t_upload.append((time.perf_counter() - t) * 1e3)
    out.update(cost_fields(b.tree_cost(), "upload"))
    f, v = frames(b, st, args.frames)
    out["frame_ms_upload"], out["node_visits_per_ray_upload"] = round(f, 3), round(v, 2)
    out["regraft_meshes_wall_ms"], out["upload_scene_wall_ms"] = round(float(np.median(t_regraft)), 2), round(float(np.median(t_upload)), 1)
    out["upload_over_regraft"] = round(float(np.median(t_upload)) / float(np.median(t_regraft)), 1)
    out["regraft_meshes_wall_ms_samples"], out["upload_scene_wall_ms_samples"] = [round(x, 2) for x in t_regraft], [round(x, 1) for x in t_upload]
    a.close()
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--diameters", type=float, default=3.0)
    ap.add_argument("--placement", type=int, default=1)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cam = scenes.hall_camera(args.width, args.height)
    mk = scenes.hall_scene_small if args.small else scenes.hall_scene
    probe = mk()
    n_col = sum(1 for _, c, _ in probe.meshes if c == probe.meshes[12][1])                    # 12 wall quads, then the columns, the drapes, the light meshes
    n_light = sum(1 for _, _, mi in probe.meshes if mi >= 12)
    cases = {"column": 12 + n_col // 2, "drape": 12 + n_col + 1, "light_mesh": len(probe.meshes) - n_light + 1}
    del probe
    st = capi.Settings(technique=capi.RESTIR_DI, use_temporal_reuse=1, use_spatial_reuse=1, sky_color=(0.1, 0.2, 0.3))
    warm_sc = scenes.cornell_box()
    warm = capi.Context(0)
    warm.set_append_placement(args.placement)
    warm.upload_scene(warm_sc)
    warm.regraft_meshes([5])
    warm.tree_cost()
    warm.close()
    lines = []
    for key12 in (0, 2):
        for name, mesh_index in cases.items():
            lines.append(json.dumps(one_case(args, mk, cam, st, key12, name, mesh_index)))
            print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
