#!/usr/bin/env python3
"""Cost of object motion in the temporal denoiser (fyprt_denoise_temporal_set_motion) on the bench workload, GPU.
The bench hall (1M triangles) at 1920x1080, ReSTIR DI with bench.py's settings and to_accumulate = 0, defaults of the denoiser.  Contexts in
one process, visited in turn within every repetition (a frame, then a temporal call; the moving ones apply their edit before the frame):
  parent        the parent commit's library (--lib-parent), if given: its steady-state call — the yardstick
  off           mode off
  on            mode on, never edited: no snapshot, the plain reprojection kernel
  column        mode on, the most visible column moved by update_transforms before every frame
  all           mode on, every mesh moved before every frame: every wave rebuilds its hits
  off + column  mode off, the same column edit — its update_transforms is the edit without the snapshot copy (its calls are first calls)
Times: hipEvent times of the calls' kernels (FrameStats of the host entry; the reproject part includes the moved-flag kernel), medians
over --reps after warm-up, with the spread (min, max) of the same repetitions; update_transforms by the host's clock around the blocking
call.  One JSON line per context.
  usage: python tools/temporal_motion_rate.py [--reps 20] [--lib-parent PATH] [--out profiles/temporal/motion_rate.jsonl]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402
from fypraytracer_amd.scene import mesh_matrix  # noqa: E402
from tools.temporal_rate import bench_settings  # noqa: E402


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--lib-parent", default=None, help="the parent commit's libfyprt.so: its steady-state call is timed beside")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "temporal" / "motion_rate.jsonl"))
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    lib = capi.load_library()
    plan = [("off", lib, False, None), ("on", lib, True, None), ("column", lib, True, "column"), ("all", lib, True, "all"),
            ("off + column", lib, False, "column")]
    if a.lib_parent:
        plan.insert(0, ("parent", capi.load_library(a.lib_parent), False, None))
    st = bench_settings()
    tp = capi.TemporalParams()
    runs = []
    column = None
    sc = scenes.hall_scene()           # one host scene for all, never edited: a context's edit is the matrices it hands to the device
    sc.manager().perform_all_scene_updates(sc)
    base = [dict(t) for t in sc.mesh_transforms]
    for label, l, motion, edit in plan:
        ctx = capi.Context(0, lib=l)
        ctx.resize(W, H)
        ctx.upload_scene(sc)
        ctx.set_camera(scenes.hall_camera(W, H))
        if edit:
            ctx.set_object_vertices(sc)
        if motion:
            ctx.denoise_temporal_set_motion(True)
        if column is None and label != "parent":                       # the column most pixels see (meshes 12 .. 75 are the columns)
            ctx.render(st)
            tri = ctx.read_buffer(capi.BUF_PAYLOAD)["objectIndex"]
            seen = [int(((tri >= f) & (tri < f + c)).sum()) for f, c, _ in sc.meshes]
            column = 12 + int(np.argmax(seen[12:76]))
        meshes = [] if not edit else ([column] if edit == "column" else list(range(len(sc.meshes))))
        runs.append(dict(label=label, ctx=ctx, meshes=meshes, call=[], reproject=[], frame=[], edit_ms=[]))
    for rep in range(a.warmup + a.reps):
        st.rand_seed = rep + 1
        for r in runs:
            ctx = r["ctx"]
            if r["meshes"]:
                d = 0.01 * (1 + rep % 2)                               # back and forth between two poses
                mats = [mesh_matrix((base[m]["pos"][0] + d, base[m]["pos"][1], base[m]["pos"][2] + d), base[m]["rotation"], base[m]["scale"])
                        for m in r["meshes"]]
                t0 = time.perf_counter()
                ctx.update_transforms(sc, r["meshes"], mats)
                ms = (time.perf_counter() - t0) * 1e3
            fr = ctx.render(st).kernel_ms
            s = ctx.denoise_temporal(tp, want_radiance=False, with_stats=True)[2]
            if rep >= a.warmup:
                r["call"].append(s.kernel_ms); r["reproject"].append(s.kernel_ms_part[1]); r["frame"].append(fr)
                if r["meshes"]:
                    r["edit_ms"].append(ms)
    lines = []
    for r in runs:
        tri = r["ctx"].read_buffer(capi.BUF_PAYLOAD)["objectIndex"]
        moved = sum(int(((tri >= sc.meshes[m][0]) & (tri < sc.meshes[m][0] + sc.meshes[m][1])).sum()) for m in r["meshes"])
        N = r["ctx"].read_buffer(capi.BUF_TEMPORAL)["N"]
        line = {"what": "temporal call, hall 1M", "context": r["label"], "size": a.size, "reps": a.reps, "call_ms": stats(r["call"]),
                "reproject_ms": stats(r["reproject"]), "frame_ms": stats(r["frame"]), "meshes_edited": len(r["meshes"]),
                "pixels_on_edited_meshes": moved, "largest_N": float(N.max())}
        if r["edit_ms"]:
            line["update_transforms_host_ms"] = stats(r["edit_ms"])
        lines.append(line)
        print(json.dumps(line), flush=True)
        r["ctx"].close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
