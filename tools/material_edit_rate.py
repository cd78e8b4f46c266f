#!/usr/bin/env python3
"""What a material edit costs on the 1M-triangle hall: fyprt_update_materials next to fyprt_upload_scene of the same edited scene, in
the same process, for three edits —
  (i)   the albedo of a palette material (the fast path: table only);
  (ii)  the emission power of one light material (emissive list, light records, that mesh's light tree);
  (iii) a column mesh (7 680 triangles) reassigned to a light material and back (reassignment kernel, list, records, all light trees).
Wall time: medians over interleaved repetitions (update, upload, next case, ...).  Device time: the sum of the kernel times (and, apart,
of the copies) of one update_materials call, from a rocprofv3 kernel + memory-copy trace of a child process that runs the same edits;
the cases are separated in the trace by a one-ray query, whose kernel serves as a marker (MARKER matches the kernel names of the
closest-hit lane state, rt::k_query<rt::RayLane<false, ...>> and k_query_simple of it, whichever tuning key 15 chooses).
  usage: material_edit_rate.py [--reps 7] [--no-trace] [--out profiles/materials/material_edit_rate.jsonl]
         material_edit_rate.py --child REPS          (what runs under rocprofv3)"""
import argparse
import csv
import json
import shutil
import subprocess
import sys
import tempfile
import time
from dataclasses import replace
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402

CASES = ("albedo", "emission_power", "reassign_column")
UPDATE_KERNELS = ("k_set_mesh_material", "k_emissive_count", "k_emissive_scan", "k_emissive_scatter", "k_build_light_records")
MARKER = "RayLane<false"


def make_scene():
    sc = scenes.hall_scene()
    sc.manager().perform_all_scene_updates(sc)
    n_palette = 12
    column = next(m for m, (_, count, _) in enumerate(sc.meshes) if count == 7680)
    return sc, n_palette, column, sc.meshes[column][2]


def apply_edit(sc, case, step, n_palette, column, column_material):
    """Edit number `step` of a case (alternating, so that every call has something to do); returns the reassigned meshes."""
    mgr = sc.manager()
    meshes = []
    if case == "albedo":
        sc.materials[4] = replace(sc.materials[4], albedo=(0.2, 0.9, 0.4) if step % 2 == 0 else (0.7, 0.4, 0.5))
        mgr.material_edited(4)
    elif case == "emission_power":
        sc.materials[n_palette] = replace(sc.materials[n_palette], emission_power=12.0 if step % 2 == 0 else 31.0)
        mgr.material_edited(n_palette)
    else:
        mgr.set_mesh_material(sc, column, n_palette if step % 2 == 0 else column_material)
        meshes = [column]
    mgr.perform_all_scene_updates(sc)
    return meshes


def child(reps):
    sc, n_palette, column, column_material = make_scene()
    ctx = capi.Context(0)
    ctx.upload_scene(sc)
    o, d = np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32)
    ctx.trace_rays(o, d)
    for case in CASES:
        for step in range(reps):
            ctx.update_materials(sc, apply_edit(sc, case, step, n_palette, column, column_material))
        ctx.trace_rays(o, d)
    ctx.close()


def device_times(reps):
    """{case: {kernel_us, copy_us, kernels: {name: us}}} per update_materials call, from a traced child."""
    if shutil.which("rocprofv3") is None:
        return None
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, str(Path(__file__).resolve()), "--child", str(reps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        kernels, copies = [], []
        for f in Path(tmp).rglob("*_kernel_trace.csv"):
            kernels += list(csv.DictReader(open(f)))
        for f in Path(tmp).rglob("*_memory_copy_trace.csv"):
            copies += list(csv.DictReader(open(f)))
    kernels.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [int(r["Start_Timestamp"]) for r in kernels if MARKER in r["Kernel_Name"]]
    if len(marks) != len(CASES) + 1:
        raise RuntimeError(f"expected {len(CASES) + 1} marker kernels in the trace, found {len(marks)}")
    out = {}
    for k, case in enumerate(CASES):
        lo, hi = marks[k], marks[k + 1]
        per = {}
        for r in kernels:
            t = int(r["Start_Timestamp"])
            if lo < t < hi and MARKER not in r["Kernel_Name"]:
                name = next((n for n in UPDATE_KERNELS if n in r["Kernel_Name"]), r["Kernel_Name"].split("(")[0])
                per[name] = per.get(name, 0) + int(r["End_Timestamp"]) - t
        copy_ns = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in copies if lo < int(r["Start_Timestamp"]) < hi)
        n_copies = sum(1 for r in copies if lo < int(r["Start_Timestamp"]) < hi)
        out[case] = {"kernel_us_per_call": round(sum(per.values()) / reps / 1e3, 2), "copy_us_per_call": round(copy_ns / reps / 1e3, 2),
                     "copies_per_call": round(n_copies / reps, 1), "kernels_us_per_call": {n: round(v / reps / 1e3, 2) for n, v in sorted(per.items())}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return
    dev = None if args.no_trace else device_times(6)         # first: the child has the GPU to itself
    sc, n_palette, column, column_material = make_scene()
    a, b = capi.Context(0), capi.Context(0)
    a.upload_scene(sc)
    b.upload_scene(sc)
    wall = {c: {"update": [], "upload": []} for c in CASES}
    for step in range(args.reps + 1):                        # interleaved; the first round warms up and is dropped
        for case in CASES:
            meshes = apply_edit(sc, case, step, n_palette, column, column_material)
            t = time.perf_counter(); a.update_materials(sc, meshes); t_update = time.perf_counter() - t
            t = time.perf_counter(); b.upload_scene(sc); t_upload = time.perf_counter() - t
            if step:
                wall[case]["update"].append(t_update)
                wall[case]["upload"].append(t_upload)
    same = np.array_equal(a.export_emissive(), b.export_emissive())
    lines = []
    for case in CASES:
        u, f = np.array(wall[case]["update"]), np.array(wall[case]["upload"])
        rec = {"case": case, "scene": "hall", "triangles": int(len(sc.triangles)), "meshes": len(sc.meshes), "reps": args.reps,
               "update_materials_wall_ms_median": round(float(np.median(u)) * 1e3, 3), "update_materials_wall_ms_min_max": [round(float(u.min()) * 1e3, 3), round(float(u.max()) * 1e3, 3)],
               "upload_scene_wall_ms_median": round(float(np.median(f)) * 1e3, 1), "upload_scene_wall_ms_min_max": [round(float(f.min()) * 1e3, 1), round(float(f.max()) * 1e3, 1)],
               "upload_over_update": round(float(np.median(f) / np.median(u)), 1), "emissive_lists_equal_at_end": bool(same)}
        if dev:
            rec.update(dev[case])
        lines.append(json.dumps(rec))
        print(lines[-1])
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    a.close()
    b.close()


if __name__ == "__main__":
    main()
