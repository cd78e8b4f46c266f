#!/usr/bin/env python3
"""What a geometry edit costs on the 1M-triangle hall with the full passes and with the partial refit (rt_partial.h), in one process.
Edits: a light mesh (16 triangles), a column (7 680), a drape (31 752), and every mesh.  Per builder (tuning key 12 = 0 host, 2 device
PLOC) and edit:
  * fyprt_update_transforms with tuning key 22 = 0 (the full passes) and 1 (the partial refit), alternating after a warm-up of each:
    host clock around the blocking call, arguments prepared before; medians, extremes and all samples;
  * fyprt_update_vertices (the whole vertex array crosses the bus) against fyprt_update_mesh_vertices (the listed ranges), the same way;
  * what the last partial edit covered (fyprt_last_edit_stats).
Per builder, once: the first partial edit after the upload (it builds the links and, on a host-built tree, fills every node's exact box)
next to a later one of the same mesh, the bytes the links and the walk's scratch hold, and a ReSTIR DI frame for scale.
  usage: partial_refit_rate.py [--reps 15] [--width 1920 --height 1080] [--small] [--out profiles/partial_refit/rate.jsonl]
  (--small: the 11k-triangle hall, to try the tool itself)"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402


def summary(samples_s):
    ms = np.asarray(samples_s, dtype=np.float64) * 1e3
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
            "samples_ms": [round(float(v), 4) for v in ms]}


def timed(fn):
    t = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t
    if rc != 0:
        raise RuntimeError(f"call failed: {rc}")
    return dt


class Edit:
    """One edit prepared for the four calls: the mesh list, two sets of matrices to alternate between (so that every call moves
    something) and the matching world vertices, whole and per listed range."""

    def __init__(self, ctx, sc, mgr, meshes):
        self.ctx, self.meshes = ctx, [int(m) for m in meshes]
        self.idx = (C.c_uint32 * len(self.meshes))(*self.meshes)
        self.variants = []
        home = [dict(sc.mesh_transforms[m]) for m in self.meshes]
        for shift in (0.05, 0.0):
            for m, h in zip(self.meshes, home):
                mgr.set_mesh_transform(sc, m, pos=(h["pos"][0] + shift, h["pos"][1], h["pos"][2] - shift))
            mgr.perform_all_scene_updates(sc)
            mats = np.ascontiguousarray(np.stack([np.asarray(sc.mesh_matrix(m), dtype=np.float32).reshape(4, 4) for m in self.meshes]).reshape(-1))
            whole = np.ascontiguousarray(sc.world_vertices).copy()
            starts = [tr["vertex_start"] for tr in sc.mesh_transforms] + [len(whole)]
            part = np.ascontiguousarray(np.concatenate([whole[starts[m]:starts[m + 1]] for m in self.meshes]))
            self.variants.append((mats, whole, part))
        self.triangles = int(sum(sc.meshes[m][1] for m in self.meshes))
        self.flip = 0

    def _next(self):
        self.flip ^= 1
        return self.variants[self.flip]

    def transforms(self, key22):
        mats, _, _ = self._next()
        self.ctx.set_tuning(22, key22)
        lib, h, n = self.ctx.lib, self.ctx.h, len(self.meshes)
        return timed(lambda: lib.fyprt_update_transforms(h, self.idx, mats.ctypes.data_as(C.POINTER(C.c_float)), n))

    def vertices(self, partial):
        _, whole, part = self._next()
        lib, h, n = self.ctx.lib, self.ctx.h, len(self.meshes)
        if partial:
            return timed(lambda: lib.fyprt_update_mesh_vertices(h, self.idx, n, part.ctypes.data, len(part)))
        return timed(lambda: lib.fyprt_update_vertices(h, whole.ctypes.data, len(whole)))


def alternate(reps, first, second):
    """A warm-up of each, then first / second in turn; returns the two sample lists."""
    first(); second()
    a, b = [], []
    for _ in range(reps):
        a.append(first())
        b.append(second())
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 9:
        ap.error("--reps: at least 9")
    W, H = args.width, args.height
    cam = scenes.hall_camera(W, H)
    st = capi.Settings(technique=capi.RESTIR_DI, use_temporal_reuse=1, use_spatial_reuse=1, sky_color=(0.1, 0.2, 0.3))
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for key12 in (0, 2):
        sc = (scenes.hall_scene_small if args.small else scenes.hall_scene)()
        mgr = sc.manager()
        mgr.perform_all_scene_updates(sc)
        n_col = sum(1 for _, c, _ in sc.meshes if c == sc.meshes[12][1])                      # 12 wall quads, then the columns, the drapes, the light meshes
        n_light = sum(1 for _, _, mi in sc.meshes if mi >= 12)
        cases = {"light_mesh": [len(sc.meshes) - n_light + 1], "column": [12 + n_col // 2], "drape": [12 + n_col + 1], "all_meshes": list(range(len(sc.meshes)))}
        ctx = capi.Context(0)
        ctx.set_tuning(12, key12)
        ctx.resize(W, H)
        ctx.upload_scene(sc)
        ctx.set_camera(cam)
        ctx.set_object_vertices(sc)
        bvh = ctx.export_bvh()
        base = {"scene": "hall_small" if args.small else "hall", "builder_key12": key12, "triangles": int(len(sc.triangles)), "nodes": int(len(bvh["nodes"])),
                "levels": int(bvh["max_stack"])}
        ms = []
        for f in range(12):
            st.rand_seed = f + 1
            ms.append(ctx.render(st).kernel_ms)
        frame_ms = round(float(np.median(ms[4:])), 4)
        edits = {name: Edit(ctx, sc, mgr, meshes) for name, meshes in cases.items()}
        # the one-off: the first partial edit of this tree against a later one of the same edit
        held = capi.live_device_bytes()
        first = edits["light_mesh"].transforms(1)
        link_bytes = capi.live_device_bytes() - held
        later = [edits["light_mesh"].transforms(1) for _ in range(args.reps)]
        emit({**base, "what": "first partial edit", "edit": "light_mesh", "first_partial_edit_ms": round(first * 1e3, 4), "later_partial_edit": summary(later),
              "links_and_scratch_bytes": int(link_bytes), "host_built_tree_gets_node_boxes_first": key12 == 0, "frame": f"ReSTIR DI {W}x{H}", "frame_kernel_ms": frame_ms})
        for name, e in edits.items():
            full, part = alternate(args.reps, lambda: e.transforms(0), lambda: e.transforms(1))
            stats = ctx.last_edit_stats()
            rec = {**base, "what": "update_transforms", "edit": name, "meshes": len(e.meshes), "moved_triangles": e.triangles,
                   "key22_0_full": summary(full), "key22_1_partial": summary(part),
                   "full_over_partial": round(float(np.median(full)) / float(np.median(part)), 2),
                   "partial_stats": {"triangles_refreshed": stats.triangles_refreshed, "leaf_records_refreshed": stats.leaf_records_refreshed,
                                     "nodes_refit": stats.nodes_refit, "level_launches": stats.level_launches}}
            emit(rec)
            whole, listed = alternate(args.reps, lambda: e.vertices(False), lambda: e.vertices(True))
            emit({**base, "what": "update_vertices against update_mesh_vertices", "edit": name, "meshes": len(e.meshes), "moved_triangles": e.triangles,
                  "vertex_bytes_whole": int(e.variants[0][1].nbytes), "vertex_bytes_listed": int(e.variants[0][2].nbytes),
                  "update_vertices": summary(whole), "update_mesh_vertices": summary(listed),
                  "whole_over_listed": round(float(np.median(whole)) / float(np.median(listed)), 2)})
        ctx.set_tuning(22, 0)
        ctx.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
