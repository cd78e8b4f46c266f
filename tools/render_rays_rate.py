#!/usr/bin/env python3
"""Rate of the radiance queries (fyprt_render_rays) against the frame they generalise, GPU.
The bench hall (1M triangles) at 1920x1080, with the config 3 settings (NEE, 1 spp, 2 bounces) and with cosine sampling (1 spp,
2 bounces).  For each: the frame's kernel_ms (fyprt_render stats), and render_rays' kernel_ms on the same camera rays, in 8x8-tile order
(pixel indices) and in row-major order (first_index 0); after warm-up, frame and the two queries alternate over --reps repetitions.
One JSON line per (settings, variant): median, min, max ms and the ratio of the medians to the frame's.
  usage: python tools/render_rays_rate.py [--reps 20] [--out profiles/r05/render_rays_rate.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from common import settings_for  # noqa: E402
from fypraytracer_amd import capi, scenes  # noqa: E402

F32 = np.float32


def tile_order(W, H, t=8):
    """Pixel indices of a W x H image (both multiples of t) walked t x t tile after tile, tiles in row-major order."""
    ty, tx, iy, ix = np.meshgrid(np.arange(H // t), np.arange(W // t), np.arange(t), np.arange(t), indexing="ij")
    return ((ty * t + iy) * W + tx * t + ix).reshape(-1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r05" / "render_rays_rate.jsonl"))
    a = ap.parse_args()
    W, H = 1920, 1080
    cam = scenes.hall_camera(W, H)
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(scenes.hall_scene())
    ctx.set_camera(cam)
    d = cam.ray_directions().reshape(-1, 3).astype(F32)
    o = np.broadcast_to(np.asarray(cam.position, F32), d.shape).copy()
    tiles = tile_order(W, H)
    ot, dt = o[tiles].copy(), d[tiles].copy()
    lines = []
    for label, st in (("config3_nee_1spp_2b", settings_for(capi.NEE, sample_count=1, light_bounces=2)),
                      ("cosine_1spp_2b", settings_for(capi.COSINE_WEIGHTED_SAMPLING, sample_count=1, light_bounces=2))):
        st.to_accumulate = 0
        runs = {"frame": [], "query_tile8x8": [], "query_rowmajor": []}
        for rep in range(a.warmup + a.reps):
            f = ctx.render(st).kernel_ms
            qt = ctx.render_rays(ot, dt, st, pixel_indices=tiles, with_stats=True)[1]
            qr = ctx.render_rays(o, d, st, with_stats=True)[1]
            if rep >= a.warmup:
                runs["frame"].append(f); runs["query_tile8x8"].append(qt.kernel_ms); runs["query_rowmajor"].append(qr.kernel_ms)
        fmed = statistics.median(runs["frame"])
        for k, v in runs.items():
            med = statistics.median(v)
            line = {"settings": label, "variant": k, "rays": W * H, "reps": a.reps, "ms_median": round(med, 4), "ms_min": round(min(v), 4),
                    "ms_max": round(max(v), 4), "ratio_to_frame": round(med / fmed, 3)}
            if k != "frame":
                line["launches"] = qt.launches
            lines.append(line)
            print(json.dumps(line), flush=True)
    ctx.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
