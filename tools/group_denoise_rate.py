#!/usr/bin/env python3
"""Cost of the group denoiser (fyprt_group_denoise) beside fyprt_denoise of one context on the same frame, GPU.
The bench hall (1M triangles), ReSTIR DI with bench.py's settings, 1920x1080, default denoise parameters.  Splits of 1, 2, 4 and 8 even
bands, the contexts dealt round-robin over the GPUs that exist; per split, after warm-up, --reps repetitions in which the single
context's call and the group's call alternate: wall time of either blocking call (both copy the RGBA8 frame back), the single call's
hipEvent kernel time, the per-band hipEvent times (band_ms, waits for the neighbours included) and the bytes the bands pull from each
other per call (fyprt_group_denoise_plan).  Medians, one JSON line per split.
With fewer GPUs than bands the bands share a device and run one after the other: the figures then show the overhead of the split
(more launches, the pulls, the collect), not scaling.
  usage: python tools/group_denoise_rate.py [--reps 20] [--splits 1,2,4,8] [--lib PATH --label NAME] [--out profiles/denoise/group_denoise_rate.jsonl]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402

GUIDE_BYTES, COLOUR_BYTES = 32, 16


def bench_settings():
    return capi.Settings(technique=capi.RESTIR_DI, light_bounces=1, sample_count=1, sky_color=(0.0, 0.0, 0.0), light_candidate_count=4,
                         use_temporal_reuse=1, use_spatial_reuse=1, temporal_history_limit=2, spatial_neighbor_num=5, spatial_neighbor_radius=30)


def med(v):
    return round(statistics.median(v), 4)


def gpu_count(limit, lib):
    n = 0
    while n < limit:
        try:
            capi.Context(n, lib=lib).close()
        except capi.FyprtError:
            break
        n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--splits", default="1,2,4,8")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise" / "group_denoise_rate.jsonl"))
    ap.add_argument("--lib", default=None, help="an alternative libfyprt.so to measure instead of the built one (before / after runs)")
    ap.add_argument("--label", default="default", help="the `library` field of the lines")
    a = ap.parse_args()
    lib = capi.load_library(a.lib) if a.lib else capi.load_library()
    W, H = (int(x) for x in a.size.split("x"))
    splits = [int(x) for x in a.splits.split(",")]
    gpus = gpu_count(max(splits), lib)
    sc, cam, st, par = scenes.hall_scene(), scenes.hall_camera(W, H), bench_settings(), capi.DenoiseParams()

    def context(device):
        c = capi.Context(device, lib=lib)
        c.resize(W, H)
        c.upload_scene(sc)
        c.set_camera(cam)
        return c

    single = context(0)
    single.render(st)
    members = [context(k % gpus) for k in range(max(splits))]
    lines = []
    for n in splits:
        bounds = [round(H * k / n) for k in range(n + 1)]
        for c in members[:n]:
            c.resize(W, H)                                               # a fresh frame 1, and the denoiser's buffers sized for this split
        grp = capi.Group(members[:n], bounds, halo_mode=1)
        grp.render(st)
        grp.synchronize()
        plan = capi.group_denoise_plan(bounds, H, par.iterations, lib=lib)
        pulled = sum((r1 - r0) * W * (GUIDE_BYTES if stage == 0 else COLOUR_BYTES) for stage, _, _, r0, r1 in plan)
        wall_s, wall_g, kern_s, band = [], [], [], []
        same = None
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            img_s, _, stats = single.denoise(par, want_radiance=False, with_stats=True)
            t1 = time.perf_counter()
            img_g, _, ms = grp.denoise(par, want_radiance=False, with_band_ms=True)
            t2 = time.perf_counter()
            if same is None:
                same = bool((img_s == img_g).all())
            if rep >= a.warmup:
                wall_s.append((t1 - t0) * 1e3); wall_g.append((t2 - t1) * 1e3); kern_s.append(stats.kernel_ms); band.append(ms)
        line = {"what": "group_denoise", "library": a.label, "size": a.size, "iterations": par.iterations, "bands": n, "gpus": min(gpus, n), "bands_share_a_gpu": gpus < n,
                "reps": a.reps, "equal_to_single": same, "single_wall_ms": med(wall_s), "single_kernel_ms": med(kern_s),
                "group_wall_ms": med(wall_g), "group_wall_ms_min": round(min(wall_g), 4), "group_wall_ms_max": round(max(wall_g), 4),
                "band_ms": [med([b[k] for b in band]) for k in range(n)], "transfers": len(plan), "pulled_MB": round(pulled / 1e6, 2)}
        lines.append(line)
        print(json.dumps(line), flush=True)
        grp.close()
    for c in members + [single]:
        c.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
