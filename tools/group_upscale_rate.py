#!/usr/bin/env python3
"""Cost of the group upscaler (fyprt_group_denoise_upscale) beside fyprt_denoise_upscale of one context, GPU.
The bench hall (1M triangles), ReSTIR DI with bench.py's settings and to_accumulate = 0, 1920x1080 -> 3840x2160 (scale 2), default
parameters, spatial mode.  Splits of 1, 2, 4 and 8 even bands, the contexts dealt round-robin over the GPUs that exist.  Per split, after
warm-up, --reps repetitions of: a frame on the single context and on the group, then — interleaved, in the same session — the single
context's call and the group's call on the same frame (both copy the RGBA8 hi-res frame back).  Wall time of either blocking call, the
single call's hipEvent kernel time and its three parts, the per-band hipEvent times (band_ms, waits for the neighbours included) and the
bytes the bands pull from each other per call (fyprt_group_denoise_upscale_plan).  Medians with minimum and maximum, one JSON line per
split.
With --lib-b (the library of another commit): one more line, the single-context call of both libraries on the same frames, calls
alternating — what the band form of the two hi-res kernels costs the full-frame call, beside that library's own run-to-run spread.
With fewer GPUs than bands the bands share a device and run one after the other: the figures then show the cost of the split (more
launches, the pulls, the collect), not scaling, and no scaling is claimed from them.
  usage: python tools/group_upscale_rate.py [--reps 20] [--splits 1,2,4,8] [--lib PATH --label NAME] [--lib-b PATH --label-b NAME] [--out profiles/upscale/group_upscale_rate.jsonl]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402


def bench_settings():
    st = capi.Settings(technique=capi.RESTIR_DI, light_bounces=1, sample_count=1, sky_color=(0.0, 0.0, 0.0), light_candidate_count=4,
                       use_temporal_reuse=1, use_spatial_reuse=1, temporal_history_limit=2, spatial_neighbor_num=5, spatial_neighbor_radius=30)
    st.to_accumulate = 0
    return st


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


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
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--splits", default="1,2,4,8")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--lib", default=None, help="an alternative libfyprt.so to measure instead of the built one")
    ap.add_argument("--label", default="default", help="the `library` field of the lines")
    ap.add_argument("--lib-b", default=None, help="an alternative libfyprt.so whose single-context call alternates with the built one's (A/B)")
    ap.add_argument("--label-b", default="variant")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "upscale" / "group_upscale_rate.jsonl"))
    a = ap.parse_args()
    lib = capi.load_library(a.lib) if a.lib else capi.load_library()
    W, H = (int(x) for x in a.size.split("x"))
    s = a.scale
    splits = [int(x) for x in a.splits.split(",")]
    gpus = gpu_count(max(splits), lib)
    sc, cam, st, par = scenes.hall_scene(), scenes.hall_camera(W, H), bench_settings(), capi.UpscaleParams(scale=s)
    it = par.filter.spatial.iterations

    def context(device, lb=lib):
        c = capi.Context(device, lib=lb)
        c.resize(W, H)
        c.upload_scene(sc)
        c.set_camera(cam)
        return c

    single = context(0)
    lines = []
    if a.lib_b:                                                          # (a) the full-frame call: this library beside another commit's
        other = context(0, capi.load_library(a.lib_b))
        parts = {a.label: [], a.label_b: []}
        same = True
        for rep in range(a.warmup + a.reps):
            st.rand_seed = rep + 1
            outs = []
            for label, c in ((a.label, single), (a.label_b, other)) if rep % 2 == 0 else ((a.label_b, other), (a.label, single)):
                c.render(st)
                img, _, stats = c.denoise_upscale(par, want_radiance=False, with_stats=True)
                outs.append(img)
                if rep >= a.warmup:
                    parts[label].append((stats.kernel_ms,) + tuple(stats.kernel_ms_part[:3]))
            same = same and bool((outs[0] == outs[1]).all())
        line = {"what": "single_context_call_a_b", "size": a.size, "scale": s, "output": f"{W * s}x{H * s}", "reps": a.reps, "images_equal": same}
        for label, v in parts.items():
            line[label] = {"kernel_ms": spread([p[0] for p in v]), "ms_lowres_stage": spread([p[1] for p in v]),
                           "ms_up_primary": spread([p[2] for p in v]), "ms_up_resolve": spread([p[3] for p in v])}
        lines.append(line)
        print(json.dumps(line), flush=True)
        other.close()
    members = [context(k % gpus) for k in range(max(splits))]
    for n in splits:
        bounds = [round(H * k / n) for k in range(n + 1)]
        for c in members[:n] + [single]:
            c.resize(W, H)                                               # a fresh frame 1, the buffers sized for this split
        grp = capi.Group(members[:n], bounds, halo_mode=1)
        plan = capi.group_denoise_upscale_plan(bounds, H, it, False, lib=lib)
        pulled = sum((r1 - r0) * W * (32 if stage == 0 else 16) for stage, _, _, r0, r1 in plan)
        wall_s, wall_g, kern_s, band = [], [], [], []
        same = True
        for rep in range(a.warmup + a.reps):
            st.rand_seed = rep + 1
            single.render(st)
            grp.render(st)
            grp.synchronize()
            single.synchronize()
            t0 = time.perf_counter()
            img_s, _, stats = single.denoise_upscale(par, want_radiance=False, with_stats=True)
            t1 = time.perf_counter()
            img_g, _, ms = grp.denoise_upscale(par, want_radiance=False, with_band_ms=True)
            t2 = time.perf_counter()
            if rep < a.warmup:
                same = same and bool((img_s == img_g).all())
            else:
                wall_s.append((t1 - t0) * 1e3); wall_g.append((t2 - t1) * 1e3); kern_s.append(stats.kernel_ms); band.append(ms)
        line = {"what": "group_denoise_upscale", "library": a.label, "size": a.size, "scale": s, "output": f"{W * s}x{H * s}", "iterations": it, "bands": n,
                "gpus": min(gpus, n), "bands_share_a_gpu": gpus < n, "reps": a.reps, "equal_to_single_in_warmup": same,
                "single_wall_ms": spread(wall_s), "single_kernel_ms": spread(kern_s), "group_wall_ms": spread(wall_g),
                "band_ms": [spread([b[k] for b in band]) for k in range(n)], "band_ms_sum": spread([sum(b) for b in band]),
                "transfers": len(plan), "pulled_MB": round(pulled / 1e6, 2)}
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
