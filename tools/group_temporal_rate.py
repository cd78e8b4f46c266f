#!/usr/bin/env python3
"""Cost of the group temporal denoiser (fyprt_group_denoise_temporal) beside fyprt_denoise_temporal of one context, GPU.
The bench hall (1M triangles), ReSTIR DI with bench.py's settings and to_accumulate = 0, 1920x1080, default parameters.  Splits of 1, 2, 4
and 8 even bands, the contexts dealt round-robin over the GPUs that exist; per split and per history window (history_rows 0, 32 and the
height), after warm-up, --reps repetitions of: a frame on the single context and on the group, then the single context's call and the
group's call (both in steady state: a history of the calls before; both copy the RGBA8 frame back).  Wall time of either blocking call,
the single call's hipEvent kernel time, the per-band hipEvent times (band_ms, waits for the neighbours included) and the bytes the bands
pull from each other per call and per stage (fyprt_group_denoise_temporal_plan).  Medians, one JSON line per split and window.
With fewer GPUs than bands the bands share a device and run one after the other: the figures then show the overhead of the split
(more launches, the pulls, the collect), not scaling.
  usage: python tools/group_temporal_rate.py [--reps 20] [--splits 1,2,4,8] [--lib PATH --label NAME] [--out profiles/denoise/group_temporal_rate.jsonl]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402

STAGE_BYTES = {0: 32, 1: 16, 2: 64}        # guide, prepared colour, history; stage 3 + k: colour 16 + variance 4


def bench_settings():
    st = capi.Settings(technique=capi.RESTIR_DI, light_bounces=1, sample_count=1, sky_color=(0.0, 0.0, 0.0), light_candidate_count=4,
                       use_temporal_reuse=1, use_spatial_reuse=1, temporal_history_limit=2, spatial_neighbor_num=5, spatial_neighbor_radius=30)
    st.to_accumulate = 0
    return st


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
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--splits", default="1,2,4,8")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise" / "group_temporal_rate.jsonl"))
    ap.add_argument("--lib", default=None, help="an alternative libfyprt.so to measure instead of the built one (before / after runs)")
    ap.add_argument("--label", default="default", help="the `library` field of the lines")
    a = ap.parse_args()
    lib = capi.load_library(a.lib) if a.lib else capi.load_library()
    W, H = (int(x) for x in a.size.split("x"))
    splits = [int(x) for x in a.splits.split(",")]
    gpus = gpu_count(max(splits), lib)
    sc, cam, st, par = scenes.hall_scene(), scenes.hall_camera(W, H), bench_settings(), capi.TemporalParams()

    def context(device):
        c = capi.Context(device, lib=lib)
        c.resize(W, H)
        c.upload_scene(sc)
        c.set_camera(cam)
        return c

    single = context(0)
    members = [context(k % gpus) for k in range(max(splits))]
    lines = []
    for n in splits:
        bounds = [round(H * k / n) for k in range(n + 1)]
        for R in (0, capi.GROUP_HISTORY_ROWS, H):
            for c in members[:n] + [single]:
                c.resize(W, H)                                           # a fresh frame 1, no history, the buffers sized for this split
            grp = capi.Group(members[:n], bounds, halo_mode=1)
            plan = capi.group_denoise_temporal_plan(bounds, H, par.spatial.iterations, R, lib=lib)
            per_stage = {}
            for stage, _, _, r0, r1 in plan:
                per_stage[stage] = per_stage.get(stage, 0) + (r1 - r0) * W * STAGE_BYTES.get(stage, 20)
            wall_s, wall_g, kern_s, band = [], [], [], []
            same = True
            for rep in range(a.warmup + a.reps):
                st.rand_seed = rep + 1
                single.render(st)
                grp.render(st)
                grp.synchronize()
                t0 = time.perf_counter()
                img_s, _, stats = single.denoise_temporal(par, want_radiance=False, with_stats=True)
                t1 = time.perf_counter()
                img_g, _, ms = grp.denoise_temporal(par, history_rows=R, want_radiance=False, with_band_ms=True)
                t2 = time.perf_counter()
                if rep < a.warmup:
                    same = same and bool((img_s == img_g).all())
                else:
                    wall_s.append((t1 - t0) * 1e3); wall_g.append((t2 - t1) * 1e3); kern_s.append(stats.kernel_ms); band.append(ms)
            line = {"what": "group_denoise_temporal", "library": a.label, "size": a.size, "iterations": par.spatial.iterations, "bands": n, "history_rows": R,
                    "gpus": min(gpus, n), "bands_share_a_gpu": gpus < n, "reps": a.reps, "equal_to_single_in_warmup": same,
                    "single_wall_ms": med(wall_s), "single_kernel_ms": med(kern_s), "group_wall_ms": med(wall_g),
                    "group_wall_ms_min": round(min(wall_g), 4), "group_wall_ms_max": round(max(wall_g), 4),
                    "band_ms": [med([b[k] for b in band]) for k in range(n)], "transfers": len(plan),
                    "pulled_MB_per_stage": {str(k): round(v / 1e6, 2) for k, v in sorted(per_stage.items())},
                    "pulled_MB": round(sum(per_stage.values()) / 1e6, 2)}
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
