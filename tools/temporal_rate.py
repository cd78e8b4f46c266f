#!/usr/bin/env python3
"""Cost of the temporal denoiser (fyprt_denoise_temporal) on the bench workload, GPU.
The bench hall (1M triangles), ReSTIR DI with bench.py's settings and to_accumulate = 0, at 1920x1080 and 3840x2160.  In one process,
alternating per repetition: a frame, a steady-state temporal call (full history: every pixel takes the temporal variance), a first call
(after fyprt_denoise_temporal_reset: every pixel takes the 5 x 5 spatial variance estimate) and a spatial call (fyprt_denoise) at the
same `iterations` — hipEvent times of the calls' kernels (FrameStats of the host entries, no copies), per kernel group (prepare,
reproject + variance, iterations), median over --reps after warm-up.  The compulsory traffic of the reproject kernel (prepare's guide
32 B + colour 16 B in, four 64-byte history lines gathered at most — 64 B when the taps of neighbours are shared —, one 64-byte record +
16 B colour + 4 B variance out: 196 B per pixel) over its time as a share of the HBM peak (8 TB/s).  Per iteration count 1..5 the
iterations' time of both denoisers, so that the increment of k_dt_iterate<STEP> over k_dn_iterate<STEP> shows per step.  With --lib-b
(tools/build_variant.sh gather -DRT_DN_LDS_MAX_STEP=0: every step gathers) the same for the gather form, calls alternating between the
libraries; with --lib-parent the parent commit's library joins for its spatial call alone (the yardstick).  One JSON line each.
  usage: python tools/temporal_rate.py [--reps 50] [--lib-b .../variants/libfyprt_gather.so] [--lib-parent PATH] [--out profiles/temporal/temporal_rate.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s (specification)
REPROJECT_BYTES = 32 + 16 + 64 + 64 + 16 + 4


def bench_settings():
    st = capi.Settings(technique=capi.RESTIR_DI, light_bounces=1, sample_count=1, sky_color=(0.0, 0.0, 0.0), light_candidate_count=4,
                       use_temporal_reuse=1, use_spatial_reuse=1, temporal_history_limit=2, spatial_neighbor_num=5, spatial_neighbor_radius=30)
    st.to_accumulate = 0
    return st


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--lib-b", default=None, help="an alternative libfyprt.so with the temporal entry to alternate with (A/B)")
    ap.add_argument("--label-b", default="gather")
    ap.add_argument("--lib-parent", default=None, help="the parent commit's libfyprt.so: its fyprt_denoise is timed beside")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "temporal" / "temporal_rate.jsonl"))
    a = ap.parse_args()
    libs = [("default", capi.load_library(), True)]
    if a.lib_b:
        libs.append((a.label_b, capi.load_library(a.lib_b), True))
    if a.lib_parent:
        libs.append(("parent commit", capi.load_library(a.lib_parent), False))
    sc = scenes.hall_scene()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        ctxs = []
        for label, lib, temporal in libs:
            ctx = capi.Context(0, lib=lib)
            ctx.resize(W, H)
            ctx.upload_scene(sc)
            ctx.set_camera(scenes.hall_camera(W, H))
            ctxs.append((label, ctx, temporal))
        st = bench_settings()
        for it in (5, 1, 2, 3, 4):
            tp, dp = capi.TemporalParams(iterations=it), capi.DenoiseParams(iterations=it)
            runs = {label: {k: [] for k in ("frame", "steady", "steady_prepare", "steady_reproject", "steady_iterate", "first", "first_reproject",
                                            "spatial", "spatial_iterate")} for label, _, _ in ctxs}
            for rep in range(a.warmup + a.reps):
                st.rand_seed = rep + 1
                for label, ctx, temporal in ctxs:                      # alternating, same calls
                    r = {"frame": ctx.render(st).kernel_ms}
                    if temporal:
                        s = ctx.denoise_temporal(tp, want_radiance=False, with_stats=True)[2]      # history of the calls before: steady state
                        r.update(steady=s.kernel_ms, steady_prepare=s.kernel_ms_part[0], steady_reproject=s.kernel_ms_part[1],
                                 steady_iterate=s.kernel_ms_part[2])
                    s = ctx.denoise(dp, want_radiance=False, with_stats=True)[2]
                    r.update(spatial=s.kernel_ms, spatial_iterate=s.kernel_ms_part[1])
                    if rep >= a.warmup:
                        for k, v in r.items():
                            runs[label][k].append(v)
            if it == 5:                                                # first calls, in a pass of their own (a reset would break the steady state)
                for rep in range(a.warmup + a.reps):
                    for label, ctx, temporal in ctxs:
                        if not temporal:
                            continue
                        ctx.denoise_temporal_reset()
                        s = ctx.denoise_temporal(tp, want_radiance=False, with_stats=True)[2]
                        if rep >= a.warmup:
                            runs[label]["first"].append(s.kernel_ms); runs[label]["first_reproject"].append(s.kernel_ms_part[1])
                for label, ctx, temporal in ctxs:                      # rebuild the history for the counts that follow
                    for _ in range(4 if temporal else 0):
                        ctx.denoise_temporal(tp, want_radiance=False)
            for label, _, temporal in ctxs:
                r = runs[label]
                line = {"what": "temporal" if temporal else "spatial only", "library": label, "size": size, "iterations": it, "reps": a.reps,
                        "frame_ms": med(r["frame"]), "spatial_ms": med(r["spatial"]), "spatial_iterations_ms": med(r["spatial_iterate"])}
                if temporal:
                    rp = statistics.median(r["steady_reproject"])
                    line.update(steady_ms=med(r["steady"]), steady_min=round(min(r["steady"]), 4), steady_max=round(max(r["steady"]), 4),
                                prepare_ms=med(r["steady_prepare"]), reproject_ms=round(rp, 4), iterations_ms=med(r["steady_iterate"]),
                                reproject_MB=round(REPROJECT_BYTES * W * H / 1e6, 1),
                                reproject_hbm_peak_share=round(REPROJECT_BYTES * W * H / (rp * 1e-3) / HBM_PEAK, 3),
                                iterations_over_spatial=round(statistics.median(r["steady_iterate"]) / statistics.median(r["spatial_iterate"]), 3),
                                steady_over_spatial=round(statistics.median(r["steady"]) / statistics.median(r["spatial"]), 3),
                                steady_over_frame=round(statistics.median(r["steady"]) / statistics.median(r["frame"]), 3))
                    if r["first"]:
                        line.update(first_ms=med(r["first"]), first_reproject_ms=med(r["first_reproject"]),
                                    first_over_spatial=round(statistics.median(r["first"]) / statistics.median(r["spatial"]), 3))
                emit(line)
        for _, ctx, _ in ctxs:
            ctx.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
