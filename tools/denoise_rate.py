#!/usr/bin/env python3
"""Cost and effect of the denoiser (fyprt_denoise) on the bench workload, GPU.
The bench hall (1M triangles), ReSTIR DI with bench.py's settings, at 1920x1080 and 3840x2160.  Per size and iteration count 1..6: the
hipEvent time of a denoise call (FrameStats of the host entry: the call's kernels, no copies), after warm-up, over --reps repetitions,
next to the frame's own kernel time in the same session; the compulsory traffic of the iterations (read guide 32 B + colour 16 B, write
colour 16 B: 64 B per pixel and iteration) over their time as a share of the HBM peak (8 TB/s); the increment over the previous count
as the cost of that step.  With --lib-b: the same for an alternative build (tools/build_variant.sh, e.g. -DRT_DN_LDS_MAX_STEP=0: every
step gathers), calls alternating between the two libraries, for the A/B of the LDS-staged kernel at steps 1 and 2.  Finally, at
1920x1080: PSNR (MisUtils::ComputePSNR on the 8-bit images) of frame 1 raw and denoised against a 256-frame accumulation.
One JSON line each.
  usage: python tools/denoise_rate.py [--reps 50] [--lib-b fypraytracer_amd/csrc/variants/libfyprt_gather.so] [--out profiles/denoise/denoise_rate.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from common import mse_psnr  # noqa: E402
from fypraytracer_amd import capi, scenes  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s (specification)


def bench_settings():
    return capi.Settings(technique=capi.RESTIR_DI, light_bounces=1, sample_count=1, sky_color=(0.0, 0.0, 0.0), light_candidate_count=4,
                         use_temporal_reuse=1, use_spatial_reuse=1, temporal_history_limit=2, spatial_neighbor_num=5, spatial_neighbor_radius=30)


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib-b", default=None, help="an alternative libfyprt.so to alternate with (A/B)")
    ap.add_argument("--label-b", default="variant")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--psnr-frames", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise" / "denoise_rate.jsonl"))
    a = ap.parse_args()
    libs = [("default", capi.load_library())]
    if a.lib_b:
        libs.append((a.label_b, capi.load_library(a.lib_b)))
    sc = scenes.hall_scene()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        ctxs = []
        for label, lib in libs:
            ctx = capi.Context(0, lib=lib)
            ctx.resize(W, H)
            ctx.upload_scene(sc)
            ctx.set_camera(scenes.hall_camera(W, H))
            ctxs.append((label, ctx))
        st = bench_settings()
        frame_ms = []
        for rep in range(a.warmup + 20):
            st.rand_seed = rep + 1
            ms = [ctx.render(st).kernel_ms for _, ctx in ctxs]
            if rep >= a.warmup:
                frame_ms.append(ms[0])
        emit({"what": "frame", "size": size, "technique": "RESTIR_DI", "reps": 20, "ms_median": med(frame_ms), "ms_min": round(min(frame_ms), 4),
              "ms_max": round(max(frame_ms), 4)})
        prev = {label: 0.0 for label, _ in ctxs}
        for it in range(1, 7):
            par = capi.DenoiseParams(iterations=it)
            runs = {label: {"total": [], "prepare": [], "iterate": []} for label, _ in ctxs}
            for rep in range(a.warmup + a.reps):
                for label, ctx in ctxs:                                # alternating, same call
                    s = ctx.denoise(par, want_radiance=False, with_stats=True)[2]
                    if rep >= a.warmup:
                        runs[label]["total"].append(s.kernel_ms); runs[label]["prepare"].append(s.kernel_ms_part[0]); runs[label]["iterate"].append(s.kernel_ms_part[1])
            for label, _ in ctxs:
                r = runs[label]
                itms = statistics.median(r["iterate"])
                emit({"what": "denoise", "library": label, "size": size, "iterations": it, "reps": a.reps, "launches": it + 1,
                      "ms_median": med(r["total"]), "ms_min": round(min(r["total"]), 4), "ms_max": round(max(r["total"]), 4),
                      "ms_prepare": med(r["prepare"]), "ms_iterations": round(itms, 4), "ms_last_step": round(itms - prev[label], 4), "last_step": 1 << (it - 1),
                      "compulsory_MB": round(64 * W * H * it / 1e6, 1), "hbm_peak_share": round(64 * W * H * it / (itms * 1e-3) / HBM_PEAK, 3),
                      "ratio_to_frame": round(statistics.median(r["total"]) / statistics.median(frame_ms), 3)})
                prev[label] = itms
        if (W, H) == (1920, 1080) and a.psnr_frames > 1:
            ctx = ctxs[0][1]
            ctx.reset_frame_index()
            st = bench_settings()
            raw = den = None
            for f in range(a.psnr_frames):
                st.rand_seed = f + 1
                ctx.render(st)
                if f == 0:
                    raw = ctx.readback(want_accum=False)[0].copy()
                    den = ctx.denoise(want_radiance=False)[0].copy()
            ref = ctx.readback(want_accum=False)[0]
            (mr, pr), (md, pd) = mse_psnr(raw, ref), mse_psnr(den, ref)
            emit({"what": "psnr", "size": size, "reference_frames": a.psnr_frames, "params": "defaults", "raw_mse": round(mr, 3), "raw_psnr_db": round(pr, 2),
                  "denoised_mse": round(md, 3), "denoised_psnr_db": round(pd, 2)})
        for _, ctx in ctxs:
            ctx.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
