#!/usr/bin/env python3
"""Cost and effect of the upscaler (fyprt_denoise_upscale) on the bench workload, GPU.
The bench hall (1M triangles) with bench.py's ReSTIR DI settings and config 5's ReSTIR GI (2 bounces), at 960x540 -> 1920x1080 (s = 2),
1920x1080 -> 3840x2160 (s = 2) and 1280x720 -> 3840x2160 (s = 3).  Per size and technique, one JSON line each:
  upscale   the hipEvent time of the call's three parts (FrameStats of the host entry: the low-res stage, k_up_primary, k_up_resolve;
            median over --reps after warm-up), and the resolve kernel's compulsory bytes — per hi-res pixel guide 32 B + albedo 16 B read,
            rgba8 4 B written; per low-res pixel guide 32 B + colour 16 B + accumulation 16 B + albedo 16 B read — over its time as a
            share of the HBM peak (8 TB/s).  With --lib-b: the same for an alternative build (tools/build_variant.sh), calls
            alternating between the two libraries — how the resolve kernel's gather form was timed before it was removed.
  compare   "frame at sW x sH + fyprt_denoise" against "frame at W x H + this call", both in this session (no figure of another commit).
  psnr      MisUtils::ComputePSNR on the 8-bit images against a --psnr-frames accumulation at sW x sH of: the native one-frame denoised
            image, the upscaled image, the low-res denoised image replicated s x s.
            The same three on the textured banana scene (ReSTIR DI), where the hi-res albedo carries detail the low-res frame lacks.
and per size (the scene's geometry alone decides it):
  primary   k_up_primary against fyprt_trace_rays' closest-hit query on the same sW x sH camera rays (tools/query_rate.py's set (a)) plus
            a k_dn_prepare launch at that size.
  usage: python tools/upscale_rate.py [--reps 30] [--lib-b fypraytracer_amd/csrc/variants/libfyprt_NAME.so] [--out profiles/upscale/upscale_rate.jsonl]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from common import mse_psnr  # noqa: E402
from fypraytracer_amd import capi, scenes  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s (specification)
CASES = [(960, 540, 2), (1920, 1080, 2), (1280, 720, 3)]


def settings(tech):
    return capi.Settings(technique=tech, light_bounces=2 if tech != capi.RESTIR_DI else 1, sample_count=1, sky_color=(0.0, 0.0, 0.0),
                         light_candidate_count=4, use_temporal_reuse=1, use_spatial_reuse=1, temporal_history_limit=2, spatial_neighbor_num=5,
                         spatial_neighbor_radius=30)


def med(v):
    return round(statistics.median(v), 4)


def spread(v):
    return {"ms_median": med(v), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def frames_ms(ctx, st, warmup, reps):
    ms = []
    for rep in range(warmup + reps):
        st.rand_seed = rep + 1
        t = ctx.render(st).kernel_ms
        if rep >= warmup:
            ms.append(t)
    return ms


def psnr_line(low, high, scene, tech, size, s, frames):
    """PSNR against `frames` accumulated frames of `high` (sW x sH) of: its denoised frame 1, frame 1 of `low` (W x H) upscaled, and
    that frame denoised and replicated s x s.  Both contexts hold the scene and their cameras."""
    for ctx in (low, high):
        ctx.reset_frame_index()
    st = settings(tech)
    st.rand_seed = 1
    low.render(st)
    up_img = low.denoise_upscale(capi.UpscaleParams(scale=s), want_radiance=False)[0].copy()
    rep_img = np.repeat(np.repeat(low.denoise(want_radiance=False)[0], s, axis=0), s, axis=1)
    nat_img = None
    for f in range(frames):
        st.rand_seed = f + 1
        high.render(st)
        if f == 0:
            nat_img = high.denoise(want_radiance=False)[0].copy()
    ref = high.readback(want_accum=False)[0]
    res = {k: mse_psnr(img, ref) for k, img in (("native", nat_img), ("upscaled", up_img), ("replicated", rep_img))}
    for ctx in (low, high):
        ctx.reset_frame_index()
    return {"what": "psnr", "scene": scene, "technique": capi.TECHNIQUE_NAMES[tech], "size": size, "scale": s, "output": f"{low.width * s}x{low.height * s}",
            "reference_frames": frames, "params": "defaults", **{f"{k}_psnr_db": round(v[1], 2) for k, v in res.items()},
            **{f"{k}_mse": round(v[0], 3) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib-b", default=None, help="an alternative libfyprt.so to alternate with (A/B)")
    ap.add_argument("--label-b", default="variant")
    ap.add_argument("--psnr-frames", type=int, default=256)
    ap.add_argument("--query-calls", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "upscale" / "upscale_rate.jsonl"))
    a = ap.parse_args()
    libs = [("default", capi.load_library())]
    if a.lib_b:
        libs.append((a.label_b, capi.load_library(a.lib_b)))
    sc = scenes.hall_scene()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    def context(lib):
        ctx = capi.Context(0, lib=lib)
        ctx.resize(16, 16)
        ctx.upload_scene(sc)
        return ctx

    lows = [(label, context(lib)) for label, lib in libs]
    high = context(libs[0][1])
    for W, H, s in CASES:
        size, up = f"{W}x{H}", f"{W * s}x{H * s}"
        for _, ctx in lows:
            ctx.resize(W, H)
            ctx.set_camera(scenes.hall_camera(W, H))
        high.resize(W * s, H * s)
        cam_hi = scenes.hall_camera(W * s, H * s)
        high.set_camera(cam_hi)
        low = lows[0][1]
        for tech in (capi.RESTIR_DI, capi.RESTIR_GI):
            name = capi.TECHNIQUE_NAMES[tech]
            st = settings(tech)
            for _, ctx in lows[1:]:
                frames_ms(ctx, st, 0, 2)
            lo_ms = frames_ms(low, st, a.warmup, 20)
            hi_ms = frames_ms(high, st, a.warmup, 20)
            par = capi.UpscaleParams(scale=s)
            runs = {label: [[], [], [], []] for label, _ in lows}
            for rep in range(a.warmup + a.reps):
                for label, ctx in lows:                                # alternating, same call
                    fs = ctx.denoise_upscale(par, want_radiance=False, with_stats=True)[2]
                    if rep >= a.warmup:
                        for k in range(3):
                            runs[label][k].append(fs.kernel_ms_part[k])
                        runs[label][3].append(fs.kernel_ms)
            for label, _ in lows:
                r = runs[label]
                nbytes = 52 * W * s * H * s + 80 * W * H
                emit({"what": "upscale", "library": label, "technique": name, "size": size, "scale": s, "output": up, "reps": a.reps,
                      "launches": 1 + par.filter.spatial.iterations + 2, **spread(r[3]), "ms_lowres_stage": med(r[0]), "ms_up_primary": med(r[1]),
                      "ms_up_primary_min": round(min(r[1]), 4), "ms_up_primary_max": round(max(r[1]), 4), "ms_up_resolve": med(r[2]),
                      "ms_up_resolve_min": round(min(r[2]), 4), "ms_up_resolve_max": round(max(r[2]), 4), "resolve_compulsory_MB": round(nbytes / 1e6, 1),
                      "resolve_hbm_peak_share": round(nbytes / (statistics.median(r[2]) * 1e-3) / HBM_PEAK, 3)})
            dn = [high.denoise(want_radiance=False, with_stats=True)[2] for _ in range(a.warmup + a.reps)][a.warmup:]
            dn_ms = [x.kernel_ms for x in dn]
            native, ours = statistics.median(hi_ms) + statistics.median(dn_ms), statistics.median(lo_ms) + statistics.median(runs["default"][3])
            emit({"what": "compare", "technique": name, "size": size, "scale": s, "output": up, "ms_frame_lowres": med(lo_ms), "ms_upscale_call": med(runs["default"][3]),
                  "ms_frame_hires": med(hi_ms), "ms_denoise_hires": med(dn_ms), "ms_native_total": round(native, 4), "ms_upscaled_total": round(ours, 4),
                  "native_over_upscaled": round(native / ours, 3)})
            if tech == capi.RESTIR_DI:                                 # k_up_primary against the query + a prepare launch at the hi-res size
                d = cam_hi.ray_directions().reshape(-1, 3).astype(np.float32)
                o = np.broadcast_to(np.asarray(cam_hi.position, np.float32), d.shape).copy()
                for _ in range(2):
                    low.trace_rays(o, d, 0.0, np.inf)
                q_ms = [low.trace_rays(o, d, 0.0, np.inf, with_stats=True)[1].kernel_ms for _ in range(a.query_calls)]
                del o, d
                prep = [x.kernel_ms_part[0] for x in dn]
                pair = statistics.median(q_ms) + statistics.median(prep)
                emit({"what": "primary", "size": size, "scale": s, "output": up, "rays": W * s * H * s, "ms_up_primary": med(runs["default"][1]),
                      "ms_up_primary_min": round(min(runs["default"][1]), 4), "ms_up_primary_max": round(max(runs["default"][1]), 4),
                      "ms_query_closest": med(q_ms), "ms_query_min": round(min(q_ms), 4), "ms_query_max": round(max(q_ms), 4), "query_calls": a.query_calls,
                      "ms_dn_prepare_hires": med(prep), "ms_query_plus_prepare": round(pair, 4),
                      "up_primary_over_pair": round(statistics.median(runs["default"][1]) / pair, 3)})
            if a.psnr_frames > 1:
                emit(psnr_line(low, high, "hall_1M", tech, size, s, a.psnr_frames))
    for _, ctx in lows:
        ctx.close()
    high.close()
    if a.psnr_frames > 1:                                              # the textured scene (config 2's banana), quality only
        banana = scenes.banana_scene()
        for W, H, s in CASES:
            low, high = capi.Context(0), capi.Context(0)
            for ctx, k in ((low, 1), (high, s)):
                ctx.resize(W * k, H * k)
                ctx.upload_scene(banana)
                ctx.set_camera(scenes.banana_camera(W * k, H * k))
            emit(psnr_line(low, high, "banana", capi.RESTIR_DI, f"{W}x{H}", s, a.psnr_frames))
            low.close()
            high.close()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
