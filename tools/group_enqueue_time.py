#!/usr/bin/env python3
"""Host time of one device call of the denoisers, GPU: fyprt_denoise_device, fyprt_denoise_temporal_device and
fyprt_denoise_upscale_device on one context ("bands": 1), and their fyprt_group_* counterparts on 2, 4 and 8 even bands on GPU 0.  Each
returns when everything is enqueued, so the wall time of a batch of calls is what the host spends per call (building the filter's list
of steps, and for a group the band schedule of fyprt_multi.h: events, waits, peer copies, launches) — what a change to the host side of
the denoisers moves, without the noise of bands sharing one device.
The Cornell box at 1920x1080 (the scene does not matter to the calls), NEE, default parameters (upscale: scale 2, spatial), history_rows
32, the RGBA8 output alone, written into the image buffer of a context of twice the size.  With --lib-b both libraries run in one
process, round by round with the order swapped; per round 10 calls of each kind, then a synchronise; two rounds of warm-up.  One JSON
line per library, call and split: median, minimum and maximum of the rounds, in microseconds per call.
  usage: python tools/group_enqueue_time.py [--rounds 10] [--lib-b PATH --label-b NAME] [--out profiles/denoise/group_enqueue_time.jsonl]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from fypraytracer_amd import capi, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--lib-b", default=None, help="an alternative libfyprt.so to alternate with (before / after runs)")
ap.add_argument("--label-b", default="parent commit")
ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise" / "group_enqueue_time.jsonl"))
a = ap.parse_args()
W, H, WARMUP = 1920, 1080, 2
libs = [("this change" if a.lib_b else "default", capi.load_library())]
if a.lib_b:
    libs.append((a.label_b, capi.load_library(a.lib_b)))
sc, cam = scenes.cornell_box(), scenes.cornell_camera(W, H)
st = capi.Settings(technique=capi.NEE, sky_color=(0.0, 0.0, 0.0))
out = []
KINDS = ("spatial", "temporal", "upscale")
for n in (1, 2, 4, 8):
    bounds = [round(H * k / n) for k in range(n + 1)]
    rigs = []
    for label, lib in libs:
        ctxs = []
        for _ in range(n):
            c = capi.Context(0, lib=lib); c.resize(W, H); c.upload_scene(sc); c.set_camera(cam); ctxs.append(c)
        big = capi.Context(0, lib=lib); big.resize(2 * W, 2 * H)      # its image buffer holds the upscaled frame
        grp = capi.Group(ctxs, bounds, halo_mode=0) if n > 1 else None
        st.rand_seed = 1
        if grp:
            grp.render(st); grp.synchronize()
        else:
            ctxs[0].render(st)
        rigs.append((label, lib, ctxs, grp, big))
    sp, tp, up = capi.DenoiseParams(), capi.TemporalParams(), capi.UpscaleParams()
    res = {label: {what: [] for what in KINDS} for label, _ in libs}
    for rnd in range(WARMUP + a.rounds):
        for label, lib, ctxs, grp, big in (rigs if rnd % 2 == 0 else rigs[::-1]):
            ptr, h = C.c_void_p(big.image_device_ptr()), ctxs[0].h
            calls = {"spatial": lambda: lib.fyprt_denoise_device(h, C.byref(sp), ptr, None),
                     "temporal": lambda: lib.fyprt_denoise_temporal_device(h, C.byref(tp), ptr, None),
                     "upscale": lambda: lib.fyprt_denoise_upscale_device(h, C.byref(up), ptr, None)}
            if grp:
                calls = {"spatial": lambda: lib.fyprt_group_denoise_device(grp.h, C.byref(sp), 0, ptr, None),
                         "temporal": lambda: lib.fyprt_group_denoise_temporal_device(grp.h, C.byref(tp), 32, 0, ptr, None),
                         "upscale": lambda: lib.fyprt_group_denoise_upscale_device(grp.h, C.byref(up), 32, 0, ptr, None)}
            for what in KINDS:
                t0 = time.perf_counter()
                for _ in range(10):
                    rc = calls[what]()
                    assert rc == 0, rc
                t1 = time.perf_counter()
                grp.synchronize() if grp else ctxs[0].synchronize()
                if rnd >= WARMUP:
                    res[label][what].append((t1 - t0) * 1e5)      # us per call
    for label, _ in libs:
        for what in KINDS:
            v = res[label][what]
            line = {"what": "host time of one device call", "library": label, "call": what, "bands": n, "size": "1920x1080", "rounds": len(v), "calls_per_round": 10,
                    "us_per_call_median": round(statistics.median(v), 1), "us_per_call_min": round(min(v), 1), "us_per_call_max": round(max(v), 1)}
            out.append(line); print(json.dumps(line), flush=True)
    for _, _, ctxs, grp, big in rigs:
        if grp:
            grp.close()
        for c in ctxs + [big]:
            c.close()
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in out))
