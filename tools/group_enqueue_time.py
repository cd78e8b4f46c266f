#!/usr/bin/env python3
"""Host time of one fyprt_group_denoise_device / fyprt_group_denoise_temporal_device call, GPU.  Either returns when everything is
enqueued, so the wall time of a batch of calls is what the host spends per call (the band schedule of fyprt_multi.h: events, waits, peer
copies, launches) — what a change to the host side of the group denoisers moves, without the noise of bands sharing one device.
The Cornell box at 1920x1080 (the scene does not matter to the calls), NEE, 2, 4 and 8 even bands on GPU 0, default parameters,
history_rows 32, the RGBA8 output alone, written into member 0's image buffer.  With --lib-b both libraries run in one process, round
by round with the order swapped; per round 10 calls of each kind, then a group synchronise; two rounds of warm-up.  One JSON line per
library, call and split: median, minimum and maximum of the rounds, in microseconds per call.
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
for n in (2, 4, 8):
    bounds = [round(H * k / n) for k in range(n + 1)]
    rigs = []
    for label, lib in libs:
        ctxs = []
        for _ in range(n):
            c = capi.Context(0, lib=lib); c.resize(W, H); c.upload_scene(sc); c.set_camera(cam); ctxs.append(c)
        grp = capi.Group(ctxs, bounds, halo_mode=0)
        st.rand_seed = 1
        grp.render(st); grp.synchronize()
        rigs.append((label, lib, ctxs, grp))
    sp, tp = capi.DenoiseParams(), capi.TemporalParams()
    res = {label: {"spatial": [], "temporal": []} for label, _ in libs}
    for rnd in range(WARMUP + a.rounds):
        for label, lib, ctxs, grp in (rigs if rnd % 2 == 0 else rigs[::-1]):
            ptr = C.c_void_p(ctxs[0].image_device_ptr())
            for what in ("spatial", "temporal"):
                t0 = time.perf_counter()
                for _ in range(10):
                    rc = lib.fyprt_group_denoise_device(grp.h, C.byref(sp), 0, ptr, None) if what == "spatial" else \
                         lib.fyprt_group_denoise_temporal_device(grp.h, C.byref(tp), 32, 0, ptr, None)
                    assert rc == 0, rc
                t1 = time.perf_counter()
                grp.synchronize()
                if rnd >= WARMUP:
                    res[label][what].append((t1 - t0) * 1e5)      # us per call
    for label, _ in libs:
        for what in ("spatial", "temporal"):
            v = res[label][what]
            line = {"what": "host time of one group device call", "library": label, "call": what, "bands": n, "size": "1920x1080", "rounds": len(v), "calls_per_round": 10,
                    "us_per_call_median": round(statistics.median(v), 1), "us_per_call_min": round(min(v), 1), "us_per_call_max": round(max(v), 1)}
            out.append(line); print(json.dumps(line), flush=True)
    for _, _, ctxs, grp in rigs:
        grp.close()
        for c in ctxs:
            c.close()
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in out))
