"""fyprt_group_denoise* and fyprt_group_denoise_temporal* back to back: the two calls share the group's events, the bands' staging and the
colour buffers, so a call of one enqueued behind a call of the other, with no host wait between them, has to be ordered against it by
those events alone.  The device entries, called alternately on three frames with a different root each time, are compared bitwise with
the blocking entries on the same frames (which wait for the host around every call)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from common import settings_for
from fypraytracer_amd import capi
from test_gpu_group_temporal import MOVES, Rig, _same

pytestmark = pytest.mark.gpu

W, H, BOUNDS = 97, 61, [0, 1, 17, 18, 61]      # tests/test_gpu_group_temporal.py's test_band_windows: off every tile size, one-row bands, halos with several owners
ITERATIONS, HISTORY_ROWS = 4, 16               # halo (up to 16 rows) and history window cross several bands
ROOTS = (1, 3, 0, 2, 3, 1)                     # per call, in issue order: no two in a row alike, every member at least once


def test_spatial_and_temporal_calls_back_to_back():
    """In a fresh process that initialises torch's CUDA before the library is loaded (tests/test_gpu_query.py explains why)."""
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_group_denoise_interleaved as t; "
            "t._torch_checks(); print('interleaved group denoisers ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "interleaved group denoisers ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_checks():
    import torch
    sp, tp = capi.DenoiseParams(iterations=ITERATIONS), capi.TemporalParams(iterations=ITERATIONS)
    st = settings_for(capi.NEE)
    st.to_accumulate = 0

    def tensors():
        return torch.empty((H, W), dtype=torch.int32, device="cuda:0"), torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")

    # rig A, the blocking entries: after each frame the spatial call, then the temporal one
    rig = Rig("cornell", W, H, BOUNDS, 0)
    want = []
    for f in range(3):
        rig.frame(st, MOVES[f])
        for img, rad in (rig.grp.denoise(sp), rig.grp.denoise_temporal(tp, history_rows=HISTORY_ROWS)):
            want.append((rad, img))
    want_hist = rig.stitched(capi.BUF_TEMPORAL)
    rig.close()
    # rig B, the device entries: the same frames and calls, a different root each, no host wait until everything is enqueued
    rig = Rig("cornell", W, H, BOUNDS, 0)
    outs = []
    for f in range(3):
        rig.frame(st, MOVES[f])
        img, rad = tensors()
        rig.grp.denoise_tensor(img, rad, sp, root=ROOTS[2 * f])
        outs.append((img, rad))
        img, rad = tensors()
        rig.grp.denoise_temporal_tensor(img, rad, tp, history_rows=HISTORY_ROWS, root=ROOTS[2 * f + 1])
        outs.append((img, rad))
    rig.grp.synchronize()
    assert len(set(ROOTS)) == len(BOUNDS) - 1 and all(a != b for a, b in zip(ROOTS, ROOTS[1:]))
    for k, ((img, rad), (want_rad, want_img)) in enumerate(zip(outs, want)):
        got = (rad.cpu().numpy(), img.cpu().numpy().view(np.uint32), None)
        _same(f"frame {k // 2 + 1}, {'temporal' if k % 2 else 'spatial'} call, root {ROOTS[k]}", got, (want_rad, want_img, None))
    _same("the history after the three frames", (None, None, rig.stitched(capi.BUF_TEMPORAL)), (None, None, want_hist))
    rig.close()
