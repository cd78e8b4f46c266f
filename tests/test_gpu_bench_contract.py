"""bench.py's output contract (the driver parses it): ONE JSON line on stdout with the agreed keys, `value` consistent with
`ms_per_step`; with --full a roofline object whose fraction cannot exceed 1 and a CPU baseline; without it none of that, and
--dump-outputs holds the frame of the last timed step — run here on a small frame of the small hall so that it takes seconds (the
real sizes are bench.py's defaults)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from common import bits_equal
from fypraytracer_amd import capi, scenes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_bench_prints_one_json_line_with_the_contract_keys():
    env = dict(os.environ, OMP_NUM_THREADS="8")
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--scene", "hall_small", "--width", "256", "--height", "144", "--steps", "4", "--warmup", "2",
                        "--cpu-frames", "1", "--full"], capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    b = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in b, k
    assert b["n_gpus"] == 1 and b["steps"] == 4 and b["warmup"] == 2 and b["higher_is_better"] is True and b["vs_baseline"] is None
    assert b["unit"] == "Mrays/s" and b["dtype"] == "f32" and b["data"] == "synthetic" and "workload" in b["config"] and "model" not in b["config"]
    assert b["value"] > 0 and b["ms_per_step"] > 0
    rays = b["config"].get("rays_per_frame") or b.get("rays_per_frame")
    if rays:                                                                 # value = rays of a frame / time of a frame
        assert abs(b["value"] - rays / b["ms_per_step"] / 1e3) <= 0.02 * b["value"]
    r = b["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and 0.0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = b["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == b["unit"]


def test_plain_run_is_lean_and_dumps_the_last_timed_frame(tmp_path):
    """Without --full: the headline keys only (no CPU leg, no roofline), `steps` timed steps, and --dump-outputs writes the image and
    the accumulation of the last timed step — equal, bit for bit, to the same warmup + steps frames rendered one by one."""
    W, H, warm, steps = 256, 144, 2, 3
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--scene", "hall_small", "--width", str(W), "--height", str(H), "--steps", str(steps),
                        "--warmup", str(warm), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    b = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in b, k
    assert b["steps"] == steps and b["warmup"] == warm and b["value"] > 0 and b["ms_per_step"] > 0
    assert abs(b["value"] - b["config"]["rays_per_frame"] / b["ms_per_step"] / 1e3) <= 0.02 * b["value"]
    for k in ("roofline", "cpu_baseline", "parity_vs_cpu_baseline", "kernel_ms_sum_per_frame"):
        assert k not in b, k
    img, acc = np.load(out / "image.npy"), np.load(out / "accumulation.npy")
    assert img.dtype == np.float32 and img.shape == (H, W, 4) and acc.dtype == np.float32 and acc.shape == (H * W, 4)
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(scenes.hall_scene_small())
    ctx.set_camera(scenes.hall_camera(W, H))
    st = capi.Settings(technique=capi.RESTIR_DI, light_bounces=1, sample_count=1, sky_color=(0.0, 0.0, 0.0), light_candidate_count=4,
                       use_temporal_reuse=1, use_spatial_reuse=1, temporal_history_limit=2, spatial_neighbor_num=5, spatial_neighbor_radius=30)
    for f in range(warm + steps):
        st.rand_seed = f + 1
        ctx.render(st)
    ref_img, ref_acc = ctx.readback()
    ctx.close()
    assert np.array_equal(img, ref_img.view(np.uint8).reshape(H, W, 4).astype(np.float32))
    assert bits_equal(acc, ref_acc.reshape(-1, 4)).all()
