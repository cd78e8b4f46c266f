"""What the blocking denoiser calls of a context report (fyprt_denoise, fyprt_denoise_temporal, fyprt_denoise_upscale): the number of
kernels launched, which kernel_ms_part entries are used, and kernel_ms as their sum — and that every device form (the *_tensor calls)
writes the blocking form's bits.  One table of calls on the Cornell box, NEE, at 33 x 17: odd in both dimensions and smaller than one
tile of the step-16 and step-32 iteration kernels.
Launches (include/fyprt.h): spatial 1 + iterations, + 1 finish kernel without an iteration; temporal 2 + iterations, + 1 finish kernel
without an iteration, + 1 for the moved flags while a geometry edit is pending in motion mode; upscale the low-res stage without a
finish kernel + 2.  Parts: spatial prepare | iterations or finish; temporal prepare | moved flags + reprojection | iterations or finish;
upscale low-res stage | hi-res primary rays | resolve.
The device forms run on a twin context that is given the same frames, edits and calls, so both see the same history."""
import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 33, 17
MOVED_MESH = 5
CALLS = {"spatial": ("denoise", capi.DenoiseParams, 2), "temporal": ("denoise_temporal", capi.TemporalParams, 3),
         "upscale": ("denoise_upscale", capi.UpscaleParams, 3)}


class Twins:
    """A context for the blocking calls and, with `tensor`, a second one for the device forms; everything but the calls goes to both."""
    def __init__(self, lib, tensor, motion=False):
        self.sc = SCENES["cornell"][0]()
        self.mgr = self.sc.manager()
        self.mgr.perform_all_scene_updates(self.sc)
        self.ctxs = [capi.Context(0, lib=lib) for _ in range(2 if tensor else 1)]
        for c in self.ctxs:
            c.resize(W, H)
            c.upload_scene(self.sc)
            c.set_object_vertices(self.sc)
            c.set_camera(SCENES["cornell"][1](W, H))
            if motion:
                c.denoise_temporal_set_motion(True)
        self.seed = 0
        self.frame()

    def frame(self):
        self.seed += 1
        for c in self.ctxs:
            c.render(settings_for(capi.NEE, rand_seed=self.seed))

    def reset(self):
        for c in self.ctxs:
            c.denoise_temporal_reset()

    def move_mesh(self):
        pos = self.sc.mesh_transforms[MOVED_MESH]["pos"]
        self.mgr.set_mesh_transform(self.sc, MOVED_MESH, pos=(F(pos[0]) + F(0.02), F(pos[1]), F(pos[2]) + F(0.01)))
        self.mgr.perform_all_scene_updates(self.sc)
        for c in self.ctxs:
            c.update_transforms(self.sc, [MOVED_MESH])

    def call(self, name, kind, launches, **par):
        """One call of `kind` with the parameters `par`, checked; returns what the comparison with another library needs."""
        method, params, parts = CALLS[kind]
        p = params(**par)
        img, rad, st = getattr(self.ctxs[0], method)(p, with_stats=True)
        ms = [F(st.kernel_ms_part[k]) for k in range(4)]
        print(f"{name}: launches {st.launches}, kernel_ms {st.kernel_ms!r}, parts {ms}")
        assert st.launches == launches, name
        assert all(ms[k] > 0 for k in range(parts)) and all(ms[k] == 0 for k in range(parts, 4)), (name, ms)
        total = F(0)
        for k in range(parts):
            total = F(total + ms[k])
        assert F(st.kernel_ms) == total, (name, st.kernel_ms, ms)
        if len(self.ctxs) > 1:
            import torch
            img_t = torch.empty(img.shape, dtype=torch.int32, device="cuda:0")
            rad_t = torch.empty(rad.shape, dtype=torch.float32, device="cuda:0")
            getattr(self.ctxs[1], method + "_tensor")(img_t, rad_t, p)
            assert (img_t.cpu().numpy().view(np.uint32) == img).all() and bits_equal(rad_t.cpu().numpy(), rad).all(), name
        return name, int(st.launches), tuple(m > 0 for m in ms), img, rad

    def close(self):
        for c in self.ctxs:
            c.close()


def run_table(lib=None, tensor=False):
    """Every case of the table on library `lib`; returns [(case, launches, parts used, image, radiance), ...]."""
    out = []
    t = Twins(lib, tensor)
    for it in (0, 1, 3):
        out.append(t.call(f"spatial, {it} iterations", "spatial", 1 + it + (it == 0), iterations=it))
    for s in (2, 3):
        for it in (0, 2):
            out.append(t.call(f"upscale x{s}, spatial, {it} iterations", "upscale", 1 + it + 2, scale=s, iterations=it))
    for it in (0, 2):
        t.reset()
        for state in ("first call", "with history"):
            out.append(t.call(f"temporal, {it} iterations, {state}", "temporal", 2 + it + (it == 0), iterations=it))
    for s in (2, 3):
        for it in (0, 2):
            out.append(t.call(f"upscale x{s}, temporal, {it} iterations", "upscale", 2 + it + 2, scale=s, temporal=1, iterations=it))
    t.close()
    m = Twins(lib, tensor, motion=True)
    out.append(m.call("motion, first call", "temporal", 2 + 2, iterations=2))
    m.move_mesh()
    m.frame()
    out.append(m.call("motion, edit pending", "temporal", 2 + 2 + 1, iterations=2))
    out.append(m.call("motion, the call after", "temporal", 2 + 2, iterations=2))
    m.move_mesh()
    m.frame()
    out.append(m.call("motion, edit pending, upscale x2", "upscale", 2 + 2 + 1 + 2, scale=2, temporal=1, iterations=2))
    m.close()
    return out


def test_launch_counts_and_parts():
    assert len(run_table()) == 19


def test_device_forms_write_the_blocking_bits():
    """The table again with the twin context, in a fresh process that initialises torch's CUDA before the library is loaded
    (tests/test_gpu_query.py explains why)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_denoise_counts as t; "
            "t.run_table(tensor=True); print('device forms ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
