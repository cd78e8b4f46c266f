"""Radiance queries (fyprt_render_rays) without a GPU: the declarations, the chunk constant, the argument / state errors of both entry
points on a host-only context in the documented order, and the Python wrappers' own checks."""
import re
from pathlib import Path

import numpy as np
import pytest

from common import SCENES
from fypraytracer_amd import capi

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
HEADER = Path(__file__).resolve().parent.parent / "include" / "fyprt.h"


def test_render_rays_symbols_and_chunk_constant():
    lib = capi.load_library()
    assert {"fyprt_render_rays", "fyprt_render_rays_device"} <= set(capi.EXPORTED_SYMBOLS)
    assert hasattr(lib, "fyprt_render_rays") and hasattr(lib, "fyprt_render_rays_device")
    text = HEADER.read_text()
    assert re.search(r"int fyprt_render_rays\(", text) and re.search(r"int fyprt_render_rays_device\(", text)
    m = re.search(r"#define FYPRT_RENDER_RAYS_CHUNK \(1u << (\d+)\)", text)
    assert m and int(m.group(1)) == 21
    assert capi.RENDER_RAYS_CHUNK == 1 << 21


def _calls(lib, ctx):
    rays = np.zeros(4, dtype=capi.RAY_DTYPE)
    rays["direction"][:, 2], rays["tmax"] = 1.0, np.inf
    rad = np.zeros((4, 4), dtype=np.float32)
    dev = np.zeros(64, dtype=np.float32)                     # (never dereferenced: every call below fails before a launch)
    base = (dev.ctypes.data + 63) & ~63                      # 64-byte aligned inside `dev`

    def host(st, f=1, r=rays.ctypes.data, n=4, o=rad.ctypes.data, h=None):
        return lib.fyprt_render_rays(h if h is not None else ctx.h, st, f, r, None, 0, n, o, None, None)

    def device(st, f=1, r=base, n=4, o=base + 64, p=None, i=None, h=None):
        return lib.fyprt_render_rays_device(h if h is not None else ctx.h, st, f, r, i, 0, n, o, p)

    return host, device, base


def test_render_rays_errors_in_order_on_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    host, device, base = _calls(lib, ctx)
    ok = capi.Settings(technique=2)                         # cosine-weighted sampling
    bad_tech = [capi.Settings(technique=t) for t in (-1, 7, 8, 9)]
    for call in (host, device):
        # FYPRT_EINVAL: NULL settings, technique outside 0..6, frame_index 0, NULL rays / radiance with count > 0 ...
        assert call(None) == EINVAL
        for st in bad_tech:
            assert call(st) == EINVAL
        assert call(bad_tech[1], f=0) == EINVAL                               # (every EINVAL case before the state)
        assert call(ok, f=0) == EINVAL
        assert call(ok, r=None) == EINVAL and call(ok, o=None) == EINVAL
        assert call(ok, r=None, n=0) == ESTATE                                # NULL arrays are fine with count 0 ...
        # ... then FYPRT_ESTATE: no scene, host-only context
        assert call(ok) == ESTATE
        assert call(ok, n=0) == ESTATE                                        # (count 0 returns OK only past the state checks)
    # the device entry's alignment: rays / radiance 16 B, payloads 8 B, indices 4 B, all refused before the state
    assert device(ok, r=base + 8) == EINVAL and device(ok, o=base + 72) == EINVAL
    assert device(ok, p=base + 4) == EINVAL and device(ok, i=base + 2) == EINVAL
    assert device(ok, p=base + 8, i=base + 4) == ESTATE                        # aligned: the state is next
    assert device(bad_tech[1], r=base + 8) == EINVAL
    ctx.upload_scene(SCENES["cornell"][0]())
    for call in (host, device):
        assert call(ok) == ESTATE                                             # a host-only context cannot render, with a scene too
        assert call(bad_tech[1]) == EINVAL and call(ok, f=0) == EINVAL
        assert call(capi.Settings(technique=5)) == ESTATE
    assert lib.fyprt_render_rays(None, ok, 1, None, None, 0, 0, None, None, None) == EINVAL
    assert lib.fyprt_render_rays_device(None, ok, 1, None, None, 0, 0, None, None) == EINVAL
    with pytest.raises(capi.FyprtError):
        ctx.render_rays(np.zeros((1, 3)), np.ones((1, 3)), ok)
    ctx.close()


def test_render_rays_wrappers_check_before_the_library():
    ctx = capi.Context(-1)                                    # no scene: a call that reached the library would raise FyprtError
    st = capi.Settings(technique=2)
    with pytest.raises(ValueError):
        ctx.render_rays(np.zeros((3, 3)), np.ones((2, 3)), st)
    with pytest.raises(ValueError):
        ctx.render_rays(np.zeros((3, 3)), np.ones((3, 3)), st, pixel_indices=[0, 1])
    with pytest.raises(ValueError):
        ctx.render_rays(np.zeros((3, 3)), np.ones((3, 3)), st, pixel_indices=np.arange(4))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        ctx.render_rays_tensor(torch.zeros((4, 8), dtype=torch.float64), st)
    with pytest.raises(ValueError):
        ctx.render_rays_tensor(torch.zeros((4, 7), dtype=torch.float32), st)
    with pytest.raises(ValueError):
        ctx.render_rays_tensor(torch.zeros((4, 8), dtype=torch.float32).t().contiguous().t(), st)
    with pytest.raises(ValueError):
        ctx.render_rays_tensor(torch.zeros((4, 8), dtype=torch.float32), st)      # on the CPU, not on the context's GPU
    ctx.close()
