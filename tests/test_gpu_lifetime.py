"""Nothing a context allocates outlives it: fyprt_live_device_bytes — the library's own count of the device bytes its buffers hold, so
the answer does not depend on what else runs on the card — returns to where it was after a context (or a group of them) that has been
through every call that allocates is closed, after a second resize, and after an upload that failed half-way."""
import gc

import numpy as np
import pytest

from common import SCENES, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _base():
    gc.collect()                                             # contexts other tests dropped without close() go first
    return capi.live_device_bytes()


def test_a_context_that_used_everything_frees_everything():
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    base = _base()
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    for tech in (capi.RESTIR_DI, capi.RESTIR_GI, capi.NEE):
        ctx.render(settings_for(tech))
    assert capi.live_device_bytes() - base >= W * H * 16     # the counter counts: at least the accumulation buffer
    ctx.update_vertices(sc)
    ctx.set_object_vertices(sc)
    mgr.set_mesh_transform(sc, 5, pos=(0.2, 0.0, 0.1), rotation=(0, 30, 0))
    mgr.perform_all_scene_updates(sc)
    ctx.update_transforms(sc, [5])
    for builder in (1, 2):                                   # the device builders' scratch (LBVH, PLOC)
        ctx.set_tuning(12, builder)
        ctx.upload_scene(sc)
    rng = np.random.default_rng(1)
    o = np.tile(np.asarray(cam.position, dtype=np.float32), (256, 1))
    d = rng.normal(size=(256, 3)).astype(np.float32)
    ctx.trace_rays(o, d)
    ctx.render_rays(o, d, settings_for(capi.NEE))
    ctx.render(settings_for(capi.NEE))
    ctx.denoise()
    ctx.denoise_temporal()
    img, _ = ctx.readback()
    ctx.compare_image(img)
    ctx.resize(W + 16, H + 16)                               # drops the denoiser groups ...
    ctx.set_camera(mk_cam(W + 16, H + 16))
    ctx.render(settings_for(capi.NEE))
    ctx.denoise()                                            # ... and these grow them again
    ctx.denoise_temporal()
    ctx.close()
    assert capi.live_device_bytes() == base


def test_a_group_of_two_contexts_frees_everything():
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    base = _base()
    ctxs = []
    for _ in range(2):
        c = capi.Context(0)
        c.resize(W, H)
        c.upload_scene(sc)
        c.set_camera(cam)
        ctxs.append(c)
    grp = capi.Group(ctxs, [0, H // 2, H])
    grp.render(settings_for(capi.RESTIR_DI))
    grp.synchronize()
    grp.close()
    for c in ctxs:
        c.close()
    assert capi.live_device_bytes() == base


def test_a_failed_upload_frees_everything():
    mk_scene, _ = SCENES["cornell"]
    bad = mk_scene()
    bad.triangles = bad.triangles.copy()
    bad.triangles["v0"][3] = 10_000                          # vertex index out of range: FYPRT_EINVAL
    base = _base()
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(mk_scene())
    with pytest.raises(capi.FyprtError, match="out of range"):
        ctx.upload_scene(bad)
    ctx.close()
    assert capi.live_device_bytes() == base
