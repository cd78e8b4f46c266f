"""The denoiser (fyprt_denoise / fyprt_denoise_device) on the GPU against the numpy restatement of its contract (tests/denoise_ref.py),
fed with the context's own accumulation, payload, albedo and frame index.  "Equal" is bitwise (NaN-aware) on every pixel of radiance4
and rgba8: scenes x techniques x accumulation states, a parameter sweep, sizes that are no multiple of the tile, the full frame
as the band [0, H) beside a one-band group; the albedo buffer itself; the identity configuration; no frame state moves; the torch
path; the state errors; quality on the device; the 1M-triangle hall at 1920 x 1080."""
import numpy as np
import pytest

import oraclelib
from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import DEFAULTS, assert_numpy_keeps_subnormals, denoise_ref, guides_from_scene, oracle_texture_sampler
from fypraytracer_amd import capi, scenes

pytestmark = pytest.mark.gpu
F = np.float32


def _context(scene_name, W, H, sc=None):
    mk_scene, mk_cam = SCENES[scene_name]
    sc = sc if sc is not None else mk_scene()
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(mk_cam(W, H))
    return ctx, sc


def _frame(ctx, st, seed):
    """Renders one frame; returns the frame index it was rendered with."""
    n = ctx.frame_index
    st.rand_seed = seed
    ctx.render(st)
    return n


def _check(ctx, n, what="", **kw):
    """fyprt_denoise with parameters kw == denoise_ref on the context's own buffers, every pixel of both outputs."""
    H, W = ctx.height, ctx.width
    par = dict(DEFAULTS)
    par.update(kw)
    img, rad = ctx.denoise(capi.DenoiseParams(**par))
    acc = ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)
    pay = ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    alb = ctx.read_buffer(capi.BUF_ALBEDO).reshape(H, W, 4)
    want_rad, want_img = denoise_ref(acc, pay, alb, n, **par)
    eq = bits_equal(rad, want_rad)
    assert eq.all(), f"{what} {par}: {(~eq).sum()} of {eq.size} radiance values differ, first at {np.argwhere(~eq)[:3].tolist()}"
    assert (img == want_img).all(), f"{what} {par}: {(img != want_img).sum()} packed pixels differ"
    return img, rad, alb


@pytest.mark.parametrize("tech", [capi.COSINE_WEIGHTED_SAMPLING, capi.NEE, capi.RESTIR_DI, capi.RESTIR_GI])
@pytest.mark.parametrize("scene_name", ["cornell", "hall_small", "banana"])
def test_denoise_equals_the_contract(scene_name, tech):
    """Frame 1, an accumulation of 4 frames, and a to_accumulate = 0 frame; default parameters; 96 x 64."""
    assert_numpy_keeps_subnormals()
    ctx, _ = _context(scene_name, 96, 64)
    st = settings_for(tech)
    n = _frame(ctx, st, 1)
    assert n == 1
    _, rad, alb = _check(ctx, n, f"{scene_name} tech {tech} frame 1")
    assert (alb[..., 3] != 0).any()                                   # something was filtered ...
    acc = ctx.read_buffer(capi.BUF_ACCUM).reshape(64, 96, 4)
    assert (rad[..., :3] != acc[..., :3]).any()                        # ... and changed
    for f in range(1, 4):
        n = _frame(ctx, st, f + 1)
    assert n == 4
    _check(ctx, n, f"{scene_name} tech {tech} 4 frames")
    st.to_accumulate = 0
    n = _frame(ctx, st, 9)                                             # rendered with index 5 on top of the sum, as the reference does
    _check(ctx, n, f"{scene_name} tech {tech} to_accumulate 0, first")
    n = _frame(ctx, st, 10)
    assert n == 1
    _check(ctx, n, f"{scene_name} tech {tech} to_accumulate 0")
    ctx.close()


def test_denoise_parameter_sweep():
    assert_numpy_keeps_subnormals()
    ctx, _ = _context("hall_small", 96, 64)
    n = _frame(ctx, settings_for(capi.RESTIR_DI), 1)
    for it in range(7):
        for sl in (0.0, 1.0, 16.0):
            for npl in (0, 7):
                _check(ctx, n, "sweep", iterations=it, sigma_luminance=sl, normal_power_log2=npl)
        _check(ctx, n, "sweep", iterations=it, demodulate_albedo=0)
        _check(ctx, n, "sweep", iterations=it, demodulate_albedo=0, sigma_luminance=0.0, normal_power_log2=0, sigma_plane=0.5)
    _check(ctx, n, "sweep", iterations=8, sigma_plane=1e-4)
    _check(ctx, n, "sweep", sigma_luminance=-1.0)
    ctx.close()


@pytest.mark.parametrize("size", [(97, 61), (24, 20), (16, 16), (33, 5)])
@pytest.mark.parametrize("scene_name,tech", [("cornell", capi.NEE), ("banana", capi.RESTIR_DI), ("hall_small", capi.COSINE_WEIGHTED_SAMPLING)])
def test_denoise_sizes_off_the_tile(scene_name, tech, size):
    ctx, _ = _context(scene_name, *size)
    n = _frame(ctx, settings_for(tech), 1)
    for it in (0, 1, 2, 3, 6):
        _check(ctx, n, f"{scene_name} {size}", iterations=it)
    _check(ctx, n, f"{scene_name} {size}", iterations=6, sigma_luminance=1.0, normal_power_log2=7)
    _check(ctx, n, f"{scene_name} {size}", iterations=3, sigma_luminance=16.0, normal_power_log2=0, demodulate_albedo=0)
    ctx.close()


def test_full_frame_is_the_band_0_H():
    """The full frame runs the kernels as the band [0, H): cornell 97 x 61 (no multiple of any tile span), NEE, one frame, iterations
    0..8 — the finish kernel, the staged steps 1..32 and the gather form at steps 64 and 128, every one clipped by rowEnd = 61 (at step 32
    a tile spans 128 rows: its tile rows 2 and 3 lie below the image in every row phase, tile row 1 in phases 29..31).  Each equals
    denoise_ref, and a one-band group [0, 61] on the same frame gives the same bits.  (Workgroups whose first row lies below the frame
    need H mod the tile span < STEP: the 24 x 20, 16 x 16 and 33 x 5 frames of test_denoise_sizes_off_the_tile.)"""
    assert_numpy_keeps_subnormals()
    W, H = 97, 61
    ctx, sc = _context("cornell", W, H)
    member, _ = _context("cornell", W, H, sc)
    grp = capi.Group([member], [0, H])
    st = settings_for(capi.NEE)
    n = _frame(ctx, st, 1)
    grp.render(st)
    grp.synchronize()
    assert bits_equal(member.read_buffer(capi.BUF_ACCUM), ctx.read_buffer(capi.BUF_ACCUM)).all()      # the same frame
    for it in range(9):
        img, rad, _ = _check(ctx, n, "band [0, H)", iterations=it)
        g_img, g_rad = grp.denoise(capi.DenoiseParams(**dict(DEFAULTS, iterations=it)))
        assert bits_equal(g_rad, rad).all() and (g_img == img).all(), f"iterations {it}: the one-band group differs from the context"
    grp.close()
    member.close()
    ctx.close()


@pytest.mark.parametrize("scene_name", ["cornell", "hall_small", "banana"])
def test_albedo_buffer(scene_name, oracle_built):
    """FYPRT_BUF_ALBEDO: the material's albedo (the re-quantised bilinear sample of the oracle library on the textured banana), the
    flag from payload + materials, zero colour where the pixel is not filterable."""
    W, H = 96, 64
    ctx, sc = _context(scene_name, W, H)
    with pytest.raises(capi.FyprtError):
        ctx.read_buffer(capi.BUF_ALBEDO)                              # written by a denoise call
    _frame(ctx, settings_for(capi.RESTIR_DI), 1)
    ctx.denoise(capi.DenoiseParams(iterations=1))
    alb = ctx.read_buffer(capi.BUF_ALBEDO).reshape(H, W, 4)
    pay = ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    want = guides_from_scene(sc, pay, oracle_texture_sampler(oraclelib.lib()))
    assert bits_equal(alb, want).all()
    flt = alb[..., 3] != 0
    assert flt.any() and set(np.unique(alb[..., 3]).tolist()) <= {0.0, 1.0}
    assert (pay["objectIndex"][flt] >= 0).all()
    if scene_name == "banana":
        mats = sc.materials_array()
        textured = (mats["isUseAlbedoMap"][sc.triangles["materialIndex"][np.where(flt, pay["objectIndex"], 0)]] != 0) & flt
        assert textured.sum() > 50 and len(np.unique(alb[textured][:, :3], axis=0)) > 10      # really sampled, not one colour
    elif scene_name == "cornell":
        assert (~flt).any()                                            # the light is seen directly
    ctx.close()


@pytest.mark.parametrize("tech", [capi.NEE, capi.RESTIR_DI])
def test_identity_configuration_returns_the_frame(tech):
    ctx, _ = _context("cornell", 97, 61)
    st = settings_for(tech)
    for f in range(3):
        _frame(ctx, st, f + 1)
        img, rad = ctx.denoise(capi.DenoiseParams(iterations=0, demodulate_albedo=0))
        frame_img, acc = ctx.readback()
        assert (img == frame_img).all()
        assert bits_equal(rad, acc / F(f + 1)).all()
        only_img, none = ctx.denoise(capi.DenoiseParams(iterations=0, demodulate_albedo=0), want_radiance=False)
        assert none is None and (only_img == frame_img).all()
    ctx.close()


def _state(ctx):
    ctx.synchronize()
    return [ctx.read_buffer(b) for b in range(9)], ctx.frame_index, ctx.frame_timings()


def _same_state(a, b, timings=True):
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        eq = struct_equal(x, y) if x.dtype.names else bits_equal(x, y)
        assert eq.all(), f"buffer {k} differs"
    assert a[1] == b[1]
    if timings:
        assert a[2] == b[2]


@pytest.mark.parametrize("tech", [capi.COSINE_WEIGHTED_SAMPLING, capi.RESTIR_DI, capi.RESTIR_GI])
def test_no_frame_state_moves(tech):
    ctx, _ = _context("hall_small", 96, 64)
    st = settings_for(tech)
    for f in range(2):
        _frame(ctx, st, f + 1)
    before = _state(ctx)
    ctx.denoise()
    ctx.denoise(capi.DenoiseParams(iterations=2, demodulate_albedo=0))
    _same_state(before, _state(ctx))
    ctx.close()


@pytest.mark.parametrize("use_async", [False, True])
@pytest.mark.parametrize("tech", [capi.RESTIR_DI, capi.RESTIR_GI])
def test_frames_after_a_denoise_are_the_frames_without_it(tech, use_async):
    """frame, denoise, frame, denoise, frame leaves the buffers of frame, frame, frame (ReSTIR DI pipelined over two streams, key 11 = 1)."""
    results = []
    for with_denoise in (True, False):
        ctx, _ = _context("hall_small", 96, 64)
        ctx.set_tuning(11, 1)
        st = settings_for(tech)
        for f in range(3):
            st.rand_seed = f + 1
            if use_async:
                ctx.render_async(st)
            else:
                ctx.render(st)
            if with_denoise and f < 2:
                n = f + 1
                _check(ctx, n, f"tech {tech} async {use_async} frame {n}", iterations=3)
        results.append(_state(ctx))
        ctx.close()
    _same_state(results[0], results[1], timings=False)


def test_state_errors_and_resize():
    ctx, sc = _context("cornell", 96, 64)
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise()                                                  # no frame yet
    st = settings_for(capi.NEE)
    n = _frame(ctx, st, 1)
    a = _check(ctx, n, "first")
    b = _check(ctx, n, "second call, other parameters", iterations=2, sigma_luminance=1.0)
    assert (a[1] != b[1]).any()
    c = _check(ctx, n, "third call, first parameters")
    assert bits_equal(a[1], c[1]).all() and (a[0] == c[0]).all()
    ctx.update_vertices(sc)                                            # a geometry update invalidates the frame for the denoiser
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise()
    n = _frame(ctx, st, 2)
    _check(ctx, n, "after the next frame")
    ctx.set_rows(0, 32)                                                # a band
    with pytest.raises(capi.FyprtError, match="every row"):
        ctx.denoise()
    ctx.set_rows(0, 64)
    ctx.set_row_stripes(8, 2, 0)                                       # stripes
    with pytest.raises(capi.FyprtError, match="every row"):
        ctx.denoise()
    ctx.set_row_stripes(0)
    _check(ctx, n, "whole frame again")
    ctx.resize(40, 24)                                                 # another size: buffers dropped, no frame
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise()
    with pytest.raises(capi.FyprtError):
        ctx.read_buffer(capi.BUF_ALBEDO)
    ctx.set_camera(SCENES["cornell"][1](40, 24))
    n = _frame(ctx, st, 1)
    _check(ctx, n, "after resize")
    ctx.upload_scene(sc)
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise()
    ctx.close()


def test_quality_on_the_device():
    """hall_small 128 x 128, ReSTIR DI: the denoised frame 1 has at most half the raw frame's MSE (linear radiance) against the context's
    own 256-frame accumulation."""
    W = H = 128
    ctx, _ = _context("hall_small", W, H)
    st = settings_for(capi.RESTIR_DI, sky_color=(0.0, 0.0, 0.0), sample_count=1)
    _frame(ctx, st, 1)
    raw = ctx.readback()[1][..., :3].astype(np.float64)
    den = ctx.denoise()[1][..., :3].astype(np.float64)
    for f in range(1, 256):
        _frame(ctx, st, f + 1)
    ref = (ctx.readback()[1][..., :3] / F(256)).astype(np.float64)
    ctx.close()
    mse_raw, mse_den = float(np.mean((raw - ref) ** 2)), float(np.mean((den - ref) ** 2))
    print(f"hall_small ReSTIR DI: MSE raw {mse_raw:.6g} -> denoised {mse_den:.6g} (ratio {mse_den / mse_raw:.3f})")
    assert mse_raw > 0 and mse_den <= 0.5 * mse_raw


def test_hall_1m_triangles_1080p():
    """The bench workload once: defaults, ReSTIR DI.  Two calls give identical bits; rows 500..563 equal denoise_ref run on rows 436..627
    (five iterations reach 2 * 31 = 62 rows, the margin is 64; the numpy code on the full frame is too slow)."""
    W, H = 1920, 1080
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(scenes.hall_scene())
    ctx.set_camera(scenes.hall_camera(W, H))
    n = _frame(ctx, settings_for(capi.RESTIR_DI), 1)
    img, rad = ctx.denoise()
    img2, rad2 = ctx.denoise()
    assert (img == img2).all() and bits_equal(rad, rad2).all()
    acc = ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)
    pay = ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    alb = ctx.read_buffer(capi.BUF_ALBEDO).reshape(H, W, 4)
    ctx.close()
    y0, y1, m = 500, 564, 64
    want_rad, want_img = denoise_ref(acc[y0 - m:y1 + m], pay[y0 - m:y1 + m], alb[y0 - m:y1 + m], n, **DEFAULTS)
    assert bits_equal(rad[y0:y1], want_rad[m:-m]).all()
    assert (img[y0:y1] == want_img[m:-m]).all()
    assert (alb[y0:y1, :, 3] != 0).mean() > 0.5 and (rad[y0:y1, :, :3] != acc[y0:y1, :, :3]).any()


def test_torch_path_is_ordered_and_equals_the_host_entry():
    """In a fresh process that initialises torch's CUDA before the library is loaded (tests/test_gpu_query.py explains why)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_denoise as t; "
            "t._torch_checks(); print('torch path ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_checks():
    import torch
    W, H = 96, 64
    par = capi.DenoiseParams(iterations=4, sigma_luminance=2.0)
    # the device entry between asynchronous, pipelined ReSTIR DI frames, never synchronised by the host: equals the host entry after
    # each frame of a blocking sequence, and the frames are the frames without the calls
    ctx, _ = _context("hall_small", W, H)
    ctx.set_tuning(11, 1)
    st = settings_for(capi.RESTIR_DI)
    outs = []
    for f in range(3):
        st.rand_seed = f + 1
        ctx.render_async(st)
        img_t = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
        rad_t = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
        big = torch.randn(2048, 2048, device="cuda:0") @ torch.randn(2048, 2048, device="cuda:0")
        ctx.denoise_tensor(img_t, rad_t, par)
        outs.append((img_t, rad_t * 1.0))
        del big
    only = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    ctx.denoise_tensor(None, only, par)
    async_state = _state(ctx)
    ref, _ = _context("hall_small", W, H)
    ref.set_tuning(11, 1)
    for f in range(3):
        st.rand_seed = f + 1
        ref.render(st)
        img, rad = ref.denoise(par)
        assert (outs[f][0].cpu().numpy().view(np.uint32) == img).all(), f
        assert bits_equal(outs[f][1].cpu().numpy(), rad).all(), f
    assert bits_equal(only.cpu().numpy(), rad).all()
    _same_state(async_state, _state(ref), timings=False)
    plain, _ = _context("hall_small", W, H)
    plain.set_tuning(11, 1)
    for f in range(3):
        st.rand_seed = f + 1
        plain.render_async(st)
    _same_state(async_state, _state(plain), timings=False)
    with pytest.raises(ValueError):
        ctx.denoise_tensor(torch.empty((H, W), dtype=torch.float32, device="cuda:0"), None)
    for c in (ctx, ref, plain):
        c.close()
