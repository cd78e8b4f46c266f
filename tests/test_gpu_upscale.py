"""The upscaler (fyprt_denoise_upscale / _device) on the GPU against the numpy restatement of its contract (tests/upscale_ref.py), fed with
the context's own low-res buffers (accumulation, payload, albedo, frame index) and its two hi-res buffers.  "Equal" is bitwise (NaN-aware)
on every pixel of radiance4 and rgba8: scenes x techniques x scales on frame 1 and on an accumulation, a parameter sweep, sizes off the
tile, the hi-res buffers against a context that renders at the hi-res size, the aligned identity, the temporal mode beside
fyprt_denoise_temporal (camera and object motion), every branch of the resolve, the camera / sky snapshot, and the state."""
import numpy as np
import pytest

import oraclelib
from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import assert_numpy_keeps_subnormals, oracle_texture_sampler
from fypraytracer_amd import capi
from temporal_motion_ref import temporal_motion_ref
from temporal_ref import DEFAULTS as T_DEFAULTS, camera_matrix
from upscale_ref import (ALIGNED, BILINEAR, BRANCH_NAMES, NO_TAP, PASS_THROUGH, SPATIAL_KEYS, WEIGHTED, _predemodulated, hires_from_payload,
                         lowres_colour, lowres_colour_temporal, sliver_camera, sliver_scene, upscale_ref)

pytestmark = pytest.mark.gpu
F = np.float32
S_DEFAULTS = {k: T_DEFAULTS[k] for k in SPATIAL_KEYS}
# tests/test_gpu_moving_camera.py's MOVES: (keys held, mouse delta in pixels) per frame
MOVES = [("", (0.0, 0.0)), ("W", (60.0, -25.0)), ("DE", (-140.0, 40.0)), ("S", (90.0, 70.0)), ("AQ", (-35.0, -110.0)), ("W", (20.0, 10.0))]


def _context(scene_name, W, H, sc=None, cam=None):
    mk_scene, mk_cam = SCENES[scene_name]
    sc = sc if sc is not None else mk_scene()
    cam = cam if cam is not None else mk_cam(W, H)
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    return ctx, sc, cam


def _frame(ctx, st, seed):
    """Renders one frame; returns the frame index it was rendered with."""
    n = ctx.frame_index
    st.rand_seed = seed
    ctx.render(st)
    return n


def _lowres(ctx):
    H, W = ctx.height, ctx.width
    return (ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4), ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W),
            ctx.read_buffer(capi.BUF_ALBEDO).reshape(H, W, 4))


def _hires(ctx, s):
    H, W = ctx.height * s, ctx.width * s
    return ctx.read_buffer(capi.BUF_UPSCALE_GUIDE).reshape(H, W), ctx.read_buffer(capi.BUF_UPSCALE_ALBEDO).reshape(H, W, 4)


def _same(what, rad, img, want_rad, want_img):
    eq = bits_equal(rad, want_rad)
    assert eq.all(), f"{what}: {(~eq).sum()} of {eq.size} radiance values differ, first at {np.argwhere(~eq)[:3].tolist()}"
    assert (img == want_img).all(), f"{what}: {(img != want_img).sum()} packed pixels differ"


def _check(ctx, n, s, what="", **kw):
    """fyprt_denoise_upscale (temporal = 0) at scale s with spatial parameters kw == upscale_ref on the context's own buffers, every pixel
    of both outputs.  Returns (image, radiance, branch map)."""
    par = dict(S_DEFAULTS)
    par.update(kw)
    img, rad = ctx.denoise_upscale(capi.UpscaleParams(scale=s, **par))
    assert img.shape == (ctx.height * s, ctx.width * s) and rad.shape == img.shape + (4,)
    acc, pay, alb = _lowres(ctx)
    g, a_hi = _hires(ctx, s)
    e = lowres_colour(acc, pay, alb, n, **par)
    want_rad, want_img, br = upscale_ref(e, pay, alb, acc, n, g, a_hi, s, **par)
    _same(f"{what} scale {s} {par}", rad, img, want_rad, want_img)
    return img, rad, br


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("tech", [capi.COSINE_WEIGHTED_SAMPLING, capi.NEE, capi.RESTIR_DI])
@pytest.mark.parametrize("scene_name", ["cornell", "hall_small", "banana"])
def test_upscale_equals_the_contract(scene_name, tech, s):
    """Frame 1 and an accumulation of 4 frames; default parameters; 48 x 32."""
    assert_numpy_keeps_subnormals()
    ctx, _, _ = _context(scene_name, 48, 32)
    st = settings_for(tech)
    n = _frame(ctx, st, 1)
    assert n == 1
    _, rad, br = _check(ctx, n, s, f"{scene_name} tech {tech} frame 1")
    assert (br == WEIGHTED).any() and (br == ALIGNED).sum() == 48 * 32
    assert np.isfinite(rad).all()
    for f in range(1, 4):
        n = _frame(ctx, st, f + 1)
    assert n == 4
    _check(ctx, n, s, f"{scene_name} tech {tech} 4 frames")
    ctx.close()


def test_upscale_parameter_sweep():
    assert_numpy_keeps_subnormals()
    ctx, _, _ = _context("hall_small", 48, 32)
    n = _frame(ctx, settings_for(capi.RESTIR_DI), 1)
    k = 0
    for it in (0, 1, 5):
        for dm in (0, 1):
            for npl in (0, 7):
                for sp in (1e-4, 0.5):
                    _check(ctx, n, 2 + k % 3, "sweep", iterations=it, demodulate_albedo=dm, normal_power_log2=npl, sigma_plane=sp)
                    k += 1
    ctx.close()


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("size", [(37, 23), (24, 20), (16, 16), (33, 5)])
def test_upscale_sizes_off_the_tile(size, s):
    """The last low-res row and column have no right / lower tap; the hi-res sizes are no multiple of the 16 x 16 tile."""
    scene_name, tech = {(37, 23): ("cornell", capi.NEE), (24, 20): ("banana", capi.RESTIR_DI), (16, 16): ("hall_small", capi.COSINE_WEIGHTED_SAMPLING),
                        (33, 5): ("cornell", capi.RESTIR_DI)}[size]
    ctx, _, _ = _context(scene_name, *size)
    n = _frame(ctx, settings_for(tech), 1)
    _check(ctx, n, s, f"{scene_name} {size}")
    _check(ctx, n, s, f"{scene_name} {size}", iterations=2, demodulate_albedo=0, normal_power_log2=0)
    ctx.close()


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("scene_name", ["cornell", "hall_small", "banana"])
def test_hires_buffers_are_a_hires_frames_records(scene_name, s, oracle_built):
    """FYPRT_BUF_UPSCALE_GUIDE / _ALBEDO against a second context resized to sW x sH with the same scene and the same camera description
    except the viewport, which renders one frame of technique 0: its payload gives the guide records bit for bit and, through
    guides_from_scene plus sky / emission for the pass-through pixels, the albedo; the records at [::s, ::s] are the low-res payload's."""
    W, H = 48, 32
    ctx, sc, cam = _context(scene_name, W, H)
    st = settings_for(capi.RESTIR_DI)
    _frame(ctx, st, 1)
    ctx.denoise_upscale(capi.UpscaleParams(scale=s, iterations=1))
    g, a_hi = _hires(ctx, s)
    pay = ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    cam.width, cam.height = W * s, H * s                               # the same matrices and position, another viewport
    big, _, _ = _context(scene_name, W * s, H * s, sc, cam)
    _frame(big, settings_for(0), 1)
    pay_hi = big.read_buffer(capi.BUF_PAYLOAD).reshape(H * s, W * s)
    big.close()
    ctx.close()
    want_g, want_a = hires_from_payload(sc, pay_hi, tuple(st.sky_color), oracle_texture_sampler(oraclelib.lib()))
    for name in g.dtype.names:
        eq = bits_equal(g[name], want_g[name])
        assert eq.all(), f"guide field {name}: {(~eq).sum()} of {eq.size} values differ, first at {np.argwhere(~eq)[:3].tolist()}"
    eq = bits_equal(a_hi, want_a)
    assert eq.all(), f"albedo: {(~eq).sum()} of {eq.size} values differ, first at {np.argwhere(~eq)[:3].tolist()}"
    assert set(np.unique(a_hi[..., 3]).tolist()) <= {0.0, 1.0} and (a_hi[..., 3] != 0).any()
    lo = g[::s, ::s]
    assert bits_equal(lo["worldPosition"], pay["worldPosition"]).all() and bits_equal(lo["hitDistance"], pay["hitDistance"]).all()
    assert bits_equal(lo["worldNormal"], pay["worldNormal"]).all()
    if scene_name == "banana":
        mats = sc.materials_array()
        flt = a_hi[..., 3] != 0
        textured = (mats["isUseAlbedoMap"][sc.triangles["materialIndex"][np.where(flt, pay_hi["objectIndex"], 0)]] != 0) & flt
        assert textured.sum() > 50 and len(np.unique(a_hi[textured][:, :3], axis=0)) > 10      # really sampled at the hi-res size
    if scene_name == "cornell":
        em = (a_hi[..., 3] == 0) & (pay_hi["objectIndex"] >= 0)
        assert em.any() and bits_equal(a_hi[em][:, :3], np.broadcast_to(F(40.0), (em.sum(), 3))).all()    # the light's emission


@pytest.mark.parametrize("s", [2, 3, 4])
def test_aligned_pixels_are_the_denoisers_output(s):
    ctx, _, _ = _context("hall_small", 48, 32)
    st = settings_for(capi.RESTIR_DI)
    for f in range(2):
        _frame(ctx, st, f + 1)
    for kw in (dict(), dict(iterations=0), dict(iterations=3, demodulate_albedo=0, sigma_luminance=1.0)):
        par = dict(S_DEFAULTS, **kw)
        img, rad = ctx.denoise_upscale(capi.UpscaleParams(scale=s, **par))
        d_img, d_rad = ctx.denoise(capi.DenoiseParams(**par))
        assert bits_equal(rad[::s, ::s], d_rad).all() and (img[::s, ::s] == d_img).all(), kw
        only_img, none = ctx.denoise_upscale(capi.UpscaleParams(scale=s, **par), want_radiance=False)
        assert none is None and (only_img == img).all()
    ctx.close()


def _temporal_par(**kw):
    par = dict(T_DEFAULTS)
    par.update(kw)
    return par


def test_temporal_mode_beside_the_temporal_denoiser():
    """An 8-frame moving-camera sequence of one-sample frames on two contexts: one calls denoise_temporal, the other
    denoise_upscale(temporal = 1) every frame.  FYPRT_BUF_TEMPORAL and the aligned output pixels are equal after every frame; the whole
    output equals upscale_ref (e from temporal_ref continued from the history of the frame before) on frames 1, 2 and 8."""
    assert_numpy_keeps_subnormals()
    W, H, s = 48, 32, 2
    par = _temporal_par()
    a, _, cam_a = _context("hall_small", W, H)
    b, _, cam_b = _context("hall_small", W, H)
    st = settings_for(capi.RESTIR_DI, sample_count=1)
    st.to_accumulate = 0
    hist, M_prev = None, None
    for f in range(8):
        for ctx, cam in ((a, cam_a), (b, cam_b)):
            cam.on_update(0.05, *MOVES[f % len(MOVES)])
            ctx.set_camera(cam)
            n = _frame(ctx, st, f + 1)
        M = camera_matrix(cam_b)
        cam_a.commit_frame()
        cam_b.commit_frame()
        t_img, t_rad = a.denoise_temporal(capi.TemporalParams(**par))
        img, rad, stats = b.denoise_upscale(capi.UpscaleParams(scale=s, temporal=1, **par), with_stats=True)
        assert stats.launches == 2 + par["iterations"] + 2
        rec_a, rec_b = a.read_buffer(capi.BUF_TEMPORAL), b.read_buffer(capi.BUF_TEMPORAL)
        assert struct_equal(rec_a, rec_b).all(), f"frame {f + 1}: the histories differ"
        assert bits_equal(rad[::s, ::s], t_rad).all() and (img[::s, ::s] == t_img).all(), f"frame {f + 1}: aligned pixels"
        if f in (0, 1, 7):
            acc, pay, alb = _lowres(b)
            g, a_hi = _hires(b, s)
            e, new = lowres_colour_temporal(acc, pay, alb, n, M_prev, hist, **par)
            assert struct_equal(new.ravel(), rec_b).all()
            want_rad, want_img, _ = upscale_ref(e, pay, alb, acc, n, g, a_hi, s, **par)
            _same(f"temporal frame {f + 1}", rad, img, want_rad, want_img)
        hist, M_prev = rec_b.reshape(H, W), M
    assert (hist["N"] > 2).any()                                        # a history was really carried along
    a.close()
    b.close()


def test_temporal_mode_with_object_motion():
    """The same with object motion on and a dragged mesh (cornell, meshes 5 and 6 edited before every frame, moving camera)."""
    from test_gpu_temporal_motion import Rig
    assert_numpy_keeps_subnormals()
    W, H, s = 48, 32, 3
    par = _temporal_par()
    ra, rb = Rig("cornell", W, H), Rig("cornell", W, H)
    st = settings_for(capi.RESTIR_DI, sample_count=1)
    st.to_accumulate = 0
    hist, M_prev, verts_prev = None, None, None
    for f in range(8):
        for rig in (ra, rb):
            rig.edit()
            n, M = rig.frame(st, MOVES[f % len(MOVES)])
        t_img, t_rad = ra.ctx.denoise_temporal(capi.TemporalParams(**par))
        img, rad = rb.ctx.denoise_upscale(capi.UpscaleParams(scale=s, temporal=1, **par))
        rec_a, rec_b = ra.ctx.read_buffer(capi.BUF_TEMPORAL), rb.ctx.read_buffer(capi.BUF_TEMPORAL)
        assert struct_equal(rec_a, rec_b).all(), f"frame {f + 1}: the histories differ"
        assert bits_equal(rad[::s, ::s], t_rad).all() and (img[::s, ::s] == t_img).all(), f"frame {f + 1}: aligned pixels"
        if f in (0, 1, 7):
            acc, pay, alb = _lowres(rb.ctx)
            g, a_hi = _hires(rb.ctx, s)
            r, _, new = temporal_motion_ref(_predemodulated(acc, alb, n, 1), pay, alb, 1, M_prev, hist, rb.sc.triangles, rb.verts,
                                            verts_prev if hist is not None else None, **dict(par, demodulate_albedo=0))
            assert struct_equal(new.ravel(), rec_b).all()
            want_rad, want_img, _ = upscale_ref(r[..., :3], pay, alb, acc, n, g, a_hi, s, **par)
            _same(f"object motion frame {f + 1}", rad, img, want_rad, want_img)
        hist, M_prev, verts_prev = rec_b.reshape(H, W), M, rb.verts
    on = rb.on_meshes(pay["objectIndex"], [5, 6]) & (hist["filterable"] != 0)
    assert on.any() and (hist["N"][on] > 2).any()                       # the dragged meshes kept a history
    ra.close()
    rb.close()


def test_every_branch_runs():
    """The sliver scene (tests/upscale_ref.py; test_upscale_cpu.py confirms it with the oracle's payloads): a strip that only hi-res pixels
    between the sample positions see, in front of a floor whose normal is perpendicular to its own (S = 0: the bilinear branch) and in
    front of the sky (no usable tap).  Together with the aligned, pass-through and S > 0 pixels of the same frame: all five."""
    assert_numpy_keeps_subnormals()
    W = H = 16
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(sliver_scene())
    ctx.set_camera(sliver_camera(W, H))
    seen = set()
    for tech in (capi.COSINE_WEIGHTED_SAMPLING, capi.RESTIR_DI):
        ctx.reset_frame_index()
        n = _frame(ctx, settings_for(tech), 1)
        for kw in (dict(), dict(demodulate_albedo=0, normal_power_log2=0)):
            _, rad, br = _check(ctx, n, 2, f"sliver tech {tech}", **kw)
            counts = {BRANCH_NAMES[k]: int((br == k).sum()) for k in range(5)}
            print(f"sliver tech {tech} {kw}: {counts}")
            assert min(counts.values()) >= 4, counts
            assert np.isfinite(rad).all()
            seen |= set(np.unique(br).tolist())
    assert seen == {ALIGNED, PASS_THROUGH, WEIGHTED, BILINEAR, NO_TAP}
    ctx.close()


def test_camera_and_sky_are_the_frames():
    """A set_camera between frame and call changes nothing: the hi-res rays are the enqueued frame's."""
    W, H, s = 48, 32, 2
    ctx, _, cam = _context("cornell", W, H)
    twin, _, _ = _context("cornell", W, H)
    st = settings_for(capi.NEE, sky_color=(0.7, 0.1, 0.4))
    for c in (ctx, twin):
        _frame(c, st, 1)
    cam.on_update(0.05, *MOVES[2])
    ctx.set_camera(cam)                                                # after the frame, before the call
    img, rad = ctx.denoise_upscale(capi.UpscaleParams(scale=s))
    t_img, t_rad = twin.denoise_upscale(capi.UpscaleParams(scale=s))
    assert bits_equal(rad, t_rad).all() and (img == t_img).all()
    for x, y in zip(_hires(ctx, s), _hires(twin, s)):
        assert (struct_equal(x.ravel(), y.ravel()) if x.dtype.names else bits_equal(x, y)).all()
    ctx.close()
    twin.close()


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
    """Accumulation, image, payload, depth, normals, reservoirs, frame index and timings stay; the frames rendered afterwards are a
    twin's that never called (ReSTIR DI pipelined over its streams, key 11 = 1)."""
    W, H = 48, 32
    ctx, _, _ = _context("hall_small", W, H)
    twin, _, _ = _context("hall_small", W, H)
    st = settings_for(tech)
    for c in (ctx, twin):
        c.set_tuning(11, 1)
        for f in range(2):
            _frame(c, st, f + 1)
    before = _state(ctx)
    ctx.denoise_upscale()
    ctx.denoise_upscale(capi.UpscaleParams(scale=3, temporal=1, iterations=2, demodulate_albedo=0))
    _same_state(before, _state(ctx))
    for f in range(2, 4):
        for c in (ctx, twin):
            st.rand_seed = f + 1
            c.render_async(st)
        ctx.denoise_upscale(capi.UpscaleParams(scale=4), want_radiance=False)
    _same_state(_state(ctx), _state(twin), timings=False)
    ctx.close()
    twin.close()


def test_spatial_mode_leaves_the_history_alone():
    W, H = 48, 32
    ctx, _, _ = _context("hall_small", W, H)
    twin, _, _ = _context("hall_small", W, H)
    st = settings_for(capi.RESTIR_DI)
    outs = []
    for c in (ctx, twin):
        _frame(c, st, 1)
        c.denoise_temporal()
        rec = c.read_buffer(capi.BUF_TEMPORAL)
        if c is ctx:
            c.denoise_upscale(capi.UpscaleParams(scale=2, temporal=0))
            assert struct_equal(c.read_buffer(capi.BUF_TEMPORAL), rec).all()
        _frame(c, st, 2)
        if c is ctx:
            c.denoise_upscale(capi.UpscaleParams(scale=3, temporal=0, iterations=1))
        outs.append(c.denoise_temporal() + (c.read_buffer(capi.BUF_TEMPORAL),))
    assert (outs[0][0] == outs[1][0]).all() and bits_equal(outs[0][1], outs[1][1]).all() and struct_equal(outs[0][2], outs[1][2]).all()
    ctx.close()
    twin.close()


def test_state_errors_buffers_and_memory():
    start = capi.live_device_bytes()
    W, H = 48, 32
    ctx, sc, _ = _context("cornell", W, H)
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise_upscale()                                          # no frame yet
    st = settings_for(capi.NEE)
    n = _frame(ctx, st, 1)
    for b in (capi.BUF_UPSCALE_GUIDE, capi.BUF_UPSCALE_ALBEDO):
        with pytest.raises(capi.FyprtError, match="UPSCALE"):
            ctx.read_buffer(b)                                         # written by a call
    with pytest.raises(capi.FyprtError, match="scale"):
        ctx.denoise_upscale(capi.UpscaleParams(scale=5))
    base = capi.live_device_bytes()
    _check(ctx, n, 2, "first")
    px = W * H
    assert capi.live_device_bytes() - base == px * 80 + 4 * px * (48 + 20)       # the denoiser's guide 32 + albedo 16 + two colours 32, the hi-res 48, the staging 20
    _check(ctx, n, 3, "another scale")
    assert capi.live_device_bytes() - base == px * 80 + 9 * px * (48 + 20)       # reallocated, not added
    ctx.denoise_upscale(capi.UpscaleParams(scale=4), want_radiance=False)
    assert capi.live_device_bytes() - base == px * 80 + 16 * px * (48 + 4)
    _check(ctx, n, 2, "the first scale again")
    ctx.resize(W, H)                                                   # drops the denoiser's and the upscaler's buffers
    assert capi.live_device_bytes() == base
    for b in (capi.BUF_UPSCALE_GUIDE, capi.BUF_UPSCALE_ALBEDO):
        with pytest.raises(capi.FyprtError, match="UPSCALE"):
            ctx.read_buffer(b)
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise_upscale()
    n = _frame(ctx, st, 1)
    _check(ctx, n, 3, "after resize")
    ctx.update_vertices(sc)                                            # a geometry update invalidates the frame
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise_upscale()
    n = _frame(ctx, st, 2)
    ctx.set_rows(0, 16)                                                # a band
    with pytest.raises(capi.FyprtError, match="every row"):
        ctx.denoise_upscale()
    ctx.set_rows(0, H)
    ctx.set_row_stripes(8, 2, 0)                                       # stripes
    with pytest.raises(capi.FyprtError, match="every row"):
        ctx.denoise_upscale()
    ctx.set_row_stripes(0)
    _check(ctx, n, 2, "whole frame again")
    ctx.close()
    assert capi.live_device_bytes() == start


def test_part_one_pending_is_refused():
    ctx, _, _ = _context("cornell", 48, 32)
    st = settings_for(capi.RESTIR_DI)
    _frame(ctx, st, 1)
    ctx.render_part(st, 1)
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise_upscale()
    ctx.render_part(st, 2)
    ctx.synchronize()
    ctx.denoise_upscale()
    ctx.close()


def test_torch_path_with_two_scales_back_to_back():
    """In a fresh process that initialises torch's CUDA before the library is loaded (tests/test_gpu_query.py explains why)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_upscale as t; "
            "t._torch_checks(); print('torch path ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_checks():
    import torch
    W, H = 48, 32
    ctx, _, _ = _context("hall_small", W, H)
    ctx.set_tuning(11, 1)
    st = settings_for(capi.RESTIR_DI)
    outs = []
    for f in range(2):
        st.rand_seed = f + 1
        ctx.render_async(st)
        frame_outs = []
        for s in (2, 3):                                                 # back to back, never synchronised by the host
            img_t = torch.empty((H * s, W * s), dtype=torch.int32, device="cuda:0")
            rad_t = torch.empty((H * s, W * s, 4), dtype=torch.float32, device="cuda:0")
            ctx.denoise_upscale_tensor(img_t, rad_t, capi.UpscaleParams(scale=s, iterations=3))
            frame_outs.append((img_t, rad_t * 1.0))
        outs.append(frame_outs)
    only = torch.empty((H * 3, W * 3, 4), dtype=torch.float32, device="cuda:0")
    ctx.denoise_upscale_tensor(None, only, capi.UpscaleParams(scale=3, iterations=3))
    async_state = _state(ctx)
    g3 = _hires(ctx, 3)
    ref, _, _ = _context("hall_small", W, H)
    ref.set_tuning(11, 1)
    for f in range(2):
        st.rand_seed = f + 1
        ref.render(st)
        for k, s in enumerate((2, 3)):
            img, rad = ref.denoise_upscale(capi.UpscaleParams(scale=s, iterations=3))
            assert (outs[f][k][0].cpu().numpy().view(np.uint32) == img).all(), (f, s)
            assert bits_equal(outs[f][k][1].cpu().numpy(), rad).all(), (f, s)
    assert bits_equal(only.cpu().numpy(), rad).all()
    for x, y in zip(g3, _hires(ref, 3)):
        assert (struct_equal(x.ravel(), y.ravel()) if x.dtype.names else bits_equal(x, y)).all()
    _same_state(async_state, _state(ref), timings=False)
    with pytest.raises(ValueError):
        ctx.denoise_upscale_tensor(torch.empty((H, W), dtype=torch.int32, device="cuda:0"), None)
    ctx.close()
    ref.close()
