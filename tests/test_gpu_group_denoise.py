"""fyprt_group_denoise / fyprt_group_denoise_device: the denoiser on the row bands of a group, every pixel filtered by the context
that owns its row, the rows either side pulled from their owners.  The contract is fyprt_denoise's for a single context holding the
same frame, so every comparison is bitwise (NaN-aware): against the numpy restatement (tests/denoise_ref.py) fed with the bands'
accumulation, payload and albedo rows stitched together, and against Context.denoise of a single context rendering the same sequence.
The box has one GPU: the contexts share device 0, as in tests/test_gpu_group.py."""
import ctypes as C
import gc

import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import DEFAULTS, assert_numpy_keeps_subnormals, denoise_ref
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
TWO, FIVE = [0, 96, 192], [0, 40, 70, 150, 192]          # FIVE: the 30-row band makes band 0's step-16 halo (32 rows) span two owners


def _contexts(n, scene_name, W, H, sc=None):
    mk_scene, mk_cam = SCENES[scene_name]
    sc = sc if sc is not None else mk_scene()
    cam = mk_cam(W, H)
    out = []
    for _ in range(n):
        c = capi.Context(0)
        c.resize(W, H)
        c.upload_scene(sc)
        c.set_camera(cam)
        out.append(c)
    return out, sc


def _group(scene_name, W, H, bounds, halo_mode):
    ctxs, _ = _contexts(len(bounds) - 1, scene_name, W, H)
    return capi.Group(ctxs, bounds, halo_mode=halo_mode), ctxs


def _close(grp, ctxs):
    grp.close()
    for c in ctxs:
        c.close()


def _stitched(ctxs, bounds, which):
    """Buffer `which` of the frame: every band's rows from the context that owns them."""
    H, W = ctxs[0].height, ctxs[0].width
    out = None
    for c, b, e in zip(ctxs, bounds, bounds[1:]):
        a = c.read_buffer(which)
        a = a.reshape(H, W, -1) if a.dtype.names is None and a.size != H * W else a.reshape(H, W)
        if out is None:
            out = np.zeros_like(a)
        out[b:e] = a[b:e]
    return out


def _eq(x, y):
    """Bitwise, NaN-aware equality of two buffers (plain or structured), per element / record."""
    return struct_equal(x.reshape(-1), y.reshape(-1)) if x.dtype.names else bits_equal(x, y)


def _same(got, want, what):
    img, rad = got
    want_img, want_rad = want
    if rad is not None and want_rad is not None:
        eq = bits_equal(rad, want_rad)
        assert eq.all(), f"{what}: {(~eq).sum()} of {eq.size} radiance values differ, first at {np.argwhere(~eq)[:3].tolist()}"
    if img is not None and want_img is not None:
        ne = img != want_img
        assert not ne.any(), f"{what}: {ne.sum()} packed pixels differ, rows {sorted(set(np.argwhere(ne)[:, 0].tolist()))[:8]}"


def _contract(ctxs, bounds, n, par, frame=None):
    """denoise_ref on the stitched frame -> (image, radiance).  `frame`: (accum, payload) stitched earlier (no call moves them)."""
    acc, pay = frame if frame is not None else (_stitched(ctxs, bounds, capi.BUF_ACCUM), _stitched(ctxs, bounds, capi.BUF_PAYLOAD))
    alb = _stitched(ctxs, bounds, capi.BUF_ALBEDO)
    rad, img = denoise_ref(acc, pay, alb, n, **par)
    return img, rad


def _check(grp, ctxs, bounds, n, what, frame=None, **kw):
    par = dict(DEFAULTS)
    par.update(kw)
    got = grp.denoise(capi.DenoiseParams(**par))
    _same(got, _contract(ctxs, bounds, n, par, frame), f"{what} {kw}")
    return got


_single_cache = {}


def _single(tech, frames):
    """Context.denoise (defaults) after every frame of a single context on hall_small 160 x 192; computed once per technique."""
    if tech not in _single_cache:
        (ctx,), _ = _contexts(1, "hall_small", 160, 192)
        st = settings_for(tech)
        outs = []
        for f in range(frames):
            st.rand_seed = f + 1
            ctx.render(st)
            outs.append(ctx.denoise())
        ctx.close()
        _single_cache[tech] = outs
    return _single_cache[tech]


# ------------------------------------------------------------------------------------------------ 1. the contract and the single context
@pytest.mark.parametrize("bounds", [TWO, FIVE])
@pytest.mark.parametrize("tech,halo_mode,frames", [(capi.RESTIR_DI, 1, 3), (capi.RESTIR_GI, 1, 3), (capi.NEE, 0, 2), (capi.COSINE_WEIGHTED_SAMPLING, 0, 2)])
def test_group_denoise_equals_the_contract_and_the_single_context(tech, halo_mode, frames, bounds):
    assert_numpy_keeps_subnormals()
    single = _single(tech, 3)
    grp, ctxs = _group("hall_small", 160, 192, bounds, halo_mode)
    st = settings_for(tech)
    for f in range(frames):
        st.rand_seed = f + 1
        grp.render(st)
        got = _check(grp, ctxs, bounds, f + 1, f"tech {tech} bands {bounds} frame {f + 1}")
        _same(got, single[f], f"tech {tech} bands {bounds} frame {f + 1} against the single context")
    alb = _stitched(ctxs, bounds, capi.BUF_ALBEDO)
    assert (alb[..., 3] != 0).any()                                  # something was filtered
    _close(grp, ctxs)


# ------------------------------------------------------------------------------------------------ 2. every kernel form
@pytest.fixture(scope="module")
def hall_five():
    grp, ctxs = _group("hall_small", 160, 192, FIVE, 1)
    grp.render(settings_for(capi.RESTIR_DI))
    grp.synchronize()
    frame = (_stitched(ctxs, FIVE, capi.BUF_ACCUM), _stitched(ctxs, FIVE, capi.BUF_PAYLOAD))
    yield grp, ctxs, frame
    _close(grp, ctxs)


@pytest.mark.parametrize("iterations", range(9))
def test_iteration_sweep(hall_five, iterations):
    """0: k_dn_finish alone; 1..6: the staged steps 1..32; 7, 8: the gather form at steps 64 and 128, whose halos (up to 256 rows)
    clip at the image and cross every band."""
    grp, ctxs, frame = hall_five
    _check(grp, ctxs, FIVE, 1, "sweep", frame, iterations=iterations)
    if iterations in (3, 6):
        _check(grp, ctxs, FIVE, 1, "sweep", frame, iterations=iterations, demodulate_albedo=0)
        for sl in (0.0, 16.0):
            _check(grp, ctxs, FIVE, 1, "sweep", frame, iterations=iterations, sigma_luminance=sl)


# ------------------------------------------------------------------------------------------------ 3. windows that can go wrong
@pytest.mark.parametrize("scene_name,W,H,bounds", [
    ("hall_small", 160, 192, [0, 1, 2, 95, 96, 192]),            # one-row bands at the image edge and mid-image
    ("cornell", 97, 61, [0, 1, 17, 18, 61]),                     # off every tile size
    ("banana", 33, 5, [0, 2, 5]),                                # textures
])
def test_band_windows(scene_name, W, H, bounds):
    grp, ctxs = _group(scene_name, W, H, bounds, 0)
    grp.render(settings_for(capi.NEE))
    grp.synchronize()
    frame = (_stitched(ctxs, bounds, capi.BUF_ACCUM), _stitched(ctxs, bounds, capi.BUF_PAYLOAD))
    for it in (0, 1, 2, 3, 6):
        _check(grp, ctxs, bounds, 1, f"{scene_name} {bounds}", frame, iterations=it)
    _close(grp, ctxs)


# ------------------------------------------------------------------------------------------------ 4. roots and outputs (torch)
def test_roots_outputs_and_the_device_entry():
    """In a fresh process that initialises torch's CUDA before the library is loaded (tests/test_gpu_query.py explains why)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_group_denoise as t; "
            "t._torch_checks(); print('group torch path ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "group torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _frame_state(ctxs, bounds):
    return [_stitched(ctxs, bounds, b) for b in (capi.BUF_ACCUM, capi.BUF_IMAGE, capi.BUF_PAYLOAD)]


def _torch_checks():
    import torch
    W, H, bounds = 160, 192, FIVE
    par_a = dict(DEFAULTS, iterations=4, sigma_luminance=2.0)
    par_b = dict(DEFAULTS, iterations=2, demodulate_albedo=0)
    grp, ctxs = _group("hall_small", W, H, bounds, 1)
    plain, pctxs = _group("hall_small", W, H, bounds, 1)             # the same frames without any call
    st = settings_for(capi.RESTIR_DI)

    def tensors():
        return torch.empty((H, W), dtype=torch.int32, device="cuda:0"), torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")

    def host(t):
        return None if t is None else (t.cpu().numpy().view(np.uint32) if t.dtype == torch.int32 else t.cpu().numpy())

    st.rand_seed = 1
    grp.render(st)
    plain.render(st)
    # two device calls with different parameters back to back, a root other than 0, no host wait in between; then the next frame
    img_a, rad_a = tensors()
    img_b, rad_b = tensors()
    grp.denoise_tensor(img_a, rad_a, capi.DenoiseParams(**par_a), root=2)
    grp.denoise_tensor(img_b, rad_b, capi.DenoiseParams(**par_b), root=1)
    st.rand_seed = 2
    grp.render(st)
    plain.render(st)
    img_c, rad_c = tensors()
    grp.denoise_tensor(img_c, rad_c, capi.DenoiseParams(**par_a), root=0)      # frame 2, straight after the render
    only_img, _ = tensors()
    _, only_rad = tensors()
    grp.denoise_tensor(only_img, None, capi.DenoiseParams(**par_b), root=3)
    grp.denoise_tensor(None, only_rad, capi.DenoiseParams(**par_b), root=3)
    got_a, got_b, got_c = (host(img_a), host(rad_a)), (host(img_b), host(rad_b)), (host(img_c), host(rad_c))
    got_only = (host(only_img), host(only_rad))
    grp.synchronize()
    # frame 2 is what it is without the calls, and its denoised outputs equal the host entry and the contract
    for x, y in zip(_frame_state(ctxs, bounds), _frame_state(pctxs, bounds)):
        assert _eq(x, y).all()
    _same(got_c, grp.denoise(capi.DenoiseParams(**par_a)), "device entry, frame 2")
    _same(got_c, _contract(ctxs, bounds, 2, par_a), "device entry, frame 2, contract")
    want_b2 = grp.denoise(capi.DenoiseParams(**par_b))
    _same(got_only, want_b2, "image only / radiance only")
    img_only, none = grp.denoise(capi.DenoiseParams(**par_b), want_radiance=False)
    assert none is None
    _same((img_only, None), want_b2, "host entry, image only")
    rad_only = np.empty((H * W, 4), np.float32)
    p = capi.DenoiseParams(**par_b)
    grp._check(grp.lib.fyprt_group_denoise(grp.h, C.byref(p), None, rad_only.ctypes.data_as(C.c_void_p), None))
    _same((None, rad_only.reshape(H, W, 4)), want_b2, "host entry, radiance only")
    # frame 1's calls: against a group that stops at frame 1
    one, octxs = _group("hall_small", W, H, bounds, 1)
    st.rand_seed = 1
    one.render(st)
    _same(got_a, one.denoise(capi.DenoiseParams(**par_a)), "first of two device calls")
    _same(got_a, _contract(octxs, bounds, 1, par_a), "first of two device calls, contract")
    _same(got_b, one.denoise(capi.DenoiseParams(**par_b)), "second of two device calls")
    _same(got_b, _contract(octxs, bounds, 1, par_b), "second of two device calls, contract")
    with pytest.raises(ValueError):
        grp.denoise_tensor(torch.empty((H, W), dtype=torch.float32, device="cuda:0"), None)
    with pytest.raises(ValueError):
        grp.denoise_tensor(img_a, None, root=4)
    for g, cs in ((grp, ctxs), (plain, pctxs), (one, octxs)):
        _close(g, cs)


# ------------------------------------------------------------------------------------------------ 5. no frame state moves
def _member_state(c):
    c.synchronize()
    return [c.read_buffer(b) for b in range(9)], c.frame_index


@pytest.mark.parametrize("tech", [capi.RESTIR_DI, capi.RESTIR_GI])
def test_no_frame_state_moves_and_the_sequence_is_the_sequence_without_the_calls(tech):
    """Per member: accumulation, image, payload, depth, normals, the ReSTIR buffers and frame index before and after a call (the frame
    timings: test_buffers_are_counted...; a member of an exchange-mode frame, rendered in two parts, has none to read).  Then
    six frames in halo mode 1 with a call after every frame against the same six frames without, the borders moved after frame 3
    (fyprt_balance_rows + Group.set_rows): the frames are equal frame by frame, and the call after the move is still exact."""
    bounds = list(TWO)
    grp, ctxs = _group("hall_small", 160, 192, bounds, 1)
    plain, pctxs = _group("hall_small", 160, 192, bounds, 1)
    st = settings_for(tech)
    for f in range(6):
        st.rand_seed = f + 1
        grp.render(st)
        plain.render(st)
        if f == 1:
            before = [_member_state(c) for c in ctxs]
            grp.denoise()
            grp.denoise(capi.DenoiseParams(iterations=2, demodulate_albedo=0))
            for (a, ia), (b, ib) in zip(before, [_member_state(c) for c in ctxs]):
                for k, (x, y) in enumerate(zip(a, b)):
                    assert _eq(x, y).all(), f"buffer {k} moved"
                assert ia == ib
        _check(grp, ctxs, bounds, f + 1, f"tech {tech} frame {f + 1} bands {bounds}", iterations=3 + (f % 3))
        for k, (x, y) in enumerate(zip(_frame_state(ctxs, bounds), _frame_state(pctxs, bounds))):
            assert _eq(x, y).all(), f"frame {f + 1}: buffer {k} differs from the sequence without calls"
        if f == 2:
            bounds = capi.balance_rows(bounds, [2.0, 1.0], min_rows=16, max_shift=24)
            assert 72 <= bounds[1] < 96
            grp.set_rows(bounds)
            plain.set_rows(bounds)
    _close(grp, ctxs)
    _close(plain, pctxs)


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors():
    W, H, bounds = 96, 64, [0, 20, 64]
    ctxs, sc = _contexts(2, "cornell", W, H)
    grp = capi.Group(ctxs, bounds, halo_mode=0)
    lib, p = grp.lib, capi.DenoiseParams()
    img = np.empty(W * H, np.uint32)
    out = img.ctypes.data_as(C.c_void_p)
    dev = C.c_void_p(ctxs[0].image_device_ptr())                         # a device address for the refused device calls (never written)

    def rc(params=p, rgba8=out, radiance4=None):
        return lib.fyprt_group_denoise(grp.h, C.byref(params) if params is not None else None, rgba8, radiance4, None)

    assert rc() == ESTATE                                                # before any frame
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        grp.denoise()
    # the argument errors come first, with or without a frame
    for _ in range(2):
        assert rc(params=None) == EINVAL
        assert rc(params=capi.DenoiseParams(iterations=9)) == EINVAL
        assert rc(params=capi.DenoiseParams(sigma_plane=0.0)) == EINVAL
        assert lib.fyprt_group_denoise_device(grp.h, C.byref(p), 2, dev, None) == EINVAL     # root out of range
        assert lib.fyprt_group_denoise_device(grp.h, C.byref(p), -1, dev, None) == EINVAL
        assert lib.fyprt_group_denoise_device(grp.h, C.byref(p), 0, C.c_void_p(dev.value + 2), None) == EINVAL   # misaligned
        assert lib.fyprt_group_denoise_device(grp.h, C.byref(p), 0, None, C.c_void_p(dev.value + 4)) == EINVAL
        assert rc(rgba8=None) == EINVAL                                  # both outputs NULL
        assert lib.fyprt_group_denoise_device(grp.h, C.byref(p), 0, None, None) == EINVAL
        grp.render(settings_for(capi.NEE))
    _check(grp, ctxs, bounds, 2, "valid")
    ctxs[1].update_materials(sc)                                         # one member's frame no longer matches its materials
    assert rc() == ESTATE
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        grp.denoise()
    grp.render(settings_for(capi.NEE))
    _check(grp, ctxs, bounds, 3, "after the next frame")
    ctxs[0].set_rows(0, 10)                                              # rows moved behind the group
    with pytest.raises(capi.FyprtError, match="not its band"):
        grp.denoise()
    ctxs[0].set_rows(0, 20)
    grp.denoise()
    with pytest.raises(capi.FyprtError, match="every row"):
        ctxs[0].denoise()                                                # a member on its own stays refused
    ctxs[1].render(settings_for(capi.NEE))                               # one member a frame ahead
    with pytest.raises(capi.FyprtError, match="frame index"):
        grp.denoise()
    grp.set_interleave(16)
    for c in ctxs:
        c.reset_frame_index()
    grp.render(settings_for(capi.COSINE_WEIGHTED_SAMPLING))
    assert rc() == ESTATE
    with pytest.raises(capi.FyprtError, match="striped"):
        grp.denoise()
    grp.set_interleave(0)
    for c in ctxs:
        c.reset_frame_index()
    grp.render(settings_for(capi.COSINE_WEIGHTED_SAMPLING))
    _check(grp, ctxs, bounds, 1, "contiguous bands again")
    _close(grp, ctxs)


# ------------------------------------------------------------------------------------------------ 7. lifetime
def test_buffers_are_counted_dropped_by_resize_and_freed():
    gc.collect()
    base = capi.live_device_bytes()
    W, H, bounds = 96, 64, [0, 20, 41, 64]
    grp, ctxs = _group("cornell", W, H, bounds, 0)
    st = settings_for(capi.NEE)
    grp.render(st)
    grp.synchronize()
    rendered = capi.live_device_bytes()
    timings = [c.frame_timings() for c in ctxs]
    grp.denoise()
    used = capi.live_device_bytes()
    assert [c.frame_timings() for c in ctxs] == timings               # the members' frame timings are not touched
    # per member guide + albedo + two colour buffers (80 B per pixel); root 0 stages the frame, the others their band's rows (20 B per pixel)
    assert used - rendered == 3 * 80 * W * H + 20 * W * H + 20 * W * (H - 20)
    grp.denoise(capi.DenoiseParams(iterations=2), want_radiance=False)
    assert capi.live_device_bytes() == used                              # allocated once
    grp.synchronize()
    for c in ctxs:
        c.resize(W, H)
    assert capi.live_device_bytes() == rendered                          # resize drops them
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        grp.denoise()
    grp.render(st)
    _check(grp, ctxs, bounds, 1, "after resize")
    assert capi.live_device_bytes() == used
    one, octxs = _group("cornell", W, H, [0, H], 0)                      # a one-member group equals fyprt_denoise
    one.render(st)
    got = one.denoise()
    one.close()
    octxs[0].set_rows(0, H)
    _same(got, octxs[0].denoise(), "one-member group")
    octxs[0].close()
    _close(grp, ctxs)
    gc.collect()
    assert capi.live_device_bytes() == base
