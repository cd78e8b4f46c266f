"""The temporal denoiser (fyprt_denoise_temporal) without a GPU: declarations and defaults, the argument / state errors of both entry
points on a host-only context in the documented order, and the numpy restatement of the contract (tests/temporal_ref.py) on frame
sequences of the CPU oracle — determinism, pass-through, the two degenerate settings, history lengths under a static and a moving camera,
and a sanity bound on what the history buys over the spatial filter."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import assert_numpy_keeps_subnormals, denoise_ref, guides_from_scene, tonemap_pack
from fypraytracer_amd import capi
from oraclelib import Oracle
from temporal_ref import DEFAULTS, camera_matrix, matmul_cm, temporal_ref

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
HEADER = Path(__file__).resolve().parent.parent / "include" / "fyprt.h"
F = np.float32
# tests/test_gpu_moving_camera.py's MOVES: (keys held, mouse delta in pixels) per frame
MOVES = [("", (0.0, 0.0)), ("W", (60.0, -25.0)), ("DE", (-140.0, 40.0)), ("S", (90.0, 70.0)), ("AQ", (-35.0, -110.0)), ("W", (20.0, 10.0))]
NAMES = {"fyprt_denoise_temporal_default_params", "fyprt_denoise_temporal", "fyprt_denoise_temporal_device", "fyprt_denoise_temporal_reset"}


def test_temporal_symbols_struct_and_defaults():
    lib = capi.load_library()
    assert NAMES <= set(capi.EXPORTED_SYMBOLS)
    text = HEADER.read_text()
    for n in NAMES:
        assert hasattr(lib, n) and re.search(r"int %s\(" % n, text)
    assert re.search(r"FYPRT_BUF_TEMPORAL = 10\b", text) and capi.BUF_TEMPORAL == 10
    assert capi.BUFFER_DTYPES[capi.BUF_TEMPORAL].itemsize == 64
    assert C.sizeof(capi.TemporalParams) == 36
    p = capi.TemporalParams(iterations=0, sigma_luminance=0.0, sigma_plane=0.0, normal_power_log2=0, demodulate_albedo=0,
                            history_limit=0, normal_min=0.0, plane_max=0.0, feedback=0)
    assert bytes(p) == bytes(36)
    assert lib.fyprt_denoise_temporal_default_params(C.byref(p)) == 0
    s = p.spatial
    got = (s.iterations, s.sigma_luminance, s.sigma_plane, s.normal_power_log2, s.demodulate_albedo, p.history_limit, p.normal_min,
           p.plane_max, p.feedback)
    assert got == (5, 4.0, F(0.01), 6, 1, 32, F(0.9), F(0.02), 1)
    assert bytes(capi.TemporalParams()) == bytes(p)                    # the Python defaults are the library's
    assert bytes(p.spatial) == bytes(capi.DenoiseParams())             # ... and its spatial part is the spatial denoiser's
    assert DEFAULTS == dict(iterations=5, sigma_luminance=4.0, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1,
                            history_limit=32, normal_min=0.9, plane_max=0.02, feedback=1)
    assert bytes(capi.TemporalParams(**DEFAULTS)) == bytes(p)
    assert lib.fyprt_denoise_temporal_default_params(None) == EINVAL
    assert lib.fyprt_denoise_temporal_reset(None) == EINVAL
    with pytest.raises(AttributeError):
        capi.TemporalParams(no_such_field=1)


def test_temporal_errors_in_order_on_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    img = np.zeros(16, dtype=np.uint32)
    buf = np.zeros(64, dtype=np.float32)
    base = (buf.ctypes.data + 63) & ~63                      # 64-byte aligned inside `buf` (never dereferenced)
    T = capi.TemporalParams
    ok = T()

    def host(p, i=img.ctypes.data, r=base, h=None):
        return lib.fyprt_denoise_temporal(h if h is not None else ctx.h, p, i, r, None)

    def device(p, i=base, r=base + 64, h=None):
        return lib.fyprt_denoise_temporal_device(h if h is not None else ctx.h, p, i, r)

    nan, inf = float("nan"), float("inf")
    bad = [T(history_limit=0), T(history_limit=257), T(feedback=2), T(normal_min=nan), T(normal_min=inf), T(plane_max=0.0),
           T(plane_max=-1.0), T(plane_max=nan), T(plane_max=inf),
           # the spatial part's, as fyprt_denoise refuses them
           T(iterations=9), T(normal_power_log2=8), T(demodulate_albedo=2), T(sigma_luminance=nan), T(sigma_luminance=inf),
           T(sigma_plane=0.0), T(sigma_plane=-1.0), T(sigma_plane=nan), T(sigma_plane=inf)]
    fine = [T(history_limit=1), T(history_limit=256, feedback=0), T(normal_min=-1.0), T(normal_min=0.999, plane_max=10.0),
            T(iterations=8, normal_power_log2=7, demodulate_albedo=0), T(iterations=0), T(sigma_luminance=0.0), T(sigma_luminance=-3.0)]
    assert lib.fyprt_denoise_temporal(None, ok, img.ctypes.data, None, None) == EINVAL
    assert lib.fyprt_denoise_temporal_device(None, ok, base, None) == EINVAL
    for call in (host, device):
        assert call(None) == EINVAL
        for p in bad:
            assert call(p) == EINVAL
        assert call(ok, i=None, r=None) == EINVAL                     # both outputs NULL
        assert call(bad[0], i=None, r=None) == EINVAL
        assert call(ok) == ESTATE                                      # ... then the state: a host-only context has no frame
        assert call(ok, i=None) == ESTATE and call(ok, r=None) == ESTATE
        for p in fine:
            assert call(p) == ESTATE
    assert device(ok, i=base + 2) == EINVAL and device(ok, r=base + 72) == EINVAL and device(ok, r=base + 68) == EINVAL
    assert device(ok, i=base + 4, r=base + 80) == ESTATE
    ctx.upload_scene(SCENES["cornell"][0]())
    assert host(ok) == ESTATE and device(ok) == ESTATE and host(bad[0]) == EINVAL
    assert lib.fyprt_denoise_temporal_reset(ctx.h) == 0               # nothing to drop: fine
    with pytest.raises(capi.FyprtError):
        ctx.denoise_temporal()
    with pytest.raises(capi.FyprtError):
        ctx.read_buffer(capi.BUF_TEMPORAL)
    ctx.denoise_temporal_reset()
    ctx.close()


def test_temporal_tensor_wrapper_checks_before_the_library():
    torch = pytest.importorskip("torch")
    ctx = capi.Context(-1)
    ctx.width, ctx.height = 8, 4
    with pytest.raises(ValueError):
        ctx.denoise_temporal_tensor(None, None)
    with pytest.raises(ValueError):
        ctx.denoise_temporal_tensor(torch.zeros((4, 8), dtype=torch.float32), None)
    with pytest.raises(ValueError):
        ctx.denoise_temporal_tensor(torch.zeros((8, 4), dtype=torch.int32), None)
    with pytest.raises(ValueError):
        ctx.denoise_temporal_tensor(None, torch.zeros((4, 8, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        ctx.denoise_temporal_tensor(torch.zeros((4, 8), dtype=torch.int32), None)          # on the CPU, not on the context's GPU
    ctx.close()


def test_matmul_cm_is_the_column_major_product():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(16).astype(F), rng.standard_normal(16).astype(F)
    want = (a.reshape(4, 4).T.astype(np.float64) @ b.reshape(4, 4).T.astype(np.float64)).T     # [col][row] storage
    assert np.allclose(matmul_cm(a, b), want, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------- the contract on CPU-oracle sequences
@functools.lru_cache(maxsize=None)
def _oracle_sequence(scene_name, W, H, frames, moving):
    """One-sample ReSTIR DI frames (both reuses, to_accumulate = 0; its seeds move on under a static camera, unlike techniques 0-6), frame
    f rendered with rand_seed = f + 1.  Per frame: (accum, payload H x W, albedo guide, projection x view of its camera).  Moving: the
    camera takes MOVES[f] before frame f and commits after it.  Also returns the scene and the last camera."""
    sc = SCENES[scene_name][0]()
    cam = SCENES[scene_name][1](W, H)
    orc = Oracle(sc, W, H)
    st = settings_for(capi.RESTIR_DI, sky_color=(0.0, 0.0, 0.0), sample_count=1)
    st.to_accumulate = 0
    out = []
    for f in range(frames):
        if moving:
            cam.on_update(0.05, *MOVES[f % len(MOVES)])
        orc.set_camera(cam)
        st.rand_seed = f + 1
        orc.render(st)
        acc = orc.accum().copy()
        pay = orc.read_buffer(capi.BUF_PAYLOAD).reshape(H, W).copy()
        out.append((acc, pay, guides_from_scene(sc, pay), camera_matrix(cam)))
        if moving:
            cam.commit_frame()
    orc.close()
    return out, sc, cam


def _run(frames, **kw):
    """temporal_ref chained over the frames; returns the list of (radiance4, rgba8, history)."""
    hist, M, res = None, None, []
    for acc, pay, alb, pv in frames:
        rad, img, hist = temporal_ref(acc, pay, alb, 1, M, hist, **kw)
        res.append((rad, img, hist))
        M = pv
    return res


def test_reference_contract_properties(oracle_built):
    assert_numpy_keeps_subnormals()
    frames, _, _ = _oracle_sequence("cornell", 24, 20, 3, True)
    acc, pay, alb, _ = frames[0]
    flt = alb[..., 3] != 0
    assert flt.any() and (~flt).any()                                  # walls and the directly seen light
    # twice -> identical bits (6 iterations reach step 32, larger than the image), finite
    a, b = _run(frames, iterations=6), _run(frames, iterations=6)
    for (ra, ia, ha), (rb, ib, hb) in zip(a, b):
        assert bits_equal(ra, rb).all() and (ia == ib).all() and struct_equal(ha.ravel(), hb.ravel()).all()
        assert np.isfinite(ra).all() and np.isfinite(ha["variance"]).all() and (ha["variance"] >= 0).all()
    # pixels that are not filterable come back unchanged and carry no history, whatever the parameters
    for kw in (dict(DEFAULTS), dict(iterations=3, sigma_luminance=0.0, sigma_plane=0.5, normal_power_log2=0, demodulate_albedo=0, feedback=0)):
        for (acc_k, pay_k, alb_k, _), (rad, img, hist) in zip(frames, _run(frames, **kw)):
            nf = alb_k[..., 3] == 0
            c = acc_k[..., :3] / F(1)
            assert bits_equal(rad[nf][:, :3], c[nf]).all() and (rad[..., 3] == acc_k[..., 3]).all()
            assert (hist["N"][nf] == 0).all() and (hist["variance"][nf] == 0).all() and (hist["filterable"][nf] == 0).all()
            assert (hist["N"][~nf] >= 1).all() and bits_equal(hist["worldPosition"], pay_k["worldPosition"]).all()
            assert (rad[~nf][:, :3] != c[~nf]).any()
    # degenerate 1: the first call with iterations = 0, demodulate_albedo = 0 returns the frame's own radiance and image
    rad, img, hist = temporal_ref(acc, pay, alb, 1, None, None, iterations=0, demodulate_albedo=0)
    c = acc[..., :3] / F(1)
    assert bits_equal(rad[..., :3], c).all() and bits_equal(hist["colour"], c).all()
    assert (img == tonemap_pack(np.concatenate([c, acc[..., 3:]], axis=-1))).all()
    # degenerate 2: history_limit = 1 never blends — every call equals a first call on its frame
    for (acc_k, pay_k, alb_k, _), (rad, img, hist) in zip(frames, _run(frames, history_limit=1)):
        r1, i1, h1 = temporal_ref(acc_k, pay_k, alb_k, 1, None, None)
        assert bits_equal(rad, r1).all() and (img == i1).all() and struct_equal(hist.ravel(), h1.ravel()).all()
    # feedback = 0 keeps the integrated colour: with it the first call's history colour is e0, with feedback the first iteration's output
    h_fb0 = temporal_ref(acc, pay, alb, 1, None, None, feedback=0, demodulate_albedo=0)[2]
    h_fb1 = temporal_ref(acc, pay, alb, 1, None, None, feedback=1, demodulate_albedo=0)[2]
    assert bits_equal(h_fb0["colour"], c).all() and (h_fb1["colour"][flt] != c[flt]).any()
    it1 = temporal_ref(acc, pay, alb, 1, None, None, iterations=1, demodulate_albedo=0)
    assert bits_equal(it1[2]["colour"], it1[0][..., :3]).all()         # one iteration: the output is what is fed back


@pytest.mark.parametrize("limit", [32, 3])
def test_static_camera_history_length_is_the_call_number(oracle_built, limit):
    """Cornell 96 x 80, ReSTIR DI, 8 frames, static camera: N == min(k, history_limit) on every filterable pixel after call k (pixel i
    reprojects to sx = i up to rounding, and the bilinear taps do not care on which side of i it lands)."""
    frames, _, _ = _oracle_sequence("cornell", 96, 80, 8, False)
    for k, ((acc, pay, alb, _), (_, _, hist)) in enumerate(zip(frames, _run(frames, history_limit=limit)), start=1):
        flt = alb[..., 3] != 0
        assert flt.sum() > 0.5 * flt.size
        assert (hist["N"][flt] == min(k, limit)).all(), f"call {k}: {(hist['N'][flt] != min(k, limit)).sum()} filterable pixels off"
        assert (hist["N"][~flt] == 0).all()


@pytest.mark.parametrize("scene_name,size", [("cornell", (96, 80)), ("hall_small", (160, 96))])
def test_moving_camera_reuses_and_rejects(oracle_built, scene_name, size):
    """Under MOVES, calls 2..6: the share of filterable pixels with a full history (N == k) is below 1 and above 0.5 — reuse and rejection
    are both exercised; and a pixel whose reprojection leaves the viewport starts over with N = 1."""
    W, H = size
    frames, _, _ = _oracle_sequence(scene_name, W, H, 6, True)
    res = _run(frames)
    left = 0
    for k in range(2, 7):
        acc, pay, alb, _ = frames[k - 1]
        hist = res[k - 1][2]
        flt = alb[..., 3] != 0
        share = float((hist["N"][flt] == k).mean())
        print(f"{scene_name} call {k}: share of filterable pixels with N == k: {share:.4f}")
        assert 0.5 < share < 1.0
        # independent reprojection in float64 with the previous frame's matrix: pixels that land clearly (1/2 pixel) outside [-1, W) x [-1, H)
        M = frames[k - 2][3].astype(np.float64)                        # [col][row]
        P = np.concatenate([pay["worldPosition"].astype(np.float64), np.ones((H, W, 1))], axis=-1)
        clip = np.einsum("cr,hwc->hwr", M, P)
        with np.errstate(all="ignore"):
            sx = (clip[..., 0] / clip[..., 3] * 0.5 + 0.5) * W
            sy = (clip[..., 1] / clip[..., 3] * 0.5 + 0.5) * H
        outside = flt & ((clip[..., 3] < -1e-3) | ((clip[..., 3] > 1e-3) & ((sx < -1.5) | (sx > W + 0.5) | (sy < -1.5) | (sy > H + 0.5))))
        left += int(outside.sum())
        assert (hist["N"][outside] == 1).all()
    assert left > 0                                                    # the camera did turn far enough for some


def test_history_halves_the_error_of_the_spatial_filter(oracle_built):
    """Sanity bound of the specification itself, not a quality bar: Cornell 96 x 80, ReSTIR DI with both reuses, to_accumulate = 0, static
    camera, defaults: MSE(temporal call 8) <= 0.5 * MSE(denoise_ref of the same frame 8), linear radiance, against 128 accumulated frames."""
    W, H, truth_frames = 96, 80, 128
    frames, sc, cam = _oracle_sequence("cornell", W, H, 8, False)
    tr = Oracle(sc, W, H)
    tr.set_camera(cam)
    st = settings_for(capi.RESTIR_DI, sky_color=(0.0, 0.0, 0.0), sample_count=1)
    for g in range(truth_frames):
        st.rand_seed = 1000 + g
        tr.render(st)
    truth = (tr.accum()[..., :3] / F(truth_frames)).astype(np.float64)
    tr.close()
    acc, pay, alb, _ = frames[7]
    temporal = _run(frames)[7][0]
    spatial, _ = denoise_ref(acc, pay, alb, 1)

    def mse(x):
        return float(np.mean((x[..., :3].astype(np.float64) - truth) ** 2))
    raw, spa, tem = mse(acc), mse(spatial), mse(temporal)
    print(f"cornell ReSTIR DI frame 8: MSE raw {raw:.5f}, spatial {spa:.5f}, temporal {tem:.5f} (temporal / spatial {tem / spa:.3f})")
    assert np.isfinite([raw, spa, tem]).all() and spa > 0
    assert tem <= 0.5 * spa
