"""The upscaler (fyprt_denoise_upscale) without a GPU: declarations and defaults, the argument / state errors of both entry points on a
host-only context in the contract's order, and the numpy restatement of the resolve (tests/upscale_ref.py) on frames of the CPU oracle —
aligned pixels are the denoiser's output, a constant colour stays constant, tap order and weights on a hand-made 2 x 2 frame, and the
sliver scene of the GPU suite really takes the two rare branches."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for
from denoise_ref import DEFAULTS, assert_numpy_keeps_subnormals, denoise_ref, guides_from_scene
from fypraytracer_amd import capi
from oraclelib import Oracle
from upscale_ref import (ALIGNED, BILINEAR, NO_TAP, PASS_THROUGH, WEIGHTED, hires_from_payload, lowres_colour, sliver_camera, sliver_scene,
                         upscale_ref)

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
HEADER = Path(__file__).resolve().parent.parent / "include" / "fyprt.h"
F = np.float32
SKY = (0.1, 0.2, 0.3)


def test_upscale_symbols_struct_and_defaults():
    lib = capi.load_library()
    names = {"fyprt_upscale_default_params", "fyprt_denoise_upscale", "fyprt_denoise_upscale_device"}
    assert names <= set(capi.EXPORTED_SYMBOLS)
    text = HEADER.read_text()
    for n in names:
        assert hasattr(lib, n) and re.search(r"int %s\(" % n, text)
    assert re.search(r"FYPRT_BUF_UPSCALE_GUIDE = 11\b", text) and capi.BUF_UPSCALE_GUIDE == 11
    assert re.search(r"FYPRT_BUF_UPSCALE_ALBEDO = 12\b", text) and capi.BUF_UPSCALE_ALBEDO == 12
    assert capi.BUFFER_DTYPES[capi.BUF_UPSCALE_GUIDE].itemsize == 32 and capi.BUFFER_DTYPES[capi.BUF_UPSCALE_ALBEDO].itemsize == 16
    assert C.sizeof(capi.UpscaleParams) == 44
    p = capi.UpscaleParams(scale=4, temporal=1, iterations=0, history_limit=7, feedback=0)
    assert (p.scale, p.temporal, p.filter.spatial.iterations, p.filter.history_limit, p.filter.feedback) == (4, 1, 0, 7, 0)
    assert lib.fyprt_upscale_default_params(C.byref(p)) == 0
    assert (p.scale, p.temporal) == (2, 0)
    assert bytes(p.filter) == bytes(capi.TemporalParams())            # the defaults of fyprt_denoise_temporal_default_params
    assert bytes(capi.UpscaleParams()) == bytes(p)                    # the Python defaults are the library's
    assert lib.fyprt_upscale_default_params(None) == EINVAL
    with pytest.raises(AttributeError):
        capi.UpscaleParams(no_such_field=1)


def test_upscale_errors_in_order_on_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    img = np.zeros(16, dtype=np.uint32)
    buf = np.zeros(64, dtype=np.float32)
    base = (buf.ctypes.data + 63) & ~63                      # 64-byte aligned inside `buf` (never dereferenced)
    ok = capi.UpscaleParams()

    def host(p, i=img.ctypes.data, r=base, h=None):
        return lib.fyprt_denoise_upscale(h if h is not None else ctx.h, p, i, r, None)

    def device(p, i=base, r=base + 64, h=None):
        return lib.fyprt_denoise_upscale_device(h if h is not None else ctx.h, p, i, r)

    U = capi.UpscaleParams
    bad_scale = [U(scale=0), U(scale=1), U(scale=5), U(temporal=2)]
    bad_temporal = [U(history_limit=0), U(history_limit=257), U(feedback=2), U(normal_min=float("nan")), U(plane_max=0.0), U(plane_max=float("inf"))]
    bad_spatial = [U(iterations=9), U(normal_power_log2=8), U(demodulate_albedo=2), U(sigma_luminance=float("nan")), U(sigma_plane=0.0),
                   U(sigma_plane=float("inf"))]
    fine = [U(scale=3), U(scale=4, temporal=1), U(iterations=0, demodulate_albedo=0), U(temporal=1, history_limit=1, feedback=0)]
    assert lib.fyprt_denoise_upscale(None, ok, img.ctypes.data, None, None) == EINVAL
    assert lib.fyprt_denoise_upscale_device(None, ok, base, None) == EINVAL
    for call in (host, device):
        assert call(None) == EINVAL
        for p in bad_scale + bad_spatial:
            assert call(p) == EINVAL
            assert call(p, i=None, r=None) == EINVAL
        for p in bad_temporal:                                        # read only with temporal = 1
            assert call(p) == ESTATE
            p.temporal = 1
            assert call(p) == EINVAL
            p.temporal = 0
        assert call(ok, i=None, r=None) == EINVAL                     # both outputs NULL
        # ... then the state: a host-only context has no frame
        assert call(ok) == ESTATE
        assert call(ok, i=None) == ESTATE and call(ok, r=None) == ESTATE   # either output alone is fine
        for p in fine:
            assert call(p) == ESTATE
    # the messages name the first refusal in the contract's order: scale before the temporal parameters before the spatial ones
    # before the outputs
    def first(p, **kw):
        assert host(p, **kw) == EINVAL
        return lib.fyprt_last_error(ctx.h).decode()
    assert "scale" in first(U(scale=7, temporal=1, history_limit=0, iterations=9), i=None, r=None)
    assert "history_limit" in first(U(temporal=1, history_limit=0, iterations=9), i=None, r=None)
    assert "iterations" in first(U(temporal=1, iterations=9), i=None, r=None)
    assert "NULL" in first(U(temporal=1), i=None, r=None)
    # the device entry's alignment, refused before the state
    assert device(ok, i=base + 2) == EINVAL and device(ok, r=base + 72) == EINVAL and device(ok, r=base + 68) == EINVAL
    assert device(ok, i=base + 4, r=base + 80) == ESTATE
    ctx.upload_scene(SCENES["cornell"][0]())
    assert host(ok) == ESTATE and device(ok) == ESTATE and host(bad_scale[0]) == EINVAL
    with pytest.raises(capi.FyprtError):
        ctx.denoise_upscale()
    for b in (capi.BUF_UPSCALE_GUIDE, capi.BUF_UPSCALE_ALBEDO):
        with pytest.raises(capi.FyprtError):
            ctx.read_buffer(b)
    ctx.close()


def test_upscale_tensor_wrapper_checks_before_the_library():
    torch = pytest.importorskip("torch")
    ctx = capi.Context(-1)
    ctx.width, ctx.height = 8, 4
    with pytest.raises(ValueError):
        ctx.denoise_upscale_tensor(None, None)
    with pytest.raises(ValueError):
        ctx.denoise_upscale_tensor(torch.zeros((4, 8), dtype=torch.int32), None)           # the low-res shape
    with pytest.raises(ValueError):
        ctx.denoise_upscale_tensor(torch.zeros((8, 16), dtype=torch.float32), None)
    with pytest.raises(ValueError):
        ctx.denoise_upscale_tensor(None, torch.zeros((12, 24, 4), dtype=torch.float32))     # scale 3, params say 2
    with pytest.raises(ValueError):
        ctx.denoise_upscale_tensor(torch.zeros((8, 16), dtype=torch.int32), None)          # on the CPU, not on the context's GPU
    ctx.close()


# ---------------------------------------------------------------------------------------------- the contract on CPU-oracle frames
def _oracle_pair(sc, mk_cam, W, H, s, tech=capi.RESTIR_DI):
    """(accum, payload) of one low-res frame and the payload of the same camera description at s W x s H (ReSTIR DI: the oracle writes
    the payload there)."""
    st = settings_for(tech, sky_color=SKY, sample_count=1)
    lo = Oracle(sc, W, H)
    lo.set_camera(mk_cam(W, H))
    lo.render(st)
    acc, pay = lo.accum().copy(), lo.read_buffer(capi.BUF_PAYLOAD).reshape(H, W).copy()
    lo.close()
    hi = Oracle(sc, W * s, H * s)
    hi.set_camera(mk_cam(W * s, H * s))
    hi.render(st)
    pay_hi = hi.read_buffer(capi.BUF_PAYLOAD).reshape(H * s, W * s).copy()
    hi.close()
    return acc, pay, pay_hi


@pytest.mark.parametrize("s", [2, 3, 4])
def test_reference_aligned_pixels_and_constant_colour(oracle_built, s):
    assert_numpy_keeps_subnormals()
    W, H = 16, 12
    sc = SCENES["cornell"][0]()
    acc, pay, pay_hi = _oracle_pair(sc, SCENES["cornell"][1], W, H, s)
    # the rays of (s x, s y) are the low-res rays: so are the records
    for name in pay.dtype.names:
        assert bits_equal(pay_hi[name][::s, ::s], pay[name]).all() if pay[name].dtype.kind == "f" else (pay_hi[name][::s, ::s] == pay[name]).all(), name
    alb = guides_from_scene(sc, pay)
    g, a_hi = hires_from_payload(sc, pay_hi, SKY)
    assert bits_equal(a_hi[::s, ::s, 3], alb[..., 3]).all() and bits_equal(a_hi[::s, ::s][alb[..., 3] != 0], alb[alb[..., 3] != 0]).all()
    for par in (dict(DEFAULTS), dict(DEFAULTS, iterations=2, demodulate_albedo=0, normal_power_log2=0, sigma_plane=0.5)):
        e = lowres_colour(acc, pay, alb, 1, **par)
        want_rad, want_img = denoise_ref(acc, pay, alb, 1, **par)
        rad, img, br = upscale_ref(e, pay, alb, acc, 1, g, a_hi, s, **par)
        assert rad.shape == (H * s, W * s, 4) and img.shape == (H * s, W * s)
        assert (br[::s, ::s] == ALIGNED).all() and (br == ALIGNED).sum() == W * H
        assert bits_equal(rad[::s, ::s], want_rad).all() and (img[::s, ::s] == want_img).all()        # out[::s, ::s] is the denoiser's output
        assert {PASS_THROUGH, WEIGHTED} <= set(np.unique(br).tolist())                                # the light is seen directly; walls
        assert np.isfinite(rad).all()
        # a pass-through pixel carries the light's emission (no sky is visible inside the box)
        assert bits_equal(rad[br == PASS_THROUGH][:, :3], a_hi[br == PASS_THROUGH][:, :3]).all()
    # A constant e: E = fl(sum fl(e w)) / fl(sum w).  Not the same bits in general — each product, each of the up to three additions of
    # either sum and the division round once, all terms have one sign: |E - e| <= ((1 + u)^8 - 1) e < 8.000001 u e, u = 2^-24, as long as
    # no product underflows.  Checked on the pixels whose S is at least 2^-100 (their products are normal numbers).
    par = dict(DEFAULTS, demodulate_albedo=0)
    const = np.broadcast_to(np.array([0.3, 0.7, 1.9], dtype=F), (H, W, 3)).copy()
    rad, _, br = upscale_ref(const, pay, alb, acc, 1, g, a_hi, s, **par)
    big = upscale_ref(np.broadcast_to(np.array([1, 1, 1], dtype=F), (H, W, 3)).copy(), pay, alb, acc, 1, g, a_hi, s, **par)[0][..., 0] >= F(2.0 ** -100)
    sel = ((br == WEIGHTED) & big) | (br == BILINEAR)
    assert (br == WEIGHTED).sum() > 0 and ((br == WEIGHTED) & big).sum() > 0.9 * (br == WEIGHTED).sum()
    err = np.abs(rad[sel][:, :3].astype(np.float64) - const[0, 0].astype(np.float64)) / const[0, 0].astype(np.float64)
    exact = bits_equal(rad[sel][:, :3], np.broadcast_to(const[0, 0], rad[sel][:, :3].shape)).mean()
    print(f"scale {s}: constant colour: largest relative deviation {err.max() / 2.0 ** -24:.3f} u, {100 * exact:.1f} % of the values bit-exact")
    assert err.max() <= 8.000001 * 2.0 ** -24


def _hand_frame():
    """A 2 x 2 low-res frame on the plane z = 0 seen from z = 1 and its 4 x 4 hi-res records (scale 2), every hit on that plane."""
    pay = np.zeros((2, 2), dtype=capi.PAYLOAD_DTYPE)
    pay["hitDistance"] = 1.0
    pay["worldNormal"] = (0, 0, 1)
    pay["objectIndex"] = 0
    for y in range(2):
        for x in range(2):
            pay["worldPosition"][y, x] = (x, y, 0)
    g = np.zeros((4, 4), dtype=capi.UPSCALE_GUIDE_DTYPE)
    g["hitDistance"], g["worldNormal"], g["filterable"] = 1.0, (0, 0, 1), 1.0
    for y in range(4):
        for x in range(4):
            g["worldPosition"][y, x] = (x / 2, y / 2, 0)
    alb = np.ones((2, 2, 4), dtype=F)
    a_hi = np.ones((4, 4, 4), dtype=F)
    a_hi[..., :3] = (0.5, 0.25, 2.0)
    acc = np.zeros((2, 2, 4), dtype=F)
    acc[..., 3] = 3.0
    return pay, alb, acc, g, a_hi


def test_reference_tap_order_and_weights_by_hand():
    pay, alb, acc, g, a_hi = _hand_frame()
    # taps of Q = (1, 1): (0,0), (1,0), (0,1), (1,1), b = 1/4 each, every w_n = w_z = 1.  Values whose sum depends on the order:
    e = np.zeros((2, 2, 3), dtype=F)
    e[0, 0], e[0, 1], e[1, 0], e[1, 1] = (1e8, 1, 3), (1, 1, 5), (-1e8, 1, 7), (1, 2, 9)
    rad, _, br = upscale_ref(e, pay, alb, acc, 3, g, a_hi, 2, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1)
    q = F(0.25)
    C0 = F(F(F(F(F(0) + F(F(1e8) * q)) + F(F(1) * q)) + F(F(-1e8) * q)) + F(F(1) * q))       # in tap order: 0.25, not 0.5
    assert C0 == F(0.25)
    S = F(F(F(F(0) + q) + q) + q) + q
    assert br[1, 1] == WEIGHTED and rad[1, 1, 0] == F(F(C0 / S) * F(0.5))
    assert rad[1, 1, 1] == F(F(F(1.25) / S) * F(0.25)) and rad[1, 1, 2] == F(F(F(6) / S) * F(2))
    assert rad[1, 1, 3] == F(1.0)                                        # accum.w / n
    # Q = (1, 0): fy = 0, the lower taps have b = 0 and are not usable: the upper two alone, 1/2 each
    assert rad[0, 1, 2] == F(F(F(F(3) * F(0.5)) + F(F(5) * F(0.5))) / F(1) * F(2))
    # Q = (3, 3): x0 = y0 = 1, only tap (1, 1) is inside the image: E = e_(1,1) exactly, b = 1/4
    assert br[3, 3] == WEIGHTED and bits_equal(rad[3, 3, :3], e[1, 1] * a_hi[3, 3, :3]).all()
    # aligned pixels are out_p, here e * max(a, 1e-3) with a = 1
    assert (br[::2, ::2] == ALIGNED).all() and bits_equal(rad[::2, ::2, :3], e).all()
    # weights: tap (1, 0) on another plane (far off the tangent plane of Q) and tap (0, 1) with a perpendicular normal drop out of C / S
    pay2 = pay.copy()
    pay2["worldPosition"][0, 1] = (1, 0, 5)
    pay2["worldNormal"][1, 0] = (0, 1, 0)
    rad2, _, br2 = upscale_ref(e, pay2, alb, acc, 3, g, a_hi, 2, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=0)
    xz = F(F(5) / F(F(0.01) * F(1)))
    wz = F(F(1) / F(F(1) + F(xz * xz)))
    w1 = F(F(F(1) * wz) * q)
    S2 = F(F(F(F(F(0) + q) + w1) + F(0)) + q)
    C2 = F(F(F(F(F(0) + F(F(3) * q)) + F(F(5) * w1)) + F(F(7) * F(0))) + F(F(9) * q))
    assert br2[1, 1] == WEIGHTED and rad2[1, 1, 2] == F(C2 / S2)
    # no normal agrees: S = 0 and the plain bilinear mean of the usable taps; a tap that is not filterable is skipped in both sums
    pay3 = pay.copy()
    pay3["worldNormal"] = (0, 1, 0)
    alb3 = alb.copy()
    alb3[1, 1, 3] = 0
    rad3, _, br3 = upscale_ref(e, pay3, alb3, acc, 3, g, a_hi, 2, sigma_plane=0.01, normal_power_log2=0, demodulate_albedo=0)
    assert br3[1, 1] == BILINEAR and rad3[1, 1, 2] == F(F(F(F(F(0) + F(F(3) * q)) + F(F(5) * q)) + F(F(7) * q)) / F(F(F(F(0) + q) + q) + q))
    # nothing filterable around a filterable Q: the low-res pixel's own output; a Q that is not filterable: its pass-through colour
    alb4 = alb.copy()
    alb4[..., 3] = 0
    a_hi4 = a_hi.copy()
    a_hi4[1, 2] = (0.1, 0.2, 0.3, 0.0)
    rad4, _, br4 = upscale_ref(e, pay, alb4, acc, 3, g, a_hi4, 2, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1)
    assert br4[1, 1] == NO_TAP and bits_equal(rad4[1, 1, :3], e[0, 0]).all()
    assert br4[1, 2] == PASS_THROUGH and bits_equal(rad4[1, 2, :3], np.array([0.1, 0.2, 0.3], dtype=F)).all()


def test_sliver_scene_takes_the_two_rare_branches(oracle_built):
    """The scene the GPU suite relies on for the bilinear and the no-tap branch, confirmed with the oracle's payloads: at 16 x 16 -> 32 x 32
    no low-res pixel sees the strip, its hi-res pixels over the floor take the bilinear branch and those over the sky the no-tap one."""
    W = H = 16
    sc = sliver_scene()
    acc, pay, pay_hi = _oracle_pair(sc, sliver_camera, W, H, 2, tech=capi.RESTIR_DI)
    strip = (pay_hi["objectIndex"] == 2) | (pay_hi["objectIndex"] == 3)
    assert strip.sum() >= 16 and not ((pay["objectIndex"] == 2) | (pay["objectIndex"] == 3)).any()
    assert (np.nonzero(strip)[1] % 2 == 1).all()
    alb = guides_from_scene(sc, pay)
    g, a_hi = hires_from_payload(sc, pay_hi, SKY)
    e = lowres_colour(acc, pay, alb, 1, **DEFAULTS)
    rad, _, br = upscale_ref(e, pay, alb, acc, 1, g, a_hi, 2, **DEFAULTS)
    assert set(np.unique(br).tolist()) == {ALIGNED, PASS_THROUGH, WEIGHTED, BILINEAR, NO_TAP}
    assert (br[strip] == BILINEAR).sum() >= 4 and (br[strip] == NO_TAP).sum() >= 4 and set(np.unique(br[strip]).tolist()) <= {BILINEAR, NO_TAP}
    assert bits_equal(rad[br == NO_TAP][:, :3], np.broadcast_to(np.array(SKY, dtype=F), ((br == NO_TAP).sum(), 3))).all()     # the sky behind it, as sampled
    assert np.isfinite(rad).all()
