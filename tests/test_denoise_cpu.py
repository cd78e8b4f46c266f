"""The denoiser (fyprt_denoise) without a GPU: declarations and defaults, the argument / state errors of both entry points on a host-only
context in the documented order, and the numpy restatement of the contract (tests/denoise_ref.py) on frames of the CPU oracle —
determinism, pass-through, the identity configuration, steps larger than the image, and a sanity bound on what the filter does to the
error of a one-sample frame."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for
from denoise_ref import DEFAULTS, assert_numpy_keeps_subnormals, denoise_ref, guides_from_scene, tonemap_pack
from fypraytracer_amd import capi
from oraclelib import Oracle

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
HEADER = Path(__file__).resolve().parent.parent / "include" / "fyprt.h"
F = np.float32


def test_denoise_symbols_struct_and_defaults():
    lib = capi.load_library()
    names = {"fyprt_denoise_default_params", "fyprt_denoise", "fyprt_denoise_device"}
    assert names <= set(capi.EXPORTED_SYMBOLS)
    text = HEADER.read_text()
    for n in names:
        assert hasattr(lib, n) and re.search(r"int %s\(" % n, text)
    assert re.search(r"FYPRT_BUF_ALBEDO = 9\b", text) and capi.BUF_ALBEDO == 9
    assert capi.BUFFER_DTYPES[capi.BUF_ALBEDO].itemsize == 16
    assert C.sizeof(capi.DenoiseParams) == 20
    p = capi.DenoiseParams(iterations=0, sigma_luminance=0.0, sigma_plane=0.0, normal_power_log2=0, demodulate_albedo=0)
    assert lib.fyprt_denoise_default_params(C.byref(p)) == 0
    got = (p.iterations, p.sigma_luminance, p.sigma_plane, p.normal_power_log2, p.demodulate_albedo)
    assert got == (5, 4.0, F(0.01), 6, 1)
    q = capi.DenoiseParams()
    assert bytes(q) == bytes(p)                                       # the Python defaults are the library's
    assert DEFAULTS == dict(iterations=5, sigma_luminance=4.0, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1)
    assert lib.fyprt_denoise_default_params(None) == EINVAL


def test_denoise_errors_in_order_on_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    img = np.zeros(16, dtype=np.uint32)
    buf = np.zeros(64, dtype=np.float32)
    base = (buf.ctypes.data + 63) & ~63                      # 64-byte aligned inside `buf` (never dereferenced)
    ok = capi.DenoiseParams()

    def host(p, i=img.ctypes.data, r=base, h=None):
        return lib.fyprt_denoise(h if h is not None else ctx.h, p, i, r, None)

    def device(p, i=base, r=base + 64, h=None):
        return lib.fyprt_denoise_device(h if h is not None else ctx.h, p, i, r)

    bad = [capi.DenoiseParams(iterations=9), capi.DenoiseParams(normal_power_log2=8), capi.DenoiseParams(demodulate_albedo=2),
           capi.DenoiseParams(sigma_luminance=float("nan")), capi.DenoiseParams(sigma_luminance=float("inf")),
           capi.DenoiseParams(sigma_plane=0.0), capi.DenoiseParams(sigma_plane=-1.0), capi.DenoiseParams(sigma_plane=float("nan")),
           capi.DenoiseParams(sigma_plane=float("inf"))]
    fine = [capi.DenoiseParams(iterations=8, normal_power_log2=7, demodulate_albedo=0), capi.DenoiseParams(iterations=0),
            capi.DenoiseParams(sigma_luminance=0.0), capi.DenoiseParams(sigma_luminance=-3.0)]
    assert lib.fyprt_denoise(None, ok, img.ctypes.data, None, None) == EINVAL
    assert lib.fyprt_denoise_device(None, ok, base, None) == EINVAL
    for call in (host, device):
        assert call(None) == EINVAL
        for p in bad:
            assert call(p) == EINVAL
        assert call(ok, i=None, r=None) == EINVAL                     # both outputs NULL
        assert call(bad[0], i=None, r=None) == EINVAL
        # ... then the state: a host-only context has no frame
        assert call(ok) == ESTATE
        assert call(ok, i=None) == ESTATE and call(ok, r=None) == ESTATE   # either output alone is fine
        for p in fine:
            assert call(p) == ESTATE
    # the device entry's alignment, refused before the state
    assert device(ok, i=base + 2) == EINVAL and device(ok, r=base + 72) == EINVAL and device(ok, r=base + 68) == EINVAL
    assert device(ok, i=base + 4, r=base + 80) == ESTATE
    ctx.upload_scene(SCENES["cornell"][0]())
    assert host(ok) == ESTATE and device(ok) == ESTATE and host(bad[0]) == EINVAL
    with pytest.raises(capi.FyprtError):
        ctx.denoise()
    with pytest.raises(capi.FyprtError):
        ctx.read_buffer(capi.BUF_ALBEDO)
    ctx.close()


def test_denoise_tensor_wrapper_checks_before_the_library():
    torch = pytest.importorskip("torch")
    ctx = capi.Context(-1)
    ctx.width, ctx.height = 8, 4
    with pytest.raises(ValueError):
        ctx.denoise_tensor(None, None)
    with pytest.raises(ValueError):
        ctx.denoise_tensor(torch.zeros((4, 8), dtype=torch.float32), None)
    with pytest.raises(ValueError):
        ctx.denoise_tensor(torch.zeros((8, 4), dtype=torch.int32), None)
    with pytest.raises(ValueError):
        ctx.denoise_tensor(None, torch.zeros((4, 8, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        ctx.denoise_tensor(torch.zeros((4, 8), dtype=torch.int32), None)          # on the CPU, not on the context's GPU
    ctx.close()


# ---------------------------------------------------------------------------------------------- the contract on CPU-oracle frames
def _oracle_frames(scene_name, W, H, tech, frames):
    """(accum after frame 1, accum after `frames` frames, payload H x W, scene): frame f rendered with rand_seed = f + 1.  The payload comes
    from a ReSTIR DI frame of the same camera (the oracle writes it only there)."""
    sc = SCENES[scene_name][0]()
    cam = SCENES[scene_name][1](W, H)
    orc = Oracle(sc, W, H)
    orc.set_camera(cam)
    st = settings_for(tech, sky_color=(0.0, 0.0, 0.0), sample_count=1)
    first = None
    for f in range(frames):
        st.rand_seed = f + 1
        orc.render(st)
        if f == 0:
            first = orc.accum().copy()
    last = orc.accum().copy()
    if tech == capi.RESTIR_DI:
        pay = orc.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    else:
        di = Oracle(sc, W, H)
        di.set_camera(cam)
        di.render(settings_for(capi.RESTIR_DI, sky_color=(0.0, 0.0, 0.0), sample_count=1))
        pay = di.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
        di.close()
    orc.close()
    return first, last, pay, sc


def test_reference_contract_properties(oracle_built):
    assert_numpy_keeps_subnormals()
    W, H = 24, 20
    acc, _, pay, sc = _oracle_frames("cornell", W, H, capi.RESTIR_DI, 1)
    alb = guides_from_scene(sc, pay)
    flt = alb[..., 3] != 0
    assert flt.any() and (~flt).any()                                  # walls and the directly seen light
    c = acc[..., :3] / F(1)
    # twice -> identical bits; 6 iterations reach step 32, larger than the image: finite
    a = denoise_ref(acc, pay, alb, 1, iterations=6)
    b = denoise_ref(acc, pay, alb, 1, iterations=6)
    assert bits_equal(a[0], b[0]).all() and (a[1] == b[1]).all()
    assert np.isfinite(a[0]).all()
    # non-filterable pixels come back unchanged, whatever the parameters
    for kw in (dict(DEFAULTS), dict(iterations=3, sigma_luminance=0.0, sigma_plane=0.5, normal_power_log2=0, demodulate_albedo=0)):
        rad, img = denoise_ref(acc, pay, alb, 1, **kw)
        assert bits_equal(rad[~flt][:, :3], c[~flt]).all()
        assert (rad[..., 3] == acc[..., 3]).all()
        assert (rad[flt][:, :3] != c[flt]).any()                        # ... and the filter does something elsewhere
    # iterations = 0, demodulate = 0: the frame's own radiance and image
    rad, img = denoise_ref(acc, pay, alb, 1, iterations=0, demodulate_albedo=0)
    assert bits_equal(rad[..., :3], c).all()
    full = np.concatenate([c, acc[..., 3:]], axis=-1)
    assert (img == tonemap_pack(full)).all()


@pytest.mark.parametrize("tech", [capi.NEE, capi.RESTIR_DI])
def test_reference_filter_halves_the_error_of_a_one_sample_frame(oracle_built, tech):
    """Sanity bound of the specification itself: MSE(denoised frame 1) <= 0.5 * MSE(frame 1) against 256 accumulated frames of the same
    technique, linear radiance, Cornell box 128 x 128, default parameters.  (A guard against a broken filter, not a quality bar.)"""
    W = H = 128
    first, last, pay, sc = _oracle_frames("cornell", W, H, tech, 256)
    ref = (last[..., :3] / F(256)).astype(np.float64)
    alb = guides_from_scene(sc, pay)
    rad, _ = denoise_ref(first, pay, alb, 1, **DEFAULTS)
    raw = float(np.mean((first[..., :3].astype(np.float64) - ref) ** 2))
    den = float(np.mean((rad[..., :3].astype(np.float64) - ref) ** 2))
    print(f"technique {tech}: MSE raw {raw:.5f} -> denoised {den:.5f} (ratio {den / raw:.3f})")
    assert np.isfinite(raw) and np.isfinite(den) and raw > 0
    assert den <= 0.5 * raw
