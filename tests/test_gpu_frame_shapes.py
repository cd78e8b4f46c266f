"""Frame kernels at odd, tiny and one-row frames and bands, HIP path against the CPU oracle walking the product's own tree, bit for bit
("equal" = bitwise, NaN-aware), with no tolerance and no skipped pixels.  Shapes, bands, forms and the driver: tests/frame_shapes.py;
that these shapes exercise partial waves, sky, shadow rays and the unsigned neighbour wrap: tests/test_frame_shapes_cpu.py.

(a) whole frames of all nine techniques at every shape, default radius 30 (wider than most of these frames);
(b) every kernel form (tuning keys) at five shapes, each against the oracle, not against the default form, and the instrumented
    kernels with their counters;
(c) asynchronous ReSTIR DI frames (the pipelined, split Part 1);
(d) bands of a 97x61 frame, one-row bands and the extra Part-1 row of a top band included; ReSTIR bands against the oracle's band
    (a band keeps history for its own rows only), per-pixel techniques against the full frame's rows;
(e) interleaved stripes at a width of 97;
(f) ray and radiance queries of the frame's own camera rays, ray counts that are no multiple of 64."""
import numpy as np
import pytest

import frame_shapes as fs
from common import bits_equal, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
_shape_id = lambda s: f"{s[0]}x{s[1]}"
_band_id = lambda b: f"rows{b[0]}-{b[1]}"


def _fresh_oracle(ctx, sc, cam):
    from oraclelib import Oracle
    orc = Oracle(sc, ctx.width, ctx.height)
    orc.set_camera(cam)
    orc.use_product_bvh(ctx.export_bvh())
    return orc


def _run(ctx, orc, sc, cam, tech, frames, **kw):
    """run_pair on a fresh oracle (the first one comes with the pair)"""
    orc = orc or _fresh_oracle(ctx, sc, cam)
    try:
        fs.run_pair(ctx, orc, tech, frames, **kw)
    finally:
        orc.close()


# ---------------------------------------------------------------------------------------------- (a) whole frames
@pytest.mark.parametrize("shape", fs.SHAPES, ids=_shape_id)
@pytest.mark.parametrize("scene_name", fs.SCENE_NAMES)
def test_whole_frames_of_every_technique(oracle_built, scene_name, shape):
    ctx, orc, sc, cam = fs.make_pair(scene_name, *shape)
    for tech in range(9):
        _run(ctx, orc, sc, cam, tech, 3, label=f"{scene_name} default")
        orc = None
    ctx.close()


# ---------------------------------------------------------------------------------------------- (b) kernel forms
@pytest.mark.parametrize("family", list(fs.FORMS))
@pytest.mark.parametrize("shape", fs.FORM_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("scene_name", fs.SCENE_NAMES)
def test_kernel_forms_equal_the_oracle(oracle_built, scene_name, shape, family):
    for name, techs, knobs in fs.FORMS[family]:
        ctx, orc, sc, cam = fs.make_pair(scene_name, *shape, knobs=knobs)
        for key, value in knobs.items():
            assert ctx.get_tuning(key) == value
        for tech in techs:
            _run(ctx, orc, sc, cam, tech, 3, label=f"{scene_name} {name} {knobs}")
            orc = None
        ctx.close()


@pytest.mark.parametrize("shape", fs.FORM_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("scene_name", fs.SCENE_NAMES)
def test_instrumented_frames_and_their_counters_equal_the_oracle(oracle_built, scene_name, shape):
    """the counting instantiations of the kernels (fyprt_set_ray_counting): the same frames, and the counts the oracle's restatement of
    the same traversal gives — with lanes of a live wave outside the frame nothing may be counted for them"""
    ctx, orc, sc, cam = fs.make_pair(scene_name, *shape)
    ctx.set_ray_counting(True)
    for tech in range(9):
        _run(ctx, orc, sc, cam, tech, 3, counters=True, label=f"{scene_name} instrumented")
        orc = None
    ctx.close()


# ---------------------------------------------------------------------------------------------- (c) asynchronous frames
@pytest.mark.parametrize("shape", fs.ASYNC_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("scene_name", fs.SCENE_NAMES)
def test_async_restir_di_frames(oracle_built, scene_name, shape):
    ctx, orc, sc, cam = fs.make_pair(scene_name, *shape)
    assert ctx.get_tuning(21) != 0 and ctx.get_tuning(11) != 0               # the pipelined frame with the split Part 1
    _run(ctx, orc, sc, cam, capi.RESTIR_DI, 4, use_async=True, label=f"{scene_name} async")
    ctx.close()


# ---------------------------------------------------------------------------------------------- (d) bands
_BANDS = [(fs.BAND_SHAPE, b) for b in fs.BANDS] + [(fs.NARROW_BAND_SHAPE, b) for b in fs.NARROW_BANDS]
_bands_id = lambda sb: f"{_shape_id(sb[0])}-{_band_id(sb[1])}"


@pytest.mark.parametrize("shape_band", _BANDS, ids=_bands_id)
@pytest.mark.parametrize("scene_name", fs.SCENE_NAMES)
def test_band_of_a_per_pixel_technique_equals_the_full_frame_rows(oracle_built, scene_name, shape_band):
    shape, band = shape_band
    ctx, orc, sc, cam = fs.make_pair(scene_name, *shape)
    for tech in fs.PER_PIXEL:
        _run(ctx, orc, sc, cam, tech, 2, rows=band, label=f"{scene_name} band")
        orc = None
    ctx.close()


@pytest.mark.parametrize("shape_band", _BANDS, ids=_bands_id)
@pytest.mark.parametrize("scene_name", fs.SCENE_NAMES)
def test_restir_band_equals_the_oracle_band(oracle_built, scene_name, shape_band):
    shape, band = shape_band
    ctx, orc, sc, cam = fs.make_pair(scene_name, *shape)
    for tech in (capi.RESTIR_DI, capi.RESTIR_GI):
        _run(ctx, orc, sc, cam, tech, 3, rows=band, halo=fs.BAND_HALO, spatial_neighbor_radius=fs.BAND_HALO, label=f"{scene_name} band halo {fs.BAND_HALO}")
        orc = None
    ctx.close()


# ---------------------------------------------------------------------------------------------- (e) stripes
@pytest.mark.parametrize("stripe,parts", fs.STRIPES)
@pytest.mark.parametrize("scene_name", fs.SCENE_NAMES)
def test_stripes_equal_the_full_frame_rows(oracle_built, scene_name, stripe, parts):
    ctx, orc, sc, cam = fs.make_pair(scene_name, *fs.STRIPE_SHAPE)
    for tech in (capi.BRUTE_FORCE, capi.NEE):
        for part in range(parts):
            _run(ctx, orc, sc, cam, tech, 2, stripes=(stripe, parts, part), label=f"{scene_name} stripes")
            orc = None
    ctx.close()


# ---------------------------------------------------------------------------------------------- (f) queries
def _records_equal(a, b):
    a8, b8 = np.ascontiguousarray(a).view(np.uint8).reshape(-1, 40), np.ascontiguousarray(b).view(np.uint8).reshape(-1, 40)
    return a8.shape == b8.shape and not (a8 != b8).any()


@pytest.mark.parametrize("shape", fs.SHAPES, ids=_shape_id)
@pytest.mark.parametrize("scene_name", fs.SCENE_NAMES)
def test_queries_of_the_camera_rays_equal_the_frame(oracle_built, scene_name, shape):
    W, H = shape
    ctx, orc, sc, cam = fs.make_pair(scene_name, W, H)
    o, d = fs.camera_rays(orc, cam, W, H)
    orc.close()
    ctx.render_part(settings_for(capi.RESTIR_DI), 1)
    ctx.synchronize()
    frame = ctx.read_buffer(capi.BUF_PAYLOAD)
    got = ctx.trace_rays(o, d)
    assert _records_equal(got, frame), f"{scene_name} {W}x{H}: trace_rays differs from Part 1's payload"
    for tech in (capi.BRUTE_FORCE, capi.NEE):
        ctx.resize(W, H)                                          # zero accumulation, frame index 1
        st = settings_for(tech)
        st.to_accumulate = 0
        ctx.render(st)
        acc = ctx.readback()[1].reshape(-1, 4)
        pay = ctx.read_buffer(capi.BUF_PAYLOAD)
        rad, qpay = ctx.render_rays(o, d, st, frame_index=1, want_payload=True)
        ok = bits_equal(F32(0) + rad, acc).all(axis=-1)
        assert ok.all(), f"{scene_name} {W}x{H} {capi.TECHNIQUE_NAMES[tech]}: render_rays differs from the frame, first at pixel {int(np.argmax(~ok))}"
        assert _records_equal(qpay, pay)
    ctx.close()
