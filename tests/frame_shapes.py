"""Frame shapes, bands and kernel forms at which every frame kernel is held to the oracle, and the driver that renders a frame on both
sides and compares.  Shared by tests/test_gpu_frame_shapes.py (device against the oracle walking the product's tree, bit for bit) and
tests/test_frame_shapes_cpu.py (the non-vacuity conditions on the oracle alone, which need no GPU).  No tests in here.

A wave is an 8x8 pixel tile and a workgroup 16x16 pixels (pixel_of_thread, rt_kernels.h): at a width that is no multiple of 8 part of
a live wave lies outside the frame while the wave goes on to ballot, compact, sort, claim chunks and refill."""
import ctypes as C

import numpy as np

from common import SCENES, _compare_buffers, bits_equal, settings_for
from fypraytracer_amd import capi

SCENE_NAMES = ["cornell", "hall_small"]

SHAPES = [
    (1, 1),       # a single lane: one pixel, one live lane in one wave, every queue 0 or 1 task long
    (1, 37),      # a single column: one lane of every wave row, three tile rows
    (37, 1),      # a single row: the first row of three tile columns, the last one 5 pixels wide
    (7, 5),       # less than one wave
    (9, 17),      # 16+1 high: a tile row of one pixel row; the second wave column holds one pixel column
    (17, 9),      # 16+1 wide: a tile column of one pixel column; the second wave row holds one pixel row
    (63, 3),      # around one wave width from below: the last wave misses one column
    (65, 33),     # around one wave width from above: 4 tile columns + one pixel column, 2 tile rows + one pixel row
    (97, 61),     # the denoiser's odd size
    (129, 17),    # 9 tile columns by 2 tile rows: tile orders 1 and 2 leave most of the padded grid empty
]

# (b): the shapes every kernel form runs at
FORM_SHAPES = [(1, 1), (7, 5), (17, 9), (37, 1), (97, 61)]
# (c): asynchronous frames
ASYNC_SHAPES = [(7, 5), (37, 1), (97, 61)]

# (d): bands of a 97x61 frame: one row at the top, at the bottom and inside; borders at no multiple of 8; one whole tile row; with
# halo 3 the band (0, 7) takes the extra Part-1 row (part1_rows in fyprt.hip: rowBegin < halo and rowEnd + halo < H)
BAND_SHAPE = (97, 61)
BANDS = [(0, 1), (60, 61), (30, 31), (5, 22), (16, 32), (13, 48), (0, 7), (55, 61)]
NARROW_BAND_SHAPE = (9, 17)
NARROW_BANDS = [(0, 1), (3, 4)]
BAND_HALO = 3                   # == the bands' spatial_neighbor_radius

# (e): (stripe rows, parts) at 97x61
STRIPE_SHAPE = (97, 61)
STRIPES = [(1, 3), (5, 2)]

PER_PIXEL = list(range(capi.RESTIR_DI))       # techniques 0-6: every pixel independent of every other

# (b): kernel forms as (name, techniques, tuning keys).  Every one of them must equal the oracle.
FORMS = {
    "di": [(n, [capi.RESTIR_DI], k) for n, k in [
        ("part2_fused", {1: 0}), ("setup_speculative", {14: 1}), ("setup_lds", {14: 2}), ("light_sorted", {3: 1}),
        ("one_stream", {11: 0}), ("dead_rays_traced", {18: 0}), ("small_grid_chunks", {2: 1, 4: 16, 9: 3}),
        ("tiles_linear", {0: 0}), ("tiles_eighths", {0: 1}), ("primary_not_kept", {25: 0})]],
    "gi": [(f"gi_part2_{v}", [capi.RESTIR_GI], {19: v}) for v in (0, 1, 2)],
    "stage": [("stages", list(range(6)), {17: 1}), ("fused_frame", list(range(6)), {17: 2})],
    "ray_kernel": [("rays_persistent", PER_PIXEL, {15: 1}), ("rays_per_thread", PER_PIXEL, {15: 2})],
}


def make_pair(scene_name, W, H, knobs=None):
    """(ctx, orc, scene, camera): a context with `knobs` set and the oracle walking that context's tree"""
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES[scene_name]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = capi.Context(0)
    for k, v in (knobs or {}).items():
        ctx.set_tuning(k, v)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    orc = Oracle(sc, W, H)
    orc.set_camera(cam)
    orc.use_product_bvh(ctx.export_bvh())
    return ctx, orc, sc, cam


def product_oracle(scene_name, W, H):
    """the oracle over the product tree of a host-only context (no GPU)"""
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES[scene_name]
    sc, cam = mk_scene(), mk_cam(W, H)
    host = capi.Context(-1)
    host.upload_scene(sc)
    orc = Oracle(sc, W, H)
    orc.set_camera(cam)
    orc.use_product_bvh(host.export_bvh())
    host.close()
    return orc, sc, cam


def stripe_rows(H, stripe, parts, part):
    return np.array([y for y in range(H) if (y // stripe) % parts == part], np.int64)


def _first_difference(ok):
    """(x, y) of the first False of a (rows, W) mask, y relative to the mask"""
    y, x = np.argwhere(~ok)[0]
    return int(x), int(y)


def _compare_frame(ctx, orc, own, where):
    img, acc = ctx.readback()
    for name, g, o in (("accumulation", acc, orc.accum()), ("image", img, orc.image())):
        ok = bits_equal(g[own], o[own]) if g.dtype.kind == "f" else g[own] == o[own]
        ok = ok.all(axis=-1) if ok.ndim > 2 else ok
        if not ok.all():
            x, y = _first_difference(ok)
            raise AssertionError(f"{where}: {name} differs in {(~ok).sum()} of {ok.size} pixels, first at (x, y) = ({x}, {int(own[y])})")


def run_pair(ctx, orc, tech, frames, rows=None, halo=0, stripes=None, use_async=False, counters=False, label="", **settings):
    """Render `frames` frames of technique `tech` on the device and in the oracle, rand_seed = f + 1, and compare after every frame
    the accumulation and the image, NaN-aware (common.bits_equal), and for ReSTIR the per-pixel buffers of common._compare_buffers.
    `rows` = (begin, end): the context renders that band (fyprt_set_rows with `halo`) and its rows are compared; the reference is the
    oracle's band for ReSTIR (a band keeps history for its own rows only) and the oracle's full frame for the per-pixel techniques.
    `stripes` = (stripe rows, parts, part): the context renders those stripes, compared with the full frame's rows.
    `use_async`: fyprt_render_async for every frame, one synchronize, one comparison after the last.
    `counters`: the context counts (fyprt_set_ray_counting); rays, box tests, triangle tests, hits and node visits of every frame equal the oracle's.
    The context is resized first (zero buffers, frame index 1); the oracle must be fresh.  `label` names scene and form in a failure."""
    W, H = ctx.width, ctx.height
    restir = tech >= capi.RESTIR_DI
    ctx.resize(W, H)
    own = np.arange(H)
    if rows is not None:
        ctx.set_rows(rows[0], rows[1], halo)
        own = np.arange(rows[0], rows[1])
    elif stripes is not None:
        ctx.set_row_stripes(*stripes)
        own = stripe_rows(H, *stripes)
    st = settings_for(tech, **settings)
    for f in range(frames):
        st.rand_seed = f + 1
        g = ctx.render_async(st) if use_async else ctx.render(st)
        o = orc.render(st, rows=rows, halo=halo) if restir and rows is not None else orc.render(st)
        if use_async and f + 1 < frames:
            continue
        ctx.synchronize()
        where = f"{label} {W}x{H} {capi.TECHNIQUE_NAMES[tech]} rows {rows} stripes {stripes} frame {f + 1}"
        if counters:
            got = {k: int(getattr(g, k)) for k in ("rays", "box_tests", "tri_tests", "hits", "node_visits")}
            assert got == {k: int(o[k]) for k in got}, f"{where}: counters {got}, the oracle's {o}"
        _compare_frame(ctx, orc, own, where)
        if restir:
            try:
                _compare_buffers(ctx, orc, tech, rows=rows)
            except AssertionError as e:
                raise AssertionError(f"{where}: {e}") from None


def camera_rays(orc, cam, W, H):
    """(origins, directions) of every pixel in row-major order, directions from the oracle's camera (orc_ray_direction)"""
    out3 = np.zeros(3, np.float32)
    d = np.zeros((H * W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            orc.lib.orc_ray_direction(orc.h, x, y, out3.ctypes.data_as(C.c_void_p))
            d[y * W + x] = out3
    return np.broadcast_to(np.asarray(cam.position, np.float32), d.shape).copy(), d


# ---------------------------------------------------------------------------------------------- neighbor_index, restated
def pcg_hash(v):
    """pcg_hash of rt_math.h on uint32 arrays"""
    v = np.asarray(v, np.uint32)
    with np.errstate(over="ignore"):
        state = v * np.uint32(747796405) + np.uint32(2891336453)
        word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
    return (word >> np.uint32(22)) ^ word


def neighbor_index(W, H, x, y, radius, s1, s2):
    """neighbor_from_states of rt_wavefront.h (== neighbor_index of rt_kernels.h with its two draws given as stream states s1, s2):
    the offset is truncated to int, added in UNSIGNED arithmetic and only then clamped to the frame, so a neighbour left of column 0 or
    above row 0 wraps to about 2^32 and clamps to the LAST column or row.  Returns (index, wrapped in x, wrapped in y)."""
    F = np.float32
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    out, wrapped = [], []
    for c, s, size in ((x, s1, W), (y, s2, H)):
        o = F(2.0) * (np.asarray(s, np.uint32).astype(F) * F(2.0 ** -32)) - F(1.0)
        step = (o * F(radius)).astype(np.int32).astype(np.int64)              # (int): toward zero
        u = (c + step) & 0xFFFFFFFF                                          # uint32 wrap
        wrapped.append(c + step < 0)
        f = u.astype(np.uint32).astype(F)
        f = np.maximum(F(0.0), np.minimum(F(size) - F(1.0), f))
        out.append(f.astype(np.uint32).astype(np.int64))
    return out[0] + out[1] * W, wrapped[0], wrapped[1]


def first_neighbor_draws(W, H, frame_index, rand_seed):
    """The stream states of the first spatial neighbour's two draws of every pixel in ReSTIR DI Part 2 (k_di_part2 / part2_setup in
    rt_kernels.h / rt_wavefront.h): seed = i * (frameIndex + 213 + randSeed), one draw by the pixel's own di_update, then ox, then oy."""
    i = np.arange(W * H, dtype=np.uint32)
    with np.errstate(over="ignore"):
        s = i * np.uint32(frame_index + 213 + rand_seed)
    s1 = pcg_hash(pcg_hash(s))
    return s1, pcg_hash(s1)
