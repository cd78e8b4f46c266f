"""The conditions under which tests/test_gpu_frame_shapes.py tests something real, asserted on the oracle alone (no GPU): the oracle
walks the product tree exported from a host-only context.  Every shape sees geometry, some see sky and some none, a ReSTIR DI frame
traces shadow rays at every shape, the default radius of 30 sends neighbour draws through the unsigned wrap at every shape narrower or
lower than the radius, and the band (0, 7) with halo 3 takes the extra Part-1 row."""
import numpy as np
import pytest

import frame_shapes as fs
from common import settings_for
from fypraytracer_amd import capi


@pytest.fixture(scope="module")
def di_frames(oracle_built):
    """per shape: (payload, ReSTIR DI reservoirs, rays traced) of the oracle's first ReSTIR DI frame on cornell"""
    out = {}
    for W, H in fs.SHAPES:
        orc, _, _ = fs.product_oracle("cornell", W, H)
        cnt = orc.render(settings_for(capi.RESTIR_DI))
        out[(W, H)] = (orc.read_buffer(capi.BUF_PAYLOAD), orc.read_buffer(capi.BUF_DI), int(cnt["rays"]))
        orc.close()
    return out


def test_shape_lists():
    assert len(set(fs.SHAPES)) == 10
    assert set(fs.FORM_SHAPES) <= set(fs.SHAPES) and set(fs.ASYNC_SHAPES) <= set(fs.SHAPES)
    assert all(s in fs.SHAPES for s in (fs.BAND_SHAPE, fs.NARROW_BAND_SHAPE, fs.STRIPE_SHAPE))
    assert sum(W % 8 != 0 for W, _ in fs.SHAPES) == 10                       # no width is a whole number of waves
    assert all(0 <= b < e <= fs.BAND_SHAPE[1] for b, e in fs.BANDS) and all(0 <= b < e <= fs.NARROW_BAND_SHAPE[1] for b, e in fs.NARROW_BANDS)
    # every form of the issue, once
    keys = [tuple(sorted(k.items())) for forms in fs.FORMS.values() for _, _, k in forms]
    assert len(keys) == len(set(keys)) == 17
    for stripe, parts in fs.STRIPES:                                           # the parts own every row exactly once
        owned = np.concatenate([fs.stripe_rows(fs.STRIPE_SHAPE[1], stripe, parts, p) for p in range(parts)])
        assert sorted(owned.tolist()) == list(range(fs.STRIPE_SHAPE[1]))


def test_every_shape_sees_geometry_and_some_see_sky(di_frames):
    with_sky = without_sky = 0
    for shape, (pay, _, _) in di_frames.items():
        assert (pay["hitDistance"] > 0).any(), shape
        sky = bool((pay["hitDistance"] < 0).any())
        with_sky += sky
        without_sky += not sky
    assert with_sky >= 3 and without_sky >= 2, (with_sky, without_sky)


def test_restir_di_traces_shadow_rays_at_every_shape(di_frames):
    for (W, H), (_, _, rays) in di_frames.items():
        assert rays > W * H, ((W, H), rays)


def test_neighbor_index_restated():
    """the restatement itself: inside the frame it is the plain offset; left of column 0 / above row 0 it is the LAST column / row"""
    W, H, r = 40, 20, 30
    s = lambda u: np.uint32(int(u * 2 ** 32))                                # the stream state of a draw u
    x, y = np.array([20, 0, 39, 5]), np.array([10, 0, 19, 5])
    #                 ox = 0      ox = -0.5 (-15)   ox = +0.5 (+15)    ox = -0.25 (-7)
    s1 = np.array([s(0.5), s(0.25), s(0.75), s(0.375)])
    s2 = np.array([s(0.5), s(0.25), s(0.75), s(0.5)])
    i, wx, wy = fs.neighbor_index(W, H, x, y, r, s1, s2)
    assert i.tolist() == [20 + 10 * W, 39 + 19 * W, 39 + 19 * W, 39 + 5 * W]
    assert wx.tolist() == [False, True, False, True] and wy.tolist() == [False, True, False, False]


def test_radius_30_wraps_at_every_small_shape(di_frames):
    """Frames 1-3 of the GPU tests (frame index = rand_seed = 1, 2, 3): the first neighbour draw of the pixels Part 2 shades — those
    whose reservoir the oracle's first frame filled — with the stream of first_neighbor_draws."""
    radius = settings_for(capi.RESTIR_DI).spatial_neighbor_radius
    assert radius == 30
    small = [(W, H) for W, H in fs.SHAPES if W < radius or H < radius]
    assert len(small) == 8
    for W, H in small:
        live = di_frames[(W, H)][1]["M"] > 0
        assert live.any(), (W, H)
        i = np.arange(W * H)
        wraps = 0
        for f in (1, 2, 3):
            s1, s2 = fs.first_neighbor_draws(W, H, f, f)
            ni, wx, wy = fs.neighbor_index(W, H, i % W, i // W, radius, s1, s2)
            assert ((0 <= ni) & (ni < W * H)).all()
            assert (ni[wx] % W == W - 1).all() and (ni[wy] // W == H - 1).all()          # the wrap lands on the last column / row
            wraps += int(((wx | wy) & live).sum())
        assert wraps >= 1, (W, H)


class _Side:
    """stands in for a context and for an oracle in run_pair: hands out a fixed frame"""

    def __init__(self, W, H, acc):
        self.width, self.height, self.acc, self.calls = W, H, acc, []
        self.img = (acc[..., 0] * 255).astype(np.uint32)

    def resize(self, W, H): self.calls.append(("resize", W, H))
    def set_rows(self, b, e, halo): self.calls.append(("rows", b, e, halo))
    def set_row_stripes(self, s, n, k): self.calls.append(("stripes", s, n, k))
    def render(self, st, **kw): self.calls.append(("render", st.rand_seed, kw))
    def synchronize(self): pass
    def readback(self): return self.img, self.acc
    def accum(self): return self.acc
    def image(self): return self.img


def test_the_driver_reports_a_single_differing_pixel():
    """one pixel of 9x17 differs in its last bit: the frame, the band and the stripes that own its row fail and name (x, y), those that
    do not own it pass; NaN against NaN passes"""
    W, H = 9, 17
    base = np.random.default_rng(3).random((H, W, 4), dtype=np.float32)
    for kind in ("bit", "nan"):
        a, b = base.copy(), base.copy()
        if kind == "bit":
            b[11, 4, 2] = np.nextafter(b[11, 4, 2], np.float32(2))
        else:
            a[11, 4, 2] = b[11, 4, 2] = np.nan
        for kw, owns in (({}, True), ({"rows": (11, 12)}, True), ({"rows": (3, 11)}, False), ({"stripes": (1, 3, 2)}, True), ({"stripes": (1, 3, 0)}, False)):
            ctx, orc = _Side(W, H, a), _Side(W, H, b)
            if kind == "bit" and owns:
                with pytest.raises(AssertionError, match=r"cornell form 9x17 NEE .* frame 1: accumulation differs in 1 of \d+ pixels, first at \(x, y\) = \(4, 11\)"):
                    fs.run_pair(ctx, orc, capi.NEE, 2, label="cornell form", **kw)
            else:
                fs.run_pair(ctx, orc, capi.NEE, 2, label="cornell form", **kw)
                assert [c[1] for c in ctx.calls if c[0] == "render"] == [1, 2] == [c[1] for c in orc.calls if c[0] == "render"]
                assert all(c[2] == {} for c in orc.calls if c[0] == "render")            # per-pixel technique: the oracle's full frame


def test_band_0_7_takes_the_extra_part1_row():
    H, halo = fs.BAND_SHAPE[1], fs.BAND_HALO
    assert (0, 7) in fs.BANDS
    takes = [(b, e) for b, e in fs.BANDS if b < halo and e + halo < H]       # part1_rows in fyprt.hip: `extra`
    assert (0, 7) in takes and (0, 1) in takes
    assert all(not (b < halo and e + halo < H) for b, e in fs.BANDS if b >= halo)
