"""What the tests of fyprt_group_denoise_upscale share — a test helper, not a test.

The contract needs no restatement of its own: it is upscale_ref (tests/upscale_ref.py) on the stitched low-res buffers and the stitched
hi-res records, with e from denoise_ref or group_temporal_ref.  What is here is the frame the GPU suite runs on and the check that this
frame can tell a band that pulled the low-res row below it from one that did not."""
import numpy as np

from common import bits_equal
from upscale_ref import WEIGHTED, upscale_ref

SCENE, W, H = "hall_small", 48, 64
TWO, FIVE = [0, 32, 64], [0, 13, 14, 31, 48, 64]      # FIVE: a one-row band; no border is a multiple of a tile or of any scale
# tests/test_gpu_moving_camera.py's MOVES: (keys held, mouse delta in pixels) per frame
MOVES = [("", (0.0, 0.0)), ("W", (60.0, -25.0)), ("DE", (-140.0, 40.0)), ("S", (90.0, 70.0)), ("AQ", (-35.0, -110.0)), ("W", (20.0, 10.0))]


def assert_border_rows_matter(e, payload, albedo, accum, n, up_guide, up_albedo, s, bounds, want=None, **par):
    """The frame is no vacuous case for the bands of `bounds`: in every band but the last, the last s - 1 hi-res rows hold at least one
    "S > 0" pixel, and upscale_ref with the colour of the low-res row below the band zeroed gives other bits in those rows — so a band
    that resolved without its neighbour's row e would be caught.  want: upscale_ref's result for the unchanged e, if the caller has it."""
    rad, _, br = want if want is not None else upscale_ref(e, payload, albedo, accum, n, up_guide, up_albedo, s, **par)
    zeroed = np.array(e, dtype=np.float32, copy=True)
    zeroed[bounds[1:-1]] = 0
    rad0 = upscale_ref(zeroed, payload, albedo, accum, n, up_guide, up_albedo, s, **par)[0]
    for k, eb in enumerate(bounds[1:-1]):
        rows = slice(s * eb - (s - 1), s * eb)
        assert (br[rows] == WEIGHTED).any(), f"scale {s}, band {k}: no S > 0 pixel in its last {s - 1} hi-res rows"
        assert not bits_equal(rad[rows, :, :3], rad0[rows, :, :3]).all(), f"scale {s}, band {k}: row {eb}'s colour does not reach its last hi-res rows"
