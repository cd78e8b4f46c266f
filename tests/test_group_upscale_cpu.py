"""fyprt_group_denoise_upscale without a GPU: the declarations, and — on frames of the CPU oracle — that the frame and the band tables the
GPU suite uses (tests/group_upscale_ref.py) are no vacuous case: the low-res row below a band really reaches the band's last hi-res rows
at every scale, and the moving sequence really leaves a history window of 4 rows."""
import re
from pathlib import Path

import numpy as np
import pytest

from common import SCENES, settings_for
from denoise_ref import DEFAULTS, assert_numpy_keeps_subnormals, guides_from_scene
from fypraytracer_amd import capi
from group_temporal_ref import rows_needed
from group_upscale_ref import FIVE, H, MOVES, SCENE, TWO, W, assert_border_rows_matter
from oraclelib import Oracle
from temporal_ref import camera_matrix
from upscale_ref import hires_from_payload, lowres_colour

HEADER = Path(__file__).resolve().parent.parent / "include" / "fyprt.h"
SKY = (0.1, 0.2, 0.3)


def test_symbols_and_declarations():
    lib = capi.load_library()
    names = {"fyprt_group_denoise_upscale", "fyprt_group_denoise_upscale_device", "fyprt_group_denoise_upscale_plan"}
    assert names <= set(capi.EXPORTED_SYMBOLS)
    text = HEADER.read_text()
    for n in names:
        assert hasattr(lib, n) and re.search(r"int %s\(" % n, text)
    assert hasattr(capi.Group, "denoise_upscale") and hasattr(capi.Group, "denoise_upscale_tensor")


def _payload(sc, cam, w, h, st):
    orc = Oracle(sc, w, h)
    orc.set_camera(cam)
    orc.render(st)
    out = orc.accum().copy(), orc.read_buffer(capi.BUF_PAYLOAD).reshape(h, w).copy()
    orc.close()
    return out


@pytest.mark.parametrize("s", [2, 3, 4])
def test_the_row_below_a_band_reaches_its_last_hires_rows(oracle_built, s):
    assert_numpy_keeps_subnormals()
    mk_scene, mk_cam = SCENES[SCENE]
    sc = mk_scene()
    st = settings_for(capi.RESTIR_DI, sky_color=SKY, sample_count=1)
    acc, pay = _payload(sc, mk_cam(W, H), W, H, st)
    _, pay_hi = _payload(sc, mk_cam(W * s, H * s), W * s, H * s, st)
    alb = guides_from_scene(sc, pay)
    g, a_hi = hires_from_payload(sc, pay_hi, SKY)
    for par in (dict(DEFAULTS), dict(DEFAULTS, iterations=0, demodulate_albedo=0)):
        e = lowres_colour(acc, pay, alb, 1, **par)
        for bounds in (TWO, FIVE):
            assert_border_rows_matter(e, pay, alb, acc, 1, g, a_hi, s, bounds, **par)


def test_the_moving_sequence_leaves_a_window_of_four_rows(oracle_built):
    mk_scene, mk_cam = SCENES[SCENE]
    sc = mk_scene()
    cam = mk_cam(W, H)
    st = settings_for(capi.RESTIR_DI, sky_color=SKY, sample_count=1)
    M_prev, reach = None, []
    for move in MOVES:
        cam.on_update(0.05, *move)
        _, pay = _payload(sc, cam, W, H, st)
        M = camera_matrix(cam)
        cam.commit_frame()
        if M_prev is not None:
            reach.append(int(rows_needed(pay, guides_from_scene(sc, pay), M_prev, FIVE).max()))
        M_prev = M
    print("rows beyond the band per call:", reach)
    assert max(reach) > 4 and min(reach) >= 0
