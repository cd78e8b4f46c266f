"""Host logic of the group upscaler (no GPU): the transfer plan of one fyprt_group_denoise_upscale call, through the C ABI of the built
library (fyprt_group_denoise_upscale_plan).  It is the plan of the low-res stage — fyprt_group_denoise_plan or, in temporal mode,
fyprt_group_denoise_temporal_plan — followed by one more stage: every band but the last pulls the one colour row below it, the low-res
row its last hi-res rows tap."""
import ctypes as C

import pytest

from fypraytracer_amd import capi

EINVAL = -1
BOUNDS, H = [0, 13, 14, 31, 48], 48


def _prefix(bounds, height, iterations, temporal, history_rows):
    if temporal:
        return capi.group_denoise_temporal_plan(bounds, height, iterations, history_rows)
    return capi.group_denoise_plan(bounds, height, iterations)


@pytest.mark.parametrize("history_rows", [0, 4, 48])
@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_plan_is_the_low_res_plan_and_one_more_stage(iterations, temporal, history_rows):
    plan = capi.group_denoise_upscale_plan(BOUNDS, H, iterations, temporal, history_rows)
    prefix = _prefix(BOUNDS, H, iterations, temporal, history_rows)
    assert plan[:len(prefix)] == prefix
    stage = (3 if temporal else 1) + iterations
    assert all(t[0] < stage for t in prefix)                                              # the added stage is numbered after every other
    assert plan[len(prefix):] == [(stage, k, k + 1, BOUNDS[k + 1], BOUNDS[k + 1] + 1) for k in range(3)]


@pytest.mark.parametrize("temporal", [False, True])
def test_spatial_mode_does_not_read_history_rows(temporal):
    a, b = (capi.group_denoise_upscale_plan(BOUNDS, H, 2, temporal, r) for r in (0, 7))
    assert (a == b) == (not temporal)


@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("iterations", [0, 3])
def test_a_single_band_adds_no_entry(iterations, temporal):
    assert capi.group_denoise_upscale_plan([0, H], H, iterations, temporal, 4) == _prefix([0, H], H, iterations, temporal, 4) == []


def test_every_band_but_the_last_pulls_the_row_its_neighbour_owns():
    for bounds, height in (([0, 1, 2, 95, 96, 192], 192), ([0, 60, 61], 61)):
        plan = capi.group_denoise_upscale_plan(bounds, height, 3, False)
        added = [t for t in plan if t[0] == 4]
        assert [t[1] for t in added] == list(range(len(bounds) - 2))
        for _, recv, owner, r0, r1 in added:
            assert r0 == bounds[recv + 1] and r1 == r0 + 1 and bounds[owner] <= r0 < bounds[owner + 1]


@pytest.mark.parametrize("temporal", [0, 1])
@pytest.mark.parametrize("bounds,height,it", [([1, 24, 48], 48, 3), ([0, 24, 46], 48, 3), ([0, 24, 24, 48], 48, 3), ([0, 30, 24, 48], 48, 3),
                                              ([0, 24, 48], 48, 9)])
def test_bad_tables_are_refused(bounds, height, it, temporal):
    lib = capi.load_library()
    assert lib.fyprt_group_denoise_upscale_plan(capi._u32_array(bounds), len(bounds) - 1, height, it, temporal, 4, None, 0) == EINVAL
    with pytest.raises(capi.FyprtError):
        capi.group_denoise_upscale_plan(bounds, height, it, bool(temporal), 4)


@pytest.mark.parametrize("temporal", [0, 1])
def test_capacity_query_and_partial_capacity_write_nothing_beyond(temporal):
    lib = capi.load_library()
    arr = capi._u32_array(BOUNDS)
    full = capi.group_denoise_upscale_plan(BOUNDS, H, 5, bool(temporal), 4)
    cnt = lib.fyprt_group_denoise_upscale_plan(arr, 4, H, 5, temporal, 4, None, 0)
    assert cnt == len(full) > 8
    out = (C.c_uint32 * (5 * cnt))(*([0xDEADBEEF] * (5 * cnt)))
    assert lib.fyprt_group_denoise_upscale_plan(arr, 4, H, 5, temporal, 4, out, 0) == cnt and all(v == 0xDEADBEEF for v in out)
    assert lib.fyprt_group_denoise_upscale_plan(arr, 4, H, 5, temporal, 4, out, 3) == cnt
    assert [tuple(out[5 * k: 5 * k + 5]) for k in range(3)] == full[:3] and all(v == 0xDEADBEEF for v in out[15:])
    assert lib.fyprt_group_denoise_upscale_plan(arr, 4, H, 5, temporal, 4, out, cnt) == cnt
    assert [tuple(out[5 * k: 5 * k + 5]) for k in range(cnt)] == full


def test_null_arguments():
    lib = capi.load_library()
    assert lib.fyprt_group_denoise_upscale_plan(None, 2, 48, 3, 0, 0, None, 0) == EINVAL
    assert lib.fyprt_group_denoise_upscale_plan(capi._u32_array([0, 48]), 0, 48, 3, 0, 0, None, 0) == EINVAL
    p = capi.UpscaleParams()
    img = (C.c_uint32 * 4)()
    assert lib.fyprt_group_denoise_upscale(None, C.byref(p), 0, img, None, None) == EINVAL
    assert lib.fyprt_group_denoise_upscale_device(None, C.byref(p), 0, 0, None, None) == EINVAL
