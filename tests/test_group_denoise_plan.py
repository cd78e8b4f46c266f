"""Host logic of the group denoiser (no GPU): the transfer plan of one fyprt_group_denoise call, through the C ABI of the built
library (fyprt_group_denoise_plan).  Stage 0 carries the guide records of the 2^iterations rows either side of a band, stage 1 + k the
colour rows iteration k reads (2^(k+1) either side); halos are clipped to the image and split over the bands that own their rows."""
import ctypes as C

import pytest

from fypraytracer_amd import capi

EINVAL = -1
TABLES = [
    (192, [0, 96, 192]), (192, [0, 40, 70, 150, 192]), (192, [0, 1, 2, 95, 96, 192]), (192, [0, 192]),
    (61, [0, 1, 17, 18, 61]), (61, [0, 30, 61]), (61, [0, 61]),
]


def _rows(lo, hi, H):
    return set(range(max(0, lo), min(H, hi)))


@pytest.mark.parametrize("iterations", range(9))
@pytest.mark.parametrize("H,bounds", TABLES)
def test_plan_covers_exactly_the_halo_of_every_band_and_stage(H, bounds, iterations):
    n = len(bounds) - 1
    plan = capi.group_denoise_plan(bounds, H, iterations)
    if iterations == 0 or n == 1:
        assert plan == []
        return
    stages = [t[0] for t in plan]
    assert stages == sorted(stages) and set(stages) == set(range(iterations + 1))      # issue order: the stages ascend, none is missing
    got = {}
    for stage, recv, owner, r0, r1 in plan:
        assert recv != owner and r0 < r1
        assert bounds[owner] <= r0 and r1 <= bounds[owner + 1]                          # every row comes from the band that owns it
        rows = got.setdefault((stage, recv), set())
        assert not rows & set(range(r0, r1)), "entries overlap"
        rows |= set(range(r0, r1))
    for stage in range(iterations + 1):
        h = 2 ** iterations if stage == 0 else 2 ** stage                              # stage 1 + k: 2^(k+1) rows
        for r in range(n):
            b, e = bounds[r], bounds[r + 1]
            assert got.get((stage, r), set()) == _rows(b - h, b, H) | _rows(e, e + h, H), (stage, r)


def test_capacity_query_and_partial_capacity_write_nothing_beyond():
    lib = capi.load_library()
    bounds, H, it = [0, 40, 70, 150, 192], 192, 5
    arr = capi._u32_array(bounds)
    cnt = lib.fyprt_group_denoise_plan(arr, 4, H, it, None, 0)
    full = capi.group_denoise_plan(bounds, H, it)
    assert cnt == len(full) > 8
    out = (C.c_uint32 * (5 * cnt))(*([0xDEADBEEF] * (5 * cnt)))
    assert lib.fyprt_group_denoise_plan(arr, 4, H, it, out, 0) == cnt and all(v == 0xDEADBEEF for v in out)
    assert lib.fyprt_group_denoise_plan(arr, 4, H, it, out, 3) == cnt
    assert [tuple(out[5 * k: 5 * k + 5]) for k in range(3)] == full[:3] and all(v == 0xDEADBEEF for v in out[15:])


@pytest.mark.parametrize("bounds,H,it", [([1, 96, 192], 192, 3), ([0, 96, 190], 192, 3), ([0, 96, 96, 192], 192, 3), ([0, 100, 96, 192], 192, 3),
                                         ([0, 96, 192], 192, 9)])
def test_bad_tables_are_refused(bounds, H, it):
    lib = capi.load_library()
    assert lib.fyprt_group_denoise_plan(capi._u32_array(bounds), len(bounds) - 1, H, it, None, 0) == EINVAL
    with pytest.raises(capi.FyprtError):
        capi.group_denoise_plan(bounds, H, it)


def test_null_arguments():
    lib = capi.load_library()
    assert lib.fyprt_group_denoise_plan(None, 2, 192, 3, None, 0) == EINVAL
    assert lib.fyprt_group_denoise_plan(capi._u32_array([0, 192]), 0, 192, 3, None, 0) == EINVAL
    p = capi.DenoiseParams()
    img = (C.c_uint32 * 4)()
    assert lib.fyprt_group_denoise(None, C.byref(p), img, None, None) == EINVAL
    assert lib.fyprt_group_denoise_device(None, C.byref(p), 0, None, None) == EINVAL
