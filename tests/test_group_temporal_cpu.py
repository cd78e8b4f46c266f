"""fyprt_group_denoise_temporal without a GPU: declarations, the errors that need no device, the transfer plan against a restatement
and its coverage properties, and the contract's one new term — the history window — on CPU-oracle sequences: the helper
(tests/group_temporal_ref.py) against plain temporal_ref with windows that hold every tap, and with one that cuts history."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from common import bits_equal, struct_equal
from denoise_ref import assert_numpy_keeps_subnormals
from fypraytracer_amd import capi
from group_temporal_ref import band_masked_ref, group_temporal_ref, history_window, rows_needed, windowed_temporal_ref
from temporal_ref import DEFAULTS, temporal_ref
from test_temporal_cpu import _oracle_sequence

EINVAL = -1
HEADER = Path(__file__).resolve().parent.parent / "include" / "fyprt.h"
NAMES = ["fyprt_group_denoise_temporal", "fyprt_group_denoise_temporal_device", "fyprt_group_denoise_temporal_reset",
         "fyprt_group_denoise_temporal_plan"]
TABLES = [[0, 96, 192], [0, 40, 70, 150, 192], [0, 1, 2, 95, 96, 192]]
FIVE = TABLES[1]
BYTES = {0: 32, 1: 16, 2: 64}                                       # per pixel; stage 3 + k: 16 + 4


def test_symbols_header_and_macro():
    lib = capi.load_library()
    text = HEADER.read_text()
    for n in NAMES:
        assert n in capi.EXPORTED_SYMBOLS and hasattr(lib, n) and re.search(r"int %s\(" % n, text), n
    assert re.search(r"#define FYPRT_GROUP_HISTORY_ROWS 32u\b", text) and capi.GROUP_HISTORY_ROWS == 32
    assert "has no temporal form" not in text
    for f in ("denoise_temporal", "denoise_temporal_tensor", "denoise_temporal_reset"):
        assert callable(getattr(capi.Group, f))


def test_errors_that_need_no_device():
    lib = capi.load_library()
    p = capi.TemporalParams()
    img = np.zeros(16, dtype=np.uint32)
    assert lib.fyprt_group_denoise_temporal(None, C.byref(p), 32, img.ctypes.data, None, None) == EINVAL
    assert lib.fyprt_group_denoise_temporal(None, None, 32, img.ctypes.data, None, None) == EINVAL
    assert lib.fyprt_group_denoise_temporal_device(None, C.byref(p), 32, 0, img.ctypes.data, None) == EINVAL
    assert lib.fyprt_group_denoise_temporal_reset(None) == EINVAL
    plan = lib.fyprt_group_denoise_temporal_plan
    tab = capi._u32_array([0, 96, 192])
    assert plan(tab, 2, 192, 5, 32, None, 0) > 0
    assert plan(None, 2, 192, 5, 32, None, 0) == EINVAL
    assert plan(tab, 0, 192, 5, 32, None, 0) == EINVAL and plan(tab, -1, 192, 5, 32, None, 0) == EINVAL
    assert plan(tab, 2, 192, 9, 32, None, 0) == EINVAL                 # iterations > 8
    assert plan(tab, 2, 191, 5, 32, None, 0) == EINVAL                 # the table does not end at the height
    assert plan(capi._u32_array([1, 96, 192]), 2, 192, 5, 32, None, 0) == EINVAL
    assert plan(capi._u32_array([0, 96, 96, 192]), 3, 192, 5, 32, None, 0) == EINVAL      # an empty band
    assert plan(capi._u32_array([0, 100, 96, 192]), 3, 192, 5, 32, None, 0) == EINVAL     # unordered
    with pytest.raises(capi.FyprtError):
        capi.group_denoise_temporal_plan([0, 96, 192], 192, 9)
    assert plan(capi._u32_array([0, 192]), 1, 192, 5, 32, None, 0) == 0                    # one band pulls nothing


# ---------------------------------------------------------------------------------------------- the plan
def _stage_rows(stage, iterations, history_rows, H):
    """Rows either side of a band that stage reads: §"transfer plan" of the header, from what each kernel reads."""
    if stage == 0:
        return max(2, 1 << iterations)                                   # the farthest a-trous tap; the 5 x 5 estimate's 2 rows at least
    if stage == 1:
        return 2
    if stage == 2:
        return min(history_rows, H)
    return 2 << (stage - 3)


def _plan_restated(bounds, H, iterations, history_rows):
    out = []
    n = len(bounds) - 1
    for stage in range(3 + iterations):
        h = _stage_rows(stage, iterations, history_rows, H)
        for r in range(n):
            b, e = bounds[r], bounds[r + 1]
            for lo, hi in ((max(0, b - h), b), (e, min(H, e + h))):
                for j in range(n):
                    a0, a1 = max(lo, bounds[j]), min(hi, bounds[j + 1])
                    if j != r and a0 < a1:
                        out.append((stage, r, j, a0, a1))
    return out


@pytest.mark.parametrize("bounds", TABLES)
def test_plan_equals_the_restatement_and_covers_what_a_band_reads(bounds):
    lib = capi.load_library()
    H, n = bounds[-1], len(bounds) - 1
    for iterations in range(9):
        for R in (0, 1, 4, 32, 192, 10 ** 6):
            plan = capi.group_denoise_temporal_plan(bounds, H, iterations, R)
            assert plan == _plan_restated(bounds, H, iterations, R), (iterations, R)
            assert [t[0] for t in plan] == sorted(t[0] for t in plan)                      # issue order: stage by stage
            assert {t[0] for t in plan} <= set(range(3 + iterations))
            assert (R == 0) == (not any(t[0] == 2 for t in plan))
            covered = {}
            for stage, rcv, own, r0, r1 in plan:
                assert rcv != own and 0 <= r0 < r1 <= H
                assert bounds[own] <= r0 and r1 <= bounds[own + 1]                         # split per owner
                rows = covered.setdefault((stage, rcv), [])
                rows.extend(range(r0, r1))
            for stage in range(3 + iterations):
                h = _stage_rows(stage, iterations, R, H)
                for k in range(n):
                    b, e = bounds[k], bounds[k + 1]
                    want = list(range(max(0, b - h), b)) + list(range(e, min(H, e + h)))  # clipped to the image
                    assert sorted(covered.get((stage, k), [])) == want, (stage, k, iterations, R)      # every row exactly once
            # the history stage is the band's history window without the band
            for k in range(n):
                lo, hi = history_window(bounds[k], bounds[k + 1], R, H)
                assert sorted(covered.get((2, k), [])) == list(range(lo, bounds[k])) + list(range(bounds[k + 1], hi))
            # the count comes back under a short capacity, and nothing is written beyond it
            if plan:
                out = (C.c_uint32 * 10)(*([0xFFFFFFFF] * 10))
                assert lib.fyprt_group_denoise_temporal_plan(capi._u32_array(bounds), n, H, iterations, R, out, 1) == len(plan)
                assert tuple(out[:5]) == plan[0] and list(out[5:]) == [0xFFFFFFFF] * 5
    # the bytes per pixel column and side at the defaults: the history stage (2048) pulls what the spatial call's guide and colour stages
    # pull together (2016) — where FYPRT_GROUP_HISTORY_ROWS comes from
    assert 32 * BYTES[2] == 2048 and 32 * BYTES[0] + sum(2 << k for k in range(5)) * 16 == 2016


# ---------------------------------------------------------------------------------------------- the window on CPU-oracle sequences
W, H = 160, 192
QUICK = dict(DEFAULTS, iterations=1)                                   # one iteration: the feedback colour reads the neighbours, and the run stays short


@functools.lru_cache(maxsize=None)
def _plain(quick):
    """temporal_ref chained over the six moving frames: [(radiance, image, history)]."""
    frames, _, _ = _oracle_sequence("hall_small", W, H, 6, True)
    par = QUICK if quick else DEFAULTS
    hist, M, res = None, None, []
    for acc, pay, alb, pv in frames:
        out = temporal_ref(acc, pay, alb, 1, M, hist, **par)
        res.append(out)
        hist, M = out[2], pv
    return res


def _same(a, b):
    return bits_equal(a[0], b[0]).all() and (a[1] == b[1]).all() and struct_equal(a[2].ravel(), b[2].ravel()).all()


def _needs():
    frames, _, _ = _oracle_sequence("hall_small", W, H, 6, True)
    return [None] + [rows_needed(frames[k][1], frames[k][2], frames[k - 1][3], FIVE) for k in range(1, 6)]


def test_the_conditions_the_tests_rely_on(oracle_built):
    """hall_small 160 x 192, ReSTIR DI, MOVES, bands [0, 40, 70, 150, 192]: no tap reaches more than 15 rows beyond its band, so a
    window of 16 holds every tap; on calls 4 and 5, 1670 and 2676 pixels reach 8 rows or more, so a window of 4 must cut history."""
    needs = _needs()
    assert max(int(n.max()) for n in needs[1:]) == 15
    assert int((needs[3] >= 8).sum()) == 1670 and int((needs[4] >= 8).sum()) == 2676
    assert all((n >= 0).all() for n in needs[1:])


@pytest.mark.parametrize("R,quick", [(192, False), (16, True)])
def test_a_window_that_holds_every_tap_is_the_single_context(oracle_built, R, quick):
    assert_numpy_keeps_subnormals()
    frames, _, _ = _oracle_sequence("hall_small", W, H, 6, True)
    par = QUICK if quick else DEFAULTS
    hist, M = None, None
    for k, ((acc, pay, alb, pv), want) in enumerate(zip(frames, _plain(quick)), start=1):
        got = group_temporal_ref(acc, pay, alb, 1, M, hist, FIVE, R, **par)
        assert _same(got, want), f"R = {R}, call {k}"
        assert _same(band_masked_ref(acc, pay, alb, 1, M, hist, FIVE, R, **par), want), f"R = {R}, call {k}, per band on a masked history"
        if quick and hist is not None:                                   # the restatement with windows that cut nothing is temporal_ref's text
            assert _same(windowed_temporal_ref(acc, pay, alb, 1, M, hist, np.zeros(H, int), np.full(H, H), **par), want)
        hist, M = got[2], pv


def test_a_window_of_four_rows_cuts_history_where_the_taps_leave_it(oracle_built):
    assert_numpy_keeps_subnormals()
    frames, _, _ = _oracle_sequence("hall_small", W, H, 6, True)
    plain, needs, R = _plain(True), _needs(), 4
    hist, M = None, None
    for k, (acc, pay, alb, pv) in enumerate(frames, start=1):
        chained = group_temporal_ref(acc, pay, alb, 1, M, hist, FIVE, R, **QUICK)
        hist, M = chained[2], pv
        differs = not bits_equal(chained[2]["N"], plain[k - 1][2]["N"]).all()
        print(f"call {k}: chained with R = 4, N differs from the single context's: {differs}")
        if k in (4, 5):
            assert differs
        if k == 1:
            assert _same(chained, plain[0])
            continue
        # the same input history as the single context's: only the window tells the two apart, pixel by pixel
        got = group_temporal_ref(acc, pay, alb, 1, frames[k - 2][3], plain[k - 2][2], FIVE, R, **QUICK)
        want, need = plain[k - 1], needs[k - 1]
        inside = need <= R
        for f in ("N", "m1", "m2", "variance", "worldPosition", "worldNormal", "filterable", "hitDistance"):
            eq = bits_equal(got[2][f], want[2][f])
            eq = eq.all(axis=-1) if eq.ndim == 3 else eq
            assert eq[inside].all(), f"call {k}: {f} differs on a pixel whose taps lie inside its window"
        cut = ~inside & (want[2]["N"] > 1)
        if k in (4, 5):
            assert cut.any() and (got[2]["N"][cut] <= want[2]["N"][cut]).all() and (got[2]["N"][cut] < want[2]["N"][cut]).any()
        # per band on a masked history: a pixel's own reprojection exactly, and all of it while no neighbour's colour enters
        masked = band_masked_ref(acc, pay, alb, 1, frames[k - 2][3], plain[k - 2][2], FIVE, R, **QUICK)
        for f in ("N", "m1", "m2", "variance"):
            assert bits_equal(masked[2][f], got[2][f]).all(), f"call {k}: {f}"
        unfiltered = dict(QUICK, iterations=0)
        assert _same(band_masked_ref(acc, pay, alb, 1, frames[k - 2][3], plain[k - 2][2], FIVE, R, **unfiltered),
                     group_temporal_ref(acc, pay, alb, 1, frames[k - 2][3], plain[k - 2][2], FIVE, R, **unfiltered)), f"call {k}"
        # a row all of whose iteration-0 taps (2 rows either side) keep their history is the single context's row in full
        far = np.array([inside[max(0, y - 2):y + 3].all() for y in range(H)])
        assert bits_equal(got[0][far], want[0][far]).all() and (got[1][far] == want[1][far]).all()
        assert struct_equal(got[2][far].ravel(), want[2][far].ravel()).all()
        if k == 6:
            assert far.all()                                             # the last move is small: four rows hold every tap
