"""Tuning key 25 (kept primary hits of ReSTIR DI frames) and its readout on a host-only context: the key is accepted and range-checked as on
a device, and a context that never renders reports no kept frame."""
import ctypes as C

import pytest

from fypraytracer_amd import capi

EINVAL = -1


def test_host_only_context_accepts_key_25():
    ctx = capi.Context(-1)
    assert ctx.get_tuning(25) == 1                       # keeping is the default
    ctx.set_tuning(25, 0)
    assert ctx.get_tuning(25) == 0
    with pytest.raises(capi.FyprtError, match="0..1"):
        ctx.set_tuning(25, 2)
    assert ctx.lib.fyprt_set_tuning(ctx.h, 25, -1) == EINVAL
    assert ctx.get_tuning(25) == 0
    ctx.set_tuning(25, 1)
    assert ctx.get_tuning(25) == 1
    for key, value in ((23, 1), (24, 0), (24, 1)):       # key 23 stays reserved, 24 unassigned (the tuning tests assert it is refused)
        with pytest.raises(capi.FyprtError):
            ctx.set_tuning(key, value)
    assert ctx.lib.fyprt_set_tuning(ctx.h, 26, 0) == EINVAL
    ctx.close()


def test_kept_primary_frames_is_zero_without_a_device():
    ctx = capi.Context(-1)
    assert ctx.kept_primary_frames() == 0
    n = C.c_uint64(7)
    assert ctx.lib.fyprt_kept_primary_frames(None, C.byref(n)) == EINVAL
    assert ctx.lib.fyprt_kept_primary_frames(ctx.h, None) == EINVAL
    assert "fyprt_kept_primary_frames" in capi.EXPORTED_SYMBOLS
    ctx.close()
