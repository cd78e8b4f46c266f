"""Multi-hit queries (fyprt_trace_ray_hits) without a GPU: the symbols and the record's layout, the errors of both entry points in the
header's order on a host-only context, the Python wrappers' argument checks, and the brute-force reference of the GPU tests
(tests/multihit_ref.py) checked against what exists: its first hit is bruteforce.closest's, and continuation passes concatenate to
one long pass."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import bruteforce
import multihit_ref as mh
from common import SCENES
from fypraytracer_amd import capi

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
F32 = np.float32


def test_symbols_and_record_layout():
    lib = capi.load_library()
    assert {"fyprt_trace_ray_hits", "fyprt_trace_ray_hits_device"} <= set(capi.EXPORTED_SYMBOLS)
    assert hasattr(lib, "fyprt_trace_ray_hits") and hasattr(lib, "fyprt_trace_ray_hits_device")
    assert capi.RAY_HIT_DTYPE.itemsize == 16
    assert [capi.RAY_HIT_DTYPE.fields[k][1] for k in ("t", "triangle", "u", "v")] == [0, 4, 8, 12]
    header = (Path(__file__).resolve().parent.parent / "include" / "fyprt.h").read_text()
    assert int(re.search(r"#define\s+FYPRT_QUERY_MAX_HITS\s+(\d+)", header).group(1)) == capi.QUERY_MAX_HITS == 8
    assert "fyprt_trace_ray_hits_device" in header and "typedef struct fyprt_ray_hit" in header
    assert mh.UNUSED.tobytes() == np.array([-1.0], F32).tobytes() + b"\xff\xff\xff\xff" + bytes(8)


def test_errors_in_the_headers_order_on_a_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    rays = np.zeros(4, dtype=capi.RAY_DTYPE)
    rays["direction"][:, 2], rays["tmax"] = 1.0, np.inf
    hits = np.zeros((4, 8), dtype=capi.RAY_HIT_DTYPE)
    counts = np.zeros(4, dtype=np.uint32)
    dev = np.zeros(64, dtype=np.float32)                      # (never dereferenced: every call below fails before a launch)
    base = dev.ctypes.data + (-dev.ctypes.data) % 16          # a 16-byte aligned address inside it

    def host(k=4, r=rays.ctypes.data, n=4, h=hits.ctypes.data, c=counts.ctypes.data, a=None):
        return lib.fyprt_trace_ray_hits(ctx.h, r, a, n, k, h, c, None)

    def device(k=4, r=base, n=4, h=base, c=base, a=None):
        return lib.fyprt_trace_ray_hits_device(ctx.h, r, a, n, k, h, c)

    for call in (host, device):
        assert call() == ESTATE                                               # no scene yet
        assert call(c=None) == ESTATE                                         # hit_counts may be NULL
        for k in (0, 9):
            assert call(k=k) == EINVAL                                        # max_hits before the state ...
            assert call(k=k, r=None) == EINVAL
            assert call(k=k, n=0) == EINVAL                                   # ... and before the empty call
        assert call(r=None) == EINVAL and call(h=None) == EINVAL              # NULL rays / hits with count > 0
        assert call(k=1) == ESTATE and call(k=8) == ESTATE
    for bad in (dict(r=base + 4), dict(a=base + 8), dict(h=base + 4), dict(c=base + 2)):
        assert device(**bad) == EINVAL, bad                                   # misaligned device pointers: refused before the state
    assert device(c=base + 4, a=base + 16) == ESTATE                          # counts need 4 bytes only
    ctx.upload_scene(SCENES["cornell"][0]())
    for call in (host, device):
        assert call() == ESTATE                                               # a host-only context cannot trace
        assert call(k=0) == EINVAL and call(k=9) == EINVAL and call(r=None) == EINVAL and call(h=None) == EINVAL
        assert call(n=0) == ESTATE                                            # the state comes before the empty call
    assert device(h=base + 8) == EINVAL
    assert lib.fyprt_trace_ray_hits(None, rays.ctypes.data, None, 4, 4, hits.ctypes.data, None, None) == EINVAL
    assert lib.fyprt_trace_ray_hits_device(None, None, None, 0, 4, None, None) == EINVAL
    with pytest.raises(capi.FyprtError):
        ctx.trace_ray_hits(np.zeros((1, 3)), np.ones((1, 3)))
    ctx.close()


class _NoLibrary:
    """Stands in for the loaded library: any call into it is a failure of the wrapper's own checks."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrappers_check_arguments_before_the_library_is_called():
    ctx = capi.Context(-1)
    real = ctx.lib
    ctx.lib = _NoLibrary()
    try:
        o, d = np.zeros((3, 3), F32), np.ones((3, 3), F32)
        for bad in (0, 9, -1, 2.5, True, None):
            with pytest.raises(ValueError):
                ctx.trace_ray_hits(o, d, max_hits=bad)
            with pytest.raises(ValueError):
                ctx.trace_all_hits(o, d, max_hits=bad)
            with pytest.raises(ValueError):
                ctx.trace_ray_hits_tensor(None, bad)
        with pytest.raises(ValueError):
            ctx.trace_ray_hits(o, d[:2])
        with pytest.raises(ValueError):
            ctx.trace_all_hits(o, d[:2])
        with pytest.raises(ValueError):
            ctx.trace_ray_hits(o, d, after=np.zeros(2, dtype=capi.RAY_HIT_DTYPE))          # wrong length
        with pytest.raises(ValueError):
            ctx.trace_ray_hits(o, d, after=np.zeros((3, 4), dtype=F32))                    # wrong dtype
        import torch
        for rays in (torch.zeros(4, 7), torch.zeros(4, 8, dtype=torch.float64), torch.zeros(8, 4).t(), torch.zeros(4, 8)):   # the last: not on the GPU
            with pytest.raises(ValueError):
                ctx.trace_ray_hits_tensor(rays, 4)
    finally:
        ctx.lib = real
    ctx.close()


def _cases():
    """(name, bvh, origins, directions): cornell with random rays and the layers scene with its own."""
    out = []
    for name in ("cornell", "layers"):
        sc = SCENES[name][0]() if name == "cornell" else mh.layers_scene()
        ctx = capi.Context(-1)
        ctx.upload_scene(sc)
        bvh = ctx.export_bvh()
        ctx.close()
        o, d = bruteforce.random_rays(sc, 300, seed=5) if name == "cornell" else mh.layers_rays(300)
        out.append((name, bvh, o, d))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_first_hit_is_the_closest_querys(cases):
    for name, bvh, o, d in cases:
        for lo, hi in ((0.0, np.inf), (0.3, 2.5)):
            hits, counts, totals = mh.k_nearest(bvh, o, d, lo, hi, 1)
            best, _, ties = bruteforce.closest(bvh, o, d, lo, hi)
            assert np.array_equal(counts > 0, best >= 0) and np.array_equal(counts, np.minimum(totals, 1)), name
            assert 0 < (counts > 0).sum()
            for i in range(len(o)):
                if counts[i]:
                    assert hits["t"][i, 0].view(np.uint32) == best[i].view(np.uint32), (name, i)
                    assert int(hits["triangle"][i, 0]) == min(ties[i]), (name, i)
                else:
                    assert hits[i, 0] == mh.UNUSED
        if name == "layers":
            assert any(len(t) > 1 for t in ties)                              # the coplanar copies do tie


def test_continuation_passes_concatenate_to_one_pass(cases):
    for name, bvh, o, d in cases:
        _, _, totals = mh.k_nearest(bvh, o, d, 0.0, np.inf, 1)
        kmax = int(totals.max())
        assert kmax > 3, name
        full, full_counts, _ = mh.k_nearest(bvh, o, d, 0.0, np.inf, kmax)
        assert np.array_equal(full_counts, totals)
        keys = mh.hit_keys(full)
        for i in range(len(o)):
            assert (np.diff(keys[i, :totals[i]].astype(object)) > 0).all()    # strictly ascending: no hit twice
        got = [[] for _ in range(len(o))]
        after, passes = None, 0
        while True:
            hits, counts, _ = mh.k_nearest(bvh, o, d, 0.0, np.inf, 3, after=after)
            if not counts.any():
                break
            for i in np.nonzero(counts)[0]:
                got[i].append(hits[i, :counts[i]])
            after = hits[:, 2].copy()                                         # the last record, unused ones included: those rays are finished
            passes += 1
        assert passes == -(-kmax // 3)
        for i in range(len(o)):
            cat = np.concatenate(got[i]) if got[i] else np.empty(0, dtype=capi.RAY_HIT_DTYPE)
            assert mh.records_equal(cat, full[i, :totals[i]]), (name, i)
        flat, offsets = mh.all_hits(bvh, o, d, 0.0, np.inf)
        assert np.array_equal(np.diff(offsets), totals) and mh.records_equal(flat[offsets[7]:offsets[8]], full[7, :totals[7]])
