"""Batched ray queries (fyprt_trace_rays) without a GPU: the ray record's layout, the argument / state errors of both entry points on
a host-only context, and the brute-force reference of the GPU query tests (tests/bruteforce.py) pinned against the oracle's twin of
the product traversal (Oracle.trace on ctx.export_bvh()), so that the GPU tests compare against a reference that is itself checked."""
import ctypes as C

import numpy as np
import pytest

import bruteforce
from common import SCENES
from fypraytracer_amd import capi

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE


def test_ray_dtype_matches_fyprt_ray():
    assert capi.RAY_DTYPE.itemsize == 32
    assert [capi.RAY_DTYPE.fields[k][1] for k in ("origin", "tmin", "direction", "tmax")] == [0, 12, 16, 28]
    assert (capi.QUERY_CLOSEST, capi.QUERY_OCCLUDED) == (0, 1)
    assert {"fyprt_trace_rays", "fyprt_trace_rays_device"} <= set(capi.EXPORTED_SYMBOLS)


def test_query_errors_on_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    rays = np.zeros(4, dtype=capi.RAY_DTYPE)
    rays["direction"][:, 2], rays["tmax"] = 1.0, np.inf
    out = np.zeros(4, dtype=capi.PAYLOAD_DTYPE)
    dev = np.zeros(16, dtype=np.float32)                      # (never dereferenced: every call below fails before a launch)

    def host(kind, r=rays.ctypes.data, n=4, o=out.ctypes.data):
        return lib.fyprt_trace_rays(ctx.h, kind, r, n, o, None)

    def device(kind, r=dev.ctypes.data, n=4, o=dev.ctypes.data):
        return lib.fyprt_trace_rays_device(ctx.h, kind, r, n, o)

    for call in (host, device):
        assert call(capi.QUERY_CLOSEST) == ESTATE                             # no scene yet
        assert call(capi.QUERY_OCCLUDED) == ESTATE
    ctx.upload_scene(SCENES["cornell"][0]())
    for call in (host, device):
        assert call(capi.QUERY_CLOSEST) == ESTATE                             # a host-only context cannot trace
        assert call(2) == EINVAL and call(-1) == EINVAL                       # unknown query kind
        assert call(capi.QUERY_CLOSEST, r=None) == EINVAL                     # NULL rays with count > 0
        assert call(capi.QUERY_OCCLUDED, o=None) == EINVAL                    # NULL results with count > 0
    assert device(capi.QUERY_CLOSEST, r=dev.ctypes.data + 4) == EINVAL        # misaligned device pointers: refused before the state
    assert device(capi.QUERY_CLOSEST, o=dev.ctypes.data + 4) == EINVAL
    assert lib.fyprt_trace_rays(None, capi.QUERY_CLOSEST, rays.ctypes.data, 4, out.ctypes.data, None) == EINVAL
    assert lib.fyprt_trace_rays_device(None, capi.QUERY_CLOSEST, None, 0, None) == EINVAL
    with pytest.raises(capi.FyprtError):
        ctx.trace_rays(np.zeros((1, 3)), np.ones((1, 3)))
    ctx.close()


@pytest.mark.parametrize("name", ["cornell", "hall_small"])
def test_bruteforce_matches_oracle_product_trace(oracle_built, name):
    """4 000 random rays: the brute force's closest accepted t equals the oracle's twin of the product traversal bit for bit, and the
    oracle's triangle is one of the brute force's exact-t ties (a tree may find any of them first)."""
    from oraclelib import Oracle
    mk_scene, mk_cam = SCENES[name]
    sc = mk_scene()
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    bvh = ctx.export_bvh()
    orc = Oracle(sc, 8, 8)
    orc.use_product_bvh(bvh)
    o, d = bruteforce.random_rays(sc, 4000, seed=11 if name == "cornell" else 12)
    pay = np.zeros(len(o), dtype=capi.PAYLOAD_DTYPE)
    for i in range(len(o)):
        pay[i] = orc.trace(o[i], d[i])[0]
    best, tri, ties = bruteforce.closest(bvh, o, d)
    assert bruteforce.check_closest(pay, best, ties) == []
    hits = int((best >= 0).sum())
    assert 0.2 * len(o) < hits                                               # the rays do hit things
    occ = bruteforce.occluded(bvh, o, d, 0.0, np.inf)
    assert np.array_equal(occ, best >= 0)
    orc.close()
    ctx.close()
