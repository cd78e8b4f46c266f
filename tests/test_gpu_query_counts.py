"""The claim and refill arithmetic the four query families share (rt_query.h: query_body, query_simple_body), at record counts where
it can go wrong: one record, one short of / exactly / one past the 16-record minimum share and the 64 lanes of a wave, a few waves'
worth (257) and more than the static shares hold (1025).  Closest hit, occlusion, multi-hit K = 3 and nearest points K = 3, on both
kernels of tuning key 15 — the persistent one with 16 records per claim, one static chunk per wave and a 16-record minimum claim, so
that claims from the shared head start at small counts — counted and uncounted.  Every record equals the brute force over the leaf
records (bruteforce.py, multihit_ref.py, points_ref.py) bit for bit; a counted call counts N records in one launch."""
import numpy as np
import pytest

import bruteforce
import multihit_ref as mh
import points_ref as pr
from common import SCENES
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
COUNTS = (1, 15, 16, 17, 63, 64, 65, 257, 1025)
FAMILIES = ("closest", "occluded", "hits", "points")
K = 3


def make_context(sc, key15):
    ctx = capi.Context(0)
    ctx.set_tuning(15, key15)
    if key15 == 1:
        for key, value in ((4, 16), (9, 1), (10, 16)):
            ctx.set_tuning(key, value)
    ctx.upload_scene(sc)
    return ctx


def make_inputs(sc):
    """The largest count's rays, occlusion interval and points; a smaller count takes a prefix (a record's answer is its own)."""
    n = max(COUNTS)
    o, d = bruteforce.random_rays(sc, n, seed=57)
    pos = sc.world_vertices["position"].astype(np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.2
    p = np.random.default_rng(58).uniform(mid - half, mid + half, size=(n, 3)).astype(F32)
    return {"o": o, "d": d, "p": p, "tmin": F32(1e-3), "tmax": F32(0.25 * np.linalg.norm(hi - lo))}


def run_query(ctx, family, inp, n):
    """One call of `family` on the first n records: (what it returned without the stats, the stats)."""
    o, d, p = inp["o"][:n], inp["d"][:n], inp["p"][:n]
    if family == "closest":
        out = ctx.trace_rays(o, d, with_stats=True)
    elif family == "occluded":
        out = ctx.trace_rays(o, d, inp["tmin"], inp["tmax"], occluded=True, with_stats=True)
    elif family == "hits":
        out = ctx.trace_ray_hits(o, d, max_hits=K, with_stats=True)
    else:
        out = ctx.nearest_points(p, max_hits=K, with_stats=True)
    return out[:-1], out[-1]


@pytest.fixture(scope="module")
def world():
    sc = SCENES["banana_standin"][0]()
    inp = make_inputs(sc)
    ctx = make_context(sc, 2)
    bvh = ctx.export_bvh()
    ctx.close()
    ref = {"closest": bruteforce.closest(bvh, inp["o"], inp["d"]),
           "occluded": bruteforce.occluded(bvh, inp["o"], inp["d"], inp["tmin"], inp["tmax"]),
           "hits": mh.k_nearest(bvh, inp["o"], inp["d"], 0.0, np.inf, K),
           "points": pr.k_nearest(bvh, inp["p"], np.inf, K)}
    assert (ref["closest"][0] >= 0).sum() > len(inp["o"]) // 8 and 0 < ref["occluded"].sum() < len(inp["o"])
    assert (ref["hits"][1] == K).any() and (ref["points"][1] == K).all()
    return sc, inp, ref


def check_records(family, got, ref, n, tag):
    if family == "closest":
        best, _, ties = ref
        bad = bruteforce.check_closest(got[0], best[:n], ties[:n])
        assert len(got[0]) == n and bad == [], (tag, bad[:5])
    elif family == "occluded":
        assert got[0].dtype == bool and np.array_equal(got[0], ref[:n]), (tag, np.nonzero(got[0] != ref[:n])[0][:5])
    else:
        hits, counts = got
        assert hits.shape == (n, K) and counts.dtype == np.uint32
        bad = mh.record_diff(hits, ref[0][:n])
        assert len(bad) == 0, (tag, bad[:5], hits[bad[:2]], ref[0][bad[:2]])
        assert np.array_equal(counts, ref[1][:n]), (tag, np.nonzero(counts != ref[1][:n])[0][:5])


@pytest.mark.parametrize("key15", [1, 2])
@pytest.mark.parametrize("family", FAMILIES)
def test_every_count_equals_bruteforce(world, family, key15):
    sc, inp, ref = world
    ctx = make_context(sc, key15)
    for counting in (True, False):
        ctx.set_ray_counting(counting)
        for n in COUNTS:
            got, st = run_query(ctx, family, inp, n)
            check_records(family, got, ref[family], n, (family, key15, counting, n))
            assert st.launches == 1
            if counting:
                assert st.rays == n == st.part_rays[0], (family, key15, n, st.rays)
    ctx.close()
