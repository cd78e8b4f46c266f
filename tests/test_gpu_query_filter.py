"""Query filters on the GPU (fyprt_set_mesh_query_masks / fyprt_set_query_mask, rt_filter.h and the filtered lane states of rt_query.h,
rt_points.h, rt_boxes.h).  Every comparison is bit for bit: each family's existing brute force (bruteforce, multihit_ref, points_ref,
boxes_ref) run over the admitted leaf records of ctx.export_bvh() alone (tests/filter_ref.py) — records, unused slots, counts, totals.
  * the stack of coplanar layers under a table of group bits and eight query masks, all four families, both kernels of tuning key 15,
    several K, the continuation loops; the duplicated layers carry bit 2 on BOTH copies, so that the mask that admits only them leaves
    every pair tied and the masks that exclude the copies leave none;
  * hall_small under the three builders with a seeded random word per mesh, about 2 000 records per family; the persistent kernel's
    claims at small record counts; a twin context that removed the meshes instead; counters on hand-countable trees; on and off; scene
    edits on the device; stack budget extremes; frames and radiance queries untouched; the tensor path; device memory; errors."""
import ctypes as C

import numpy as np
import pytest

import boxes_ref as br
import bruteforce as bf
import filter_ref as fr
import multihit_ref as mh
import points_ref as pr
from append_common import append_patch
from common import SCENES, bits_equal, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = 0xFFFFFFFF
NOTHING = 0x80000000            # a bit no table of these tests sets
EINVAL, ESTATE = -1, -3


def _ctx(sc, key15=0, counting=False, builder=0):
    ctx = capi.Context(0)
    ctx.set_tuning(15, key15)
    ctx.set_tuning(12, builder)
    ctx.upload_scene(sc)
    ctx.set_ray_counting(counting)
    return ctx


def _host_export(sc):
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    return bvh


def _same_leaf_records(a, b):
    ka, kb = np.argsort(a["tris"]["tri"]), np.argsort(b["tris"]["tri"])
    return all(np.array_equal(a["tris"][f][ka].view(np.uint32), b["tris"][f][kb].view(np.uint32)) for f in ("v0", "e1", "e2", "tri"))


def _scene_box(sc):
    p = sc.world_vertices["position"].astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


class Inputs:
    """The records of the four families for one scene: rays (o, d) with the occlusion query's interval, points with a radius, boxes."""
    def __init__(self, o, d, tmin, tmax, p, radius, lo, hi):
        self.o, self.d, self.tmin, self.tmax, self.p, self.radius, self.lo, self.hi = o, d, F32(tmin), F32(tmax), p, F32(radius), lo, hi

    def head(self, n):
        return Inputs(self.o[:n], self.d[:n], self.tmin, self.tmax, self.p[:n], self.radius, self.lo[:n], self.hi[:n])


class Reference:
    """The filtered brute force of every family on `bvh` for (meshes, M, Q), each computed on first use at the largest K and kept."""
    def __init__(self, bvh, meshes, M, Q, inp, k_list=8, k_box=32, box_cache=None):
        self.fb, self.inp, self.k_list, self.k_box, self.memo = fr.filtered(bvh, meshes, M, Q), inp, k_list, k_box, {}
        self.bvh, self.adm, self.box_cache = bvh, fr.admitted(bvh, meshes, M, Q), box_cache
        self.admitted = int(self.adm.sum())

    def _get(self, name, make):
        if name not in self.memo:
            self.memo[name] = make()
        return self.memo[name]

    def closest(self):
        if self.admitted == 0:                                                # (bruteforce.closest reduces over the records: none, every ray misses)
            n = len(self.inp.o)
            return np.full(n, -1.0, dtype=F32), np.full(n, -1, dtype=np.int64), [frozenset()] * n
        return self._get("closest", lambda: bf.closest(self.fb, self.inp.o, self.inp.d))

    def occluded(self):
        return self._get("occluded", lambda: bf.occluded(self.fb, self.inp.o, self.inp.d, self.inp.tmin, self.inp.tmax))

    def hits(self, k):
        h, _, totals = self._get("hits", lambda: mh.k_nearest(self.fb, self.inp.o, self.inp.d, 0.0, np.inf, self.k_list))
        return np.ascontiguousarray(h[:, :k]), np.minimum(totals, k).astype(np.uint32)

    def points(self, k):
        h, _, totals = self._get("points", lambda: pr.k_nearest(self.fb, self.inp.p, self.inp.radius, self.k_list))
        return np.ascontiguousarray(h[:, :k]), np.minimum(totals, k).astype(np.uint32)

    def _box_decisions(self):
        """boxes_ref.accepted on the admitted records; with a `box_cache` (a dict shared by the references of one tree and one box set)
        the separating-axis test runs once over every record and each mask takes its columns."""
        if self.box_cache is None:
            return None
        if "ok_ids" not in self.box_cache:
            self.box_cache["ok_ids"] = br.accepted(self.bvh, self.inp.lo, self.inp.hi)
        ok, ids = self.box_cache["ok_ids"]
        return np.ascontiguousarray(ok[:, self.adm]), ids[self.adm]

    def boxes(self, k):
        t, _, totals = self._get("boxes", lambda: br.k_lowest(self.fb, self.inp.lo, self.inp.hi, self.k_box, ok_ids=self._box_decisions()))
        return np.ascontiguousarray(t[:, :k]), np.minimum(totals, k).astype(np.uint32), totals


def _check_closest(ctx, ref, tag, n=None):
    inp = ref.inp if n is None else ref.inp.head(n)
    best, _, ties = ref.closest()
    pay = ctx.trace_rays(inp.o, inp.d)
    bad = bf.check_closest(pay, best[:len(pay)], ties[:len(pay)])
    assert not bad, (tag, "closest", len(bad), bad[:8])
    return pay


def _check_occluded(ctx, ref, tag, n=None):
    inp = ref.inp if n is None else ref.inp.head(n)
    got = ctx.trace_rays(inp.o, inp.d, inp.tmin, inp.tmax, occluded=True)
    want = ref.occluded()[:len(got)]
    assert got.dtype == bool and np.array_equal(got, want), (tag, "occluded", np.nonzero(got != want)[0][:8])


def _check_list(got, want, tag):
    (gh, gc), (wh, wc) = got[:2], want[:2]
    assert gh.shape == wh.shape and gc.dtype == np.uint32
    bad = mh.record_diff(gh, wh)
    assert len(bad) == 0, (tag, len(bad), bad[:8], gh[bad[:2]], wh[bad[:2]])
    assert np.array_equal(gc, wc), (tag, np.nonzero(gc != wc)[0][:8])


def _check_hits(ctx, ref, k, tag, n=None):
    inp = ref.inp if n is None else ref.inp.head(n)
    got = ctx.trace_ray_hits(inp.o, inp.d, max_hits=k)
    wh, wc = ref.hits(k)
    _check_list(got, (wh[:len(inp.o)], wc[:len(inp.o)]), (tag, "hits", k))
    return got


def _check_points(ctx, ref, k, tag, n=None):
    inp = ref.inp if n is None else ref.inp.head(n)
    got = ctx.nearest_points(inp.p, inp.radius, max_hits=k)
    wh, wc = ref.points(k)
    _check_list(got, (wh[:len(inp.p)], wc[:len(inp.p)]), (tag, "points", k))
    return got


def _check_boxes(ctx, ref, k, tag, n=None):
    inp = ref.inp if n is None else ref.inp.head(n)
    gt, gc, gn = ctx.overlap_boxes(inp.lo, inp.hi, max_hits=k)
    wt, wc, wn = (a[:len(inp.lo)] for a in ref.boxes(k))
    assert gt.shape == wt.shape and gt.dtype == np.uint32
    bad = np.nonzero((gt != wt).any(axis=1))[0]
    assert len(bad) == 0, (tag, "boxes", k, len(bad), bad[:8], gt[bad[:2]], wt[bad[:2]])
    assert np.array_equal(gc, wc) and np.array_equal(gn, wn), (tag, "boxes", k)
    return gt, gc, gn


def _check_families(ctx, ref, tag, k_list=4, k_box=8):
    _check_closest(ctx, ref, tag)
    _check_occluded(ctx, ref, tag)
    _check_hits(ctx, ref, k_list, tag)
    _check_points(ctx, ref, k_list, tag)
    _check_boxes(ctx, ref, k_box, tag)


# ---- 1. the layers scene: 12 layers as meshes 0-11, the copies of layers 0, 4 and 7 as meshes 12-14; mesh m = triangles 2m, 2m + 1
COPY_OF = {12: 0, 13: 4, 14: 7}
LAYER_QS = (1, 2, 4, 3, 5, 7, NOTHING, ALL)


def _layers_table():
    """Bit 0 on even layers, bit 1 on odd ones, bit 2 on the three duplicated layers (the copies carry nothing else, their originals keep
    their parity bit), and layer 5 with mask 0: no query sees it."""
    M = np.array([1 if j % 2 == 0 else 2 for j in range(12)] + [4, 4, 4], dtype=np.uint32)
    for original in COPY_OF.values():
        M[original] |= 4
    M[5] = 0
    return M


def _copy_ties(values, triangles, counts):
    """Per list, the number of pairs of entries at the same value bits whose triangles are a copy and its original."""
    vb = np.ascontiguousarray(values).view(np.uint32)
    out = np.zeros(len(counts), dtype=np.int64)
    for i, c in enumerate(counts):
        for a in range(int(c)):
            for b in range(a + 1, int(c)):
                ma, mb = int(triangles[i, a]) // 2, int(triangles[i, b]) // 2
                if vb[i, a] == vb[i, b] and (COPY_OF.get(mb) == ma or COPY_OF.get(ma) == mb) and triangles[i, a] % 2 == triangles[i, b] % 2:
                    out[i] += 1
    return out


@pytest.fixture(scope="module")
def layers():
    from test_gpu_boxes import _layers_boxes
    sc = mh.layers_scene()
    o, d = mh.layers_rays(300, seed=11)
    rng = np.random.default_rng(23)
    p = np.stack([rng.uniform(-1.6, 1.6, 250), rng.uniform(-3.2, 0.6, 250), rng.uniform(-1.6, 1.6, 250)], 1).astype(F32)
    p[:40, 1] = F32(-0.25) * rng.integers(0, 12, 40).astype(F32)             # some exactly on a layer: distance2 = +0
    lo, hi = _layers_boxes()
    lo, hi = lo[::2], hi[::2]
    inp = Inputs(o, d, 0.0, 2.0, p, 1.0, lo, hi)
    bvh = _host_export(sc)
    M = _layers_table()
    assert len(sc.meshes) == 15 and len(bvh["tris"]) == 30 and [m[0] for m in sc.meshes] == list(range(0, 30, 2))
    refs = {Q: Reference(bvh, sc.meshes, M, Q, inp) for Q in LAYER_QS}
    assert [refs[Q].admitted for Q in LAYER_QS] == [12, 10, 12, 22, 20, 28, 0, 28]
    return sc, inp, bvh, M, refs


@pytest.mark.parametrize("key15", [1, 2])
def test_layers_every_mask_every_family(layers, key15):
    sc, inp, bvh, M, refs = layers
    ctx = _ctx(sc, key15)
    assert _same_leaf_records(ctx.export_bvh(), bvh)
    ctx.set_mesh_query_masks(M)
    for Q in LAYER_QS:
        ctx.set_query_mask(Q)
        ref, tag = refs[Q], (key15, hex(Q))
        _check_closest(ctx, ref, tag)
        _check_occluded(ctx, ref, tag)
        for k in (1, 3, 8):
            hits = _check_hits(ctx, ref, k, tag)
            near = _check_points(ctx, ref, k, tag)
            if k == 8 and Q in (3, 4):
                # the inputs exercise what they are for: with the copies excluded (Q = 3) no list holds a copy and its original at one
                # value; with only the duplicated layers admitted (Q = 4) every list of two or more does
                for name, (rec, counts), field in (("hits", hits, "t"), ("points", near, "distance2")):
                    ties = _copy_ties(rec[field], rec["triangle"], counts)
                    many = counts >= 2
                    assert many.sum() > 50, (name, Q)
                    assert (ties[many] == 0).all() if Q == 3 else (ties[many] >= 1).all(), (name, Q)
        for k in (1, 8, 32):
            _check_boxes(ctx, ref, k, tag)
        if Q == NOTHING:
            assert not ctx.trace_rays(inp.o, inp.d, occluded=True).any() and (ctx.trace_rays(inp.o, inp.d)["objectIndex"] == -1).all()
            assert (ctx.overlap_boxes(inp.lo, inp.hi, max_hits=4)[2] == 0).all()
    ctx.close()


@pytest.mark.parametrize("key15", [1, 2])
def test_layers_continuation_enumerates_the_admitted_set(layers, key15):
    sc, inp, bvh, M, refs = layers
    ctx = _ctx(sc, key15)
    ctx.set_mesh_query_masks(M)
    for Q in (3, 5, NOTHING, ALL):
        ctx.set_query_mask(Q)
        fb = refs[Q].fb
        got, off = ctx.trace_all_hits(inp.o, inp.d, max_hits=3)
        want, want_off = mh.all_hits(fb, inp.o, inp.d, 0.0, np.inf)
        assert np.array_equal(off, want_off) and mh.records_equal(got, want), (key15, hex(Q), "hits")
        got, off = ctx.triangles_within(inp.p, 0.8, max_hits=3)
        want, want_off = pr.all_within(fb, inp.p, F32(0.8))
        assert np.array_equal(off, want_off) and mh.records_equal(got, want), (key15, hex(Q), "points")
        got, off = ctx.triangles_in_boxes(inp.lo, inp.hi, max_hits=3)
        want, want_off = br.all_in_boxes(fb, inp.lo, inp.hi)
        assert np.array_equal(off, want_off) and np.array_equal(got, want), (key15, hex(Q), "boxes")
        if Q == 5:
            assert np.diff(want_off).max() > 9                               # several passes per box
    ctx.close()


# ---- 2. hall_small: a seeded random word per mesh, about 2 000 records per family
HALL_QS = (1 << 7, 0x00010008, ALL)


def _hall_inputs(sc, n=2000):
    from test_gpu_boxes import _uniform_boxes
    rng = np.random.default_rng(91)
    o, d = bf.random_rays(sc, n, 47)
    lo, hi = _scene_box(sc)
    uniform = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), size=(n // 2, 3))
    verts = sc.world_vertices["position"][rng.integers(0, len(sc.world_vertices), n - n // 2)].astype(np.float64)
    on_surface = verts + rng.normal(scale=0.01, size=verts.shape) * (rng.integers(0, 2, (len(verts), 1)) == 1)     # half of them exactly on a vertex
    p = np.concatenate([on_surface, uniform]).astype(F32)
    blo, bhi = _uniform_boxes(sc, n - 4, 39, scale=1.2)
    blo = np.concatenate([blo, np.tile((lo - 1).astype(F32), (4, 1))]).astype(F32)
    bhi = np.concatenate([bhi, np.tile((hi + 1).astype(F32), (4, 1))]).astype(F32)
    return Inputs(o, d, 0.0, 1.5, p, 0.5, blo, bhi)


def _hall_table(n_meshes, seed=101):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n_meshes, dtype=np.uint64).astype(np.uint32)


@pytest.fixture(scope="module")
def hall():
    sc = SCENES["hall_small"][0]()
    inp = _hall_inputs(sc)
    bvh = _host_export(sc)
    M = _hall_table(len(sc.meshes))
    cache = {}
    refs = {Q: Reference(bvh, sc.meshes, M, Q, inp, k_list=4, k_box=8, box_cache=cache) for Q in HALL_QS}
    counts = [refs[Q].admitted for Q in HALL_QS]
    assert 0 < counts[0] < counts[1] < counts[2] <= len(bvh["tris"]), counts  # each mask admits a different part of the scene
    return sc, inp, bvh, M, refs


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_hall_small_equals_filtered_bruteforce(hall, builder):
    sc, inp, bvh, M, refs = hall
    for key15 in (1, 2):
        ctx = _ctx(sc, key15, builder=builder)
        assert _same_leaf_records(ctx.export_bvh(), bvh)                      # the references are functions of the leaf records alone
        ctx.set_mesh_query_masks(M)
        for Q in HALL_QS:
            ctx.set_query_mask(Q)
            _check_families(ctx, refs[Q], (builder, key15, hex(Q)))
        assert ctx.query_filter()[2] == 1                                     # built once: a new Q builds nothing
        ctx.close()


@pytest.mark.parametrize("n, family", [(1, "closest"), (63, "occluded"), (64, "hits"), (65, "points"), (257, "boxes")])
def test_persistent_kernel_claims_at_small_counts(hall, n, family):
    sc, inp, bvh, M, refs = hall
    ctx = _ctx(sc, key15=1)
    ctx.set_mesh_query_masks(M)
    ctx.set_query_mask(HALL_QS[1])
    ref = refs[HALL_QS[1]]
    {"closest": lambda: _check_closest(ctx, ref, n, n), "occluded": lambda: _check_occluded(ctx, ref, n, n), "hits": lambda: _check_hits(ctx, ref, 4, n, n),
     "points": lambda: _check_points(ctx, ref, 4, n, n), "boxes": lambda: _check_boxes(ctx, ref, 8, n, n)}[family]()
    ctx.close()


# ---- 3. the twin: a context that removed the meshes the filter does not admit
def test_twin_that_removed_the_meshes(hall):
    sc, inp, bvh, M, refs = hall
    Q = HALL_QS[1]
    kept = (M & np.uint32(Q)) != 0
    new_index = fr.renumbering(sc.meshes, kept)
    a = _ctx(sc, key15=1)
    a.set_mesh_query_masks(M)
    a.set_query_mask(Q)
    twin_scene = SCENES["hall_small"][0]()
    b = _ctx(twin_scene, key15=1)
    b.remove_meshes(twin_scene.remove_meshes_from_scene([m for m in range(len(kept)) if not kept[m]]))
    assert len(twin_scene.triangles) == int((new_index >= 0).sum())

    def mapped(tri):
        out = tri.copy()
        used = tri != np.uint32(ALL)
        out[used] = new_index[tri[used]].astype(np.uint32)
        assert (new_index[tri[used]] >= 0).all()
        return out
    n = 1000
    ha, ca = a.trace_ray_hits(inp.o[:n], inp.d[:n], max_hits=4)
    hb, cb = b.trace_ray_hits(inp.o[:n], inp.d[:n], max_hits=4)
    ha["triangle"] = mapped(ha["triangle"])
    assert mh.records_equal(ha, hb) and np.array_equal(ca, cb) and ca.sum() > n // 2
    pa, ca = a.nearest_points(inp.p[:n], inp.radius, max_hits=4)
    pb, cb = b.nearest_points(inp.p[:n], inp.radius, max_hits=4)
    pa["triangle"] = mapped(pa["triangle"])
    assert mh.records_equal(pa, pb) and np.array_equal(ca, cb) and ca.sum() > n // 2
    ta, ca, na = a.overlap_boxes(inp.lo[:n], inp.hi[:n], max_hits=8)
    tb, cb, nb = b.overlap_boxes(inp.lo[:n], inp.hi[:n], max_hits=8)
    assert np.array_equal(mapped(ta), tb) and np.array_equal(ca, cb) and np.array_equal(na, nb) and ca.sum() > n // 2
    assert np.array_equal(a.trace_rays(inp.o, inp.d, inp.tmin, inp.tmax, occluded=True), b.trace_rays(inp.o, inp.d, inp.tmin, inp.tmax, occluded=True))
    # closest hits: every field but objectIndex (mapped), where the brute force's tie set has one member — two trees may order a tie
    # differently.  The brute force alone shows that this covers at least 95 % of the rays that hit
    best, _, ties = refs[Q].closest()
    hit = best >= 0
    single = hit & np.array([len(t) == 1 for t in ties])
    assert hit.sum() > 1000 and single.sum() >= 0.95 * hit.sum(), (hit.sum(), single.sum())
    ya, yb = a.trace_rays(inp.o, inp.d), b.trace_rays(inp.o, inp.d)
    assert np.array_equal(new_index[ya["objectIndex"][single]], yb["objectIndex"][single])
    for f in ya.dtype.names:
        if f != "objectIndex":
            assert bits_equal(ya[f][single], yb[f][single]).all(), f
    a.close(); b.close()


# ---- 4. counters
@pytest.mark.parametrize("key15", [1, 2])
def test_counters_follow_the_masks(key15):
    sc = SCENES["cornell"][0]()
    ctx = _ctx(sc, key15, counting=True)
    bvh = ctx.export_bvh()
    M = np.array([1, 2, 4, 8, 3, 16, 32, 5], dtype=np.uint32)
    assert len(sc.meshes) == len(M)
    lm = fr.leaf_masks(bvh, sc.meshes, M)
    nm, reached = fr.node_masks(bvh, lm), fr.node_masks_by_sets(bvh, lm)[1]
    assert reached.all()
    lo, hi = np.full((1, 3), -9, F32), np.full((1, 3), 9, F32)                # one box around everything
    plain = ctx.overlap_boxes(lo, hi, max_hits=8, with_stats=True)
    ctx.set_mesh_query_masks(M)
    for Q in (1, 16, 4 | 32, 7, ALL):
        ctx.set_query_mask(Q)
        tris, counts, totals, st = ctx.overlap_boxes(lo, hi, max_hits=8, with_stats=True)
        met = (nm & np.uint32(Q)) != 0
        admitted = int(((lm & np.uint32(Q)) != 0).sum())
        children = sum(int(n["meta"]) & 7 for n in bvh["nodes"][met])
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (1, children, admitted, 1, int(met.sum())), (key15, hex(Q))
        assert totals[0] == admitted
    # a mask that admits nothing: every record is counted, nothing is fetched or tested
    ctx.set_query_mask(NOTHING)
    o, d = bf.random_rays(sc, 70, 5)
    p = ((o + d) * F32(0.5)).astype(F32)
    blo, bhi = (p - F32(0.3)).astype(F32), (p + F32(0.3)).astype(F32)
    for st in (ctx.trace_rays(o, d, with_stats=True)[1], ctx.trace_rays(o, d, occluded=True, with_stats=True)[1], ctx.trace_ray_hits(o, d, max_hits=4, with_stats=True)[2],
               ctx.nearest_points(p, max_hits=4, with_stats=True)[2], ctx.overlap_boxes(blo, bhi, max_hits=4, with_stats=True)[3]):
        assert (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits) == (70, 0, 0, 0, 0)
    # a table and a mask of all ones: the answers and the counters of the unfiltered kernels
    unfiltered = capi.Context(0)
    unfiltered.set_tuning(15, key15)
    unfiltered.upload_scene(sc)
    unfiltered.set_ray_counting(True)
    ctx.set_mesh_query_masks(np.full(len(M), ALL, dtype=np.uint32))
    ctx.set_query_mask(ALL)
    runs = []
    for c in (unfiltered, ctx):
        r = [c.trace_rays(o, d, with_stats=True), c.trace_rays(o, d, 0.0, 1.0, occluded=True, with_stats=True), c.trace_ray_hits(o, d, max_hits=4, with_stats=True),
             c.nearest_points(p, max_hits=4, with_stats=True), c.overlap_boxes(blo, bhi, max_hits=4, with_stats=True)]
        runs.append(r)
    for ra, rb in zip(*runs):
        for xa, xb in zip(ra[:-1], rb[:-1]):
            assert xa.tobytes() == xb.tobytes()
        sa, sb = ra[-1], rb[-1]
        assert (sa.rays, sa.box_tests, sa.tri_tests, sa.hits, sa.node_visits) == (sb.rays, sb.box_tests, sb.tri_tests, sb.hits, sb.node_visits)
        assert sa.tri_tests > 0
    assert plain[0].tobytes() == ctx.overlap_boxes(lo, hi, max_hits=8)[0].tobytes()
    assert unfiltered.query_filter()[2] == 0
    unfiltered.close(); ctx.close()


# ---- 5. on and off
def test_set_then_clear_is_a_context_that_never_set(hall):
    sc, inp, bvh, M, refs = hall
    inp = inp.head(500)
    never, ctx = _ctx(sc), _ctx(sc)
    ctx.set_mesh_query_masks(M)
    ctx.set_query_mask(HALL_QS[0])
    assert ctx.query_filter()[2] == 0                                         # nothing is built before a query asks
    assert not np.array_equal(ctx.overlap_boxes(inp.lo, inp.hi, max_hits=8)[0], never.overlap_boxes(inp.lo, inp.hi, max_hits=8)[0])
    assert ctx.query_filter()[2] == 1
    ctx.set_mesh_query_masks(None)                                            # Q stays at a single bit: without a table it means nothing
    for c in (never, ctx):
        c.answers = [c.trace_rays(inp.o, inp.d), c.trace_rays(inp.o, inp.d, inp.tmin, inp.tmax, occluded=True), *c.trace_ray_hits(inp.o, inp.d, max_hits=4),
                     *c.nearest_points(inp.p, inp.radius, max_hits=4), *c.overlap_boxes(inp.lo, inp.hi, max_hits=8)]
    for x, y in zip(never.answers, ctx.answers):
        assert x.tobytes() == y.tobytes()
    assert ctx.query_filter() == (None, HALL_QS[0], 1) and never.query_filter() == (None, ALL, 0)      # builds does not move while the filter is off
    ctx.set_mesh_query_masks(M)
    _check_boxes(ctx, refs[HALL_QS[0]], 8, "on again", 500)
    assert ctx.query_filter()[2] == 2
    never.close(); ctx.close()


# ---- 6. edits on the device
def test_filter_follows_scene_edits():
    mk_scene, mk_cam = SCENES["hall_small"]
    sc, cam = mk_scene(), mk_cam(64, 64)
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    ctx = _ctx(sc)
    ctx.set_object_vertices(sc)
    inp = _hall_inputs(sc, 300)
    M = _hall_table(len(sc.meshes), seed=7)
    M &= np.uint32(ALL & ~0x10)                                               # the meshes the edits move are in one group of their own
    M[3] = M[5] = 0x10
    ctx.set_mesh_query_masks(M)
    builds = [0]

    def check(tag, masks, rebuilt):
        table = ctx.query_filter()[0]
        bvh = ctx.export_bvh()
        assert len(bvh["tris"]) == len(sc.triangles) and len(table) == len(sc.meshes)
        for i, Q in enumerate(masks):
            ctx.set_query_mask(Q)
            _check_families(ctx, Reference(bvh, sc.meshes, table, Q, inp, k_list=4, k_box=8), (tag, hex(Q)))
            if i == 0:
                builds[0] += 1 if rebuilt else 0
            assert ctx.query_filter()[2] == builds[0], (tag, hex(Q))          # one build per topology change, none for a new Q
        return table
    check("upload", (0x10, 1 << 9), True)
    mgr.set_mesh_transform(sc, 3, pos=(0.7, 0.0, -0.4), rotation=(0, 25, 0))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_vertices(sc)
    check("update_vertices", (ALL & ~0x10,), False)
    mgr.set_mesh_transform(sc, 5, pos=(-0.5, 0.2, 0.3))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_transforms(sc, [5])
    check("update_transforms", (0x10,), False)
    new = append_patch(sc, cam, "hall_small", 300, 0)
    ctx.append_meshes(sc, new)
    table = check("append_meshes", (1 << 30, 0x10), True)
    assert table[new] == ALL and np.array_equal(table[:new], M)
    # the new mesh is admitted by every non-zero Q: a point on it finds it under each single bit
    centre = sc.world_vertices["position"][-1].astype(F32)
    first_new = sc.meshes[new][0]
    for bit in range(0, 32, 5):
        ctx.set_query_mask(1 << bit)
        near = ctx.nearest_points(centre[None], max_hits=4)[0]
        assert near["distance2"][0, 0] == 0 and (near["triangle"][0] >= first_new).any(), bit
    for mode in (0, 1):
        ctx.set_append_placement(mode)
        ctx.regraft_meshes([3, new])
        assert np.array_equal(check("regraft_meshes %d" % mode, (ALL & ~0x10,) if mode else (0x10,), True), table)
    ctx.remove_meshes(sc.remove_meshes_from_scene([4, new]))
    table = check("remove_meshes", (1 << 9,), True)
    assert np.array_equal(table, np.delete(M, 4))
    ctx.close()


# ---- 7. stack budget extremes
@pytest.mark.parametrize("budget", [1, 31])
def test_stack_budget_extremes(hall, budget):
    """Tuning key 8 at its ends: the smallest budget (raised to the tree's level count) makes the node visits push resume entries, which
    meet masked nodes like any other reference; the largest is the deepest stack."""
    sc, inp, bvh, M, refs = hall
    for key15 in (1, 2):
        ctx = capi.Context(0)
        ctx.set_tuning(15, key15)
        ctx.set_tuning(8, budget)
        ctx.upload_scene(sc)
        ctx.set_mesh_query_masks(M)
        for Q in HALL_QS[:2]:
            ctx.set_query_mask(Q)
            _check_families(ctx, refs[Q], (budget, key15, hex(Q)))
        ctx.close()


# ---- 8. what the filter does not touch
def test_frames_and_radiance_queries_ignore_the_filter():
    mk_scene, mk_cam = SCENES["hall_small"]
    sc, W, H = mk_scene(), 96, 64
    cam = mk_cam(W, H)
    o, d = bf.random_rays(sc, 600, 13)
    runs = []
    for with_filter in (False, True):
        ctx = _ctx(sc)
        ctx.resize(W, H)
        ctx.set_camera(cam)
        if with_filter:
            ctx.set_mesh_query_masks(np.zeros(len(sc.meshes), dtype=np.uint32))      # admits nothing under any Q
            ctx.set_query_mask(1)
            assert (ctx.trace_rays(o, d)["objectIndex"] == -1).all()
        out = []
        for tech in (capi.RESTIR_DI, 2):
            st = settings_for(tech)
            ctx.reset_frame_index()
            for f in range(2):
                st.rand_seed = f + 1
                ctx.render(st)
            img, acc = ctx.readback()
            out += [img, acc, ctx.read_buffer(capi.BUF_PAYLOAD)]
        rad, pay = ctx.render_rays(o, d, settings_for(capi.NEE), want_payload=True)[:2]
        assert (pay["objectIndex"] >= 0).sum() > 300
        out += [rad, pay]
        if with_filter:
            assert (ctx.trace_rays(o, d)["objectIndex"] == -1).all()
        runs.append(out)
        ctx.close()
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()


# ---- 9. the device path
def test_tensor_path_under_a_filter():
    """Run in a fresh process that initialises torch's CUDA before the library is loaded (see test_gpu_query's torch test)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_query_filter as t; t._tensor_path_checks(); print('tensor path ok')"
            % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "tensor path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _tensor_path_checks():
    """The tensor methods equal the host entries under a filter; two back-to-back device calls with set_query_mask between them answer
    each with the mask in effect when it was enqueued, without a synchronisation by the caller."""
    import torch
    sc = SCENES["hall_small"][0]()
    inp = _hall_inputs(sc, 2048)
    M = _hall_table(len(sc.meshes))
    ctx = _ctx(sc, key15=1)
    ctx.set_mesh_query_masks(M)
    qa, qb = HALL_QS[0], HALL_QS[1]
    want = {}
    for Q in (qa, qb):
        ctx.set_query_mask(Q)
        want[Q] = (ctx.trace_rays(inp.o, inp.d), ctx.trace_rays(inp.o, inp.d, occluded=True), ctx.trace_ray_hits(inp.o, inp.d, max_hits=4),
                   ctx.nearest_points(inp.p, inp.radius, max_hits=4), ctx.overlap_boxes(inp.lo, inp.hi, max_hits=8))
    assert want[qa][0].tobytes() != want[qb][0].tobytes() and not np.array_equal(want[qa][4][0], want[qb][4][0])
    n = len(inp.o)
    col = lambda v: torch.full((n, 1), float(v), device="cuda:0")
    ot, dt = torch.from_numpy(inp.o).to("cuda:0"), torch.from_numpy(inp.d).to("cuda:0")
    rays = torch.cat([ot, col(0.0), dt, col(float("inf"))], 1).contiguous()
    pts = torch.cat([torch.from_numpy(inp.p).to("cuda:0"), col(inp.radius)], 1).contiguous()
    boxes = torch.cat([torch.from_numpy(inp.lo).to("cuda:0"), col(0.0), torch.from_numpy(inp.hi).to("cuda:0"), col(0.0)], 1).contiguous()
    for _ in range(2):
        got = {}
        big = torch.randn(2048, 2048, device="cuda:0") @ torch.randn(2048, 2048, device="cuda:0")
        for Q in (qa, qb):                                                    # no synchronisation between the calls or the mask changes
            ctx.set_query_mask(Q)
            got[Q] = (ctx.trace_rays_tensor(rays), ctx.trace_rays_tensor(rays, occluded=True), ctx.trace_ray_hits_tensor(rays, 4),
                      ctx.nearest_points_tensor(pts, 4), ctx.overlap_boxes_tensor(boxes, 8))
        for Q in (qa, qb):
            pay, occ, (hits, hc), (near, nc), (tris, tc, tn) = got[Q]
            wpay, wocc, (whits, whc), (wnear, wnc), (wtris, wtc, wtn) = want[Q]
            assert np.ascontiguousarray(pay.cpu().numpy()).tobytes() == wpay.tobytes()
            assert np.array_equal(occ.cpu().numpy() != 0, wocc)
            assert mh.records_equal(np.ascontiguousarray(hits.cpu().numpy()).view(capi.RAY_HIT_DTYPE).reshape(whits.shape), whits)
            assert mh.records_equal(np.ascontiguousarray(near.cpu().numpy()).view(capi.POINT_HIT_DTYPE).reshape(wnear.shape), wnear)
            assert np.array_equal(hc.cpu().numpy().astype(np.uint32), whc) and np.array_equal(nc.cpu().numpy().astype(np.uint32), wnc)
            assert np.array_equal(tris.cpu().numpy().view(np.uint32), wtris)
            assert np.array_equal(tc.cpu().numpy().view(np.uint32), wtc) and np.array_equal(tn.cpu().numpy().view(np.uint32), wtn)
        del big
    assert ctx.query_filter()[2] == 1
    ctx.close()


# ---- 10. memory
def test_device_memory_follows_the_filter(layers):
    sc, inp, bvh, M = layers[:4]
    base = capi.live_device_bytes()
    ctx = _ctx(sc)
    ctx.overlap_boxes(inp.lo, inp.hi, max_hits=8)                             # the family's staging is allocated before the filter is
    loaded = capi.live_device_bytes()
    ctx.set_mesh_query_masks(M)
    assert capi.live_device_bytes() == loaded                                 # nothing until a query asks
    ctx.overlap_boxes(inp.lo, inp.hi, max_hits=8)
    n_nonempty = sum(1 for m in sc.meshes if m[1])
    assert capi.live_device_bytes() - loaded == 4 * len(bvh["tris"]) + 4 * len(bvh["nodes"]) + 8 * n_nonempty
    ctx.set_query_mask(2)
    ctx.overlap_boxes(inp.lo, inp.hi, max_hits=8)
    ctx.set_mesh_query_masks(M[::-1].copy())                                  # a new table of the same size reuses the buffers
    ctx.overlap_boxes(inp.lo, inp.hi, max_hits=8)
    assert capi.live_device_bytes() - loaded == 4 * len(bvh["tris"]) + 4 * len(bvh["nodes"]) + 8 * n_nonempty
    ctx.set_mesh_query_masks(None)
    assert capi.live_device_bytes() == loaded                                 # released when the filter is switched off
    ctx.set_mesh_query_masks(M)
    ctx.overlap_boxes(inp.lo, inp.hi, max_hits=8)
    ctx.close()
    assert capi.live_device_bytes() == base                                   # ... and on destroy


# ---- 11. errors, on a device context
def test_error_order_on_a_device_context():
    sc = SCENES["cornell"][0]()
    nM = len(sc.meshes)

    def raw(ctx, masks, count, handle=True):
        arr = None if masks is None else (C.c_uint32 * max(1, len(masks)))(*masks)
        return ctx.lib.fyprt_set_mesh_query_masks(ctx.h if handle else None, arr, count)
    fresh = capi.Context(0)
    assert raw(fresh, [1] * nM, nM, handle=False) == EINVAL
    assert raw(fresh, None, 3) == EINVAL and raw(fresh, [1], 0) == EINVAL      # argument cases before the state
    assert raw(fresh, [1] * nM, nM) == ESTATE and raw(fresh, None, 0) == ESTATE
    fresh.set_query_mask(3)                                                   # any state
    fresh.upload_scene(sc)
    assert fresh.query_filter() == (None, ALL, 0)                             # the upload reset it
    assert raw(fresh, [1] * (nM + 1), nM + 1) == EINVAL and raw(fresh, None, nM) == EINVAL
    assert fresh.query_filter()[0] is None
    assert raw(fresh, [1] * nM, nM) == 0 and raw(fresh, None, 0) == 0
    # the query entry points keep their own error order with a table set
    fresh.set_mesh_query_masks(np.ones(nM, dtype=np.uint32))
    assert fresh.lib.fyprt_overlap_boxes(fresh.h, None, None, 1, 0, None, None, None, None) == EINVAL
    assert fresh.lib.fyprt_nearest_points(fresh.h, None, None, 0, 4, None, None, None) == 0
    assert fresh.query_filter()[2] == 0                                       # an empty call builds nothing
    fresh.close()
