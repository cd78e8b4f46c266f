"""Triangle-overlap queries (fyprt_overlap_triangles) without a GPU: the symbols and the record's layout, the errors of both entry
points in the header's order on a host-only context, the Python wrappers' argument checks, and the brute-force reference of the GPU tests
(tests/triangles_ref.py) held to what can be known without the kernel: independent float64 tests on random pairs in general position
and in one plane, hand cases with exactly known answers, the traversal's cull rule against the rounded rule on every child box of every
node, and continuation passes."""
import re
from pathlib import Path

import numpy as np
import pytest

import boxes_ref as br
import triangles_ref as tr
from common import SCENES
from fypraytracer_amd import capi

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
F32 = np.float32
SCENE_NAMES = ("cornell", "hall_small", "banana_standin")


def test_symbols_record_layout_and_the_header():
    lib = capi.load_library()
    assert {"fyprt_overlap_triangles", "fyprt_overlap_triangles_device"} <= set(capi.EXPORTED_SYMBOLS)
    assert hasattr(lib, "fyprt_overlap_triangles") and hasattr(lib, "fyprt_overlap_triangles_device")
    assert capi.QUERY_TRIANGLE_DTYPE.itemsize == 48
    assert [capi.QUERY_TRIANGLE_DTYPE.fields[k][1] for k in ("v0", "pad0", "v1", "pad1", "v2", "pad2")] == [0, 12, 16, 28, 32, 44]
    header = (Path(__file__).resolve().parent.parent / "include" / "fyprt.h").read_text()
    assert "fyprt_overlap_triangles_device" in header and "typedef struct fyprt_triangle " in header
    assert "ten entry points" in header and "eight entry points" not in header
    assert re.search(r"bit-equal to a record's v0 always accepts", header)
    # the pads are ignored: the wrapper's records carry zeros there, and whatever a caller puts there changes no field the rule reads
    rec = capi.Context._tri_records("t", np.arange(18, dtype=F32).reshape(2, 3, 3))
    assert rec["v1"][1].tolist() == [12, 13, 14] and not rec["pad0"].any() and not rec["pad1"].any() and not rec["pad2"].any()
    three = capi.Context._tri_records("t", (rec["v0"], rec["v1"], rec["v2"]))
    assert three.tobytes() == rec.tobytes()
    rec["pad0"], rec["pad1"], rec["pad2"] = 0xFFFFFFFF, 0x7FC00000, 0x7F800000
    assert np.array_equal(np.stack([rec["v0"], rec["v1"], rec["v2"]], axis=1), np.arange(18, dtype=F32).reshape(2, 3, 3))


def test_errors_in_the_headers_order_on_a_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    q = np.zeros(4, dtype=capi.QUERY_TRIANGLE_DTYPE)
    q["v1"][:, 0] = 1.0
    q["v2"][:, 1] = 1.0
    tris = np.zeros((4, 32), dtype=np.uint32)
    counts, totals = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    dev = np.zeros(64, dtype=np.float32)                      # (never dereferenced: every call below fails before a launch)
    base = dev.ctypes.data + (-dev.ctypes.data) % 16          # a 16-byte aligned address inside it

    def host(k=4, r=q.ctypes.data, n=4, h=tris.ctypes.data, c=counts.ctypes.data, t=totals.ctypes.data, a=None):
        return lib.fyprt_overlap_triangles(ctx.h, r, a, n, k, h, c, t, None)

    def device(k=4, r=base, n=4, h=base, c=base, t=base, a=None):
        return lib.fyprt_overlap_triangles_device(ctx.h, r, a, n, k, h, c, t)

    for call in (host, device):
        assert call() == ESTATE                                               # no scene yet
        assert call(c=None) == ESTATE and call(t=None) == ESTATE              # hit_counts and totals may be NULL
        for k in (0, 33):
            assert call(k=k) == EINVAL                                        # max_hits before the state ...
            assert call(k=k, r=None) == EINVAL
            assert call(k=k, n=0) == EINVAL                                   # ... and before the empty call
        assert call(r=None) == EINVAL and call(h=None) == EINVAL              # NULL query / answer triangles with count > 0
        assert call(k=1) == ESTATE and call(k=32) == ESTATE
    for bad in (dict(r=base + 4), dict(r=base + 8), dict(a=base + 2), dict(h=base + 1), dict(c=base + 2), dict(t=base + 3)):
        assert device(**bad) == EINVAL, bad                                   # misaligned device pointers: refused before the state
    assert device(a=base + 4, h=base + 8, c=base + 12, t=base + 20) == ESTATE  # the words need 4 bytes only
    ctx.upload_scene(SCENES["cornell"][0]())
    for call in (host, device):
        assert call() == ESTATE                                               # a host-only context cannot query
        assert call(k=0) == EINVAL and call(k=33) == EINVAL and call(r=None) == EINVAL and call(h=None) == EINVAL
        assert call(n=0) == ESTATE                                            # the state comes before the empty call
    assert device(h=base + 2) == EINVAL
    assert lib.fyprt_overlap_triangles(None, q.ctypes.data, None, 4, 4, tris.ctypes.data, None, None, None) == EINVAL
    assert lib.fyprt_overlap_triangles_device(None, None, None, 0, 4, None, None, None) == EINVAL
    with pytest.raises(capi.FyprtError):
        ctx.overlap_triangles(np.zeros((1, 3, 3)))
    ctx.close()


def test_argument_error_texts_of_the_entry_points():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    dev = np.zeros(64, dtype=np.float32)
    base = dev.ctypes.data + (-dev.ctypes.data) % 16
    name, aligned = "fyprt_overlap_triangles", "triangles must be 16-byte and after, triangles, hit_counts and totals 4-byte aligned"
    host, device = getattr(lib, name), getattr(lib, name + "_device")

    def text(rc, code):
        assert rc == code
        return lib.fyprt_last_error(ctx.h).decode()

    for who, call in ((name, lambda r=base, n=4, k=4, h=base, c=base: host(ctx.h, r, None, n, k, h, c, base, None)),
                      (name + "_device", lambda r=base, n=4, k=4, h=base, c=base: device(ctx.h, r, None, n, k, h, c, base))):
        assert text(call(k=0), EINVAL) == text(call(k=33), EINVAL) == f"{who}: max_hits must be 1..32"
        assert text(call(r=None), EINVAL) == text(call(h=None), EINVAL) == f"{who}: NULL triangles / triangles with a non-zero count"
        assert text(call(), ESTATE) == f"{who}: host-only context (device -1) cannot query"
    assert text(device(ctx.h, base + 4, None, 4, 4, base, base, base), EINVAL) == f"{name}_device: {aligned}"
    assert text(device(ctx.h, base, None, 4, 4, base, base + 2, base), EINVAL) == f"{name}_device: {aligned}"
    ctx.upload_scene(SCENES["cornell"][0]())
    ctx.close()
    ctx = capi.Context(-1)
    assert text(host(ctx.h, base, None, 4, 4, base, base, base, None), ESTATE) == f"{name}: host-only context (device -1) cannot query"
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
        q = np.zeros((3, 3, 3), F32)
        for bad in (0, 33, -1, 2.5, True, None):
            with pytest.raises(ValueError):
                ctx.overlap_triangles(q, max_hits=bad)
            with pytest.raises(ValueError):
                ctx.triangles_touching(q, max_hits=bad)
            with pytest.raises(ValueError):
                ctx.overlap_triangles_tensor(None, bad)
        for bad_tris in (np.zeros((3, 3, 2), F32), np.zeros((3, 2, 3), F32), np.zeros(9, F32), F32(1.0), np.zeros((2, 3, 3, 3), F32),
                         (np.zeros((3, 3), F32), np.zeros((3, 3), F32), np.zeros((2, 3), F32)),       # a different count
                         (np.zeros((3, 3), F32), np.zeros((3, 2), F32), np.zeros((3, 3), F32))):
            with pytest.raises(ValueError):
                ctx.overlap_triangles(bad_tris)
            with pytest.raises(ValueError):
                ctx.triangles_touching(bad_tris)
        with pytest.raises(ValueError):
            ctx.overlap_triangles(q, after=np.zeros(2, dtype=np.uint32))                    # wrong length
        with pytest.raises(ValueError):
            ctx.overlap_triangles(q, after=np.zeros(3, dtype=np.int64))                     # wrong dtype
        import torch
        for t in (None, torch.zeros(4, 9), torch.zeros(4, 12, dtype=torch.float64), torch.zeros(12, 4).t()[:, :], torch.zeros(8, 12)[::2], torch.zeros(4, 12)):   # the last: not on the GPU
            with pytest.raises(ValueError):
                ctx.overlap_triangles_tensor(t, 4)
    finally:
        ctx.lib = real
    ctx.close()


# ---- the reference against independent float64 facts
def _records(t):
    """Leaf records of triangles (N, 3, 3) given by their vertices, as the builders form them: v0, fl(v1 - v0), fl(v2 - v0)."""
    t = np.asarray(t, F32).reshape(-1, 3, 3)
    return t[:, 0], (t[:, 1] - t[:, 0]).astype(F32), (t[:, 2] - t[:, 0]).astype(F32)


def _edges_through(a, b, eps=1e-4):
    """Float64: the three edges of triangles a (N, 3, 3) against triangles b.  For each edge the end points' signed distances to b's
    plane (unit normal); where they lie on opposite sides, the crossing point's barycentric coordinates in b.  Returns (crosses,
    undecided): an edge passes through b's interior; an end point within eps of the plane or a crossing within eps of an edge of b in
    barycentric units."""
    t0, u, v = b[:, 0], b[:, 1] - b[:, 0], b[:, 2] - b[:, 0]
    nrm = np.cross(u, v)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    uu, uv, vv = (u * u).sum(1), (u * v).sum(1), (v * v).sum(1)
    det = uu * vv - uv * uv
    crosses = np.zeros(len(a), bool)
    undecided = np.zeros(len(a), bool)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        p, q = a[:, i], a[:, j]
        dp, dq = ((p - t0) * nrm).sum(1), ((q - t0) * nrm).sum(1)
        undecided |= (np.abs(dp) < eps) | (np.abs(dq) < eps)
        opposite = (dp > 0) != (dq > 0)
        with np.errstate(all="ignore"):
            s = np.where(opposite, dp / (dp - dq), 0.0)
        w = p + s[:, None] * (q - p) - t0
        wu, wv = (w * u).sum(1), (w * v).sum(1)
        b1, b2 = (vv * wu - uv * wv) / det, (uu * wv - uv * wu) / det
        bary = np.stack([b1, b2, 1.0 - b1 - b2], axis=1)
        undecided |= opposite & (np.abs(bary).min(axis=1) < eps)
        crosses |= opposite & (bary.min(axis=1) > 0)
    return crosses, undecided


def _general_pairs(n, seed):
    """The issue's generator: centres uniform in [-10, 10]^3, size 10^U(-2, 0.5), scene triangle = centre + N(0,1) size per vertex, query
    triangle = centre + N(0,1) size + N(0,1) size 10^U(-0.5, 0.5) per vertex, vertices rounded to float32."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-10, 10, size=(n, 1, 3))
    size = 10.0 ** rng.uniform(-2, 0.5, size=(n, 1, 1))
    scene = (centre + rng.normal(size=(n, 3, 3)) * size).astype(F32)
    query = (centre + rng.normal(size=(n, 3, 3)) * size + rng.normal(size=(n, 3, 3)) * size * 10.0 ** rng.uniform(-0.5, 0.5, size=(n, 1, 1))).astype(F32)
    return scene, query


def test_reference_against_float64_edge_tests_in_general_position():
    """Two triangles in general position intersect iff an edge of one passes through the other.  That test in float64 on the float32
    vertices; the float32 rule must accept every pair it calls intersecting and reject every pair it calls apart, outside the undecided
    band (an end point within 1e-4 of the other plane, a crossing within 1e-4 of an edge in barycentric units), which holds at most 2 %
    of the pairs."""
    n = 400000
    scene, query = _general_pairs(n, seed=11)
    got = tr.tri_pairs(query, *_records(scene))
    s64, q64 = scene.astype(np.float64), query.astype(np.float64)
    c1, u1 = _edges_through(q64, s64)
    c2, u2 = _edges_through(s64, q64)
    intersecting, undecided = c1 | c2, u1 | u2
    decided = ~undecided
    print(f"general position: {undecided.mean() * 100:.3f} % undecided, {intersecting[decided].mean() * 100:.2f} % of the decided intersect, "
          f"{(got != intersecting)[undecided].sum()} disagreements inside the band")
    assert undecided.mean() <= 0.02
    assert intersecting[decided].sum() > n // 20 and (~intersecting[decided]).sum() > n // 20
    assert not (decided & intersecting & ~got).any(), np.nonzero(decided & intersecting & ~got)[0][:4]       # no rejected intersecting pair
    assert not (decided & ~intersecting & got).any(), np.nonzero(decided & ~intersecting & got)[0][:4]       # no accepted clearly-apart pair


def _coplanar_pairs(n, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-10, 10, size=(n, 1)).astype(F32)
    centre = rng.uniform(-10, 10, size=(n, 1, 2))
    size = 10.0 ** rng.uniform(-1.5, 0.5, size=(n, 1, 1))
    scene = (centre + rng.normal(size=(n, 3, 2)) * size).astype(F32)
    query = (centre + rng.normal(size=(n, 3, 2)) * size + rng.normal(size=(n, 3, 2)) * size * 10.0 ** rng.uniform(-0.5, 0.5, size=(n, 1, 1))).astype(F32)
    lift = lambda t: np.concatenate([t, np.broadcast_to(z[:, None, :], (n, 3, 1))], axis=2).astype(F32)
    return lift(scene), lift(query), size.reshape(n)


def _gap_2d(a, b):
    """Float64 separating-axis test in the plane: the largest signed gap between the two triangles' intervals over the six unit edge
    normals.  Positive: separated by that much; negative: they overlap, by at least that depth, on every axis."""
    best = np.full(len(a), -np.inf)
    for t in (a, b):
        for i, j in ((0, 1), (1, 2), (2, 0)):
            e = t[:, j] - t[:, i]
            ax = np.stack([-e[:, 1], e[:, 0]], axis=1)
            ax /= np.linalg.norm(ax, axis=1, keepdims=True)
            pa, pb = (a * ax[:, None, :]).sum(2), (b * ax[:, None, :]).sum(2)
            best = np.maximum(best, np.maximum(pa.min(1) - pb.max(1), pb.min(1) - pa.max(1)))
    return best


def test_reference_against_a_float64_test_in_one_plane_and_the_in_plane_axes_are_needed():
    """Pairs lying exactly in one plane z = const: the normals are parallel and every edge pair's cross product is parallel to them, so
    only the six in-plane edge normals can separate.  Against a float64 2D separating-axis test, undecided inside a gap of 1e-4 * size
    (at most 2 % of the pairs).  Without the six in-plane axes the same reference accepts separated pairs: the check has teeth."""
    n = 200000
    scene, query, size = _coplanar_pairs(n, seed=13)
    rec = _records(scene)
    assert (rec[1][:, 2] == 0).all() and (rec[2][:, 2] == 0).all()
    coord, normals, pairs, inplane = tr.tri_pairs(query, *rec, steps=True)
    got = coord & normals & pairs & inplane
    gap = _gap_2d(scene[:, :, :2].astype(np.float64), query[:, :, :2].astype(np.float64))
    undecided = np.abs(gap) < 1e-4 * size
    apart, overlapping = ~undecided & (gap > 0), ~undecided & (gap < 0)
    without = coord & normals & pairs
    print(f"coplanar: {undecided.mean() * 100:.4f} % undecided, {apart.sum()} apart, {overlapping.sum()} overlapping, "
          f"{(without & apart).sum()} separated pairs accepted without the in-plane axes")
    assert undecided.mean() <= 0.02
    assert apart.sum() > n // 20 and overlapping.sum() > n // 20
    assert not (overlapping & ~got).any(), np.nonzero(overlapping & ~got)[0][:4]
    assert not (apart & got).any(), np.nonzero(apart & got)[0][:4]
    assert (without & apart).sum() > 1000


# ---- hand cases
def _ask(q, t, steps=False):
    r = tr.tri_pairs(np.array([q], F32), *_records(np.array([t], F32)), steps=steps)
    return tuple(bool(x[0]) for x in r) if steps else bool(r[0])


def test_cases_by_hand():
    big = ((-10, -10, 0), (30, -10, 0), (-10, 30, 0))                         # a large triangle in z = 0; its hypotenuse is x + y = 20
    # a shared vertex: a query vertex bit-equal to the record's v0 always accepts, whichever vertex it is and whatever the rest
    rng = np.random.default_rng(1)
    V = (rng.uniform(-100, 100, size=(600, 3, 3)) * 10.0 ** rng.uniform(-3, 0, size=(600, 1, 1))).astype(F32)
    rec = _records(V)
    for slot in range(3):
        Q = (rng.uniform(-100, 100, size=(600, 3, 3))).astype(F32)
        Q[:300] = (V[:300] + rng.normal(size=(300, 3, 3)) * 1e-3).astype(F32)         # some nearly on the record, some anywhere
        Q[:, slot] = V[:, 0]
        assert tr.tri_pairs(Q, *rec).all(), slot
    assert not tr.tri_pairs(rng.uniform(-100, 100, size=(600, 3, 3)).astype(F32), *rec).all()
    # a shared edge, the other vertices on different sides / in another plane
    assert _ask(((0, 0, 0), (1, 0, 0), (0, -1, 1)), ((0, 0, 0), (1, 0, 0), (0, 1, 0)))
    assert _ask(((1, 0, 0), (0, 0, 0), (0, -1, 0)), ((0, 0, 0), (1, 0, 0), (0, 1, 0)))           # coplanar, touching along the edge only
    # piercing: through the interior; through the plane beyond the hypotenuse
    assert _ask(((1, 1, -1), (1, 1, 1), (2, 1, 1)), big)
    assert not _ask(((12, 12, -1), (12, 12, 1), (13, 12, 1)), big)
    assert _ask(((12, 12, -1), (12, 12, 1), (13, 12, 1)), big, steps=True)[0]                     # inside the bounds: the coordinate axes do not separate
    # coplanar: contained, containing, and beside the hypotenuse inside the bounding box — there only the in-plane axes separate
    assert _ask(((1, 1, 0), (2, 1, 0), (1, 2, 0)), big)
    assert _ask(((-100, -100, 0), (300, -100, 0), (-100, 300, 0)), big)
    assert _ask(((12, 12, 0), (13, 12, 0), (12, 13, 0)), big, steps=True) == (True, True, True, False)
    assert _ask(((9, 9, 0), (10, 10, 0), (9, 10, 0)), big)                                        # a vertex on the hypotenuse: touching, exact
    # parallel planes one ulp apart: separated; in the same plane: touching
    up = float(np.nextafter(F32(0), F32(1)))
    assert not _ask(((1, 1, up), (2, 1, up), (1, 2, up)), big)
    assert not _ask(((1, 1, -up), (2, 1, -up), (1, 2, -up)), big)
    one = float(np.nextafter(F32(1), F32(2)))
    assert not _ask(((1, 1, one), (2, 1, one), (1, 2, one)), ((-10, -10, 1), (30, -10, 1), (-10, 30, 1)))
    assert _ask(((1, 1, 1), (2, 1, 1), (1, 2, 1)), ((-10, -10, 1), (30, -10, 1), (-10, 30, 1)))
    # a zero-area query: a point inside, above and beside the triangle; a needle through it and beside it
    assert _ask(((1, 1, 0),) * 3, big)
    assert not _ask(((1, 1, 1),) * 3, big)
    assert not _ask(((12, 12, 0),) * 3, big)
    assert _ask(((1, 1, -1), (1, 1, 1), (1, 1, 1)), big)
    assert not _ask(((12, 12, -1), (12, 12, 1), (12, 12, 1)), big)
    assert not tr.invalid_triangles(np.array([((1, 1, 0),) * 3], F32)).any()
    # a zero-area record: a point in the query's plane inside it, beside it and off the plane
    point = ((1, 2, 3),) * 3
    assert _ask(((0, 0, 3), (4, 0, 3), (0, 4, 3)), point)
    assert not _ask(((0, 0, 3), (1, 0, 3), (0, 1, 3)), point)
    assert not _ask(((0, 0, 3.5), (4, 0, 3.5), (0, 4, 2.75)), point)
    # NaN and infinite records are never accepted, whichever field holds them
    nan, inf = F32(np.nan), F32(np.inf)
    q = np.array([((1, 1, -1), (1, 1, 1), (2, 1, 1))], F32)
    v0, e1, e2 = _records(np.array([big], F32))
    assert tr.tri_pairs(q, v0, e1, e2)[0]
    for field in range(3):
        for comp in range(3):
            for bad in (nan, inf):
                r = [v0.copy(), e1.copy(), e2.copy()]
                r[field][0, comp] = bad
                assert not tr.tri_pairs(q, *r)[0], (field, comp, bad)
    # each invalid form: a non-finite vertex component, and finite vertices whose difference overflows
    tris = np.zeros(1, dtype=capi.BVH_TRI_DTYPE)
    tris["v0"], tris["e1"], tris["e2"], tris["tri"] = v0, e1, e2, [7]
    qs = np.repeat(q, 9, axis=0)
    qs[1, 0, 0] = nan; qs[2, 1, 2] = nan; qs[3, 2, 1] = nan; qs[4, 0, 1] = inf; qs[5, 1, 0] = -inf; qs[6, 2, 2] = inf
    qs[7, 0, 0], qs[7, 1, 0] = -3e38, 3e38                                   # f1 overflows
    qs[8, 0, 1], qs[8, 2, 1] = 3e38, -3e38                                   # f2 overflows
    assert tr.invalid_triangles(qs).tolist() == [False] + [True] * 8
    t, c, tot = tr.k_lowest({"tris": tris}, qs, 2)
    assert c.tolist() == [1] + [0] * 8 and tot.tolist() == [1] + [0] * 8
    assert t[0].tolist() == [7, 0xFFFFFFFF] and (t[1:] == tr.NONE).all()
    assert tr.k_lowest({"tris": tris}, qs[:1], 2, after=np.array([7], np.uint32))[2].tolist() == [0]
    assert tr.k_lowest({"tris": tris}, qs[:1], 2, after=np.array([6], np.uint32))[1].tolist() == [1]
    assert tr.k_lowest({"tris": tris}, qs[:1], 2, after=np.array([0xFFFFFFFF], np.uint32))[2].tolist() == [0]
    # the query filter: a triangle that is not admitted is not answered
    assert tr.k_lowest({"tris": tris}, qs[:1], 2, admitted=np.zeros(8, bool))[2].tolist() == [0]


# ---- the scenes, their exported trees and a query set each
def _export(sc):
    ctx = capi.Context(-1)
    ctx.set_tuning(12, 0)
    ctx.upload_scene(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    return bvh


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in SCENE_NAMES:
        sc = SCENES[name][0]()
        bvh = _export(sc)
        q = tr.scene_queries(sc, bvh, 48, seed=5)
        out[name] = (sc, bvh, q, tr.accepted(bvh, q))
    return out


def test_cull_rule_skips_no_child_with_an_accepted_record(cases):
    """On the host builder's trees (a host-only context builds with it whatever tuning key 12 says; the device builders' trees are held
    to the same check in tests/test_gpu_triangles.py)."""
    for name, (sc, bvh, q, (ok, ids)) in cases.items():
        assert ok.any(axis=1).sum() > len(q) // 4, name
        assert tr.check_cull(bvh, q, ok, name) >= 2 * len(q) * len(bvh["nodes"])
    sc, bvh = cases["banana_standin"][:2]
    lo, hi, where = br.protruding_boxes(bvh)                                   # bounds that begin exactly on a protruding rounded vertex
    if len(where):
        q = np.stack([lo, hi, np.stack([lo[:, 0], hi[:, 1], lo[:, 2]], axis=1)], axis=1).astype(F32)
        tr.check_cull(bvh, q, tr.accepted(bvh, q)[0], "protruding")


def test_continuation_passes_concatenate_to_one_pass(cases):
    for name in ("cornell", "banana_standin"):
        sc, bvh, q, ok_ids = cases[name]
        flat, offsets = tr.all_touching(bvh, q, ok_ids)
        _, _, totals = tr.k_lowest(bvh, q, 1, ok_ids=ok_ids)
        assert np.array_equal(np.diff(offsets), totals) and totals.max() > 3 and (totals == 0).any(), name
        got = [[] for _ in range(len(q))]
        after, passes = None, 0
        while True:
            tris, counts, tot = tr.k_lowest(bvh, q, 3, after=after, ok_ids=ok_ids)
            if not counts.any():
                break
            done = np.array([sum(len(x) for x in g) for g in got])
            assert np.array_equal(tot, totals - done)                         # the total tells what is still to come, this pass included
            for i in np.nonzero(counts)[0]:
                got[i].append(tris[i, :counts[i]])
            after = tris[:, 2].copy()                                         # the last slot, unused ones included: those records are finished
            passes += 1
        assert passes == -(-int(totals.max()) // 3)
        for i in range(len(q)):
            cat = np.concatenate(got[i]) if got[i] else np.empty(0, dtype=np.uint32)
            assert np.array_equal(cat, flat[offsets[i]:offsets[i + 1]]), (name, i)
            assert (np.diff(cat.astype(np.int64)) > 0).all()                  # strictly ascending: no triangle twice
