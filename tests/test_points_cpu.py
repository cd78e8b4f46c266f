"""Nearest-point queries (fyprt_nearest_points) without a GPU: the symbols and the records' layout, the errors of both entry points in
the header's order on a host-only context, the Python wrappers' argument checks, and the brute-force reference of the GPU tests
(tests/points_ref.py) held to what can be known without the kernel: an independent float64 closest point on the scenes' own vertices,
hand-made region cases with exactly known answers, the traversal's cull rule against the rounded triangle arithmetic on every child
box of every node, continuation passes, and degenerate records."""
import re
from pathlib import Path

import numpy as np
import pytest

import points_ref as pr
from common import SCENES
from fypraytracer_amd import capi

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
F32 = np.float32
U = 2.0 ** -24              # unit roundoff of binary32
SCENE_NAMES = ("cornell", "hall_small", "banana")


def test_symbols_and_record_layouts():
    lib = capi.load_library()
    assert {"fyprt_nearest_points", "fyprt_nearest_points_device"} <= set(capi.EXPORTED_SYMBOLS)
    assert hasattr(lib, "fyprt_nearest_points") and hasattr(lib, "fyprt_nearest_points_device")
    assert capi.POINT_DTYPE.itemsize == 16 and capi.POINT_HIT_DTYPE.itemsize == 16
    assert [capi.POINT_DTYPE.fields[k][1] for k in ("position", "max_distance")] == [0, 12]
    assert [capi.POINT_HIT_DTYPE.fields[k][1] for k in ("distance2", "triangle", "u", "v")] == [0, 4, 8, 12]
    header = (Path(__file__).resolve().parent.parent / "include" / "fyprt.h").read_text()
    assert "fyprt_nearest_points_device" in header and "typedef struct fyprt_point_hit" in header and "typedef struct fyprt_point " in header
    assert int(re.search(r"#define\s+FYPRT_QUERY_MAX_HITS\s+(\d+)", header).group(1)) == capi.QUERY_MAX_HITS
    assert pr.UNUSED.tobytes() == np.array([-1.0], F32).tobytes() + b"\xff\xff\xff\xff" + bytes(8)
    assert float(pr.KEEP) == 1.0 - 2.0 ** -20


def test_errors_in_the_headers_order_on_a_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    pts = np.zeros(4, dtype=capi.POINT_DTYPE)
    pts["max_distance"] = np.inf
    hits = np.zeros((4, 8), dtype=capi.POINT_HIT_DTYPE)
    counts = np.zeros(4, dtype=np.uint32)
    dev = np.zeros(64, dtype=np.float32)                      # (never dereferenced: every call below fails before a launch)
    base = dev.ctypes.data + (-dev.ctypes.data) % 16          # a 16-byte aligned address inside it

    def host(k=4, r=pts.ctypes.data, n=4, h=hits.ctypes.data, c=counts.ctypes.data, a=None):
        return lib.fyprt_nearest_points(ctx.h, r, a, n, k, h, c, None)

    def device(k=4, r=base, n=4, h=base, c=base, a=None):
        return lib.fyprt_nearest_points_device(ctx.h, r, a, n, k, h, c)

    for call in (host, device):
        assert call() == ESTATE                                               # no scene yet
        assert call(c=None) == ESTATE                                         # hit_counts may be NULL
        for k in (0, 9):
            assert call(k=k) == EINVAL                                        # max_hits before the state ...
            assert call(k=k, r=None) == EINVAL
            assert call(k=k, n=0) == EINVAL                                   # ... and before the empty call
        assert call(r=None) == EINVAL and call(h=None) == EINVAL              # NULL points / hits with count > 0
        assert call(k=1) == ESTATE and call(k=8) == ESTATE
    for bad in (dict(r=base + 4), dict(a=base + 8), dict(h=base + 4), dict(c=base + 2)):
        assert device(**bad) == EINVAL, bad                                   # misaligned device pointers: refused before the state
    assert device(c=base + 4, a=base + 16) == ESTATE                          # counts need 4 bytes only
    ctx.upload_scene(SCENES["cornell"][0]())
    for call in (host, device):
        assert call() == ESTATE                                               # a host-only context cannot query
        assert call(k=0) == EINVAL and call(k=9) == EINVAL and call(r=None) == EINVAL and call(h=None) == EINVAL
        assert call(n=0) == ESTATE                                            # the state comes before the empty call
    assert device(h=base + 8) == EINVAL
    assert lib.fyprt_nearest_points(None, pts.ctypes.data, None, 4, 4, hits.ctypes.data, None, None) == EINVAL
    assert lib.fyprt_nearest_points_device(None, None, None, 0, 4, None, None) == EINVAL
    with pytest.raises(capi.FyprtError):
        ctx.nearest_points(np.zeros((1, 3)))
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
        p = np.zeros((3, 3), F32)
        for bad in (0, 9, -1, 2.5, True, None):
            with pytest.raises(ValueError):
                ctx.nearest_points(p, max_hits=bad)
            with pytest.raises(ValueError):
                ctx.triangles_within(p, 1.0, max_hits=bad)
            with pytest.raises(ValueError):
                ctx.nearest_points_tensor(None, bad)
        for bad_points in (np.zeros((3, 2), F32), np.zeros(4, F32), F32(1.0)):
            with pytest.raises(ValueError):
                ctx.nearest_points(bad_points)
            with pytest.raises(ValueError):
                ctx.triangles_within(bad_points, 1.0)
        with pytest.raises(ValueError):
            ctx.nearest_points(p, max_distance=np.ones(2, F32))                             # wrong length
        with pytest.raises(ValueError):
            ctx.triangles_within(p, np.ones((3, 1), F32))
        with pytest.raises(ValueError):
            ctx.nearest_points(p, after=np.zeros(2, dtype=capi.POINT_HIT_DTYPE))            # wrong length
        with pytest.raises(ValueError):
            ctx.nearest_points(p, after=np.zeros((3, 4), dtype=F32))                        # wrong dtype
        import torch
        for pts in (None, torch.zeros(4, 3), torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 4).t()[:, :], torch.zeros(8, 4)[::2], torch.zeros(4, 4)):   # the last: not on the GPU
            with pytest.raises(ValueError):
                ctx.nearest_points_tensor(pts, 4)
    finally:
        ctx.lib = real
    ctx.close()


# ---- the scenes, their exported trees and a point set each
def _scene_points(sc, bvh, n, seed):
    """Uniform points in twice the scene box, points on vertices, and points on decoded child planes and corners of the tree's nodes."""
    rng = np.random.default_rng(seed)
    pos = sc.world_vertices["position"].astype(np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo)
    uni = rng.uniform(mid - half, mid + half, size=(n, 3)).astype(F32)
    verts = sc.world_vertices["position"][rng.integers(0, len(pos), n // 4)].astype(F32)
    planes = []
    for node in bvh["nodes"][rng.integers(0, len(bvh["nodes"]), n // 8)]:
        blo, bhi = pr.child_planes(node)
        c = int(rng.integers(0, len(blo)))
        corner = np.where(rng.integers(0, 2, 3) == 1, bhi[c], blo[c]).astype(F32)
        face = rng.uniform(blo[c], bhi[c]).astype(F32)
        a = int(rng.integers(0, 3))
        face[a] = (blo[c] if rng.integers(0, 2) else bhi[c])[a]
        planes += [corner, face]
    return np.concatenate([uni, verts, np.array(planes, F32)]).astype(F32)


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
        out[name] = (sc, bvh, _scene_points(sc, bvh, 160, seed=3))
    return out


# ---- the reference against float64 on the caller's own vertices
def _closest_f64(p, A, B, C):
    """Independent closest point on a triangle in float64: the plane projection if it lies inside, else the nearest of the three
    edge segments.  p (P, 3) x triangles (T, 3) -> squared distance (P, T)."""
    p = p[:, None, :]
    ab, ac = (B - A)[None], (C - A)[None]
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    ap = p - A[None]
    with np.errstate(all="ignore"):
        # barycentrics of the projection from signed sub-areas
        w_b = (np.cross(ap, ac) * n).sum(-1) / nn
        w_c = (np.cross(ab, ap) * n).sum(-1) / nn
        inside = (w_b >= 0) & (w_c >= 0) & (w_b + w_c <= 1) & (nn > 0)
        plane = (ap * n).sum(-1) ** 2 / nn

    def seg(P0, P1):
        d = (P1 - P0)[None]
        dd = (d * d).sum(-1)
        with np.errstate(all="ignore"):
            t = np.clip(np.where(dd > 0, ((p - P0[None]) * d).sum(-1) / dd, 0.0), 0.0, 1.0)
        x = P0[None] + t[..., None] * d
        return ((p - x) ** 2).sum(-1)
    edges = np.minimum(np.minimum(seg(A, B), seg(A, C)), seg(B, C))
    return np.where(inside, np.minimum(plane, edges), edges)


def test_reference_agrees_with_float64_on_the_scenes_vertices(cases):
    """Bounds, per point and triangle, from the error argument of DESIGN.md §4 ("Nearest-point queries"), u = 2^-24:
      E   = 12 u |S|, S_a = max(|p_a|, |A_a|, |B_a|, |C_a|): the rounded `diff` differs from p - X(u, v), X evaluated exactly on the true
            vertices, by at most 11 u S_a per axis, and X lies within u S_a of the triangle (u + v may exceed 1 by 2^-25);
      (i)  |distance2 - |p - X(u, v)|^2| <= 2 D E + E^2 + 4 u (D + E)^2, D = |p - X(u, v)|: the three roundings of the final dot product;
      (ii) sqrt(distance2) >= (d_true - E) (1 - 2u): no point of the triangle is nearer than the true closest one;
      (iii) sqrt(distance2) <= (d_true + E + 64 u (|p - A| + L) / sin^2(theta_min)) (1 + 2u): the rounded region tests and barycentrics
            displace X along the triangle by at most that (dot products of relative error 5u, the quotients' denominators |e|^2 and
            |e1 x e2|^2 = (L1 L2 sin)^2), L the longest edge, theta_min the smallest corner angle; no bound for a zero-area triangle."""
    for name, (sc, bvh, pts) in cases.items():
        pos = sc.world_vertices["position"].astype(np.float64)
        t = sc.triangles
        ids = bvh["tris"]["tri"].astype(np.int64)
        A, B, C = pos[t["v0"][ids]], pos[t["v1"][ids]], pos[t["v2"][ids]]
        v0, e1, e2, _ = pr.bruteforce.leaf_records(bvh)
        d2, u, v = pr.point_tri(pts, v0, e1, e2)
        p64 = pts.astype(np.float64)
        true = _closest_f64(p64, A, B, C)
        X = A[None] + u.astype(np.float64)[..., None] * (B - A)[None] + v.astype(np.float64)[..., None] * (C - A)[None]
        D = np.sqrt(((p64[:, None, :] - X) ** 2).sum(-1))
        S = np.maximum(np.abs(p64)[:, None, :], np.maximum(np.maximum(np.abs(A), np.abs(B)), np.abs(C))[None])
        E = 12 * U * np.sqrt((S * S).sum(-1))
        got = d2.astype(np.float64)
        assert np.isfinite(got).all(), name
        assert (np.abs(got - D * D) <= 2 * D * E + E * E + 4 * U * (D + E) ** 2).all(), name
        dist, dtrue = np.sqrt(got), np.sqrt(true)
        assert (dist >= np.maximum(dtrue - E, 0.0) * (1 - 2 * U)).all(), name
        edges = [B - A, C - A, C - B]
        L = np.sqrt(np.max([(e * e).sum(-1) for e in edges], axis=0))
        with np.errstate(all="ignore"):
            sin2 = np.min([(np.cross(x, y) ** 2).sum(-1) / ((x * x).sum(-1) * (y * y).sum(-1)) for x, y in ((edges[0], edges[1]), (edges[0], edges[2]), (edges[1], edges[2]))], axis=0)
            shift = 64 * U * (np.sqrt(((p64[:, None, :] - A[None]) ** 2).sum(-1)) + L[None]) / sin2[None]
        shift = np.where(np.isfinite(shift), shift, np.inf)
        assert (dist <= (dtrue + E + shift) * (1 + 2 * U)).all(), (name, float(np.max(dist - dtrue)))
        assert np.isfinite(shift).mean() > 0.9                                # the bound means something on these scenes


def test_region_cases_by_hand():
    """One point per vertex, edge and interior region of the triangle A = (0,0,0), B = (4,0,0), C = (0,4,0); every value is exact."""
    v0, e1, e2 = np.zeros((1, 3), F32), np.array([[4, 0, 0]], F32), np.array([[0, 4, 0]], F32)
    cases = [  # point, region, u, v, distance2
        ((-1, -1, 2), 0, 0.0, 0.0, 6.0),       # vertex A
        ((6, -1, 0), 1, 1.0, 0.0, 5.0),        # vertex B
        ((1, -2, 0), 2, 0.25, 0.0, 4.0),       # edge AB
        ((-1, 6, 1), 3, 0.0, 1.0, 6.0),        # vertex C
        ((-2, 1, 0), 4, 0.0, 0.25, 4.0),       # edge AC
        ((3, 3, 0), 5, 0.5, 0.5, 2.0),         # edge BC
        ((1, 1, 3), 6, 0.25, 0.25, 9.0),       # interior
        ((1, 1, 0), 6, 0.25, 0.25, 0.0),       # on the triangle
        ((0, 0, 0), 0, 0.0, 0.0, 0.0),         # on vertex A
        ((4, 0, 0), 1, 1.0, 0.0, 0.0),         # on vertex B
        ((0, 4, 0), 3, 0.0, 1.0, 0.0),         # on vertex C
    ]
    p = np.array([c[0] for c in cases], F32)
    d2, u, v = pr.point_tri(p, v0, e1, e2)
    assert pr.region_of(p, v0, e1, e2)[:, 0].tolist() == [c[1] for c in cases]
    assert u[:, 0].tolist() == [c[2] for c in cases] and v[:, 0].tolist() == [c[3] for c in cases]
    assert d2[:, 0].tolist() == [c[4] for c in cases]
    assert set(c[1] for c in cases) == set(range(7))
    # the same through k_nearest: the record, the key order of a tie, and the radius at exactly distance2
    tris = np.zeros(2, dtype=capi.BVH_TRI_DTYPE)
    tris["v0"], tris["e1"], tris["e2"], tris["tri"] = v0, e1, e2, [1, 0]                 # the same triangle twice: exact ties
    exact = {0.0: 0.0, 4.0: 2.0, 9.0: 3.0}                                               # radii whose square is distance2 exactly; 3 elsewhere
    hits, counts, totals = pr.k_nearest({"tris": tris}, p, np.array([exact.get(c[4], 3.0) for c in cases], F32), 2)
    assert (counts == 2).all() and (totals == 2).all()
    assert hits["triangle"].tolist() == [[0, 1]] * len(cases) and hits["distance2"][:, 0].tolist() == [c[4] for c in cases]
    below = np.nextafter(np.array([2.0, 3.0], F32), F32(0))                              # radii just below sqrt(4) and sqrt(9)
    _, counts, _ = pr.k_nearest({"tris": tris}, p[[2, 6]], below, 2)
    assert counts.tolist() == [0, 0]


# ---- the cull rule against the rounded triangle arithmetic
def _check_cull(bvh, pts, tag):
    v0, e1, e2, _ = pr.bruteforce.leaf_records(bvh)
    d2, _, _ = pr.point_tri(pts, v0, e1, e2)
    d2 = np.where(np.isnan(d2), np.inf, d2)                                   # a rejected record bounds nothing
    below = pr.leaf_records_below(bvh)
    tested = positive = 0
    for node, slots in zip(bvh["nodes"], below):
        if slots is None:
            continue
        lb2 = pr.child_lower_bounds(node, pts)
        for c, recs in enumerate(slots):
            best = d2[:, recs].min(axis=1)
            # at the bound itself (the list's worst entry is this very triangle) the child must be visited
            assert not pr.culled(lb2[:, c], best).any(), (tag, c, node)
            assert (lb2[:, c] <= best).all(), (tag, c)                        # the argument's stronger statement: monotonic rounding
            tested += len(pts)
            positive += int((lb2[:, c] > 0).sum())
    assert tested > 0 and positive > tested // 4, tag                         # the rule is exercised, not vacuous
    return tested


def test_cull_rule_is_conservative_on_every_child_box(cases):
    for name, (sc, bvh, pts) in cases.items():
        pos = sc.world_vertices["position"]
        lo, hi = pos.min(axis=0).astype(np.float64), pos.max(axis=0).astype(np.float64)
        diam = float(np.linalg.norm(hi - lo))
        rng = np.random.default_rng(17)
        d = rng.normal(size=(40, 3))
        far = ((lo + hi) / 2 + 1e4 * diam * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
        allpts = np.concatenate([pts, far])
        assert _check_cull(bvh, allpts, name) >= 2 * len(allpts) * len(bvh["nodes"])     # every node, every child
    # a scene translated to coordinates near 1e3: the slack grows with the coordinates, as the roundings do
    sc = SCENES["hall_small"][0]()
    sc.world_vertices["position"] += np.array([1000.0, -1000.0, 1000.0], F32)
    bvh = _export(sc)
    pts = _scene_points(sc, bvh, 120, seed=9)
    assert np.abs(pts).max() > 900
    _check_cull(bvh, pts, "translated")


def test_continuation_passes_concatenate_to_one_pass(cases):
    for name in ("cornell", "banana"):
        sc, bvh, pts = cases[name]
        pts = np.concatenate([pts[:30], pts[160:190]])                        # uniform points and points on vertices
        tenth = pr.k_nearest(bvh, pts, np.inf, 10)[0]["distance2"][:, 9]
        radius = np.sqrt(tenth.min())                                         # about ten triangles for the most crowded point, fewer elsewhere
        _, _, totals = pr.k_nearest(bvh, pts, radius, 1)
        kmax = int(totals.max())
        assert kmax > 3, name
        full, full_counts, _ = pr.k_nearest(bvh, pts, radius, kmax)
        assert np.array_equal(full_counts, totals)
        keys = pr.hit_keys(full)
        for i in range(len(pts)):
            assert (np.diff(keys[i, :totals[i]].astype(object)) > 0).all()    # strictly ascending: no triangle twice
            assert (full["distance2"][i, :totals[i]] <= radius * radius).all()
        got = [[] for _ in range(len(pts))]
        after, passes = None, 0
        while True:
            hits, counts, _ = pr.k_nearest(bvh, pts, radius, 3, after=after)
            if not counts.any():
                break
            for i in np.nonzero(counts)[0]:
                got[i].append(hits[i, :counts[i]])
            after = hits[:, 2].copy()                                         # the last record, unused ones included: those points are finished
            passes += 1
        assert passes == -(-kmax // 3)
        for i in range(len(pts)):
            cat = np.concatenate(got[i]) if got[i] else np.empty(0, dtype=capi.POINT_HIT_DTYPE)
            assert pr.records_equal(cat, full[i, :totals[i]]), (name, i)
        flat, offsets = pr.all_within(bvh, pts, radius)
        assert np.array_equal(np.diff(offsets), totals) and pr.records_equal(flat[offsets[7]:offsets[8]], full[7, :totals[7]])


def test_invalid_points_and_degenerate_records(cases):
    sc, bvh, pts = cases["cornell"]
    nan, inf = F32(np.nan), F32(np.inf)
    p = np.array([(nan, 0, 0), (0, inf, 0), (0, 0, -inf), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)], F32)
    md = np.array([1, 1, 1, nan, -1.0, -0.0, inf], F32)
    hits, counts, totals = pr.k_nearest(bvh, p, md, 2)
    assert counts.tolist() == [0, 0, 0, 0, 0, 0, 2] and (hits[:6] == pr.UNUSED).all()
    # zero-area records appended: a point triangle is a vertex (answered), a needle whose rule divides 0 by 0 gives a NaN (rejected)
    tris = np.zeros(len(bvh["tris"]) + 2, dtype=capi.BVH_TRI_DTYPE)
    tris[:-2] = bvh["tris"]
    n = len(sc.triangles)
    tris["v0"][-2:], tris["tri"][-2:] = (0.25, 0.25, 0.25), (n, n + 1)
    tris["e2"][-1] = (0.5, 0, 0)                                              # e1 = 0, e2 != 0
    ext = {"tris": tris}
    q = np.array([(0.25, 0.25, 0.25), (0.5, 0.25, 0.25), (0.3, 0.3, 0.2)], F32)
    d2, u, v = pr.point_tri(q, tris["v0"][-2:], tris["e1"][-2:], tris["e2"][-2:])
    ap = q - tris["v0"][-1]
    want = ((ap[:, 0] * ap[:, 0] + ap[:, 1] * ap[:, 1]) + ap[:, 2] * ap[:, 2]).astype(F32)
    assert np.array_equal(d2[:, 0], want) and (u[:, 0] == 0).all() and (v[:, 0] == 0).all()
    assert d2[0, 1] == 0 and np.isnan(d2[1:, 1]).all()                        # at v0 the vertex case answers; elsewhere 0 / 0
    hits, counts, totals = pr.k_nearest(ext, q, inf, len(tris))
    base = pr.k_nearest(bvh, q, inf, len(tris))[2]
    assert totals.tolist() == (base + np.array([2, 1, 1])).tolist()           # the NaN records are never answered
    assert hits["triangle"][0, :2].tolist() == [n, n + 1] and (hits["distance2"][0, :2] == 0).all()      # exact ties in index order
    assert np.isfinite(hits["distance2"][hits["triangle"] != 0xFFFFFFFF]).all()
