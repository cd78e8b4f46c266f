"""Box-overlap queries (fyprt_overlap_boxes) without a GPU: the symbols and the record's layout, the errors of both entry points in the
header's order on a host-only context, the Python wrappers' argument checks, and the brute-force reference of the GPU tests
(tests/boxes_ref.py) held to what can be known without the kernel: the scenes' own triangles clipped against the box in float64, hand
cases with exactly known answers, the traversal's cull rule against the rounded rule on every child box of every node, and
continuation passes."""
import re
from pathlib import Path

import numpy as np
import pytest

import boxes_ref as br
from common import SCENES
from fypraytracer_amd import capi

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
F32 = np.float32
SCENE_NAMES = ("cornell", "hall_small", "banana")


def test_symbols_record_layout_and_the_header_constant():
    lib = capi.load_library()
    assert {"fyprt_overlap_boxes", "fyprt_overlap_boxes_device"} <= set(capi.EXPORTED_SYMBOLS)
    assert hasattr(lib, "fyprt_overlap_boxes") and hasattr(lib, "fyprt_overlap_boxes_device")
    assert capi.BOX_DTYPE.itemsize == 32
    assert [capi.BOX_DTYPE.fields[k][1] for k in ("lo", "pad0", "hi", "pad1")] == [0, 12, 16, 28]
    header = (Path(__file__).resolve().parent.parent / "include" / "fyprt.h").read_text()
    assert "fyprt_overlap_boxes_device" in header and "typedef struct fyprt_box " in header
    assert int(re.search(r"#define\s+FYPRT_OVERLAP_MAX_HITS\s+(\d+)", header).group(1)) == capi.OVERLAP_MAX_HITS == 32
    assert int(br.NONE) == capi.NO_TRIANGLE == 0xFFFFFFFF and float(br.SLACK) == 2.0 ** -20


def test_errors_in_the_headers_order_on_a_host_only_context():
    lib = capi.load_library()
    ctx = capi.Context(-1)
    boxes = np.zeros(4, dtype=capi.BOX_DTYPE)
    boxes["hi"] = 1.0
    tris = np.zeros((4, 32), dtype=np.uint32)
    counts, totals = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    dev = np.zeros(64, dtype=np.float32)                      # (never dereferenced: every call below fails before a launch)
    base = dev.ctypes.data + (-dev.ctypes.data) % 16          # a 16-byte aligned address inside it

    def host(k=4, r=boxes.ctypes.data, n=4, h=tris.ctypes.data, c=counts.ctypes.data, t=totals.ctypes.data, a=None):
        return lib.fyprt_overlap_boxes(ctx.h, r, a, n, k, h, c, t, None)

    def device(k=4, r=base, n=4, h=base, c=base, t=base, a=None):
        return lib.fyprt_overlap_boxes_device(ctx.h, r, a, n, k, h, c, t)

    for call in (host, device):
        assert call() == ESTATE                                               # no scene yet
        assert call(c=None) == ESTATE and call(t=None) == ESTATE              # hit_counts and totals may be NULL
        for k in (0, 33):
            assert call(k=k) == EINVAL                                        # max_hits before the state ...
            assert call(k=k, r=None) == EINVAL
            assert call(k=k, n=0) == EINVAL                                   # ... and before the empty call
        assert call(r=None) == EINVAL and call(h=None) == EINVAL              # NULL boxes / triangles with count > 0
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
    assert lib.fyprt_overlap_boxes(None, boxes.ctypes.data, None, 4, 4, tris.ctypes.data, None, None, None) == EINVAL
    assert lib.fyprt_overlap_boxes_device(None, None, None, 0, 4, None, None, None) == EINVAL
    with pytest.raises(capi.FyprtError):
        ctx.overlap_boxes(np.zeros((1, 3)), np.ones((1, 3)))
    ctx.close()


def test_argument_error_texts_of_the_three_list_queries():
    """The list queries share one argument check; every entry point keeps its own text, byte for byte (callers may match them)."""
    lib = capi.load_library()
    ctx = capi.Context(-1)
    dev = np.zeros(64, dtype=np.float32)                      # (never dereferenced: every call below fails before a launch)
    base = dev.ctypes.data + (-dev.ctypes.data) % 16
    families = (("fyprt_trace_ray_hits", "rays", "hits", 8, "trace", "rays, after and hits must be 16-byte and hit_counts 4-byte aligned", ()),
                ("fyprt_nearest_points", "points", "hits", 8, "query", "points, after and hits must be 16-byte and hit_counts 4-byte aligned", ()),
                ("fyprt_overlap_boxes", "boxes", "triangles", 32, "query",
                 "boxes must be 16-byte and after, triangles, hit_counts and totals 4-byte aligned", (base,)))

    def text(rc, code):
        assert rc == code
        return lib.fyprt_last_error(ctx.h).decode()

    for name, noun, out, cap, verb, aligned, totals in families:
        host, device = getattr(lib, name), getattr(lib, name + "_device")
        for who, call in ((name, lambda r=base, n=4, k=4, h=base, c=base: host(ctx.h, r, None, n, k, h, c, *totals, None)),
                          (name + "_device", lambda r=base, n=4, k=4, h=base, c=base: device(ctx.h, r, None, n, k, h, c, *totals))):
            assert text(call(k=0), EINVAL) == text(call(k=cap + 1), EINVAL) == f"{who}: max_hits must be 1..{cap}"
            assert text(call(r=None), EINVAL) == text(call(h=None), EINVAL) == f"{who}: NULL {noun} / {out} with a non-zero count"
            assert text(call(), ESTATE) == f"{who}: host-only context (device -1) cannot {verb}"      # (comes before the scene's state)
        assert text(device(ctx.h, base + 4, None, 4, 4, base, base, *totals), EINVAL) == f"{name}_device: {aligned}"
        assert text(device(ctx.h, base, None, 4, 4, base, base + 2, *totals), EINVAL) == f"{name}_device: {aligned}"
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
        lo, hi = np.zeros((3, 3), F32), np.ones((3, 3), F32)
        for bad in (0, 33, -1, 2.5, True, None):
            with pytest.raises(ValueError):
                ctx.overlap_boxes(lo, hi, max_hits=bad)
            with pytest.raises(ValueError):
                ctx.triangles_in_boxes(lo, hi, max_hits=bad)
            with pytest.raises(ValueError):
                ctx.overlap_boxes_tensor(None, bad)
        for bad_corner in (np.zeros((3, 2), F32), np.zeros(4, F32), F32(1.0), np.zeros((2, 3), F32)):     # the last: a different count
            with pytest.raises(ValueError):
                ctx.overlap_boxes(bad_corner, hi)
            with pytest.raises(ValueError):
                ctx.overlap_boxes(lo, bad_corner)
            with pytest.raises(ValueError):
                ctx.triangles_in_boxes(lo, bad_corner)
        with pytest.raises(ValueError):
            ctx.overlap_boxes(lo, hi, after=np.zeros(2, dtype=np.uint32))                   # wrong length
        with pytest.raises(ValueError):
            ctx.overlap_boxes(lo, hi, after=np.zeros(3, dtype=np.int64))                    # wrong dtype
        import torch
        for boxes in (None, torch.zeros(4, 6), torch.zeros(4, 8, dtype=torch.float64), torch.zeros(8, 4).t()[:, :], torch.zeros(8, 8)[::2], torch.zeros(4, 8)):   # the last: not on the GPU
            with pytest.raises(ValueError):
                ctx.overlap_boxes_tensor(boxes, 4)
    finally:
        ctx.lib = real
    ctx.close()


# ---- the scenes, their exported trees and a box set each
def _export(sc):
    ctx = capi.Context(-1)
    ctx.set_tuning(12, 0)
    ctx.upload_scene(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    return bvh


def _scene_boxes(sc, bvh, n, seed):
    """Random boxes of several sizes in the scene box, boxes with one face through a vertex, boxes with faces on decoded child planes of
    the tree's nodes, and point boxes on vertices."""
    rng = np.random.default_rng(seed)
    pos = sc.world_vertices["position"].astype(np.float64)
    slo, shi = pos.min(axis=0), pos.max(axis=0)
    ext = shi - slo
    centre = rng.uniform(slo - 0.1 * ext, shi + 0.1 * ext, size=(n, 3))
    half = ext[None, :] * rng.choice([0.01, 0.05, 0.2], size=(n, 1)) * rng.uniform(0.3, 1.0, size=(n, 3))
    lo, hi = (centre - half).astype(F32), (centre + half).astype(F32)
    snap = rng.integers(0, len(pos), n // 2)                                  # one face of every second box through a vertex
    for j, v in enumerate(snap):
        a = int(rng.integers(0, 3))
        if rng.integers(0, 2):
            lo[2 * j, a] = F32(pos[v, a]); hi[2 * j, a] = max(hi[2 * j, a], lo[2 * j, a])
        else:
            hi[2 * j, a] = F32(pos[v, a]); lo[2 * j, a] = min(lo[2 * j, a], hi[2 * j, a])
    plo, phi = [], []
    for node in bvh["nodes"][rng.integers(0, len(bvh["nodes"]), n // 4)] if len(bvh["nodes"]) else []:
        blo, bhi = br.child_planes(node)
        c = int(rng.integers(0, len(blo)))
        d = (bhi[c] - blo[c]) * F32(0.5) + F32(0.01)
        side = rng.integers(0, 2, 3) == 1                                     # per axis: the box ends on the child's lo plane, or begins on its hi plane
        plo.append(np.where(side, blo[c] - d, bhi[c]).astype(F32))
        phi.append(np.where(side, blo[c], bhi[c] + d).astype(F32))
        plo.append(blo[c]); phi.append(bhi[c])                                # the child's own box
    verts = sc.world_vertices["position"][rng.integers(0, len(pos), n // 8)].astype(F32)
    lo = np.concatenate([lo] + ([np.array(plo, F32)] if plo else []) + [verts]).astype(F32)
    hi = np.concatenate([hi] + ([np.array(phi, F32)] if phi else []) + [verts]).astype(F32)
    assert not br.invalid_boxes(lo, hi).any()
    return lo, hi


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in SCENE_NAMES:
        sc = SCENES[name][0]()
        bvh = _export(sc)
        lo, hi = _scene_boxes(sc, bvh, 96, seed=5)
        out[name] = (sc, bvh, lo, hi, br.accepted(bvh, lo, hi))
    return out


# ---- the reference against float64 clipping on the caller's own vertices
def _clip_nonempty(tri, lo, hi):
    """Sutherland–Hodgman in float64, vectorised over pairs: triangle (N, 3, 3) clipped against the six half-spaces of [lo, hi] (N, 3);
    True where a vertex is left.  Boundary points are inside: the box is closed."""
    n, slots = len(tri), 12                                                   # a triangle cut by six planes has at most nine vertices
    poly = np.zeros((n, slots, 3))
    poly[:, :3] = tri
    cnt = np.full(n, 3)
    j = np.arange(slots)[None, :]
    rows = np.arange(n)[:, None]
    for axis in range(3):
        for sign, bound in ((1.0, hi[:, axis]), (-1.0, lo[:, axis])):
            dist = sign * (bound[:, None] - poly[:, :, axis])                 # >= 0 inside
            nxt = (j + 1) % np.maximum(cnt, 1)[:, None]
            valid = j < cnt[:, None]
            dn = np.take_along_axis(dist, nxt, axis=1)
            pn = poly[rows, nxt]
            inside, inside_n = dist >= 0, dn >= 0
            keep = valid & inside
            cross = valid & (inside != inside_n)
            with np.errstate(all="ignore"):
                t = np.where(cross, dist / (dist - dn), 0.0)
            cut = poly + t[..., None] * (pn - poly)
            cut[..., axis] = np.where(cross, bound[:, None], cut[..., axis])   # exactly on the plane: later planes see no drift
            flags = np.stack([keep, cross], axis=2).reshape(n, 2 * slots)     # output order: the vertex, then the cut of its edge
            pts = np.stack([poly, cut], axis=2).reshape(n, 2 * slots, 3)
            place = np.cumsum(flags, axis=1) - 1
            cnt = flags.sum(axis=1)
            assert cnt.max(initial=0) <= slots
            new = np.zeros_like(poly)
            r, c = np.nonzero(flags)
            new[r, place[r, c]] = pts[r, c]
            poly = new
    return cnt > 0


def test_reference_agrees_with_float64_clipping(cases):
    """The float32 rule against an independent fact, the caller's own triangle clipped against the box in float64: non-empty iff they
    overlap.  The two may differ only where the float64 decision itself flips when the box is grown or shrunk by 2^-18 * m per side, m
    the largest coordinate magnitude of the box and the scene — rounding moves the record's vertices, the centre and the products by a
    few 2^-24 m, a decision that far from flipping cannot change.  Such pairs are at most 1 % of all pairs."""
    for name, (sc, bvh, lo, hi, (ok, ids)) in cases.items():
        pos = sc.world_vertices["position"].astype(np.float64)
        t = sc.triangles
        order = bvh["tris"]["tri"].astype(np.int64)
        tri = np.stack([pos[t["v0"][order]], pos[t["v1"][order]], pos[t["v2"][order]]], axis=1)          # (T, 3, 3), leaf-record order
        lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
        m = np.maximum(np.abs(lo64).max(axis=1), np.abs(hi64).max(axis=1))
        m = np.maximum(m, np.abs(pos).max())[:, None]
        grow = 2.0 ** -18 * m
        # far pairs need no clipping: bounding boxes apart by more than the margin are apart in every variant, and the rule must say so
        tlo, thi = tri.min(axis=1), tri.max(axis=1)
        near = ((tlo[None] <= (hi64 + grow)[:, None]) & (thi[None] >= (lo64 - grow)[:, None])).all(axis=2)
        assert not ok[~near].any(), name
        b, k = np.nonzero(near)
        exact = _clip_nonempty(tri[k], lo64[b], hi64[b])
        differ = exact != ok[b, k]
        if differ.any():
            bd, kd = b[differ], k[differ]
            grown = _clip_nonempty(tri[kd], (lo64 - grow)[bd], (hi64 + grow)[bd])
            shrunk_box_ok = ((lo64 + grow) <= (hi64 - grow)).all(axis=1)[bd]
            shrunk = _clip_nonempty(tri[kd], (lo64 + grow)[bd], (hi64 - grow)[bd]) & shrunk_box_ok           # a box thinner than the margin shrinks to nothing
            assert (grown != shrunk).all(), (name, int((grown == shrunk).sum()), bd[grown == shrunk][:4], kd[grown == shrunk][:4])
        assert differ.sum() <= 0.01 * ok.size, (name, int(differ.sum()), ok.size)
        assert exact.any() and (~exact).any(), name                           # both answers occur among the near pairs


# ---- hand cases
def _records(*tris):
    """Leaf records of triangles given by their vertices, as the builders form them: v0, fl(v1 - v0), fl(v2 - v0)."""
    t = np.array(tris, F32)
    return t[:, 0], (t[:, 1] - t[:, 0]).astype(F32), (t[:, 2] - t[:, 0]).astype(F32)


def test_cases_by_hand():
    big = ((-10, -10, 0), (30, -10, 0), (-10, 30, 0))                         # a large triangle in z = 0; its hypotenuse is x + y = 20
    v0, e1, e2 = _records(big)

    def ask(lo, hi, steps=False):
        r = br.box_tri(np.array([lo], F32), np.array([hi], F32), v0, e1, e2, steps)
        return tuple(bool(x[0, 0]) for x in r) if steps else bool(r[0, 0])
    assert ask((1, 1, -1), (2, 2, 1))                                         # a box inside the triangle: no vertex in it, no edge through it
    assert ask((1, 1, 1), (2, 2, 3), steps=True) == (False, False, False)     # above it: the z axis, the in-plane edges' axes and the plane all separate
    # beside the plane, inside the triangle's bounding box on every axis: a tilted triangle, only the plane separates
    tv0, te1, te2 = _records(((0, 0, 0), (8, 0, 8), (0, 8, 8)))
    r = br.box_tri(np.array([(1, 1, 5)], F32), np.array([(2, 2, 6)], F32), tv0, te1, te2, steps=True)
    assert tuple(bool(x[0, 0]) for x in r) == (True, True, False)
    r = br.box_tri(np.array([(1, 1, 2)], F32), np.array([(2, 2, 3)], F32), tv0, te1, te2, steps=True)
    assert tuple(bool(x[0, 0]) for x in r) == (True, True, True)              # the plane z = x + y passes through this one
    # beyond the hypotenuse, in the plane and inside the bounding box: only an edge axis separates
    assert ask((12, 12, -1), (13, 13, 1), steps=True) == (True, False, True)
    assert ask((9, 9, -1), (10, 10, 1))                                       # its corner (10, 10) on the hypotenuse: touching, exact
    assert ask((10, 10, -1), (11, 11, 1))                                     # touching from outside
    assert not ask((10.001, 10.001, -1), (11, 11, 1))
    # a touching face: the box ends exactly on z = 0 / begins on it; one ulp away it does not touch
    assert ask((1, 1, -2), (2, 2, 0)) and ask((1, 1, 0), (2, 2, 2))
    assert not ask((1, 1, -2), (2, 2, np.nextafter(F32(0), F32(-1)))) and not ask((1, 1, np.nextafter(F32(0), F32(1))), (2, 2, 2))
    # a point box on v0 always accepts its record, whatever the edges; at the caller's second vertex it need not
    rng = np.random.default_rng(1)
    V = rng.uniform(-100, 100, size=(600, 3, 3)).astype(F32)
    rv0, re1, re2 = _records(*V)
    own = br.box_tri(rv0, rv0, rv0, re1, re2)
    assert own.diagonal().all()                                               # p_0 = 0: every s_0 and d are 0, and 0 <= 0
    axes, edges, plane = (x.diagonal() for x in br.box_tri(V[:, 1], V[:, 1], rv0, re1, re2, steps=True))
    same = (rv0 + re1 == V[:, 1]).all(axis=1)                                 # the record's second vertex is the caller's
    assert same.any() and (~same).any()
    assert axes[same].all() and edges[same].all()                             # p_1 = 0 there: every s_1 is 0 ...
    assert not (axes & edges & plane).all()                                   # ... but d = dot(n, v0 - V1) is rounded, and r is 0
    # zero-area records: step 2 alone decides — a point triangle and a needle along x
    zv0, ze1, ze2 = _records(((1, 2, 3), (1, 2, 3), (1, 2, 3)), ((0, 0, 0), (0, 0, 0), (4, 0, 0)))
    lo = np.array([(1, 2, 3), (0.5, 1.5, 2.5), (1.5, 1.5, 2.5), (2, 0, 0), (2, -1, -1), (2, 0.5, -1), (5, 0, 0)], F32)
    hi = np.array([(1, 2, 3), (1, 2, 3), (2, 2.5, 3.5), (2, 0, 0), (3, 1, 1), (3, 1, 1), (6, 0, 0)], F32)
    got = br.box_tri(lo, hi, zv0, ze1, ze2)
    axes = br.box_tri(lo, hi, zv0, ze1, ze2, steps=True)[0]
    assert got[:, 0].tolist() == [True, True, False, False, False, False, False]
    assert got[:, 1].tolist() == [False, False, False, True, True, False, False]
    assert np.array_equal(got, axes)
    # NaN and infinite records are never accepted, whichever field holds them; nor is anything by an invalid box
    nan, inf = F32(np.nan), F32(np.inf)
    everything = (np.array([(-1e30, -1e30, -1e30)], F32), np.array([(1e30, 1e30, 1e30)], F32))
    assert br.box_tri(*everything, v0, e1, e2)[0, 0]
    for field in range(3):
        for comp in range(3):
            rec = [v0.copy(), e1.copy(), e2.copy()]
            rec[field][0, comp] = nan
            assert not br.box_tri(*everything, *rec)[0, 0], (field, comp)
    tris = np.zeros(1, dtype=capi.BVH_TRI_DTYPE)
    tris["v0"], tris["e1"], tris["e2"], tris["tri"] = v0, e1, e2, [7]
    bad_lo = np.array([(0, 0, 0), (nan, 0, 0), (0, 0, 0), (-inf, 0, 0), (-3e38, 0, 0), (2, 0, 0), (0, 0, 0)], F32)
    bad_hi = np.array([(1, 1, 1), (1, 1, 1), (1, nan, 1), (1, 1, 1), (3e38, 1, 1), (1, 1, 1), (1, 1, inf)], F32)
    assert br.invalid_boxes(bad_lo, bad_hi).tolist() == [False, True, True, True, True, True, True]
    t, c, tot = br.k_lowest({"tris": tris}, bad_lo, bad_hi, 2)
    assert c.tolist() == [1, 0, 0, 0, 0, 0, 0] and tot.tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert t[0].tolist() == [7, 0xFFFFFFFF] and (t[1:] == br.NONE).all()
    assert br.k_lowest({"tris": tris}, bad_lo[:1], bad_hi[:1], 2, after=np.array([7], np.uint32))[2].tolist() == [0]
    assert br.k_lowest({"tris": tris}, bad_lo[:1], bad_hi[:1], 2, after=np.array([6], np.uint32))[1].tolist() == [1]
    assert br.k_lowest({"tris": tris}, bad_lo[:1], bad_hi[:1], 2, after=np.array([0xFFFFFFFF], np.uint32))[2].tolist() == [0]


# ---- the cull rule against the rounded rule
def _check_cull(bvh, lo, hi, ok, tag):
    below = br.leaf_records_below(bvh)
    tested = skipped = 0
    for node, slots in zip(bvh["nodes"], below):
        if slots is None:
            continue
        apart = br.children_apart(node, lo, hi)
        for c, recs in enumerate(slots):
            wanted = ok[:, recs].any(axis=1)                                  # an accepted record below this child
            assert not (apart[:, c] & wanted).any(), (tag, c, node, np.nonzero(apart[:, c] & wanted)[0][:4])
            tested += len(lo)
            skipped += int(apart[:, c].sum())
    assert tested > 0 and skipped > tested // 4, (tag, skipped, tested)       # the rule is exercised, not vacuous
    return tested


def test_cull_rule_skips_no_child_with_an_accepted_record(cases):
    for name, (sc, bvh, lo, hi, (ok, ids)) in cases.items():
        assert _check_cull(bvh, lo, hi, ok, name) >= 2 * len(lo) * len(bvh["nodes"])       # every node, every child
    # a scene translated to coordinates near 1e3: the slack grows with the coordinates, as the roundings do
    sc = SCENES["hall_small"][0]()
    sc.world_vertices["position"] += np.array([1000.0, -1000.0, 1000.0], F32)
    bvh = _export(sc)
    lo, hi = _scene_boxes(sc, bvh, 64, seed=9)
    assert np.abs(lo).max() > 900
    _check_cull(bvh, lo, hi, br.accepted(bvh, lo, hi)[0], "translated")


def test_the_rounded_vertices_leave_the_planes_by_less_than_the_slack():
    """The derivation of DESIGN.md §4 on random triangles: |fl(V0 + fl(V1 - V0)) - V1| <= 3 * 2^-24 * max(|V0|, |V1|) (1 + 2^-23), a
    fifth of the slack k * max(|planeLo|, |planeHi|) >= 2^-20 * max(|V0|, |V1|) (1 - 2^-24)."""
    rng = np.random.default_rng(7)
    a = (rng.uniform(-1, 1, 400000) * 2.0 ** rng.integers(-20, 20, 400000)).astype(F32)
    b = (rng.uniform(-1, 1, 400000) * 2.0 ** rng.integers(-20, 20, 400000)).astype(F32)
    b[::4] = (a[::4] * (1 + rng.uniform(-1e-3, 1e-3, 100000))).astype(F32)   # nearly equal: short edges far from the origin
    got = (a + (b - a).astype(F32)).astype(F32).astype(np.float64)
    err = np.abs(got - b.astype(np.float64))
    m = np.maximum(np.abs(a), np.abs(b)).astype(np.float64)
    assert (err <= 3 * 2.0 ** -24 * m * (1 + 2.0 ** -23)).all()
    assert err.max() > 0 and (err / m).max() > 2.0 ** -25                     # and the rounded vertex does leave them


def test_continuation_passes_concatenate_to_one_pass(cases):
    for name in ("cornell", "banana"):
        sc, bvh, lo, hi, ok_ids = cases[name]
        flat, offsets = br.all_in_boxes(bvh, lo, hi, ok_ids)
        _, _, totals = br.k_lowest(bvh, lo, hi, 1, ok_ids=ok_ids)
        assert np.array_equal(np.diff(offsets), totals) and totals.max() > 6 and (totals == 0).any(), name
        got = [[] for _ in range(len(lo))]
        after, passes = None, 0
        while True:
            tris, counts, tot = br.k_lowest(bvh, lo, hi, 3, after=after, ok_ids=ok_ids)
            if not counts.any():
                break
            done = np.array([sum(len(x) for x in g) for g in got])
            assert np.array_equal(tot, totals - done)                         # the total tells what is still to come, this pass included
            for i in np.nonzero(counts)[0]:
                got[i].append(tris[i, :counts[i]])
            after = tris[:, 2].copy()                                         # the last slot, unused ones included: those boxes are finished
            passes += 1
        assert passes == -(-int(totals.max()) // 3)
        for i in range(len(lo)):
            cat = np.concatenate(got[i]) if got[i] else np.empty(0, dtype=np.uint32)
            assert np.array_equal(cat, flat[offsets[i]:offsets[i + 1]]), (name, i)
            assert (np.diff(cat.astype(np.int64)) > 0).all()                  # strictly ascending: no triangle twice


def test_the_slack_is_needed_and_suffices_where_a_rounded_vertex_leaves_the_planes(cases):
    """banana has records whose rounded second or third vertex lies outside a decoded plane above them.  A box that begins exactly on
    such a vertex accepts the record; a cull without slack would skip the child, the cull with it does not."""
    sc, bvh = cases["banana"][:2]
    lo, hi, where = br.protruding_boxes(bvh)
    assert len(where) >= 10
    ok, _ = br.accepted(bvh, lo, hi)
    lost = kept = 0
    for i, (ni, c, r) in enumerate(where):
        if not ok[i, r]:
            continue
        lost += int(br.children_apart(bvh["nodes"][ni], lo[i:i + 1], hi[i:i + 1], slack=0.0)[0, c])
        kept += int(not br.children_apart(bvh["nodes"][ni], lo[i:i + 1], hi[i:i + 1])[0, c])
    assert lost >= 10 and kept == int(sum(ok[i, r] for i, (_, _, r) in enumerate(where)))
    _check_cull(bvh, lo, hi, ok, "protruding")
