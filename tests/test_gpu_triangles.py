"""Triangle-overlap queries on the GPU (fyprt_overlap_triangles / fyprt_overlap_triangles_device, rt_triangles.h: TriLaneT behind
rt_query.h's kernel templates).  Every comparison is bit for bit against tests/triangles_ref.py (every leaf record of ctx.export_bvh()
tested, no tree): indices, unused slots, counts and totals.
  * a stack of 40 parallel triangles and query triangles through all of them: every K from 1 to 32, both kernels of tuning key 15;
  * hall_small under the three builders: random triangles of three sizes, the scene's own triangles unmoved and jittered, triangles
    with a vertex bit-equal to a record's v0, triangles in the planes of the scene's flat quads, zero-area and invalid ones; the cull
    rule on each builder's exported tree; continuation against all_touching;
  * stack budget extremes; the seams of the persistent kernel's scheduling, counted and uncounted; counters on hand-countable trees;
    invalid, empty and misaligned calls; banana_standin's protruding rounded vertices; the query filter; the editor sequence (append,
    mask out, move into a wall, remove); frames and the other families untouched; device memory; the torch path."""

import numpy as np
import pytest

import boxes_ref as br
import filter_ref as fr
import triangles_ref as tr
from common import SCENES, bits_equal, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

F32 = np.float32
KMAX = capi.OVERLAP_MAX_HITS


def _ctx(sc, key15=0, counting=False, builder=0):
    ctx = capi.Context(0)
    ctx.set_tuning(15, key15)
    ctx.set_tuning(12, builder)
    ctx.upload_scene(sc)
    ctx.set_ray_counting(counting)
    return ctx


def _truncate(ref, k):
    """The answer for max_hits = k from a reference computed with a larger K: the k lowest indices are a prefix of the K lowest."""
    tris, _, totals = ref
    return np.ascontiguousarray(tris[:, :k]), np.minimum(totals, k).astype(np.uint32), totals


def _rows(ref, sel):
    return tuple(np.ascontiguousarray(a[sel]) for a in ref[:3])


def _assert_equal(got, want, tag):
    (gt, gc, gn), (wt, wc, wn) = got[:3], want[:3]
    assert gt.shape == wt.shape and gt.dtype == np.uint32 and gc.dtype == np.uint32 and gn.dtype == np.uint32
    bad = np.nonzero((gt != wt).any(axis=1))[0]
    assert len(bad) == 0, (tag, len(bad), bad[:8], gt[bad[:2]], wt[bad[:2]])
    assert np.array_equal(gc, wc), (tag, np.nonzero(gc != wc)[0][:8])
    assert np.array_equal(gn, wn), (tag, np.nonzero(gn != wn)[0][:8], gn[gn != wn][:8], wn[gn != wn][:8])


def _same_leaf_records(a, b):
    ka, kb = np.argsort(a["tris"]["tri"]), np.argsort(b["tris"]["tri"])
    return all(np.array_equal(a["tris"][f][ka].view(np.uint32), b["tris"][f][kb].view(np.uint32)) for f in ("v0", "e1", "e2", "tri"))


def _stats(st):
    return (st.rays, st.box_tests, st.tri_tests, st.hits, st.node_visits)


# ---- the stack: 40 parallel triangles 0.1 apart (normal +y), every one its own mesh
def _stack_scene(n=40):
    from fypraytracer_amd.scene import Material, Scene
    sc = Scene()
    sc.materials = [Material(albedo=(1, 1, 1), roughness=1.0, metallic=0.0), Material(albedo=(1, 1, 1), emission_color=(1, 1, 1), emission_power=5.0)]
    nrm, uv, idx = np.tile(np.array([0, 1, 0], F32), (3, 1)), np.array([[0, 0], [1, 0], [0, 1]], F32), np.array([[0, 1, 2]], np.uint32)
    for j in range(n):
        y = -0.1 * j
        sc.add_new_mesh_to_scene(np.array([(-1, y, -1), (2, y, -1), (-1, y, 2)], F32), nrm, uv, idx, material_index=1 if j == n - 1 else 0)
    sc.init_scene_emissive_triangles()
    return sc


@pytest.fixture(scope="module")
def stack():
    sc = _stack_scene()
    rng = np.random.default_rng(3)
    through = np.array([((0, 1, 0), (0.1, -5, 0), (0, -5, 0.1))] * 8, F32)                      # a sliver through all 40
    through[1:] += rng.uniform(-0.2, 0.2, size=(7, 1, 3)).astype(F32) * np.array([1, 0, 1], F32)
    part = through.copy()                                                                       # ends between the layers: some of them
    part[:, 1:, 1] = rng.uniform(-3.9, -0.05, size=(8, 1)).astype(F32)
    on = np.array([((0, -0.1 * j, 0), (0.5, -0.1 * j, 0), (0, -0.1 * j, 0.5)) for j in (0, 7, 39)], F32)   # lying in a layer
    q = np.concatenate([through, part, on]).astype(F32)
    ctx = _ctx(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    ref = tr.k_lowest(bvh, q, KMAX)
    assert len(bvh["tris"]) == 40 and (ref[2][:8] == 40).all() and ((ref[2][8:16] > 0) & (ref[2][8:16] < 40)).all()
    return sc, q, bvh, ref


@pytest.mark.parametrize("key15", [1, 2])
def test_stack_every_k_both_kernels(stack, key15):
    sc, q, bvh, ref = stack
    ctx = _ctx(sc, key15)
    for k in range(1, KMAX + 1):
        got = ctx.overlap_triangles(q, max_hits=k)
        _assert_equal(got, _truncate(ref, k), (key15, k))
        assert (got[2][:8] == 40).all() and (got[0][:8, :k] == np.arange(k, dtype=np.uint32)).all()
    ctx.close()


# ---- hall_small
def _flat_quad_queries(bvh, n, seed):
    """Triangles lying in the planes of the scene's axis-aligned flat surfaces: records whose three rounded vertices share a
    coordinate exactly; the query is the record's triangle shrunk, shifted within the plane, and one that leaves the surface."""
    v0, e1, e2, _ = br.bruteforce.leaf_records(bvh)
    v1, v2 = (v0 + e1).astype(F32), (v0 + e2).astype(F32)
    rng = np.random.default_rng(seed)
    out = []
    for a in range(3):
        flat = np.nonzero((v0[:, a] == v1[:, a]) & (v0[:, a] == v2[:, a]))[0]
        for r in flat[rng.permutation(len(flat))[: n // 3]]:
            t = np.stack([v0[r], v1[r], v2[r]]).astype(np.float64)
            c = t.mean(axis=0)
            shift = rng.normal(size=3) * np.abs(t - c).max() * rng.choice([0.2, 1.0, 3.0])
            shift[a] = 0.0
            moved = ((t - c) * rng.uniform(0.2, 1.2) + c + shift).astype(F32)
            moved[:, a] = v0[r, a]                                            # exactly in the plane
            out.append(moved)
    return np.array(out, F32).reshape(-1, 3, 3)


@pytest.fixture(scope="module")
def hall_small():
    sc = SCENES["hall_small"][0]()
    ctx = _ctx(sc)
    bvh = ctx.export_bvh()
    ctx.close()
    q = tr.scene_queries(sc, bvh, 112, seed=17)                                  # random (three sizes), own, jittered, shared v0, zero-area
    flat = _flat_quad_queries(bvh, 48, seed=19)
    assert len(flat) >= 24
    bad = q[:6].copy()
    bad[0, 0, 0] = np.nan; bad[1, 1, 1] = np.inf; bad[2, 2, 2] = -np.inf
    bad[3, 0, 0], bad[3, 1, 0] = -3e38, 3e38; bad[4, 0, 2], bad[4, 2, 2] = 3e38, -3e38; bad[5] = np.nan
    q = np.concatenate([q, flat, bad]).astype(F32)
    assert 280 <= len(q) <= 420 and tr.invalid_triangles(q).sum() == 6
    ok_ids = tr.accepted(bvh, q)
    ref = tr.k_lowest(bvh, q, KMAX, ok_ids=ok_ids)
    totals = ref[2]
    assert (totals == 0).sum() > 20 and ((totals > 0) & (totals < 8)).sum() > 20 and (totals > 32).any()
    assert (totals[112:112 + 56] > 0).all()                                   # the scene's own triangles touch themselves at least
    assert (totals[-len(flat) - 6:-6] > 0).sum() > len(flat) // 3 and (totals[-6:] == 0).all()
    return sc, q, bvh, ref, ok_ids


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_hall_small_equals_bruteforce(hall_small, builder):
    sc, q, bvh, ref, ok_ids = hall_small
    for key15 in (1, 2):
        ctx = _ctx(sc, key15, builder=builder)
        tree = ctx.export_bvh()
        assert _same_leaf_records(tree, bvh)                                  # the reference is a function of the leaf records alone
        for k in (1, 8, 32):
            _assert_equal(ctx.overlap_triangles(q, max_hits=k), _truncate(ref, k), (builder, key15, k))
        if key15 == 1:
            # the cull on this builder's tree: the leaf records come in another order, the decisions are per record
            order = np.argsort(tree["tris"]["tri"])[np.argsort(np.argsort(bvh["tris"]["tri"]))]
            ok_here = np.empty_like(ok_ids[0])
            ok_here[:, order] = ok_ids[0]
            assert np.array_equal(tree["tris"]["tri"][order], bvh["tris"]["tri"])
            tr.check_cull(tree, q, ok_here, ("hall_small", builder))
            few = np.nonzero(ref[2] <= 60)[0][::3]
            got, off = ctx.triangles_touching(q[few], max_hits=8)
            want, want_off = tr.all_touching(bvh, q[few], ok_ids=(ok_ids[0][few], ok_ids[1]))
            assert got.dtype == np.uint32 and np.array_equal(off, want_off) and np.array_equal(got, want), builder
            assert np.diff(want_off).max() > 8 and (np.diff(want_off) == 0).any()
        ctx.close()


@pytest.mark.parametrize("builder", [1, 2])
@pytest.mark.parametrize("name", ["cornell", "banana_standin"])
def test_cull_rule_on_the_device_builders_trees(name, builder):
    """The cull check of tests/test_triangles_cpu.py (host builder) on the device builders' exports of the other two scenes; hall_small's
    are checked above.  The answers on the same tree, both kernels, against the reference."""
    sc = SCENES[name][0]()
    ctx = _ctx(sc, 1, builder=builder)
    tree = ctx.export_bvh()
    q = tr.scene_queries(sc, tree, 48, seed=5)
    ok_ids = tr.accepted(tree, q)
    assert ok_ids[0].any(axis=1).sum() > len(q) // 4
    tr.check_cull(tree, q, ok_ids[0], (name, builder))
    want = tr.k_lowest(tree, q, 8, ok_ids=ok_ids)
    _assert_equal(ctx.overlap_triangles(q, max_hits=8), want, (name, builder, 1))
    ctx.set_tuning(15, 2)
    _assert_equal(ctx.overlap_triangles(q, max_hits=8), want, (name, builder, 2))
    ctx.close()


@pytest.mark.parametrize("budget", [1, 31])
def test_stack_budget_extremes(hall_small, budget):
    """Tuning key 8 at its ends: the smallest budget makes the node visit push resume entries, which fetch a node again — no index
    twice, no record counted twice; the largest, with K = 32, is the 64 KB workgroup."""
    sc, q, bvh, ref = hall_small[:4]
    for key15 in (1, 2):
        ctx = capi.Context(0)
        ctx.set_tuning(15, key15)
        ctx.set_tuning(8, budget)
        ctx.upload_scene(sc)
        assert (ctx.get_tuning(8) == 31) == (budget == 31)
        _assert_equal(ctx.overlap_triangles(q, max_hits=32), ref, (budget, key15))
        ctx.close()


# ---- seams of the scheduling, counters
def _cull_counts(bvh, q):
    """What the walk counts for each query triangle by the reference cull alone: (child boxes tested, records tested, nodes visited).
    Every child of a visited node is a box test; a leaf child that is not apart has all its records tested."""
    lo, hi = tr.bounds(q)
    out = []
    for i in range(len(q)):
        if tr.invalid_triangles(q[i:i + 1])[0]:
            out.append((0, 0, 0))
            continue
        if bvh["root"] < 0 or len(bvh["nodes"]) == 0:
            out.append((0, len(bvh["tris"]), 0))
            continue
        boxes = tris = nodes = 0
        todo = [int(bvh["root"])]
        while todo:
            node = bvh["nodes"][todo.pop()]
            nodes += 1
            cnt = int(node["meta"]) & 7
            boxes += cnt
            apart = tr.children_apart(node, lo[i:i + 1], hi[i:i + 1])[0]
            for c in range(cnt):
                if apart[c]:
                    continue
                ref = int(node["child"][c])
                if ref >= 0:
                    todo.append(ref)
                else:
                    tris += ((~ref) & 3) + 1
        out.append((boxes, tris, nodes))
    return np.array(out, dtype=np.int64)


def test_seams_counted_and_uncounted():
    sc = SCENES["banana_standin"][0]()
    ctx = _ctx(sc)
    bvh = ctx.export_bvh()
    q = tr.scene_queries(sc, bvh, 400, seed=23)[:1025]
    assert len(q) == 1025
    ref = tr.k_lowest(bvh, q, 3)
    want_counts = _cull_counts(bvh, q[:65])
    ctx.close()
    for key15 in (1, 2):
        ctx = _ctx(sc, key15)
        if key15 == 1:
            for key, value in ((4, 16), (9, 1), (10, 16)):
                ctx.set_tuning(key, value)
        for n in (1, 63, 64, 65, 257, 1025):
            for counting in (False, True):
                ctx.set_ray_counting(counting)
                got = ctx.overlap_triangles(q[:n], max_hits=3, with_stats=True)
                _assert_equal(got, _rows(ref, slice(0, n)), (key15, n, counting))
                st = got[3]
                assert st.launches == 1
                if counting:
                    assert st.rays == n and st.hits == int((got[1] > 0).sum())
                    if n <= 65:
                        # every record is tested once; a node may be fetched again through a resume entry, never less often than the cull says
                        boxes, tris, nodes = (int(v) for v in want_counts[:n].sum(axis=0))
                        assert st.tri_tests == tris and st.node_visits >= nodes and st.box_tests >= boxes, (key15, n, _stats(st), (boxes, tris, nodes))
        ctx.close()


def test_counters_on_hand_countable_trees():
    from fypraytracer_amd.scene import Material, Scene
    from fypraytracer_amd.scenes import _quad
    one = Scene()
    one.materials = [Material(albedo=(1, 1, 1), emission_color=(1, 1, 1), emission_power=5.0)]
    one.add_new_mesh_to_scene(*_quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0)), material_index=0)
    one.init_scene_emissive_triangles()
    through = np.array([((0.5, -1, 0.25), (0.5, 1, 0.25), (0.6, 1, 0.25))], F32)      # pierces the first triangle of the quad only
    for key15 in (1, 2):
        # a one-leaf tree: the root reference is the leaf of both triangles — no node visit, two triangle tests
        ctx = _ctx(one, key15, counting=True)
        bvh = ctx.export_bvh()
        assert len(bvh["nodes"]) == 0 and bvh["root"] < 0 and len(bvh["tris"]) == 2
        got = ctx.overlap_triangles(through, max_hits=2, with_stats=True)
        assert _stats(got[3]) == (1, 0, 2, 1, 0)
        _assert_equal(got, tr.k_lowest(bvh, through, 2), "one leaf")
        assert got[2][0] == 1
        got = ctx.overlap_triangles(through + F32(3), max_hits=2, with_stats=True)
        assert _stats(got[3]) == (1, 0, 2, 0, 0) and got[1][0] == 0 and got[2][0] == 0
        ctx.close()
        # cornell: a triangle far from everything visits the root, tests its children's boxes and nothing else; one around everything
        # visits every node, tests every child box and every record
        ctx = _ctx(SCENES["cornell"][0](), key15, counting=True)
        bvh = ctx.export_bvh()
        root_children = int(bvh["nodes"][bvh["root"]]["meta"]) & 7
        far = ctx.overlap_triangles(through + np.array([50, 60, -70], F32), max_hits=8, with_stats=True)
        assert _stats(far[3]) == (1, root_children, 0, 0, 1) and far[1][0] == 0
        huge = np.array([((-90, -90, -90), (90, 90, -90), (0, 90, 90))], F32)
        every = ctx.overlap_triangles(huge, max_hits=8, with_stats=True)
        children = sum(int(n["meta"]) & 7 for n in bvh["nodes"])
        want = tr.k_lowest(bvh, huge, 8)
        assert _stats(every[3]) == (1, children, len(bvh["tris"]), int(want[1][0] > 0), len(bvh["nodes"]))
        _assert_equal(every, want, "every")
        assert tuple(_cull_counts(bvh, huge)[0]) == (children, len(bvh["tris"]), len(bvh["nodes"]))
        # and a mixed set: the counters are the reference cull's sums (the tree is three levels deep: no resume entry, no second fetch)
        q = tr.scene_queries(SCENES["cornell"][0](), bvh, 16, seed=29)
        got = ctx.overlap_triangles(q, max_hits=8, with_stats=True)
        _assert_equal(got, tr.k_lowest(bvh, q, 8), "mixed")
        boxes, tris, nodes = (int(v) for v in _cull_counts(bvh, q).sum(axis=0))
        assert _stats(got[3]) == (len(q), boxes, tris, int((got[1] > 0).sum()), nodes) and 0 < tris < len(q) * len(bvh["tris"])
        ctx.close()


def test_invalid_triangles_empty_and_misaligned_calls():
    sc = SCENES["cornell"][0]()
    ctx = _ctx(sc)
    huge = np.array([((-5, -0.5, -5), (5, -0.5, -5), (0, 0.5, 9))], F32)           # cuts through the whole box
    nan, inf = F32(np.nan), F32(np.inf)
    bad = np.repeat(huge, 7, axis=0)
    bad[0, 0, 0] = nan; bad[1, 1, 1] = nan; bad[2, 2, 2] = nan; bad[3, 0, 1] = inf; bad[4, 2, 0] = -inf
    bad[5, 0, 0], bad[5, 1, 0] = -3e38, 3e38                                   # f1 overflows
    bad[6, 0, 1], bad[6, 2, 1] = 3e38, -3e38                                   # f2 overflows
    assert tr.invalid_triangles(bad).all()
    valid = ctx.overlap_triangles(huge, max_hits=2)
    assert valid[1][0] == 2 and valid[2][0] > 2                                # the valid version answers
    for key15 in (1, 2):
        ctx.set_tuning(15, key15)
        for k in (1, 32):
            tris, counts, totals = ctx.overlap_triangles(bad, max_hits=k)
            assert (counts == 0).all() and (totals == 0).all() and (tris == tr.NONE).all(), (key15, k)
        ctx.set_ray_counting(True)
        assert _stats(ctx.overlap_triangles(bad, max_hits=3, with_stats=True)[3]) == (len(bad), 0, 0, 0, 0)
        ctx.set_ray_counting(False)
        # NULL hit_counts and totals: the indices alone; the pads are ignored
        rr = np.zeros(2, dtype=capi.QUERY_TRIANGLE_DTYPE)
        rr["v0"], rr["v1"], rr["v2"] = huge[0, 0], huge[0, 1], huge[0, 2]
        rr["pad0"], rr["pad1"], rr["pad2"] = 0xDEADBEEF, 0x7FC00000, 0x7F800000
        out = np.zeros((2, 3), dtype=np.uint32)
        assert ctx.lib.fyprt_overlap_triangles(ctx.h, rr.ctypes.data, None, 2, 3, out.ctypes.data, None, None, None) == 0
        assert np.array_equal(out, np.repeat(ctx.overlap_triangles(huge, max_hits=3)[0], 2, axis=0))
    # count 0: OK, nothing launched
    e = np.zeros(0, dtype=capi.QUERY_TRIANGLE_DTYPE)
    assert ctx.lib.fyprt_overlap_triangles(ctx.h, e.ctypes.data, None, 0, 4, None, None, None, None) == 0
    assert ctx.lib.fyprt_overlap_triangles_device(ctx.h, None, None, 0, 4, None, None, None) == 0
    tris, counts, totals = ctx.overlap_triangles(np.zeros((0, 3, 3)), max_hits=5)
    assert tris.shape == (0, 5) and counts.shape == (0,) and totals.shape == (0,)
    rec, off = ctx.triangles_touching(np.zeros((0, 3, 3)))
    assert len(rec) == 0 and off.tolist() == [0]
    # misaligned device pointers (device memory of the context: its image buffer, 16-byte aligned; refused before any launch)
    ctx.resize(16, 16)
    img = ctx.image_device_ptr()
    dev = ctx.lib.fyprt_overlap_triangles_device
    assert dev(ctx.h, img + 8, None, 1, 1, img + 64, img + 128, img + 192) == -1
    assert dev(ctx.h, img, img + 66, 1, 1, img + 64, img + 128, img + 192) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 65, img + 128, img + 192) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 64, img + 130, img + 192) == -1
    assert dev(ctx.h, img, None, 1, 1, img + 64, img + 128, img + 193) == -1
    assert dev(ctx.h, img, None, 1, 0, img + 64, None, None) == -1 and dev(ctx.h, img, None, 1, 33, img + 64, None, None) == -1
    ctx.close()
    # before upload
    ctx = capi.Context(0)
    with pytest.raises(capi.FyprtError):
        ctx.overlap_triangles(huge)
    ctx.close()


@pytest.mark.parametrize("key15", [1, 2])
def test_bounds_on_rounded_vertices_outside_the_planes(key15):
    """banana_standin: query triangles whose bounds begin exactly on a record's rounded vertex where that vertex lies outside a decoded
    plane above the record (boxes_ref.protruding_boxes): only a cull with slack finds the record."""
    sc = SCENES["banana_standin"][0]()
    ctx = _ctx(sc, key15)
    bvh = ctx.export_bvh()
    lo, hi, where = br.protruding_boxes(bvh)
    assert len(where) >= 5
    v0, e1, e2, _ = br.bruteforce.leaf_records(bvh)
    q = []
    for i, (_, _, r) in enumerate(where):
        # the bounds are exactly [lo, hi]: two opposite corners and the record's protruding rounded vertex, which lies on the face
        # the box begins (or ends) on; a query vertex bit-equal to a rounded vertex of the record always touches it
        vs = np.stack([v0[r], (v0[r] + e1[r]).astype(F32), (v0[r] + e2[r]).astype(F32)])
        on_face = [k for k in range(3) if ((vs[k] == lo[i]) | (vs[k] == hi[i])).any() and ((vs[k] >= lo[i]) & (vs[k] <= hi[i])).all()]
        assert on_face, i
        q.append(np.stack([lo[i], hi[i], vs[on_face[0]]]))
    q = np.array(q, F32)
    assert np.array_equal(tr.bounds(q)[0], lo) and np.array_equal(tr.bounds(q)[1], hi)
    ok_ids = tr.accepted(bvh, q)
    assert all(bool(ok_ids[0][i, r]) for i, (_, _, r) in enumerate(where))
    lost = sum(bool(tr.children_apart(bvh["nodes"][ni], lo[i:i + 1], hi[i:i + 1], slack=0.0)[0, c]) for i, (ni, c, _) in enumerate(where))
    assert lost >= 5                                                          # a cull without slack would have skipped them
    _assert_equal(ctx.overlap_triangles(q, max_hits=32), tr.k_lowest(bvh, q, 32, ok_ids=ok_ids), key15)
    ctx.close()


# ---- the query filter
def test_filter_one_mesh_masked_out(hall_small):
    sc, q, bvh, ref, ok_ids = hall_small
    n_tri = len(sc.triangles)
    mesh_of = fr.mesh_of_triangle(sc.meshes, n_tri)
    sizes = np.array([int(m[1]) for m in sc.meshes])
    out = int(np.argmax(sizes))                                               # the largest mesh leaves
    M = np.full(len(sc.meshes), 1, dtype=np.uint32)
    M[out] = 2
    admitted = mesh_of != out
    want = tr.k_lowest(bvh, q, 8, ok_ids=ok_ids, admitted=None)
    ok_f = ok_ids[0].copy()
    ok_f[:, ~admitted[ok_ids[1]]] = False
    want_f = tr.k_lowest(bvh, q, 8, ok_ids=(ok_f, ok_ids[1]))
    assert (want_f[2] < want[2]).any() and want_f[2].sum() > 0
    for key15 in (1, 2):
        ctx = _ctx(sc, key15, counting=True)
        builds0 = ctx.query_filter()[-1]
        plain = ctx.overlap_triangles(q, max_hits=8, with_stats=True)
        _assert_equal(plain, want, (key15, "no table"))
        assert ctx.query_filter()[-1] == builds0                              # no table: the unfiltered kernels, nothing built
        ctx.set_mesh_query_masks(M)
        ctx.set_query_mask(1)
        got = ctx.overlap_triangles(q, max_hits=8, with_stats=True)
        _assert_equal(got, want_f, (key15, "masked"))
        used = got[0][got[0] != tr.NONE]
        assert admitted[used].all()                                           # only admitted triangles are answered
        assert ctx.query_filter()[-1] == builds0 + 1
        assert got[3].node_visits < plain[3].node_visits and got[3].tri_tests < plain[3].tri_tests
        got_all, off = ctx.triangles_touching(q[::5], max_hits=4)
        want_all = tr.all_touching(bvh, q[::5], ok_ids=(ok_f[::5], ok_ids[1]))
        assert np.array_equal(got_all, want_all[0]) and np.array_equal(off, want_all[1])
        ctx.set_query_mask(3)                                                 # both groups: the unfiltered answer through the filtered kernels
        _assert_equal(ctx.overlap_triangles(q, max_hits=8), want, (key15, "all admitted"))
        ctx.set_mesh_query_masks(None)
        _assert_equal(ctx.overlap_triangles(q, max_hits=8), want, (key15, "off again"))
        ctx.close()


def _mesh_triangles(sc, mesh):
    first, count, _ = sc.meshes[mesh]
    t = sc.triangles[first:first + count]
    p = sc.world_vertices["position"]
    return np.stack([p[t["v0"]], p[t["v1"]], p[t["v2"]]], axis=1).astype(F32)


@pytest.mark.parametrize("key15", [1, 2])
def test_editor_sequence_append_mask_move_remove(key15):
    """The mesh in hand: appended clear of the scene, masked out and queried with its own triangles (nothing), moved into a wall by a
    transform edit and queried again (the contacts of the reference on the new export), removed (a later query equals the reference)."""
    from append_common import patch
    sc = SCENES["hall_small"][0]()
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    ctx = _ctx(sc, key15)
    ctx.set_object_vertices(sc)
    pos = sc.world_vertices["position"].astype(np.float64)
    slo, shi = pos.min(axis=0), pos.max(axis=0)
    clear = tuple(float(v) for v in (shi + (shi - slo)))                       # a scene size beyond its corner
    new = sc.add_new_mesh_to_scene(*patch(60, 0.6), pos=clear, material_index=0)
    ctx.append_meshes(sc, new)
    M = np.full(len(sc.meshes), 1, dtype=np.uint32)
    M[new] = 2
    ctx.set_mesh_query_masks(M)
    ctx.set_query_mask(1)
    own = _mesh_triangles(sc, new)
    assert len(own) == 60
    tris, counts, totals = ctx.overlap_triangles(own, max_hits=8)
    assert (totals == 0).all() and (counts == 0).all() and (tris == tr.NONE).all()
    ctx.set_query_mask(3)
    assert (ctx.overlap_triangles(own, max_hits=8)[2] > 0).all()              # unmasked, each triangle touches itself
    ctx.set_query_mask(1)
    # into a wall: onto a vertex of the scene's largest mesh, tilted so that it cuts through
    first, count, _ = sc.meshes[int(np.argmax([m[1] for m in sc.meshes[:new]]))]
    target = sc.world_vertices["position"][sc.triangles["v0"][first + count // 2]]
    mgr.set_mesh_transform(sc, new, pos=tuple(float(v) for v in target), rotation=(35, 20, 10))
    assert mgr.perform_all_scene_updates(sc) is True
    ctx.update_transforms(sc, [new])
    moved = _mesh_triangles(sc, new)
    bvh = ctx.export_bvh()
    admitted = fr.mesh_of_triangle(sc.meshes, len(sc.triangles)) != new
    want = tr.k_lowest(bvh, moved, 8, admitted=admitted)
    assert want[2].sum() > 0                                                  # there are contacts
    got = ctx.overlap_triangles(moved, max_hits=8)
    _assert_equal(got, want, (key15, "moved"))
    assert (got[0][got[0] != tr.NONE] < sc.meshes[new][0]).all()              # none of them its own
    ctx.remove_meshes(sc.remove_meshes_from_scene([new]))
    bvh = ctx.export_bvh()
    assert len(bvh["tris"]) == len(sc.triangles) and len(ctx.query_filter()[0]) == len(sc.meshes)
    _assert_equal(ctx.overlap_triangles(moved, max_hits=8), tr.k_lowest(bvh, moved, 8), (key15, "removed"))
    ctx.close()


def test_queries_leave_frames_and_other_queries_untouched(hall_small):
    sc, W, H = hall_small[0], 96, 64
    cam = SCENES["hall_small"][1](W, H)
    q = hall_small[1][:-6:2]
    lo, hi = tr.bounds(q)
    pts = ((lo + hi) * F32(0.5)).astype(F32)
    d = cam.ray_directions().reshape(-1, 3).astype(F32)[::16]
    o = np.broadcast_to(np.asarray(cam.position, F32), d.shape)
    runs = []
    for with_query in (False, True):
        ctx = _ctx(sc)
        ctx.resize(W, H)
        ctx.set_camera(cam)
        st = settings_for(capi.RESTIR_DI)
        for f in range(3):
            st.rand_seed = f + 1
            ctx.render(st)
            if with_query:
                ctx.overlap_triangles(q, max_hits=32)
        img, acc = ctx.readback()
        runs.append((ctx.frame_index, img, acc, ctx.read_buffer(capi.BUF_PAYLOAD)))
        if with_query:
            # the other four families' staging is their own: their answers before and after a triangle query are the same bytes
            def others():
                return (ctx.trace_rays(o, d).tobytes(), ctx.trace_ray_hits(o, d, max_hits=4)[0].tobytes(),
                        ctx.nearest_points(pts, max_hits=4)[0].tobytes(), ctx.overlap_boxes(lo, hi, max_hits=8)[0].tobytes())
            before = others()
            ctx.overlap_triangles(q, max_hits=7)
            assert others() == before
        ctx.close()
    (ia, imga, acca, pa), (ib, imgb, accb, pb) = runs
    assert ia == ib
    assert np.array_equal(imga, imgb) and bits_equal(acca, accb).all() and pa.tobytes() == pb.tobytes()


def test_device_memory_returns_after_close(stack):
    sc, q = stack[:2]
    q = np.tile(q, (20, 1, 1))
    base = capi.live_device_bytes()
    ctx = _ctx(sc)
    loaded = capi.live_device_bytes()
    ctx.overlap_triangles(q, max_hits=32, after=np.zeros(len(q), dtype=np.uint32))
    n = len(q)
    staged = capi.live_device_bytes() - loaded
    assert staged >= n * (48 + 4 + 32 * 4 + 4 + 4) + 64                      # triangles, after, indices, totals, counts, counters: all counted
    ctx.overlap_triangles(q[:100], max_hits=2)
    assert capi.live_device_bytes() - loaded == staged                       # the staging is kept, a smaller call allocates nothing
    ctx.close()
    assert capi.live_device_bytes() == base


def test_torch_path_equals_host_entry():
    """Run in a fresh process that initialises torch's CUDA before the library is loaded (see test_gpu_query's torch test)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_triangles as t; t._torch_path_checks(); print('torch path ok')"
            % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_path_checks():
    """Triangles produced by torch ops, indices consumed by torch ops, no synchronisation by the caller; two back-to-back device calls
    at different K (two LDS sizes), then a continuation pass from the first call's last slots."""
    import torch
    sc = SCENES["hall_small"][0]()
    ctx = _ctx(sc, key15=1)
    q = tr.scene_queries(sc, ctx.export_bvh(), 600, seed=31)
    want2, want32 = ctx.overlap_triangles(q, max_hits=2), ctx.overlap_triangles(q, max_hits=32)
    want_next = ctx.overlap_triangles(q, max_hits=3, after=want2[0][:, 1].copy())
    for _ in range(2):
        qt = torch.from_numpy(q).to("cuda:0", non_blocking=True)
        big = torch.randn(2048, 2048, device="cuda:0") @ torch.randn(2048, 2048, device="cuda:0")   # (an unordered query would read unwritten triangles)
        rec = torch.cat([qt, torch.zeros((len(q), 3, 1), device="cuda:0")], 2).reshape(len(q), 12).contiguous()
        t2, c2, n2 = ctx.overlap_triangles_tensor(rec, 2)
        t32, c32, n32 = ctx.overlap_triangles_tensor(rec, 32)
        tn, cn, nn = ctx.overlap_triangles_tensor(rec, 3, after=t2[:, 1].contiguous())
        total = (c2 + c32).sum()                                              # consumed by torch ops without a synchronisation
        for (t, c, n), (wt, wc, wn) in (((t2, c2, n2), want2), ((t32, c32, n32), want32), ((tn, cn, nn), want_next)):
            assert t.dtype == torch.int32 and c.dtype == torch.int32 and n.dtype == torch.int32 and tuple(t.shape) == wt.shape
            assert np.array_equal(t.cpu().numpy().view(np.uint32), wt)
            assert np.array_equal(c.cpu().numpy().view(np.uint32), wc) and np.array_equal(n.cpu().numpy().view(np.uint32), wn)
        assert int(total) == int(want2[1].sum()) + int(want32[1].sum())
        del rec, big, qt
    with pytest.raises(ValueError):
        ctx.overlap_triangles_tensor(torch.zeros(4, 9, device="cuda:0"), 4)
    with pytest.raises(ValueError):
        ctx.overlap_triangles_tensor(torch.zeros(4, 12, device="cuda:0"), 4, after=torch.zeros(3, dtype=torch.int32, device="cuda:0"))
    ctx.close()
