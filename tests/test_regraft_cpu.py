"""fyprt_regraft_meshes / fyprt_tree_cost on host-only contexts (capi.Context(-1)): symbols and errors; the cost against its restatement
in numpy on the export (regraft_common.tree_cost_ref); the regrafted tree against the twin that removes the meshes in one call and
appends them again (regraft_common.regraft_against_twin), in both placement modes; lights, reports of earlier calls and later edits
untouched; and a mode-1 regraft of a mesh that mode 0 put at the root does not raise the surface-area cost."""
import ctypes as C

import numpy as np
import pytest

import placement_ref as pr
import regraft_common as rc
from append_common import add_emitter_material, append_patch
from common import SCENES, check_bvh_invariants, struct_equal
from fypraytracer_amd import capi
from fypraytracer_amd.scene import Scene
from remove_common import check_prune, removed_triangles
from test_append_placement_cpu import SHIFTS

W, H = 128, 80
EINVAL, ESTATE = -1, -3


def host(sc, mode=0):
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    ctx.set_append_placement(mode)
    return ctx


def maker(name, mode, patches=()):
    """make() of regraft_against_twin: the scene uploaded, then one append per entry of `patches` (n triangles, shift)."""
    def make():
        mk_scene, mk_cam = SCENES[name]
        sc, cam = mk_scene(), mk_cam(W, H)
        ctx = host(sc, mode)
        for n, shift in patches:
            ctx.append_meshes(sc, append_patch(sc, cam, name, n, 0, shift=shift))
        return ctx, sc
    return make


def _raw(ctx, meshes, count=None, reports=True):
    idx = None if meshes is None else (C.c_uint32 * max(1, len(meshes)))(*meshes)
    n = len(meshes) if count is None else count
    out = (capi.AppendPlacement * max(1, n))() if reports else None
    return ctx.lib.fyprt_regraft_meshes(ctx.h, idx, n, out)


def _exports(ctx, n_meshes):
    return ctx.export_bvh(), ctx.export_lighttrees(n_meshes), ctx.export_emissive()


def _same_exports(e0, e1):
    assert rc.same_export(e0[0], e1[0])
    for k in ("tlas", "blas", "blas_first", "blas_count", "blas_root"):
        assert e0[1][k].tobytes() == e1[1][k].tobytes(), k
    assert e0[1]["tlas_root"] == e1[1]["tlas_root"] and np.array_equal(e0[2], e1[2])


# ---- symbols and errors
def test_symbols_and_struct_sizes():
    lib = capi.load_library()
    for f in ("fyprt_regraft_meshes", "fyprt_tree_cost"):
        assert f in capi.EXPORTED_SYMBOLS and hasattr(lib, f)
    assert C.sizeof(capi.TreeCost) == 40 and C.sizeof(capi.AppendPlacement) == 36
    assert capi.TreeCost.leaf_area.offset == 16 and capi.TreeCost.nodes.offset == 24 and capi.TreeCost.levels.offset == 36


def test_errors_in_the_headers_order_and_a_failed_call_changes_nothing():
    lib = capi.load_library()
    cost = capi.TreeCost()
    sc = SCENES["cornell"][0]()
    ctx = capi.Context(-1)
    assert lib.fyprt_regraft_meshes(None, None, 0, None) == EINVAL              # a NULL context
    assert lib.fyprt_tree_cost(None, C.byref(cost)) == EINVAL
    assert lib.fyprt_tree_cost(ctx.h, None) == EINVAL                           # NULL arguments before the state
    assert lib.fyprt_tree_cost(ctx.h, C.byref(cost)) == ESTATE
    assert _raw(ctx, None, count=2) == EINVAL                                   # bad arguments before the state
    assert _raw(ctx, [0]) == EINVAL
    assert _raw(ctx, []) == ESTATE                                              # before the upload only the empty call has valid arguments
    ctx.upload_scene(sc)
    e0 = _exports(ctx, len(sc.meshes))
    assert _raw(ctx, None, count=2) == EINVAL                                   # NULL mesh_indices with a non-zero count
    assert _raw(ctx, [8]) == EINVAL                                             # a mesh index out of range
    assert _raw(ctx, [8, 8]) == EINVAL                                          # ... comes before "listed twice"
    assert _raw(ctx, [3, 5, 3]) == EINVAL                                       # a mesh listed twice
    assert _raw(ctx, []) == 0 and _raw(ctx, [], reports=False) == 0             # mesh_count == 0
    assert ctx.regraft_meshes([]) == []
    _same_exports(e0, _exports(ctx, len(sc.meshes)))
    assert _raw(ctx, [5], reports=False) == 0                                   # NULL reports are allowed
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    ctx.close()
    # a scene uploaded with prebuilt light trees may be regrafted: the light trees are not touched
    pre = capi.Context(-1)
    pre.upload_scene(sc)
    lt = pre.export_lighttrees(len(sc.meshes))
    pre.upload_scene(sc, light_trees=lt)
    e0 = _exports(pre, len(sc.meshes))
    pre.regraft_meshes([5, 7])
    e1 = _exports(pre, len(sc.meshes))
    for k in ("tlas", "blas", "blas_first", "blas_count", "blas_root"):
        assert e0[1][k].tobytes() == e1[1][k].tobytes(), k
    check_bvh_invariants(e1[0], sc, require_wide=False)
    pre.close()


# ---- tree_cost against numpy on the export
@pytest.mark.parametrize("name", ["cornell", "hall_small"])
def test_tree_cost_equals_numpy_on_the_export(name):
    sc = SCENES[name][0]()
    ctx = host(sc)
    got, want = rc.cost_tuple(ctx.tree_cost()), rc.tree_cost_ref(ctx.export_bvh(), sc)
    print(name, "library", got, "numpy", want)
    rc.assert_cost_close(got, want)
    assert got[3] > 0 and got[5] == len(sc.triangles) and got[0] > 0 and got[2] > 0
    assert rc.cost_tuple(ctx.tree_cost()) == got                                # the same bits twice
    ctx.close()


def test_tree_cost_of_an_empty_scene_and_of_a_leaf_code_root():
    mk_scene, mk_cam = SCENES["cornell"]
    cam = mk_cam(W, H)
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.25], [0, 1, 0]], dtype=np.float32)
    for n in (1, 2):                                                            # a scene of one mesh: one leaf code of 1 / of 2 triangles
        sc = Scene()
        sc.materials = mk_scene().materials
        ctx = host(sc)
        assert rc.cost_tuple(ctx.tree_cost()) == (0.0, 0.0, 0.0, 0, 0, 0, 0)
        if n == 1:
            m = append_patch(sc, cam, "cornell", 1, 0)
        else:
            m = sc.add_new_mesh_to_scene(quad, np.tile(np.array([0, 0, 1], dtype=np.float32), (4, 1)), np.zeros((4, 2), dtype=np.float32),
                                         np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32))
        ctx.append_meshes(sc, m)
        e = ctx.export_bvh()
        assert e["root"] < 0 and len(e["nodes"]) == 0
        got, want = rc.cost_tuple(ctx.tree_cost()), rc.tree_cost_ref(e, sc)
        rc.assert_cost_close(got, want)
        assert got[3:] == (0, 1, n, 0) and got[0] > 0 and got[1] == 0.0 and got[2] == n * got[0]
        fresh = host(sc)                                                        # ... and the same from an upload of that scene
        assert rc.cost_tuple(fresh.tree_cost()) == got
        fresh.close()
        ctx.close()


# ---- regraft equals the twin
# (scene, appended patches (n, shift), the meshes regrafted; negative = counted from the last mesh), and a branch of the prune rule the
# twin's removal must meet.  cornell: mesh 1 is a wall of two triangles whose leaf shares a node with one other child (a splice); mesh 5
# the tall box.  hall_small: 15 a column, 25 a light mesh, 21 a drape of 1800 triangles.
TWINS = [
    ("cornell", (), (1,), "splice onto a leaf code"),                                           # <= 4 triangles: S is a leaf code
    ("cornell", ((5, SHIFTS["cornell"][1]),), (-1,), None),                                     # 5 triangles
    ("cornell", ((300, SHIFTS["cornell"][0]),), (-1,), None),                                   # a few hundred
    ("hall_small", ((5, SHIFTS["hall_small"][1]),), (-1,), None),
    ("hall_small", (), (15, 25), None),                                                         # two meshes in one call ...
    ("hall_small", (), (25, 15), None),                                                         # ... in both orders
    ("hall_small", (), (21,), "node dropped"),
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,patches,meshes,branch", TWINS)
def test_regraft_equals_the_twin(name, patches, meshes, branch, mode):
    n_meshes = len(SCENES[name][0]().meshes) + len(patches)
    meshes = [m % n_meshes for m in meshes]
    ctx, sc, reports, met = rc.regraft_against_twin(maker(name, mode, patches), meshes)
    assert all(r.mode == mode and r.kind in (pr.SLOT, pr.PAIR, pr.ROOT_PAIR) for r in reports)
    assert branch is None or branch in met, met
    rc.assert_cost_close(rc.cost_tuple(ctx.tree_cost()), rc.tree_cost_ref(ctx.export_bvh(), sc))
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_a_regraft_that_collapses_a_chain_of_splices(mode):
    """test_remove_cpu.py's chain: three mode-0 grafts onto cornell's full root (a new root that takes two more children), a fourth
    (another new root).  Regrafting all four in one call takes both roots away again — a chain of two splices — before they come back."""
    def make():
        mk_scene, mk_cam = SCENES["cornell"]
        sc, cam = mk_scene(), mk_cam(W, H)
        ctx = host(sc, 0)
        for k, n in enumerate((5, 1, 4, 5)):
            ctx.append_meshes(sc, append_patch(sc, cam, "cornell", n, 0, shift=(0.2 * k - 0.4, 0.1, 0.0)))
        ctx.set_append_placement(mode)
        return ctx, sc
    ctx, sc, reports, met = rc.regraft_against_twin(make, [8, 9, 10, 11])
    assert {"chain of splices", "root replaced"} <= met, met
    plain = host(SCENES["cornell"][0]())
    assert reports[0].levels_before == plain.export_bvh()["max_stack"]          # cornell's own tree again before the first graft
    plain.close()
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_the_only_mesh_of_a_scene(mode):
    """The prune leaves an empty tree, so the graft's kind is "first" in either mode and the tree is what it was."""
    def make():
        mk_scene, mk_cam = SCENES["cornell"]
        sc = Scene()
        sc.materials = mk_scene().materials
        ctx = host(sc, mode)
        ctx.append_meshes(sc, append_patch(sc, mk_cam(W, H), "cornell", 300, 0))
        return ctx, sc
    ref, _ = make()
    ctx, sc, reports, met = rc.regraft_against_twin(make, [0])
    assert rc.placement_tuple(reports[0])[1:7] == (pr.FIRST, 0, 0, 0, 0, 0)
    assert rc.same_export(ctx.export_bvh(), ref.export_bvh())
    ref.close()
    ctx.close()


def test_a_graft_without_a_place_rebuilds_the_tree():
    """The 31-level chain of test_append_placement_cpu.py, built in mode 0 under a full root.  The first two imports sit at the bottom of
    the chain beside a third, so pruning them leaves the 31 levels and the full root, and mode 0's graft would need a 32nd level:
    the tree is rebuilt as an upload builds it, and this and the remaining report say kind 4."""
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = host(sc, 0)
    k, chain = 0, ctx.export_bvh()
    while chain["max_stack"] < 31 or (int(chain["nodes"][chain["root"]]["meta"]) & 7) < 4:
        ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 1, 0, shift=(0.01 * k - 0.6, -0.3, 0.0)))
        k, chain = k + 1, ctx.export_bvh()
        assert k < 120
    placed = rc.placement_tuple(ctx.last_append_placement())
    reports = ctx.regraft_meshes([8, 9])
    assert rc.placement_tuple(reports[0])[:7] == (0, pr.REBUILT, 0, 0, 0, 0, 31)
    fresh = host(sc)
    e = ctx.export_bvh()
    assert rc.same_export(e, fresh.export_bvh()) and e["max_stack"] < 31
    assert rc.placement_tuple(reports[1]) == (0, pr.REBUILT, 0, 0, 0, 0, e["max_stack"], e["max_stack"], 0) and reports[0].levels_after == e["max_stack"]
    assert rc.placement_tuple(ctx.last_append_placement()) == placed
    fresh.close()
    ctx.close()


def test_a_mesh_without_triangles_is_skipped():
    mk_scene, mk_cam = SCENES["cornell"]
    sc = mk_scene()
    empty = sc.add_new_mesh_to_scene(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 3), dtype=np.uint32))
    ctx = host(sc, 1)
    e0 = ctx.export_bvh()
    reports = ctx.regraft_meshes([empty])
    assert rc.placement_tuple(reports[0]) == (1, 0, 0, 0, 0, 0, 0, 0, 0) and rc.same_export(e0, ctx.export_bvh())
    reports = ctx.regraft_meshes([empty, 5])
    assert rc.placement_tuple(reports[0]) == (1, 0, 0, 0, 0, 0, 0, 0, 0) and reports[1].kind in (pr.SLOT, pr.PAIR, pr.ROOT_PAIR)
    check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
    ctx.close()


# ---- everything else is untouched
@pytest.mark.parametrize("name,meshes", [("cornell", (7, 5)), ("hall_small", (25, 15))])        # a light mesh and a plain one
def test_nothing_but_the_tree_moves(name, meshes):
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    ctx = host(sc, 1)
    ctx.append_meshes(sc, append_patch(sc, cam, name, 5, light, shift=SHIFTS[name][1]))
    placed = rc.placement_tuple(ctx.last_append_placement())
    st = capi.EditStats()
    assert ctx.lib.fyprt_last_edit_stats(ctx.h, C.byref(st)) == ESTATE
    e0 = _exports(ctx, len(sc.meshes))
    ctx.regraft_meshes(list(meshes) + [len(sc.meshes) - 1])
    e1 = _exports(ctx, len(sc.meshes))
    for k in ("tlas", "blas"):
        assert struct_equal(e0[1][k], e1[1][k]).all(), k
    for k in ("blas_first", "blas_count", "blas_root"):
        assert np.array_equal(e0[1][k], e1[1][k]), k
    assert e0[1]["tlas_root"] == e1[1]["tlas_root"] and np.array_equal(e0[2], e1[2])
    assert rc.placement_tuple(ctx.last_append_placement()) == placed
    assert ctx.lib.fyprt_last_edit_stats(ctx.h, C.byref(st)) == ESTATE
    check_bvh_invariants(e1[0], sc, require_wide=False)
    # afterwards an append and a removal behave as on an upload of the same scene: the rules and the invariants, and the lights of a
    # context that uploads the result
    before, t0 = e1[0], len(sc.triangles)
    ctx.append_meshes(sc, append_patch(sc, cam, name, 300, light, shift=SHIFTS[name][0]))
    after = ctx.export_bvh()
    pl = ctx.last_append_placement()
    want = pr.place(before, sc.world_vertices["position"], sc.triangles, (t0, t0 + 300), pr.sub_levels(before, after, 300))
    assert pr.report_tuple(pl) == want
    check_bvh_invariants(after, sc, require_wide=False)
    dead = removed_triangles(sc, meshes)
    ctx.remove_meshes(sc.remove_meshes_from_scene(meshes))
    pruned = ctx.export_bvh()
    check_prune(after, pruned, dead)
    check_bvh_invariants(pruned, sc, require_wide=False)
    ref = host(sc)
    _same_exports((pruned,) + _exports(ref, len(sc.meshes))[1:], (pruned,) + _exports(ctx, len(sc.meshes))[1:])
    ref.close()
    ctx.close()


# ---- regraft lowers the cost
# inner_area after a mode-1 regraft of a mesh that mode 0 grafted, against inner_area before.  The prune takes the mode-0 graft away
# again, so both trees are the same old tree plus one graft of the same sub-tree, and the place mode 0 took (the root's free slot or the
# root pair) is among the candidates the search offers.  A candidate's cost is the exact change of inner_area apart from its binary32
# roundings: on a path of at most 31 nodes at most 31 differences g(Y), one union area and 31 additions, 63 roundings, each of at most
# 2^-24 relative of a term or partial sum that is at most 32 * A(U(b(R), B)).  So each computed cost is within 63 * 32 * 2^-24 * A(U(b(R),
# B)) of the exact one, and the winner's exact cost exceeds mode 0's by at most twice that: 4032 * 2^-24 < 2^-12 times A(U(b(R), B)).  The
# two binary64 sums of fyprt_tree_cost add 2^-26 relative of themselves (regraft_common.COST_RTOL).
INNER_SLACK = 2.0 ** -12


def test_a_mode_1_regraft_does_not_raise_the_inner_area():
    name = "hall_small"
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = host(sc, 0)
    base = ctx.export_bvh()
    t0 = len(sc.triangles)
    m = append_patch(sc, cam, name, 5, 0, shift=SHIFTS[name][1])                # the shift the numpy rule places below the root
    ctx.append_meshes(sc, m)
    assert ctx.last_append_placement().kind in (pr.SLOT, pr.ROOT_PAIR)
    at_root = ctx.tree_cost()
    ctx.set_append_placement(1)
    report, = ctx.regraft_meshes([m])
    placed = ctx.tree_cost()
    pos = sc.world_vertices["position"]
    lo, hi, _, _ = pr.exact_boxes(base, pos, sc.triangles)
    corners = pr.triangle_corners(pos, sc.triangles, np.arange(t0, t0 + 5)).reshape(-1, 3)
    bound = float(pr.union_area(lo[base["root"]], hi[base["root"]], corners.min(axis=0), corners.max(axis=0)))
    slack = INNER_SLACK * bound + rc.COST_RTOL * (at_root.inner_area + placed.inner_area)
    print("inner area at the root", at_root.inner_area, "regrafted", placed.inner_area, "slack", slack, "report", rc.placement_tuple(report))
    assert placed.inner_area <= at_root.inner_area + slack
    assert report.kind in (pr.SLOT, pr.PAIR) and report.node != base["root"]    # below the root, where the rule places it ...
    assert placed.inner_area < at_root.inner_area                               # ... and there the cost really falls
    assert abs(placed.leaf_area - at_root.leaf_area) <= rc.COST_RTOL * at_root.leaf_area and placed.leaf_children == at_root.leaf_children
    ctx.close()
