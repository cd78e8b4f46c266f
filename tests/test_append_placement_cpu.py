"""fyprt_set_append_placement / fyprt_last_append_placement on host-only contexts (capi.Context(-1)): the place the library picks against
the placement rule restated in numpy (placement_ref.place), field for field and bit for bit in the cost; the link rule on two exports
(placement_ref.check_placed_graft); mode 0 unchanged; lights as an upload; ties, the level limit, the cost against mode 0, sequences of
imports, and an append after a removal of the placed mesh."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import placement_ref as pr
from append_common import SIZES, add_emitter_material, append_patch, check_graft
from common import SCENES, check_bvh_invariants
from edit_sequences import same_exports as same_light_exports
from fypraytracer_amd import capi
from fypraytracer_amd.scene import Scene
from remove_common import check_prune, removed_triangles

W, H = 128, 80
EINVAL, ESTATE = -1, -3
# two positions per scene (shifts of append_common.append_patch).  By the numpy rule alone: cornell takes a pair at the root node for
# the first and a free slot two levels down for the second; hall_small takes pairs three levels down.
SHIFTS = {"cornell": ((0.0, 0.0, 0.0), (0.3, -0.7, 0.8)), "hall_small": ((0.0, 0.0, 0.0), (-4.0, 0.5, -3.0))}
CASES = [(name, n, k) for name in ("cornell", "hall_small") for n in (SIZES[0], SIZES[2], SIZES[3]) for k in (0, 1)]


def host(sc, mode=None):
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    if mode is not None:
        ctx.set_append_placement(mode)
    return ctx


def placed_append(ctx, sc, cam, name, n, material, shift):
    """One mode-1 append checked against the numpy rule, the link rule and the invariants.  Returns (before, after, report)."""
    before = ctx.export_bvh()
    t0 = len(sc.triangles)
    ctx.append_meshes(sc, append_patch(sc, cam, name, n, material, shift=shift))
    after = ctx.export_bvh()
    pl = ctx.last_append_placement()
    want = pr.place(before, sc.world_vertices["position"], sc.triangles, (t0, t0 + n), pr.sub_levels(before, after, n))
    assert pr.report_tuple(pl) == want, (pr.report_tuple(pl), want)
    assert pl.mode == 1 and pl.levels_before == before["max_stack"] and pl.levels_after == after["max_stack"]
    if pl.kind in (pr.SLOT, pr.PAIR):
        pr.check_placed_graft(before, after, n, pl)
    else:
        check_graft(before, after, n)
    check_bvh_invariants(after, sc, require_wide=False)
    return before, after, pl


def test_symbols_and_struct_size():
    lib = capi.load_library()
    for f in ("fyprt_set_append_placement", "fyprt_last_append_placement"):
        assert f in capi.EXPORTED_SYMBOLS and hasattr(lib, f)
    assert C.sizeof(capi.AppendPlacement) == 36


def test_errors_in_the_headers_order():
    lib = capi.load_library()
    pl = capi.AppendPlacement()
    assert lib.fyprt_set_append_placement(None, 0) == EINVAL
    assert lib.fyprt_last_append_placement(None, C.byref(pl)) == EINVAL
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = capi.Context(-1)
    for mode in (-1, 2, 7):
        assert lib.fyprt_set_append_placement(ctx.h, mode) == EINVAL
    assert lib.fyprt_last_append_placement(ctx.h, None) == EINVAL               # NULL arguments before the state
    assert lib.fyprt_last_append_placement(ctx.h, C.byref(pl)) == ESTATE
    ctx.upload_scene(sc)
    assert lib.fyprt_last_append_placement(ctx.h, C.byref(pl)) == ESTATE        # an upload is no append
    assert lib.fyprt_set_append_placement(ctx.h, 1) == 0 and lib.fyprt_set_append_placement(ctx.h, 0) == 0
    ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 1, 0))
    assert lib.fyprt_last_append_placement(ctx.h, C.byref(pl)) == 0 and pl.mode == 0
    ctx.close()


def test_mode_0_reports_and_changes_nothing():
    mk_scene, mk_cam = SCENES["cornell"]
    cam = mk_cam(W, H)
    kinds = []
    # an empty tree, then a leaf-code root, then a root with free slots
    sa, sb = Scene(), Scene()
    for s in (sa, sb):
        s.materials = mk_scene().materials
    a, b = host(sa, 0), host(sb)                                                # b never calls the setter
    for step, n in enumerate((1, 1, 4, 5, 300)):
        for ctx, s in ((a, sa), (b, sb)):
            ctx.append_meshes(s, append_patch(s, cam, "cornell", n, 0, shift=(0.3 * step - 0.45, 0.2, 0.05 * step)))
        ea, eb = a.export_bvh(), b.export_bvh()
        assert ea["nodes"].tobytes() == eb["nodes"].tobytes() and ea["tris"].tobytes() == eb["tris"].tobytes() and ea["root"] == eb["root"]
        pl = a.last_append_placement()
        assert (pl.mode, pl.cost_bits, pl.depth, pl.levels_after) == (0, 0, 0, ea["max_stack"])
        if pl.kind == pr.SLOT:
            assert pl.node == ea["root"] and int(ea["nodes"][pl.node]["meta"]) & 7 == pl.slot + 1
        kinds.append(pl.kind)
    assert kinds[:2] == [pr.FIRST, pr.ROOT_PAIR] and set(kinds) == {pr.FIRST, pr.SLOT, pr.ROOT_PAIR}, kinds
    a.close()
    b.close()
    # cornell's root is full: the same against an untouched context on a scene with a tree
    sa, sb = mk_scene(), mk_scene()
    a, b = host(sa, 0), host(sb)
    for step, n in enumerate(SIZES):
        for ctx, s in ((a, sa), (b, sb)):
            ctx.append_meshes(s, append_patch(s, cam, "cornell", n, 0, shift=(0.3 * step - 0.45, 0.2, 0.05 * step)))
        ea, eb = a.export_bvh(), b.export_bvh()
        assert ea["nodes"].tobytes() == eb["nodes"].tobytes() and ea["tris"].tobytes() == eb["tris"].tobytes() and ea["root"] == eb["root"]
    a.close()
    b.close()


@lru_cache(maxsize=None)
def _case(name, n, k):
    """One case of CASES, checked; returns (kind, the node is not the root)."""
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    ctx = host(sc, 1)
    before, after, pl = placed_append(ctx, sc, cam, name, n, light if n == 5 else 0, SHIFTS[name][k])
    ref = host(sc)
    same_light_exports(ctx, ref, len(sc.meshes))
    ref.close()
    ctx.close()
    return pl.kind, pl.kind in (pr.SLOT, pr.PAIR) and pl.node != before["root"]


@pytest.mark.parametrize("name,n,k", CASES)
def test_mode_1_equals_the_numpy_rule(name, n, k):
    _case(name, n, k)


def test_the_positions_cover_non_root_places_a_slot_and_a_pair():
    """The report equals the numpy rule in every case (_case asserts it), so this is what the rule alone picks."""
    seen = {c: _case(*c) for c in CASES}
    for name in ("cornell", "hall_small"):
        assert any(deep for (s, _, _), (_, deep) in seen.items() if s == name), name
    assert {pr.SLOT, pr.PAIR} <= {kind for kind, _ in seen.values()}


def _triangle_mesh(sc, centre, material=0):
    """One triangle whose box is symmetric about centre.x and centre.y: exact coordinates, identity transform."""
    cx, cy, cz = centre
    p = np.array([[cx - 0.5, cy - 0.5, cz], [cx + 0.5, cy - 0.5, cz], [cx, cy + 0.5, cz]], dtype=np.float32)
    nrm = np.tile(np.array([0, 0, 1], dtype=np.float32), (3, 1))
    uv = np.zeros((3, 2), dtype=np.float32)
    return sc.add_new_mesh_to_scene(p, nrm, uv, np.array([[0, 1, 2]], dtype=np.uint32), pos=(0.0, 0.0, 0.0), rotation=(0, 0, 0), material_index=material)


def test_a_cost_tie_goes_to_the_lower_id():
    """Four one-triangle meshes: two mirrored about x = 0, two further away along y.  A triangle at the origin costs the same beside
    either of the mirrored two, bit for bit."""
    sc = Scene()
    sc.materials = SCENES["cornell"][0]().materials
    for centre in ((-3.0, 0.0, 0.0), (3.0, 0.0, 0.0), (0.0, -6.0, 0.0), (0.0, 6.0, 0.0)):
        _triangle_mesh(sc, centre)
    ctx = host(sc, 1)
    before = ctx.export_bvh()
    t0 = len(sc.triangles)
    _triangle_mesh(sc, (0.0, 0.0, 0.0))
    ctx.append_meshes(sc, len(sc.meshes) - 1)
    after = ctx.export_bvh()
    pl = ctx.last_append_placement()
    cands, _ = pr.candidates(before, sc.world_vertices["position"], sc.triangles, (t0, t0 + 1), 0)
    cands.sort()
    assert cands[0][0] == cands[1][0] and cands[0][1] < cands[1][1], cands[:3]     # the tie exists in the rule itself
    assert pl.cost_bits == cands[0][0] and (pl.node * 8 + (4 if pl.kind == pr.SLOT else pl.slot)) == cands[0][1]
    assert pr.report_tuple(pl) == pr.place(before, sc.world_vertices["position"], sc.triangles, (t0, t0 + 1), 0)
    pr.check_placed_graft(before, after, 1, pl)
    check_bvh_invariants(after, sc, require_wide=False)
    ctx.close()


def test_a_31_level_chain_excludes_deep_candidates():
    """The chain of test_append_cpu.py's 120 imports, built in mode 0 up to the level limit.  Mode 0's next import at a full root
    rebuilds the tree (kind 4).  In mode 1 the rule excludes every candidate with d(X) + hX > 31 — for a five-triangle import (h = 1)
    every node whose own level count is below h + 1 at the end of a full-length path — and still finds a feasible one near the top of the
    chain (a pair with a leaf child of the root keeps the root's 31 levels), so the tree stays at 31 levels without a rebuild: with the
    rule as stated, a chain built through the API leaves no state in which mode 1 has no feasible candidate."""
    mk_scene, mk_cam = SCENES["cornell"]
    sc, cam = mk_scene(), mk_cam(W, H)
    ctx = host(sc, 0)
    k, chain = 0, ctx.export_bvh()
    while chain["max_stack"] < 31 or (int(chain["nodes"][chain["root"]]["meta"]) & 7) < 4:      # 31 levels under a full root
        ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 1, 0, shift=(0.01 * k - 0.6, -0.3, 0.0)))
        k, chain = k + 1, ctx.export_bvh()
        assert k < 120
    assert chain["max_stack"] == 31
    # mode 1 on the full chain: the numpy rule, fewer candidates than without the level limit, no rebuild
    ctx.set_append_placement(1)
    before, after, pl = placed_append(ctx, sc, cam, "cornell", 5, 0, (0.2, 0.3, 0.1))
    assert pl.kind in (pr.SLOT, pr.PAIR, pr.ROOT_PAIR) and after["max_stack"] == 31
    structural = sum(int(m) & 7 for m in before["nodes"]["meta"]) + sum((int(m) & 7) < 4 for m in before["nodes"]["meta"]) + 1
    assert pl.candidates < structural
    ctx.close()
    # mode 0 on the same chain: the fall-back, reported as kind 4
    sc0, cam = mk_scene(), mk_cam(W, H)
    c0 = host(sc0, 0)
    for j in range(k):
        c0.append_meshes(sc0, append_patch(sc0, cam, "cornell", 1, 0, shift=(0.01 * j - 0.6, -0.3, 0.0)))
    assert c0.export_bvh()["nodes"].tobytes() == chain["nodes"].tobytes()
    c0.append_meshes(sc0, append_patch(sc0, cam, "cornell", 5, 0, shift=(0.2, 0.3, 0.1)))
    p0 = c0.last_append_placement()
    assert (p0.mode, p0.kind, p0.node, p0.slot, p0.depth, p0.cost_bits) == (0, pr.REBUILT, 0, 0, 0, 0)
    assert p0.levels_before == 31 and p0.levels_after == c0.export_bvh()["max_stack"] < 31
    c0.close()


@pytest.mark.parametrize("name,n,k", [("cornell", 1, 1), ("cornell", 300, 0), ("hall_small", 5, 1), ("hall_small", 300, 0)])
def test_cost_is_not_above_mode_0s(name, n, k):
    """Sum of A(b(Y)) over all inner nodes (float64, exact boxes) after the same append in both modes.  The slack covers at most 33
    terms (the path, N, the root pair), each off by a few ulp of an area no larger than A(U(b(R), B))."""
    mk_scene, mk_cam = SCENES[name]
    sums, deep = [], False
    for mode in (0, 1):
        sc, cam = mk_scene(), mk_cam(W, H)
        ctx = host(sc, mode)
        before = ctx.export_bvh()
        t0 = len(sc.triangles)
        ctx.append_meshes(sc, append_patch(sc, cam, name, n, 0, shift=SHIFTS[name][k]))
        after = ctx.export_bvh()
        pl = ctx.last_append_placement()
        pos = sc.world_vertices["position"]
        sums.append(pr.inner_area_sum(after, pos, sc.triangles))
        if mode == 1:
            deep = pl.kind in (pr.SLOT, pr.PAIR) and pl.node != before["root"]
            lo, hi, _, _ = pr.exact_boxes(before, pos, sc.triangles)
            corners = pr.triangle_corners(pos, sc.triangles, np.arange(t0, t0 + n)).reshape(-1, 3)
            R = before["root"]
            bound = float(pr.union_area(lo[R], hi[R], corners.min(axis=0), corners.max(axis=0)))
        ctx.close()
    print(name, n, k, "sum mode 0", sums[0], "sum mode 1", sums[1], "slack", 256 * 2.0 ** -23 * bound)
    assert sums[1] <= sums[0] + 256 * 2.0 ** -23 * bound
    if (name, n, k) in (("cornell", 1, 1), ("hall_small", 5, 1)):             # the cases the numpy rule places below the root
        assert deep and sums[1] < sums[0]


def test_a_sequence_of_imports_stays_shallower_than_mode_0():
    """24 one-triangle imports at scattered shifts into cornell: mode 0 adds a level about every third import."""
    mk_scene, mk_cam = SCENES["cornell"]
    rng = np.random.default_rng(7)
    shifts = rng.uniform(-0.8, 0.8, size=(24, 3))
    levels = []
    for mode in (0, 1):
        sc, cam = mk_scene(), mk_cam(W, H)
        ctx = host(sc, mode)
        got = []
        for s in shifts:
            ctx.append_meshes(sc, append_patch(sc, cam, "cornell", 1, 0, shift=tuple(float(v) for v in s)))
            got.append(ctx.export_bvh()["max_stack"])
            assert ctx.last_append_placement().levels_after == got[-1]
        check_bvh_invariants(ctx.export_bvh(), sc, require_wide=False)
        levels.append(got)
        ctx.close()
    print("levels mode 0", levels[0], "mode 1", levels[1])
    assert all(b <= a for a, b in zip(*levels))
    assert levels[1][-1] < levels[0][-1]


@pytest.mark.parametrize("name,k", [("cornell", 1), ("hall_small", 1)])
def test_append_remove_append(name, k):
    mk_scene, mk_cam = SCENES[name]
    sc, cam = mk_scene(), mk_cam(W, H)
    light = add_emitter_material(sc)
    ctx = host(sc, 1)
    _, _, pl = placed_append(ctx, sc, cam, name, 5, light, SHIFTS[name][k])
    assert pl.kind in (pr.SLOT, pr.PAIR)
    m = len(sc.meshes) - 1
    before = ctx.export_bvh()
    dead = removed_triangles(sc, [m])
    ctx.remove_meshes(sc.remove_meshes_from_scene([m]))
    after = ctx.export_bvh()
    check_prune(before, after, dead)
    check_bvh_invariants(after, sc, require_wide=False)
    placed_append(ctx, sc, cam, name, 300, light, SHIFTS[name][k])
    ref = host(sc)
    same_light_exports(ctx, ref, len(sc.meshes))
    ref.close()
    ctx.close()
