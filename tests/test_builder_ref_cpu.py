"""builder_ref.py — the numpy restatement of the device builders and of the refit rule — held against facts that do not come from
it, and the inputs of test_gpu_builder_ref.py held to the mechanisms they are there for.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import builder_cases as bc
import builder_ref as br
from builder_ref import LEAF
from common import SCENES
from fypraytracer_amd import capi

F = np.float32


# ------------------------------------------------------------------------------------------------ Morton keys
def test_morton_keys_are_the_bitwise_interleave_of_the_cells():
    rng = np.random.default_rng(1)
    p = rng.uniform(-3.0, 5.0, size=(500, 3, 3)).astype(F)
    p[:50, :, 1] = p[0, 0, 1]                                   # some triangles flat in y (the grid is not)
    lo, hi = br.grid_of(p)
    cells, keys = br.morton_cells(p, lo, hi), br.morton_keys(p, lo, hi)
    assert cells.max() <= 2097151 and len(np.unique(cells[:, 0])) > 400
    for c, k in zip(cells.tolist(), keys.tolist()):
        want = 0
        for bit in range(21):
            want |= ((c[0] >> bit) & 1) << (3 * bit + 2) | ((c[1] >> bit) & 1) << (3 * bit + 1) | ((c[2] >> bit) & 1) << (3 * bit)
        assert k == want and k < 1 << 63


def test_morton_cells_at_known_places():
    """The grid's corners and centre, a point outside (clamped) and an axis without extent (cell 0)."""
    tri = lambda c: np.tile(np.asarray(c, dtype=F), (3, 1))
    p = np.stack([tri((0, 0, 7)), tri((8, 4, 7)), tri((4, 2, 7)), tri((16, -4, 7)), tri((1, 3, 7))])
    cells = br.morton_cells(p, F([0, 0, 7]), F([8, 4, 7]))
    assert cells.tolist() == [[0, 0, 0], [2097151, 2097151, 0], [1 << 20, 1 << 20, 0], [2097151, 0, 0], [1 << 18, 3 << 19, 0]]


# ------------------------------------------------------------------------------------------------ radix tree
def split_by_definition(keys):
    """The binary radix tree by its definition: a range splits at the highest bit in which its first and last key differ, the sorted
    position being the tiebreak below bit 0 (32 more bits)."""
    ext = [(int(k) << 32) | i for i, k in enumerate(keys)]

    def build(a, b):
        if a == b:
            return a
        bit = (ext[a] ^ ext[b]).bit_length() - 1
        m = next(i for i in range(a, b + 1) if (ext[i] >> bit) & 1)
        return (build(a, m - 1), build(m, b))

    return build(0, len(ext) - 1)


@pytest.mark.parametrize("kind", ["random", "runs", "all_equal", "narrow"])
@pytest.mark.parametrize("n", [2, 3, 5, 64, 257, 300])
def test_radix_tree_is_the_top_down_split(kind, n):
    rng = np.random.default_rng(n)
    if kind == "random":
        keys = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    elif kind == "runs":
        keys = np.repeat(rng.integers(0, 1 << 63, size=max(1, n // 7), dtype=np.uint64), 9)[:n]
        keys = np.resize(keys, n)
    elif kind == "all_equal":
        keys = np.full(n, 0x1234567, dtype=np.uint64)
    else:
        keys = rng.integers(0, 8, size=n, dtype=np.uint64)       # long runs and differences in the lowest bits only
    keys = np.sort(keys)
    t = br.radix_tree(keys)
    assert t.nested() == split_by_definition(keys)
    assert t.span[0] == n and all(t.last[i] - t.first[i] + 1 == t.span[i] and i in (t.first[i], t.last[i]) for i in range(n - 1))


# ------------------------------------------------------------------------------------------------ PLOC by hand
def x_boxes(intervals):
    """Boxes [x0, x1] x [0, 1] x [0, 1]: the cost of a union is 2 * dx + 1, so the nearest neighbour is the one with the smallest span."""
    return np.array([[a, 0, 0, b, 1, 1] for a, b in intervals], dtype=F)


def test_ploc_four_boxes():
    # A B close, C D close: both pairs are mutual in round 1, the two results merge in round 2
    t, _, rounds, forced, _ = br.ploc_tree(x_boxes([(0, 1), (1.5, 2.5), (4, 5), (5.25, 6.25)]))
    assert t.nested() == ((0, 1), (2, 3)) and rounds == 2 and forced == []


def test_ploc_five_boxes():
    # round 1: A-B and C-D (C prefers D at span 2.125 over B at 2.25); E wants D, which does not want E.  round 2: AB-CD; E waits.  round 3: the rest
    t, box, rounds, _, st = br.ploc_tree(x_boxes([(0, 1), (1.125, 2.125), (2.375, 3.375), (3.5, 4.5), (10, 11)]))
    assert t.nested() == (((0, 1), (2, 3)), 4) and rounds == 3
    assert box[t.root].tolist() == [0, 0, 0, 11, 1, 1] and st == {"cross_block": 0, "tie_to_partner": 0, "tie_to_lowest": 0}


def test_ploc_equal_boxes_pair_up_with_their_partners():
    """All costs equal: everybody takes i ^ 1 and the list halves; a search that began at the window's start would send 2 and 3 to
    0 and leave one pair per round."""
    t, _, rounds, _, st = br.ploc_tree(x_boxes([(0, 1)] * 4))
    assert t.nested() == ((0, 1), (2, 3)) and rounds == 2
    assert st["tie_to_partner"] == 2 and st["tie_to_lowest"] == 0       # clusters 2 and 3 had an equal choice below their partner
    t, _, rounds, _, _ = br.ploc_tree(x_boxes([(0, 1)] * 7))             # the unpaired last one's partner is i - 1, which has its own
    assert t.nested() == (((0, 1), (2, 3)), ((4, 5), 6)) and rounds == 3


def test_ploc_tie_goes_to_the_lowest_position_when_the_partner_is_worse():
    # 0, 2, 3 are one and the same box, 1 is far away.  round 1: 0 -> 2 (2 and 3 tie, the lower wins), 1 -> 0 (all equal: partner),
    # 2 -> 3 and 3 -> 2 (partners, although 0 ties below them): the pair is (2, 3).  round 2 over [0, 1, (23)]: 0 -> (23), (23) -> 0
    # (its partner, 2 ^ 1 = 3, is outside the list: 1 takes its place, at a higher cost).  round 3: the rest.
    near, st = br.ploc_nearest(x_boxes([(0, 1), (9, 10), (0, 1), (0, 1)]), 16)
    assert near.tolist() == [2, 0, 3, 2] and st == {"cross_block": 0, "tie_to_partner": 2, "tie_to_lowest": 1}
    t, _, rounds, _, _ = br.ploc_tree(x_boxes([(0, 1), (9, 10), (0, 1), (0, 1)]))
    assert t.nested() == ((0, (2, 3)), 1) and rounds == 3


def test_ploc_search_radius_and_block_borders():
    # the only close neighbour of cluster 0 is 3 positions away: radius 2 does not see it
    boxes = x_boxes([(0, 1), (50, 51), (100, 101), (1, 2)])
    assert br.ploc_nearest(boxes, 2)[0][0] == 1 and br.ploc_nearest(boxes, 3)[0][0] == 3
    # 300 boxes in a row, each next to the one before: 255 and 256 choose each other across the border of the first 256-block
    row = [(2 * i, 2 * i + 1) for i in range(300)]
    row[255], row[256] = (510, 511), (511.25, 512.25)
    near, st = br.ploc_nearest(x_boxes(row), 16)
    assert near[255] == 256 and near[256] == 255 and st["cross_block"] >= 2


def test_ploc_force_rule():
    """More than 4096 clusters and a round that kept more than n - n / 16: the next round pairs (2k, 2k + 1), the one after is free again."""
    n = bc.FORCED_N
    r = bc.reference("line", n, 2)
    assert r["forced"] == [1]
    free = bc.reference("line", n, 2, 16, False)
    assert free["forced"] == [] and free["rounds"] > r["rounds"] and free["tree"] != r["tree"]
    small = br.build_ref(bc.triangles("line", n)[:4096], bc.triangles("line", n)[:4096], 2)     # 4096 is not "more than 4096"
    assert small["forced"] == []


# ------------------------------------------------------------------------------------------------ collapse by hand
def hand_tree(shape, areas):
    """A BinaryTree from nested pairs of leaf numbers; `areas`: per internal node in the order of first appearance (parents first,
    left before right), realised as boxes a x 1 x 0, whose area is a."""
    t = br.BinaryTree(0)
    boxes = []

    def add(s):
        if not isinstance(s, tuple):
            t.n_leaves += 1
            return LEAF | s
        k = len(t.left)
        t.left.append(None); t.right.append(None); t.span.append(0); boxes.append([0, 0, 0, areas[k], 1, 0])
        l = add(s[0]); r = add(s[1])
        t.left[k], t.right[k], t.span[k] = l, r, t.span_of(l) + t.span_of(r)
        return k

    t.root = add(shape)
    return t, np.array(boxes, dtype=F)


def test_collapse_opens_the_largest_inner_child_then_splits_the_largest_leaf():
    #   root(14) = X(10) Y(4);  X = X1(5) X2(5);  X1 = (0 1)(2 (3 4));  X2 = (5 6)((7 8) 9);  Y = (10 11)(12 13)
    shape = ((((0, 1), (2, (3, 4))), ((5, 6), ((7, 8), 9))), ((10, 11), (12, 13)))
    #        root X   X1  X1a X1b X1bb X2  X2a X2b X2ba Y   Ya  Yb
    areas = [99, 50, 10, 3, 4, 1, 20, 2, 5, 1, 30, 1, 1]
    t, box = hand_tree(shape, areas)
    c = br.collapse(t, box)
    # root: [X Y] -> loop 1 opens X, the only child above 4 triangles -> [X1 X2 Y] -> opens X2 (20 > 10) -> [X1 X2a X2b Y]: full.
    # X1 (5 triangles) is the one inner child; X2a, X2b, Y become leaves of 2, 3 and 4 records.
    # X1: [X1a X1b], nothing above 4 -> loop 2 splits X1b (4 > 3) -> [X1a 2 X1bb] -> splits X1a (3 > 1) -> [0 1 2 X1bb]
    assert c["tree"] == ((("leaf", 0, 1), ("leaf", 1, 1), ("leaf", 2, 1), ("leaf", 3, 2)), ("leaf", 5, 2), ("leaf", 7, 3), ("leaf", 10, 4))
    assert c["leaf_positions"].tolist() == list(range(14)) and c["level_counts"] == [1, 1] and not c["too_deep"]
    assert c["stats"] == {"loop1": 2, "loop2": 2, "tie1": 0, "tie2": 0}
    assert br.levels_by_path(c["tree"]) == {(): 2, (0,): 1}


def test_collapse_keeps_the_first_of_equal_areas_and_lays_leaves_left_first():
    # the same tree with leaves numbered against the order and with ties: X1 and X2 both 10 -> X1, the first, is opened;
    # below X2 = (5 6)((7 8) 9): X2a and X2b both 5 -> X2a, the first, is split, then X2b
    shape = ((((13, 1), (2, (3, 4))), ((5, 6), ((7, 8), 9))), ((10, 11), (12, 0)))
    areas = [99, 50, 10, 3, 4, 1, 10, 5, 5, 1, 30, 1, 1]
    t, box = hand_tree(shape, areas)
    c = br.collapse(t, box)
    assert c["tree"] == (("leaf", 0, 2), ("leaf", 2, 3), (("leaf", 5, 1), ("leaf", 6, 1), ("leaf", 7, 2), ("leaf", 9, 1)), ("leaf", 10, 4))
    assert c["leaf_positions"].tolist() == [13, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0]
    assert c["stats"] == {"loop1": 2, "loop2": 2, "tie1": 1, "tie2": 1}
    # round trip through the export form
    assert br.canonical(br.export_from_canonical(c["tree"], c["leaf_positions"])) == c["tree"]
    assert br.first_tree_difference(c["tree"], c["tree"]) is None
    other = br.collapse(*hand_tree(shape, [99, 50, 10, 3, 4, 1, 20, 5, 5, 1, 30, 1, 1]))["tree"]
    assert br.first_tree_difference(c["tree"], other)[0] == (0,)


def test_collapse_reports_more_than_31_levels():
    for builder, deep in ((1, False), (2, True)):
        r = bc.reference(*bc.TOO_DEEP, builder)
        assert r["too_deep"] == deep and (len(r["level_counts"]) > br.STACK_BUDGET) == deep
    chain = 0
    for k in range(1, 200):                                     # a chain that sheds two pairs and a triangle per step: one wide level each
        chain = ((5 * k, 5 * k + 1), ((5 * k + 2, 5 * k + 3), (5 * k + 4, chain)))
    t, box = hand_tree(chain, [1.0] * 1000)
    assert len(br.collapse(t, box[:len(t.left)])["level_counts"]) == 199


# ------------------------------------------------------------------------------------------------ the quantisation rule
def scene_tri_boxes(sc):
    lb = br.leaf_boxes(bc.scene_triangles(sc))
    return lb[:, :3], lb[:, 3:]


@pytest.fixture(scope="module")
def host_exports():
    """name -> (export, tri_lo, tri_hi) of host-built trees: Collapser::quantise in bvh_build.cpp states refit_node's rule in the same words."""
    out = {}
    for name in ("hall_small", "cornell", "banana"):
        sc = SCENES[name][0]()
        ctx = capi.Context(-1)
        ctx.upload_scene(sc)
        out[name] = (ctx.export_bvh(), *scene_tri_boxes(sc))
        ctx.close()
    return out


@pytest.fixture(scope="module")
def reference_exports():
    """(family, n, builder) -> (export-shaped reference tree, tri_lo, tri_hi) for every GPU case whose tree the device keeps."""
    out = {}
    for family, n in bc.CASES:
        lb = br.leaf_boxes(bc.triangles(family, n))
        for builder in (1, 2):
            r = bc.reference(family, n, builder)
            out[family, n, builder] = (br.export_from_canonical(r["tree"], r["leaf_tris"]), lb[:, :3], lb[:, 3:])
    return out


def test_quantise_ref_equals_the_host_builder(host_exports):
    """Every node of the host-built trees of three scenes, byte for byte: origin, exponents and all 24 plane bytes.  (Run: no node
    differs, so nothing is excused.)"""
    for name, (export, tri_lo, tri_hi) in host_exports.items():
        stats = {}
        bad = br.quantisation_differences(export, tri_lo, tri_hi, stats=stats)
        assert stats["nodes"] == len(export["nodes"]) > 5
        assert not bad, (name, len(bad), bad[:3])


def test_quantisation_is_minimal_up_to_the_slack_the_rule_keeps(host_exports, reference_exports):
    """Per node and axis, on the host-built trees and on the reference's trees of the GPU cases.
    Exponent: it is the smallest one allowed — the step below fails the rule (or the exponent is 1).
    Planes: the rule subtracts / adds 1/16 step before it rounds down / up, so a plane is the tightest byte that contains the child
    in binary32, or — exactly when the child's bound lies less than 1/16 step beyond that byte — the next looser one.  That second
    case is the rule's own slack and nothing else is excused: the test computes the offset as an exact fraction and demands the
    tightest byte whenever the fraction is outside [0, 1/16)."""
    loose = tight = 0
    todo = list(host_exports.values()) + [reference_exports[k] for k in (("soup", 257, 1), ("sheet", 257, 2), ("far", 511, 1), ("ruler", 254, 2), ("duplicates", 256, 2))]
    for export, tri_lo, tri_hi in todo:
        for idx, (clo, chi) in br.exact_child_boxes(export, tri_lo, tri_hi).items():
            q = br.quantise_ref(clo, chi)
            for a in range(3):
                lo, e = q["origin"][a], int(q["ex"][a])
                ext = float(chi[:, a].max()) - float(lo)
                assert e == 1 or not br.quantise_axis_at(e - 1, lo, ext, clo[:, a], chi[:, a])[0]
                sf = F(math.ldexp(1.0, e - 127))
                step = Fraction(2) ** (e - 127)
                for i in range(len(clo)):
                    ql, qh = int(q["qlo"][a, i]), int(q["qhi"][a, i])
                    assert br._plane(ql, sf, lo) <= clo[i, a] and br._plane(qh, sf, lo) >= chi[i, a]
                    xl = (Fraction(float(clo[i, a])) - Fraction(float(lo))) / step          # exact offsets in steps
                    xh = (Fraction(float(chi[i, a])) - Fraction(float(lo))) / step
                    for tightest, got, frac in ((math.floor(xl), ql, xl - math.floor(xl)), (math.ceil(xh), qh, math.ceil(xh) - xh)):
                        sign = -1 if got is ql else 1
                        slack = frac < Fraction(1, 16)
                        assert got == min(255, max(0, tightest + (sign if slack else 0)))
                        loose += slack; tight += not slack
    assert loose > 100 and tight > 10000


def test_the_correction_loops_and_the_exponent_raise_cannot_fire():
    """refit_node (and Collapser::quantise) verify every plane in binary32, move it while it does not hold and raise the exponent
    when that is not enough.  With the rule as it stands none of this can happen for finite boxes, so no input family can reach it:
    the first guess satisfies origin + q * step <= bound in exact arithmetic (floor(x - 1/16) <= x, and the 1/16 covers the double
    rounding of x), q * step is exact in binary32, the plane is therefore ONE rounding of that exact sum, rounding is monotone and
    the bound is itself a binary32 number — so the rounded plane is <= the bound as well.  The same holds for the upper planes, and
    254 steps always reach the top because the start exponent was chosen so.  The loops guard against a rule without the slack.
    Held here on adversarial magnitudes (origins up to 1e30 times the extent), and on every node of every GPU case in the coverage test."""
    rng = np.random.default_rng(5)
    moved = raised = 0
    for _ in range(3000):
        k = int(rng.integers(2, 5))
        mag = 10.0 ** rng.uniform(-30, 30, size=3)
        ext = 10.0 ** rng.uniform(-8, 0, size=3) * mag
        a = rng.uniform(-1, 1, size=3) * mag + rng.uniform(0, 1, size=(k, 3)) * ext
        b = a + rng.uniform(0, 1, size=(k, 3)) * ext * rng.choice([0.0, 1e-6, 1.0], size=(k, 3))
        q = br.quantise_ref(np.minimum(a, b).astype(F), np.maximum(a, b).astype(F))
        moved += q["moved_lo"] + q["moved_hi"]; raised += sum(q["raised"])
    assert moved == 0 and raised == 0


# ------------------------------------------------------------------------------------------------ what the GPU inputs reach
def test_the_gpu_inputs_reach_every_mechanism(host_exports, reference_exports):
    """Counted on the reference alone, per builder where the mechanism belongs to one.  Conditions, not measurements."""
    seen = {b: {} for b in (1, 2)}
    quant = {}
    for (family, n, builder), (export, tri_lo, tri_hi) in reference_exports.items():
        r = bc.reference(family, n, builder)
        s = seen[builder]
        keys = r["keys"]
        lo, hi = br.grid_of(bc.triangles(family, n))
        s["equal_keys"] = s.get("equal_keys", 0) + (len(keys) - len(np.unique(keys)))
        s["flat_axis"] = s.get("flat_axis", 0) + int((hi == lo).any())
        for k, v in list(r["stats"].items()) + list(r.get("ploc_stats", {}).items()):
            s[k] = s.get(k, 0) + v
        s["forced"] = s.get("forced", 0) + len(r.get("forced", []))
        s["levels"] = max(s.get("levels", 0), len(r["level_counts"]))
        br.quantisation_differences(export, tri_lo, tri_hi, stats=quant)        # for the counters: the export-shaped reference has no bytes to compare
    for b in (1, 2):
        for k in ("equal_keys", "flat_axis", "loop1", "loop2", "tie1", "tie2"):
            assert seen[b][k] > 0, (b, k)
        assert seen[b]["levels"] >= 5                          # several BFS levels
    for k in ("cross_block", "tie_to_partner", "tie_to_lowest", "forced"):
        assert seen[2][k] > 0, k
    # the forced round shows in the tree: the reference without the force rule builds another one (test_ploc_force_rule)
    assert bc.reference("line", bc.FORCED_N, 2)["tree"] != bc.reference("line", bc.FORCED_N, 2, 16, False)["tree"]
    # the search radius decides the tree at both sizes of the radius test, and 40 is 32
    for _, n in bc.RADIUS_CASES:
        t = {r: bc.reference("soup", n, 2, r)["tree"] for r in (1, 16, 32, 40)}
        assert t[1] != t[16] != t[32] != t[1] and t[40] == t[32]
    # the fallback: only PLOC can exceed 31 levels on test_gpu_lbvh.py's shapes (a radix tree is at most 63 + 32 binary levels deep,
    # and sheds at most one level per three of them); test_collapse_reports_more_than_31_levels
    assert bc.reference(*bc.TOO_DEEP, 2)["too_deep"] and not bc.reference(*bc.TOO_DEEP, 1)["too_deep"]
    # block borders of the first PLOC round and of the 128-thread launches (collapse, levels, refit): a level of more than 128 nodes
    assert any(max(bc.reference(f, n, b)["level_counts"]) > 128 for f, n in bc.CASES for b in (1, 2))
    # the quantisation: the `m == 0.5` case of the start exponent; the loops and the raise cannot fire (see above) and do not
    assert quant["nodes"] > 3000 and quant["exact_254"] > 0
    assert quant["raised"] == 0 and quant["moved_lo"] == 0 and quant["moved_hi"] == 0
    # nodes of 2, 3 and 4 children: a device-built node above 4 triangles always fills its four slots (loop 2 splits down to single
    # triangles), so 2 and 3 come from the host builder here and, on the GPU, from the graft of an append (root pair, then attach)
    counts = {2: 0, 3: 0, 4: 0}
    for export, _, _ in host_exports.values():
        for k, v in zip(*np.unique(export["nodes"]["meta"] & 7, return_counts=True)):
            counts[int(k)] += int(v)
    assert all(counts[k] > 0 for k in (2, 3, 4)), counts
    assert all(br.child_counts(bc.reference(f, n, b)["tree"])[4] > 0 for f, n in bc.CASES for b in (1, 2))
