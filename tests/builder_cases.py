"""Inputs of the builder-reference tests (test_builder_ref_cpu.py, test_gpu_builder_ref.py): the triangle families, the sizes, and
the reference result per case (computed once per process).  Sizes are the smallest at which a mechanism can go wrong: the
threshold to the device builder and the first leaves (5..17), the borders of the 128- and 256-thread launches, several PLOC rounds
and BFS levels (1000), and one PLOC build whose first round is long enough to be forced (> 4096).  Not a test file."""
import functools

import numpy as np

import builder_ref as br

F = np.float32
FORCED_N = 4160                     # 130 blocks of 32 triangles: the first PLOC round runs over more than 4096 clusters


def soup(n, seed=0):
    """Random triangles in a cube; triangle ids are unrelated to position."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    c = rng.uniform(-1.0, 1.0, size=(n, 1, 3))
    return (c + rng.normal(scale=0.06, size=(n, 3, 3))).astype(F)


def sheet(n, seed=0):
    """A flat, grid-aligned sheet in the plane z = 0: one axis without extent; cell size 1/8, so boxes and areas are exact and many
    areas are equal.  Ids in random order."""
    per_row = int(np.ceil(np.sqrt(n)))
    j = np.random.default_rng(2000 + n + seed).permutation(n)
    x, y = (j % per_row).astype(F) * F(0.125), (j // per_row).astype(F) * F(0.125)
    p = np.zeros((n, 3, 3), dtype=F)
    p[:, :, 0], p[:, :, 1] = x[:, None], y[:, None]
    p[:, 1, 0] += F(0.125); p[:, 2, 1] += F(0.125)
    return p


def duplicates(n, seed=0):
    """Equal sort keys: a third of the triangles are exact copies of a few triangles, a third have different shapes around one and
    the same centroid, the rest is a random soup."""
    rng = np.random.default_rng(3000 + n + seed)
    p = soup(n, seed + 1)
    a, b = n // 3, 2 * (n // 3)
    originals = p[rng.integers(b, n, size=max(1, n // 24))]
    p[:a] = originals[rng.integers(0, len(originals), size=a)]
    d = rng.normal(size=(b - a, 3)).astype(F) * F(0.3)
    p[a:b, 0] = d; p[a:b, 1] = -d * F(0.5) + np.roll(d, 1, axis=1) * F(0.5); p[a:b, 2] = -(p[a:b, 0] + p[a:b, 1])
    return p[rng.permutation(n)]


def far(n, seed=0):
    """A cluster far from the origin (1e4, 1e5 and 1e6 on the three axes) of triangles with extents near 1e-3: the spacing of
    binary32 there is of the size of the quantisation step — where the rule's binary32 verification of every plane would have to
    correct one, if it ever had to (test_builder_ref_cpu.py: it cannot)."""
    rng = np.random.default_rng(4000 + n + seed)
    centre = np.array([1.0e4, -1.0e5, 1.0e6])
    c = centre + rng.uniform(-0.5, 0.5, size=(n, 1, 3)) * np.array([1.0, 4.0, 16.0])
    return (c + rng.uniform(-1.0, 1.0, size=(n, 3, 3)) * rng.uniform(0.5e-3, 2.0e-3, size=(n, 1, 1)) * np.array([1.0, 8.0, 64.0])).astype(F)


def line(n, seed=0):
    """Equal triangles on a line, the gaps growing within every block of 32 and starting over at the next: each triangle's nearest
    neighbour is the one before it, so a PLOC round finds one mutual pair per block (1/32 of the list) — the degenerate input
    the driver's forced round is for.  Ids in random order."""
    gap = F(1.0) + F(0.1) * (np.arange(n) % 32).astype(F)
    x = np.concatenate([[0.0], np.cumsum(gap[:-1] + F(0.5), dtype=np.float64)]).astype(F)
    p = np.zeros((n, 3, 3), dtype=F)
    p[:, :, 0] = x[:, None]
    p[:, 1, 0] += F(0.5); p[:, 2, 1] += F(0.5)
    return p[np.random.default_rng(5000 + n + seed).permutation(n)]


def ruler(n, seed=0):
    """n triangles of width 1/8 side by side along x: the root's extent is n / 8, exactly 254 steps of 2^-3 for n = 254 (and of 2^-4
    for a half of 127) — the case in which refit_node lowers the exponent that frexp gives.  Ids in random order."""
    x = np.random.default_rng(6000 + n + seed).permutation(n).astype(F) * F(0.125)
    p = np.zeros((n, 3, 3), dtype=F)
    p[:, :, 0] = x[:, None]
    p[:, 1, 0] += F(0.125); p[:, 2, 1] += F(0.125)
    return p


def nested(n, seed=0):
    """test_gpu_lbvh.py's nested triangles sharing a corner: every PLOC round finds one mutual pair, the two smallest clusters, so
    the PLOC tree is a chain of more than 31 wide levels and the driver falls back to the host builder."""
    s = (0.999 ** np.arange(n, dtype=np.float64)).astype(F)
    p = np.zeros((n, 3, 3), dtype=F)
    p[:, 1, 0] = s; p[:, 2, 1] = s
    return p


FAMILIES = {"soup": soup, "sheet": sheet, "duplicates": duplicates, "far": far, "line": line, "ruler": ruler, "nested": nested}

THRESHOLD = (5, 6, 7, 8, 9, 17)
BORDERS = (127, 128, 129, 255, 256, 257, 511, 513)
CASES = ([("soup", n) for n in THRESHOLD + BORDERS + (1000,)]
         + [("sheet", n) for n in (9, 129, 257, 1000)]
         + [("duplicates", n) for n in (8, 17, 256, 513)]
         + [("far", n) for n in (7, 128, 511, 1000)]
         + [("ruler", 254)]
         + [("line", FORCED_N)])
TOO_DEEP = ("nested", 160)          # too deep for PLOC (builder 2) only: the radix tree's depth is bounded by the key's 63 bits
RADIUS_CASES = [(radius, n) for radius in (1, 16, 32, 40) for n in (255, 257)]      # 40 is clamped to 32; the sizes straddle a block border
EDIT_CASE = ("soup", 600)           # the mid-sized soup the edits are applied to
APPEND_SIZES = (5, 65, 300)


@functools.lru_cache(maxsize=None)
def triangles(family, n):
    p = FAMILIES[family](n)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(family, n, builder, radius=16, force_rule=True):
    """build_ref of a case whose grid is the box of its own vertices (an upload of nothing else)."""
    p = triangles(family, n)
    return br.build_ref(p, p, builder, radius, force_rule)


def make_scene(tri_pos):
    """A scene of one mesh holding the triangles as they are (identity transform, three vertices per triangle)."""
    from fypraytracer_amd.scene import Material, Scene
    p = np.asarray(tri_pos, dtype=F).reshape(-1, 3)
    n = len(p) // 3
    sc = Scene()
    sc.materials = [Material(albedo=(0.8, 0.8, 0.8))]
    sc.add_new_mesh_to_scene(p, np.tile(np.array([0, 0, 1], F), (n * 3, 1)), np.zeros((n * 3, 2), F), np.arange(n * 3, dtype=np.uint32).reshape(-1, 3), material_index=0)
    return sc


def scene_triangles(sc, first=0, count=None):
    """(count, 3, 3) world positions of the scene's triangles [first, first + count)."""
    t = sc.triangles[first:(None if count is None else first + count)]
    pos = sc.world_vertices["position"]
    return np.stack([pos[t["v0"]], pos[t["v1"]], pos[t["v2"]]], axis=1).astype(F)
