"""CPU-side tests of the C-ABI library: it loads, exports every symbol include/fyprt.h declares, keeps
the documented struct layouts, validates its inputs, and its host builders (acceleration structure,
light trees) satisfy their invariants.  No compute call is made without a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from common import check_bvh_invariants, struct_equal
from fypraytracer_amd import capi, scenes

ROOT = Path(__file__).resolve().parent.parent


def test_library_exports_every_declared_symbol():
    header = (ROOT / "include" / "fyprt.h").read_text()
    declared = sorted(set(re.findall(r"\b(fyprt_[a-z_0-9]+)\s*\(", header)))
    assert len(declared) >= 20
    lib = capi.load_library()
    for name in declared:
        assert hasattr(lib, name), f"libfyprt.so does not export {name}"
    assert sorted(capi.EXPORTED_SYMBOLS) == declared
    assert b"gfx950" in lib.fyprt_version()


def test_struct_layouts_match_reference_sizes():
    # RenderingSettings 52 B, Vertex 32 B, Material 44 B, RayHitPayload 40 B, DI reservoir 20 B, GI reservoir 72 B
    assert C.sizeof(capi.Settings) == 52 and capi.VERTEX_DTYPE.itemsize == 32 and capi.MATERIAL_DTYPE.itemsize == 44
    assert capi.PAYLOAD_DTYPE.itemsize == 40 and capi.DI_DTYPE.itemsize == 20 and capi.GI_DTYPE.itemsize == 72
    s = capi.Settings()
    assert (s.to_accumulate, s.light_bounces, s.sample_count, s.technique, s.light_candidate_count, s.rand_seed) == (1, 1, 1, 0, 4, 1)
    assert (s.use_temporal_reuse, s.use_spatial_reuse, s.temporal_history_limit, s.spatial_neighbor_num, s.spatial_neighbor_radius) == (0, 0, 2, 5, 30)
    assert tuple(s.sky_color) == (1.0, 1.0, 1.0)                     # RenderingSettings.h:7-21 defaults
    assert capi.Settings.technique.offset == 24 and capi.Settings.rand_seed.offset == 32 and capi.Settings.temporal_history_limit.offset == 40


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.FyprtError):
        capi.Context(0)
    missing = ROOT / "fypraytracer_amd" / "csrc" / "does_not_exist.so"
    with pytest.raises(capi.FyprtError):
        capi.load_library(missing)


def test_host_only_context_refuses_to_render_and_validates_scenes():
    ctx = capi.Context(-1)
    with pytest.raises(capi.FyprtError):
        ctx.resize(16, 16)
    sc = scenes.cornell_box()
    ctx.upload_scene(sc)
    assert capi.live_device_bytes() == 0                              # a host-only context allocates nothing on a device
    with pytest.raises(capi.FyprtError):
        ctx.render(capi.Settings())
    bad = scenes.cornell_box()
    bad.triangles = bad.triangles.copy()
    bad.triangles["v0"][3] = 10_000                                   # vertex index out of range
    with pytest.raises(capi.FyprtError, match="out of range"):
        ctx.upload_scene(bad)
    bad2 = scenes.cornell_box()
    bad2.meshes = bad2.meshes[:-1]                                    # meshes no longer partition the triangles
    with pytest.raises(capi.FyprtError, match="partition"):
        ctx.upload_scene(bad2)
    ctx.close()
    assert capi.live_device_bytes() == 0


@pytest.mark.parametrize("name", ["cornell", "hall_small"])
def test_bvh_invariants(name):
    sc = scenes.cornell_box() if name == "cornell" else scenes.hall_scene_small()
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    b = ctx.export_bvh()
    check_bvh_invariants(b, sc)
    ctx.close()


def _one_mesh_scene(pos):
    from fypraytracer_amd.scene import Material, Scene
    n = len(pos) // 3
    sc = Scene()
    sc.materials = [Material(albedo=(1, 1, 1))]
    sc.add_new_mesh_to_scene(pos, np.tile(np.array([0, 0, 1], dtype=np.float32), (n * 3, 1)), np.zeros((n * 3, 2), dtype=np.float32),
                             np.arange(n * 3, dtype=np.uint32).reshape(-1, 3), material_index=0)
    return sc


def _tree_levels(b):
    nodes = b["nodes"]

    def lv(ref):
        if ref < 0:
            return 0
        n = nodes[ref]
        return 1 + max(lv(int(c)) for c in n["child"][:int(n["meta"]) & 7])
    return lv(b["root"])


@pytest.mark.parametrize("force_safe", [False, True])
@pytest.mark.parametrize("shape", ["nested", "exponential"])
def test_bvh_depth_is_bounded_by_construction(shape, force_safe, monkeypatch):
    """Pathological inputs for SAH — a long chain of ever smaller nested triangles sharing a corner, and triangles at
    exponentially shrinking distances (every split peels off a handful) — must still give a tree of <= 31 wide levels: the
    binary builder falls back to median splits when its depth budget runs out, first under a generous bound (48), and the
    whole build is repeated under the bound that guarantees it (30) should the collapse still be too deep; `force_safe`
    runs that second build unconditionally."""
    if force_safe:
        monkeypatch.setenv("FYPRT_BVH_FORCE_SAFE_DEPTH", "1")
    if shape == "nested":
        n = 6000
        s = 0.999 ** np.arange(n, dtype=np.float64)
        pos = np.zeros((n * 3, 3), dtype=np.float32)
        pos[1::3, 0] = s
        pos[2::3, 1] = s
    else:
        n = 480
        x = (2.0 ** -(np.arange(n, dtype=np.float64) * 0.25)).astype(np.float32)
        pos = np.zeros((n * 3, 3), dtype=np.float32)
        pos[0::3, 0] = x
        pos[1::3, 0] = x * 1.01
        pos[2::3, 0] = x
        pos[2::3, 1] = x * 0.01
    sc = _one_mesh_scene(pos)
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    b = ctx.export_bvh()
    assert b["max_stack"] <= 31 and _tree_levels(b) == b["max_stack"]
    if force_safe:
        assert b["max_stack"] <= 30
    assert sorted(b["tris"]["tri"].tolist()) == list(range(n))
    assert ctx.get_tuning(8) >= b["max_stack"]                                # the stack budget never undercuts the level count
    ctx.close()


def test_light_tree_builder_does_not_depend_on_the_host_libm(oracle_built):
    """The light trees fix the light-sampling distribution (LightTree.cpp:21-340), so a drop-in library must build the same trees on every
    host.  (1) the builder's object file imports no transcendental of the C library — its acos / cos / sin are rt_hostmath.h's fixed
    binary64 algorithms, the device's own; (2) on the 256-light hall the trees equal the oracle's restatement bit for bit, and the
    oracle's builder evaluates the same functions with ITS deterministic routines; (3) the libm flavour of the oracle (the reference's own
    __host__ behaviour: acosf / cosf / sinf of glibc) agrees with them except where glibc rounds a value the other way — counted and
    printed, not required to be zero: that residue is exactly what the product no longer inherits from the host."""
    import subprocess
    from pathlib import Path
    from oraclelib import Oracle
    obj = Path(capi.__file__).resolve().parent / "csrc" / "lighttree_build.o"
    undefined = subprocess.run(["nm", "-u", str(obj)], capture_output=True, text=True, check=True).stdout.split()
    libm = [sym for sym in undefined if sym.split("@")[0] in {"acos", "acosf", "cos", "cosf", "sin", "sinf", "sincos", "sincosf", "tan", "tanf", "atan2", "atan2f", "pow", "powf"}]
    assert not libm, libm
    sc = scenes.hall_scene(columns=8, column_segments=24, column_rings=10, drapes=2, drape_n=30, light_quads=128, lights_per_mesh=1)   # 256 emissive triangles in 128 one-quad meshes: a deep TLAS
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    mine = ctx.export_lighttrees(len(sc.meshes))
    det = Oracle(sc, 8, 8).export_lighttrees()
    assert len(mine["tlas"]) == len(det["tlas"]) > 100
    for k in ("tlas", "blas"):
        assert struct_equal(mine[k], det[k]).all()
    host = Oracle(sc, 8, 8, libm=True).export_lighttrees()
    differing = sum(int((~struct_equal(mine[k], host[k])).sum()) for k in ("tlas", "blas") if len(mine[k]) == len(host[k]))
    print(f"light-tree nodes that differ under glibc's acosf / cosf / sinf: {differing} of {len(mine['tlas']) + len(mine['blas'])}")
    ctx.close()


@pytest.mark.parametrize("name", ["cornell", "hall_small"])
def test_light_trees_equal_the_oracles_restatement(oracle_built, name):
    """LIGHT_SOURCE_SAMPLING / NEE parity hinges on the light trees (LightTree.cpp:21-293, quirks included):
    the library's builder and the oracle's independent restatement must agree bit for bit."""
    from oraclelib import Oracle
    sc = scenes.cornell_box() if name == "cornell" else scenes.hall_scene_small()
    ctx = capi.Context(-1)
    ctx.upload_scene(sc)
    mine = ctx.export_lighttrees(len(sc.meshes))
    orc = Oracle(sc, 8, 8)
    ref = orc.export_lighttrees()
    assert mine["tlas_root"] == ref["tlas_root"] and len(mine["tlas"]) == len(ref["tlas"]) > 0
    for k in ("tlas", "blas"):
        assert struct_equal(mine[k], ref[k]).all()
    for k in ("blas_first", "blas_count", "blas_root"):
        assert np.array_equal(mine[k], ref[k])
    # prebuilt trees (option (i) of the boundary) are accepted and exported unchanged
    ctx2 = capi.Context(-1)
    ctx2.upload_scene(sc, light_trees=ref)
    again = ctx2.export_lighttrees(len(sc.meshes))
    assert struct_equal(again["tlas"], ref["tlas"]).all() and struct_equal(again["blas"], ref["blas"]).all()
    assert np.array_equal(orc.emissive(), sc.emissive_triangles)
    ctx.close(); ctx2.close()
