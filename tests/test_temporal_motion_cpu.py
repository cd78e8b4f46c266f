"""Object motion for the temporal denoiser (fyprt_denoise_temporal_set_motion) without a GPU: the symbol and its errors on a host-only
context, the numpy restatement of the contract (tests/temporal_motion_ref.py) against tests/temporal_ref.py where no triangle moved, and
the contract itself on CPU-oracle sequences in which a mesh is dragged a step before every frame — the moved mesh keeps its history, the
rest of the image keeps its own, and the kept history beats starting over."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import assert_numpy_keeps_subnormals, guides_from_scene
from fypraytracer_amd import capi
from oraclelib import Oracle
from temporal_motion_ref import moved_triangles, temporal_motion_ref
from temporal_ref import camera_matrix, temporal_ref

EINVAL, ESTATE = -1, -3     # FYPRT_EINVAL, FYPRT_ESTATE
HEADER = Path(__file__).resolve().parent.parent / "include" / "fyprt.h"
F = np.float32
MOVES = [("", (0.0, 0.0)), ("W", (60.0, -25.0)), ("DE", (-140.0, 40.0)), ("S", (90.0, 70.0)), ("AQ", (-35.0, -110.0)), ("W", (20.0, 10.0))]
# (scene, size, mesh, per-frame step of the position, per-frame step of the rotation in degrees)
DRAGS = [("cornell", (96, 80), 6, (-0.02, 0.0, 0.015), (0.0, 2.0, 0.0)),
         ("cornell", (96, 80), 5, (0.015, 0.0, 0.01), (0.0, -2.0, 0.0)),
         ("hall_small", (160, 96), 7, (0.02, 0.0, -0.015), (0.0, 1.5, 0.0))]
FAST = ("cornell", (96, 80), 6, (-0.08, 0.0, 0.06), (0.0, 12.0, 0.0))     # the first drag at five / six times its speed: 0.1 units, 12 degrees


def test_symbol_errors_and_mode_rules_on_host_only_context():
    lib = capi.load_library()
    name = "fyprt_denoise_temporal_set_motion"
    assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(r"int %s\(" % name, HEADER.read_text())
    assert lib.fyprt_denoise_temporal_set_motion(None, 0) == EINVAL and lib.fyprt_denoise_temporal_set_motion(None, 1) == EINVAL
    ctx = capi.Context(-1)
    for bad in (2, -1, 256, 1 << 20):
        assert lib.fyprt_denoise_temporal_set_motion(ctx.h, bad) == EINVAL
    # allowed on a host-only context, before and after a scene: it stores the flag; every value in effect is a no-op
    for v in (0, 0, 1, 1, 0, 1):
        assert lib.fyprt_denoise_temporal_set_motion(ctx.h, v) == 0
    ctx.upload_scene(SCENES["cornell"][0]())
    for v in (1, 0, 0, 1):
        assert lib.fyprt_denoise_temporal_set_motion(ctx.h, v) == 0
        # the temporal calls themselves stay refused, and there is no history to read, whatever the mode
        with pytest.raises(capi.FyprtError):
            ctx.denoise_temporal()
        with pytest.raises(capi.FyprtError):
            ctx.read_buffer(capi.BUF_TEMPORAL)
    assert lib.fyprt_denoise_temporal_set_motion(ctx.h, 3) == EINVAL       # a refused value leaves the mode alone ...
    assert lib.fyprt_denoise_temporal_reset(ctx.h) == 0
    ctx.denoise_temporal_set_motion(True)                                  # ... and the wrapper maps truth values to 1 / 0
    ctx.denoise_temporal_set_motion(False)
    ctx.close()


# ---------------------------------------------------------------------------------------------- reference against reference
def test_motion_ref_without_motion_is_temporal_ref(oracle_built):
    """cornell 24 x 20, three frames under MOVES: no snapshot, and a snapshot bit-equal to the current vertices, both give temporal_ref's
    radiance, image and history record bit for bit — chained, so the histories are compared too."""
    assert_numpy_keeps_subnormals()
    W, H = 24, 20
    sc = SCENES["cornell"][0]()
    cam = SCENES["cornell"][1](W, H)
    orc = Oracle(sc, W, H)
    st = settings_for(capi.RESTIR_DI, sky_color=(0.0, 0.0, 0.0), sample_count=1)
    st.to_accumulate = 0
    hists, M = [None, None, None], None
    verts = sc.world_vertices
    assert not moved_triangles(sc.triangles, verts, verts.copy()).any()
    for f in range(3):
        cam.on_update(0.05, *MOVES[f])
        orc.set_camera(cam)
        st.rand_seed = f + 1
        orc.render(st)
        acc, pay = orc.accum().copy(), orc.read_buffer(capi.BUF_PAYLOAD).reshape(H, W).copy()
        alb = guides_from_scene(sc, pay)
        want = temporal_ref(acc, pay, alb, 1, M, hists[0], iterations=3)
        none = temporal_motion_ref(acc, pay, alb, 1, M, hists[1], sc.triangles, verts, None, iterations=3)
        same = temporal_motion_ref(acc, pay, alb, 1, M, hists[2], sc.triangles, verts, verts.copy(), iterations=3)
        for got in (none, same):
            assert bits_equal(got[0], want[0]).all() and (got[1] == want[1]).all() and struct_equal(got[2].ravel(), want[2].ravel()).all()
        hists, M = [want[2], none[2], same[2]], camera_matrix(cam)
        cam.commit_frame()
    assert (hists[0]["N"] == 3).any()
    orc.close()


# ---------------------------------------------------------------------------------------------- object motion on CPU-oracle sequences
@functools.lru_cache(maxsize=None)
def _drag_sequence(scene_name, size, mesh, dpos, drot, frames=8, truth_frames=128):
    """One edit before every frame: the mesh's position and rotation advance by (dpos, drot).  Every frame is rendered by a new Oracle on
    the edited scene that adopts the previous one's per-pixel state (ReSTIR DI, both reuses, one sample, to_accumulate = 0, static
    camera).  Per frame: (accum, payload, albedo guide, the world vertices it was rendered with); then the scene, the camera matrix and
    `truth_frames` accumulated frames of the final scene."""
    W, H = size
    sc = SCENES[scene_name][0]()
    cam = SCENES[scene_name][1](W, H)
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    base = dict(sc.mesh_transforms[mesh])
    st = settings_for(capi.RESTIR_DI, sky_color=(0.0, 0.0, 0.0), sample_count=1)
    st.to_accumulate = 0
    out, orc = [], None
    for f in range(frames):
        k = f + 1
        mgr.set_mesh_transform(sc, mesh, pos=tuple(F(b) + F(k) * F(d) for b, d in zip(base["pos"], dpos)),
                               rotation=tuple(F(b) + F(k) * F(d) for b, d in zip(base["rotation"], drot)))
        mgr.perform_all_scene_updates(sc)
        new = Oracle(sc, W, H)
        new.set_camera(cam)
        if orc is not None:
            new.adopt_frame(orc)
            orc.close()
        orc = new
        st.rand_seed = k
        orc.render(st)
        pay = orc.read_buffer(capi.BUF_PAYLOAD).reshape(H, W).copy()
        out.append((orc.accum().copy(), pay, guides_from_scene(sc, pay), sc.world_vertices.copy()))
    orc.close()
    tr = Oracle(sc, W, H)
    tr.set_camera(cam)
    st.to_accumulate = 1
    for g in range(truth_frames):
        st.rand_seed = 1000 + g
        tr.render(st)
    truth = (tr.accum()[..., :3] / F(truth_frames)).astype(np.float64)
    tr.close()
    return out, sc, camera_matrix(cam), truth


def _kept_and_dropped(case):
    """The contract chained over the sequence with the history kept (a snapshot before every call but the first), and a first call on the
    last frame (what the edits leave without the mode).  Returns per call the shares of pixels with N == k on and off the moved mesh, and
    the two whole-image MSEs (linear radiance) at the last call."""
    scene_name, size, mesh, dpos, drot = case
    frames, sc, M, truth = _drag_sequence(*case)
    first, count, _ = sc.meshes[mesh]
    hist, prev, on_mesh, off_mesh = None, None, [], []
    for k, (acc, pay, alb, verts) in enumerate(frames, start=1):
        rad, _, hist = temporal_motion_ref(acc, pay, alb, 1, M, hist, sc.triangles, verts, prev)
        prev = verts
        flt = alb[..., 3] != 0
        on = flt & (pay["objectIndex"] >= first) & (pay["objectIndex"] < first + count)
        assert on.sum() > 20 and (flt & ~on).sum() > 0.5 * flt.size
        on_mesh.append(float((hist["N"][on] == k).mean()))
        off_mesh.append(float((hist["N"][flt & ~on] == k).mean()))
    acc, pay, alb, _ = frames[-1]
    dropped = temporal_ref(acc, pay, alb, 1, None, None)[0]

    def mse(x):
        return float(np.mean((x[..., :3].astype(np.float64) - truth) ** 2))
    return on_mesh, off_mesh, mse(rad), mse(dropped)


@pytest.mark.parametrize("case", DRAGS, ids=lambda c: f"{c[0]}-mesh{c[2]}")
def test_dragged_mesh_keeps_its_history(oracle_built, case):
    assert_numpy_keeps_subnormals()
    on_mesh, off_mesh, kept, dropped = _kept_and_dropped(case)
    print(f"{case[0]} {case[1]} mesh {case[2]} step {case[3]} {case[4]}: share with N == k on the mesh {[round(s, 4) for s in on_mesh]}, "
          f"off the mesh {[round(s, 4) for s in off_mesh]}; MSE at call 8 kept {kept:.6g}, dropped {dropped:.6g}, ratio {kept / dropped:.3f}")
    assert min(on_mesh[1:]) > 0.5, on_mesh
    assert min(off_mesh[1:]) > 0.9, off_mesh
    assert kept < dropped


def test_fast_motion_is_the_documented_limit(oracle_built):
    """Printed, not asserted: 0.1 units and 12 degrees per frame on cornell mesh 6 — a long history of a surface whose lighting changes
    lags behind it; history_limit is the control (DESIGN.md §4 quotes these numbers)."""
    on_mesh, off_mesh, kept, dropped = _kept_and_dropped(FAST)
    print(f"fast: {FAST[0]} mesh {FAST[2]} step {FAST[3]} {FAST[4]}: share with N == k on the mesh {[round(s, 4) for s in on_mesh]}, "
          f"off the mesh {[round(s, 4) for s in off_mesh]}; MSE at call 8 kept {kept:.6g}, dropped {dropped:.6g}, ratio {kept / dropped:.3f}")
    assert np.isfinite([kept, dropped]).all()
