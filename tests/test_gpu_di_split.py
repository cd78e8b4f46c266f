"""Split Part 1 of pipelined ReSTIR DI frames (tuning key 21): the history-free half (k_di_part1_primary, primary ray + light candidates)
runs on a stream of its own beside the previous frame's setup kernel and hands its pixels to the history half (k_di_part1_temporal) on the
front stream through a staging set per frame parity.  Both halves are cut out of k_di_part1 without reordering an operation, so every output
must be the same bits as with key 21 = 0 and as blocking frames: image, accumulation, payload, depth, this frame's reservoirs, the history,
the frame index — after every frame of a sequence, and at the end of sequences that are never waited for in between (only those keep
several frames in flight).  Six frames make the staging parity wrap three times; the camera turns every frame, so temporal reprojection
reads other pixels and prevProjView changes.  72 x 40 has partial tiles in both directions."""
from dataclasses import replace

import numpy as np
import pytest

from common import SCENES, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

DI, GI = capi.RESTIR_DI, capi.RESTIR_GI
TURNS = [(0.0, 0.0), (60.0, -25.0), (-140.0, 40.0), (90.0, 70.0), (-35.0, -110.0), (20.0, 10.0)]   # mouse-look per frame, in pixels
BUFFERS = {"payload": capi.BUF_PAYLOAD, "depth": capi.BUF_DEPTH, "di": capi.BUF_DI, "di_prev": capi.BUF_DI_PREV}
SIX = [("frame", {})] * 6


def _snapshot(ctx, rows, extra=None):
    ctx.synchronize()
    y0, y1 = rows[:2] if rows else (0, ctx.height)
    img, acc = ctx.readback()                      # rows outside the context's band are not copied
    snap = {"image": img[y0:y1].tobytes(), "accum": acc[y0:y1].tobytes(), "frame_index": ctx.frame_index}
    for name, b in BUFFERS.items():
        snap[name] = ctx.read_buffer(b).tobytes()
    if extra:
        snap.update(extra)
    return snap


def _execute(script, mode, scene_name="hall_small", size=(72, 40), rows=None, in_flight=False, **settings):
    """Runs `script` on a fresh context and returns its snapshots: one per operation, or with `in_flight` only the last one (nothing waits
    in between).  mode: "split" = asynchronous frames with key 21 = 1, "unsplit" = with key 21 = 0, "blocking" = fyprt_render."""
    mk_scene, mk_cam = SCENES[scene_name]
    W, H = size
    sc = mk_scene()
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    cam = mk_cam(W, H)
    ctx = capi.Context(0)
    ctx.resize(W, H)
    if rows:
        ctx.set_rows(*rows)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    ctx.set_tuning(21, 1 if mode == "split" else 0)
    snaps, f = [], 0
    for n, (kind, kw) in enumerate(script):
        extra = None
        if kind == "frame":
            cam.on_update(0.05, "", TURNS[f % len(TURNS)])
            ctx.set_camera(cam)
            st = settings_for(kw.get("tech", DI), spatial_neighbor_radius=30, temporal_history_limit=2, **settings)
            st.rand_seed = f + 1
            st.to_accumulate = kw.get("accumulate", 1)
            if kw.get("count"):                    # an instrumented frame is never pipelined: k_di_part1, with its counters
                ctx.set_ray_counting(True)
                s = ctx.render(st)
                ctx.set_ray_counting(False)
                extra = {"counters": (s.rays, s.box_tests, s.tri_tests, s.hits, s.node_visits, tuple(s.part_rays), tuple(s.part_node_visits), s.launches)}
                assert s.rays > 0
            elif mode == "blocking":
                ctx.render(st)
            else:
                ctx.render_async(st)
            cam.commit_frame()
            f += 1
        elif kind == "denoise":
            img, rad = ctx.denoise()
            extra = {"denoised": img.tobytes(), "denoised_radiance": rad.tobytes()}
        elif kind == "vertices":
            mgr.set_mesh_transform(sc, 3, pos=(0.1, 0.0, -0.1), rotation=(0.0, 20.0, 0.0))
            mgr.perform_all_scene_updates(sc)
            ctx.update_vertices(sc)
        elif kind == "materials":                  # hall: columns and drapes become emitters — emissive list, light records and trees change
            sc.materials[2] = replace(sc.materials[2], emission_color=(1.0, 0.6, 0.3), emission_power=2.5)
            mgr.material_edited(2)
            mgr.perform_all_scene_updates(sc)
            ctx.update_materials(sc)
        elif kind == "camera":                     # a posed camera: the previous-frame matrices are reset with it
            cam.set_position(tuple(np.asarray(cam.position, dtype=np.float32) + np.float32([0.2, 0.1, -0.1])))
            ctx.set_camera(cam)
        elif kind == "resize":
            W, H = kw["size"]
            ctx.resize(W, H)
            ctx.set_rows(0, H, 0)
            cam = mk_cam(W, H)
            ctx.set_camera(cam)
        else:
            raise ValueError(kind)
        if not in_flight or n == len(script) - 1:
            snaps.append(_snapshot(ctx, rows, extra))
    ctx.close()
    return snaps


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for n, (sa, sb) in enumerate(zip(a, b)):
        assert sa.keys() == sb.keys()
        for k in sa:
            assert sa[k] == sb[k], f"{what}: {k} differs after operation {n + 1} of {len(a)}"


def _check(script, with_blocking=False, **kw):
    split = _execute(script, "split", **kw)
    _assert_same(split, _execute(script, "unsplit", **kw), "key 21 = 1 against key 21 = 0")
    if with_blocking:
        _assert_same(split, _execute(script, "blocking", **kw), "key 21 = 1 against blocking frames")


@pytest.mark.parametrize("scene_name,size", [("hall_small", (72, 40)), ("cornell", (72, 40)), ("hall_small", (200, 120))])
def test_six_frames_under_a_turning_camera(scene_name, size):
    _check(SIX, with_blocking=True, scene_name=scene_name, size=size)


@pytest.mark.parametrize("scene_name", ["hall_small", "cornell"])
def test_accumulation_restarted_on_frame_3(scene_name):
    script = [("frame", {"accumulate": 0 if f == 2 else 1}) for f in range(6)]
    _check(script, with_blocking=True, scene_name=scene_name)


@pytest.mark.parametrize("settings", [{"use_temporal_reuse": 0}, {"light_candidate_count": 0}, {"light_candidate_count": 1}],
                         ids=["no_temporal_reuse", "no_candidates", "one_candidate"])
@pytest.mark.parametrize("scene_name", ["hall_small", "cornell"])
def test_settings_that_change_what_the_halves_do(scene_name, settings):
    _check(SIX, with_blocking=True, scene_name=scene_name, **settings)


@pytest.mark.parametrize("rows", [(16, 40, 30), (0, 8, 30)], ids=["bottom_band", "top_band_with_the_extra_last_row"])
def test_a_row_band_with_a_halo(rows):
    """Part 1 runs on the band's rows plus the halo — and for a band at the top of the frame on the single last row of the frame as well
    (the reference's unsigned neighbour coordinate wraps there): both kernels of the split cover the same pixels."""
    _check(SIX, with_blocking=True, rows=rows)


INTERLEAVED = {
    "denoise": [("frame", {}), ("frame", {}), ("denoise", {}), ("frame", {}), ("frame", {}), ("denoise", {}), ("frame", {})],
    "update_vertices": [("frame", {}), ("frame", {}), ("vertices", {}), ("frame", {}), ("frame", {}), ("frame", {})],
    "update_materials": [("frame", {}), ("frame", {}), ("materials", {}), ("frame", {}), ("frame", {}), ("frame", {})],
    "set_camera": [("frame", {}), ("frame", {}), ("camera", {}), ("frame", {}), ("frame", {}), ("camera", {}), ("frame", {})],
    "resize": [("frame", {}), ("frame", {}), ("frame", {}), ("resize", {"size": (56, 33)}), ("frame", {}), ("frame", {}), ("frame", {})],
    "restir_gi_frame": [("frame", {}), ("frame", {}), ("frame", {"tech": GI}), ("frame", {}), ("frame", {}), ("frame", {})],
    "ray_counting_frame": [("frame", {}), ("frame", {}), ("frame", {"count": True}), ("frame", {}), ("frame", {}), ("frame", {"count": True})],
}


@pytest.mark.parametrize("name", list(INTERLEAVED))
def test_asynchronous_frames_interleaved_with(name):
    _check(INTERLEAVED[name])


@pytest.mark.parametrize("name", list(INTERLEAVED))
def test_interleaved_sequences_never_waited_for(name):
    """The same sequences without a read in between: whatever the calls themselves do not wait for stays in flight."""
    _check(INTERLEAVED[name], in_flight=True, size=(200, 120))


def test_frames_in_flight_on_a_frame_large_enough_to_overlap():
    """Twelve frames enqueued back to back on 640 x 360 pixels: the primary kernel of frame N+1 really runs beside frame N's setup and trace
    kernels, and the staging sets are reused while two frames are in flight."""
    _check([("frame", {})] * 12, with_blocking=True, in_flight=True, size=(640, 360))


def test_a_split_frame_reports_three_parts():
    """Part 0 = the primary kernel (its own events on its stream), part 1 = temporal + setup on the front stream, part 2 = the trace kernel."""
    mk_scene, mk_cam = SCENES["hall_small"]
    W, H = 200, 120
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(mk_scene())
    ctx.set_camera(mk_cam(W, H))
    assert ctx.get_tuning(21) == 1                  # the default
    st = settings_for(DI)
    for f in range(4):
        st.rand_seed = f + 1
        ctx.render_async(st)
    ctx.synchronize()
    for back in range(4):
        ms, n = ctx.frame_timings(back)
        assert n == 3 and all(m > 0.0 for m in ms[:3]) and ms[3] == 0.0, (back, ms, n)
    ctx.close()
