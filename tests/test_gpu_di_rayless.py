"""ReSTIR DI Part 2 as a wavefront keeps the pixels without a shadow ray (sky, emitter, dead ray) out of the ray queue: the setup kernel
appends them to a list of their own at the far end of the task buffer, and the trace kernel runs their epilogues at full width before its
first refill.  Only where a pixel's epilogue runs changes, so pipelined asynchronous frames, blocking frames and the per-pixel Part 2
(tuning key 1 = 0) must agree byte for byte in image, accumulation, reservoirs, history, depth and payload — with few ray-less pixels and
with nothing else, on a queue shorter than the persistent grid, with dead rays skipped or traced (key 18), with light-sorted tasks (key 3)
and on row bands with a halo.  Five frames run both queue parities; they are never waited for in between, so that frames overlap."""
import numpy as np
import pytest

from common import SCENES, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

DI = capi.RESTIR_DI
BUFFERS = {"payload": capi.BUF_PAYLOAD, "depth": capi.BUF_DEPTH, "di": capi.BUF_DI, "di_prev": capi.BUF_DI_PREV}
FRAMES = 5
BLACK = (0.0, 0.0, 0.0)


def _camera(scene_name, view, W, H):
    cam = SCENES[scene_name][1](W, H)
    if view == "sky":                               # Cornell box from its open side, looking away from it
        cam.set_direction((0.0, 0.0, 1.0))
    elif view == "emitter":                         # a hand's breadth under the ceiling light, looking up at it
        d = np.array([0.2, 1.0, 0.1])
        cam.set_direction(tuple(d / np.linalg.norm(d)))
        cam.set_position((0.0, 0.9, 0.0))
    return cam


def _run(mode, scene_name, size, view="default", rows=None, knobs=None, sky=(0.1, 0.2, 0.3), count_last=False):
    """mode: "async" = pipelined frames nothing waits for, "blocking" = fyprt_render, "per_pixel" = blocking with key 1 = 0.
    -> every output of the last frame as bytes (+ the ray counters of one more, instrumented frame with `count_last`)"""
    W, H = size
    ctx = capi.Context(0)
    ctx.resize(W, H)
    if rows:
        ctx.set_rows(*rows)
    ctx.upload_scene(SCENES[scene_name][0]())
    ctx.set_camera(_camera(scene_name, view, W, H))
    for k, v in (knobs or {}).items():
        ctx.set_tuning(k, v)
    if mode == "per_pixel":
        ctx.set_tuning(1, 0)
    st = settings_for(DI, sky_color=sky)
    for f in range(FRAMES):
        st.rand_seed = f + 1
        if mode == "async":
            ctx.render_async(st)
        else:
            ctx.render(st)
    out = {}
    if count_last:
        ctx.set_ray_counting(True)
        st.rand_seed = FRAMES + 1
        s = ctx.render(st)
        ctx.set_ray_counting(False)
        out["counters"] = (s.rays, s.box_tests, s.tri_tests, s.hits, s.node_visits, tuple(s.part_rays), tuple(s.part_node_visits))
    ctx.synchronize()
    y0, y1 = rows[:2] if rows else (0, H)
    img, acc = ctx.readback()
    out.update(image=img.reshape(H, W)[y0:y1].tobytes(), accum=acc.reshape(H, W, 4)[y0:y1].tobytes(), frame_index=ctx.frame_index)
    for name, b in BUFFERS.items():
        out[name] = ctx.read_buffer(b).tobytes()
    out["payload_array"] = ctx.read_buffer(capi.BUF_PAYLOAD)
    ctx.close()
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if k != "payload_array":
            assert a[k] == b[k], f"{what}: {k} differs"


CASES = {
    "cornell_64x48": dict(scene_name="cornell", size=(64, 48)),
    "hall_small_160x90": dict(scene_name="hall_small", size=(160, 90)),
    "hall_small_160x90_black_sky": dict(scene_name="hall_small", size=(160, 90), sky=BLACK),      # dead rays exist only under a black sky
    "queue_shorter_than_the_grid_16x16": dict(scene_name="cornell", size=(16, 16)),
    "all_sky": dict(scene_name="cornell", size=(64, 48), view="sky"),
    "all_emitter": dict(scene_name="cornell", size=(64, 48), view="emitter"),
    "dead_rays_traced": dict(scene_name="hall_small", size=(160, 90), sky=BLACK, knobs={18: 0}),
    "dead_rays_skipped": dict(scene_name="hall_small", size=(160, 90), sky=BLACK, knobs={18: 1}),
    "sorted_tasks": dict(scene_name="hall_small", size=(160, 90), sky=BLACK, knobs={3: 1}),
    "sorted_tasks_all_sky": dict(scene_name="cornell", size=(64, 48), view="sky", knobs={3: 1}),
    "upper_band_with_halo": dict(scene_name="hall_small", size=(160, 90), sky=BLACK, rows=(0, 44, 30)),
    "lower_band_with_halo": dict(scene_name="hall_small", size=(160, 90), sky=BLACK, rows=(44, 90, 30)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_pipelined_blocking_and_per_pixel_frames_agree(name):
    kw = CASES[name]
    a = _run("async", **kw)
    _same(a, _run("blocking", **kw), "pipelined against blocking frames")
    _same(a, _run("per_pixel", **kw), "wavefront against per-pixel Part 2")
    pay = a["payload_array"]
    if kw.get("view") == "sky":                     # the case is what it says: no pixel has a ray
        assert (pay["hitDistance"] < 0.0).all()
    elif kw.get("view") == "emitter":
        assert (pay["hitDistance"] >= 0.0).all() and set(np.unique(pay["objectIndex"])) <= {30, 31}      # the light's two triangles
    elif not kw.get("rows"):
        assert (pay["hitDistance"] >= 0.0).any()


def test_dead_rays_leave_the_queue_and_the_frame_as_it_was():
    """Key 18 moves pixels between the two lists (ray queue <-> ray-less list) and nothing else."""
    kw = dict(scene_name="hall_small", size=(160, 90), sky=BLACK)
    a, b = _run("async", knobs={18: 1}, count_last=True, **kw), _run("async", knobs={18: 0}, count_last=True, **kw)
    assert a["counters"][5][2] < b["counters"][5][2]                 # fewer rays traced by the trace kernel ...
    a.pop("counters"); b.pop("counters")
    _same(a, b, "key 18 = 1 against key 18 = 0")                     # ... for the same frame


@pytest.mark.parametrize("scene_name,size,sky", [("cornell", (64, 48), (0.1, 0.2, 0.3)), ("hall_small", (160, 90), BLACK)])
def test_an_instrumented_frame_counts_what_the_per_pixel_kernel_counts(scene_name, size, sky):
    """The instrumented trace kernel follows the same queue layout; pixels without a ray were never counted, so rays, box tests, triangle
    tests, hits and node visits are those of the per-pixel Part 2, which traces the same rays one thread per pixel."""
    a = _run("blocking", scene_name, size, sky=sky, count_last=True)
    b = _run("per_pixel", scene_name, size, sky=sky, count_last=True)
    assert a["counters"][0] > 0
    assert a["counters"][:5] == b["counters"][:5]
    _same({k: v for k, v in a.items() if k != "counters"}, {k: v for k, v in b.items() if k != "counters"}, "the frame after the instrumented one")
