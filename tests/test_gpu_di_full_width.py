"""ReSTIR DI trace kernel: the production kernel's cooperative leaf phase against the instrumented kernel of the same build.

The production instantiation of k_di_part2_trace tests the triangles of a leaf phase cooperatively — all (lane, triangle) pairs of the
wave spread over its 64 lanes, one LDS word per pair, the owner's ray fetched with cross-lane reads; the instrumented instantiation
(set_ray_counting) keeps the serial leaf loop.  No operation on a ray may change, so both must write the same bytes: every case renders
3 frames (seeds 1..3, temporal and spatial reuse on) once on each kernel and compares image, accumulation, this frame's DI records, the
history records and depth after EVERY frame, bit for bit.  The production frames go through render_async (the pipelined path).

How a frame's rays reach the waves: the persistent grid is max(8, min(CUs x workgroups per CU, 16 x 16 tiles of the frame)) workgroups of
four waves, and a queue shorter than two 128-task chunks per wave is dealt out in even static shares (rt_wavefront.h: `first`).  At 96 x 54
that is 48 workgroups = 192 waves for about 3 600 rays: some 20 rays per wave, so no wave is ever full there.  Which kinds of leaf phase
each case runs was recorded once with a -DRT_DI_LEAF_STATS build, which flags them per frame (profiles/di_full_width/leaf_phase_kinds.txt;
the production kernel carries no counter):
  - cornell 8 x 8 (one partly filled wave), cornell 17 x 9 (partial tiles, several waves), hall_small 96 x 54 with a black sky, with a lit
    sky (0.1, 0.2, 0.3), with sorted tasks (key 3 = 1) and with chunks of ONE task (keys 4, 10, 9 at their smallest value 1, one workgroup per
    CU: every refill hands out a single ray): one-round cooperative phases only.
  - hall_small_full_waves, 640 x 360 with one workgroup per CU: 256 workgroups = 1024 waves for about 160 000 rays, about 157 per wave, so all
    64 lanes hold a ray.  Recorded: one-round phases, phases of MORE THAN 64 PAIRS (the loop over rounds and the clipping of an owner's
    slot range at a round's edges) in every frame, and in frame 2 a phase with a closest-mode lane (serial loop for the whole wave).
  - banana (the procedural stand-in, 64 x 64; its tree has 306 single-triangle leaves among 1729), as it is and with chunks of one task:
    in every frame phases of SINGLE-TRIANGLE LEAVES ONLY (the wave-uniform `m2 == 0` fallback to the serial loop) beside one-round phases.
    hall_small's tree has no single-triangle leaf at all (5548 leaves of two triangles) and never takes that fallback.
"""
import pytest

from common import SCENES, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

BUFFERS = {"di": capi.BUF_DI, "di_prev": capi.BUF_DI_PREV, "depth": capi.BUF_DEPTH}
BLACK, LIT = (0.0, 0.0, 0.0), (0.1, 0.2, 0.3)


def frames(scene_name, W, H, sky, tuning, counting):
    """3 frames, seeds 1..3 -> per frame a dict of the compared buffers' bytes"""
    mk_scene, mk_cam = SCENES[scene_name]
    sc = mk_scene()
    ctx = capi.Context(0)
    try:
        ctx.resize(W, H)
        ctx.upload_scene(sc)
        ctx.set_camera(mk_cam(W, H))
        for key, value in tuning:
            ctx.set_tuning(key, value)
        ctx.set_ray_counting(counting)
        out = []
        for seed in (1, 2, 3):
            st = settings_for(capi.RESTIR_DI, sky_color=sky, rand_seed=seed)
            if counting:
                stats = ctx.render(st)
                assert stats.rays > 0
            else:
                ctx.render_async(st)                      # the pipelined production path; readback synchronises
            img, acc = ctx.readback()
            snap = {"image": img.tobytes(), "accum": acc.tobytes()}
            for name, b in BUFFERS.items():
                snap[name] = ctx.read_buffer(b).tobytes()
            out.append(snap)
        return out
    finally:
        ctx.close()


CASES = {
    "cornell_8x8_partial_wave": ("cornell", 8, 8, BLACK, ()),
    "cornell_17x9": ("cornell", 17, 9, BLACK, ()),
    "hall_small": ("hall_small", 96, 54, BLACK, ()),
    "hall_small_lit_sky": ("hall_small", 96, 54, LIT, ()),
    "hall_small_sorted_tasks": ("hall_small", 96, 54, BLACK, ((3, 1),)),
    "hall_small_one_task_chunks": ("hall_small", 96, 54, BLACK, ((2, 1), (9, 1), (4, 1), (10, 1))),
    "hall_small_full_waves": ("hall_small", 640, 360, BLACK, ((2, 1),)),
    "banana": ("banana_standin", 64, 64, BLACK, ()),
    "banana_one_task_chunks": ("banana_standin", 64, 64, BLACK, ((2, 1), (9, 1), (4, 1), (10, 1))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_production_kernel_equals_instrumented_kernel(case):
    scene_name, W, H, sky, tuning = CASES[case]
    production = frames(scene_name, W, H, sky, tuning, counting=False)
    instrumented = frames(scene_name, W, H, sky, tuning, counting=True)
    for f, (a, b) in enumerate(zip(production, instrumented), 1):
        for name in a:
            assert a[name] == b[name], f"{case}: {name} of frame {f} differs between the production and the instrumented trace kernel"
    assert production[0]["accum"] != production[2]["accum"]           # (the frames did render something)
