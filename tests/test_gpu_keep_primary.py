"""Kept primary hits of ReSTIR DI frames (tuning key 25): while the camera and the geometry stand still a frame reads the payload an earlier
frame traced instead of tracing it again.  Nothing a caller can see may depend on that, so every test feeds the same calls to two contexts,
one with key 25 = 1 and one with key 25 = 0, and compares after EVERY frame, bit for bit: image, accumulation, payload, this frame's DI
records, the history records and depth.  fyprt_kept_primary_frames tells a kept frame from one that was silently traced again.
hall_small at 128 x 72 (partial tiles vertically, several workgroups) and cornell at 64 x 64."""
from dataclasses import replace

import numpy as np
import pytest

from append_common import append_patch
from common import SCENES, settings_for
from fypraytracer_amd import capi

pytestmark = pytest.mark.gpu

DI, GI, NEE = capi.RESTIR_DI, capi.RESTIR_GI, capi.NEE
BUFFERS = {"payload": capi.BUF_PAYLOAD, "di": capi.BUF_DI, "di_prev": capi.BUF_DI_PREV, "depth": capi.BUF_DEPTH}
SIZES = {"hall_small": (128, 72), "cornell": (64, 64)}
BOTH_SCENES = pytest.mark.parametrize("scene_name", ["hall_small", "cornell"])


class Pair:
    """Two contexts fed the same calls: `a` keeps primary hits (key 25 = 1, the default), `b` traces every frame (key 25 = 0)."""

    def __init__(self, scene_name, tuning=(), rows=None, with_patch=False):
        mk_scene, mk_cam = SCENES[scene_name]
        self.name, (self.W, self.H) = scene_name, SIZES[scene_name]
        self.sc = mk_scene()
        self.mgr = self.sc.manager()
        self.mgr.perform_all_scene_updates(self.sc)
        self.cam = mk_cam(self.W, self.H)
        self.patch = append_patch(self.sc, self.cam, scene_name, 40, 0) if with_patch else None   # a mesh a test may remove again
        self.rows, self.seed, self.ctxs = rows, 0, []
        for key25 in (1, 0):
            ctx = capi.Context(0)
            ctx.resize(self.W, self.H)
            if rows:
                ctx.set_rows(*rows)
            ctx.upload_scene(self.sc)
            ctx.set_object_vertices(self.sc)
            ctx.set_camera(self.cam)
            for k, v in tuning:
                ctx.set_tuning(k, v)
            ctx.set_tuning(25, key25)
            self.ctxs.append(ctx)
        self.a, self.b = self.ctxs

    def each(self, call):
        for ctx in self.ctxs:
            call(ctx)

    def set_rows(self, *rows):
        self.rows = rows
        self.each(lambda ctx: ctx.set_rows(*rows))

    def _snapshot(self, ctx):
        y0, y1 = self.rows[:2] if self.rows else (0, self.H)
        img, acc = ctx.readback()                  # synchronises; rows outside the context's band are not copied
        snap = {"image": img[y0:y1].tobytes(), "accum": acc[y0:y1].tobytes(), "frame_index": ctx.frame_index}
        for name, b in BUFFERS.items():
            snap[name] = ctx.read_buffer(b).tobytes()
        return snap

    def frame(self, tech=DI, blocking=False, count=False):
        """The next frame (seeds 1, 2, ...) on both contexts; every output compared; returns by how much `a`'s kept-frame counter moved
        (and with `count` the instrumented frame's statistics of `a` as well).  `b` must never keep."""
        self.seed += 1
        st = settings_for(tech)
        st.rand_seed = self.seed
        before, snaps, stats = self.a.kept_primary_frames(), [], []
        for ctx in self.ctxs:
            if count:
                ctx.set_ray_counting(True)
                stats.append(ctx.render(st))
                ctx.set_ray_counting(False)
            elif blocking:
                ctx.render(st)
            else:
                ctx.render_async(st)
            snaps.append(self._snapshot(ctx))
        for k in snaps[0]:
            assert snaps[0][k] == snaps[1][k], f"{self.name}: {k} differs after frame {self.seed} (key 25 = 1 against key 25 = 0)"
        assert self.b.kept_primary_frames() == 0
        kept = self.a.kept_primary_frames() - before
        return (kept, stats[0]) if count else kept

    def close(self):
        self.each(lambda ctx: ctx.close())


@pytest.fixture
def pair(request):
    made = []

    def make(*args, **kw):
        made.append(Pair(*args, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


# ---- 1. the still frame
@pytest.mark.parametrize("mode", ["split", "unsplit", "unpipelined", "blocking_frame_in_the_middle"])
@BOTH_SCENES
def test_1_still_frame(pair, scene_name, mode):
    """Eight frames, seeds 1..8: the first traces, seven keep — as split kernels (default), as the one kept kernel on the front stream
    (key 21 = 0), on the context stream (key 11 = 0), and with a blocking frame, which takes the one kernel, among split ones."""
    p = pair(scene_name, tuning={"unsplit": [(21, 0)], "unpipelined": [(11, 0)]}.get(mode, []))
    kept = [p.frame(blocking=(mode == "blocking_frame_in_the_middle" and f == 4)) for f in range(8)]
    assert kept == [0] + [1] * 7
    assert p.a.kept_primary_frames() == 7 and p.b.kept_primary_frames() == 0


# ---- 2. every invalidator, each between two kept frames
def _move_mesh(p, mesh, k=1.0):
    p.mgr.set_mesh_transform(p.sc, mesh, pos=(0.1 * k, 0.05 * k, -0.1 * k), rotation=(0.0, 20.0 * k, 0.0))
    assert p.mgr.perform_all_scene_updates(p.sc) is True


def _inv_set_camera(p):
    p.cam.set_position(tuple(np.asarray(p.cam.position, dtype=np.float32) + np.float32([0.2, 0.1, -0.1])))
    p.each(lambda ctx: ctx.set_camera(p.cam))


def _inv_update_vertices(p):
    _move_mesh(p, 3)
    p.each(lambda ctx: ctx.update_vertices(p.sc))


def _inv_update_mesh_vertices(p):
    _move_mesh(p, 3)
    p.each(lambda ctx: ctx.update_mesh_vertices(p.sc, [3]))


def _inv_update_transforms(p):
    _move_mesh(p, 3)
    p.each(lambda ctx: ctx.update_transforms(p.sc, [3]))


def _inv_append_meshes(p):
    m = append_patch(p.sc, p.cam, p.name, 40, 0, shift=(0.1, 0.1, 0.0))
    p.each(lambda ctx: ctx.append_meshes(p.sc, m))


def _inv_remove_meshes(p):
    rec = p.sc.remove_meshes_from_scene([p.patch])
    p.each(lambda ctx: ctx.remove_meshes(rec))


def _inv_regraft_meshes(p):
    p.each(lambda ctx: ctx.regraft_meshes([3]))


def _inv_upload_scene(p):
    p.each(lambda ctx: ctx.upload_scene(p.sc))


def _inv_resize(p):
    def there_and_back(ctx):
        ctx.resize(p.W - 24, p.H - 16)
        ctx.resize(p.W, p.H)
    p.each(there_and_back)


INVALIDATORS = {"set_camera": _inv_set_camera, "update_vertices": _inv_update_vertices, "update_mesh_vertices": _inv_update_mesh_vertices,
                "update_transforms": _inv_update_transforms, "append_meshes": _inv_append_meshes, "remove_meshes": _inv_remove_meshes,
                "regraft_meshes": _inv_regraft_meshes, "upload_scene": _inv_upload_scene, "resize": _inv_resize}


@pytest.mark.parametrize("name", list(INVALIDATORS))
@BOTH_SCENES
def test_2_invalidator_between_kept_frames(pair, scene_name, name):
    """traced, kept | the call | traced again (the counter stands still, the outputs are those of a traced frame), kept again"""
    p = pair(scene_name, with_patch=(name == "remove_meshes"))
    assert [p.frame(), p.frame()] == [0, 1]
    INVALIDATORS[name](p)
    assert [p.frame(), p.frame()] == [0, 1], name


@pytest.mark.parametrize("tech", [NEE, GI], ids=["nee", "restir_gi"])
@BOTH_SCENES
def test_2_a_frame_of_another_technique_invalidates(pair, scene_name, tech):
    """k_primary and k_gi_primary write the same payload buffer and keep nothing."""
    p = pair(scene_name)
    assert [p.frame(), p.frame()] == [0, 1]
    assert p.frame(tech=tech) == 0
    assert [p.frame(), p.frame()] == [0, 1]


# ---- 3. what must NOT invalidate
@BOTH_SCENES
def test_3_set_camera_with_the_same_camera_keeps(pair, scene_name):
    """The same pose handed over again, once as it is and once with prev_* := the current matrices (what an application does after every
    frame): prevProjView changes, and with it the temporal reprojection, but none of the five fields the payload depends on."""
    p = pair(scene_name)
    p.cam.on_update(0.05, "", (60.0, -25.0))             # the pose differs from the previous-frame matrices
    p.each(lambda ctx: ctx.set_camera(p.cam))
    assert [p.frame(), p.frame()] == [0, 1]
    p.each(lambda ctx: ctx.set_camera(p.cam))
    assert p.frame() == 1
    p.cam.commit_frame()
    p.each(lambda ctx: ctx.set_camera(p.cam))
    assert [p.frame(), p.frame()] == [1, 1]


@BOTH_SCENES
def test_3_update_materials_keeps(pair, scene_name):
    """A surface turns emissive and back: emissive list, light records and what a pixel finishes with change — the payload holds no material."""
    p = pair(scene_name)
    assert [p.frame(), p.frame()] == [0, 1]
    old = p.sc.materials[2]
    for mat in (replace(old, emission_color=(1.0, 0.6, 0.3), emission_power=2.5), old):
        p.sc.materials[2] = mat
        p.mgr.material_edited(2)
        p.mgr.perform_all_scene_updates(p.sc)
        p.each(lambda ctx: ctx.update_materials(p.sc))
        assert [p.frame(), p.frame()] == [1, 1]


# ---- 4. rows
def test_4_a_band_with_a_halo_and_the_extra_last_row(pair):
    """Rows [16, 48) with a halo of 30 on 72 rows: the band is a part of the frame, Part 1 runs on band + halo cut at the frame's edges.
    Then [24, 56) with the same halo: band + halo still cover the whole frame, but a moved band traces once all the same (the band is part
    of what a kept payload is compared by), and keeps afterwards."""
    p = pair("hall_small", rows=(16, 48, 30))
    assert [p.frame() for _ in range(4)] == [0, 1, 1, 1]
    p.set_rows(24, 56, 30)
    assert [p.frame() for _ in range(3)] == [0, 1, 1]


def test_4_a_top_band_whose_part_1_takes_row_h_minus_1(pair):
    """Rows [0, 20) with a halo of 30: Part 1 covers [0, 50) and the single row 71 (part1_rows: the reference's unsigned neighbour
    coordinate wraps to the last row).  Narrowing the halo changes the row set and costs one traced frame."""
    p = pair("hall_small", rows=(0, 20, 30))
    assert [p.frame() for _ in range(3)] == [0, 1, 1]
    p.set_rows(0, 20, 12)
    assert [p.frame() for _ in range(2)] == [0, 1]


# ---- 5. an instrumented frame after kept frames
@BOTH_SCENES
def test_5_an_instrumented_frame_traces_and_re_establishes(pair, scene_name):
    p = pair(scene_name)
    assert [p.frame() for _ in range(3)] == [0, 1, 1]
    kept, stats = p.frame(count=True)
    assert kept == 0 and stats.part_rays[0] == p.W * p.H
    assert [p.frame(), p.frame()] == [1, 1]              # the instrumented frame wrote the payload the next one keeps


# ---- 6. the key
def test_6_tuning_key_25():
    """Range and default as for the other keys.  The key is 25, not 24: tests/test_gpu_tuning.py asserts that set_tuning(24, 0) is refused, so
    24 stays unassigned (every value refused, like a key past the end) and 23 stays reserved."""
    ctx = capi.Context(0)
    assert ctx.get_tuning(25) == 1
    ctx.set_tuning(25, 0)
    assert ctx.get_tuning(25) == 0
    with pytest.raises(capi.FyprtError, match="0..1"):
        ctx.set_tuning(25, 2)
    assert ctx.lib.fyprt_set_tuning(ctx.h, 25, -1) == -1 and ctx.get_tuning(25) == 0
    ctx.set_tuning(25, 1)
    for key, value in ((23, 1), (24, 0), (24, 1), (26, 0)):
        with pytest.raises(capi.FyprtError):
            ctx.set_tuning(key, value)
    with pytest.raises(capi.FyprtError):
        ctx.get_tuning(26)
    assert ctx.kept_primary_frames() == 0
    ctx.close()
