"""Object motion for the temporal denoiser (fyprt_denoise_temporal_set_motion) on the GPU against the numpy restatement of its contract
(tests/temporal_motion_ref.py), in the pattern of tests/test_gpu_temporal.py: radiance4, rgba8 and FYPRT_BUF_TEMPORAL equal bit for bit
(NaN-aware) on every pixel, the reference chained on its own history and re-seeded from the device's.  The reference is handed the scene's
world vertices of the frame denoised before and of the frame denoised now, taken from scene.world_vertices around
perform_all_scene_updates — where no edit lies between two calls the two are bit-equal and the reference moves nothing, which is what a
call without a pending snapshot must compute."""
import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import assert_numpy_keeps_subnormals
from fypraytracer_amd import capi
from fypraytracer_amd.scene import mesh_matrix
from temporal_motion_ref import temporal_motion_ref
from temporal_ref import DEFAULTS, camera_matrix

pytestmark = pytest.mark.gpu
F = np.float32
# tests/test_gpu_moving_camera.py's MOVES: (keys held, mouse delta in pixels) per frame
MOVES = [("", (0.0, 0.0)), ("W", (60.0, -25.0)), ("DE", (-140.0, 40.0)), ("S", (90.0, 70.0)), ("AQ", (-35.0, -110.0)), ("W", (20.0, 10.0))]
# per scene: {mesh: (position step, rotation step in degrees, scale step)} per edit
DRAG = {"cornell": {5: ((0.015, 0.0, 0.01), (0.0, -2.0, 0.0), (0.01, 0.0, 0.01)), 6: ((-0.02, 0.0, 0.015), (0.0, 2.0, 1.0), (0.0, -0.01, 0.0))},
        "hall_small": {7: ((0.02, 0.0, -0.015), (0.0, 1.5, 0.0), (0.0, 0.0, 0.0))}}
HIDDEN_HALL_MESH = 3           # no pixel of hall_small's camera sees it


class Rig:
    """A context with the mode on (or off), its scene, and what drags it: edit() moves the listed meshes one more step and applies the edit
    by update_transforms or update_vertices; self.verts is then the geometry the next frame is traced in."""
    def __init__(self, scene_name, W, H, motion=True, tuning=()):
        self.name, self.W, self.H = scene_name, W, H
        self.sc = SCENES[scene_name][0]()
        self.mgr = self.sc.manager()
        self.mgr.perform_all_scene_updates(self.sc)
        self.cam = SCENES[scene_name][1](W, H)
        self.ctx = capi.Context(0)
        for k, v in tuning:
            self.ctx.set_tuning(k, v)
        self.ctx.resize(W, H)
        self.ctx.upload_scene(self.sc)
        self.ctx.set_object_vertices(self.sc)
        self.ctx.set_camera(self.cam)
        if motion:
            self.ctx.denoise_temporal_set_motion(True)
        self.base = [dict(t) for t in self.sc.mesh_transforms]
        self.steps = [0] * len(self.sc.meshes)
        self.verts = self.sc.world_vertices.copy()
        self.seed = 0

    def edit(self, drag=None, path="transforms"):
        drag = DRAG[self.name] if drag is None else drag
        for m, (dp, dr, ds) in drag.items():
            self.steps[m] += 1
            k, b = F(self.steps[m]), self.base[m]
            self.mgr.set_mesh_transform(self.sc, m, pos=tuple(F(x) + k * F(d) for x, d in zip(b["pos"], dp)),
                                        rotation=tuple(F(x) + k * F(d) for x, d in zip(b["rotation"], dr)),
                                        scale_=tuple(F(x) + k * F(d) for x, d in zip(b["scale"], ds)))
        self.mgr.perform_all_scene_updates(self.sc)
        self.verts = self.sc.world_vertices.copy()
        if path == "transforms":
            self.ctx.update_transforms(self.sc, list(drag))
        else:
            self.ctx.update_vertices(self.sc)

    def frame(self, st, move=None, asynchronous=False):
        """Renders one frame; returns (frame index it was rendered with, projection x view of its camera)."""
        if move is not None:
            self.cam.on_update(0.05, *move)
        self.ctx.set_camera(self.cam)
        n = self.ctx.frame_index
        self.seed += 1
        st.rand_seed = self.seed
        (self.ctx.render_async if asynchronous else self.ctx.render)(st)
        M = camera_matrix(self.cam)
        if move is not None:
            self.cam.commit_frame()
        return n, M

    def on_meshes(self, tri, meshes):
        """Mask of the payload triangle indices `tri` that belong to the listed meshes."""
        on = np.zeros(tri.shape, bool)
        for m in meshes:
            first, count, _ = self.sc.meshes[m]
            on |= (tri >= first) & (tri < first + count)
        return on

    def close(self):
        self.ctx.close()


class Ref:
    """What the reference carries from one call to the next: the history record, the matrix and the world vertices of the frame denoised."""
    def __init__(self):
        self.hist, self.M, self.verts = None, None, None

    def reset(self):
        self.hist = None


def _same(what, got, want):
    rad, img, rec = got
    want_rad, want_img, want_rec = want
    eq = bits_equal(rad, want_rad)
    assert eq.all(), f"{what}: {(~eq).sum()} of {eq.size} radiance values differ, first at {np.argwhere(~eq)[:3].tolist()}"
    assert (img == want_img).all(), f"{what}: {(img != want_img).sum()} packed pixels differ"
    for name in rec.dtype.names:
        eq = bits_equal(rec[name], want_rec[name])
        assert eq.all(), f"{what}: history field {name}: {(~eq).sum()} of {eq.size} values differ, first at {np.argwhere(~eq)[:3].tolist()}"


def _call(rig, n, M, refs, what="", **kw):
    """One fyprt_denoise_temporal call on the frame rendered last, compared with temporal_motion_ref continued from every state in `refs`:
    (Ref, reseed) pairs.  Returns (image, radiance, history record, payload triangle indices)."""
    ctx, H, W = rig.ctx, rig.H, rig.W
    par = dict(DEFAULTS)
    par.update(kw)
    img, rad = ctx.denoise_temporal(capi.TemporalParams(**par))
    acc = ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)
    pay = ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    alb = ctx.read_buffer(capi.BUF_ALBEDO).reshape(H, W, 4)
    rec = ctx.read_buffer(capi.BUF_TEMPORAL).reshape(H, W)
    for ref, reseed in refs:
        want = temporal_motion_ref(acc, pay, alb, n, ref.M, ref.hist, rig.sc.triangles, rig.verts, ref.verts if ref.hist is not None else None, **par)
        _same(f"{what} {'re-seeded' if reseed else 'chained'} {kw}", (rad, img, rec), want)
        ref.hist, ref.M, ref.verts = (rec if reseed else want[2]), M, rig.verts
    return img, rad, rec, pay["objectIndex"]


def _moved_with_full_history(rig, rec, tri, meshes, k):
    on = rig.on_meshes(tri, meshes) & (rec["filterable"] != 0)
    return on.any() and bool((rec["N"][on] == k).any())


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("tech", [capi.RESTIR_DI, capi.NEE])
@pytest.mark.parametrize("scene_name", ["cornell", "hall_small"])
def test_sequences_equal_the_contract(scene_name, tech, moving):
    """Six calls at 96 x 64, an edit before every frame (cornell: meshes 5 and 6 together, translated, rotated and scaled; hall_small:
    mesh 7), to_accumulate = 0, static camera or MOVES; the edit applied by update_transforms and, in a second context, by update_vertices
    with the host-computed vertices — both equal the contract and so each other.  The history of the moved meshes survives."""
    assert_numpy_keeps_subnormals()
    outs = {}
    for path in ("transforms", "vertices"):
        rig = Rig(scene_name, 96, 64)
        st = settings_for(tech)
        st.to_accumulate = 0
        refs = [(Ref(), False), (Ref(), True)]
        outs[path], kept = [], []
        for f in range(6):
            rig.edit(path=path)
            n, M = rig.frame(st, MOVES[f] if moving else None)
            img, rad, rec, tri = _call(rig, n, M, refs, f"{scene_name} tech {tech} {'moving' if moving else 'static'} {path} call {f + 1}")
            outs[path].append((img, rad, rec))
            kept.append(_moved_with_full_history(rig, rec, tri, DRAG[scene_name], f + 1))
        assert all(kept), kept                                          # N == call number occurs on the moved meshes after every call
        rig.close()
    for k, (a, b) in enumerate(zip(outs["transforms"], outs["vertices"])):
        assert (a[0] == b[0]).all() and bits_equal(a[1], b[1]).all() and struct_equal(a[2].ravel(), b[2].ravel()).all(), f"paths differ at call {k + 1}"


def test_snapshot_is_the_geometry_of_the_last_denoised_frame():
    """Two edits of the same mesh with a frame but no call between them, then a call: it reprojects against the geometry of the frame
    denoised last, not of the frame rendered last.  Then an edit of a mesh no pixel sees, and an edit of every mesh (every wave takes the
    reconstruction)."""
    rig = Rig("hall_small", 96, 64)
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    refs = [(Ref(), False), (Ref(), True)]
    _call(rig, *rig.frame(st), refs, "first call")
    rig.edit()
    rig.frame(st)                                                      # a frame nobody denoises
    rig.edit()
    rig.edit()                                                         # ... and two edits without a frame between them
    _, _, rec, tri = _call(rig, *rig.frame(st), refs, "one call after three edits and two frames")
    assert _moved_with_full_history(rig, rec, tri, [7], 2)
    hidden = {HIDDEN_HALL_MESH: ((0.0, 0.05, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, 0.0))}
    rig.edit(hidden)
    _, _, rec, tri = _call(rig, *rig.frame(st), refs, "an edit of a mesh no pixel sees")
    assert not rig.on_meshes(tri, [HIDDEN_HALL_MESH]).any()
    flt = rec["filterable"] != 0
    assert (rec["N"][flt] == 3).mean() > 0.9
    everything = {m: ((0.004, 0.002, -0.003), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) for m in range(len(rig.sc.meshes))}
    rig.edit(everything)
    _, _, rec, _ = _call(rig, *rig.frame(st), refs, "an edit of every mesh")
    assert (rec["N"][flt] == 4).any()
    rig.edit(everything, path="vertices")
    _call(rig, *rig.frame(st, MOVES[1]), refs, "every mesh by update_vertices, camera moved too")
    rig.close()


@pytest.mark.parametrize("size", [(33, 5), (16, 16)])
def test_sizes_off_the_tile(size):
    rig = Rig("cornell", *size)
    st = settings_for(capi.NEE)
    st.to_accumulate = 0
    refs = [(Ref(), False), (Ref(), True)]
    for f, it in enumerate((1, 0, 3, 5)):
        rig.edit()
        _call(rig, *rig.frame(st, MOVES[f]), refs, f"cornell {size} call {f + 1}", iterations=it)
    rig.close()


def test_parameter_points_on_a_moving_object_sequence():
    """cornell 96 x 64, ReSTIR DI, static camera, an edit and a frame before every call, so that every parameter point runs the motion form."""
    assert_numpy_keeps_subnormals()
    points = [dict(iterations=0), dict(iterations=3), dict(history_limit=1), dict(history_limit=2), dict(history_limit=32), dict(normal_min=0.0),
              dict(normal_min=0.999), dict(plane_max=1e-4), dict(plane_max=10.0), dict(feedback=0), dict(feedback=1)]
    rig = Rig("cornell", 96, 64)
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    refs = [(Ref(), False), (Ref(), True)]
    _call(rig, *rig.frame(st), refs, "first call")
    for k, kw in enumerate(points):
        rig.edit()
        _, _, rec, tri = _call(rig, *rig.frame(st), refs, f"point {k + 1}", **kw)
        assert (rec["N"][rig.on_meshes(tri, DRAG["cornell"])] >= (1 if kw.get("history_limit") == 1 else 2)).any()
    rig.close()


def test_mode_on_without_an_edit_is_mode_off():
    outs = []
    for motion in (False, True):
        rig = Rig("cornell", 96, 64, motion=motion)
        st = settings_for(capi.RESTIR_DI)
        st.to_accumulate = 0
        out = []
        for f in range(3):
            rig.frame(st, MOVES[f])
            out.append(rig.ctx.denoise_temporal() + (rig.ctx.read_buffer(capi.BUF_TEMPORAL),))
        outs.append(out)
        rig.close()
    for a, b in zip(*outs):
        assert (a[0] == b[0]).all() and bits_equal(a[1], b[1]).all() and struct_equal(a[2], b[2]).all()
    assert (outs[1][2][2]["N"] == 3).any()


def test_mode_semantics_and_what_still_drops_the_history():
    """Switching the mode on and off again behaves as never set; a change of the mode drops the history; upload_scene, update_materials,
    resize and the reset each drop history and pending snapshot; a refused call keeps both."""
    W, H = 96, 64
    rig = Rig("cornell", W, H, motion=False)
    ctx = rig.ctx
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    ref = Ref()
    refs = [(ref, False)]

    def first_call(what):
        _, _, rec, _ = _call(rig, *rig.frame(st), refs, what)
        assert (rec["N"] <= 1).all(), what

    def later_call(what, k=2):
        _, _, rec, tri = _call(rig, *rig.frame(st), refs, what)
        assert _moved_with_full_history(rig, rec, tri, DRAG["cornell"], k), what
        return rec

    ctx.denoise_temporal_set_motion(True)
    ctx.denoise_temporal_set_motion(False)                             # as never set: an edit drops the history
    first_call("start")
    rig.edit()
    ref.reset()
    first_call("mode off after on: an edit drops the history")
    ctx.denoise_temporal_set_motion(False)                             # the value in effect: nothing happens
    _, _, rec, _ = _call(rig, ctx.frame_index, ref.M, refs, "a no-op set_motion keeps the history")
    assert (rec["N"] == 2).any()
    ctx.denoise_temporal_set_motion(True)                              # a change of the mode drops it
    ref.reset()
    with pytest.raises(capi.FyprtError, match="FYPRT_BUF_TEMPORAL"):
        ctx.read_buffer(capi.BUF_TEMPORAL)
    _, _, rec, _ = _call(rig, ctx.frame_index, ref.M, refs, "after switching the mode on, same frame")
    assert (rec["N"] <= 1).all()
    ctx.denoise_temporal_set_motion(True)                              # the value in effect
    rig.edit()
    later_call("mode on: the edit keeps the history")
    # a refused call — no complete frame after the edit — keeps history and snapshot
    rig.edit()
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise_temporal()
    later_call("after a refused call", 3)
    # each of the four, between an edit (snapshot pending) and the next call
    rig.edit()
    ctx.denoise_temporal_reset()
    ref.reset()
    first_call("after reset with a snapshot pending")
    rig.edit()
    later_call("the reset left the mode on")
    rig.edit()
    ctx.update_materials(rig.sc)
    ref.reset()
    first_call("after update_materials")
    rig.edit()
    ctx.upload_scene(rig.sc)
    ctx.set_object_vertices(rig.sc)
    ref.reset()
    first_call("after upload_scene")
    rig.edit()
    later_call("upload_scene left the mode on")
    rig.edit()
    ctx.resize(W, H)
    ref.reset()
    first_call("after resize")
    rig.edit()
    later_call("resize left the mode on")
    ctx.denoise_temporal_set_motion(False)                             # off with a history: dropped, and edits drop it again
    ref.reset()
    first_call("after switching the mode off")
    rig.edit()
    ref.reset()
    first_call("mode off: an edit drops the history")
    rig.close()


def _state(ctx):
    ctx.synchronize()
    return [ctx.read_buffer(b) for b in range(10)], ctx.frame_index


def _same_state(a, b):
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        eq = struct_equal(x, y) if x.dtype.names else bits_equal(x, y)
        assert eq.all(), f"buffer {k} differs"
    assert a[1] == b[1]


@pytest.mark.parametrize("tech", [capi.RESTIR_DI, capi.RESTIR_GI])
def test_frames_after_calls_are_the_frames_without_them(tech):
    """edit, frame, call — three times — then a frame leaves the buffers of the same edits and frames without calls (ReSTIR DI pipelined
    over two streams, key 11 = 1; blocking entries)."""
    results = []
    for with_calls in (True, False):
        rig = Rig("hall_small", 96, 64, tuning=((11, 1),))
        st = settings_for(tech)
        st.to_accumulate = 0
        refs = [(Ref(), False)]
        for f in range(4):
            rig.edit()
            n, M = rig.frame(st)
            if with_calls and f < 3:
                _call(rig, n, M, refs, f"tech {tech} frame {f + 1}", iterations=3)
        rig.ctx.denoise()
        results.append(_state(rig.ctx))
        rig.close()
    _same_state(results[0], results[1])


def test_torch_path_between_pipelined_frames():
    """In a fresh process that initialises torch's CUDA before the library is loaded (tests/test_gpu_query.py explains why)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_temporal_motion as t; "
            "t._torch_checks(); print('torch path ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_checks():
    """The device entry into torch tensors between asynchronous pipelined frames with an edit before each, never synchronised by the host
    between frame and call: equals the host entry of a blocking sequence, history record included, and the frames are the frames of the
    same edits without calls.  ReSTIR DI and GI."""
    import torch
    W, H = 96, 64
    par = capi.TemporalParams(iterations=3)
    for tech in (capi.RESTIR_DI, capi.RESTIR_GI):
        st = settings_for(tech)
        st.to_accumulate = 0
        dev = Rig("hall_small", W, H, tuning=((11, 1),))
        outs = []
        for f in range(4):
            dev.edit()
            dev.frame(st, asynchronous=True)
            img_t = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
            rad_t = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
            dev.ctx.denoise_temporal_tensor(img_t, rad_t, par)
            outs.append((img_t, rad_t * 1.0))
        dev_rec = dev.ctx.read_buffer(capi.BUF_TEMPORAL)
        dev_state = _state(dev.ctx)
        host = Rig("hall_small", W, H, tuning=((11, 1),))
        plain = Rig("hall_small", W, H, tuning=((11, 1),))
        for f in range(4):
            host.edit()
            host.frame(st)
            img, rad = host.ctx.denoise_temporal(par)
            assert (outs[f][0].cpu().numpy().view(np.uint32) == img).all(), (tech, f)
            assert bits_equal(outs[f][1].cpu().numpy(), rad).all(), (tech, f)
            plain.edit()
            plain.frame(st, asynchronous=True)
        rec = host.ctx.read_buffer(capi.BUF_TEMPORAL)
        assert struct_equal(dev_rec, rec).all()
        tri = host.ctx.read_buffer(capi.BUF_PAYLOAD)["objectIndex"]
        assert (rec["N"][host.on_meshes(tri, [7])] == 4).any()
        plain.ctx.denoise_temporal(par)                                 # (FYPRT_BUF_ALBEDO of the last frame, so that _state can read it)
        _same_state(dev_state, _state(plain.ctx))
        for r in (dev, host, plain):
            r.close()


def test_snapshot_memory_is_released():
    """The snapshot is allocated by the first edit that has a history to keep, released by upload_scene and by switching the mode off, and
    gone with the context."""
    base = capi.live_device_bytes()
    rig = Rig("cornell", 40, 24)
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    rig.frame(st)
    rig.edit()                                                         # no history yet: nothing to keep, nothing allocated
    rig.frame(st)
    rig.ctx.denoise_temporal()
    before = capi.live_device_bytes()
    rig.edit()
    want = 32 * len(rig.sc.world_vertices) + len(rig.sc.triangles)
    assert capi.live_device_bytes() - before == want
    rig.edit()
    assert capi.live_device_bytes() - before == want
    rig.ctx.denoise_temporal_set_motion(False)
    assert capi.live_device_bytes() == before
    rig.ctx.denoise_temporal_set_motion(True)
    rig.frame(st)
    rig.ctx.denoise_temporal()
    rig.edit()
    assert capi.live_device_bytes() - before == want
    rig.ctx.upload_scene(rig.sc)
    assert capi.live_device_bytes() <= before
    rig.ctx.set_object_vertices(rig.sc)
    rig.frame(st)
    rig.ctx.denoise_temporal()
    rig.edit()
    rig.close()
    assert capi.live_device_bytes() == base


def test_update_transforms_with_given_matrices():
    """Context.update_transforms with `matrices` applies them instead of the scene's: the same frame as the edit made through the scene."""
    frames = []
    for given in (False, True):
        rig = Rig("cornell", 40, 24, motion=False)
        st = settings_for(capi.RESTIR_DI)
        st.to_accumulate = 0
        if given:
            tr = rig.sc.mesh_transforms[6]
            M = mesh_matrix(tuple(F(x) + F(d) for x, d in zip(tr["pos"], (0.05, 0.0, -0.03))), tr["rotation"], tr["scale"])
            rig.ctx.update_transforms(rig.sc, [6], [M])                # the host scene is left as it was
            with pytest.raises(ValueError):
                rig.ctx.update_transforms(rig.sc, [5, 6], [M])
        else:
            rig.edit({6: ((0.05, 0.0, -0.03), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))})
        rig.frame(st)
        frames.append(rig.ctx.readback())
        rig.close()
    assert (frames[0][0] == frames[1][0]).all() and bits_equal(frames[0][1], frames[1][1]).all()
