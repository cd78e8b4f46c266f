"""The temporal denoiser (fyprt_denoise_temporal / _device / _reset) on the GPU against the numpy restatement of its contract
(tests/temporal_ref.py), fed with the context's own accumulation, payload, albedo, frame index and the cameras' matrices.  "Equal" is
bitwise (NaN-aware) on every pixel of radiance4, rgba8 and FYPRT_BUF_TEMPORAL: call sequences over scenes x techniques under a static and
a moving camera, with the reference chained on its own history and re-seeded from the device's; a parameter sweep; sizes off the tile;
what drops the history and what does not; no frame state moves; the torch path; the 1M-triangle hall at 1920 x 1080; quality."""
import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import assert_numpy_keeps_subnormals, denoise_ref
from fypraytracer_amd import capi, scenes
from temporal_ref import DEFAULTS, camera_matrix, temporal_ref

pytestmark = pytest.mark.gpu
F = np.float32
# tests/test_gpu_moving_camera.py's MOVES: (keys held, mouse delta in pixels) per frame
MOVES = [("", (0.0, 0.0)), ("W", (60.0, -25.0)), ("DE", (-140.0, 40.0)), ("S", (90.0, 70.0)), ("AQ", (-35.0, -110.0)), ("W", (20.0, 10.0))]


def _context(scene_name, W, H, sc=None):
    mk_scene, mk_cam = SCENES[scene_name]
    sc = sc if sc is not None else mk_scene()
    cam = mk_cam(W, H)
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(sc)
    ctx.set_camera(cam)
    return ctx, sc, cam


class Ref:
    """What the reference needs from one call to the next: the history record and the matrix of the frame denoised last."""
    def __init__(self):
        self.hist, self.M = None, None

    def reset(self):
        self.hist = None


def _frame(ctx, st, seed, cam=None, move=None):
    """Renders one frame (after an optional camera move: on_update before the frame, commit_frame after); returns the frame index it was
    rendered with and projection x view of its camera."""
    if move is not None:
        cam.on_update(0.05, *move)
    if cam is not None:
        ctx.set_camera(cam)
    n = ctx.frame_index
    st.rand_seed = seed
    ctx.render(st)
    M = camera_matrix(cam) if cam is not None else None
    if move is not None:
        cam.commit_frame()
    return n, M


def _same(what, got, want):
    rad, img, rec = got
    want_rad, want_img, want_rec = want
    eq = bits_equal(rad, want_rad)
    assert eq.all(), f"{what}: {(~eq).sum()} of {eq.size} radiance values differ, first at {np.argwhere(~eq)[:3].tolist()}"
    assert (img == want_img).all(), f"{what}: {(img != want_img).sum()} packed pixels differ"
    for name in rec.dtype.names:
        eq = bits_equal(rec[name], want_rec[name])
        assert eq.all(), f"{what}: history field {name}: {(~eq).sum()} of {eq.size} values differ, first at {np.argwhere(~eq)[:3].tolist()}"


def _call(ctx, n, M, refs, what="", **kw):
    """One fyprt_denoise_temporal call with parameters kw on the frame rendered last (frame index n, camera matrix M), compared with
    temporal_ref continued from every state in `refs`: (Ref, reseed) pairs — after the call a re-seeded state takes the device's history
    record, a chained one keeps the reference's own."""
    H, W = ctx.height, ctx.width
    par = dict(DEFAULTS)
    par.update(kw)
    img, rad = ctx.denoise_temporal(capi.TemporalParams(**par))
    acc = ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)
    pay = ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    alb = ctx.read_buffer(capi.BUF_ALBEDO).reshape(H, W, 4)
    rec = ctx.read_buffer(capi.BUF_TEMPORAL).reshape(H, W)
    for ref, reseed in refs:
        want = temporal_ref(acc, pay, alb, n, ref.M, ref.hist, **par)
        _same(f"{what} {'re-seeded' if reseed else 'chained'} {kw}", (rad, img, rec), want)
        ref.hist, ref.M = (rec if reseed else want[2]), M
    return img, rad, rec


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("tech", [capi.COSINE_WEIGHTED_SAMPLING, capi.NEE, capi.RESTIR_DI, capi.RESTIR_GI])
@pytest.mark.parametrize("scene_name", ["cornell", "hall_small", "banana"])
def test_sequences_equal_the_contract(scene_name, tech, moving):
    """Six calls, one per frame, defaults, 96 x 64.  Static camera: accumulating frames (the divisor n grows); moving camera: MOVES with
    to_accumulate = 0.  The reference runs twice beside the device: chained on its own history, and re-seeded from the device's record
    after every call, so that a mismatch is pinned to the call that made it."""
    assert_numpy_keeps_subnormals()
    ctx, _, cam = _context(scene_name, 96, 64)
    st = settings_for(tech)
    st.to_accumulate = 0 if moving else 1
    refs = [(Ref(), False), (Ref(), True)]
    full = []
    for f in range(6):
        n, M = _frame(ctx, st, f + 1, cam, MOVES[f] if moving else None)
        _, rad, rec = _call(ctx, n, M, refs, f"{scene_name} tech {tech} {'moving' if moving else 'static'} call {f + 1}")
        flt = rec["filterable"] != 0
        assert flt.any()
        full.append(float((rec["N"][flt] == f + 1).mean()))
    print(f"{scene_name} tech {tech} {'moving' if moving else 'static'}: share of filterable pixels with N == call number {full}")
    if moving:
        if scene_name != "banana":                                      # (the two scenes whose shares the CPU test bounds)
            assert min(full[1:]) < 1.0 and max(full[1:]) > 0.5, full    # some history rejected, some reused
    else:
        assert full == [1.0] * 6, full                                  # pixel i reprojects onto pixel i
    ctx.close()


def test_parameter_sweep_over_a_moving_sequence():
    """hall_small 96 x 64, ReSTIR DI, MOVES with to_accumulate = 0; ten calls on every frame, each with other parameters (a call on a frame
    that was denoised before reprojects onto itself and lengthens the history), re-seeded from the device's record."""
    assert_numpy_keeps_subnormals()
    sweep = [dict(iterations=it, sigma_luminance=sl, normal_power_log2=npl) for it in (0, 1, 2, 3, 4, 5, 6, 8) for sl in (0.0, 1.0, 16.0)
             for npl in (0, 7)]
    sweep += [dict(demodulate_albedo=0), dict(demodulate_albedo=0, iterations=0), dict(history_limit=1), dict(history_limit=2),
              dict(history_limit=32, feedback=0), dict(normal_min=0.0), dict(normal_min=0.999), dict(plane_max=1e-4), dict(plane_max=10.0),
              dict(feedback=0, iterations=1), dict(feedback=1, iterations=1), dict(sigma_luminance=-1.0, sigma_plane=0.5)]
    ctx, _, cam = _context("hall_small", 96, 64)
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    refs = [(Ref(), True)]
    per_frame = (len(sweep) + 5) // 6
    for f in range(6):
        n, M = _frame(ctx, st, f + 1, cam, MOVES[f])
        for kw in sweep[f * per_frame:(f + 1) * per_frame]:
            _call(ctx, n, M, refs, f"sweep frame {f + 1}", **kw)
    ctx.close()


@pytest.mark.parametrize("size", [(97, 61), (24, 20), (16, 16), (33, 5)])
def test_sizes_off_the_tile(size):
    ctx, _, cam = _context("cornell", *size)
    st = settings_for(capi.NEE)
    st.to_accumulate = 0
    refs = [(Ref(), False), (Ref(), True)]
    for f, it in enumerate((0, 1, 3, 6, 5, 2)):
        n, M = _frame(ctx, st, f + 1, cam, MOVES[f])
        _call(ctx, n, M, refs, f"cornell {size} call {f + 1}", iterations=it)
    ctx.close()


def test_identity_configuration_and_history_limit_one():
    """The two settings that hold by construction: a first call with iterations = 0, demodulate_albedo = 0 returns the frame's own image;
    history_limit = 1 makes every call a first call."""
    ctx, _, cam = _context("cornell", 97, 61)
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    for f in range(3):
        _frame(ctx, st, f + 1, cam, MOVES[f])
        ctx.denoise_temporal_reset()
        img, rad = ctx.denoise_temporal(capi.TemporalParams(iterations=0, demodulate_albedo=0))
        frame_img, acc = ctx.readback()
        assert (img == frame_img).all() and bits_equal(rad, acc / F(1)).all()
        only_img, none = ctx.denoise_temporal(capi.TemporalParams(iterations=0, demodulate_albedo=0, history_limit=1), want_radiance=False)
        assert none is None and (only_img == frame_img).all()
    ctx.denoise_temporal_reset()
    first = ctx.denoise_temporal()
    rec_first = ctx.read_buffer(capi.BUF_TEMPORAL)
    ctx.denoise_temporal()                                             # builds a history of the same frame ...
    again = ctx.denoise_temporal(capi.TemporalParams(history_limit=1))    # ... that a limit of 1 does not blend in
    assert (again[0] == first[0]).all() and bits_equal(again[1], first[1]).all()
    assert struct_equal(ctx.read_buffer(capi.BUF_TEMPORAL), rec_first).all()
    ctx.close()


def test_what_drops_the_history_and_what_does_not():
    """Each of the five history-dropping calls makes the next call equal a first call; fyprt_denoise between two temporal calls changes
    neither; a fyprt_set_camera between frame and call changes nothing; after skipped frames a call reprojects with the camera of the last
    denoised frame."""
    W, H = 96, 64
    sc = SCENES["cornell"][0]()
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    ctx, _, cam = _context("cornell", W, H, sc)
    ctx.set_object_vertices(sc)
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise_temporal()                                         # no frame yet
    with pytest.raises(capi.FyprtError, match="FYPRT_BUF_TEMPORAL"):
        ctx.read_buffer(capi.BUF_TEMPORAL)                            # ... and no record
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    ref = Ref()
    refs = [(ref, False)]
    seed = [0]

    cams = [cam]

    def frame(move):
        seed[0] += 1
        return _frame(ctx, st, seed[0], cams[0], move)

    def two_calls(what):
        """frame, call (a first call for the reference), frame, call (one with a history); from the scene's own camera pose, so that
        the moves of the whole test do not add up to a walk out of the box"""
        cams[0] = SCENES["cornell"][1](W, H)
        _, _, rec = _call(ctx, *frame(MOVES[1]), refs, what + ": first")
        assert (rec["N"] <= 1).all()
        _, _, rec = _call(ctx, *frame(MOVES[5]), refs, what + ": second")
        assert (rec["N"] == 2).any()

    two_calls("start")
    ctx.denoise_temporal_reset()                                       # 1: the explicit reset — the frame stays valid
    ref.reset()
    with pytest.raises(capi.FyprtError, match="FYPRT_BUF_TEMPORAL"):
        ctx.read_buffer(capi.BUF_TEMPORAL)
    _, _, rec = _call(ctx, ctx.frame_index, ref.M, refs, "after reset, same frame")
    assert (rec["N"] <= 1).all()
    _, _, rec = _call(ctx, *frame(MOVES[5]), refs, "after reset, next frame")     # ... and that call left a history again
    assert (rec["N"] == 2).any()
    ctx.update_vertices(sc)                                            # 2: a geometry update (also invalidates the frame)
    ref.reset()
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        ctx.denoise_temporal()
    two_calls("after update_vertices")
    mgr.set_mesh_transform(sc, 5 % len(sc.meshes), pos=(0.2, 0.0, 0.1), rotation=(0, 30, 0))
    mgr.perform_all_scene_updates(sc)
    ctx.update_transforms(sc, [5 % len(sc.meshes)])                    # 3: a transform edit
    ref.reset()
    two_calls("after update_transforms")
    ctx.upload_scene(sc)                                               # 4: a scene upload
    ref.reset()
    two_calls("after upload_scene")
    ctx.resize(40, 24)                                                 # 5: a resize (drops the buffers too)
    ref.reset()
    cam_small = SCENES["cornell"][1](40, 24)
    with pytest.raises(capi.FyprtError, match="FYPRT_BUF_TEMPORAL"):
        ctx.read_buffer(capi.BUF_TEMPORAL)
    for k in range(2):
        n, M = _frame(ctx, st, 50 + k, cam_small, MOVES[1 + k])
        _call(ctx, n, M, refs, f"after resize, call {k + 1}")
    ctx.resize(W, H)
    ref.reset()
    two_calls("back at the first size")
    # fyprt_denoise between two temporal calls: its own result is the spatial contract's, and the temporal sequence goes on as without it
    n, M = frame(MOVES[2])
    acc = ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)
    pay = ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W)
    img_s, rad_s = ctx.denoise(capi.DenoiseParams(iterations=3))
    alb = ctx.read_buffer(capi.BUF_ALBEDO).reshape(H, W, 4)
    want_rad, want_img = denoise_ref(acc, pay, alb, n, iterations=3)
    assert bits_equal(rad_s, want_rad).all() and (img_s == want_img).all()
    _call(ctx, n, M, refs, "after a spatial call")
    img_s2, rad_s2 = ctx.denoise(capi.DenoiseParams(iterations=3))
    assert bits_equal(rad_s2, want_rad).all() and (img_s2 == want_img).all()
    # a fyprt_set_camera between the frame and the call changes nothing: the frame's own camera counts, now and for the next call
    n, M = frame(MOVES[3])
    other = SCENES["cornell"][1](W, H)
    other.on_update(0.05, "S", (300.0, 200.0))
    ctx.set_camera(other)
    _call(ctx, n, M, refs, "camera set after the frame")
    _call(ctx, *frame(MOVES[4]), refs, "the call after it")
    # skipped frames: two frames, one call — it reprojects with the camera of the last denoised frame, not of the last frame
    frame(MOVES[1])
    _, _, rec = _call(ctx, *frame(MOVES[2]), refs, "one call after two frames")
    assert (rec["N"] >= 2).any()
    # a band or stripes: refused as by fyprt_denoise, and the history survives the refusal
    ctx.set_rows(0, 32)
    with pytest.raises(capi.FyprtError, match="every row"):
        ctx.denoise_temporal()
    ctx.set_rows(0, H)
    _call(ctx, *frame(MOVES[5]), refs, "whole frame again")
    ctx.close()


def _state(ctx):
    ctx.synchronize()
    return [ctx.read_buffer(b) for b in range(10)], ctx.frame_index, ctx.frame_timings()


def _same_state(a, b, timings=True):
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        eq = struct_equal(x, y) if x.dtype.names else bits_equal(x, y)
        assert eq.all(), f"buffer {k} differs"
    assert a[1] == b[1]
    if timings:
        assert a[2] == b[2]


@pytest.mark.parametrize("tech", [capi.COSINE_WEIGHTED_SAMPLING, capi.RESTIR_DI, capi.RESTIR_GI])
def test_no_frame_state_moves(tech):
    """Every FYPRT_BUF_* of the frame (the albedo guide of that frame among them), the frame index and the frame timings are equal before
    and after temporal calls."""
    ctx, _, _ = _context("hall_small", 96, 64)
    st = settings_for(tech)
    for f in range(2):
        st.rand_seed = f + 1
        ctx.render(st)
    ctx.denoise()                                                      # (writes FYPRT_BUF_ALBEDO, so that it can be read before)
    before = _state(ctx)
    ctx.denoise_temporal()
    ctx.denoise_temporal(capi.TemporalParams(iterations=2, demodulate_albedo=0, feedback=0))
    _same_state(before, _state(ctx))
    ctx.close()


@pytest.mark.parametrize("use_async", [False, True])
@pytest.mark.parametrize("tech", [capi.RESTIR_DI, capi.RESTIR_GI])
def test_frames_after_temporal_calls_are_the_frames_without_them(tech, use_async):
    """frame, call, frame, call, frame leaves the buffers of frame, frame, frame (ReSTIR DI pipelined over two streams, key 11 = 1)."""
    results = []
    for with_calls in (True, False):
        ctx, _, cam = _context("hall_small", 96, 64)
        ctx.set_tuning(11, 1)
        st = settings_for(tech)
        refs = [(Ref(), False)]
        M = camera_matrix(cam)
        for f in range(3):
            st.rand_seed = f + 1
            if use_async:
                ctx.render_async(st)
            else:
                ctx.render(st)
            if with_calls and f < 2:
                _call(ctx, f + 1, M, refs, f"tech {tech} async {use_async} frame {f + 1}", iterations=3)
        ctx.denoise()
        results.append(_state(ctx))
        ctx.close()
    _same_state(results[0], results[1], timings=False)


def test_quality_on_the_device():
    """Sanity bound, not a quality bar: hall_small 160 x 96, ReSTIR DI with both reuses, to_accumulate = 0, static camera, defaults: the
    MSE (linear radiance) of temporal call 8 against the context's own 256-frame accumulation is no larger than that of fyprt_denoise on the
    same frame 8.  (Both results are dominated by the filter's bias on this scene, which is why the bar is 1 and not 1/2.)"""
    W, H = 160, 96
    ctx, _, _ = _context("hall_small", W, H)
    st = settings_for(capi.RESTIR_DI, sky_color=(0.0, 0.0, 0.0), sample_count=1)
    st.to_accumulate = 0
    for f in range(8):
        st.rand_seed = f + 1
        ctx.render(st)
        tem = ctx.denoise_temporal()[1][..., :3].astype(np.float64)
    spa = ctx.denoise()[1][..., :3].astype(np.float64)
    raw = ctx.readback()[1][..., :3].astype(np.float64)
    N = ctx.read_buffer(capi.BUF_TEMPORAL)["N"]
    assert N.max() == 8
    st.to_accumulate = 1
    ctx.reset_frame_index()
    for f in range(256):
        st.rand_seed = 1000 + f
        ctx.render(st)
    ref = (ctx.readback()[1][..., :3] / F(256)).astype(np.float64)
    ctx.close()
    mse_raw, mse_spa, mse_tem = (float(np.mean((x - ref) ** 2)) for x in (raw, spa, tem))
    print(f"hall_small ReSTIR DI frame 8: MSE raw {mse_raw:.6g}, spatial {mse_spa:.6g}, temporal {mse_tem:.6g} (temporal / spatial {mse_tem / mse_spa:.3f})")
    assert mse_spa > 0 and mse_tem <= mse_spa


def test_hall_1m_triangles_1080p():
    """The bench workload: ReSTIR DI, two frames with a small camera move, two iterations.  Two contexts give identical bits.  Rows
    500..563 of both calls equal temporal_ref run on rows 484..579: two iterations reach 2 * 3 = 6 rows, their variance prefilters 2 more,
    the spatial variance estimate under them 2 — 10 rows, the margin is 16 (numpy on the full frame is too slow).  The reference's second
    call is given the device's whole history record of the first, so every reprojection tap of the compared rows lies inside the rows numpy
    has, whatever the camera move (temporal_ref asserts it)."""
    W, H = 1920, 1080
    par = dict(DEFAULTS, iterations=2)
    runs = []
    sc = scenes.hall_scene()
    for _ in range(2):
        ctx = capi.Context(0)
        ctx.resize(W, H)
        ctx.upload_scene(sc)
        cam = scenes.hall_camera(W, H)
        st = settings_for(capi.RESTIR_DI)
        st.to_accumulate = 0
        out = []
        for f, move in enumerate((None, ("W", (20.0, 10.0)))):
            n, M = _frame(ctx, st, f + 1, cam, move)
            img, rad = ctx.denoise_temporal(capi.TemporalParams(**par))
            out.append(dict(n=n, M=M, img=img, rad=rad, acc=ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4),
                            pay=ctx.read_buffer(capi.BUF_PAYLOAD).reshape(H, W), alb=ctx.read_buffer(capi.BUF_ALBEDO).reshape(H, W, 4),
                            rec=ctx.read_buffer(capi.BUF_TEMPORAL).reshape(H, W)))
        ctx.close()
        runs.append(out)
    for a, b in zip(*runs):
        assert (a["img"] == b["img"]).all() and bits_equal(a["rad"], b["rad"]).all() and struct_equal(a["rec"].ravel(), b["rec"].ravel()).all()
    y0, y1, m = 500, 564, 16
    rows = slice(y0 - m, y1 + m)
    hist, M = None, None
    for k, o in enumerate(runs[0]):
        want = temporal_ref(o["acc"][rows], o["pay"][rows], o["alb"][rows], o["n"], M, hist, row0=y0 - m, full_height=H, **par)
        _same(f"1080p call {k + 1}", (o["rad"][y0:y1], o["img"][y0:y1], o["rec"][y0:y1]), tuple(w[m:-m] for w in want))
        hist, M = o["rec"], o["M"]
    rec = runs[0][1]["rec"][y0:y1]
    flt = rec["filterable"] != 0
    assert flt.mean() > 0.5 and (rec["N"][flt] == 2).any() and (runs[0][1]["rad"][y0:y1, :, :3] != runs[0][1]["acc"][y0:y1, :, :3]).any()


def test_torch_path_is_ordered_and_equals_the_host_entry():
    """In a fresh process that initialises torch's CUDA before the library is loaded (tests/test_gpu_query.py explains why)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_temporal as t; "
            "t._torch_checks(); print('torch path ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_checks():
    import torch
    W, H = 96, 64
    par = capi.TemporalParams(iterations=4, sigma_luminance=2.0)
    # the device entry between asynchronous, pipelined ReSTIR DI frames, never synchronised by the host: equals the host entry after
    # each frame of a blocking sequence, history record included, and the frames are the frames without the calls
    ctx, _, _ = _context("hall_small", W, H)
    ctx.set_tuning(11, 1)
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    outs = []
    for f in range(4):
        st.rand_seed = f + 1
        ctx.render_async(st)
        img_t = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
        rad_t = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
        big = torch.randn(2048, 2048, device="cuda:0") @ torch.randn(2048, 2048, device="cuda:0")
        if f == 3:
            ctx.denoise_temporal_tensor(None, rad_t, par)              # one output alone
        else:
            ctx.denoise_temporal_tensor(img_t, rad_t, par)
        outs.append((img_t, rad_t * 1.0))
        del big
    async_rec = ctx.read_buffer(capi.BUF_TEMPORAL)
    async_state = _state(ctx)
    ref, _, _ = _context("hall_small", W, H)
    ref.set_tuning(11, 1)
    for f in range(4):
        st.rand_seed = f + 1
        ref.render(st)
        img, rad = ref.denoise_temporal(par)
        if f < 3:
            assert (outs[f][0].cpu().numpy().view(np.uint32) == img).all(), f
        assert bits_equal(outs[f][1].cpu().numpy(), rad).all(), f
    assert struct_equal(async_rec, ref.read_buffer(capi.BUF_TEMPORAL)).all()
    assert (ref.read_buffer(capi.BUF_TEMPORAL)["N"] == 4).any()
    _same_state(async_state, _state(ref), timings=False)
    plain, _, _ = _context("hall_small", W, H)
    plain.set_tuning(11, 1)
    for f in range(4):
        st.rand_seed = f + 1
        plain.render_async(st)
    plain.denoise_temporal(par)                                        # (FYPRT_BUF_ALBEDO of the last frame, so that _state can read it)
    _same_state(async_state, _state(plain), timings=False)
    with pytest.raises(ValueError):
        ctx.denoise_temporal_tensor(torch.empty((H, W), dtype=torch.float32, device="cuda:0"), None)
    for c in (ctx, ref, plain):
        c.close()
