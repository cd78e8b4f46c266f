"""fyprt_group_denoise_upscale / _device: the guided upscaler on the row bands of a group.  The contract is fyprt_denoise_upscale's steps 1
to 3 on the stitched frame with the low-res stage replaced by the group's, so every comparison is bitwise (NaN-aware) on radiance and
packed image: against upscale_ref (tests/upscale_ref.py) fed with the bands' low-res buffers and hi-res records stitched together, and
against Context.denoise_upscale of a single context rendering the same sequence.  Frame and band tables: tests/group_upscale_ref.py
(tests/test_group_upscale_cpu.py confirms on oracle frames that they are no vacuous case; the device's frames are asserted here again).
The box has one GPU: the contexts share device 0, as in tests/test_gpu_group.py."""
import ctypes as C
import gc

import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import assert_numpy_keeps_subnormals
from fypraytracer_amd import capi
from group_temporal_ref import group_temporal_ref, rows_needed
from group_upscale_ref import FIVE, H, MOVES, SCENE, TWO, W, assert_border_rows_matter
from temporal_ref import DEFAULTS as T_DEFAULTS, camera_matrix
from test_gpu_group_temporal import Rig
from upscale_ref import SPATIAL_KEYS, _predemodulated, lowres_colour, upscale_ref

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
F = np.float32
S_DEFAULTS = {k: T_DEFAULTS[k] for k in SPATIAL_KEYS}
RESTIR = (capi.RESTIR_DI, capi.RESTIR_GI)
U = capi.UpscaleParams


def _halo_mode(tech):
    return 1 if tech in RESTIR else 0


def _eq(x, y):
    return struct_equal(x.reshape(-1), y.reshape(-1)) if x.dtype.names else bits_equal(x, y)


def _same(what, rad, img, want_rad, want_img):
    if rad is not None:
        eq = bits_equal(rad, want_rad)
        assert eq.all(), f"{what}: {(~eq).sum()} of {eq.size} radiance values differ, rows {sorted(set(np.argwhere(~eq)[:, 0].tolist()))[:12]}"
    if img is not None:
        assert (img == want_img).all(), f"{what}: {(img != want_img).sum()} packed pixels differ"


def _hires(ctx, s):
    return (ctx.read_buffer(capi.BUF_UPSCALE_GUIDE).reshape(ctx.height * s, ctx.width * s),
            ctx.read_buffer(capi.BUF_UPSCALE_ALBEDO).reshape(ctx.height * s, ctx.width * s, 4))


def _hires_stitched(rig, s):
    """The two hi-res buffers of the frame: every band's hi-res rows [s b, s e) from the context that owns them."""
    out = None
    for c, b, e in zip(rig.ctxs, rig.bounds, rig.bounds[1:]):
        bufs = _hires(c, s)
        if out is None:
            out = tuple(np.zeros_like(x) for x in bufs)
        for o, x in zip(out, bufs):
            o[s * b:s * e] = x[s * b:s * e]
    return out


def _lowres_stitched(rig):
    return tuple(rig.stitched(b) for b in (capi.BUF_ACCUM, capi.BUF_PAYLOAD, capi.BUF_ALBEDO))


def _contract(rig, n, s, par):
    """upscale_ref on the stitched frame for a spatial call with parameters par: (radiance, image, branch map, and its inputs)."""
    acc, pay, alb = _lowres_stitched(rig)
    g, a_hi = _hires_stitched(rig, s)
    e = lowres_colour(acc, pay, alb, n, **par)
    return upscale_ref(e, pay, alb, acc, n, g, a_hi, s, **par), (e, pay, alb, acc, n, g, a_hi)


def _check(rig, n, s, what="", vacuity=False, **kw):
    """Group.denoise_upscale (temporal = 0) == the contract; returns (image, radiance)."""
    par = dict(S_DEFAULTS)
    par.update(kw)
    img, rad = rig.grp.denoise_upscale(U(scale=s, **par))
    assert img.shape == (rig.H * s, rig.W * s) and rad.shape == img.shape + (4,)
    want, inputs = _contract(rig, n, s, par)
    _same(f"{what} bands {rig.bounds} scale {s} {kw} against the contract", rad, img, want[0], want[1])
    if vacuity:
        assert_border_rows_matter(*inputs, s, rig.bounds, want=want, **par)
    return img, rad


def _single_context():
    mk_scene, mk_cam = SCENES[SCENE]
    ctx = capi.Context(0)
    ctx.resize(W, H)
    ctx.upload_scene(mk_scene())
    ctx.set_camera(mk_cam(W, H))
    return ctx


# ------------------------------------------------------------------------------------------------ 1. the contract and the single context
_single_cache = {}


def _single(tech):
    """Context.denoise_upscale (defaults) at scales 2, 3, 4 after frames 1 and 4 of a single context: {(frame, s): (radiance, image,
    hi-res guide, hi-res albedo)} and {frame: accumulation}.  Computed once per technique."""
    if tech not in _single_cache:
        ctx = _single_context()
        st = settings_for(tech)
        outs, accs = {}, {}
        for f in range(1, 5):
            st.rand_seed = f
            ctx.render(st)
            if f in (1, 4):
                accs[f] = ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)
                for s in (2, 3, 4):
                    img, rad = ctx.denoise_upscale(U(scale=s))
                    outs[(f, s)] = (rad, img) + _hires(ctx, s)
        ctx.close()
        _single_cache[tech] = outs, accs
    return _single_cache[tech]


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("bounds", [TWO, FIVE], ids=["two", "five"])
@pytest.mark.parametrize("tech", [capi.RESTIR_DI, capi.NEE, capi.COSINE_WEIGHTED_SAMPLING])
def test_equals_the_contract_and_the_single_context(tech, bounds, s):
    """Frame 1 and frame 4 of an accumulation, defaults.  Both outputs equal upscale_ref on the stitched buffers and the single context's
    call; every member's hi-res records equal the single context's in the member's own hi-res rows; and the frame is no vacuous case."""
    assert_numpy_keeps_subnormals()
    outs, accs = _single(tech)
    rig = Rig(SCENE, W, H, bounds, _halo_mode(tech))
    st = settings_for(tech)
    for f in range(1, 5):
        n, _ = rig.frame(st)
        if f not in (1, 4):
            continue
        assert n == f
        img, rad = _check(rig, n, s, f"tech {tech} frame {f}", vacuity=True)
        assert bits_equal(rig.stitched(capi.BUF_ACCUM), accs[f]).all()       # the group's frame is the single context's
        want_rad, want_img, want_g, want_a = outs[(f, s)]
        _same(f"tech {tech} bands {bounds} scale {s} frame {f} against the single context", rad, img, want_rad, want_img)
        for c, b, e in zip(rig.ctxs, bounds, bounds[1:]):
            g, a_hi = _hires(c, s)
            assert _eq(g[s * b:s * e], want_g[s * b:s * e]).all() and bits_equal(a_hi[s * b:s * e], want_a[s * b:s * e]).all(), f"hi-res records of band {b}..{e}"
    rig.close()


# ------------------------------------------------------------------------------------------------ 2. which buffer is pulled
@pytest.fixture(scope="module")
def di_five():
    """One ReSTIR DI frame on FIVE, and the single context holding the same frame."""
    rig = Rig(SCENE, W, H, FIVE, 1)
    ctx = _single_context()
    st = settings_for(capi.RESTIR_DI)
    n, _ = rig.frame(st)
    st.rand_seed = 1
    ctx.render(st)
    assert bits_equal(rig.stitched(capi.BUF_ACCUM), ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)).all()
    yield rig, ctx, n
    rig.close()
    ctx.close()


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [0, 1, 2, 5])
def test_which_buffer_is_pulled(di_five, iterations, demodulate):
    """Without an iteration e is the prepared colour (dn.col[0], and the guide record of the row travels with it: the spatial plan has no
    stage 0 then); after an odd number of iterations it is dn.col[1], after an even number dn.col[0]."""
    rig, ctx, n = di_five
    s = 2 + (iterations + demodulate) % 3
    kw = dict(iterations=iterations, demodulate_albedo=demodulate)
    img, rad = _check(rig, n, s, "pulled buffer", vacuity=True, **kw)
    want_img, want_rad = ctx.denoise_upscale(U(scale=s, **dict(S_DEFAULTS, **kw)))
    _same(f"iterations {iterations} demodulate {demodulate} against the single context", rad, img, want_rad, want_img)
    d_img, d_rad = rig.grp.denoise(capi.DenoiseParams(**dict(S_DEFAULTS, **kw)))
    _same("out[::s, ::s] against Group.denoise", rad[::s, ::s], img[::s, ::s], d_rad, d_img)


# ------------------------------------------------------------------------------------------------ 3. the hi-res records
@pytest.mark.parametrize("s", [2, 3, 4])
def test_hires_records_of_every_member(di_five, s):
    rig, ctx, _ = di_five
    rig.grp.denoise_upscale(U(scale=s, iterations=1), want_radiance=False)
    ctx.denoise_upscale(U(scale=s, iterations=1), want_radiance=False)
    want_g, want_a = _hires(ctx, s)
    for c, b, e in zip(rig.ctxs, FIVE, FIVE[1:]):
        g, a_hi = _hires(c, s)
        assert g.shape == (H * s, W * s)
        assert _eq(g[s * b:s * e], want_g[s * b:s * e]).all() and bits_equal(a_hi[s * b:s * e], want_a[s * b:s * e]).all(), (b, e)


# ------------------------------------------------------------------------------------------------ 4. the temporal mode
def _moving_settings(tech):
    st = settings_for(tech, sample_count=1)
    st.to_accumulate = 0
    return st


@pytest.mark.parametrize("tech", [capi.RESTIR_DI, capi.NEE])
def test_temporal_mode_with_the_whole_history(tech):
    """The six-frame moving-camera sequence, one-sample frames, history_rows = height, scale cycling 2, 3, 4.  After every frame: the
    outputs equal the contract (upscale_ref on the e of group_temporal_ref, chained from the reference's own history); the stitched
    FYPRT_BUF_TEMPORAL equals what a twin group running Group.denoise_temporal leaves; out[::s, ::s] is that call's output; and outputs and
    history equal the single context's temporal upscale of the same sequence (the group's frame is the single context's on every one of
    these frames, which is asserted)."""
    assert_numpy_keeps_subnormals()
    par = dict(T_DEFAULTS)
    rig, twin = Rig(SCENE, W, H, FIVE, _halo_mode(tech)), Rig(SCENE, W, H, FIVE, _halo_mode(tech))
    one = _single_context()
    cam = SCENES[SCENE][1](W, H)
    st = _moving_settings(tech)
    hist, M_prev, compared = None, None, 0
    for f in range(6):
        s = 2 + f % 3
        n, M = rig.frame(st, MOVES[f])
        twin.frame(st, MOVES[f])
        cam.on_update(0.05, *MOVES[f])
        one.set_camera(cam)
        st.rand_seed = f + 1
        one.render(st)
        cam.commit_frame()
        img, rad = rig.grp.denoise_upscale(U(scale=s, temporal=1, **par), history_rows=H)
        t_img, t_rad = twin.grp.denoise_temporal(capi.TemporalParams(**par), history_rows=H)
        o_img, o_rad = one.denoise_upscale(U(scale=s, temporal=1, **par))
        rec = rig.stitched(capi.BUF_TEMPORAL)
        assert _eq(rec, twin.stitched(capi.BUF_TEMPORAL)).all(), f"frame {f + 1}: the history differs from the twin group's"
        _same(f"frame {f + 1}: out[::s, ::s] against Group.denoise_temporal", rad[::s, ::s], img[::s, ::s], t_rad, t_img)
        acc, pay, alb = _lowres_stitched(rig)
        g, a_hi = _hires_stitched(rig, s)
        e, _, new = group_temporal_ref(_predemodulated(acc, alb, n, 1), pay, alb, 1, M_prev, hist, FIVE, H, **dict(par, demodulate_albedo=0))
        assert _eq(new, rec).all(), f"frame {f + 1}: the history differs from the contract's"
        want_rad, want_img, _ = upscale_ref(e[..., :3], pay, alb, acc, n, g, a_hi, s, **par)
        _same(f"tech {tech} frame {f + 1} scale {s} against the contract", rad, img, want_rad, want_img)
        if bits_equal(acc, one.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)).all():
            compared += 1
        _same(f"tech {tech} frame {f + 1} scale {s} against the single context", rad, img, o_rad, o_img)
        assert _eq(rec, one.read_buffer(capi.BUF_TEMPORAL).reshape(H, W)).all(), f"frame {f + 1}: the history differs from the single context's"
        hist, M_prev = new, M
    print(f"tech {tech}: {compared} of 6 frames compared with the single context")
    assert compared == 6, compared
    assert (hist["N"] > 2).any()
    for r in (rig, twin):
        r.close()
    one.close()


@pytest.mark.parametrize("R", [4, 0])
def test_temporal_mode_under_a_window(R):
    """history_rows 4 and 0 on FIVE: the outputs equal upscale_ref on the e of group_temporal_ref (predemodulated input, n = 1, demodulate
    0, as lowres_colour_temporal does it), continued from the device's stitched record; at 4 rows at least one reprojection leaves its
    window."""
    assert_numpy_keeps_subnormals()
    par = dict(T_DEFAULTS)
    rig = Rig(SCENE, W, H, FIVE, 1)
    st = _moving_settings(capi.RESTIR_DI)
    hist, M_prev, reach = None, None, 0
    for f in range(6):
        s = 2 + f % 3
        n, M = rig.frame(st, MOVES[f])
        img, rad = rig.grp.denoise_upscale(U(scale=s, temporal=1, **par), history_rows=R)
        acc, pay, alb = _lowres_stitched(rig)
        g, a_hi = _hires_stitched(rig, s)
        rec = rig.stitched(capi.BUF_TEMPORAL)
        e, _, new = group_temporal_ref(_predemodulated(acc, alb, n, 1), pay, alb, 1, M_prev, hist, FIVE, R, **dict(par, demodulate_albedo=0))
        assert _eq(new, rec).all(), f"frame {f + 1}: the history differs from the contract's"
        want_rad, want_img, _ = upscale_ref(e[..., :3], pay, alb, acc, n, g, a_hi, s, **par)
        _same(f"R = {R} frame {f + 1} scale {s} against the contract", rad, img, want_rad, want_img)
        if M_prev is not None:
            reach = max(reach, int(rows_needed(pay, alb, M_prev, FIVE).max()))
        hist, M_prev = rec, M
    assert reach > 4, reach                                              # a window of 4 rows (and of none) really cut a reprojection
    rig.close()


def test_temporal_mode_with_object_motion():
    """Motion on for every member, mesh 7 dragged before every frame (tests/test_gpu_group_temporal.py), three bands, history_rows =
    height: call for call the single context's temporal upscale with motion on; every member consumes its snapshot."""
    w, h, bounds, s = 96, 64, [0, 20, 41, 64], 3
    drag = ((0.02, 0.0, -0.015), (0.0, 1.5, 0.0), (0.0, 0.0, 0.0))
    sc = SCENES[SCENE][0]()
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    rig = Rig(SCENE, w, h, bounds, 0, sc=sc)
    one = capi.Context(0)
    one.resize(w, h)
    one.upload_scene(sc)
    cam = SCENES[SCENE][1](w, h)
    for c in rig.ctxs + [one]:
        c.set_object_vertices(sc)
        c.denoise_temporal_set_motion(True)
    base = dict(sc.mesh_transforms[7])
    st = settings_for(capi.NEE)
    st.to_accumulate = 0
    for f in range(3):
        k = F(f + 1)
        mgr.set_mesh_transform(sc, 7, pos=tuple(F(x) + k * F(d) for x, d in zip(base["pos"], drag[0])),
                               rotation=tuple(F(x) + k * F(d) for x, d in zip(base["rotation"], drag[1])),
                               scale_=tuple(F(x) + k * F(d) for x, d in zip(base["scale"], drag[2])))
        mgr.perform_all_scene_updates(sc)
        for c in rig.ctxs + [one]:
            c.update_transforms(sc, [7])
        rig.seed = f
        rig.frame(st, MOVES[f])
        cam.on_update(0.05, *MOVES[f])
        one.set_camera(cam)
        st.rand_seed = f + 1
        one.render(st)
        cam.commit_frame()
        img, rad = rig.grp.denoise_upscale(U(scale=s, temporal=1), history_rows=h)
        want_img, want_rad = one.denoise_upscale(U(scale=s, temporal=1))
        _same(f"object motion call {f + 1}", rad, img, want_rad, want_img)
        rec = rig.stitched(capi.BUF_TEMPORAL)
        assert _eq(rec, one.read_buffer(capi.BUF_TEMPORAL).reshape(h, w)).all(), f"call {f + 1}: the histories differ"
    first, count, _ = sc.meshes[7]
    tri = rig.stitched(capi.BUF_PAYLOAD)["objectIndex"]
    on = (tri >= first) & (tri < first + count) & (rec["filterable"] != 0)
    assert on.any() and (rec["N"][on] == 3).any()                        # the dragged mesh kept its history through the edits
    rig.ctxs[1].denoise_temporal_set_motion(False)
    with pytest.raises(capi.FyprtError, match="motion mode"):
        rig.grp.denoise_upscale(U(scale=s, temporal=1))
    rig.grp.denoise_upscale(U(scale=s, temporal=0))                      # the spatial mode does not look at it
    rig.close()
    one.close()


# ------------------------------------------------------------------------------------------------ 5. the schedule (torch, device entry)
def test_roots_outputs_and_the_device_entry():
    """In a fresh process that initialises torch's CUDA before the library is loaded (tests/test_gpu_query.py explains why)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_group_upscale as t; "
            "t._torch_checks(); print('group upscale torch path ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "group upscale torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_checks():
    import torch
    par = dict(S_DEFAULTS, iterations=3)
    t_par = dict(T_DEFAULTS, iterations=3)
    st = settings_for(capi.RESTIR_DI)

    def tensors(s):
        return torch.empty((H * s, W * s), dtype=torch.int32, device="cuda:0"), torch.empty((H * s, W * s, 4), dtype=torch.float32, device="cuda:0")

    def host(t):
        return None if t is None else (t.cpu().numpy().view(np.uint32) if t.dtype == torch.int32 else t.cpu().numpy())

    rig = Rig(SCENE, W, H, FIVE, 1)
    n, _ = rig.frame(st)
    # what every call below must give: the blocking entry of a second group on the same frame, tied to the contract by _check
    ref = Rig(SCENE, W, H, FIVE, 1)
    ref.frame(st)
    want = {s: _check(ref, n, s, "blocking entry", **par) for s in (2, 3)}
    # two device calls back to back at scales 2 then 3, root 1 then root 0, no host wait between; then a Group.denoise and a
    # Group.denoise_temporal directly after them
    i2, r2 = tensors(2)
    i3, r3 = tensors(3)
    di, dr = tensors(1)
    ti, tr = tensors(1)
    rig.grp.denoise_upscale_tensor(i2, r2, U(scale=2, **par), root=1)
    rig.grp.denoise_upscale_tensor(i3, r3, U(scale=3, **par), root=0)
    rig.grp.denoise_tensor(di, dr, capi.DenoiseParams(**par), root=3)
    rig.grp.denoise_temporal_tensor(ti, tr, capi.TemporalParams(**t_par), history_rows=H, root=2)
    _same("device entry, scale 2, root 1", host(r2), host(i2), want[2][1], want[2][0])
    _same("device entry, scale 3, root 0", host(r3), host(i3), want[3][1], want[3][0])
    w_img, w_rad = ref.grp.denoise(capi.DenoiseParams(**par))
    _same("Group.denoise directly after", host(dr), host(di), w_rad, w_img)
    w_img, w_rad = ref.grp.denoise_temporal(capi.TemporalParams(**t_par), history_rows=H)
    _same("Group.denoise_temporal directly after", host(tr), host(ti), w_rad, w_img)
    # only the image, only the radiance, every root
    for root in range(5):
        s = 2 + root % 2
        img, _ = tensors(s)
        _, rad = tensors(s)
        rig.grp.denoise_upscale_tensor(img, None, U(scale=s, **par), root=root)
        rig.grp.denoise_upscale_tensor(None, rad, U(scale=s, **par), root=root)
        _same(f"root {root}, image only", None, host(img), None, want[s][0])
        _same(f"root {root}, radiance only", host(rad), None, want[s][1], None)
    # the temporal mode through the device entry: a second call on the frame denoised last, as the reference group makes it
    ti4, tr4 = tensors(4)
    rig.grp.denoise_upscale_tensor(ti4, tr4, U(scale=4, temporal=1, **t_par), history_rows=4, root=4)
    w_img, w_rad = ref.grp.denoise_upscale(U(scale=4, temporal=1, **t_par), history_rows=4)
    _same("temporal mode, device entry", host(tr4), host(ti4), w_rad, w_img)
    assert _eq(rig.stitched(capi.BUF_TEMPORAL), ref.stitched(capi.BUF_TEMPORAL)).all()
    # a call after set_rows moved every border
    moved = [0, 7, 22, 23, 50, 64]
    for r in (rig, ref):
        r.set_rows(moved)
        r.frame(st)
    i3, r3 = tensors(3)
    rig.grp.denoise_upscale_tensor(i3, r3, U(scale=3, **par), root=2)
    w_img, w_rad = _check(ref, n + 1, 3, "after set_rows", vacuity=True, **par)
    _same("device entry after set_rows", host(r3), host(i3), w_rad, w_img)
    with pytest.raises(ValueError):
        rig.grp.denoise_upscale_tensor(torch.empty((H, W), dtype=torch.int32, device="cuda:0"), None, U(scale=2))
    with pytest.raises(ValueError):
        rig.grp.denoise_upscale_tensor(i3, None, U(scale=3), root=5)
    with pytest.raises(ValueError):
        rig.grp.denoise_upscale_tensor(None, None)
    rig.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 6. no frame state moves
def _member_state(c):
    c.synchronize()
    return [c.read_buffer(b) for b in range(9)], c.frame_index


@pytest.mark.parametrize("tech", RESTIR)
def test_no_frame_state_moves_and_the_sequence_is_the_sequence_without_the_calls(tech):
    rig, plain = Rig(SCENE, W, H, TWO, 1), Rig(SCENE, W, H, TWO, 1)
    st = settings_for(tech)
    for f in range(5):
        rig.frame(st)
        plain.frame(st)
        before = [_member_state(c) for c in rig.ctxs]
        rig.grp.denoise_upscale(U(scale=2 + f % 3), want_radiance=False)
        rig.grp.denoise_upscale(U(scale=3, temporal=1, iterations=2, demodulate_albedo=0), history_rows=0)
        for (a, ia), (b, ib) in zip(before, [_member_state(c) for c in rig.ctxs]):
            for k, (x, y) in enumerate(zip(a, b)):
                assert _eq(x, y).all(), f"frame {f + 1}: buffer {k} moved"
            assert ia == ib
        for which in (capi.BUF_ACCUM, capi.BUF_IMAGE, capi.BUF_PAYLOAD):
            assert _eq(rig.stitched(which), plain.stitched(which)).all(), f"frame {f + 1}: buffer {which} differs from the sequence without calls"
    for c, p in zip(rig.ctxs, plain.ctxs):                                # reservoirs and every other frame buffer, member by member
        for k, (x, y) in enumerate(zip(_member_state(c)[0], _member_state(p)[0])):
            assert _eq(x, y).all(), f"buffer {k} of a member differs from the sequence without calls"
    rig.close()
    plain.close()


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors_in_the_documented_order():
    w, h, bounds = 48, 64, [0, 20, 64]
    gc.collect()
    rig = Rig("cornell", w, h, bounds, 0)
    grp, lib = rig.grp, rig.grp.lib
    ok = U()
    img = np.empty(4 * w * h, np.uint32)
    out = img.ctypes.data_as(C.c_void_p)
    dev = C.c_void_p(rig.ctxs[0].image_device_ptr())                     # a device address for the refused device calls (never written)
    live = capi.live_device_bytes()

    def rc(p=ok, rgba8=out, radiance4=None):
        return lib.fyprt_group_denoise_upscale(grp.h, C.byref(p) if p is not None else None, h, rgba8, radiance4, None)

    def rcd(p=ok, root=0, rgba8=dev, radiance4=None):
        return lib.fyprt_group_denoise_upscale_device(grp.h, C.byref(p), h, root, rgba8, radiance4)

    nan = float("nan")
    bad_temporal = [U(history_limit=0), U(history_limit=257), U(feedback=2), U(normal_min=nan), U(plane_max=0.0)]
    for have_frame in (False, True):                                     # before any frame, and with one: the argument errors come first
        assert rc(p=None) == EINVAL
        for p in (U(scale=1), U(scale=5), U(temporal=2), U(iterations=9), U(normal_power_log2=8), U(sigma_plane=0.0), U(sigma_luminance=nan)):
            assert rc(p=p) == EINVAL and rcd(p=p) == EINVAL and rcd(p=p, root=7) == EINVAL
        for p in bad_temporal:                                           # read only with temporal = 1, and then before the spatial part
            assert rc(p=p) == (0 if have_frame else ESTATE)
            p.temporal = 1
            assert rc(p=p) == EINVAL and rcd(p=p, root=7) == EINVAL
            p.temporal = 0
        assert rcd(root=2) == EINVAL and rcd(root=-1) == EINVAL
        assert rcd(rgba8=C.c_void_p(dev.value + 2)) == EINVAL           # misaligned
        assert rcd(rgba8=None, radiance4=C.c_void_p(dev.value + 4)) == EINVAL
        assert rc(rgba8=None) == EINVAL and rcd(rgba8=None) == EINVAL    # both outputs NULL
        if not have_frame:
            assert rc() == ESTATE and rcd() == ESTATE
            with pytest.raises(capi.FyprtError, match="no complete frame"):
                grp.denoise_upscale()
            assert capi.live_device_bytes() == live                      # a refused call allocates nothing
            rig.frame(settings_for(capi.NEE))
            rig.grp.synchronize()
            live = capi.live_device_bytes()
    # (the loop's second pass ran successful calls for the temporal parameters that are not read)
    used = capi.live_device_bytes()
    st = settings_for(capi.NEE)

    def refused(match, **kw):
        with pytest.raises(capi.FyprtError, match=match):
            grp.denoise_upscale(**kw)
        assert capi.live_device_bytes() == used

    def fresh_frame():
        for c in rig.ctxs:
            c.reset_frame_index()
            c.set_camera(rig.cam)
        rig.frame(st)

    rig.ctxs[1].render(st)                                               # one member a frame ahead
    refused("frame index")
    fresh_frame()
    rig.ctxs[0].set_rows(0, 10)                                          # a member re-banded behind the group
    refused("not its band")
    rig.ctxs[0].set_rows(0, 20)
    grp.denoise_upscale()
    used = capi.live_device_bytes()                                      # (the radiance staging came with this call)
    with pytest.raises(capi.FyprtError, match="every row"):
        rig.ctxs[0].denoise_upscale()                                    # a member on its own stays refused
    # members with different cameras: in the spatial mode the new case, in the temporal mode still before the camera-matrix case
    turned = SCENES["cornell"][1](w, h)
    turned.on_update(0.05, *MOVES[2])
    for c in rig.ctxs:
        c.reset_frame_index()
    rig.ctxs[1].set_camera(turned)
    grp.render(st)
    assert rc() == ESTATE
    refused("camera or sky")
    refused("camera or sky", params=U(temporal=1))
    # members with different sky colours
    fresh_frame()
    grp.denoise_upscale()
    for c in rig.ctxs:
        c.reset_frame_index()
    rig.ctxs[0].render(settings_for(capi.NEE, sky_color=(0.1, 0.2, 0.3)))
    rig.ctxs[1].render(settings_for(capi.NEE, sky_color=(0.1, 0.2, float(np.nextafter(F(0.3), F(1))))))      # one bit apart
    refused("camera or sky")
    # the temporal mode's own cases come after: the motion mode
    fresh_frame()
    rig.ctxs[0].denoise_temporal_set_motion(True)
    refused("motion mode", params=U(temporal=1))
    grp.denoise_upscale(U(temporal=0))
    rig.ctxs[1].denoise_temporal_set_motion(True)
    grp.denoise_upscale(U(temporal=1))
    used = capi.live_device_bytes()
    # a striped last frame
    grp.set_interleave(16)
    for c in rig.ctxs:
        c.reset_frame_index()
    grp.render(settings_for(capi.COSINE_WEIGHTED_SAMPLING))
    grp.synchronize()
    used = capi.live_device_bytes()                                      # (the striped frame's own buffers)
    refused("striped")
    rig.close()


# ------------------------------------------------------------------------------------------------ 8. memory
def test_buffers_are_counted_dropped_by_resize_and_freed():
    gc.collect()
    base = capi.live_device_bytes()
    w, h, bounds = 48, 64, [0, 20, 41, 64]
    rig = Rig("cornell", w, h, bounds, 0)
    st = settings_for(capi.NEE)
    rig.frame(st)
    rig.grp.synchronize()
    rendered = capi.live_device_bytes()
    px = w * h
    rig.grp.denoise_upscale(U(scale=2))
    used = capi.live_device_bytes()
    # per member: the denoiser's 80 B per pixel and the full-size hi-res records, 48 B per hi-res pixel; the hi-res staging (20 B): the
    # whole frame on member 0, the band's hi-res rows on the others
    assert used - rendered == 3 * (80 * px + 4 * 48 * px) + 4 * 20 * (px + w * (h - 20))
    for c in rig.ctxs:
        assert c.read_buffer(capi.BUF_UPSCALE_GUIDE).shape == (4 * px,) and c.read_buffer(capi.BUF_UPSCALE_ALBEDO).shape == (4 * px, 4)
    rig.frame(st)
    rig.grp.denoise_upscale(U(scale=2, iterations=2), want_radiance=False)
    assert capi.live_device_bytes() == used                              # allocated once
    rig.grp.denoise_upscale(U(scale=3), want_radiance=False)
    assert capi.live_device_bytes() - rendered == 3 * (80 * px + 9 * 48 * px) + 9 * 4 * (px + w * (h - 20))      # reallocated, not added
    rig.grp.synchronize()
    for c in rig.ctxs:
        c.resize(w, h)
    assert capi.live_device_bytes() == rendered                          # resize drops them
    rig.close()
    gc.collect()
    assert capi.live_device_bytes() == base
