"""fyprt_group_denoise_temporal / _device / _reset: the temporal denoiser on the row bands of a group.  The contract is
fyprt_denoise_temporal's on the stitched frame with one more term, the band's history window, and tests/group_temporal_ref.py restates
it; every comparison is bitwise (NaN-aware) on radiance, packed image and the stitched FYPRT_BUF_TEMPORAL: against that helper, fed with
the bands' accumulation, payload, albedo and history rows stitched together, and — where the window holds every tap and the group's
frame is the single context's — against Context.denoise_temporal of a single context rendering the same sequence.
The box has one GPU: the contexts share device 0, as in tests/test_gpu_group_denoise.py."""
import ctypes as C
import gc

import numpy as np
import pytest

from common import SCENES, bits_equal, settings_for, struct_equal
from denoise_ref import assert_numpy_keeps_subnormals
from fypraytracer_amd import capi
from group_temporal_ref import group_temporal_ref, rows_needed
from temporal_ref import DEFAULTS, camera_matrix

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
F = np.float32
W, H = 160, 192
TWO, FIVE = [0, 96, 192], [0, 40, 70, 150, 192]
# tests/test_gpu_moving_camera.py's MOVES: (keys held, mouse delta in pixels) per frame
MOVES = [("", (0.0, 0.0)), ("W", (60.0, -25.0)), ("DE", (-140.0, 40.0)), ("S", (90.0, 70.0)), ("AQ", (-35.0, -110.0)), ("W", (20.0, 10.0))]
RESTIR = (capi.RESTIR_DI, capi.RESTIR_GI)


def _halo_mode(tech):
    return 1 if tech in RESTIR else 0                                  # exchange for the ReSTIRs, recompute (nothing to exchange) otherwise


class Rig:
    """A group of contexts on device 0 with one camera for all of them; frame() renders the next frame of the sequence."""
    def __init__(self, scene_name, w, h, bounds, halo_mode, sc=None, contexts=None):
        mk_scene, mk_cam = SCENES[scene_name]
        self.sc = sc if sc is not None else mk_scene()
        self.cam = mk_cam(w, h)
        self.name, self.W, self.H, self.bounds = scene_name, w, h, list(bounds)
        self.ctxs = list(contexts) if contexts is not None else []
        while len(self.ctxs) < len(bounds) - 1:
            c = capi.Context(0)
            c.resize(w, h)
            c.upload_scene(self.sc)
            self.ctxs.append(c)
        for c in self.ctxs:
            c.set_camera(self.cam)
        self.grp = capi.Group(self.ctxs, bounds, halo_mode=halo_mode)
        self.seed = 0

    def frame(self, st, move=None):
        """Returns (frame index the frame was rendered with, projection x view of its camera)."""
        if move is not None:
            self.cam.on_update(0.05, *move)
        for c in self.ctxs:
            c.set_camera(self.cam)
        n = self.ctxs[0].frame_index
        self.seed += 1
        st.rand_seed = self.seed
        self.grp.render(st)
        M = camera_matrix(self.cam)
        if move is not None:
            self.cam.commit_frame()
        return n, M

    def set_rows(self, bounds):
        self.grp.set_rows(bounds)
        self.bounds = list(bounds)

    def stitched(self, which):
        """Buffer `which` of the frame: every band's rows from the context that owns them."""
        out = None
        for c, b, e in zip(self.ctxs, self.bounds, self.bounds[1:]):
            a = c.read_buffer(which)
            a = a.reshape(self.H, self.W, -1) if a.dtype.names is None and a.size != self.H * self.W else a.reshape(self.H, self.W)
            if out is None:
                out = np.zeros_like(a)
            out[b:e] = a[b:e]
        return out

    def close(self):
        self.grp.close()
        for c in self.ctxs:
            c.close()


class Ref:
    """What the reference carries from one call to the next: the stitched history record and the matrix of the frame denoised last."""
    def __init__(self):
        self.hist, self.M = None, None


def _eq(x, y):
    return struct_equal(x.reshape(-1), y.reshape(-1)) if x.dtype.names else bits_equal(x, y)


def _same(what, got, want):
    rad, img, rec = got
    want_rad, want_img, want_rec = want
    if rad is not None and want_rad is not None:
        eq = bits_equal(rad, want_rad)
        assert eq.all(), f"{what}: {(~eq).sum()} of {eq.size} radiance values differ, rows {sorted(set(np.argwhere(~eq)[:, 0].tolist()))[:8]}"
    if img is not None and want_img is not None:
        assert (img == want_img).all(), f"{what}: {(img != want_img).sum()} packed pixels differ"
    if rec is not None and want_rec is not None:
        for name in rec.dtype.names:
            eq = bits_equal(rec[name], want_rec[name])
            assert eq.all(), f"{what}: history field {name}: {(~eq).sum()} of {eq.size} values differ, first at {np.argwhere(~eq)[:3].tolist()}"


def _call(rig, n, M, refs, R, what="", **kw):
    """One Group.denoise_temporal call (parameters kw, history_rows R) on the frame rendered last, compared with group_temporal_ref
    continued from every state in `refs`: (Ref, reseed) pairs — afterwards a re-seeded state takes the device's stitched record, a chained
    one the reference's own.  (Two states that hold the same bits share one evaluation of the reference.)  Returns (radiance, image,
    stitched record)."""
    par = dict(DEFAULTS)
    par.update(kw)
    img, rad = rig.grp.denoise_temporal(capi.TemporalParams(**par), history_rows=R)
    acc, pay, alb, rec = (rig.stitched(b) for b in (capi.BUF_ACCUM, capi.BUF_PAYLOAD, capi.BUF_ALBEDO, capi.BUF_TEMPORAL))
    done = []
    for ref, reseed in refs:
        want = None
        for h, m, w in done:
            if (h is None) == (ref.hist is None) and (h is None or (_eq(h, ref.hist).all() and bits_equal(m, ref.M).all())):
                want = w
        if want is None:
            want = group_temporal_ref(acc, pay, alb, n, ref.M, ref.hist, rig.bounds, R, **par)
            done.append((ref.hist, ref.M, want))
        _same(f"{what} {'re-seeded' if reseed else 'chained'} R = {R} {kw}", (rad, img, rec), want)
        ref.hist, ref.M = (rec if reseed else want[2]), M
    return rad, img, rec


# ------------------------------------------------------------------------------------------------ 1. sequences
_single_cache = {}


def _single(tech, moving, frames=6):
    """Context.denoise_temporal (defaults) after every frame of a single context on hall_small 160 x 192: per frame (radiance, image,
    record, accumulation).  Computed once per sequence."""
    key = (tech, moving)
    if key not in _single_cache:
        mk_scene, mk_cam = SCENES["hall_small"]
        cam = mk_cam(W, H)
        ctx = capi.Context(0)
        ctx.resize(W, H)
        ctx.upload_scene(mk_scene())
        st = settings_for(tech)
        st.to_accumulate = 0 if moving else 1
        outs = []
        for f in range(frames):
            if moving:
                cam.on_update(0.05, *MOVES[f])
            ctx.set_camera(cam)
            st.rand_seed = f + 1
            ctx.render(st)
            if moving:
                cam.commit_frame()
            img, rad = ctx.denoise_temporal()
            outs.append((rad, img, ctx.read_buffer(capi.BUF_TEMPORAL).reshape(H, W), ctx.read_buffer(capi.BUF_ACCUM).reshape(H, W, 4)))
        ctx.close()
        _single_cache[key] = outs
    return _single_cache[key]


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("bounds", [TWO, FIVE])
@pytest.mark.parametrize("tech", [capi.RESTIR_DI, capi.RESTIR_GI, capi.NEE, capi.COSINE_WEIGHTED_SAMPLING])
def test_sequences_equal_the_contract_and_the_single_context(tech, bounds, moving):
    """Six calls, one per frame, defaults, history_rows = height.  Moving: MOVES with to_accumulate = 0; static: accumulating frames.  The
    single context's call is compared wherever the group's frame is the single context's: always but for a ReSTIR under a moving camera,
    whose temporal reuse across a band border reaches only the exchanged rows (include/fyprt.h, halo mode) — frame 1 still is."""
    assert_numpy_keeps_subnormals()
    single = _single(tech, moving)
    rig = Rig("hall_small", W, H, bounds, _halo_mode(tech))
    st = settings_for(tech)
    st.to_accumulate = 0 if moving else 1
    refs = [(Ref(), False), (Ref(), True)]
    compared = 0
    for f in range(6):
        n, M = rig.frame(st, MOVES[f] if moving else None)
        got = _call(rig, n, M, refs, H, f"tech {tech} bands {bounds} {'moving' if moving else 'static'} call {f + 1}")
        if bits_equal(rig.stitched(capi.BUF_ACCUM), single[f][3]).all():
            _same(f"tech {tech} bands {bounds} call {f + 1} against the single context", got, single[f][:3])
            compared += 1
    assert compared == 6 or (moving and tech in RESTIR and compared >= 1), compared
    rig.close()


# ------------------------------------------------------------------------------------------------ 2. the window
@pytest.mark.parametrize("tech", [capi.NEE, capi.RESTIR_DI])
@pytest.mark.parametrize("R", [16, 4, 0])
def test_the_window(tech, R):
    """The moving sequence on five bands.  No tap of it reaches more than 15 rows beyond its band (asserted here on the device's payload,
    and on the CPU oracle's in tests/test_group_temporal_cpu.py), so 16 rows are the single context; 4 rows cut history on calls 4 and 5;
    0 rows leave every band the history of its own rows."""
    single = _single(tech, True)
    rig = Rig("hall_small", W, H, FIVE, _halo_mode(tech))
    st = settings_for(tech)
    st.to_accumulate = 0
    refs = [(Ref(), False), (Ref(), True)]
    M_prev, reach = None, 0
    for f in range(6):
        n, M = rig.frame(st, MOVES[f])
        rad, img, rec = _call(rig, n, M, refs, R, f"tech {tech} call {f + 1}")
        if M_prev is not None:
            reach = max(reach, int(rows_needed(rig.stitched(capi.BUF_PAYLOAD), rig.stitched(capi.BUF_ALBEDO), M_prev, FIVE).max()))
        M_prev = M
        same_n = bits_equal(rec["N"], single[f][2]["N"]).all()          # (the history length depends on the geometry alone, not on the technique)
        if R == 16:
            assert same_n
            if tech == capi.NEE:
                _same(f"call {f + 1} against the single context", (rad, img, rec), single[f][:3])
        elif f in (3, 4):
            assert not same_n, f"call {f + 1}: a window of {R} rows cut nothing"
    assert reach == 15
    rig.close()


# ------------------------------------------------------------------------------------------------ 3. every kernel form on a second call
@pytest.fixture(scope="module")
def hall_five():
    rig = Rig("hall_small", W, H, FIVE, 1)
    yield rig
    rig.close()


def _second_call(rig, st, R, what, first=None, **kw):
    """Drops the history, renders a frame, calls (parameters `first`, default kw), turns the camera by MOVES[4] (the move whose taps reach
    15 rows), renders, and checks the second call with kw against the helper seeded with the device's record of the first."""
    rig.grp.denoise_temporal_reset()
    rig.cam = SCENES[rig.name][1](rig.W, rig.H)
    n, M = rig.frame(st, MOVES[3])
    par = dict(DEFAULTS)
    par.update(kw if first is None else first)
    rig.grp.denoise_temporal(capi.TemporalParams(**par), history_rows=R, want_radiance=False)
    ref = Ref()
    ref.hist, ref.M = rig.stitched(capi.BUF_TEMPORAL), M
    n, M = rig.frame(st, MOVES[4])
    return _call(rig, n, M, [(ref, True)], R, what, **kw)


SWEEP = [dict(iterations=it) for it in range(9)]
SWEEP += [dict(iterations=it, **kw) for it in (3, 6) for kw in (dict(demodulate_albedo=0), dict(sigma_luminance=0.0), dict(sigma_luminance=16.0),
                                                               dict(history_limit=1), dict(history_limit=2), dict(feedback=0))]


@pytest.mark.parametrize("kw", SWEEP, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_iteration_sweep(hall_five, kw):
    """0: the 2-row guide floor and k_dn_finish; 1..6: the staged steps; 7, 8: the gather form, whose halos cross every band.  A window of
    4 rows, so that the reprojection's window term is at work (the move reaches 15)."""
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0
    rad, img, rec = _second_call(hall_five, st, 4, "sweep", **kw)
    assert (rec["N"] > 1).any() or kw.get("history_limit") == 1


# ------------------------------------------------------------------------------------------------ 4. windows that can go wrong
@pytest.mark.parametrize("scene_name,w,h,bounds", [
    ("hall_small", 160, 192, [0, 1, 2, 95, 96, 192]),            # one-row bands at the image edge and mid-image
    ("cornell", 97, 61, [0, 1, 17, 18, 61]),                     # off every tile size
    ("banana", 33, 5, [0, 2, 5]),                                # textures; lower than a tile
])
def test_band_windows(scene_name, w, h, bounds):
    rig = Rig(scene_name, w, h, bounds, 0)
    st = settings_for(capi.NEE)
    st.to_accumulate = 0
    for it in (0, 1, 3, 6):
        for R in (0, 1, h):
            rig.grp.denoise_temporal_reset()
            refs = [(Ref(), True)]
            for f in (0, 1):
                n, M = rig.frame(st, MOVES[1 + f])
                if f == 1 or R == h:                                     # (the first call does not depend on R)
                    _call(rig, n, M, refs, R, f"{scene_name} {bounds} call {f + 1}", iterations=it)
                else:
                    rig.grp.denoise_temporal(capi.TemporalParams(**dict(DEFAULTS, iterations=it)), history_rows=R, want_radiance=False)
                    refs[0][0].hist, refs[0][0].M = rig.stitched(capi.BUF_TEMPORAL), M
    rig.close()


# ------------------------------------------------------------------------------------------------ 5. moved borders
@pytest.mark.parametrize("tech,moving", [(capi.NEE, True), (capi.RESTIR_DI, False)])
def test_moved_borders_keep_the_sequence(tech, moving):
    """Group.set_rows between calls moves the history records with the rows: with history_rows = height the sequence stays the single
    context's (and the helper's, which knows nothing of owners)."""
    single = _single(tech, moving)
    rig = Rig("hall_small", W, H, TWO, _halo_mode(tech))
    st = settings_for(tech)
    st.to_accumulate = 0 if moving else 1
    refs = [(Ref(), False)]
    for f in range(6):
        n, M = rig.frame(st, MOVES[f] if moving else None)
        got = _call(rig, n, M, refs, H, f"tech {tech} call {f + 1} bands {rig.bounds}")
        _same(f"tech {tech} call {f + 1} bands {rig.bounds} against the single context", got, single[f][:3])
        if f == 1:
            rig.set_rows([0, 40, 192])
        if f == 3:
            rig.set_rows([0, 150, 192])
    rig.close()


# ------------------------------------------------------------------------------------------------ 6. what drops the history
def test_what_drops_the_history():
    w, h, bounds = 96, 64, [0, 20, 64]
    rig = Rig("cornell", w, h, bounds, 0)
    st = settings_for(capi.NEE)
    st.to_accumulate = 0
    ref = Ref()

    def step(what, first):                                              # (a static camera: what is looked at is the history length)
        if first:
            ref.hist = None
        n, M = rig.frame(st)
        _, _, rec = _call(rig, n, M, [(ref, False)], h, what)
        flt = rec["filterable"] != 0
        assert ((rec["N"][flt] == 1).all()) == first, what             # a first call on all rows — or a history on some

    step("first", True)
    step("second", False)
    # a refused call drops nothing
    p = capi.TemporalParams(history_limit=0)
    img = np.empty(w * h, np.uint32)
    assert rig.grp.lib.fyprt_group_denoise_temporal(rig.grp.h, C.byref(p), h, img.ctypes.data_as(C.c_void_p), None, None) == EINVAL
    step("after a refused call", False)
    rig.grp.denoise_temporal_reset()
    step("after the group reset", True)
    step("and on", False)
    rig.ctxs[1].denoise_temporal_reset()
    step("after one member's reset", True)
    step("and on", False)
    for c in rig.ctxs:
        c.update_materials(rig.sc)
    with pytest.raises(capi.FyprtError, match="no complete frame"):
        rig.grp.denoise_temporal()
    step("after update_materials on all members", True)
    step("and on", False)
    # resize and regroup
    rig.grp.close()
    for c in rig.ctxs:
        c.resize(w, h)
    rig.grp = capi.Group(rig.ctxs, bounds, halo_mode=0)
    step("after resize and regroup", True)
    step("and on", False)
    # a regroup alone: the history was another group's
    rig.grp.close()
    rig.grp = capi.Group(rig.ctxs, bounds, halo_mode=0)
    step("after a regroup", True)
    rig.close()
    # a context that ran a single-context temporal call before it joined
    loner = capi.Context(0)
    loner.resize(w, h)
    sc = SCENES["cornell"][0]()
    loner.upload_scene(sc)
    loner.set_camera(SCENES["cornell"][1](w, h))
    loner.render(st)
    loner.denoise_temporal()
    rig = Rig("cornell", w, h, bounds, 0, sc=sc, contexts=[loner])
    for c in rig.ctxs:
        c.reset_frame_index()
    step("with a member that denoised on its own before", True)
    step("and on", False)
    with pytest.raises(capi.FyprtError, match="every row"):
        rig.ctxs[0].denoise_temporal()                                  # a member on its own stays refused
    step("after the refused member call", False)
    rig.close()


# ------------------------------------------------------------------------------------------------ 7. object motion
def test_object_motion_equals_the_single_context():
    """The dragged mesh of tests/test_gpu_temporal_motion.py (hall_small, mesh 7) on three bands: motion on for every member, the edit
    applied to every member before every frame, history_rows = height: call for call the single context with motion on.  Mixed modes are
    refused."""
    w, h, bounds = 96, 64, [0, 20, 41, 64]
    drag = {7: ((0.02, 0.0, -0.015), (0.0, 1.5, 0.0), (0.0, 0.0, 0.0))}
    sc = SCENES["hall_small"][0]()
    mgr = sc.manager()
    mgr.perform_all_scene_updates(sc)
    rig = Rig("hall_small", w, h, bounds, 0, sc=sc)
    one = Rig("hall_small", w, h, [0, h], 0, sc=sc)
    everyone = rig.ctxs + one.ctxs
    for c in everyone:
        c.set_object_vertices(sc)
        c.denoise_temporal_set_motion(True)
    base = [dict(t) for t in sc.mesh_transforms]
    st = settings_for(capi.NEE)
    st.to_accumulate = 0
    kept = []
    for f in range(5):
        for m, (dp, dr, ds) in drag.items():
            k, b = F(f + 1), base[m]
            mgr.set_mesh_transform(sc, m, pos=tuple(F(x) + k * F(d) for x, d in zip(b["pos"], dp)),
                                   rotation=tuple(F(x) + k * F(d) for x, d in zip(b["rotation"], dr)),
                                   scale_=tuple(F(x) + k * F(d) for x, d in zip(b["scale"], ds)))
        mgr.perform_all_scene_updates(sc)
        for c in everyone:
            c.update_transforms(sc, list(drag))
        for r in (rig, one):
            r.seed = f
            r.frame(st, MOVES[f])
        img, rad = rig.grp.denoise_temporal(history_rows=h)
        want_img, want_rad = one.grp.denoise_temporal(history_rows=h)   # a one-member group: the band [0, H), the single context's launch
        rec, want_rec = rig.stitched(capi.BUF_TEMPORAL), one.stitched(capi.BUF_TEMPORAL)
        _same(f"motion call {f + 1}", (rad, img, rec), (want_rad, want_img, want_rec))
        first, count, _ = sc.meshes[7]
        tri = rig.stitched(capi.BUF_PAYLOAD)["objectIndex"]
        on = (tri >= first) & (tri < first + count) & (rec["filterable"] != 0)
        kept.append(bool(on.any() and (rec["N"][on] == f + 1).any()))
    assert all(kept), kept                                              # the dragged mesh keeps its history through every edit
    rig.ctxs[1].denoise_temporal_set_motion(False)
    p = capi.TemporalParams()
    img = np.empty(w * h, np.uint32)
    assert rig.grp.lib.fyprt_group_denoise_temporal(rig.grp.h, C.byref(p), h, img.ctypes.data_as(C.c_void_p), None, None) == ESTATE
    with pytest.raises(capi.FyprtError, match="motion mode"):
        rig.grp.denoise_temporal()
    rig.close()
    one.close()


def test_one_member_motion_group_is_the_single_context():
    """What the test above compares with: a one-member group with motion on equals Context.denoise_temporal with motion on."""
    w, h = 96, 64
    drag = {7: ((0.02, 0.0, -0.015), (0.0, 1.5, 0.0), (0.0, 0.0, 0.0))}
    outs = []
    for grouped in (False, True):
        sc = SCENES["hall_small"][0]()
        mgr = sc.manager()
        mgr.perform_all_scene_updates(sc)
        rig = Rig("hall_small", w, h, [0, h], 0, sc=sc)
        ctx = rig.ctxs[0]
        ctx.set_object_vertices(sc)
        ctx.denoise_temporal_set_motion(True)
        if not grouped:
            rig.grp.close()
        base = [dict(t) for t in sc.mesh_transforms]
        st = settings_for(capi.NEE)
        st.to_accumulate = 0
        res = []
        for f in range(3):
            k, b = F(f + 1), base[7]
            dp, dr, ds = drag[7]
            mgr.set_mesh_transform(sc, 7, pos=tuple(F(x) + k * F(d) for x, d in zip(b["pos"], dp)),
                                   rotation=tuple(F(x) + k * F(d) for x, d in zip(b["rotation"], dr)),
                                   scale_=tuple(F(x) + k * F(d) for x, d in zip(b["scale"], ds)))
            mgr.perform_all_scene_updates(sc)
            ctx.update_transforms(sc, [7])
            rig.cam.on_update(0.05, *MOVES[f])
            ctx.set_camera(rig.cam)
            st.rand_seed = f + 1
            if grouped:
                rig.grp.render(st)
            else:
                ctx.set_rows(0, h)
                ctx.render(st)
            rig.cam.commit_frame()
            img, rad = rig.grp.denoise_temporal(history_rows=h) if grouped else ctx.denoise_temporal()
            res.append((rad, img, ctx.read_buffer(capi.BUF_TEMPORAL).reshape(h, w)))
        outs.append(res)
        rig.close()
    for k, (a, b) in enumerate(zip(*outs)):
        _same(f"call {k + 1}", b, a)


# ------------------------------------------------------------------------------------------------ 8. the device entry (torch)
def test_roots_outputs_and_the_device_entry():
    """In a fresh process that initialises torch's CUDA before the library is loaded (tests/test_gpu_query.py explains why)."""
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    code = ("import sys, torch; torch.cuda.init(); torch.cuda.set_device(0); sys.path[:0] = [%r, %r]; import test_gpu_group_temporal as t; "
            "t._torch_checks(); print('group temporal torch path ok')" % (str(here), str(here.parent)))
    r = subprocess.run([sys.executable, "-u", "-X", "faulthandler", "-c", code], cwd=str(here.parent), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "group temporal torch path ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _torch_checks():
    import torch
    par = dict(DEFAULTS, iterations=4)
    st = settings_for(capi.RESTIR_DI)
    st.to_accumulate = 0

    def tensors():
        return torch.empty((H, W), dtype=torch.int32, device="cuda:0"), torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")

    def host(t):
        return None if t is None else (t.cpu().numpy().view(np.uint32) if t.dtype == torch.int32 else t.cpu().numpy())

    # the blocking entry: three frames, a call after each
    rig = Rig("hall_small", W, H, FIVE, 1)
    want = []
    for f in range(3):
        rig.frame(st, MOVES[f])
        img, rad = rig.grp.denoise_temporal(capi.TemporalParams(**par), history_rows=16)
        want.append((rad, img, rig.stitched(capi.BUF_TEMPORAL)))
    rig.close()
    # the device entry: the same three frames and calls back to back, a different root each, no host wait in between
    rig = Rig("hall_small", W, H, FIVE, 1)
    outs = []
    for f in range(3):
        rig.frame(st, MOVES[f])
        img, rad = tensors()
        rig.grp.denoise_temporal_tensor(img, rad, capi.TemporalParams(**par), history_rows=16, root=(2, 4 - 1, 0)[f])
        outs.append((img, rad))
    got = [(host(rad), host(img), None) for img, rad in outs]
    rig.grp.synchronize()
    for f in range(3):
        _same(f"device entry, call {f + 1}", got[f], want[f])
    _same("device entry, the history after three calls", (None, None, rig.stitched(capi.BUF_TEMPORAL)), (None, None, want[2][2]))
    # every root, either output alone: calls on the frame denoised last reproject it onto itself
    ref_rig = Rig("hall_small", W, H, FIVE, 1)
    for f in range(3):
        ref_rig.frame(st, MOVES[f])
        ref_rig.grp.denoise_temporal(capi.TemporalParams(**par), history_rows=16, want_radiance=False)
    for root in range(4):
        img, _ = tensors()
        _, rad = tensors()
        rig.grp.denoise_temporal_tensor(img, None, capi.TemporalParams(**par), history_rows=16, root=root)
        rig.grp.denoise_temporal_tensor(None, rad, capi.TemporalParams(**par), history_rows=16, root=root)
        w_img, _ = ref_rig.grp.denoise_temporal(capi.TemporalParams(**par), history_rows=16)
        _, w_rad = ref_rig.grp.denoise_temporal(capi.TemporalParams(**par), history_rows=16)
        _same(f"root {root}, image only", (None, host(img), None), (None, w_img, None))
        _same(f"root {root}, radiance only", (host(rad), None, None), (w_rad, None, None))
    with pytest.raises(ValueError):
        rig.grp.denoise_temporal_tensor(torch.empty((H, W), dtype=torch.float32, device="cuda:0"), None)
    with pytest.raises(ValueError):
        rig.grp.denoise_temporal_tensor(outs[0][0], None, root=4)
    with pytest.raises(ValueError):
        rig.grp.denoise_temporal_tensor(None, None)
    rig.close()
    ref_rig.close()


# ------------------------------------------------------------------------------------------------ 9. state and buffers
def _member_state(c):
    c.synchronize()
    return [c.read_buffer(b) for b in range(9)], c.frame_index


@pytest.mark.parametrize("tech", RESTIR)
def test_no_frame_state_moves_and_the_sequence_is_the_sequence_without_the_calls(tech):
    rig = Rig("hall_small", W, H, TWO, 1)
    plain = Rig("hall_small", W, H, TWO, 1)
    st = settings_for(tech)
    for f in range(4):
        rig.frame(st)
        plain.frame(st)
        before = [_member_state(c) for c in rig.ctxs]
        rig.grp.denoise_temporal(want_radiance=False)
        rig.grp.denoise_temporal(capi.TemporalParams(iterations=2, demodulate_albedo=0), history_rows=0)
        for (a, ia), (b, ib) in zip(before, [_member_state(c) for c in rig.ctxs]):
            for k, (x, y) in enumerate(zip(a, b)):
                assert _eq(x, y).all(), f"frame {f + 1}: buffer {k} moved"
            assert ia == ib
        for which in (capi.BUF_ACCUM, capi.BUF_IMAGE, capi.BUF_PAYLOAD):
            assert _eq(rig.stitched(which), plain.stitched(which)).all(), f"frame {f + 1}: buffer {which} differs from the sequence without calls"
        if f == 1:
            rig.set_rows([0, 80, 192])
            plain.set_rows([0, 80, 192])
    rig.close()
    plain.close()


def test_buffers_are_counted_dropped_by_resize_and_freed():
    gc.collect()
    base = capi.live_device_bytes()
    w, h, bounds = 96, 64, [0, 20, 41, 64]
    rig = Rig("cornell", w, h, bounds, 0)
    st = settings_for(capi.NEE)
    rig.frame(st)
    rig.grp.synchronize()
    rendered = capi.live_device_bytes()
    rig.grp.denoise_temporal()
    used = capi.live_device_bytes()
    # per member: the spatial denoiser's 80 B per pixel and two history (64 B) and two variance (4 B) buffers; the staging as fyprt_group_denoise
    assert used - rendered == 3 * (80 + 2 * 64 + 2 * 4) * w * h + 20 * w * h + 20 * w * (h - 20)
    rig.frame(st)
    rig.grp.denoise_temporal(capi.TemporalParams(iterations=2), history_rows=4, want_radiance=False)
    assert capi.live_device_bytes() == used                              # allocated once
    rig.grp.synchronize()
    for c in rig.ctxs:
        c.resize(w, h)
    assert capi.live_device_bytes() == rendered                          # resize drops them
    rig.close()
    gc.collect()
    assert capi.live_device_bytes() == base


# ------------------------------------------------------------------------------------------------ 10. errors
def test_errors_in_the_documented_order():
    w, h, bounds = 96, 64, [0, 20, 64]
    rig = Rig("cornell", w, h, bounds, 0)
    grp, lib = rig.grp, rig.grp.lib
    T = capi.TemporalParams
    ok = T()
    img = np.empty(w * h, np.uint32)
    out = img.ctypes.data_as(C.c_void_p)
    dev = C.c_void_p(rig.ctxs[0].image_device_ptr())                     # a device address for the refused device calls (never written)

    def rc(p=ok, rgba8=out, radiance4=None):
        return lib.fyprt_group_denoise_temporal(grp.h, C.byref(p) if p is not None else None, h, rgba8, radiance4, None)

    def rcd(p=ok, root=0, rgba8=dev, radiance4=None):
        return lib.fyprt_group_denoise_temporal_device(grp.h, C.byref(p), h, root, rgba8, radiance4)

    nan = float("nan")
    for have_frame in (False, True):                                     # before any frame, and with one: the argument errors come first
        assert rc(p=None) == EINVAL
        for p in (T(history_limit=0), T(history_limit=257), T(feedback=2), T(normal_min=nan), T(plane_max=0.0),      # the temporal part's,
                  T(iterations=9), T(normal_power_log2=8), T(sigma_plane=0.0), T(sigma_luminance=nan)):               # then the spatial part's
            assert rc(p=p) == EINVAL and rcd(p=p) == EINVAL
            assert rcd(p=p, root=7) == EINVAL
        assert rcd(root=2) == EINVAL and rcd(root=-1) == EINVAL
        assert rcd(rgba8=C.c_void_p(dev.value + 2)) == EINVAL           # misaligned
        assert rcd(rgba8=None, radiance4=C.c_void_p(dev.value + 4)) == EINVAL
        assert rc(rgba8=None) == EINVAL and rcd(rgba8=None) == EINVAL    # both outputs NULL
        if not have_frame:
            assert rc() == ESTATE and rcd() == ESTATE
            with pytest.raises(capi.FyprtError, match="no complete frame"):
                grp.denoise_temporal()
        rig.frame(settings_for(capi.NEE))
    grp.denoise_temporal()
    rig.ctxs[1].render(settings_for(capi.NEE))                           # one member a frame ahead
    with pytest.raises(capi.FyprtError, match="frame index"):
        grp.denoise_temporal()
    for c in rig.ctxs:
        c.reset_frame_index()
    rig.frame(settings_for(capi.NEE))
    rig.ctxs[0].set_rows(0, 10)                                          # rows moved behind the group
    with pytest.raises(capi.FyprtError, match="not its band"):
        grp.denoise_temporal()
    rig.ctxs[0].set_rows(0, 20)
    grp.denoise_temporal()
    # the members' last frames differ in camera matrix: one member renders the frame again with a turned camera
    turned = SCENES["cornell"][1](w, h)
    turned.on_update(0.05, *MOVES[2])
    for c in rig.ctxs:
        c.reset_frame_index()
    rig.ctxs[1].set_camera(turned)
    st = settings_for(capi.NEE)
    grp.render(st)
    assert rc() == ESTATE
    with pytest.raises(capi.FyprtError, match="camera matrix"):
        grp.denoise_temporal()
    # ... before the motion mode is looked at
    rig.ctxs[0].denoise_temporal_set_motion(True)
    with pytest.raises(capi.FyprtError, match="camera matrix"):
        grp.denoise_temporal()
    for c in rig.ctxs:
        c.reset_frame_index()
    rig.frame(st)
    with pytest.raises(capi.FyprtError, match="motion mode"):
        grp.denoise_temporal()
    rig.ctxs[1].denoise_temporal_set_motion(True)
    grp.denoise_temporal()
    grp.set_interleave(16)
    for c in rig.ctxs:
        c.reset_frame_index()
    grp.render(settings_for(capi.COSINE_WEIGHTED_SAMPLING))
    with pytest.raises(capi.FyprtError, match="striped"):
        grp.denoise_temporal()
    rig.close()
