"""numpy restatement of the upscaler's contract (include/fyprt.h, "upscaler") — a test helper, not a test.

As tests/denoise_ref.py: every operation is binary32 in the header's order (float32 arrays, float32 scalar constants), max(a, b) is
where(a < b, b, a), a skipped tap is selected away (never multiplied by zero) and the sums run in tap order from +0.  The device kernel
(fypraytracer_amd/csrc/rt_upscale.h: k_up_resolve) must reproduce radiance and image bit for bit.

The low-res stage is not restated: lowres_colour / lowres_colour_temporal get e_p out of denoise_ref / temporal_ref by feeding them the
pre-demodulated colour (accum := e0 with w kept, n := 1, demodulate_albedo = 0).  Both references use d only to form e0 and the output,
so with d = 1 and c = e0 every intermediate value is the one of the real call and the "output" is e where filterable, c elsewhere; the
history record temporal_ref returns is the real call's for the same reason (its colour is the integrated or the feedback colour, its
moments come from L(e0))."""
import numpy as np

from denoise_ref import denoise_ref, tonemap_pack
from fypraytracer_amd.capi import UPSCALE_GUIDE_DTYPE
from temporal_ref import dot3, temporal_ref

F = np.float32
ALIGNED, PASS_THROUGH, WEIGHTED, BILINEAR, NO_TAP = range(5)      # the branch map: aligned, pass-through, S > 0, bilinear (S = 0), no usable tap
BRANCH_NAMES = ("aligned", "pass-through", "S > 0", "bilinear", "no tap")
SPATIAL_KEYS = ("iterations", "sigma_luminance", "sigma_plane", "normal_power_log2", "demodulate_albedo")


def _predemodulated(accum, albedo, n, demodulate_albedo):
    accum = np.ascontiguousarray(accum, dtype=F)
    albedo = np.ascontiguousarray(albedo, dtype=F)
    with np.errstate(all="ignore"):
        c = accum[..., :3] / F(n)
        flt = albedo[..., 3] != 0
        a = albedo[..., :3]
        d = np.where(a < F(1e-3), F(1e-3), a)
        e0 = np.where(flt[..., None], c / d, c) if demodulate_albedo else c
    acc = accum.copy()
    acc[..., :3] = e0
    return acc


def lowres_colour(accum, payload, albedo, n, **par):
    """e_p (H x W x 3) of fyprt_denoise with parameters `par` (c_p where the pixel is not filterable)."""
    acc = _predemodulated(accum, albedo, n, par.get("demodulate_albedo", 1))
    return denoise_ref(acc, payload, albedo, 1, **dict(par, demodulate_albedo=0))[0][..., :3]


def lowres_colour_temporal(accum, payload, albedo, n, M_prev, hist, **par):
    """(e_p, new history record array) of fyprt_denoise_temporal with parameters `par`."""
    acc = _predemodulated(accum, albedo, n, par.get("demodulate_albedo", 1))
    rad, _, new = temporal_ref(acc, payload, albedo, 1, M_prev, hist, **dict(par, demodulate_albedo=0))
    return rad[..., :3], new


def hires_from_payload(scene, payload, sky, sample_texture=None):
    """(guide sH x sW UPSCALE_GUIDE_DTYPE, albedo sH x sW x 4) from the payload of a frame rendered at the hi-res size: the two hi-res
    buffers as step 2 of the contract defines them.  sky: the sky colour of the settings the low-res frame was rendered with."""
    from denoise_ref import guides_from_scene
    alb = guides_from_scene(scene, payload, sample_texture)
    flt = alb[..., 3] != 0
    tri = payload["objectIndex"]
    mats = scene.materials_array()
    m = mats[scene.triangles["materialIndex"][np.where(tri >= 0, tri, 0)]]
    em = m["emissionColor"].astype(F) * m["emissionPower"].astype(F)[..., None]
    alb[..., :3] = np.where(flt[..., None], alb[..., :3], np.where((tri >= 0)[..., None], em, np.asarray(sky, dtype=F)))
    g = np.zeros(payload.shape, dtype=UPSCALE_GUIDE_DTYPE)
    g["worldPosition"], g["hitDistance"], g["worldNormal"], g["filterable"] = payload["worldPosition"], payload["hitDistance"], payload["worldNormal"], flt
    return g, alb


def upscale_ref(e, payload, albedo, accum, n, up_guide, up_albedo, scale, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1, **_unused):
    """Step 3 of the contract.  e: H x W x 3, the low-res colour after the last iteration; payload, albedo, accum, n: the low-res frame's
    as denoise_ref takes them; up_guide (sH x sW, UPSCALE_GUIDE_DTYPE) and up_albedo (sH x sW x 4): the two hi-res buffers.
    Returns (radiance4 sH x sW x 4 float32, rgba8 sH x sW uint32, branch map sH x sW of ALIGNED ... NO_TAP)."""
    s = int(scale)
    e = np.ascontiguousarray(e, dtype=F)
    albedo = np.ascontiguousarray(albedo, dtype=F)
    accum = np.ascontiguousarray(accum, dtype=F)
    up_albedo = np.ascontiguousarray(up_albedo, dtype=F)
    Hh, Ww = e.shape[:2]
    assert up_guide.shape == (Hh * s, Ww * s) and up_albedo.shape == (Hh * s, Ww * s, 4)
    with np.errstate(all="ignore"):
        flt = albedo[..., 3] != 0
        a = albedo[..., :3]
        d = np.where(a < F(1e-3), F(1e-3), a)
        out_lo = np.where(flt[..., None], e * d, e) if demodulate_albedo else e      # e holds c_p where the pixel is not filterable
        P = np.ascontiguousarray(payload["worldPosition"], dtype=F)
        N = np.ascontiguousarray(payload["worldNormal"], dtype=F)
        Y, X = np.mgrid[0:Hh * s, 0:Ww * s]
        x0, y0 = X // s, Y // s
        fx, fy = X - s * x0, Y - s * y0
        aligned = (fx == 0) & (fy == 0)
        fQ = up_albedo[..., 3] != 0
        aQ = up_albedo[..., :3]
        dQ = np.where(aQ < F(1e-3), F(1e-3), aQ)
        PQ = np.ascontiguousarray(up_guide["worldPosition"], dtype=F)
        NQ = np.ascontiguousarray(up_guide["worldNormal"], dtype=F)
        spt = F(sigma_plane) * np.ascontiguousarray(up_guide["hitDistance"], dtype=F)
        tx, ty = fx.astype(F) / F(s), fy.astype(F) / F(s)
        S, B = np.zeros(X.shape, F), np.zeros(X.shape, F)
        Cc, D = np.zeros(X.shape + (3,), F), np.zeros(X.shape + (3,), F)
        usable = np.zeros(X.shape, bool)
        for dy in (0, 1):
            for dx in (0, 1):
                b = (tx if dx else F(1) - tx) * (ty if dy else F(1) - ty)
                qx, qy = x0 + dx, y0 + dy
                inside = (qx < Ww) & (qy < Hh)
                qx, qy = np.minimum(qx, Ww - 1), np.minimum(qy, Hh - 1)
                dd = dot3(NQ, N[qy, qx])
                wn = np.where(F(0) < dd, dd, F(0))
                for _ in range(int(normal_power_log2)):
                    wn = wn * wn
                xz = np.abs(dot3(NQ, P[qy, qx] - PQ)) / spt
                wz = F(1) / (F(1) + xz * xz)
                w = (wn * wz) * b
                use = inside & flt[qy, qx] & (b > 0)
                eq = e[qy, qx]
                S = np.where(use, S + w, S)
                Cc = np.where(use[..., None], Cc + eq * w[..., None], Cc)
                B = np.where(use, B + b, B)
                D = np.where(use[..., None], D + eq * b[..., None], D)
                usable |= use
        E = np.where((S > 0)[..., None], Cc / S[..., None], D / B[..., None])
        outE = E * dQ if demodulate_albedo else E
        base = out_lo[y0, x0]
        out = np.where(aligned[..., None], base, np.where(~fQ[..., None], aQ, np.where(usable[..., None], outE, base)))
        branch = np.where(aligned, ALIGNED, np.where(~fQ, PASS_THROUGH, np.where(~usable, NO_TAP, np.where(S > 0, WEIGHTED, BILINEAR))))
        rad = np.empty(X.shape + (4,), dtype=F)
        rad[..., :3] = out
        rad[..., 3] = accum[y0, x0, 3] / F(n)
    assert rad.dtype == F and E.dtype == F and S.dtype == F
    return rad, tonemap_pack(rad), branch.astype(np.int8)


def sliver_scene():
    """A scene for the two rare branches at scale 2, low-res 16 x 16 (sliver_camera): a floor (normal +y) below a sky, and in front of
    both a vertical strip (normal +z) so thin that it covers hi-res column 17 only — between the sample columns 16 and 18, so no low-res
    pixel sees it.  Its pixels over the floor find usable taps whose normals are perpendicular to their own (w_n = 0, S = 0: the bilinear
    branch); its pixels over the sky find no filterable tap at all.  A light behind the camera keeps every technique's checks content."""
    from fypraytracer_amd.scene import Material, Scene
    from fypraytracer_amd.scenes import _quad
    sc = Scene()
    sc.materials = [Material(albedo=(0.8, 0.8, 0.8), roughness=1.0, metallic=0.0), Material(albedo=(0.2, 0.3, 1.0), roughness=1.0, metallic=0.0),
                    Material(albedo=(1, 1, 1), emission_color=(1, 1, 1), emission_power=10.0)]
    add = sc.add_new_mesh_to_scene
    add(*_quad((-60, -1, 2), (60, -1, 2), (60, -1, -60), (-60, -1, -60), (0, 1, 0)), material_index=0)            # floor
    xc = 0.0625 * np.tan(np.radians(22.5)) * 2.4                       # hi-res column 17 of 32 at the strip's depth (fov 45, aspect 1)
    add(*_quad((xc - 0.02, -0.9, 1.0), (xc + 0.02, -0.9, 1.0), (xc + 0.02, 0.9, 1.0), (xc - 0.02, 0.9, 1.0), (0, 0, 1)), material_index=1)
    add(*_quad((-0.5, -0.5, 6.0), (-0.5, 0.5, 6.0), (0.5, 0.5, 6.0), (0.5, -0.5, 6.0), (0, 0, -1)), material_index=2)   # behind the camera
    sc.init_scene_emissive_triangles()
    return sc


def sliver_camera(width, height):
    from fypraytracer_amd.scenes import cornell_camera
    return cornell_camera(width, height)
