"""numpy restatement of the temporal denoiser's contract (include/fyprt.h, "temporal denoiser") — a test helper, not a test.

As tests/denoise_ref.py: every operation is binary32 in the header's order (float32 arrays, float32 scalar constants), max(a, b) is
where(a < b, b, a), a skipped tap is selected away (never multiplied by zero) and the sums run in tap order from +0.  The device kernels
(fypraytracer_amd/csrc/rt_temporal.h) must reproduce radiance, image and history record bit for bit."""
import numpy as np

from denoise_ref import H5, _shift, luminance, tonemap_pack
from fypraytracer_amd.capi import TEMPORAL_DTYPE

F = np.float32
G3 = (F(0.25), F(0.5), F(0.25))
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1,
                history_limit=32, normal_min=0.9, plane_max=0.02, feedback=1)


def matmul_cm(a, b):
    """Column-major 4 x 4 product in the library's operation order (fyprt_set_camera's host product); returns [col][row]."""
    a = np.asarray(a, dtype=F).reshape(4, 4)
    b = np.asarray(b, dtype=F).reshape(4, 4)
    out = np.zeros((4, 4), dtype=F)
    for j in range(4):
        for r in range(4):
            t = F(F(a[0, r] * b[j, 0]) + F(a[1, r] * b[j, 1]))
            t = F(t + F(a[2, r] * b[j, 2]))
            t = F(t + F(a[3, r] * b[j, 3]))
            out[j, r] = t
    return out


def camera_matrix(cam):
    """projection x view of a camera object, what the library keeps for the frame rendered with it."""
    return matmul_cm(np.asarray(cam.projection, dtype=F).ravel(), np.asarray(cam.view, dtype=F).ravel())


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _weights_nz(N, P, spt, Nq, Pq, npow):
    dd = dot3(N, Nq)
    wn = np.where(F(0) < dd, dd, F(0))
    for _ in range(int(npow)):
        wn = wn * wn
    xz = np.abs(dot3(N, Pq - P)) / spt
    return wn, F(1) / (F(1) + xz * xz)


def temporal_ref(accum, payload, albedo, n, M_prev, hist, iterations=5, sigma_luminance=4.0, sigma_plane=0.01, normal_power_log2=6,
                 demodulate_albedo=1, history_limit=32, normal_min=0.9, plane_max=0.02, feedback=1, row0=0, full_height=None):
    """accum, payload, albedo, n as denoise_ref.  M_prev: camera_matrix of the frame the previous call denoised; hist: the history record
    array (H x W, TEMPORAL_DTYPE) that call wrote, or None for a first call.  Returns (radiance4, rgba8, new history record array).
    row0 / full_height: the frame's arrays are rows row0 .. row0 + H of an image of full_height rows; hist is then either the same rows
    (every reprojection tap must lie inside them) or the whole image.  The rows near the cut see a wrong "inside the image" in the
    spatial steps: compare inner rows only."""
    accum = np.ascontiguousarray(accum, dtype=F)
    albedo = np.ascontiguousarray(albedo, dtype=F)
    Hh, Ww = accum.shape[:2]
    Hfull = Hh if full_height is None else int(full_height)
    n = F(n)
    sigma_l, limit = F(sigma_luminance), F(history_limit)
    with np.errstate(all="ignore"):
        c = accum[..., :3] / n
        flt = albedo[..., 3] != 0
        a = albedo[..., :3]
        d = np.where(a < F(1e-3), F(1e-3), a) if demodulate_albedo else np.ones_like(a)
        e0 = np.where(flt[..., None], c / d, c) if demodulate_albedo else c.copy()
        P = np.ascontiguousarray(payload["worldPosition"], dtype=F)
        N = np.ascontiguousarray(payload["worldNormal"], dtype=F)
        t = np.ascontiguousarray(payload["hitDistance"], dtype=F)
        spt = F(sigma_plane) * t
        L = luminance(e0)
        LL = L * L
        Nn = np.where(flt, F(1), F(0)).astype(F)
        ci, m1, m2 = e0.copy(), L.copy(), LL.copy()
        if hist is not None:
            M = np.asarray(M_prev, dtype=F).reshape(4, 4)
            cl = [(M[0, r] * P[..., 0] + M[1, r] * P[..., 1]) + (M[2, r] * P[..., 2] + M[3, r]) for r in (0, 1, 3)]
            ok = flt & (cl[2] > 0)
            sx = ((cl[0] / cl[2]) * F(0.5) + F(0.5)) * F(Ww)
            sy = ((cl[1] / cl[2]) * F(0.5) + F(0.5)) * F(Hfull)
            ok &= (sx >= F(-1)) & (sx < F(Ww)) & (sy >= F(-1)) & (sy < F(Hfull))
            x0f, y0f = np.floor(sx), np.floor(sy)
            wx, wy = sx - x0f, sy - y0f
            x0 = np.where(ok, x0f, 0).astype(np.int64)
            y0 = np.where(ok, y0f, 0).astype(np.int64)
            sw = np.zeros((Hh, Ww), F)
            sc = np.zeros((Hh, Ww, 3), F)
            s1, s2, Nh = np.zeros((Hh, Ww), F), np.zeros((Hh, Ww), F), np.zeros((Hh, Ww), F)
            anyv = np.zeros((Hh, Ww), bool)
            hP, hn = hist["worldPosition"], hist["worldNormal"]
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                b = (wx if dx else F(1) - wx) * (wy if dy else F(1) - wy)
                qx, qy = x0 + dx, y0 + dy
                ins = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hfull)
                ly = qy - (0 if hist.shape[0] == Hfull else row0)
                assert not (ok & ins & ((ly < 0) | (ly >= hist.shape[0]))).any(), "a reprojection tap lies outside the history rows given"
                qx, ly = np.clip(qx, 0, Ww - 1), np.clip(ly, 0, hist.shape[0] - 1)
                q = hist[ly, qx]
                v = ok & ins & (q["filterable"] != 0) & (q["N"] >= F(1)) & (b > 0)
                v &= dot3(N, hn[ly, qx]) >= F(normal_min)
                v &= np.abs(dot3(N, hP[ly, qx] - P)) <= F(plane_max) * t
                sw = np.where(v, sw + b, sw)
                sc = np.where(v[..., None], sc + q["colour"] * b[..., None], sc)
                s1 = np.where(v, s1 + q["m1"] * b, s1)
                s2 = np.where(v, s2 + q["m2"] * b, s2)
                Nh = np.where(v & (Nh < q["N"]), q["N"], Nh)
                anyv |= v
            n1 = Nh + F(1)
            Nn = np.where(anyv, np.where(limit < n1, limit, n1), Nn).astype(F)
            blend = anyv & (Nn != F(1))
            al = F(1) / Nn
            hc, h1, h2 = sc / sw[..., None], s1 / sw, s2 / sw
            ci = np.where(blend[..., None], hc + (e0 - hc) * al[..., None], e0)
            m1 = np.where(blend, h1 + (L - h1) * al, L)
            m2 = np.where(blend, h2 + (LL - h2) * al, LL)
        # variance: temporal where N >= 4, else the 5 x 5 spatial estimate of the current frame
        tv = m2 - m1 * m1
        tv = np.where(F(0) < tv, tv, F(0))
        S0, S1, S2 = np.ones((Hh, Ww), F), L.copy(), LL.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                Lq, ins = _shift(L, dy, dx)
                wn, wz = _weights_nz(N, P, spt, _shift(N, dy, dx)[0], _shift(P, dy, dx)[0], normal_power_log2)
                w = wn * wz
                use = ins & _shift(flt, dy, dx)[0]
                S0 = np.where(use, S0 + w, S0)
                S1 = np.where(use, S1 + Lq * w, S1)
                S2 = np.where(use, S2 + (Lq * Lq) * w, S2)
        M1, M2 = S1 / S0, S2 / S0
        sv = M2 - M1 * M1
        sv = np.where(F(0) < sv, sv, F(0)) * (F(4) / Nn)
        var = np.where(flt, np.where(Nn < F(4), sv, tv), F(0)).astype(F)
        var4 = var.copy()
        e, fb = ci.copy(), ci
        for k in range(int(iterations)):
            s = 1 << k
            lum = luminance(e)
            if sigma_l > 0:
                vb, vw = np.zeros((Hh, Ww), F), np.zeros((Hh, Ww), F)
                for iy, dy in enumerate((-1, 0, 1)):
                    for ix, dx in enumerate((-1, 0, 1)):
                        g = G3[iy] * G3[ix]
                        vq, ins = _shift(var, dy, dx)
                        use = ins & _shift(flt, dy, dx)[0]
                        vb = np.where(use, vb + vq * g, vb)
                        vw = np.where(use, vw + g, vw)
                sl = sigma_l * np.sqrt(vb / vw) + F(1e-4)
            sr = np.zeros(e.shape, F)
            swt, svv = np.zeros((Hh, Ww), F), np.zeros((Hh, Ww), F)
            for iy, dy in enumerate(range(-2, 3)):
                for ix, dx in enumerate(range(-2, 3)):
                    hh = H5[iy] * H5[ix]
                    if dx == 0 and dy == 0:
                        sr = sr + e * hh
                        swt = swt + hh
                        svv = svv + var * (hh * hh)
                        continue
                    eq, ins = _shift(e, dy * s, dx * s)
                    Pq, Nq, fq, lq, vq = (_shift(x, dy * s, dx * s)[0] for x in (P, N, flt, lum, var))
                    wn, wz = _weights_nz(N, P, spt, Nq, Pq, normal_power_log2)
                    if sigma_l > 0:
                        xl = np.abs(lq - lum) / sl
                        wl = F(1) / (F(1) + xl * xl)
                    else:
                        wl = F(1)
                    w = ((wn * wz) * wl) * hh
                    use = ins & fq
                    sr = np.where(use[..., None], sr + eq * w[..., None], sr)
                    swt = np.where(use, swt + w, swt)
                    svv = np.where(use, svv + vq * (w * w), svv)
            e = np.where(flt[..., None], sr / swt[..., None], e)
            var = np.where(flt, svv / (swt * swt), var)
            if k == 0 and feedback:
                fb = e
        out = np.where(flt[..., None], e * d, c) if demodulate_albedo else np.where(flt[..., None], e, c)
        rad = np.empty(accum.shape, dtype=F)
        rad[..., :3] = out
        rad[..., 3] = accum[..., 3] / n
    new = np.zeros((Hh, Ww), dtype=TEMPORAL_DTYPE)
    new["worldPosition"], new["hitDistance"], new["worldNormal"], new["filterable"] = P, t, N, flt.astype(F)
    new["colour"], new["N"], new["m1"], new["m2"], new["variance"] = fb, Nn, m1, m2, var4
    assert rad.dtype == F and fb.dtype == F and m1.dtype == F and var4.dtype == F
    return rad, tonemap_pack(rad), new
