"""numpy restatement of fyprt_group_denoise_temporal's contract (include/fyprt.h, multi-GPU section) — a test helper, not a test.

The contract is fyprt_denoise_temporal's on the stitched frame with one more term in step 2: a history tap of a pixel is valid only if
its row lies in the HISTORY WINDOW of the band that owns the pixel — band [b, e): rows [max(0, b - R), min(H, e + R)), R =
min(history_rows, H).  Steps 4 and 5 read the real neighbours across band borders: what a neighbour's owner computed under its own window.

group_temporal_ref evaluates exactly that: windowed_temporal_ref, temporal_ref's text with a window per row.
band_masked_ref is the shorter recipe — temporal_ref once per band on the whole frame with the history's records outside the band's
window made not filterable, the band's rows kept.  It gives a pixel's own reprojection (N, the moments, the variance of step 4, the
integrated colour) exactly, but a neighbour beyond the border then enters the filter as the WRONG band's window leaves it, so its
filtered colours are the contract's only where no such neighbour differs: always when the windows hold every tap (then both are plain
temporal_ref), and with iterations = 0.  tests/test_group_temporal_cpu.py pins all three relations."""
import numpy as np

from denoise_ref import H5, _shift, luminance, tonemap_pack
from fypraytracer_amd.capi import TEMPORAL_DTYPE
from temporal_ref import G3, F, _weights_nz, dot3, temporal_ref


def history_window(b, e, history_rows, H):
    R = min(int(history_rows), H)
    return max(0, b - R), min(H, e + R)


def windowed_temporal_ref(accum, payload, albedo, n, M_prev, hist, win_lo, win_hi, iterations=5, sigma_luminance=4.0, sigma_plane=0.01,
                          normal_power_log2=6, demodulate_albedo=1, history_limit=32, normal_min=0.9, plane_max=0.02, feedback=1):
    """temporal_ref (tests/temporal_ref.py) with the one term fyprt_group_denoise_temporal adds to step 2: a history tap of a pixel in row y
    is valid only if its row lies in [win_lo[y], win_hi[y]).  Everything else is temporal_ref's text, operation for operation (the
    partial-frame arguments left out): with win_lo = 0 and win_hi = H it returns temporal_ref's bits, which the CPU test pins."""
    win_lo = np.asarray(win_lo, dtype=np.int64)[:, None]
    win_hi = np.asarray(win_hi, dtype=np.int64)[:, None]
    accum = np.ascontiguousarray(accum, dtype=F)
    albedo = np.ascontiguousarray(albedo, dtype=F)
    Hh, Ww = accum.shape[:2]
    Hfull = Hh
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
                ins = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hfull) & (qy >= win_lo) & (qy < win_hi)
                ly = qy
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


def group_temporal_ref(accum, payload, albedo, n, M_prev, hist, bounds, history_rows, **par):
    """accum, payload, albedo, n, M_prev, hist and the parameters as temporal_ref, of the stitched frame; bounds: the group's row table.
    Returns the stitched (radiance4, rgba8, history record array)."""
    H = accum.shape[0]
    lo, hi = np.zeros(H, np.int64), np.zeros(H, np.int64)
    for b, e in zip(bounds, bounds[1:]):
        lo[b:e], hi[b:e] = history_window(b, e, history_rows, H)
    if hist is None or ((lo == 0).all() and (hi == H).all()):
        return temporal_ref(accum, payload, albedo, n, M_prev, hist, **par)       # no tap is cut: the single context's call itself
    return windowed_temporal_ref(accum, payload, albedo, n, M_prev, hist, lo, hi, **par)


def band_masked_ref(accum, payload, albedo, n, M_prev, hist, bounds, history_rows, **par):
    """temporal_ref per band on a copy of the history whose records outside the band's window are not filterable; the band's rows of the
    three results, stitched.  See the module text for what it equals."""
    H = accum.shape[0]
    whole, out = None, None
    for b, e in zip(bounds, bounds[1:]):
        lo, hi = history_window(b, e, history_rows, H)
        if hist is None or (lo == 0 and hi == H):
            if whole is None:
                whole = temporal_ref(accum, payload, albedo, n, M_prev, hist, **par)
            res = whole
        else:
            h = hist.copy()
            h["filterable"][:lo] = 0
            h["filterable"][hi:] = 0
            res = temporal_ref(accum, payload, albedo, n, M_prev, h, **par)
        if out is None:
            out = tuple(np.zeros_like(r) for r in res)
        for o, r in zip(out, res):
            o[b:e] = r[b:e]
    return out


def rows_needed(payload, albedo, M_prev, bounds):
    """Per pixel (H x W, int): how many rows beyond its band the two history tap rows y0, y0 + 1 of its reprojection reach (0: both inside
    the band), for every filterable pixel whose reprojection with M_prev is in range (clip.w > 0, -1 <= sx < W, -1 <= sy < H); 0 for
    every other pixel.  Tap rows outside the image are never valid and do not count.  float64: for choosing and asserting test
    conditions only, not part of the contract."""
    H, W = albedo.shape[:2]
    M = np.asarray(M_prev, dtype=np.float64).reshape(4, 4)              # [col][row]
    P = np.concatenate([np.asarray(payload["worldPosition"], dtype=np.float64), np.ones((H, W, 1))], axis=-1)
    clip = np.einsum("cr,hwc->hwr", M, P)
    with np.errstate(all="ignore"):
        sx = (clip[..., 0] / clip[..., 3] * 0.5 + 0.5) * W
        sy = (clip[..., 1] / clip[..., 3] * 0.5 + 0.5) * H
    ok = (albedo[..., 3] != 0) & (clip[..., 3] > 0) & (sx >= -1) & (sx < W) & (sy >= -1) & (sy < H)
    y0 = np.floor(np.where(ok, sy, 0)).astype(np.int64)
    top, bottom = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    need = np.zeros((H, W), dtype=np.int64)
    for b, e in zip(bounds, bounds[1:]):
        reach = np.maximum(np.maximum(b - top[b:e], bottom[b:e] - (e - 1)), 0)
        need[b:e] = np.where(ok[b:e], reach, 0)
    return need
