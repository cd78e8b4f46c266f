"""numpy restatement of the temporal denoiser's contract with object motion (include/fyprt.h, "temporal denoiser" and
fyprt_denoise_temporal_set_motion) — a test helper, not a test.

temporal_ref.py's contract with step 2 fed from (P', n'): where a snapshot is pending and the pixel's triangle moved, the hit's point and
shading normal rebuilt in the snapshot geometry from its barycentrics in the current triangle; P_p, n_p otherwise.  Same commitments as
there: every operation binary32 in the header's order, selections instead of multiplications by zero, sums in tap order from +0.  The
device kernels (fypraytracer_amd/csrc/rt_temporal.h) must reproduce radiance, image and history record bit for bit."""
import numpy as np

from denoise_ref import H5, _shift, luminance, tonemap_pack
from fypraytracer_amd.capi import TEMPORAL_DTYPE
from temporal_ref import G3, _weights_nz, dot3

F = np.float32


def moved_triangles(triangles, verts_now, verts_prev):
    """Per triangle: any of the 18 position / normal floats of its three vertices differs bit-wise between the two vertex sets."""
    def bits(v):
        return np.concatenate([np.ascontiguousarray(v["position"], dtype=F), np.ascontiguousarray(v["normal"], dtype=F)], axis=1).view(np.uint32)
    vm = (bits(verts_now) != bits(verts_prev)).any(axis=1)
    return vm[triangles["v0"]] | vm[triangles["v1"]] | vm[triangles["v2"]]


def previous_hit(P, N, flt, tri, triangles, verts_now, verts_prev):
    """(P', n', moved mask) of the contract: per pixel the point and normal step 2 works with."""
    mt = moved_triangles(triangles, verts_now, verts_prev)
    ok = flt & (tri >= 0) & (tri < len(triangles))
    t = np.where(ok, tri, 0)
    mv = ok & mt[t]
    ix = [triangles[k][t].astype(np.int64) for k in ("v0", "v1", "v2")]
    pn, pp, nn = verts_now["position"].astype(F), verts_prev["position"].astype(F), verts_prev["normal"].astype(F)
    a, b, c = (pn[i] for i in ix)
    e1, e2, d = b - a, c - a, P - a
    d11, d12, d22, p1, p2 = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2), dot3(d, e1), dot3(d, e2)
    det = d11 * d22 - d12 * d12
    be = (d22 * p1 - d12 * p2) / det
    ga = (d11 * p2 - d12 * p1) / det
    al = (F(1) - be) - ga
    al, be, ga = al[..., None], be[..., None], ga[..., None]
    Pm = (pp[ix[0]] * al + pp[ix[1]] * be) + pp[ix[2]] * ga
    m = (nn[ix[0]] * al + nn[ix[1]] * be) + nn[ix[2]] * ga
    nm = m * (F(1) / np.sqrt(dot3(m, m)))[..., None]
    assert Pm.dtype == F and nm.dtype == F
    return np.where(mv[..., None], Pm, P), np.where(mv[..., None], nm, N), mv


def temporal_motion_ref(accum, payload, albedo, n, M_prev, hist, triangles=None, verts_now=None, verts_prev=None, iterations=5,
                        sigma_luminance=4.0, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1, history_limit=32, normal_min=0.9,
                        plane_max=0.02, feedback=1):
    """Arguments and result as temporal_ref (whole frames only); triangles (TRIANGLE_DTYPE), verts_now, verts_prev (VERTEX_DTYPE): the
    scene's topology, its world vertices when the frame was rendered and the snapshot — the world vertices of the frame the previous call
    denoised — or None when no snapshot is pending."""
    accum = np.ascontiguousarray(accum, dtype=F)
    albedo = np.ascontiguousarray(albedo, dtype=F)
    Hh, Ww = accum.shape[:2]
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
            Pr, Nr = P, N
            if verts_prev is not None:
                Pr, Nr, _ = previous_hit(P, N, flt, payload["objectIndex"], triangles, verts_now, verts_prev)
            M = np.asarray(M_prev, dtype=F).reshape(4, 4)
            cl = [(M[0, r] * Pr[..., 0] + M[1, r] * Pr[..., 1]) + (M[2, r] * Pr[..., 2] + M[3, r]) for r in (0, 1, 3)]
            ok = flt & (cl[2] > 0)
            sx = ((cl[0] / cl[2]) * F(0.5) + F(0.5)) * F(Ww)
            sy = ((cl[1] / cl[2]) * F(0.5) + F(0.5)) * F(Hh)
            ok &= (sx >= F(-1)) & (sx < F(Ww)) & (sy >= F(-1)) & (sy < F(Hh))
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
                ins = (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                qx, qy = np.clip(qx, 0, Ww - 1), np.clip(qy, 0, Hh - 1)
                q = hist[qy, qx]
                v = ok & ins & (q["filterable"] != 0) & (q["N"] >= F(1)) & (b > 0)
                v &= dot3(Nr, hn[qy, qx]) >= F(normal_min)
                v &= np.abs(dot3(Nr, hP[qy, qx] - Pr)) <= F(plane_max) * t
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
