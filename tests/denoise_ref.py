"""numpy restatement of the denoiser's contract (include/fyprt.h, "denoiser") — a test helper, not a test.

Every operation is binary32 in the header's order: arrays stay float32, constants are float32 scalars, max(a, b) is
where(a < b, b, a), a skipped tap is selected away (never multiplied by zero) and the sums run in tap order from +0.  The device
kernels (fypraytracer_amd/csrc/rt_denoise.h) must reproduce the result bit for bit."""
import ctypes as C

import numpy as np

F = np.float32
H5 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1)


def assert_numpy_keeps_subnormals():
    """The contract's weights reach subnormals (n.n' to the 64th): the process must not flush them (some libraries set FTZ / DAZ)."""
    tiny = np.full(4, 1e-20, dtype=F)
    prod = tiny * tiny
    assert prod.dtype == F and (prod > 0).all() and (prod < np.finfo(F).tiny).all(), "numpy flushes float32 subnormals in this process"
    assert ((prod / F(2)) * F(2) == prod).all()


def luminance(e):
    return (F(0.2126) * e[..., 0] + F(0.7152) * e[..., 1]) + F(0.0722) * e[..., 2]


def guides_from_scene(scene, payload, sample_texture=None):
    """(albedo H x W x 4: rgb = a_p, w = 1 filterable / 0 not, rgb 0 where not filterable) from a payload array (H x W, PAYLOAD_DTYPE) and
    the scene's materials.  `sample_texture(pixels, u, v) -> uint32 ABGR8` is needed for materials with an albedo map."""
    mats = scene.materials_array()
    tri = payload["objectIndex"]
    hit = tri >= 0
    mi = scene.triangles["materialIndex"][np.where(hit, tri, 0)]
    m = mats[mi]
    em = m["emissionColor"].astype(F) * m["emissionPower"].astype(F)[..., None]
    length = np.sqrt((em[..., 0] * em[..., 0] + em[..., 1] * em[..., 1]) + em[..., 2] * em[..., 2])
    flag = hit & ~(length > 0)
    out = np.zeros(tri.shape + (4,), dtype=F)
    out[..., :3] = m["albedo"]
    use_map = (m["isUseAlbedoMap"] & 0xFF).astype(bool) & (m["albedoMapIndex"] < len(scene.textures)) & flag
    for y, x in zip(*np.nonzero(use_map)):
        px = np.ascontiguousarray(scene.textures[int(m["albedoMapIndex"][y, x])], dtype=np.uint32)
        p = int(sample_texture(px, float(payload["u"][y, x]), float(payload["v"][y, x])))
        out[y, x, :3] = [F(p & 0xFF) * (F(1) / F(255)), F((p >> 8) & 0xFF) * (F(1) / F(255)), F((p >> 16) & 0xFF) * (F(1) / F(255))]
    out[~flag, :3] = 0
    out[..., 3] = flag
    return out


def oracle_texture_sampler(oracle_lib):
    """sample_texture for guides_from_scene over the oracle library's orc_sample_bilinear (Texture::SampleBilinear, re-quantised)."""
    def sample(px, u, v):
        return oracle_lib.orc_sample_bilinear(px.ctypes.data_as(C.c_void_p), px.shape[1], px.shape[0], u, v)
    return sample


def tonemap_pack(rad4):
    """The frame epilogue's tonemap / clamp / pack of a float32 H x W x 4 image -> uint32 ABGR8."""
    with np.errstate(all="ignore"):
        a = rad4 / (rad4 + np.array([1, 1, 1, 0], dtype=F))
        a = np.where(a < 0, F(0), a)            # gmax(x, 0) = (x < 0) ? 0 : x
        a = np.where(F(1) < a, F(1), a)         # gmin(x, 1) = (1 < x) ? 1 : x
        s = a * F(255)
        q = np.where(~(s >= 0), 0, np.where(s >= F(255), 255, np.nan_to_num(s, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64))).astype(np.uint32)
    return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (q[..., 3] << 24)


def _shift(a, dy, dx):
    """a[y + dy, x + dx] with clamped indices, and the mask of taps inside the image."""
    Hh, Ww = a.shape[:2]
    ys, xs = np.arange(Hh) + dy, np.arange(Ww) + dx
    inside = ((ys >= 0) & (ys < Hh))[:, None] & ((xs >= 0) & (xs < Ww))[None, :]
    return a[np.clip(ys, 0, Hh - 1)][:, np.clip(xs, 0, Ww - 1)], inside


def denoise_ref(accum, payload, albedo, n, iterations=5, sigma_luminance=4.0, sigma_plane=0.01, normal_power_log2=6, demodulate_albedo=1):
    """accum: H x W x 4 float32 running sum; payload: H x W PAYLOAD_DTYPE; albedo: H x W x 4 (rgb, filterable flag); n: the frame index the
    frame was rendered with.  Returns (radiance4 H x W x 4 float32, rgba8 H x W uint32)."""
    accum = np.ascontiguousarray(accum, dtype=F)
    albedo = np.ascontiguousarray(albedo, dtype=F)
    n = F(n)
    sigma_l, sigma_p = F(sigma_luminance), F(sigma_plane)
    with np.errstate(all="ignore"):
        c = accum[..., :3] / n
        flt = albedo[..., 3] != 0
        a = albedo[..., :3]
        d = np.where(a < F(1e-3), F(1e-3), a) if demodulate_albedo else np.ones_like(a)
        e = np.where(flt[..., None], c / d, c) if demodulate_albedo else c.copy()
        P = np.ascontiguousarray(payload["worldPosition"], dtype=F)
        N = np.ascontiguousarray(payload["worldNormal"], dtype=F)
        spt = sigma_p * np.ascontiguousarray(payload["hitDistance"], dtype=F)
        for k in range(int(iterations)):
            s = 1 << k
            sigma_k = sigma_l * F(2.0 ** -k)
            lum = luminance(e)
            sr = np.zeros(e.shape, dtype=F)
            sw = np.zeros(e.shape[:2], dtype=F)
            for iy, dy in enumerate(range(-2, 3)):
                for ix, dx in enumerate(range(-2, 3)):
                    hh = H5[iy] * H5[ix]
                    if dx == 0 and dy == 0:
                        sr = sr + e * hh
                        sw = sw + hh
                        continue
                    eq, inside = _shift(e, dy * s, dx * s)
                    Pq, Nq, fq, lq = _shift(P, dy * s, dx * s)[0], _shift(N, dy * s, dx * s)[0], _shift(flt, dy * s, dx * s)[0], _shift(lum, dy * s, dx * s)[0]
                    dot = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    wn = np.where(F(0) < dot, dot, F(0))
                    for _ in range(int(normal_power_log2)):
                        wn = wn * wn
                    D = Pq - P
                    xz = np.abs((N[..., 0] * D[..., 0] + N[..., 1] * D[..., 1]) + N[..., 2] * D[..., 2]) / spt
                    wz = F(1) / (F(1) + xz * xz)
                    if sigma_l > 0:
                        xl = np.abs(lq - lum) / sigma_k
                        wl = F(1) / (F(1) + xl * xl)
                    else:
                        wl = F(1)
                    w = ((wn * wz) * wl) * hh
                    use = inside & fq
                    sr = np.where(use[..., None], sr + eq * w[..., None], sr)
                    sw = np.where(use, sw + w, sw)
            e = np.where(flt[..., None], sr / sw[..., None], e)
        out = np.where(flt[..., None], e * d, c) if demodulate_albedo else np.where(flt[..., None], e, c)
        rad = np.empty(accum.shape, dtype=F)
        rad[..., :3] = out
        rad[..., 3] = accum[..., 3] / n
    assert rad.dtype == F
    return rad, tonemap_pack(rad)
