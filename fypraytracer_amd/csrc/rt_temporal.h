// Temporal denoiser (fyprt_denoise_temporal*, include/fyprt.h; DESIGN.md §4 "Temporal denoiser") — gfx950.
// The SVGF structure on top of the spatial denoiser's pieces (rt_denoise.h): the demodulated colour of the frame is blended into a
// per-pixel history that is fetched by reprojecting the primary hit with the camera of the frame denoised before, two luminance moments
// ride along and give a per-pixel variance, and the a-trous iterations scale their luminance stopping function by that variance and
// filter it along.  No reference counterpart; the contract is the header's, binary32 + - * / sqrt and selections in the order written
// there, and tests/temporal_ref.py restates it in numpy bit for bit.
//
//   k_dn_prepare   : the spatial denoiser's (rt_denoise.h), on the band [0, H) — guide record, albedo, e0 | L(e0).
//   k_dt_reproject : one thread per pixel, a wave = an 8 x 8 pixel quad (the four history taps of a wave stay within a few lines).
//                    Gathers up to four 64-byte history records (DtRecord: P.xyz t | n.xyz filterable | colour.rgb N | m1 m2 variance 0),
//                    integrates colour and moments, takes the temporal variance where N >= 4 and, behind a wave-uniform test, the 5 x 5
//                    spatial estimate where N < 4; writes the new history record, the integrated colour | its luminance and the variance.
//   k_dt_iterate   : k_dn_iterate's two forms (STEP > 0: tile + halo staged in LDS, STEP == 0: gathered) on its tile skeleton — dn_tile_pos
//                    from the band's first row and dn_stage (rt_denoise.h) — with the variance in the staged record: dn_stage's hook puts it in the place
//                    of the hit distance in the first quad, which only the centre needs and reads from memory, so the record stays
//                    48 bytes and the LDS table and bank layout of DnTile hold as they are.  The tap loop is its own (dt_tap).  The 3 x 3
//                    variance prefilter reads rows at distance 1, which a tile whose rows lie STEP apart does not hold: nine 4-byte
//                    gathers per pixel.  Iteration 0 also writes its colour into the new history record (feedback).
//   k_dt_moved / k_dt_reproject_motion : object motion (fyprt_denoise_temporal_set_motion), launched only while a vertex snapshot is
//                    pending.  k_dt_moved: one thread per triangle of the edited range, a byte per triangle — do the 18 position and normal
//                    floats of its vertices differ bit-wise between the snapshot and now.  The motion form of the reprojection loads that
//                    byte per filterable pixel and, where it is set, rebuilds the hit's point and shading normal in the snapshot
//                    geometry from its barycentrics in the current triangle (triIdx 16 B, triPos 48 B, three 32-byte snapshot vertices);
//                    a wave that sees no moved triangle pays the byte alone.
// Between the kernels the variance buffer holds -1 for a pixel that is not filterable (the record and the contract say 0 there): the
// prefilter's taps then need no second load for the flag.
// k_dt_reproject* and k_dt_iterate compute the rows of a DnBand as the a-trous set does (rt_denoise.h): the full frame is the band
// [0, H) (fyprt_denoise_temporal*), a group's frame one band per context (fyprt_group_denoise_temporal*, fyprt_multi.h).
#pragma once
#include "rt_denoise.h"
#include "rt_refit.h"

namespace rt {

struct DtCall {                      // what k_dt_reproject needs about the call
    float m[16];                     // projection x view (column-major) of the frame the previous temporal call denoised
    uint32_t haveHistory;
    float limit, normalMin, planeMax, sigmaPlane;
    uint32_t normalPow;
};

struct DtMotion {                    // what the motion form needs beyond: the frame's payload, the moved flags, topology, both geometries
    const Payload* payload; const uint8_t* moved; const uint4* triIdx; const float4* triPos; const DevVertex* snap;
};

RT_DEV float dt_g3(int d) { return d == 0 ? 0.5f : 0.25f; }

// moved[t] for the triangles [first, first + count): any of the 18 position / normal floats of its vertices differs bit-wise
__global__ void __launch_bounds__(256) k_dt_moved(const DevVertex* __restrict__ now, const DevVertex* __restrict__ snap, const uint4* __restrict__ triIdx,
                                                  uint8_t* __restrict__ moved, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= count) return;
    const uint32_t t = first + k;
    const uint4 ix = triIdx[t];
    const uint32_t v[3] = {ix.x, ix.y, ix.z};
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint32_t* a = reinterpret_cast<const uint32_t*>(now + v[j]);
        const uint32_t* b = reinterpret_cast<const uint32_t*>(snap + v[j]);
#pragma unroll
        for (int e = 0; e < 6; ++e) diff |= a[e] ^ b[e];
    }
    moved[t] = diff ? 1 : 0;
}

// The reprojection kernel's body.  MOTION: (Pq, nq) — the point and normal step 2 reprojects and tests with — are the hit's in the
// snapshot geometry where its triangle moved; everything else, and every pixel of an unmoved triangle, is the plain form's arithmetic.
// Computes the rows of `band` (the 16 x 16 tiles count from its first row; the grid covers its height) and takes history taps from the
// rows of `win` only — the band's history window (include/fyprt.h, fyprt_group_denoise_temporal): two wave-uniform bounds in the place
// of the image's.  The single context is the band [0, H) with the window [0, H).  Every buffer is full-size and indexed by the frame's
// pixel; the 5 x 5 estimate reads guide and colour rows beyond the band where the host's peer copies put them.
template <bool MOTION>
RT_DEV void dt_reproject(const DnFrame& fr, const DtCall& tc, const DtMotion& mo, DnBand band, DnBand win, const float4* __restrict__ col0,
                         const float4* __restrict__ histIn, float4* __restrict__ histOut, float4* __restrict__ colOut, float* __restrict__ varOut) {
    const uint32_t tilesX = (fr.W + 15u) / 16u;
    const uint32_t bx = blockIdx.x % tilesX, by = blockIdx.x / tilesX;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int x = (int)(bx * 16u + ((wave & 1u) << 3) + (lane & 7u)), y = (int)(band.rowBegin + by * 16u + ((wave >> 1) << 3) + (lane >> 3));
    if (x >= (int)fr.W || y >= (int)band.rowEnd) return;
    const int W = (int)fr.W, H = (int)fr.H;
    const int winLo = (int)win.rowBegin, winHi = (int)win.rowEnd;
    const size_t i = (size_t)y * fr.W + (size_t)x;
    const float4 g0 = fr.guide[2 * i], g1 = fr.guide[2 * i + 1], ce = col0[i];
    const bool filterable = g1.w != 0.0f;
    const float L = ce.w, LL = L * L;
    float cr = ce.x, cg = ce.y, cb = ce.z, m1 = L, m2 = LL, N = filterable ? 1.0f : 0.0f;
    float Px = g0.x, Py = g0.y, Pz = g0.z, nx = g1.x, ny = g1.y, nz = g1.z;
    if (MOTION) {
        bool moved = false; uint32_t tri = 0;
        if (filterable) {                    // (filterable: k_dn_prepare found the payload's triangle inside the scene)
            tri = (uint32_t)reinterpret_cast<const int32_t*>(mo.payload + i)[9];
            moved = mo.moved[tri] != 0;
        }
        if (moved) {
            const float4* tp = mo.triPos + (size_t)tri * 3;
            const float4 a = tp[0], b = tp[1], c = tp[2];
            const uint4 ix = mo.triIdx[tri];
            const float4* va = reinterpret_cast<const float4*>(mo.snap + ix.x);       // px py pz nx | ny nz u v
            const float4* vb = reinterpret_cast<const float4*>(mo.snap + ix.y);
            const float4* vc = reinterpret_cast<const float4*>(mo.snap + ix.z);
            const float4 a0 = va[0], a1 = va[1], b0 = vb[0], b1 = vb[1], c0 = vc[0], c1 = vc[1];
            const f3 e1 = mk3(b.x - a.x, b.y - a.y, b.z - a.z), e2 = mk3(c.x - a.x, c.y - a.y, c.z - a.z);
            const f3 d = mk3(g0.x - a.x, g0.y - a.y, g0.z - a.z);
            const float d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), p1 = dot(d, e1), p2 = dot(d, e2);
            const float det = d11 * d22 - d12 * d12;
            const float beta = (d22 * p1 - d12 * p2) / det, gamma = (d11 * p2 - d12 * p1) / det, alpha = (1.0f - beta) - gamma;
            Px = (a0.x * alpha + b0.x * beta) + c0.x * gamma;
            Py = (a0.y * alpha + b0.y * beta) + c0.y * gamma;
            Pz = (a0.z * alpha + b0.z * beta) + c0.z * gamma;
            const f3 mm = mk3((a0.w * alpha + b0.w * beta) + c0.w * gamma, (a1.x * alpha + b1.x * beta) + c1.x * gamma,
                              (a1.y * alpha + b1.y * beta) + c1.y * gamma);
            const f3 nn = normalize(mm);
            nx = nn.x; ny = nn.y; nz = nn.z;
        }
    }
    if (filterable && tc.haveHistory) {
        const float* m = tc.m;
        const float clipx = (m[0] * Px + m[4] * Py) + (m[8] * Pz + m[12]);
        const float clipy = (m[1] * Px + m[5] * Py) + (m[9] * Pz + m[13]);
        const float clipw = (m[3] * Px + m[7] * Py) + (m[11] * Pz + m[15]);
        if (clipw > 0.0f) {
            const float sx = ((clipx / clipw) * 0.5f + 0.5f) * (float)fr.W, sy = ((clipy / clipw) * 0.5f + 0.5f) * (float)fr.H;
            if (sx >= -1.0f && sx < (float)fr.W && sy >= -1.0f && sy < (float)fr.H) {
                const float x0f = __builtin_floorf(sx), y0f = __builtin_floorf(sy);
                const float wx = sx - x0f, wy = sy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float planeT = tc.planeMax * g0.w;
                float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f, Nh = 0.0f;
                bool any = false;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int dx = k & 1, dy = k >> 1;
                    const float b = (dx ? wx : 1.0f - wx) * (dy ? wy : 1.0f - wy);
                    const int qx = x0 + dx, qy = y0 + dy;
                    const bool in = qx >= 0 && qy >= winLo && qx < W && qy < winHi;
                    const size_t j = in ? (size_t)qy * fr.W + (size_t)qx : i;          // (outside the image or the window: the centre's own address, selected away)
                    const float4 h0 = histIn[4 * j], h1 = histIn[4 * j + 1], h2 = histIn[4 * j + 2], h3 = histIn[4 * j + 3];
                    const float dn = (nx * h1.x + ny * h1.y) + nz * h1.z;
                    const float ex = h0.x - Px, ey = h0.y - Py, ez = h0.z - Pz;
                    const float dp = __builtin_fabsf((nx * ex + ny * ey) + nz * ez);
                    const bool valid = in && h1.w != 0.0f && h2.w >= 1.0f && b > 0.0f && dn >= tc.normalMin && dp <= planeT;
                    if (valid) {
                        sw = sw + b; sr = sr + h2.x * b; sg = sg + h2.y * b; sb = sb + h2.z * b; s1 = s1 + h3.x * b; s2 = s2 + h3.y * b;
                        Nh = (Nh < h2.w) ? h2.w : Nh; any = true;
                    }
                }
                if (any) {
                    const float n1 = Nh + 1.0f;
                    N = (tc.limit < n1) ? tc.limit : n1;
                    if (N != 1.0f) {                                                     // (history_limit 1: the new sample alone)
                        const float a = 1.0f / N;
                        const float hr = sr / sw, hg = sg / sw, hb = sb / sw, h1m = s1 / sw, h2m = s2 / sw;
                        cr = hr + (ce.x - hr) * a; cg = hg + (ce.y - hg) * a; cb = hb + (ce.z - hb) * a;
                        m1 = h1m + (L - h1m) * a; m2 = h2m + (LL - h2m) * a;
                    }
                }
            }
        }
    }
    float var = 0.0f;
    const bool spatial = filterable && N < 4.0f;
    if (filterable && !spatial) { const float t = m2 - m1 * m1; var = (0.0f < t) ? t : 0.0f; }
    if (__any(spatial ? 1 : 0)) {        // steady state: disocclusions and borders only; a first call: every wave
        if (spatial) {
            const float sigmaPlaneT = tc.sigmaPlane * g0.w;
            float S0 = 1.0f, S1 = L, S2 = LL;
            for (int dy = -2; dy <= 2; ++dy) {
                for (int dx = -2; dx <= 2; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    const int qx = x + dx, qy = y + dy;
                    const bool in = qx >= 0 && qy >= 0 && qx < W && qy < H;
                    const size_t j = in ? (size_t)qy * fr.W + (size_t)qx : i;
                    const float4 q0 = fr.guide[2 * j], q1 = fr.guide[2 * j + 1];
                    const float Lq = reinterpret_cast<const float*>(col0)[4 * j + 3];
                    const float d = (g1.x * q1.x + g1.y * q1.y) + g1.z * q1.z;
                    float wn = (0.0f < d) ? d : 0.0f;
                    for (uint32_t k = 0; k < tc.normalPow; ++k) wn = wn * wn;
                    const float ex = q0.x - g0.x, ey = q0.y - g0.y, ez = q0.z - g0.z;
                    const float xz = __builtin_fabsf((g1.x * ex + g1.y * ey) + g1.z * ez) / sigmaPlaneT;
                    const float w = wn * (1.0f / (1.0f + xz * xz));
                    if (in && q1.w != 0.0f) { S0 = S0 + w; S1 = S1 + Lq * w; S2 = S2 + (Lq * Lq) * w; }
                }
            }
            const float M1 = S1 / S0, M2 = S2 / S0;
            const float t = M2 - M1 * M1;
            var = ((0.0f < t) ? t : 0.0f) * (4.0f / N);
        }
    }
    histOut[4 * i] = g0; histOut[4 * i + 1] = g1;
    histOut[4 * i + 2] = make_float4(cr, cg, cb, N);
    histOut[4 * i + 3] = make_float4(m1, m2, var, 0.0f);
    colOut[i] = make_float4(cr, cg, cb, dn_luminance(cr, cg, cb));
    varOut[i] = filterable ? var : -1.0f;
}

__global__ void __launch_bounds__(256) k_dt_reproject(DnFrame fr, DtCall tc, DnBand band, DnBand win, const float4* __restrict__ col0,
                                                      const float4* __restrict__ histIn, float4* __restrict__ histOut,
                                                      float4* __restrict__ colOut, float* __restrict__ varOut) {
    dt_reproject<false>(fr, tc, DtMotion{}, band, win, col0, histIn, histOut, colOut, varOut);
}
__global__ void __launch_bounds__(256) k_dt_reproject_motion(DnFrame fr, DtCall tc, DtMotion mo, DnBand band, DnBand win, const float4* __restrict__ col0,
                                                             const float4* __restrict__ histIn, float4* __restrict__ histOut,
                                                             float4* __restrict__ colOut, float* __restrict__ varOut) {
    dt_reproject<true>(fr, tc, mo, band, win, col0, histIn, histOut, colOut, varOut);
}
inline uint32_t dt_reproject_grid(uint32_t W, uint32_t rows) { return ((W + 15u) / 16u) * ((rows + 15u) / 16u); }

struct DtSums { float r, g, b, w, v; };
// dn_tap with the centre's own luminance scale and the variance sum; vq = the tap's variance
RT_DEV void dt_tap(const DnIter& it, const float4& c0, const float4& c1, float sigmaPlaneT, float lumP, float sigmaLp, const float4& g0,
                   const float4& g1, const float4& cq, float vq, bool use, float hh, DtSums& s) {
    const float d = (c1.x * g1.x + c1.y * g1.y) + c1.z * g1.z;
    float wn = (0.0f < d) ? d : 0.0f;
    for (uint32_t k = 0; k < it.normalPow; ++k) wn = wn * wn;
    const float dx = g0.x - c0.x, dy = g0.y - c0.y, dz = g0.z - c0.z;
    const float xz = __builtin_fabsf((c1.x * dx + c1.y * dy) + c1.z * dz) / sigmaPlaneT;
    const float wz = 1.0f / (1.0f + xz * xz);
    float wl = 1.0f;
    if (it.lumOn) { const float xl = __builtin_fabsf(cq.w - lumP) / sigmaLp; wl = 1.0f / (1.0f + xl * xl); }
    const float w = ((wn * wz) * wl) * hh;
    if (use) { s.r = s.r + cq.x * w; s.g = s.g + cq.y * w; s.b = s.b + cq.z * w; s.w = s.w + w; s.v = s.v + vq * (w * w); }
}

// Grid, tiles, staging and the band as k_dn_iterate<STEP> (dn_grid of the band's height, DnTile, dn_tile_pos from band.rowBegin, dn_stage):
// pixels below band.rowEnd leave, and so does the feedback write; taps, and the prefilter's, read the colour, variance (-1 = not
// filterable, as its owner wrote it) and guide rows beyond the band where the host's peer copies put them.  it.sigmaL = sigma_luminance
// itself (the variance carries the scale).  histOut: the new history, or null — iteration 0 of a call with feedback writes its colour there.
template <int STEP>
__global__ void __launch_bounds__(256) k_dt_iterate(DnFrame fr, DnIter it, DnBand band, const float4* __restrict__ colIn, float4* __restrict__ colOut,
                                                    const float* __restrict__ varIn, float* __restrict__ varOut, float4* __restrict__ histOut) {
    using T = DnTile<STEP>;
    __shared__ float4 sG0[T::RECORDS], sG1[T::RECORDS], sC[T::RECORDS];     // sG0.w = the variance (not the hit distance)
    const DnTilePos tp = dn_tile_pos<STEP>(fr.W, (int)band.rowBegin);
    if (tp.yBase >= (int)band.rowEnd) return;                                    // (the whole workgroup: before anything is staged)
    const int lx = tp.lx, ly = tp.ly, x = tp.x, y = tp.y;
    if (STEP) dn_stage<STEP>(fr, colIn, tp.xBase, tp.yBase, sG0, sG1, sC, [&](float4& g0, size_t j) { g0.w = varIn[j]; });
    if (x >= (int)fr.W || y >= (int)band.rowEnd) return;
    const uint32_t i = (uint32_t)y * fr.W + (uint32_t)x;
    const int lc = (ly + 2) * T::STRIDE + lx + 2 * T::S;
    const float4 c0 = STEP ? sG0[lc] : fr.guide[2 * (size_t)i];
    const float4 c1 = STEP ? sG1[lc] : fr.guide[2 * (size_t)i + 1];
    const float4 cp = STEP ? sC[lc] : colIn[i];
    const bool filterable = c1.w != 0.0f;
    f3 e = mk3(cp.x, cp.y, cp.z);
    float var = -1.0f;
    if (filterable) {
        const float tP = STEP ? reinterpret_cast<const float*>(fr.guide)[8 * (size_t)i + 3] : c0.w;
        const float vP = STEP ? c0.w : varIn[i];
        const float sigmaPlaneT = it.sigmaPlane * tP;
        float sigmaLp = 1.0f;
        if (it.lumOn) {                      // 3 x 3 Gaussian of the variance, filterable taps inside the image, the centre among them
            float vb = 0.0f, vw = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const float g = dt_g3(dy) * dt_g3(dx);
                    const int qx = x + dx, qy = y + dy;
                    const bool in = qx >= 0 && qy >= 0 && qx < (int)fr.W && qy < (int)fr.H;
                    const float v = (dx == 0 && dy == 0) ? vP : varIn[in ? (size_t)qy * fr.W + (size_t)qx : (size_t)i];
                    if (in && !(v < 0.0f)) { vb = vb + v * g; vw = vw + g; }
                }
            }
            sigmaLp = it.sigmaL * sqrt_exact(vb / vw) + 1e-4f;
        }
        DtSums s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float hh = dn_h(dy) * dn_h(dx);
                if (dx == 0 && dy == 0) {
                    s.r = s.r + cp.x * hh; s.g = s.g + cp.y * hh; s.b = s.b + cp.z * hh; s.w = s.w + hh; s.v = s.v + vP * (hh * hh);
                    continue;
                }
                if (STEP) {
                    const int k = lc + dy * T::STRIDE + dx * T::S;
                    const float4 g0 = sG0[k], g1 = sG1[k];
                    dt_tap(it, c0, c1, sigmaPlaneT, cp.w, sigmaLp, g0, g1, sC[k], g0.w, g1.w != 0.0f, hh, s);
                } else {
                    const int qx = x + dx * it.step, qy = y + dy * it.step;
                    const bool in = qx >= 0 && qy >= 0 && qx < (int)fr.W && qy < (int)fr.H;
                    const size_t j = in ? (size_t)qy * fr.W + (size_t)qx : (size_t)i;   // (outside: the centre's own address, selected away)
                    const float4 g1 = fr.guide[2 * j + 1];
                    dt_tap(it, c0, c1, sigmaPlaneT, cp.w, sigmaLp, fr.guide[2 * j], g1, colIn[j], varIn[j], in && g1.w != 0.0f, hh, s);
                }
            }
        }
        e = mk3(s.r / s.w, s.g / s.w, s.b / s.w);
        var = s.v / (s.w * s.w);
    }
    if (histOut) { float* h = reinterpret_cast<float*>(histOut + 4 * (size_t)i + 2); h[0] = e.x; h[1] = e.y; h[2] = e.z; }
    if (it.last) dn_output(fr, i, e, filterable);
    else { colOut[i] = make_float4(e.x, e.y, e.z, dn_luminance(e.x, e.y, e.z)); varOut[i] = var; }
}

}  // namespace rt
