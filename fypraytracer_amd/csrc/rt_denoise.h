// Edge-avoiding denoiser of a rendered frame (fyprt_denoise*, include/fyprt.h; DESIGN.md §4 "Denoiser") — gfx950.
// An a-trous wavelet filter: `iterations` passes of a 5x5 B3-spline stencil dilated by 2^k, every tap weighted by rational
// (Lorentzian) stopping functions of the normals, of the distance to the centre's tangent plane and of the luminance, on the frame's
// radiance divided by the primary hit's albedo.  No new reference counterpart; the contract is the header's, in binary32 + - * / and
// selections only, every operation in the order written there (the build has -ffp-contract=off, IEEE division, fp32 denormals), so a
// numpy restatement (tests/denoise_ref.py) gives the same bits.
//
//   k_dn_prepare : payload (40 B records) + accumulation -> an aligned 32-byte guide record per pixel (P.xyz, t | n.xyz, filterable),
//                  the albedo buffer (FYPRT_BUF_ALBEDO) and the demodulated colour e0 | its luminance.  The one gather into triShade /
//                  materials / textures per pixel happens here, not per tap.
//   k_dn_iterate : one launch per iteration, ping-pong colour buffers, 16-byte loads only.  STEP > 0: a tile whose rows lie STEP image
//                  rows apart and its halo are staged in LDS in 48-byte records (DnTile) and the 25 taps are ds_read_b128;
//                  STEP == 0: the taps are gathered from memory at a run-time step (the form for steps beyond the staged ones, and the
//                  correctness anchor).  The sums run in the contract's tap order in both forms.
//                  The last iteration remodulates, tonemaps and packs instead of writing the colour buffer.
//   k_dn_finish  : the same epilogue alone, for iterations == 0.
// Every kernel computes the rows [rowBegin, rowEnd) of a DnBand: the full frame is the band [0, H) (fyprt_denoise*), a frame split over
// several contexts one band each (fyprt_group_denoise, fyprt_multi.h).  The buffers stay full-size: the taps beyond a band read the halo
// rows where the host's peer copies put them.  dn_tile_pos and dn_stage — the thread-to-pixel mapping and the LDS staging of a tile —
// are shared with the temporal denoiser's iteration (rt_temporal.h: k_dt_iterate).
#pragma once
#include "rt_device.h"

namespace rt {

struct DnFrame {                     // what every denoise kernel reads about the frame and the call
    uint32_t W, H;
    float frameIndex;                // n: the frame index the last frame was rendered with (the divisor of its epilogue)
    uint32_t demodulate;
    const float4* accum;             // the frame's running sum
    float4* guide;                   // 2 x float4 per pixel: P.xyz, t | n.xyz, filterable (1.0f / 0.0f)
    float4* albedo;                  // a.rgb, filterable (1.0f / 0.0f)
    uint32_t* rgba8; float4* radiance4;   // the call's outputs (device memory; either may be null)
};
struct DnIter { int32_t step; float sigmaL; uint32_t lumOn; float sigmaPlane; uint32_t normalPow; uint32_t last; };

// Tile of a k_dn_iterate<STEP> workgroup (256 threads): TX contiguous columns x TY rows that lie STEP image rows apart — the taps of
// such a tile are the tile shifted by whole columns / tile rows, so its halo is 2 * STEP columns and 2 tile rows either side and the
// staged region is (TX + 4 STEP) x (TY + 4) records.  Steps 1 and 2: 16 x 16 (one 8 x 8 quad per wave; 20 x 20 and 24 x 20 records);
// larger steps: 64 x 4 (one row per wave; 80 ... 192 x 8 records), whose rows stay long against the 4 STEP halo columns.  The gather
// form (STEP 0) uses the dense 16 x 16 tile.
template <int STEP> struct DnTile {
    static constexpr int S = STEP ? STEP : 1;                 // row spacing of the tile
    static constexpr int TX = STEP > 2 ? 64 : 16, TY = 256 / TX;
    static constexpr int RW = TX + 4 * S, RH = TY + 4;
    // row stride (records) of the staged region.  16 x 16: with 24 the four 16-lane groups of a wave's ds_read_b128 (two half-rows of 4
    // records from four tile rows) fall on disjoint banks, with 20 they do not; 64 x 4: a wave reads 64 consecutive records, any stride
    static constexpr int STRIDE = STEP > 2 ? RW : 24;
    static constexpr int RECORDS = STEP ? RH * STRIDE : 1;
};

RT_DEV float dn_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// remodulate, write radiance4, tonemap / clamp / pack as the frame's epilogue does (rt_kernels.h: epilogue)
RT_DEV void dn_output(const DnFrame& fr, uint32_t i, f3 e, bool filterable) {
    f3 out = e;
    if (filterable && fr.demodulate) {
        const float4 a = fr.albedo[i];
        out = mk3(e.x * gmax(a.x, 1e-3f), e.y * gmax(a.y, 1e-3f), e.z * gmax(a.z, 1e-3f));
    }
    const float alpha = fr.accum[i].w / fr.frameIndex;
    if (fr.radiance4) fr.radiance4[i] = make_float4(out.x, out.y, out.z, alpha);
    if (fr.rgba8) {
        f4 a = mk4(out.x / (out.x + 1.0f), out.y / (out.y + 1.0f), out.z / (out.z + 1.0f), alpha / (alpha + 0.0f));
        a = mk4(gclamp(a.x, 0.0f, 1.0f), gclamp(a.y, 0.0f, 1.0f), gclamp(a.z, 0.0f, 1.0f), gclamp(a.w, 0.0f, 1.0f));
        fr.rgba8[i] = pack_abgr(a);
    }
}

// one pixel of k_dn_prepare
RT_DEV void dn_prepare_pixel(const DevScene& sc, const DnFrame& fr, const Payload* __restrict__ payload, float4* __restrict__ col0, uint32_t i) {
    const float2* q = reinterpret_cast<const float2*>(payload + i);          // 40-byte records: 8-byte aligned
    const float2 p0 = q[0], p1 = q[1], p2 = q[2], p3 = q[3], p4 = q[4];      // t px | py pz | nx ny | nz u | v objectIndex
    const float4 acc = fr.accum[i];
    f3 c = mk3(acc.x / fr.frameIndex, acc.y / fr.frameIndex, acc.z / fr.frameIndex);
    const int32_t tri = __float_as_int(p4.y);
    bool filterable = false; f3 a = mk3(0.0f, 0.0f, 0.0f);
    if (tri >= 0 && (uint32_t)tri < sc.triCount) {
        const Mat m = load_mat(sc, tri_material(sc, tri));
        if (!(length(emission(m)) > 0.0f)) { filterable = true; a = sample_albedo(sc, m, p3.y, p4.x); }
    }
    if (filterable && fr.demodulate) c = mk3(c.x / gmax(a.x, 1e-3f), c.y / gmax(a.y, 1e-3f), c.z / gmax(a.z, 1e-3f));
    const float flag = filterable ? 1.0f : 0.0f;
    fr.guide[2 * (size_t)i] = make_float4(p0.y, p1.x, p1.y, p0.x);
    fr.guide[2 * (size_t)i + 1] = make_float4(p2.x, p2.y, p3.x, flag);
    fr.albedo[i] = make_float4(a.x, a.y, a.z, flag);
    col0[i] = make_float4(c.x, c.y, c.z, dn_luminance(c.x, c.y, c.z));
}
// rows [rowBegin, rowEnd) of a frame: all of them, or those of a context whose other rows belong to other contexts (rowBegin < rowEnd <= H)
struct DnBand { uint32_t rowBegin, rowEnd; };
__global__ void __launch_bounds__(256) k_dn_prepare(DevScene sc, DnFrame fr, DnBand band, const Payload* __restrict__ payload, float4* __restrict__ col0) {
    const uint32_t i = band.rowBegin * fr.W + blockIdx.x * 256u + threadIdx.x;
    if (i >= band.rowEnd * fr.W) return;
    dn_prepare_pixel(sc, fr, payload, col0, i);
}

struct DnSums { float r, g, b, w; };
// one tap of a filterable centre: (g0, g1, cq) = the tap's guide record and colour | luminance; `use` = inside the image and filterable
RT_DEV void dn_tap(const DnIter& it, const float4& c0, const float4& c1, float sigmaPlaneT, float lumP, const float4& g0, const float4& g1,
                   const float4& cq, bool use, float hh, DnSums& s) {
    const float d = (c1.x * g1.x + c1.y * g1.y) + c1.z * g1.z;
    float wn = (0.0f < d) ? d : 0.0f;
    for (uint32_t k = 0; k < it.normalPow; ++k) wn = wn * wn;
    const float dx = g0.x - c0.x, dy = g0.y - c0.y, dz = g0.z - c0.z;
    const float xz = __builtin_fabsf((c1.x * dx + c1.y * dy) + c1.z * dz) / sigmaPlaneT;
    const float wz = 1.0f / (1.0f + xz * xz);
    float wl = 1.0f;
    if (it.lumOn) { const float xl = __builtin_fabsf(cq.w - lumP) / it.sigmaL; wl = 1.0f / (1.0f + xl * xl); }
    const float w = ((wn * wz) * wl) * hh;
    if (use) { s.r = s.r + cq.x * w; s.g = s.g + cq.y * w; s.b = s.b + cq.z * w; s.w = s.w + w; }
}
RT_DEV float dn_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// Where a thread of workgroup blockIdx.x stands: the tile's first column and row (xBase, yBase), the thread's place in the tile (lx, ly)
// and its pixel (x, y).  Grid: tiles across x groups of TY * S rows x S row phases (dn_grid), counted from firstRow.  16 x 16 tiles: one
// 8 x 8 quad per wave; 64 x 4 tiles: one row per wave.
struct DnTilePos { int xBase, yBase, lx, ly, x, y; };
template <int STEP> RT_DEV DnTilePos dn_tile_pos(uint32_t W, int firstRow) {
    using T = DnTile<STEP>;
    const uint32_t tilesX = (W + (T::TX - 1)) / T::TX;
    const uint32_t bx = blockIdx.x % tilesX, rest = blockIdx.x / tilesX;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    DnTilePos p;
    p.xBase = (int)bx * T::TX; p.yBase = firstRow + (int)(rest / T::S) * (T::TY * T::S) + (int)(rest % T::S);
    p.lx = T::TX == 64 ? (int)lane : (int)(((wave & 1u) << 3) + (lane & 7u));
    p.ly = T::TX == 64 ? (int)wave : (int)(((wave >> 1) << 3) + (lane >> 3));
    p.x = p.xBase + p.lx; p.y = p.yBase + p.ly * T::S;
    return p;
}
// Stages the tile at (xBase, yBase) and its halo: guide records into sG0 / sG1, colour | luminance into sC, and waits for the workgroup.
// A record outside the image is flagged unusable (sG1.w = 0).  g0w(g0, j): what the caller keeps in sG0.w of pixel j.
template <int STEP, class G0W>
RT_DEV void dn_stage(const DnFrame& fr, const float4* __restrict__ colIn, int xBase, int yBase, float4* sG0, float4* sG1, float4* sC, G0W g0w) {
    using T = DnTile<STEP>;
    for (int k = (int)threadIdx.x; k < T::RW * T::RH; k += 256) {
        const int rx = k % T::RW, ry = k / T::RW, gx = xBase - 2 * T::S + rx, gy = yBase + (ry - 2) * T::S;
        const bool in = gx >= 0 && gy >= 0 && gx < (int)fr.W && gy < (int)fr.H;
        const size_t j = in ? (size_t)gy * fr.W + (size_t)gx : 0;          // (outside the image: any valid address, the record is flagged unusable)
        float4 g0 = fr.guide[2 * j], g1 = fr.guide[2 * j + 1];
        g0w(g0, j);
        if (!in) g1.w = 0.0f;
        sG0[ry * T::STRIDE + rx] = g0; sG1[ry * T::STRIDE + rx] = g1; sC[ry * T::STRIDE + rx] = colIn[j];
    }
    __syncthreads();
}

// STEP 0: taps gathered from memory at the run-time step it.step; STEP > 0: tile + halo staged in LDS.
// The tiles start at band.rowBegin and the row phase counts from there (grid: dn_grid of the band's height), pixels below band.rowEnd
// leave.  A tap is valid wherever it lies inside the image and is filterable: rows beyond a context's band were copied from their
// owners into its guide and colour buffers.  A band lower than the tile's span (TY * S rows: 128 at step 32) has workgroups whose first
// row already lies below it.
template <int STEP>
__global__ void __launch_bounds__(256) k_dn_iterate(DnFrame fr, DnIter it, DnBand band, const float4* __restrict__ colIn, float4* __restrict__ colOut) {
    using T = DnTile<STEP>;
    __shared__ float4 sG0[T::RECORDS], sG1[T::RECORDS], sC[T::RECORDS];
    const DnTilePos tp = dn_tile_pos<STEP>(fr.W, (int)band.rowBegin);
    if (tp.yBase >= (int)band.rowEnd) return;                                    // (the whole workgroup: before anything is staged)
    const int lx = tp.lx, ly = tp.ly, x = tp.x, y = tp.y;
    if (STEP) dn_stage<STEP>(fr, colIn, tp.xBase, tp.yBase, sG0, sG1, sC, [](float4&, size_t) {});
    if (x >= (int)fr.W || y >= (int)band.rowEnd) return;
    const uint32_t i = (uint32_t)y * fr.W + (uint32_t)x;
    const int lc = (ly + 2) * T::STRIDE + lx + 2 * T::S;                        // this pixel inside the staged region
    const float4 c0 = STEP ? sG0[lc] : fr.guide[2 * (size_t)i];
    const float4 c1 = STEP ? sG1[lc] : fr.guide[2 * (size_t)i + 1];
    const float4 cp = STEP ? sC[lc] : colIn[i];
    const bool filterable = c1.w != 0.0f;
    f3 e = mk3(cp.x, cp.y, cp.z);
    if (filterable) {
        const float sigmaPlaneT = it.sigmaPlane * c0.w;
        DnSums s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float hh = dn_h(dy) * dn_h(dx);
                if (dx == 0 && dy == 0) { s.r = s.r + cp.x * hh; s.g = s.g + cp.y * hh; s.b = s.b + cp.z * hh; s.w = s.w + hh; continue; }
                if (STEP) {
                    const int k = lc + dy * T::STRIDE + dx * T::S;
                    const float4 g1 = sG1[k];
                    dn_tap(it, c0, c1, sigmaPlaneT, cp.w, sG0[k], g1, sC[k], g1.w != 0.0f, hh, s);
                } else {
                    const int qx = x + dx * it.step, qy = y + dy * it.step;
                    const bool in = qx >= 0 && qy >= 0 && qx < (int)fr.W && qy < (int)fr.H;
                    const size_t j = in ? (size_t)qy * fr.W + (size_t)qx : (size_t)i;   // (outside: the centre's own address, selected away)
                    const float4 g1 = fr.guide[2 * j + 1];
                    dn_tap(it, c0, c1, sigmaPlaneT, cp.w, fr.guide[2 * j], g1, colIn[j], in && g1.w != 0.0f, hh, s);
                }
            }
        }
        e = mk3(s.r / s.w, s.g / s.w, s.b / s.w);
    }
    if (it.last) dn_output(fr, i, e, filterable);
    else colOut[i] = make_float4(e.x, e.y, e.z, dn_luminance(e.x, e.y, e.z));
}
template <int STEP> inline uint32_t dn_grid(uint32_t W, uint32_t rows) {
    using T = DnTile<STEP>;
    return ((W + (T::TX - 1)) / T::TX) * ((rows + (T::TY * T::S - 1)) / (T::TY * T::S)) * (uint32_t)T::S;
}

__global__ void __launch_bounds__(256) k_dn_finish(DnFrame fr, DnBand band, const float4* __restrict__ colIn) {
    const uint32_t i = band.rowBegin * fr.W + blockIdx.x * 256u + threadIdx.x;
    if (i >= band.rowEnd * fr.W) return;
    const float4 c = colIn[i];
    dn_output(fr, i, mk3(c.x, c.y, c.z), fr.albedo[i].w != 0.0f);
}

}  // namespace rt
