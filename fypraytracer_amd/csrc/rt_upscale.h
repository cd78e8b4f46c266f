// Guided upscaler (fyprt_denoise_upscale*, include/fyprt.h; DESIGN.md §4 "Upscaler") — gfx950.
// The frame is shaded and denoised at W x H; only primary rays are traced at sW x sH (s = 2, 3, 4).  The demodulated colour of the low-res
// stage is interpolated under the hi-res guide records with the denoiser's normal and plane stopping functions and multiplied by the
// hi-res albedo: geometric edges and texture detail at the presented size, lighting at the rendered one.  No reference counterpart; the
// contract is the header's, binary32 + - * / and selections in the order written there (-ffp-contract=off, IEEE division, fp32
// denormals), restated in numpy by tests/upscale_ref.py.
//
//   the low-res stage : the existing kernels (rt_denoise.h / rt_temporal.h), the last iteration with DnIter::last = 0 so that the
//                       colour e stays in a colour buffer, no k_dn_finish.
//   k_up_primary      : one thread per hi-res pixel, a wave per 8 x 8 tile as k_primary maps them.  The frame's camera with the viewport
//                       replaced (pixel (s x, s y) has bit for bit the ray of low-res (x, y)), trace_ray with the stack in LDS, then what
//                       dn_prepare_pixel gathers (material, emission test, sample_albedo).  Two 16-byte guide stores and one albedo store;
//                       the 40-byte payload is never written.
//   k_up_resolve<S>   : one thread per hi-res pixel, 16 x 16 tiles as dn_tile_pos lays them out.  The tile's low-res footprint (at most
//                       9 x 9 pixels: 16 / S columns and their right neighbour) is staged in LDS as 48-byte records (guide | e) in the
//                       way dn_stage does it; the four taps are ds_read_b128.  Own guide and albedo: 16-byte global loads.
// Both hi-res kernels work on a band of hi-res rows, as k_dn_iterate does on low-res ones: the full frame is the band [0, sH), and a group
// member (fyprt_group_denoise_upscale*, fyprt_multi.h) that owns the low-res rows [b, e) runs them on [s b, s e).  The records and the
// outputs keep their place in the full-size hi-res buffers; the band bounds are kernel arguments, so they stay in scalar registers.
#pragma once
#include "rt_denoise.h"
#include "rt_kernels.h"

namespace rt {

struct UpFrame {                     // what the resolve kernel reads about the frame and the call
    uint32_t W, H;                   // the rendered (low-res) size; the outputs are S W x S H
    float frameIndex;                // n, as DnFrame
    uint32_t demodulate;
    float sigmaPlane; uint32_t normalPow;
    const float4* accum;             // low-res: the frame's running sum,
    const float4* guide;             //   the denoiser's guide records (2 quads per pixel),
    const float4* albedo;            //   its albedo buffer,
    const float4* e;                 //   the colour after the last iteration (c_p where not filterable)
    const float4* upGuide;           // hi-res: guide records (FYPRT_BUF_UPSCALE_GUIDE),
    const float4* upAlbedo;          //   albedo | 1 or pass-through colour | 0 (FYPRT_BUF_UPSCALE_ALBEDO)
    uint32_t* rgba8; float4* radiance4;   // the call's outputs, S W x S H (device memory; either may be null)
};

// cam: the frame's camera with W, H = the hi-res viewport.  sky: the sky colour the frame was rendered with.  band: the hi-res rows the
// tiles cover, counted from band.rowBegin (grid: up_primary_grid of the band's height).
__global__ __launch_bounds__(kBlock) void k_up_primary(DevScene sc, DevCamera cam, uint32_t tileOrder, f3 sky, DnBand band, float4* __restrict__ guide,
                                                        float4* __restrict__ albedo) {
    extern __shared__ int32_t s_stack[];                         // (stackBudget + 1) entries x kBlock threads, sized at launch
    DevFrame fr{}; fr.W = cam.W; fr.H = cam.H; fr.tileOrder = tileOrder;
    uint32_t x, y;
    if (!pixel_of_thread(fr, band.rowBegin, band.rowEnd, x, y)) return;
    const size_t i = (size_t)y * cam.W + x;
    const f3 pd = ray_direction(cam, x, y);
    const Payload pp = trace_ray<false>(sc, cam.position, pd, s_stack + threadIdx.x);
    f3 a = sky; float flag = 0.0f;
    if (!(pp.hitDistance < 0.0f)) {
        const Mat m = load_mat(sc, tri_material(sc, pp.objectIndex));
        if (length(emission(m)) > 0.0f) a = emission(m);
        else { a = sample_albedo(sc, m, pp.u, pp.v); flag = 1.0f; }
    }
    guide[2 * i] = make_float4(pp.px, pp.py, pp.pz, pp.hitDistance);
    guide[2 * i + 1] = make_float4(pp.nx, pp.ny, pp.nz, flag);
    albedo[i] = make_float4(a.x, a.y, a.z, flag);
}
// tile_grid for `rows` hi-res rows: padded so that every XCD owns the same number of workgroups
inline uint32_t up_primary_grid(uint32_t upW, uint32_t rows, uint32_t tileOrder) {
    const uint32_t tilesX = (upW + 15u) / 16u, tilesY = (rows + 15u) / 16u;
    return tileOrder == 2u ? tilesX * ((tilesY + 7u) / 8u) * 8u : ((tilesX * tilesY + 7u) / 8u) * 8u;
}

// Staged low-res region of a 16 x 16 hi-res tile: R x R records from (xBase / S, yBase / S).  16 consecutive hi-res columns from a
// multiple of 16 touch 8 / 6 / 4 low-res columns (S = 2 / 3 / 4), and the right tap one more.  Row stride 12 records (48 dwords): a wave
// (an 8 x 8 hi-res quad) reads at most 4 consecutive records of at most 4 staged rows per tap, and rows 48 dwords apart put those four
// 16-dword runs on disjoint banks whatever the ds_read_b128 lane groups are.
template <int S> struct UpTile {
    static constexpr int R = S == 3 ? 7 : 16 / S + 1;
    static constexpr int STRIDE = 12, RECORDS = R * STRIDE;
};

RT_DEV void up_output(const UpFrame& fr, size_t i, f3 out, float alpha) {
    if (fr.radiance4) fr.radiance4[i] = make_float4(out.x, out.y, out.z, alpha);
    if (fr.rgba8) {
        f4 a = mk4(out.x / (out.x + 1.0f), out.y / (out.y + 1.0f), out.z / (out.z + 1.0f), alpha / (alpha + 0.0f));
        a = mk4(gclamp(a.x, 0.0f, 1.0f), gclamp(a.y, 0.0f, 1.0f), gclamp(a.z, 0.0f, 1.0f), gclamp(a.w, 0.0f, 1.0f));
        fr.rgba8[i] = pack_abgr(a);
    }
}

// (A form that gathers the four taps from memory instead of staging them was timed beside this one and is gone: 0.149 against 0.126 ms
// at 1920 x 1080 -> 3840 x 2160, profiles/upscale/upscale_rate.jsonl.)
// band: the hi-res rows [S b, S e) of a band of low-res rows [b, e) — the tiles start at band.rowBegin (a multiple of S, so the low-res
// row of a hi-res row is the same division as in the full frame), pixels at or below band.rowEnd leave.  The last S - 1 rows of a band
// read the low-res row e: a group member finds it in its own guide and colour buffers, where the pull from the row's owner put it, and row
// H is outside the image as before.  Staged rows beyond e are read (any address inside the full-size buffers) and used by no pixel.
template <int S>
__global__ void __launch_bounds__(256) k_up_resolve(UpFrame fr, DnBand band) {
    using T = UpTile<S>;
    __shared__ float4 sG0[T::RECORDS], sG1[T::RECORDS], sC[T::RECORDS];
    const uint32_t upW = fr.W * (uint32_t)S;
    const DnTilePos tp = dn_tile_pos<0>(upW, (int)band.rowBegin);
    if (tp.yBase >= (int)band.rowEnd) return;                                          // (the whole workgroup: before anything is staged)
    const int bx = tp.xBase / S, by = tp.yBase / S;
    for (int k = (int)threadIdx.x; k < T::R * T::R; k += 256) {
        const int rx = k % T::R, ry = k / T::R, gx = bx + rx, gy = by + ry;
        const bool in = gx < (int)fr.W && gy < (int)fr.H;
        const size_t j = in ? (size_t)gy * fr.W + (size_t)gx : 0;                // (outside the image: any valid address, the record is flagged unusable)
        float4 g1 = fr.guide[2 * j + 1];
        if (!in) g1.w = 0.0f;
        sG0[ry * T::STRIDE + rx] = fr.guide[2 * j]; sG1[ry * T::STRIDE + rx] = g1; sC[ry * T::STRIDE + rx] = fr.e[j];
    }
    __syncthreads();
    const int X = tp.x, Y = tp.y;
    if (X >= (int)upW || Y >= (int)band.rowEnd) return;
    const size_t i = (size_t)Y * upW + (size_t)X;
    const int x0 = X / S, y0 = Y / S, fx = X - S * x0, fy = Y - S * y0;
    const size_t p = (size_t)y0 * fr.W + (size_t)x0;
    const int lc = (y0 - by) * T::STRIDE + (x0 - bx);                            // (x0, y0) inside the staged region
    const float alpha = fr.accum[p].w / fr.frameIndex;
    const float4 ep = sC[lc];
    f3 out = mk3(ep.x, ep.y, ep.z);                                              // out_(x0, y0) of a pixel that is not filterable: c_p
    if (fx == 0 && fy == 0) {                                                    // aligned: out_(x0, y0)
        const bool filterable = sG1[lc].w != 0.0f;
        if (filterable && fr.demodulate) {
            const float4 a = fr.albedo[p];
            out = mk3(ep.x * gmax(a.x, 1e-3f), ep.y * gmax(a.y, 1e-3f), ep.z * gmax(a.z, 1e-3f));
        }
    } else {
        const float4 aQ = fr.upAlbedo[i];
        if (aQ.w == 0.0f) out = mk3(aQ.x, aQ.y, aQ.z);                           // the pass-through colour
        else {
            const float4 c0 = fr.upGuide[2 * i], c1 = fr.upGuide[2 * i + 1];
            const float tx = (float)fx / (float)S, ty = (float)fy / (float)S;
            const float sigmaPlaneT = fr.sigmaPlane * c0.w;
            float sw = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f, sb = 0.0f, dr = 0.0f, dg = 0.0f, db = 0.0f;
            bool any = false;
#pragma unroll
            for (int dy = 0; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = 0; dx <= 1; ++dx) {
                    const float b = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
                    const int k = lc + dy * T::STRIDE + dx;
                    const float4 g0 = sG0[k], g1 = sG1[k], eq = sC[k];
                    const float d = (c1.x * g1.x + c1.y * g1.y) + c1.z * g1.z;
                    float wn = (0.0f < d) ? d : 0.0f;
                    for (uint32_t k = 0; k < fr.normalPow; ++k) wn = wn * wn;
                    const float ex = g0.x - c0.x, ey = g0.y - c0.y, ez = g0.z - c0.z;
                    const float xz = __builtin_fabsf((c1.x * ex + c1.y * ey) + c1.z * ez) / sigmaPlaneT;
                    const float wz = 1.0f / (1.0f + xz * xz);
                    const float w = (wn * wz) * b;
                    if (g1.w != 0.0f && b > 0.0f) {
                        sw = sw + w; cr = cr + eq.x * w; cg = cg + eq.y * w; cb = cb + eq.z * w;
                        sb = sb + b; dr = dr + eq.x * b; dg = dg + eq.y * b; db = db + eq.z * b;
                        any = true;
                    }
                }
            }
            if (any) {
                const f3 E = (sw > 0.0f) ? mk3(cr / sw, cg / sw, cb / sw) : mk3(dr / sb, dg / sb, db / sb);
                out = E;
                if (fr.demodulate) out = mk3(E.x * gmax(aQ.x, 1e-3f), E.y * gmax(aQ.y, 1e-3f), E.z * gmax(aQ.z, 1e-3f));
            }                                                                    // else: no usable tap — (x0, y0) itself is not filterable, out_(x0, y0) = c_p
        }
    }
    up_output(fr, i, out, alpha);
}
inline uint32_t up_resolve_grid(uint32_t upW, uint32_t rows) { return dn_grid<0>(upW, rows); }

}  // namespace rt
