// fyprt_selftest_functions: the shading functions of rt_math.h / rt_device.h / rt_kernels.h, one at a time, on caller-supplied arguments
// (DESIGN.md §4).  The kernel calls the very inline functions the frame kernels call — built in the same translation unit with the
// same flags — so that a test can compare each of them with the CPU oracle bit for bit at arguments no rendered picture reaches
// (tests/test_gpu_functions.py).  Records are arrays of 32-bit words; include/fyprt.h documents the layouts.
#pragma once
#include "rt_kernels.h"

namespace rt {

enum Probe {
    P_SINCOS = 0, P_ACOS = 1, P_POW5 = 2, P_RND = 3, P_OCT_ENCODE = 4, P_OCT_DECODE = 5, P_PACK_ABGR = 6, P_UNPACK_ABGR = 7,
    P_EVAL_BRDF = 8, P_PDF_BRDF = 9, P_PDF_GGX = 10, P_SAMPLE_UNIFORM = 11, P_SAMPLE_COSINE = 12, P_SAMPLE_GGX = 13, P_SAMPLE_BRDF = 14,
    P_DI_UPDATE = 15, P_SAMPLE_ALBEDO = 16, P_CLUSTER_IMPORTANCE = 17, P_CLUSTER_IMPORTANCE_GENERAL = 18, P_ASIN_KERNEL = 19, P_COUNT = 20
};
// 32-bit words per input / output record
constexpr uint32_t kProbeIn[P_COUNT] = {1, 1, 1, 1, 3, 2, 4, 1, 16, 16, 16, 16, 16, 16, 16, 4, 3, 23, 23, 2};
constexpr uint32_t kProbeOut[P_COUNT] = {2, 1, 1, 2, 2, 3, 1, 4, 3, 1, 1, 5, 5, 5, 5, 7, 3, 1, 1, 2};

RT_DEV float pw_f(const uint32_t* w, int k) { return __uint_as_float(w[k]); }
RT_DEV f3 pw_f3(const uint32_t* w, int k) { return mk3(__uint_as_float(w[k]), __uint_as_float(w[k + 1]), __uint_as_float(w[k + 2])); }
RT_DEV void pw_put(uint32_t* o, int k, float v) { o[k] = __float_as_uint(v); }
RT_DEV void pw_put3(uint32_t* o, int k, f3 v) { pw_put(o, k, v.x); pw_put(o, k + 1, v.y); pw_put(o, k + 2, v.z); }

// one record: `w` = its input words, `o` = its output words
RT_DEV void probe_record(int probe, const DevScene& sc, const uint32_t* w, uint32_t* o) {
    switch (probe) {
        case P_SINCOS: { float s, c; sincos_f(pw_f(w, 0), s, c); pw_put(o, 0, s); pw_put(o, 1, c); break; }
        case P_ACOS: pw_put(o, 0, acos_f(pw_f(w, 0))); break;
        case P_POW5: pw_put(o, 0, pow5_f(pw_f(w, 0))); break;
        case P_RND: { uint32_t seed = w[0]; pw_put(o, 0, rnd(seed)); o[1] = seed; break; }
        case P_OCT_ENCODE: { const f2 e = oct_encode(pw_f3(w, 0)); pw_put(o, 0, e.x); pw_put(o, 1, e.y); break; }
        case P_OCT_DECODE: { f2 e; e.x = pw_f(w, 0); e.y = pw_f(w, 1); pw_put3(o, 0, oct_decode(e)); break; }
        case P_PACK_ABGR: o[0] = pack_abgr(mk4(pw_f(w, 0), pw_f(w, 1), pw_f(w, 2), pw_f(w, 3))); break;
        case P_UNPACK_ABGR: { const f4 c = unpack_abgr(w[0]); pw_put(o, 0, c.x); pw_put(o, 1, c.y); pw_put(o, 2, c.z); pw_put(o, 3, c.w); break; }
        case P_EVAL_BRDF: pw_put3(o, 0, eval_brdf(pw_f3(w, 0), pw_f3(w, 3), pw_f3(w, 6), pw_f3(w, 9), pw_f(w, 12), pw_f(w, 13))); break;
        case P_PDF_BRDF: pw_put(o, 0, pdf_brdf(pw_f3(w, 0), pw_f3(w, 3), pw_f3(w, 6), pw_f3(w, 9), pw_f(w, 12), pw_f(w, 13))); break;
        case P_PDF_GGX: pw_put(o, 0, pdf_ggx(pw_f3(w, 0), pw_f3(w, 3), pw_f3(w, 6), pw_f(w, 13))); break;
        case P_SAMPLE_UNIFORM: case P_SAMPLE_COSINE: case P_SAMPLE_GGX: case P_SAMPLE_BRDF: {
            const f3 n = pw_f3(w, 0), V = pw_f3(w, 3); uint32_t seed = w[14]; float pdf; f3 L;
            if (probe == P_SAMPLE_UNIFORM) { L = sample_uniform(n, seed); pdf = pdf_uniform(); }
            else if (probe == P_SAMPLE_COSINE) { L = sample_cosine(n, seed); pdf = pdf_cosine(gmax(dot(n, L), 0.0f)); }
            else if (probe == P_SAMPLE_GGX) L = sample_ggx(n, V, pw_f(w, 13), seed, pdf);
            else L = sample_brdf(n, V, pw_f3(w, 9), pw_f(w, 12), pw_f(w, 13), seed, pdf);
            pw_put3(o, 0, L); pw_put(o, 3, pdf); o[4] = seed; break;
        }
        case P_DI_UPDATE: {
            DIRes r = di_empty(); uint32_t seed = w[3];
            const bool accepted = di_update(r, w[0], pw_f(w, 1), 1u, pw_f(w, 2), seed);
            o[0] = r.index; pw_put(o, 1, r.W); pw_put(o, 2, r.pdf); pw_put(o, 3, r.wSum); o[4] = r.M; o[5] = accepted ? 1u : 0u; o[6] = seed; break;
        }
        case P_SAMPLE_ALBEDO: {
            Mat m; m.albedo = splat3(-1.0f); m.useMap = 1u; m.mapIndex = w[2]; m.roughness = m.metallic = m.power = 0.0f; m.emColor = splat3(0.0f);
            pw_put3(o, 0, sample_albedo(sc, m, pw_f(w, 0), pw_f(w, 1))); break;
        }
        case P_ASIN_KERNEL: {  // the binary64 polynomial under acos_f, before the rounding to binary32 hides its last bits
            const double r = asin_kernel(__longlong_as_double((long long)(((unsigned long long)w[1] << 32) | w[0])));
            const unsigned long long b = (unsigned long long)__double_as_longlong(r); o[0] = (uint32_t)b; o[1] = (uint32_t)(b >> 32); break;
        }
        default: {     // P_CLUSTER_IMPORTANCE (the wave-uniform dispatch the light-tree walk uses), P_CLUSTER_IMPORTANCE_GENERAL (all eight corners)
            DevLTNode c; uint32_t* cw = reinterpret_cast<uint32_t*>(&c);
#pragma unroll
            for (int k = 0; k < 20; ++k) cw[k] = w[3 + k];
            pw_put(o, 0, probe == P_CLUSTER_IMPORTANCE ? cluster_importance(pw_f3(w, 0), c) : cluster_importance_t<-1>(pw_f3(w, 0), c)); break;
        }
    }
}
static_assert(sizeof(DevLTNode) == 80, "layout");

// Grid-stride over the records: a wave takes 64 consecutive records per step, so a test that wants one of cluster_importance's flat-box
// variants passes records that are flat along that axis in whole runs of 64.
__global__ void __launch_bounds__(kBlock) k_probe_functions(int probe, DevScene sc, const uint32_t* in, uint32_t inWords, uint32_t* out, uint32_t outWords, uint32_t count) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        uint32_t w[23], o[7];
#pragma unroll
        for (uint32_t k = 0; k < 23; ++k) w[k] = k < inWords ? in[i * inWords + k] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < 7; ++k) o[k] = 0u;
        probe_record(probe, sc, w, o);
#pragma unroll
        for (uint32_t k = 0; k < 7; ++k) if (k < outWords) out[i * outWords + k] = o[k];
    }
}

}  // namespace rt
