// Device side of a material edit (fyprt_update_materials; SceneManager::PerformAllSceneUpdates with materialsToUpdate /
// meshMatToBeUpdated, SceneManager.cpp:10-17, :69-85).  Nothing geometric changes, so the acceleration structure is not touched:
//   k_set_mesh_material    the material index of every triangle of the reassigned meshes, into the three per-triangle copies
//   k_emissive_count       } the emissive-triangle list (Scene::InitSceneEmissiveTriangles, Scene.cpp:209-221) as an ORDERED stream
//   k_emissive_scan        } compaction: ReSTIR DI draws a candidate as an index into the list, so the list must be the one an upload
//   k_emissive_scatter     } derives — ascending triangle order, the same on every run.  Positions come from a scan, never from atomics.
// The stream is the triangle range [first, nT) — the whole scene for a material edit, the appended triangles for fyprt_append_meshes, whose
// list is the old one followed by the range's emitters.
// Every workgroup owns one contiguous chunk of triangles (a multiple of the block size, the same in count and scatter):
//   count:   flags of the chunk -> one count per workgroup
//   scan:    exclusive prefix of the (at most kEmMaxGroups) counts in one workgroup; entry [groups] = the total, the host's 4-byte read
//   scatter: the chunk again, tile by tile in order: rank inside the wave from the ballot, a prefix over the waves in LDS, the tile's
//            total added to the running base
#pragma once
#include "rt_device.h"

namespace rt {

constexpr uint32_t kEmMaxGroups = 1024;        // workgroups of count / scatter: their counts are scanned by ONE workgroup, 4 per thread
constexpr uint32_t kEmMinChunk = 4 * kBlock;    // triangles a workgroup owns at least (whole tiles of kBlock)

// (first triangle, triangle count, material index, unused) per reassigned mesh; blockIdx.y = the mesh, x strides over its triangles
__global__ void k_set_mesh_material(const uint4* ranges, float4* triPos, float4* triShade, uint4* triIdx, uint32_t nT) {
    const uint4 r = ranges[blockIdx.y];
    const float bits = __int_as_float((int)r.z);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < r.y; i += gridDim.x * blockDim.x) {
        const uint32_t t = r.x + i;
        if (t >= nT) return;
        triPos[(size_t)t * 3].w = bits; triShade[(size_t)t * 4 + 3].w = bits; triIdx[t].w = r.z;
    }
}

// is triangle t an emitter: the host's per-material flag (is_emissive, the reference's operation order) through its material index
RT_DEV bool tri_emits(const uint4* triIdx, const uint32_t* matFlag, uint32_t matCount, uint32_t t, uint32_t nT) {
    if (t >= nT) return false;
    const uint32_t m = triIdx[t].w;
    return m < matCount && matFlag[m] != 0u;
}

__global__ void __launch_bounds__(kBlock) k_emissive_count(const uint4* triIdx, const uint32_t* matFlag, uint32_t matCount, uint32_t first, uint32_t nT, uint32_t perGroup, uint32_t* counts) {
    __shared__ uint32_t s_count[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t begin = first + blockIdx.x * perGroup;
    uint32_t n = 0;
    for (uint32_t tile = 0; tile < perGroup; tile += kBlock)
        n += (uint32_t)__popcll(__ballot(tri_emits(triIdx, matFlag, matCount, begin + tile + threadIdx.x, nT)));
    if (lane == 0u) s_count[wave] = n;            // every lane of a wave holds the wave's count
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);
}

// counts[0 .. groups) -> offsets[0 .. groups] (exclusive prefix, [groups] = total); one workgroup of kBlock threads, 4 entries per thread
__global__ void __launch_bounds__(kBlock) k_emissive_scan(const uint32_t* counts, uint32_t groups, uint32_t* offsets) {
    __shared__ uint32_t s_sum[kBlock];
    static_assert(kEmMaxGroups == 4 * kBlock, "four counts per thread");
    uint32_t v[4], own = 0;
    for (uint32_t k = 0; k < 4u; ++k) { const uint32_t g = threadIdx.x * 4u + k; v[k] = g < groups ? counts[g] : 0u; own += v[k]; }
    s_sum[threadIdx.x] = own;
    __syncthreads();
    for (uint32_t d = 1; d < (uint32_t)kBlock; d <<= 1) {             // inclusive Hillis-Steele over the threads' sums
        const uint32_t add = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t base = s_sum[threadIdx.x] - own;
    for (uint32_t k = 0; k < 4u; ++k) { const uint32_t g = threadIdx.x * 4u + k; if (g < groups) offsets[g] = base; base += v[k]; }
    if (threadIdx.x == (uint32_t)kBlock - 1u) offsets[groups] = s_sum[threadIdx.x];
}

__global__ void __launch_bounds__(kBlock) k_emissive_scatter(const uint4* triIdx, const uint32_t* matFlag, uint32_t matCount, uint32_t first, uint32_t nT, uint32_t perGroup,
                                                             const uint32_t* offsets, uint32_t* out, uint32_t outCount) {
    __shared__ uint32_t s_count[2][kBlock / 64];   // double-buffered: one barrier per tile
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t begin = first + blockIdx.x * perGroup;
    uint32_t base = offsets[blockIdx.x];
    for (uint32_t tile = 0, par = 0; tile < perGroup; tile += kBlock, par ^= 1u) {
        const uint32_t t = begin + tile + threadIdx.x;
        const bool em = tri_emits(triIdx, matFlag, matCount, t, nT);
        const unsigned long long mask = __ballot(em);
        if (lane == 0u) s_count[par][wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        for (uint32_t k = 0; k < wave; ++k) rank += s_count[par][k];
        if (em && base + rank < outCount) out[base + rank] = t;
        base += (s_count[par][0] + s_count[par][1]) + (s_count[par][2] + s_count[par][3]);
    }
}

}  // namespace rt
