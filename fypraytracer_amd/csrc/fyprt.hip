// libfyprt.so — C ABI (include/fyprt.h) over the gfx950 kernels of rt_kernels.h.
// Owns all device memory of one renderer context; everything stays resident in HBM between
// frames (the reference re-allocates and round-trips ~100 MB over PCIe per 1080p frame,
// Renderer.cu:37-53, :70, :244-283 — SURVEY.md §8 a14).
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "rt_host.h"
#include <hipcub/hipcub.hpp>
#include "rt_lbvh.h"
#include "rt_refit.h"
#include "rt_materials.h"
#include "rt_paths.h"
#include "rt_query.h"
#include "rt_points.h"
#include "rt_boxes.h"
#include "rt_triangles.h"
#include "rt_denoise.h"
#include "rt_temporal.h"
#include "rt_upscale.h"
#include "rt_probe.h"

using namespace rt;

// Largest step of the denoiser's iterations that runs the LDS-staged kernel (rt_denoise.h: k_dn_iterate<1> ... <32>); larger steps
// gather (iterations 7 and 8).  A build-time constant so that a variant library (tools/build_variant.sh) can time the other choice at
// every step; there is no tuning key.
#ifndef RT_DN_LDS_MAX_STEP
#define RT_DN_LDS_MAX_STEP 32
#endif
// Priority levels of the context's three streams (fyprt_create), likewise a build-time constant for a variant library: 0 = primary-ray stream
// lowest, context stream default, front stream highest; 1 = lowest / front default / context highest; 2 = front lowest, context default, primary highest.
#ifndef FYPRT_PRIORITY_ORDER
#define FYPRT_PRIORITY_ORDER 0
#endif

namespace {

thread_local std::string g_createError;

std::atomic<uint64_t> g_liveDeviceBytes{0};     // device bytes held by every DevBuf of the process (fyprt_live_device_bytes)

// Move-only owner of a device allocation.  A host-only context (device -1) records the size and allocates nothing.  `n` elements are in
// use out of `cap` allocated ones: the two differ only for a scene array that an append grew (grow_buffer).
template <class T> struct DevBuf {
    T* p = nullptr; size_t n = 0, cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; cap = o.cap; o.p = nullptr; o.n = o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count, bool hostOnly = false) {
        release(); n = cap = count;
        if (count == 0 || hostOnly) return hipSuccess;
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) g_liveDeviceBytes += cap * sizeof(T); else { p = nullptr; n = cap = 0; }
        return e;
    }
    void release() { if (p) { (void)hipFree(p); g_liveDeviceBytes -= cap * sizeof(T); } p = nullptr; n = cap = 0; }
    size_t bytes() const { return n * sizeof(T); }
};

// Move-only owner of an event / a stream (created by the caller into `h`); an empty one makes no HIP call.
template <class H, hipError_t (*Destroy)(H)> struct DevHandle {
    H h = nullptr;
    DevHandle() = default;
    DevHandle(DevHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    DevHandle& operator=(DevHandle&& o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
    ~DevHandle() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    operator H() const { return h; }
};
// Move-only owner of a few words of page-locked host memory, the target of a small read-back that must not stall the stream
struct PinnedWords {
    uint32_t* p = nullptr;
    PinnedWords() = default;
    PinnedWords(const PinnedWords&) = delete;
    PinnedWords& operator=(const PinnedWords&) = delete;
    ~PinnedWords() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t words) { return p ? hipSuccess : hipHostMalloc((void**)&p, words * sizeof(uint32_t), hipHostMallocDefault); }
};
using Event = DevHandle<hipEvent_t, hipEventDestroy>;
using Stream = DevHandle<hipStream_t, hipStreamDestroy>;
hipError_t create(Event& e, unsigned flags = hipEventDefault) { return e.h ? hipSuccess : hipEventCreateWithFlags(&e.h, flags); }

// Cached residency (workgroups per CU) of one persistent kernel, asked from the runtime once per LDS size.
struct OccCache {
    int blocks = 0; size_t lds = 0;
    template <class K> int get(K kernel, size_t ldsBytes, int fallback) {
        if (lds != ldsBytes) {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kBlock, ldsBytes) != hipSuccess || n <= 0) n = fallback;
            blocks = n; lds = ldsBytes;
        }
        return blocks;
    }
};

// Tuning keys (include/fyprt.h documents them by number): names, and {default, largest accepted value} per key; the smallest is 0.
enum TuningKey {
    K_TILE_ORDER = 0, K_DI_WAVEFRONT = 1, K_WG_PER_CU = 2, K_SORT_TASKS = 3, K_CHUNK = 4, K_REFILL_LANES = 5, K_QUORUM_SECONDARY = 6, K_QUORUM_PRIMARY = 7,
    K_STACK_BUDGET = 8, K_STATIC_CHUNKS = 9, K_MIN_CHUNK = 10, K_PIPELINE = 11, K_BUILDER = 12, K_SKIP_HALO_PART1 = 13, K_SETUP_FETCH = 14, K_RAY_KERNEL = 15,
    K_TOP_NODES = 16, K_FUSED_FRAME = 17, K_SKIP_DEAD_RAYS = 18, K_GI2_MODE = 19, K_GI2_REFILL_LANES = 20, K_DI_SPLIT = 21, K_PARTIAL_REFIT = 22, /* 23 reserved, 24 not assigned */ K_KEEP_PRIMARY = 25, K_COUNT = 26
};
constexpr struct { int def, max; } kTuning[K_COUNT] = {
    {2, 2}, {1, 1}, {0, 16}, {0, 1}, {128, 65536}, {24, 64}, {24, 64}, {32, 64}, {0, 31}, {0, 4096}, {32, 65536}, {1, 1},
    {0, 2}, {0, 1}, {0, 2}, {0, 2}, {0, 1024}, {0, 2}, {1, 1}, {2, 2}, {48, 64}, {1, 1}, {0, 1}, {0, 0}, {0, -1}, {1, 1}};

// host mat4 product, same operation order as the device / glm (column j = ((a0*bj.x + a1*bj.y) + a2*bj.z) + a3*bj.w)
void matmul_cm(const float* a, const float* b, float* out) {
    for (int j = 0; j < 4; ++j)
        for (int r = 0; r < 4; ++r) {
            float t = a[0 * 4 + r] * b[j * 4 + 0] + a[1 * 4 + r] * b[j * 4 + 1];
            t = t + a[2 * 4 + r] * b[j * 4 + 2];
            t = t + a[3 * 4 + r] * b[j * 4 + 3];
            out[j * 4 + r] = t;
        }
}

}  // namespace

struct ncclUniqueIdBytes { char b[128]; };        // == ncclUniqueId (rccl.h: 128 opaque bytes, passed by value)

struct fyprt_context {
    // multi-process multi-GPU (fyprt_comm_*, fyprt_multi.h): RCCL communicator of the ranks that share the frame, every rank's band
    void* comm = nullptr; int world = 1, rank = 0; std::vector<uint32_t> bounds; int commHaloMode = 0;
    int device = 0; std::string err; bool hostOnly = false;
    // Destruction order: members go in reverse order of declaration, so the three streams are declared before every buffer and event —
    // they are destroyed last, after what was used on them.  fyprt_destroy makes the device current first; a host-only context holds
    // only empty owners, so its destruction makes no HIP call.
    Stream stream;
    // ReSTIR DI frames are pipelined over two streams: Part 1 + Part-2 setup of frame N+1 (front stream) run beside the
    // persistent trace kernel of frame N (`stream`, on which every frame COMPLETES and which fyprt_stream() hands out)
    Stream front; Event evFront[2], evDone[2]; bool lastOverlapped = false;
    // ... and, with tuning key 21, over a third: the history-free half of Part 1 of frame N+1 (k_di_part1_primary, `prim`) runs beside the
    // setup kernel of frame N as well and hands its pixels to k_di_part1_temporal on the front stream through the staging set of the frame's
    // parity.  evPrim: the primary kernel is done; evTemp: the temporal kernel is done, the staging set free for the frame after next
    Stream prim; Event evPrim[2], evTemp[2];
    // Kept primary hits (tuning key 25).  A pixel's payload is a function of five camera fields and the geometry: ray_direction has no
    // jitter, no seed, and materials, textures, frameIndex and history do not enter trace_ray.  While both stand still — the converging
    // still frame frameIndex counts — a ReSTIR DI frame reads the payload an earlier DI frame traced instead of tracing it again.
    //   established by every ReSTIR DI frame that traced (split, unsplit, blocking, instrumented: the same trace_ray bits), at enqueue time,
    //               with its Part-1 rows and camera; evPayload is recorded behind the kernel that wrote c->payload, on `writer`
    //   used        by a DI frame that counts no rays, on exactly these rows with byte-equal camera fields (kept_primary_usable).  The band
    //               is compared as well: a moved band traces once even where band + halo, cut at the frame's edges, come out as the same
    //               Part-1 rows — one rule for every row change, at the price of one traced frame per change
    //   dropped     by whatever moves or renumbers geometry or the tree (edit_begin, set_scene_tree, fyprt_upload_scene, fyprt_resize,
    //               fyprt_set_object_vertices), by a changed tuning value (keys 7, 8 and 16 shape the traversal), and by every frame
    //               of another technique (k_primary, k_gi_primary and k_path_fused write the same buffer).  fyprt_update_materials and
    //               fyprt_append_textures keep it: a Payload holds distance, position, normal, uv and triangle index, the material is
    //               looked up from the triangle by every kernel that wants it (di_finished, k_di_part2_setup).
    struct KeptPrimary {
        bool valid = false; uint32_t begin = 0, end = 0, extraRow = 0, rowBegin = 0, rowEnd = 0;   // Part1Rows, and the band they were formed for
        m4 invProj{}, invView{}; f3 position{}; uint32_t W = 0, H = 0;
        hipStream_t writer = nullptr;
    } kept; Event evPayload; uint64_t keptFrames = 0;       // keptFrames: frames that reused the payload (fyprt_kept_primary_frames)
    void drop_kept_primary() { kept.valid = false; }
    static constexpr int kRing = 128;          // frames whose per-launch hipEvents are kept (fyprt_frame_timings)
    uint8_t ringSplit[kRing] = {};             // 0: the parts ran one after the other; 1: pipelined (the trace kernel starts at event 4); 2: Part 1 split as well (the front part starts at event 5)
    Event ring[kRing][6]; int ringLaunches[kRing] = {}; unsigned long long frameSerial = 0;
    uint32_t W = 0, H = 0, frameIndex = 1, rowBegin = 0, rowEnd = 0, halo = 0; bool rowsSet = false;
    uint32_t stripeRows = 0, stripeParts = 1, stripePart = 0;       // fyprt_set_row_stripes (per-pixel techniques only)
    uint32_t commStripeRows = 0, commLastStripeRows = 0; bool commLastStriped = false;
    int lastBuildRounds = 0;                                          // PLOC rounds of the last device build (diagnostic)
    bool haloExchange = false;   // halo rows of ReSTIR Part 1 come from the bands that own them (fyprt_multi.h) instead of being recomputed here
    bool part1Pending = false;   // fyprt_render_part(1) was called, part 2 must follow
    bool blockingCall = false;   // inside fyprt_render (which synchronises anyway): long path stages may poll the live-path count from the host
    uint32_t histDI[2] = {0, 0}, histGI[2] = {0, 0};   // rows [begin, end) whose ReSTIR DI / GI history this context holds (the band of the last such frame)
    bool haveScene = false, haveCamera = false, countRays = false;
    // per-pixel buffers
    DevBuf<float4> accum; DevBuf<uint32_t> image; DevBuf<Payload> payload; DevBuf<float> depth; DevBuf<f2> normalA, normalB;
    DevBuf<DIRes> di, diPrev; DevBuf<GIRes> gi, giPrev; DevBuf<float4> giHot; bool normalFlip = false;
    DevBuf<DIRec> drec, dprevA, dprevB; bool dprevFlip = false; int lastTech = -1;
    DevBuf<Payload> stagePayload; DevBuf<DIRec> stageRec;             // the split Part 1's staging sets, one per frame parity (written before they are read: not zeroed)
    int lastRestir = -1;                                              // technique of the last ReSTIR frame (-1: none since the buffers were zeroed): k_sync_history_normals
    uint32_t* externalImage = nullptr;
    // scene
    // what a device refit needs beyond the tree itself (fyprt_update_vertices): vertices, per-triangle vertex indices, the nodes of
    // every level (bottom level first), a box per node; and the topology the host light-tree builder is fed again
    DevBuf<DevVertex> dverts; DevBuf<uint4> triIdx; DevBuf<uint32_t> levelNodes; DevBuf<float4> nodeBox; std::vector<uint32_t> levelOffset;
    // fyprt_update_transforms: object-space vertices on the device, the meshes' vertex ranges, a host copy of the world vertices (the host
    // light-tree builder reads the emissive meshes' vertices from it)
    DevBuf<DevVertex> objVerts; std::vector<uint32_t> meshFirstVertex; std::vector<fyprt_vertex> hostVerts;
    std::vector<uint32_t> topoTris; std::vector<fyprt_mesh> topoMeshes; std::vector<fyprt_material> topoMats; uint32_t vertexCount = 0; bool prebuiltLightTrees = false;
    bool hostBvhStale = false;                      // the device tree was refitted: fyprt_export_bvh reads it back first
    bool nodeBoxValid = false;                      // nodeBox holds every node's exact box (a refit pass wrote it; a host-built tree has none yet)
    bool hostVertsStale = false;                    // world vertices were recomputed on the device: the host copy only follows for emissive meshes
    DevBuf<float4> nodes, leafTris, triPos, triShade, mats; DevBuf<DevTexture> texTable; std::vector<DevBuf<uint32_t>> texPixels;
    DevBuf<uint32_t> emissive; DevBuf<float4> lightRecs; DevBuf<DevLTNode> ltTlas, ltBlas; DevBuf<uint32_t> ltFirst, ltCount, ltRoot, ltLeafOfTri;
    // fyprt_update_materials: the emissive list as the host handed it over or derived it (host-only contexts answer fyprt_export_emissive
    // from it; on a device the list a compaction wrote lives in `emissive` alone and the copy is empty), whether it was handed over, and
    // the call's device scratch, grown on demand and kept (per-material flags, workgroup counts + offsets, reassigned triangle ranges)
    std::vector<uint32_t> hostEmissive; bool emissiveExplicit = false;
    DevBuf<uint32_t> matFlags, emCounts; DevBuf<uint4> matRanges;
    // fyprt_append_meshes / fyprt_append_textures: the scene arrays grow in place (DevBuf::cap, grow_buffer); the nodes a graft refits
    // (rt_graft.h), grown on demand and kept; the texture table as uploaded, which a longer one starts from
    DevBuf<uint32_t> graftList; std::vector<DevTexture> texHost;
    // fyprt_set_append_placement: the mode, the report of the last append with triangles (fyprt_last_append_placement), and the search's
    // two result words (best key, candidate count), allocated by the first search and kept
    int appendPlacement = 0; fyprt_append_placement placement{}; bool havePlacement = false; DevBuf<unsigned long long> placeOut;
    // fyprt_tree_cost (rt_treecost.h): the root's area and one (inner, leaf) pair of sums per workgroup, grown on demand and kept
    DevBuf<double> costPartials;
    // partial refit (rt_partial.h), all allocated on the first partial edit: the way up from a triangle (its leaf record, the record's
    // node, a node's parent) and the walk's scratch (per-level lists of dirty nodes, a flag per node, the list counts).  linksValid: the
    // maps describe the tree as it is — whatever changes the topology (upload, append, removal) clears it, the next partial edit rebuilds
    // them.  editStats: what the last geometry edit covered (fyprt_last_edit_stats)
    DevBuf<uint32_t> nodeParent, leafParent, leafOfTri, partialLists, partialDirty, partialCounters; bool linksValid = false;
    fyprt_edit_stats editStats{}; bool haveEditStats = false; PinnedWords partialCountsHost; bool partialCountsPending = false;
    DevBuf<unsigned long long> rayCounter;
    DevScene dsc{}; DevCamera dcam{};
    rth::SceneBVH hostBvh; rth::LightTrees hostLt; uint32_t meshCount = 0;
    int lastLaunches = 0;
    size_t queueStride = 0;                     // float4s per task queue
    size_t sortGroups = 0;                      // setup workgroups the sort scratch is sized for (per parity)
    OccCache traceOcc, pathOcc, gi2Occ;        // k_di_part2_trace, k_trace_rays, k_gi2_persistent
    int tuning[K_COUNT];                        // by TuningKey, defaults from kTuning
    int numCUs = 256;
    // wavefront path engine (rt_paths.h): two ray lists + results (ping-pong), per-pixel path state, pixel lists, list counters
    DevBuf<float4> wfRays[2], wfHits[2], wfState; DevBuf<uint32_t> wfPixels, wfPixels2, wfCounters;
    DevBuf<uint32_t> refImage;                 // fyprt_compare_image's reference
    DevBuf<float4> shadowTasks; DevBuf<uint32_t> queueCounters, sortCounts, sortOffset, sortTotal, sortIndex; DevBuf<uint8_t> sortKeys; DevBuf<uint16_t> sortHist;
    // One query family's state, allocated by its first query and kept: its own counters ([0..4] as a frame's launch, [5] low word = queue
    // head of the persistent kernel), the host entry's staging (records in, `after` records, results in 4-byte words, counts), grown on
    // demand, its two timing events, the occupancy of its persistent kernel (per kind for the ray query, [0] for the list queries).  The
    // box query's `after` words share `after` (a quad holds four), its totals lie in `out` behind the triangle indices
    struct QueryFamily {
        DevBuf<unsigned long long> counters; DevBuf<float4> in, after; DevBuf<uint32_t> out, counts; Event ev[2]; OccCache occ[2];
        OccCache occFiltered[2];               // ... and of its filtered form, indexed as `occ`
    };
    QueryFamily rayQuery, hitsQuery, pointsQuery;      // fyprt_trace_rays* (and the primary segments of fyprt_render_rays*), fyprt_trace_ray_hits*, fyprt_nearest_points*
    QueryFamily boxesQuery;                            // fyprt_overlap_boxes*
    QueryFamily trianglesQuery;                        // fyprt_overlap_triangles*
    // Query filter (fyprt_set_mesh_query_masks / fyprt_set_query_mask, rt_filter.h).  meshMasks: one word per mesh of the scene, empty =
    // filter off.  The derived device data — the non-empty meshes' first triangles ascending and their masks (what the leaf pass searches),
    // a word per leaf record, a word per node — is built on the context stream by the first filtered query after the table was set or
    // the tree changed (ensure_query_filter; filterValid says it describes table and tree as they are) and released when the filter
    // is switched off.  filterFirstHost / filterMaskHost: what the build uploads, kept while a copy may be in flight.
    std::vector<uint32_t> meshMasks, filterFirstHost, filterMaskHost; uint32_t queryMask = 0xFFFFFFFFu; uint64_t filterBuilds = 0; bool filterValid = false;
    DevBuf<uint32_t> filterFirst, filterMeshMask, leafMask, nodeMask;
    void release_query_filter() { filterFirst.release(); filterMeshMask.release(); leafMask.release(); nodeMask.release(); filterValid = false; }
    // radiance queries (fyprt_render_rays*, rt_query.h: k_render_rays_primary + the path stages), allocated on first use for
    // min(count, FYPRT_RENDER_RAYS_CHUNK) rays and kept: primary records, path state, ray / result lists, live lists, list counters + queue
    // heads; the host entry's staging (rays, pixel indices, radiance) and its two timing events
    DevBuf<Payload> rrPayload; DevBuf<float4> rrRays[2], rrHits[2], rrState; DevBuf<uint32_t> rrPixels, rrPixels2, rrCounters;
    DevBuf<float4> rrIn, rrOut; DevBuf<uint32_t> rrIndices; Event rrEv[2];
    // denoiser (fyprt_denoise*, rt_denoise.h), all allocated on the first call and dropped by fyprt_resize: guide records (2 quads per pixel),
    // albedo (FYPRT_BUF_ALBEDO), two ping-pong colour buffers, the host entry's output staging (for a group member, fyprt_group_denoise*: the
    // staging of its band's output rows, which the root collects); its timing events and the event the front stream waits for before the
    // next pipelined frame's Part 1 overwrites the payload the denoiser reads
    struct Denoise { DevBuf<float4> guide, albedo, col[2], outRad; DevBuf<uint32_t> outImg; } dn; Event dnEv[3], dnDone;
    bool frameComplete = false;                // a whole frame was rendered since the last resize / scene upload / geometry update
    uint32_t lastFrameIndex = 0;               // the frame index that frame was rendered with (the divisor of its epilogue)
    bool albedoValid = false;                  // FYPRT_BUF_ALBEDO holds the albedo of a denoised frame
    // temporal denoiser (fyprt_denoise_temporal*, rt_temporal.h), allocated on the first temporal call and dropped by fyprt_resize: two
    // history buffers (4 quads per pixel; a call reads any pixel of the old one while it writes the new one) and two variance buffers.
    // camPV = projection x view of the camera set last, framePV = that of the camera the last frame was enqueued with, dtPV = that of the
    // frame the last temporal call denoised (what the next one reprojects with); dtValid: dt.hist[dtCur] holds a history
    struct Temporal { DevBuf<float4> hist[2]; DevBuf<float> var[2]; } dt; Event dtEv[4]; int dtCur = 0; bool dtValid = false;
    uint64_t dtGroup = 0;                      // who wrote that history: 0 = a single-context call, else the group's serial (fyprt_group_denoise_temporal*)
    float camPV[16] = {}, framePV[16] = {}, dtPV[16] = {};
    // object motion (fyprt_denoise_temporal_set_motion): with the mode on a geometry edit keeps the history and copies the world vertices
    // as the frame denoised last saw them into dtSnap (allocated at the first snapshot, with a moved flag per triangle).  dtSnapPending:
    // from that copy until the next temporal call, which reprojects through it; [dtEditLo, dtEditHi): the triangles of the meshes edited
    // since the copy — all others are bit-identical in both vertex sets, their flags stay at the zeros the snapshot left
    bool dtMotion = false, dtSnapPending = false; uint32_t dtEditLo = 0, dtEditHi = 0;
    DevBuf<DevVertex> dtSnap; DevBuf<uint8_t> dtMoved;
    void drop_history() { dtValid = false; dtSnapPending = false; }
    void release_temporal() { dt = Temporal(); drop_history(); }
    void release_snapshot() { dtSnap.release(); dtMoved.release(); dtSnapPending = false; }
    void release_denoise() { dn = Denoise(); albedoValid = false; }
    // upscaler (fyprt_denoise_upscale*, rt_upscale.h): the hi-res guide records (2 quads per hi-res pixel) and albedo | pass-through colour
    // (FYPRT_BUF_UPSCALE_GUIDE / _ALBEDO) and the host entry's hi-res output staging (for a group member, fyprt_group_denoise_upscale*: full-size
    // records of which its band's hi-res rows are valid, and the staging of those rows), allocated on the first call for its scale, reallocated
    // when the scale changes, dropped by fyprt_resize; its timing events.  frameCam / frameSky: the camera and the sky colour the last
    // frame was enqueued with (taken where framePV is) — what the hi-res primary rays are formed and the misses coloured with
    struct Upscale { DevBuf<float4> guide, albedo, outRad; DevBuf<uint32_t> outImg; } up; Event upEv[4];
    uint32_t upScale = 0; bool upValid = false;      // the scale the hi-res buffers are sized for (0: none); they hold a call's records
    DevCamera frameCam{}; f3 frameSky{};
    void release_upscale() { up = Upscale(); upScale = 0; upValid = false; }

    fyprt_context() { for (int k = 0; k < K_COUNT; ++k) tuning[k] = kTuning[k].def; }

    int fail(int code, const std::string& m) { err = m; return code; }
    int hip(hipError_t e, const char* what) {
        if (e == hipSuccess) return FYPRT_OK;
        err = std::string(what) + ": " + hipGetErrorString(e);
        std::fprintf(stderr, "fyprt: %s\n", err.c_str());     // the reference prints and continues (Renderer.cu:29-47)
        return FYPRT_EHIP;
    }
};

#define HIPCHK(ctx, call) do { int _rc = (ctx)->hip((call), #call); if (_rc != FYPRT_OK) return _rc; } while (0)
#define TRY(call) do { const int _rc = (call); if (_rc != FYPRT_OK) return _rc; } while (0)      // a call that has reported its own error

static hipError_t sync_all(fyprt_context* c) {      // all three streams: `prim` only ever runs ahead of the front one, and that one ahead of `stream`
    hipError_t e = c->prim ? hipStreamSynchronize(c->prim) : hipSuccess;
    const hipError_t e1 = c->front ? hipStreamSynchronize(c->front) : hipSuccess;
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    return e != hipSuccess ? e : e1 != hipSuccess ? e1 : e2;
}

// Effective pending-entry budget of node_step's stack rule for the uploaded tree: tuning key 8 if set; otherwise a few entries
// above the tree's level count, rounded DOWN to a stack size at which one more 256-thread workgroup fits the CU's 160 KB of
// LDS (entries x 1 KB per workgroup: 32 -> 5 workgroups, 26 -> 6, 22 -> 7, 20 -> 8, 17 -> 9, 16 -> 10) as long as at least 4
// entries of slack above the level count remain.  Never below the level count (the induction needs it), never above 31.
// (k_di_part2_trace<false> adds 256 B of static LDS, the pair bytes of its cooperative leaf phase: the sizes 26, 22 and 17 keep their
// residency, the exact fits 32, 20 and 16 hold one workgroup fewer for that kernel alone — which shows in unpipelined frames only,
// pipelined ones cap the persistent grid at 4 per CU.  The table is not re-tuned for it: not measured.)
static int effective_stack_budget(const fyprt_context* c) {
    const int levels = (int)c->hostBvh.levels;
    if (c->tuning[K_STACK_BUDGET] > 0) return std::min((int)rth::kStackBudget, std::max(levels, c->tuning[K_STACK_BUDGET]));
    static const int kSizes[6] = {16, 17, 20, 22, 26, 32};
    int entries = 32;
    for (int i = 5; i >= 0; --i) if (kSizes[i] <= std::max(levels + 9, 16) && kSizes[i] - 1 >= levels + 4) { entries = kSizes[i]; break; }
    return std::min((int)rth::kStackBudget, std::max(levels, entries - 1));
}
// ... and what a traversing launch takes from it: the budget for its scene descriptor and a workgroup's dynamic LDS, the stack
// ((budget + 1) entries per thread: LDS is what limits residency) + `topCount` staged top nodes (a -DRT_TOPCACHE build only)
struct StackLds { int budget; size_t bytes; };
static StackLds stack_lds(const fyprt_context* c, uint32_t topCount) { const int b = effective_stack_budget(c); return {b, (size_t)(b + 1) * kBlock * sizeof(int32_t) + (size_t)topCount * 64u}; }
// Ray kernels of the path engine and the batched queries (tuning key 15: 0 = by tree size): small trees (cheap rays) one thread per ray, big ones persistent waves with lane refill
static bool simple_ray_kernel(const fyprt_context* c) { return c->tuning[K_RAY_KERNEL] == 2 || (c->tuning[K_RAY_KERNEL] == 0 && c->hostBvh.tris.size() < 65536u); }
// fyprt_settings as the kernels read them, with the reference's uint8_t casts (Renderer.cu:2444, :2480-2481)
static DevSettings dev_settings(const fyprt_context* c, const fyprt_settings* s) {
    DevSettings st; st.sky = f3{s->sky_color[0], s->sky_color[1], s->sky_color[2]}; st.maxBounces = (uint8_t)s->light_bounces; st.sampleCount = (uint8_t)s->sample_count;
    st.candidateCount = (uint32_t)s->light_candidate_count; st.randSeed = s->rand_seed;
    st.useTemporal = s->use_temporal_reuse ? 1u : 0u; st.useSpatial = s->use_spatial_reuse ? 1u : 0u;
    st.historyLimit = (uint8_t)s->temporal_history_limit; st.numNeighbors = (uint8_t)s->spatial_neighbor_num; st.radius = (uint8_t)s->spatial_neighbor_radius;
    st.skipDeadRays = c->tuning[K_SKIP_DEAD_RAYS] ? 1u : 0u;
    return st;
}
// The descriptor of a launch that traces incoherent rays: the node-loop quorum of its kind, its own block of ray counters (or none)
static DevScene secondary_scene(DevScene sc, uint32_t quorum, unsigned long long* counters) { sc.nodeQuorum = quorum; sc.rayCounter = counters; return sc; }

static int upload(fyprt_context* c, void* dst, const void* src, size_t bytes) {
    if (bytes == 0 || c->hostOnly) return FYPRT_OK;
    return c->hip(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
}
// (re)allocates `b` for `count` elements and fills it from host memory / with zeros (on the context stream)
template <class T> static int alloc_upload(fyprt_context* c, DevBuf<T>& b, const void* src, size_t count) {
    HIPCHK(c, b.alloc(count, c->hostOnly));
    return upload(c, b.p, src, b.bytes());
}
template <class T> static int alloc_zeroed(fyprt_context* c, DevBuf<T>& b, size_t count) {
    HIPCHK(c, b.alloc(count));
    HIPCHK(c, hipMemsetAsync(b.p, 0, b.bytes(), c->stream));
    return FYPRT_OK;
}

// `b` grown to `count` elements for an append (fyprt_append_meshes): within the capacity nothing moves; beyond it the capacity at least
// doubles and (`move`) the old contents move device to device.  All streams are idle; complete on return.
template <class T> static int grow_buffer(fyprt_context* c, DevBuf<T>& b, size_t count, bool move = true) {
    if (c->hostOnly) { b.n = b.cap = count; return FYPRT_OK; }
    if (count <= b.cap) { b.n = count; return FYPRT_OK; }
    DevBuf<T> nb;
    HIPCHK(c, nb.alloc(std::max(count, 2 * b.cap)));
    if (move && b.n) { HIPCHK(c, hipMemcpyAsync(nb.p, b.p, b.bytes(), hipMemcpyDeviceToDevice, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    nb.n = count;
    b = std::move(nb);
    return FYPRT_OK;
}

// glm::length2(GetEmission()) > 0 (Scene.cpp:216), in that operation order
static bool is_emissive(const fyprt_material& m) {
    const float ex = m.emission_color[0] * m.emission_power, ey = m.emission_color[1] * m.emission_power, ez = m.emission_color[2] * m.emission_power;
    return ((ex * ex + ey * ey) + ez * ez) > 0.0f;
}

// Material.cuh:7-16 -> the device's 3 quads per material, and is_emissive per material
static void pack_materials(const fyprt_material* materials, uint32_t count, std::vector<float>& mats, std::vector<char>& emissiveMat) {
    mats.assign((size_t)count * 12, 0.0f); emissiveMat.assign(count, 0);
    for (uint32_t i = 0; i < count; ++i) {
        const fyprt_material& m = materials[i]; float* q = &mats[(size_t)i * 12];
        q[0] = m.albedo[0]; q[1] = m.albedo[1]; q[2] = m.albedo[2];
        uint32_t info = ((m.is_use_albedo_map & 0xFFu) ? 0x80000000u : 0u) | (m.albedo_map_index > 0x7FFFFFFFu ? 0x7FFFFFFFu : m.albedo_map_index);
        std::memcpy(&q[3], &info, 4);
        q[4] = m.roughness; q[5] = m.metallic; q[6] = m.emission_power;
        q[8] = m.emission_color[0]; q[9] = m.emission_color[1]; q[10] = m.emission_color[2];
        emissiveMat[i] = is_emissive(m);
    }
}

// The scheduling parameters every persistent queue shares (TraceQueue, GI2Queue, ShadowQueue, QueryRays); `refillKey`: K_REFILL_LANES
// or, for k_gi2_persistent, K_GI2_REFILL_LANES.  Static chunks, auto: two per wave — config 3 3.13 -> 3.08 ms, profiles/README.md r03.
template <class Q> static void set_queue_params(const fyprt_context* c, Q& q, int refillKey) {
    const int* t = c->tuning;
    q.chunk = (uint32_t)(t[K_CHUNK] > 0 ? t[K_CHUNK] : 128);
    q.refillLanes = (uint32_t)(t[refillKey] > 0 ? t[refillKey] : (refillKey == K_GI2_REFILL_LANES ? 48 : 24));
    q.staticChunks = (uint32_t)(t[K_STATIC_CHUNKS] > 0 ? t[K_STATIC_CHUNKS] : 2);
    q.minChunk = (uint32_t)(t[K_MIN_CHUNK] > 0 ? t[K_MIN_CHUNK] : q.chunk);
}

// one launch's ray counters (rays, box tests, triangle tests, hits, node visits) into part `k` of the stats and into their totals
static void add_ray_stats(fyprt_frame_stats* s, int k, const unsigned long long* r) {
    s->part_rays[k] = r[0]; s->part_box_tests[k] = r[1]; s->part_tri_tests[k] = r[2]; s->part_hits[k] = r[3]; s->part_node_visits[k] = r[4];
    s->rays += r[0]; s->box_tests += r[1]; s->tri_tests += r[2]; s->hits += r[3]; s->node_visits += r[4];
}

// ---- what the query families share (the entry points: "batched ray queries" below)
// Enqueues one query launch on the context stream (q: the record pointers in device memory and count > 0; kernels[simple][counted]);
// `timed` brackets it with the family's events.  A workgroup's LDS is the stack plus `listBytes` per thread (the list queries' 16 bytes,
// the box query's 4 bytes per entry of this call's max_hits).  The families have always differed in how tuning key 2 and a failed occupancy query are taken,
// and keep doing so: `clampWg` holds key 2 to the occupancy, `occFallback` stands in for an occupancy the runtime cannot give.
template <class Q>
static int launch_query_kernels(fyprt_context* c, fyprt_context::QueryFamily& f, OccCache& occ, Q q, void (*const kernels[2][2])(DevScene, Q), size_t listBytes,
                                bool clampWg, int occFallback, bool timed) {
    if (!f.counters.p) { HIPCHK(c, f.counters.alloc(8)); }
    HIPCHK(c, hipMemsetAsync(f.counters.p, 0, 64, c->stream));
    const StackLds stack = stack_lds(c, 0u);                      // the query kernels stage no top nodes (not even in a -DRT_TOPCACHE build)
    // the path engine's ray kernels' quorum (incoherent rays in general), the family's own counters
    DevScene qs = secondary_scene(c->dsc, (uint32_t)c->tuning[K_QUORUM_SECONDARY], c->countRays ? f.counters.p : nullptr);
    qs.stackBudget = stack.budget;
    const size_t ldsBytes = stack.bytes + listBytes * kBlock;     // <= 32 KB + 32 KB
    q.head = reinterpret_cast<uint32_t*>(f.counters.p + 5);
    set_queue_params(c, q, K_REFILL_LANES);
    const uint32_t blocksForRecords = (uint32_t)(((size_t)q.count + kBlock - 1) / kBlock);
    const bool simple = simple_ray_kernel(c);                     // tuning key 15 as in the path engine
    int perCU = 16;
    if (!simple) {
        const int o = occ.get(kernels[0][0], ldsBytes, occFallback), wg = c->tuning[K_WG_PER_CU];
        perCU = wg > 0 ? (clampWg ? std::min(wg, o) : wg) : o;
    }
    const dim3 grid(std::max(1u, std::min<uint32_t>((uint32_t)(c->numCUs * perCU), blocksForRecords)));   // no more workgroups than the records fill
    if (timed) HIPCHK(c, hipEventRecord(f.ev[0], c->stream));
    hipLaunchKernelGGL(kernels[simple ? 1 : 0][c->countRays ? 1 : 0], grid, dim3(kBlock), ldsBytes, c->stream, qs, q);
    HIPCHK(c, hipGetLastError());
    if (timed) HIPCHK(c, hipEventRecord(f.ev[1], c->stream));
    return FYPRT_OK;
}
// A family's kernels[simple][counted] in both forms, and the launch every query entry point ends in: the filtered form iff a mesh
// mask table is set (`filterable`: the entry point is one the filter applies to — the radiance queries' primary pass is not), behind
// the lazy build of the filter's device data; with the filter off the launch is the one it always was.  occIndex: which of the
// family's occupancy entries (the ray query's kind).
template <class Q> struct QueryKernels { void (*plain[2][2])(DevScene, Q); void (*filtered[2][2])(DevScene, Filtered<Q>); };
// ... derived from the family's lane state LaneT<FILTER> (rt_query.h's three kernel templates): no cell is typed by hand
template <template <bool> class LaneT> static constexpr QueryKernels<typename LaneT<false>::Query> query_kernels() {
    return {{{k_query<LaneT<false>>, k_query_counted<LaneT<false>>}, {k_query_simple<LaneT<false>, false>, k_query_simple<LaneT<false>, true>}},
            {{k_query<LaneT<true>>, k_query_counted<LaneT<true>>}, {k_query_simple<LaneT<true>, false>, k_query_simple<LaneT<true>, true>}}};
}
static int ensure_query_filter(fyprt_context* c);
template <class Q>
static int launch_query(fyprt_context* c, fyprt_context::QueryFamily& f, int occIndex, const Q& q, const QueryKernels<Q>& k, size_t listBytes,
                        bool clampWg, int occFallback, bool timed, bool filterable = true) {
    if (!filterable || c->meshMasks.empty()) return launch_query_kernels(c, f, f.occ[occIndex], q, k.plain, listBytes, clampWg, occFallback, timed);
    TRY(ensure_query_filter(c));
    Filtered<Q> fq{};
    static_cast<Q&>(fq) = q;
    fq.flt.nodeMask = c->nodeMask.p; fq.flt.leafMask = c->leafMask.p; fq.flt.queryMask = c->queryMask;
    return launch_query_kernels(c, f, f.occFiltered[occIndex], fq, k.filtered, listBytes, clampWg, occFallback, timed);
}

// A blocking entry point behind its checks: host records through the family's staging (which grows and is kept), one timed launch by
// `enqueue(in, after, out, counts)` on the staging pointers, results back, the launch's time and ray counters into `stats`.
// inQuads: float4s per input record; after / counts: the list queries' (counts is staged for them whether or not the caller wants it).
// afterBytes: one `after` record; tailBytes: a second result array staged in `out` behind the first (the box query's totals), copied
// back to `tail` if the caller wants it.
struct HostQuery {
    const void* in; size_t inQuads; const void* after; void* out; size_t outBytes; uint32_t* counts; bool list;
    size_t afterBytes = sizeof(float4); void* tail = nullptr; size_t tailBytes = 0;
};
template <class Enqueue>
static int run_host_query(fyprt_context* c, fyprt_context::QueryFamily& f, const HostQuery& h, uint32_t count, fyprt_frame_stats* stats, Enqueue enqueue) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (count == 0) return FYPRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (Event& e : f.ev) HIPCHK(c, create(e));
    if (f.in.n < (size_t)count * h.inQuads) { HIPCHK(c, f.in.alloc((size_t)count * h.inQuads)); }         // staging grows, is kept
    const size_t afterQuads = ((size_t)count * h.afterBytes + sizeof(float4) - 1) / sizeof(float4);
    if (h.after && f.after.n < afterQuads) { HIPCHK(c, f.after.alloc(afterQuads)); }
    if (f.out.bytes() < h.outBytes + h.tailBytes) { HIPCHK(c, f.out.alloc((h.outBytes + h.tailBytes) / 4)); }
    if (h.list && f.counts.n < (size_t)count) { HIPCHK(c, f.counts.alloc(count)); }
    HIPCHK(c, hipMemcpyAsync(f.in.p, h.in, (size_t)count * h.inQuads * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (h.after) HIPCHK(c, hipMemcpyAsync(f.after.p, h.after, (size_t)count * h.afterBytes, hipMemcpyHostToDevice, c->stream));
    TRY(enqueue(f.in.p, h.after ? f.after.p : nullptr, f.out.p, f.counts.p));
    HIPCHK(c, hipMemcpyAsync(h.out, f.out.p, h.outBytes, hipMemcpyDeviceToHost, c->stream));
    if (h.counts) HIPCHK(c, hipMemcpyAsync(h.counts, f.counts.p, (size_t)count * 4u, hipMemcpyDeviceToHost, c->stream));
    if (h.tail) HIPCHK(c, hipMemcpyAsync(h.tail, f.out.p + h.outBytes / 4, h.tailBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (stats) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, f.ev[0], f.ev[1]));
        stats->kernel_ms = ms; stats->kernel_ms_part[0] = ms; stats->launches = 1;
        if (c->countRays) {
            unsigned long long r[5] = {0, 0, 0, 0, 0};
            HIPCHK(c, hipMemcpy(r, f.counters.p, sizeof r, hipMemcpyDeviceToHost));
            add_ray_stats(stats, 0, r);
        }
    }
    return FYPRT_OK;
}

// ---- the list queries: multi-hit (rt_query.h), nearest points (rt_points.h), box overlap (rt_boxes.h) and triangle overlap
// (rt_triangles.h).  As the batched queries:
// the scene is read, the query's own results and counters are written, no frame state moves.
// A family: state, kernels[simple][counted] in both forms, and what differs between the families — float4s per input record, bytes per
// `after` record and per list entry (16: a hit record; 4: a bare triangle index), the cap on max_hits, whether a totals array follows
// the list; `noun` / `outNoun`: what its records and answers are called, `verb`: what a host-only context is told it cannot do.
template <class Q> struct ListQuery {
    fyprt_context::QueryFamily fyprt_context::* family; QueryKernels<Q> kernels;
    size_t inQuads, afterBytes, entryBytes; uint32_t maxHitsCap; bool totals;
    const char *noun, *outNoun, *verb;
};
static const ListQuery<QueryHits> kRayHits = {&fyprt_context::hitsQuery, query_kernels<HitsLaneT>(), 2, 16, 16, FYPRT_QUERY_MAX_HITS, false, "rays", "hits", "trace"};
static const ListQuery<QueryHits> kNearestPoints = {&fyprt_context::pointsQuery, query_kernels<PointsLaneT>(), 1, 16, 16, FYPRT_QUERY_MAX_HITS, false, "points", "hits", "query"};
static const ListQuery<QueryBoxes> kOverlapBoxes = {&fyprt_context::boxesQuery, query_kernels<BoxLaneT>(), 2, 4, 4, FYPRT_OVERLAP_MAX_HITS, true, "boxes", "triangles", "query"};
static const ListQuery<QueryTriangles> kOverlapTriangles = {&fyprt_context::trianglesQuery, query_kernels<TriLaneT>(), 3, 4, 4, FYPRT_OVERLAP_MAX_HITS, true, "triangles", "triangles", "query"};

// `who`: the entry point.  Input records are loaded as 16-byte quads; `after` and the list are loaded and stored in their own units.
template <class Q>
static int check_list_query(fyprt_context* c, const ListQuery<Q>& l, const char* who, const void* in, const void* after, uint32_t count, uint32_t maxHits, const void* out,
                            const void* hitCounts, const void* totals, bool device) {
    if (!c) return FYPRT_EINVAL;
    if (maxHits == 0 || maxHits > l.maxHitsCap) return c->fail(FYPRT_EINVAL, std::string(who) + ": max_hits must be 1.." + std::to_string(l.maxHitsCap));
    if (count && (!in || !out)) return c->fail(FYPRT_EINVAL, std::string(who) + ": NULL " + l.noun + " / " + l.outNoun + " with a non-zero count");
    if (device && (((uintptr_t)in & 15u) || ((uintptr_t)after & (l.afterBytes - 1)) || ((uintptr_t)out & (l.entryBytes - 1)) || ((uintptr_t)hitCounts & 3u) || ((uintptr_t)totals & 3u))) {
        std::vector<const char*> by[2] = {{l.noun}, {}};          // what must be 16-byte, what 4-byte aligned
        by[l.afterBytes == 16 ? 0 : 1].push_back("after"); by[l.entryBytes == 16 ? 0 : 1].push_back(l.outNoun);
        by[1].push_back("hit_counts"); if (l.totals) by[1].push_back("totals");
        const auto join = [](const std::vector<const char*>& v) {
            std::string s;
            for (size_t i = 0; i < v.size(); ++i) s += std::string(i == 0 ? "" : i + 1 == v.size() ? " and " : ", ") + v[i];
            return s;
        };
        return c->fail(FYPRT_EINVAL, std::string(who) + ": " + join(by[0]) + " must be 16-byte and " + join(by[1]) + " 4-byte aligned");
    }
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, std::string(who) + ": host-only context (device -1) cannot " + l.verb);
    if (!c->haveScene) return c->fail(FYPRT_ESTATE, std::string(who) + " before fyprt_upload_scene");
    return FYPRT_OK;
}
static void list_record(QueryHits& q, const float4* in, const void* after, void* out, uint32_t* counts, uint32_t*) {
    q.rays = in; q.after = static_cast<const float4*>(after); q.hits = static_cast<float4*>(out); q.counts = counts;
}
static void list_record(QueryBoxes& q, const float4* in, const void* after, void* out, uint32_t* counts, uint32_t* totals) {
    q.boxes = in; q.after = static_cast<const uint32_t*>(after); q.triangles = static_cast<uint32_t*>(out); q.counts = counts; q.totals = totals;
}
static void list_record(QueryTriangles& q, const float4* in, const void* after, void* out, uint32_t* counts, uint32_t* totals) {
    q.tris = in; q.after = static_cast<const uint32_t*>(after); q.triangles = static_cast<uint32_t*>(out); q.counts = counts; q.totals = totals;
}
// (device memory, count > 0, after / counts / totals may be NULL)
template <class Q>
static int enqueue_list_query(fyprt_context* c, const ListQuery<Q>& l, const float4* in, const void* after, uint32_t count, uint32_t maxHits, void* out, uint32_t* counts,
                              uint32_t* totals, bool timed) {
    Q q{};
    list_record(q, in, after, out, counts, totals); q.count = count; q.maxHits = maxHits;
    // key 2 no higher than the occupancy, 2 workgroups per CU without one
    return launch_query(c, c->*l.family, 0, q, l.kernels, (size_t)maxHits * l.entryBytes, true, 2, timed);
}
template <class Q>
static int host_list_query(fyprt_context* c, const ListQuery<Q>& l, const void* in, const void* after, uint32_t count, uint32_t maxHits, void* out, uint32_t* hitCounts,
                           uint32_t* totals, fyprt_frame_stats* stats) {
    HostQuery h{in, l.inQuads, after, out, (size_t)count * maxHits * l.entryBytes, hitCounts, true};
    h.afterBytes = l.afterBytes;
    if (l.totals) { h.tail = totals; h.tailBytes = (size_t)count * 4u; }       // staged behind the list whether or not the caller wants it
    return run_host_query(c, c->*l.family, h, count, stats, [&](const float4* dIn, const float4* dAfter, uint32_t* dOut, uint32_t* dCounts) {
        return enqueue_list_query(c, l, dIn, dAfter, count, maxHits, dOut, dCounts, l.totals ? dOut + h.outBytes / 4 : nullptr, true); });
}
template <class Q>
static int device_list_query(fyprt_context* c, const ListQuery<Q>& l, const void* in, const void* after, uint32_t count, uint32_t maxHits, void* out, void* hitCounts,
                             void* totals) {
    if (count == 0) return FYPRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_list_query(c, l, static_cast<const float4*>(in), after, count, maxHits, out, static_cast<uint32_t*>(hitCounts), static_cast<uint32_t*>(totals), false);
}

extern "C" {

void fyprt_comm_destroy(fyprt_context* c);

uint64_t fyprt_live_device_bytes(void) { return g_liveDeviceBytes.load(); }

const char* fyprt_version(void) { return "fyprt 0.1.0 gfx950 (wave64, LDS traversal stack, fp-contract off)"; }

int fyprt_create(int device_ordinal, fyprt_context** out) {
    if (!out) { g_createError = "fyprt_create: out is NULL"; return FYPRT_EINVAL; }
    *out = nullptr;
    if (device_ordinal == -1) {          // host-only context: scene ingestion + builders + exports, no device (CPU tests)
        auto* hc = new fyprt_context(); hc->device = -1; hc->hostOnly = true; *out = hc; return FYPRT_OK;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) { g_createError = std::string("no HIP device: ") + hipGetErrorString(e); return FYPRT_EHIP; }
    if (device_ordinal < 0 || device_ordinal >= count) { g_createError = "device ordinal out of range"; return FYPRT_EINVAL; }
    e = hipSetDevice(device_ordinal);
    if (e != hipSuccess) { g_createError = std::string("hipSetDevice: ") + hipGetErrorString(e); return FYPRT_EHIP; }
    auto* c = new fyprt_context(); c->device = device_ordinal;
    {   // The three streams sit on three different priority levels: HIP deals the streams of one priority level round-robin over a
        // few hardware queues (GPU_MAX_HW_QUEUES, default 4), and two streams that land on the same queue run strictly one
        // after the other.  With torch + RCCL streams in the process two of ours at one level shared a queue and nothing overlapped
        // (1.12 instead of 0.99 ms per frame); a different priority level uses a different set of queues (profiles/README.md r01).
        // `prim` is the lowest: its kernel soaks up the issue slots the others leave; the front stream, the frame's critical path, the
        // highest (against lowest measured neutral in r03, before there was a third stream); the context stream keeps the default.
        // -DFYPRT_PRIORITY_ORDER=1 / 2 build the other two assignments measured in profiles/README.md (di_split).
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        const int mid = (lo + hi) / 2;
#if FYPRT_PRIORITY_ORDER == 1
        const int pStream = hi, pFront = mid, pPrim = lo;
#elif FYPRT_PRIORITY_ORDER == 2
        const int pStream = mid, pFront = lo, pPrim = hi;
#else
        const int pStream = mid, pFront = hi, pPrim = lo;
#endif
        e = hipStreamCreateWithPriority(&c->stream.h, hipStreamNonBlocking, pStream);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->front.h, hipStreamNonBlocking, pFront);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->prim.h, hipStreamNonBlocking, pPrim);
    }
    for (int k = 0; k < 2 && e == hipSuccess; ++k)
        for (Event* ev : {&c->evFront[k], &c->evDone[k], &c->evPrim[k], &c->evTemp[k]}) if (e == hipSuccess) e = create(*ev, hipEventDisableTiming);
    if (e == hipSuccess) e = create(c->evPayload, hipEventDisableTiming);
    if (e != hipSuccess) { g_createError = std::string("streams / events: ") + hipGetErrorString(e); delete c; return FYPRT_EHIP; }
    for (auto& row : c->ring) for (auto& e : row) (void)create(e);
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0) c->numCUs = prop.multiProcessorCount; }
    if (const char* e = std::getenv("FYPRT_TOP_NODES")) c->tuning[K_TOP_NODES] = std::min(1024, std::max(0, std::atoi(e)));
    (void)c->queueCounters.alloc(8);          // two queues (frame parity): ray tail, ray-less count, head, pad each
    (void)c->rayCounter.alloc(32);            // 4 launches x (rays, box tests, triangle tests, hits, node visits, 3 unused)
    (void)hipMemset(c->rayCounter.p, 0, 256);
    *out = c;
    return FYPRT_OK;
}

void fyprt_destroy(fyprt_context* c) {
    if (!c) return;
    if (!c->hostOnly) { (void)hipSetDevice(c->device); (void)sync_all(c); fyprt_comm_destroy(c); }
    delete c;                                  // every buffer, event and stream releases itself (order: see fyprt_context)
}

const char* fyprt_last_error(const fyprt_context* c) { return c ? c->err.c_str() : g_createError.c_str(); }

int fyprt_resize(fyprt_context* c, uint32_t w, uint32_t h) {
    if (!c) return FYPRT_EINVAL;
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 31)) return c->fail(FYPRT_EINVAL, "fyprt_resize: bad size");
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, "host-only context (device -1) has no device buffers");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    c->release_denoise(); c->release_temporal(); c->release_upscale(); c->frameComplete = false; c->drop_kept_primary();
    const size_t n = (size_t)w * h;
    // cudaMemset(…, 0, …) of every buffer: Renderer.cu:333-355, :372, :393, :414
    TRY(alloc_zeroed(c, c->accum, n)); TRY(alloc_zeroed(c, c->image, n)); TRY(alloc_zeroed(c, c->payload, n)); TRY(alloc_zeroed(c, c->depth, n));
    TRY(alloc_zeroed(c, c->normalA, n)); TRY(alloc_zeroed(c, c->normalB, n));
    TRY(alloc_zeroed(c, c->di, n)); TRY(alloc_zeroed(c, c->diPrev, n)); TRY(alloc_zeroed(c, c->gi, n)); TRY(alloc_zeroed(c, c->giPrev, n)); TRY(alloc_zeroed(c, c->giHot, n * 4));
    TRY(alloc_zeroed(c, c->drec, n)); TRY(alloc_zeroed(c, c->dprevA, n)); TRY(alloc_zeroed(c, c->dprevB, n));
    HIPCHK(c, c->stagePayload.alloc(2 * n)); HIPCHK(c, c->stageRec.alloc(2 * n));
    {   // shadow-task storage: 256 slots per setup workgroup (grid padded to whole groups of 8 tile rows), + the sort scratch
        const size_t tilesX = (w + 15u) / 16u, tilesY = (h + 15u) / 16u;
        const size_t maxGroups = std::max(tilesX * ((tilesY + 7u) / 8u) * 8u, ((tilesX * tilesY + 7u) / 8u) * 8u);
        HIPCHK(c, c->shadowTasks.alloc((size_t)maxGroups * 256u * 4u * 2u));   // two queues (frame parity) of 64-byte tasks
        c->queueStride = (size_t)maxGroups * 256u * 4u;
        // the sort scratch alternates with the frame parity like the queues: frame N+1's setup / scan / scatter (front stream) run
        // beside frame N's trace kernel, which still reads its `sorted` index
        c->sortGroups = maxGroups;
        HIPCHK(c, c->sortCounts.alloc(4 * maxGroups)); HIPCHK(c, c->sortKeys.alloc(2 * maxGroups * 256u)); HIPCHK(c, c->sortHist.alloc(2 * maxGroups * kSortBins));
        HIPCHK(c, c->sortOffset.alloc(2 * maxGroups * kSortBins)); HIPCHK(c, c->sortTotal.alloc(2 * kSortBins)); HIPCHK(c, c->sortIndex.alloc(2 * maxGroups * 256u));
    }
    HIPCHK(c, sync_all(c));
    c->part1Pending = false;
    c->stripeRows = 0; c->stripeParts = 1; c->stripePart = 0;
    c->W = w; c->H = h; c->frameIndex = 1; c->normalFlip = false; c->dprevFlip = false; c->lastTech = -1; c->lastRestir = -1; c->externalImage = nullptr;
    c->histDI[0] = c->histGI[0] = 0; c->histDI[1] = c->histGI[1] = h;        // zero-filled history: "valid" everywhere, M = 0
    if (!c->rowsSet || c->rowEnd > h) { c->rowBegin = 0; c->rowEnd = h; c->halo = 0; c->rowsSet = false; }
    return FYPRT_OK;
}

// rows of the frame a striped context owns: the stripes k * parts + part, the last one cut at the frame's end
static uint32_t stripe_row_count(uint32_t H, uint32_t stripe, uint32_t parts, uint32_t part) {
    uint32_t n = 0;
    for (uint64_t r0 = (uint64_t)part * stripe; r0 < H; r0 += (uint64_t)parts * stripe) n += (uint32_t)std::min<uint64_t>(stripe, H - r0);
    return n;
}

int fyprt_set_rows(fyprt_context* c, uint32_t b, uint32_t e, uint32_t halo) {
    if (!c) return FYPRT_EINVAL;
    if (c->H == 0) return c->fail(FYPRT_ESTATE, "fyprt_set_rows before fyprt_resize");
    if (b >= e || e > c->H) return c->fail(FYPRT_EINVAL, "fyprt_set_rows: need row_begin < row_end <= height");
    c->rowBegin = b; c->rowEnd = e; c->halo = halo; c->rowsSet = true; c->stripeRows = 0;
    return FYPRT_OK;
}
// The interleaved split of SURVEY.md §8(e) for the techniques whose pixels are independent (0-6): the frame is cut into stripes of
// `stripe_rows` rows and this context renders every `parts`-th of them, starting with stripe `part` — the stripes of one context
// sample the whole image, so the parts cost the same without any balancing.  stripe_rows 0 returns to the band of fyprt_set_rows
// (whole frame if none was set).  ReSTIR frames refuse a striped context: spatial reuse reads the rows around a pixel.
int fyprt_set_row_stripes(fyprt_context* c, uint32_t stripe_rows, uint32_t parts, uint32_t part) {
    if (!c) return FYPRT_EINVAL;
    if (c->H == 0) return c->fail(FYPRT_ESTATE, "fyprt_set_row_stripes before fyprt_resize");
    if (stripe_rows == 0) { c->stripeRows = 0; c->stripeParts = 1; c->stripePart = 0; return FYPRT_OK; }
    if (parts == 0 || part >= parts) return c->fail(FYPRT_EINVAL, "fyprt_set_row_stripes: need part < parts");
    if (stripe_row_count(c->H, stripe_rows, parts, part) == 0) return c->fail(FYPRT_EINVAL, "fyprt_set_row_stripes: this part owns no row (fewer stripes than parts)");
    c->stripeRows = stripe_rows; c->stripeParts = parts; c->stripePart = part;
    c->rowBegin = 0; c->rowEnd = c->H; c->halo = 0; c->rowsSet = false;
    return FYPRT_OK;
}

// the node array back from the device, into HOST form (rt_host.h: inner references are indices on the host, byte offsets on the device)
static int download_nodes(fyprt_context* c) {
    if (c->hostBvh.nodes.empty()) return FYPRT_OK;
    HIPCHK(c, hipMemcpy(c->hostBvh.nodes.data(), c->nodes.p, c->hostBvh.nodes.size() * 64, hipMemcpyDeviceToHost));
    rth::nodes_to_host_form(c->hostBvh.nodes.data(), c->hostBvh.nodes.size());
    return FYPRT_OK;
}

}  // extern "C"
// what the builders below and the tree edits share
#include "rt_tree_host.h"
// The query filter's device data for the table and the tree as they are (rt_filter.h), enqueued on the context stream: the mesh table
// up, one launch over the leaf records, one launch per level of the refit passes' grouping (bottom level first; the single-launch form
// over parent links would need the partial refit's maps, which the same edits invalidate: DESIGN.md §4, "Query filters").  Buffers are
// reallocated only when their size changes.  Whoever changes table or tree does so with the stream idle, so the host tables are free.
static int ensure_query_filter(fyprt_context* c) {
    if (c->filterValid) return FYPRT_OK;
    if (c->meshMasks.size() != c->topoMeshes.size()) return c->fail(FYPRT_ESTATE, "query filter: the mask table does not match the scene's meshes");
    std::vector<std::pair<uint32_t, uint32_t>> byFirst;
    for (size_t m = 0; m < c->topoMeshes.size(); ++m) if (c->topoMeshes[m].triangle_count) byFirst.push_back({c->topoMeshes[m].first_triangle, c->meshMasks[m]});
    std::sort(byFirst.begin(), byFirst.end());
    c->filterFirstHost.clear(); c->filterMaskHost.clear();
    for (const auto& e : byFirst) { c->filterFirstHost.push_back(e.first); c->filterMaskHost.push_back(e.second); }
    const uint32_t nMesh = (uint32_t)byFirst.size(), nLeaf = (uint32_t)(c->leafTris.n / 3), nNodes = (uint32_t)(c->nodes.n / 4);
    if (c->filterFirst.n != nMesh) { HIPCHK(c, c->filterFirst.alloc(nMesh)); HIPCHK(c, c->filterMeshMask.alloc(nMesh)); }
    if (c->leafMask.n != nLeaf) HIPCHK(c, c->leafMask.alloc(nLeaf));
    if (c->nodeMask.n != nNodes) HIPCHK(c, c->nodeMask.alloc(nNodes));
    if (nMesh) {
        HIPCHK(c, hipMemcpyAsync(c->filterFirst.p, c->filterFirstHost.data(), (size_t)nMesh * 4u, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->filterMeshMask.p, c->filterMaskHost.data(), (size_t)nMesh * 4u, hipMemcpyHostToDevice, c->stream));
    }
    if (nLeaf) hipLaunchKernelGGL(k_filter_leaf_masks, dim3((nLeaf + 255u) / 256u), dim3(256), 0, c->stream, (const float4*)c->leafTris.p, nLeaf,
                                  (const uint32_t*)c->filterFirst.p, (const uint32_t*)c->filterMeshMask.p, nMesh, c->leafMask.p);
    if (nNodes && (c->levelOffset.empty() || c->levelOffset.back() != nNodes || c->levelNodes.n < nNodes))
        return c->fail(FYPRT_ESTATE, "query filter: the level grouping does not describe the node array");
    if (nNodes)
        for_each_level(c->levelOffset, [&](uint32_t first, uint32_t count, dim3 grid) {
            hipLaunchKernelGGL(k_filter_level, grid, dim3(kLevelBlock), 0, c->stream, (const float4*)c->nodes.p, (const uint32_t*)(c->levelNodes.p + first), count, nNodes,
                               (const uint32_t*)c->leafMask.p, nLeaf, c->nodeMask.p);
        });
    HIPCHK(c, hipGetLastError());
    c->filterValid = true; ++c->filterBuilds;
    return FYPRT_OK;
}
extern "C" {
// the refit pass over the whole tree (rt_refit.h): leaf triangles from the per-triangle positions, then boxes + quantisation
// level by level, bottom level first (the grouping's levels are the tree's: upload_level_grouping)
static int run_refit(fyprt_context* c) {
    const uint32_t nLeaf = (uint32_t)c->hostBvh.tris.size();
    if (nLeaf) hipLaunchKernelGGL(k_refresh_leaf_tris, dim3((nLeaf + 255u) / 256u), dim3(256), 0, c->stream, c->triPos.p, c->leafTris.p, nLeaf);
    for_each_level(c->levelOffset, [&](uint32_t first, uint32_t count, dim3 grid) {
        hipLaunchKernelGGL(k_refit_level, grid, dim3(kLevelBlock), 0, c->stream, c->nodes.p, c->levelNodes.p + first, count, c->leafTris.p, c->triPos.p, c->nodeBox.p);
    });
    HIPCHK(c, hipGetLastError());
    c->nodeBoxValid = true;
    return FYPRT_OK;
}

// Device builder (tuning key 12, rt_lbvh.h): Morton keys -> radix sort -> Karras radix tree -> BFS collapse into 4-wide nodes ->
// level counts, over the triangle range [firstTri, firstTri + nT) — the whole scene for an upload, the appended triangles for
// fyprt_append_meshes; `verts` span the range's Morton grid.  Destination: the leaf records (triangle indices in sorted order) go to
// c->leafTris from record `leafBase` on, where the caller has made room for nT of them; the nodes (topology only, references relative
// to the tree: node 0 is its root, leaf record 0 is record leafBase) are left in the scratch `wide`, from where the caller takes
// them.  Boxes come from the refit pass.  kLbvhTooDeep: more than 31 wide levels.
constexpr int kLbvhTooDeep = -1000;
struct LbvhTree { uint32_t nodes = 0, levels = 0; };
static int env_int(const char* name, int fallback) { const char* v = std::getenv(name); return (v && *v) ? std::atoi(v) : fallback; }
static int build_device_lbvh(fyprt_context* c, const fyprt_vertex* verts, uint32_t nV, uint32_t firstTri, uint32_t nT, bool ploc, size_t leafBase, DevBuf<float4>& wide, LbvhTree* tree) {
    rth::HostBox grid;
    for (uint32_t i = 0; i < nV; ++i) grid.grow(verts[i].position);
    const float *lo = grid.lo, *hi = grid.hi;
    float3 l3 = make_float3(lo[0], lo[1], lo[2]), ie = make_float3(hi[0] > lo[0] ? 1.0f / (hi[0] - lo[0]) : 0.0f, hi[1] > lo[1] ? 1.0f / (hi[1] - lo[1]) : 0.0f, hi[2] > lo[2] ? 1.0f / (hi[2] - lo[2]) : 0.0f);
    // scratch of the build, freed on every way out
    DevBuf<unsigned long long> keysA, keysB; DevBuf<uint32_t> valsA, valsB, parentOfNode, parentOfLeaf, arrived; DevBuf<float> box; DevBuf<RadixNode> radix; DevBuf<CollapseItem> qA, qB; DevBuf<uint32_t> counters; DevBuf<uint8_t> temp;
    DevBuf<uint32_t> clA, clB, nearest; DevBuf<uint8_t> keep, selTemp;                          // PLOC
    if (!ploc) {
        HIPCHK(c, parentOfNode.alloc(nT)); HIPCHK(c, parentOfLeaf.alloc(nT)); HIPCHK(c, arrived.alloc(nT)); HIPCHK(c, box.alloc((size_t)nT * 6));
        HIPCHK(c, hipMemsetAsync(arrived.p, 0, (size_t)nT * 4, c->stream));
    } else {
        HIPCHK(c, box.alloc((size_t)nT * 12)); HIPCHK(c, clA.alloc(nT)); HIPCHK(c, clB.alloc(nT)); HIPCHK(c, nearest.alloc(nT)); HIPCHK(c, keep.alloc(nT));
    }
    HIPCHK(c, keysA.alloc(nT)); HIPCHK(c, keysB.alloc(nT)); HIPCHK(c, valsA.alloc(nT)); HIPCHK(c, valsB.alloc(nT)); HIPCHK(c, radix.alloc(nT)); HIPCHK(c, qA.alloc(nT)); HIPCHK(c, qB.alloc(nT));
    HIPCHK(c, counters.alloc(4)); HIPCHK(c, wide.alloc((size_t)nT * 4));
    hipLaunchKernelGGL(k_lbvh_keys, dim3((nT + 255u) / 256u), dim3(256), 0, c->stream, c->triPos.p, firstTri, nT, l3, ie, keysA.p, valsA.p);
    size_t tempBytes = 0;
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tempBytes, keysA.p, keysB.p, valsA.p, valsB.p, (int)nT, 0, 63, c->stream));
    HIPCHK(c, temp.alloc(tempBytes));
    HIPCHK(c, hipcub::DeviceRadixSort::SortPairs(temp.p, tempBytes, keysA.p, keysB.p, valsA.p, valsB.p, (int)nT, 0, 63, c->stream));
    uint32_t rootNode = 0;
    if (!ploc) {
        hipLaunchKernelGGL(k_lbvh_radix, dim3((nT + 255u) / 256u), dim3(256), 0, c->stream, keysB.p, (int)nT, radix.p, parentOfNode.p, parentOfLeaf.p);
        hipLaunchKernelGGL(k_lbvh_boxes, dim3((nT + 255u) / 256u), dim3(256), 0, c->stream, radix.p, parentOfNode.p, parentOfLeaf.p, valsB.p, c->triPos.p, nT, arrived.p, box.p);
    } else {
        // PLOC rounds over the sorted order (rt_lbvh.h).  Every round has at least one mutual pair (the pair of globally smallest
        // union), real scenes lose 20-35 % of their clusters per round (54 rounds for 1 M triangles).  A round over a LONG list
        // that loses less than 1/16 is followed by a forced one (neighbours i, i ^ 1 merge), which halves the list, so degenerate
        // input cannot take O(n) rounds of O(n) work; short lists (the top of the tree, where quality counts most) are never forced.
        const int radius = std::min(kPlocMaxRadius, std::max(1, env_int("FYPRT_PLOC_RADIUS", 16)));
        hipLaunchKernelGGL(k_ploc_leaves, dim3((nT + 255u) / 256u), dim3(256), 0, c->stream, valsB.p, c->triPos.p, nT, box.p, clA.p);
        HIPCHK(c, hipMemsetAsync(counters.p + 2, 0, 8, c->stream));                     // [2] binary nodes allocated, [3] clusters kept by the compaction
        size_t selBytes = 0;
        HIPCHK(c, hipcub::DeviceSelect::Flagged(nullptr, selBytes, clB.p, keep.p, clA.p, counters.p + 3, (int)nT, c->stream));
        HIPCHK(c, selTemp.alloc(selBytes));
        uint32_t n = nT; uint32_t* cur = clA.p; uint32_t* merged = clB.p; int force = 0, rounds = 0;
        while (n > 1) {
            const dim3 g((n + kPlocBlock - 1) / kPlocBlock);
            hipLaunchKernelGGL(k_ploc_nearest, g, dim3(kPlocBlock), 0, c->stream, (const uint32_t*)cur, n, (const float*)box.p, nT, radius, force, nearest.p);
            hipLaunchKernelGGL(k_ploc_merge, g, dim3(kPlocBlock), 0, c->stream, (const uint32_t*)cur, (const uint32_t*)nearest.p, n, nT, radix.p, box.p, counters.p + 2, merged, keep.p);
            hipError_t e = hipcub::DeviceSelect::Flagged(selTemp.p, selBytes, merged, keep.p, cur, counters.p + 3, (int)n, c->stream);     // back into `cur`, order kept
            uint32_t kept = 0;
            if (e == hipSuccess) e = hipMemcpyAsync(&kept, counters.p + 3, 4, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess || kept == 0 || kept >= n) return e != hipSuccess ? c->hip(e, "PLOC round") : c->fail(FYPRT_EHIP, "PLOC round made no progress");
            if (env_int("FYPRT_BVH_DEBUG", 0)) std::fprintf(stderr, "PLOC round %d: %u -> %u clusters%s\n", rounds, n, kept, force ? " (forced)" : "");
            force = (!force && n > 4096u && kept > n - n / 16u) ? 1 : 0;
            n = kept; ++rounds;
        }
        HIPCHK(c, hipMemcpy(&rootNode, cur, 4, hipMemcpyDeviceToHost));
        c->lastBuildRounds = rounds;
    }
    // BFS collapse, one launch per level; the nodes of a level are contiguous: [levelFirst[l], levelFirst[l + 1])
    const CollapseItem rootItem{rootNode, 0u, 0u};
    uint32_t h_counters[2] = {1u, 0u};
    HIPCHK(c, hipMemcpyAsync(qA.p, &rootItem, sizeof rootItem, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(counters.p, h_counters, 8, hipMemcpyHostToDevice, c->stream));
    std::vector<uint32_t> levelFirst{0u};
    uint32_t nIn = 1, total = 1;
    CollapseItem *in = qA.p, *out = qB.p;
    while (nIn) {
        hipLaunchKernelGGL(k_lbvh_collapse, dim3((nIn + 127u) / 128u), dim3(128), 0, c->stream, (const RadixNode*)radix.p, (const float*)box.p, (const uint32_t*)valsB.p, (const CollapseItem*)in, nIn, out, counters.p, wide.p, c->leafTris.p + leafBase * 3);
        HIPCHK(c, hipMemcpyAsync(h_counters, counters.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        levelFirst.push_back(total);
        nIn = h_counters[1]; total = h_counters[0];
        h_counters[1] = 0;
        HIPCHK(c, hipMemcpyAsync(counters.p + 1, &h_counters[1], 4, hipMemcpyHostToDevice, c->stream));
        std::swap(in, out);
        if (levelFirst.size() > rth::kStackBudget + 1u) return kLbvhTooDeep;
    }
    const uint32_t nLevels = (uint32_t)levelFirst.size() - 1u;                      // BFS levels = wide levels of the tree
    for (uint32_t l = nLevels; l-- > 0;) {
        const uint32_t first = levelFirst[l], count = levelFirst[l + 1] - first;
        if (count) hipLaunchKernelGGL(k_lbvh_levels, dim3((count + 127u) / 128u), dim3(128), 0, c->stream, wide.p, first, count);
    }
    HIPCHK(c, hipGetLastError());
    if (total >= rth::kMaxNodes) return c->fail(FYPRT_EINVAL, "device builder: too many nodes for the node reference range");
    tree->nodes = total; tree->levels = nLevels;
    return FYPRT_OK;
}

// The host light trees (c->hostLt) onto the device, with the emitter -> TLAS-leaf table, and into the scene descriptor.
// `keep` (a removal): the per-mesh and per-triangle tables are written into the buffers they have (the scene shrank: they fit), so their
// capacity stays, as the capacity of the scene's arrays does, and a later append of the removed size fits without growing
static int upload_light_table(fyprt_context* c, DevBuf<uint32_t>& b, const uint32_t* src, size_t count, bool keep) {
    if (!keep || c->hostOnly || count > b.cap) return alloc_upload(c, b, src, count);
    b.n = count;
    return upload(c, b.p, src, b.bytes());
}
static int upload_light_trees(fyprt_context* c, uint32_t nT, uint32_t nM, bool keep = false) {
    const rth::LightTrees& lt = c->hostLt;
    static_assert(sizeof(DevLTNode) == sizeof(fyprt_lighttree_node), "light tree node layout");
    TRY(alloc_upload(c, c->ltTlas, lt.tlas.data(), lt.tlas.size())); TRY(alloc_upload(c, c->ltBlas, lt.blas.data(), lt.blas.size()));
    TRY(upload_light_table(c, c->ltFirst, lt.first.data(), nM, keep)); TRY(upload_light_table(c, c->ltCount, lt.count.data(), nM, keep)); TRY(upload_light_table(c, c->ltRoot, lt.root.data(), nM, keep));
    // ComputeDirectEmitterPMF (LightTree.cu:170-199) starts with a linear search for the first TLAS leaf whose mesh tree
    // holds the emitter; the answer does not depend on the shading point, so it is tabled per triangle here (same search
    // order: first match wins).
    std::vector<uint32_t> leafOfTri(nT, ~0u);
    for (uint32_t i = 0; i < (uint32_t)lt.tlas.size(); ++i) {
        if (!lt.tlas[i].is_leaf) continue;
        const uint32_t mesh = lt.tlas[i].right_or_emitter;
        if (mesh >= nM) continue;
        for (uint32_t j = 0; j < lt.count[mesh]; ++j) {
            const fyprt_lighttree_node& n = lt.blas[lt.first[mesh] + j];
            if (n.is_leaf && n.right_or_emitter < nT && leafOfTri[n.right_or_emitter] == ~0u) leafOfTri[n.right_or_emitter] = i;
        }
    }
    TRY(upload_light_table(c, c->ltLeafOfTri, leafOfTri.data(), nT, keep));
    DevScene& d = c->dsc;
    d.ltLeafOfTri = c->ltLeafOfTri.p; d.ltTlas = c->ltTlas.p; d.ltTlasCount = (uint32_t)lt.tlas.size(); d.ltTlasRoot = lt.tlasRoot;
    d.ltBlas = c->ltBlas.p; d.ltFirst = c->ltFirst.p; d.ltCount = c->ltCount.p; d.ltRoot = c->ltRoot.p;
    return FYPRT_OK;
}

// An append that brings no emitter changes no light tree, but the per-triangle and per-mesh tables must cover the combined scene as
// upload_light_trees leaves them: a removal sizes its tables by the scene it finds, and fyprt_remove_meshes promises never to grow the
// device memory.  The tables grow like the scene's arrays (grow_buffer) and move device to device; the new triangles lie in no TLAS leaf
// and the new meshes have no tree (their entries of c->hostLt go up: 12 bytes per new mesh).  All streams are idle.
static int extend_light_tables(fyprt_context* c, uint32_t nT, uint32_t nM) {
    const rth::LightTrees& lt = c->hostLt;
    const size_t t0 = c->ltLeafOfTri.n, m0 = c->ltFirst.n;
    if (nT < t0 || nM < m0 || lt.first.size() < nM) return c->fail(FYPRT_EHIP, "fyprt_append_meshes: the light tables do not cover the scene before the append");
    TRY(grow_buffer(c, c->ltLeafOfTri, nT)); TRY(grow_buffer(c, c->ltFirst, nM)); TRY(grow_buffer(c, c->ltCount, nM)); TRY(grow_buffer(c, c->ltRoot, nM));
    if (c->hostOnly) return FYPRT_OK;
    if (nT > t0) HIPCHK(c, hipMemsetAsync(c->ltLeafOfTri.p + t0, 0xFF, (nT - t0) * sizeof(uint32_t), c->stream));
    if (nM > m0) {
        TRY(upload(c, c->ltFirst.p + m0, lt.first.data() + m0, (nM - m0) * sizeof(uint32_t)));
        TRY(upload(c, c->ltCount.p + m0, lt.count.data() + m0, (nM - m0) * sizeof(uint32_t)));
        TRY(upload(c, c->ltRoot.p + m0, lt.root.data() + m0, (nM - m0) * sizeof(uint32_t)));
    }
    DevScene& d = c->dsc;
    d.ltLeafOfTri = c->ltLeafOfTri.p; d.ltFirst = c->ltFirst.p; d.ltCount = c->ltCount.p; d.ltRoot = c->ltRoot.p;
    return FYPRT_OK;
}

// The acceleration structure of the scene whose per-triangle records are on the device (c->triPos): built on the host (binned SAH +
// collapse, bvh_build.cpp) or, with tuning key 12, on the device (LBVH / PLOC + collapse, rt_lbvh.h, boxes by the refit pass).  Leaves
// c->nodes, c->leafTris, the level grouping, c->nodeBox and the host's copy c->hostBvh.  `what`: the caller's name for error texts.
static int build_scene_tree(fyprt_context* c, const char* what, const fyprt_vertex* verts, uint32_t nV, const uint8_t* tb, uint32_t stride, const fyprt_mesh* meshes, uint32_t nM, uint32_t nT) {
    bool deviceBuild = !c->hostOnly && c->tuning[K_BUILDER] != 0 && nT > 4;
    c->linksValid = false;                     // another tree: the partial refit's maps go with the old one
    if (deviceBuild) {
        DevBuf<float4> wide; LbvhTree tree;
        HIPCHK(c, c->leafTris.alloc((size_t)nT * 3));
        const int rc = build_device_lbvh(c, verts, nV, 0, nT, c->tuning[K_BUILDER] == 2, 0, wide, &tree);
        if (rc == kLbvhTooDeep) deviceBuild = false;                      // > 31 wide levels: the host builder bounds them
        else if (rc != FYPRT_OK) return rc;
        else {
            HIPCHK(c, c->nodes.alloc((size_t)tree.nodes * 4));
            HIPCHK(c, hipMemcpyAsync(c->nodes.p, wide.p, (size_t)tree.nodes * 64, hipMemcpyDeviceToDevice, c->stream));
            rth::SceneBVH& b = c->hostBvh; b = rth::SceneBVH();
            b.nodes.resize(tree.nodes); b.tris.resize(nT); b.rootRef = 0; b.levels = tree.levels;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            TRY(download_nodes(c));                                        // topology + meta: the level grouping needs it
        }
    }
    if (!deviceBuild) {
        rth::BuildSceneBVH(verts, tb, stride, meshes, nM, c->hostBvh);
        if (c->hostBvh.levels > rth::kStackBudget || c->hostBvh.nodes.size() >= (size_t)rth::kMaxNodes)
            return c->fail(FYPRT_EINVAL, std::string(what) + ": acceleration structure (" + std::to_string(c->hostBvh.levels) + " levels, " +
                           std::to_string(c->hostBvh.nodes.size()) + " nodes) exceeds the traversal stack / node index range");
        std::vector<rth::Node> dn;                                        // the array in device form (inner references = byte offsets)
        if (!c->hostOnly) { dn = c->hostBvh.nodes; rth::nodes_to_device_form(dn.data(), dn.size()); }
        TRY(alloc_upload(c, c->nodes, dn.data(), c->hostBvh.nodes.size() * 4));
        TRY(alloc_upload(c, c->leafTris, c->hostBvh.tris.data(), c->hostBvh.tris.size() * 3));
    }
    // refit support: the nodes grouped by level, a box per node
    TRY(upload_level_grouping(c, false)); HIPCHK(c, c->nodeBox.alloc(c->hostBvh.nodes.size() * 2, c->hostOnly));
    c->hostBvhStale = false; c->nodeBoxValid = deviceBuild;
    if (deviceBuild) {                     // the device builder leaves boxes and quantisation to the refit pass
        TRY(run_refit(c));
        HIPCHK(c, sync_all(c));
        TRY(download_nodes(c));
        HIPCHK(c, hipMemcpy(c->hostBvh.tris.data(), c->leafTris.p, c->hostBvh.tris.size() * 48, hipMemcpyDeviceToHost));
    }
    return FYPRT_OK;
}

int fyprt_upload_scene(fyprt_context* c, const fyprt_scene_desc* s) {
    if (!c || !s) return FYPRT_EINVAL;
    if ((s->triangle_count && (!s->triangles || !s->vertices || s->triangle_stride < 16)) || (s->mesh_count && !s->meshes) ||
        (s->material_count && !s->materials))
        return c->fail(FYPRT_EINVAL, "fyprt_upload_scene: NULL array with non-zero count");
    if (!c->hostOnly) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c)); }
    c->frameComplete = false;                  // the payload's triangle indices belong to the scene they were traced in (fyprt_denoise)
    c->drop_kept_primary();
    c->drop_history(); c->release_snapshot();  // world positions of another scene are not comparable (fyprt_denoise_temporal)
    c->meshMasks.clear(); c->release_query_filter(); c->queryMask = 0xFFFFFFFFu;     // the query filter belongs to the scene it was set for
    const uint8_t* tb = (const uint8_t*)s->triangles;
    auto tri = [&](uint32_t i) { return reinterpret_cast<const uint32_t*>(tb + (size_t)i * s->triangle_stride); };
    for (uint32_t i = 0; i < s->triangle_count; ++i) {
        const uint32_t* t = tri(i);
        if (t[0] >= s->vertex_count || t[1] >= s->vertex_count || t[2] >= s->vertex_count || (int32_t)t[3] < 0 || t[3] >= s->material_count)
            return c->fail(FYPRT_EINVAL, "fyprt_upload_scene: triangle " + std::to_string(i) + " references a vertex/material out of range");
    }
    uint64_t covered = 0;
    for (uint32_t m = 0; m < s->mesh_count; ++m) {
        const fyprt_mesh& me = s->meshes[m];
        if ((uint64_t)me.first_triangle + me.triangle_count > s->triangle_count || me.material_index < 0 || (uint32_t)me.material_index >= s->material_count)
            return c->fail(FYPRT_EINVAL, "fyprt_upload_scene: mesh " + std::to_string(m) + " range/material out of bounds");
        covered += me.triangle_count;
    }
    if (covered != s->triangle_count) return c->fail(FYPRT_EINVAL, "fyprt_upload_scene: meshes must partition the triangle list");
    // per-triangle gather records
    const uint32_t nT = s->triangle_count;
    std::vector<float> pos((size_t)nT * 12), shade((size_t)nT * 16);
    for (uint32_t i = 0; i < nT; ++i) {
        const uint32_t* t = tri(i);
        const fyprt_vertex &a = s->vertices[t[0]], &b = s->vertices[t[1]], &cc = s->vertices[t[2]];
        float* p = &pos[(size_t)i * 12]; float* q = &shade[(size_t)i * 16];
        float matBits; std::memcpy(&matBits, &t[3], 4);
        p[0] = a.position[0]; p[1] = a.position[1]; p[2] = a.position[2]; p[3] = matBits;
        p[4] = b.position[0]; p[5] = b.position[1]; p[6] = b.position[2]; p[7] = 0.0f;
        p[8] = cc.position[0]; p[9] = cc.position[1]; p[10] = cc.position[2]; p[11] = 0.0f;
        q[0] = a.normal[0]; q[1] = a.normal[1]; q[2] = a.normal[2]; q[3] = a.uv[0];
        q[4] = b.normal[0]; q[5] = b.normal[1]; q[6] = b.normal[2]; q[7] = a.uv[1];
        q[8] = cc.normal[0]; q[9] = cc.normal[1]; q[10] = cc.normal[2]; q[11] = b.uv[0];
        q[12] = b.uv[1]; q[13] = cc.uv[0]; q[14] = cc.uv[1]; q[15] = matBits;
    }
    TRY(alloc_upload(c, c->triPos, pos.data(), (size_t)nT * 3)); TRY(alloc_upload(c, c->triShade, shade.data(), (size_t)nT * 4));
    // acceleration structure (ours), on the host or, with tuning key 12, on the device from the records above
    TRY(build_scene_tree(c, "fyprt_upload_scene", s->vertices, s->vertex_count, tb, s->triangle_stride, s->meshes, s->mesh_count, nT));
    // refit support: vertices + per-triangle indices on the device
    c->vertexCount = s->vertex_count; c->hostVertsStale = false;
    c->hostVerts.assign(s->vertices, s->vertices + s->vertex_count); c->objVerts.release(); c->meshFirstVertex.clear();
    c->topoTris.resize((size_t)nT * 4);
    for (uint32_t i = 0; i < nT; ++i) std::memcpy(&c->topoTris[(size_t)i * 4], tri(i), 16);
    c->topoMeshes.assign(s->meshes, s->meshes + s->mesh_count); c->topoMats.assign(s->materials, s->materials + s->material_count);
    c->prebuiltLightTrees = s->light_trees && s->light_trees->tlas_nodes;
    TRY(alloc_upload(c, c->dverts, s->vertices, s->vertex_count)); TRY(alloc_upload(c, c->triIdx, c->topoTris.data(), nT));
    // materials (Material.cuh:7-16 -> 3 quads)
    std::vector<float> mats; std::vector<char> emissiveMat;
    pack_materials(s->materials, s->material_count, mats, emissiveMat);
    TRY(alloc_upload(c, c->mats, mats.data(), (size_t)s->material_count * 3));
    // textures
    c->texPixels.clear(); c->texPixels.resize(s->texture_count);
    std::vector<DevTexture> tt(s->texture_count);
    for (uint32_t i = 0; i < s->texture_count; ++i) {
        const fyprt_texture& t = s->textures[i];
        if (!t.pixels || t.width == 0 || t.height == 0) return c->fail(FYPRT_EINVAL, "fyprt_upload_scene: empty texture");
        TRY(alloc_upload(c, c->texPixels[i], t.pixels, (size_t)t.width * t.height));
        tt[i] = DevTexture{c->texPixels[i].p, t.width, t.height, 0};
    }
    TRY(alloc_upload(c, c->texTable, tt.data(), s->texture_count));
    c->texHost.swap(tt);
    // emissive list (Scene::InitSceneEmissiveTriangles, Scene.cpp:209-221)
    std::vector<uint32_t> em;
    if (s->emissive_triangles) em.assign(s->emissive_triangles, s->emissive_triangles + s->emissive_count);
    else for (uint32_t i = 0; i < nT; ++i) if (emissiveMat[tri(i)[3]]) em.push_back(i);
    for (uint32_t e : em) if (e >= nT) return c->fail(FYPRT_EINVAL, "fyprt_upload_scene: emissive triangle index out of range");
    TRY(alloc_upload(c, c->emissive, em.data(), em.size()));
    c->emissiveExplicit = s->emissive_triangles != nullptr;
    // light trees: prebuilt (reference shape) or ours
    rth::LightTrees& lt = c->hostLt; lt = rth::LightTrees();
    c->meshCount = s->mesh_count;
    if (s->light_trees && s->light_trees->tlas_nodes) {
        const fyprt_lighttrees& L = *s->light_trees;
        lt.tlas.assign(L.tlas_nodes, L.tlas_nodes + L.tlas_node_count); lt.tlasRoot = L.tlas_root;
        lt.first.assign(L.blas_first, L.blas_first + s->mesh_count); lt.count.assign(L.blas_count, L.blas_count + s->mesh_count);
        lt.root.assign(L.blas_root, L.blas_root + s->mesh_count);
        uint32_t total = 0; for (uint32_t m = 0; m < s->mesh_count; ++m) total = std::max(total, lt.first[m] + lt.count[m]);
        lt.blas.assign(L.blas_nodes, L.blas_nodes + total);
    } else {
        rth::BuildLightTrees(s->vertices, tb, s->triangle_stride, s->meshes, s->mesh_count, s->materials, lt);
    }
    TRY(upload_light_trees(c, nT, s->mesh_count));
    DevScene& d = c->dsc;
    set_scene_triangles(c, nT);
    d.mats = c->mats.p; d.textures = c->texTable.p; d.textureCount = s->texture_count;
    d.emissive = c->emissive.p; d.emissiveCount = (uint32_t)em.size();
    d.rayCounter = nullptr; d.topCount = 0u; d.stackBudget = 0; d.nodeQuorum = 0u;     // per launch: every launch sets them on its own copy
    // per-light records for ReSTIR DI, computed on the device with the kernels' own arithmetic
    HIPCHK(c, c->lightRecs.alloc(em.size() * 3, c->hostOnly));
    d.lightRecs = c->lightRecs.p;
    TRY(launch_light_records(c));
    if (!c->hostOnly && !em.empty()) HIPCHK(c, sync_all(c));
    c->hostEmissive.swap(em);
    c->haveScene = true;
    return FYPRT_OK;
}

// (Re)build the light trees from the given vertices with the stored topology and upload them (+ the emitter -> TLAS-leaf table).
static int rebuild_light_trees(fyprt_context* c, const fyprt_vertex* verts, const uint8_t* touched = nullptr, bool keep = false) {
    rth::LightTrees& lt = c->hostLt;
    if (!touched) lt = rth::LightTrees();
    const uint32_t nT = (uint32_t)(c->topoTris.size() / 4), nM = (uint32_t)c->topoMeshes.size();
    rth::BuildLightTrees(verts, (const uint8_t*)c->topoTris.data(), 16, c->topoMeshes.data(), nM, c->topoMats.data(), lt, touched);
    return upload_light_trees(c, nT, nM, keep);
}

// What a geometry edit means to the temporal denoiser (all streams idle).  Motion mode off: the history is dropped.  On: it is kept, and
// the first edit after a temporal call copies the world vertices that call's frame was traced in: device to device on the context
// stream, so ahead of whatever the edit enqueues there.  An edit that writes dverts any other way waits for the copy first.
static int temporal_edit_begin(fyprt_context* c) {
    if (!c->dtMotion) { c->dtValid = false; return FYPRT_OK; }
    if (!c->dtValid || c->dtSnapPending) return FYPRT_OK;
    const uint32_t nT = (uint32_t)(c->topoTris.size() / 4);
    if (c->dtSnap.n != c->dverts.n) HIPCHK(c, c->dtSnap.alloc(c->dverts.n));
    if (c->dtMoved.n != nT) HIPCHK(c, c->dtMoved.alloc(nT));
    if (c->dverts.n) HIPCHK(c, hipMemcpyAsync(c->dtSnap.p, c->dverts.p, c->dverts.bytes(), hipMemcpyDeviceToDevice, c->stream));
    if (nT) HIPCHK(c, hipMemsetAsync(c->dtMoved.p, 0, nT, c->stream));
    c->dtSnapPending = true; c->dtEditLo = c->dtEditHi = 0;
    return FYPRT_OK;
}
// ... and every edit widens the triangle range the next temporal call compares with the snapshot by [firstTri, firstTri + triCount)
static void temporal_edit_range(fyprt_context* c, uint32_t firstTri, uint32_t triCount) {
    if (!c->dtSnapPending || !triCount) return;
    const bool empty = c->dtEditHi == c->dtEditLo;
    c->dtEditLo = empty ? firstTri : std::min(c->dtEditLo, firstTri);
    c->dtEditHi = empty ? firstTri + triCount : std::max(c->dtEditHi, firstTri + triCount);
}

}  // extern "C"
// the tree's part of the scene edits: graft (append, regraft), partial refit (geometry edits), prune (removal, regraft), surface-area cost
#include "rt_partial.h"
#include "rt_graft.h"
#include "rt_prune.h"
#include "rt_treecost.h"
extern "C" {

// ---- what the edit entry points below share
// The state an edit needs, asked for flag by flag and checked in this order; `who`: the entry point's name, which starts every text.
// Argument checks stay with the entry points, each of which keeps its own order of the two kinds.
enum : unsigned { kNeedScene = 1u, kNeedSceneAndRanges = 2u, kNeedRanges = 4u, kNeedOwnLightTrees = 8u, kNeedDevice = 16u };
static int edit_check_state(fyprt_context* c, const char* who, unsigned needs) {
    auto refuse = [&](const char* why) { return c->fail(FYPRT_ESTATE, std::string(who) + why); };
    if ((needs & kNeedScene) && !c->haveScene) return refuse(" before fyprt_upload_scene");
    if ((needs & kNeedSceneAndRanges) && (!c->haveScene || c->meshFirstVertex.empty())) return refuse(" before fyprt_upload_scene + fyprt_set_object_vertices");
    if ((needs & kNeedRanges) && c->meshFirstVertex.empty()) return refuse(" needs the mesh vertex ranges of fyprt_set_object_vertices");
    if ((needs & kNeedOwnLightTrees) && c->prebuiltLightTrees) return refuse(": the scene was uploaded with prebuilt light trees; upload it again instead");
    if ((needs & kNeedDevice) && c->hostOnly) return refuse(" needs a device (host-only context)");
    return FYPRT_OK;
}
// An edit begins, every check passed: all streams idle, and what the edit means to the last frame and to the temporal denoiser's history.
// kEditGeometry: the history stays under motion (temporal_edit_begin); kEditShading: it goes; kEditTopology: it goes with the snapshot;
// kEditTreeOnly: neither the frame nor the history is touched (the tree moves, what it holds does not).
enum EditKind { kEditGeometry, kEditShading, kEditTopology, kEditTreeOnly };
static int edit_begin(fyprt_context* c, EditKind kind) {
    if (!c->hostOnly) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c)); }
    if (kind == kEditTreeOnly) return FYPRT_OK;         // (a call that changes the tree re-points the descriptor: set_scene_tree drops the kept primary hits)
    c->frameComplete = false;                  // the payload's triangles, texture coordinates and materials are the old scene's (fyprt_denoise)
    if (kind != kEditShading) c->drop_kept_primary();   // ... but the hits themselves outlive a shading edit: no material in a Payload (fyprt_context::KeptPrimary)
    if (kind == kEditGeometry) return temporal_edit_begin(c);
    c->drop_history(); if (kind == kEditTopology) c->release_snapshot();
    return FYPRT_OK;
}
// A list of `n` mesh indices: every index in range, and (`distinct` == NULL) no mesh listed twice.  `listed`: NULL or a mark per mesh
// of the scene; `distinct`: NULL or the listed meshes once each, in the order of their first entry.
static int check_mesh_list(fyprt_context* c, const char* who, const uint32_t* indices, uint32_t n, std::vector<uint8_t>* listed, std::vector<uint32_t>* distinct = nullptr) {
    const uint32_t nM = (uint32_t)c->topoMeshes.size();
    for (uint32_t k = 0; k < n; ++k) if (indices[k] >= nM) return c->fail(FYPRT_EINVAL, std::string(who) + ": mesh index out of range");
    if (!listed) return FYPRT_OK;
    listed->assign(nM, 0);
    for (uint32_t k = 0; k < n; ++k) {
        uint8_t& mark = (*listed)[indices[k]];
        if (mark && !distinct) return c->fail(FYPRT_EINVAL, std::string(who) + ": mesh " + std::to_string(indices[k]) + " is listed twice");
        if (!mark && distinct) distinct->push_back(indices[k]);
        mark = 1;
    }
    return FYPRT_OK;
}
// The tail of a geometry edit whose records and tree are enqueued: the light trees of the emissive meshes that moved (`touched`, a mark
// per mesh; NULL: all of them) from the host's vertices — `waitForReadback`: which the context stream is still bringing back —, the light
// records, and the edit complete on return.
static int finish_geometry_edit(fyprt_context* c, const uint8_t* touched, bool lightsMoved, bool waitForReadback) {
    c->hostBvhStale = true;
    if (lightsMoved && waitForReadback) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (lightsMoved) TRY(rebuild_light_trees(c, c->hostVerts.data(), touched));
    TRY(launch_light_records(c));
    HIPCHK(c, sync_all(c));
    partial_finish_stats(c);
    return FYPRT_OK;
}

// Scene geometry moved, topology unchanged (SceneManager::PerformAllSceneUpdates with a transform edit, SceneManager.cpp:24-66):
// new world vertices -> per-triangle records, leaf triangles and the tree's boxes are refreshed ON THE DEVICE (rt_refit.h),
// the per-light records are rebuilt by their kernel, the (small) light trees on the host.  The tree keeps its shape.
int fyprt_update_vertices(fyprt_context* c, const fyprt_vertex* vertices, uint32_t vertex_count) {
    if (!c || !vertices) return FYPRT_EINVAL;
    TRY(edit_check_state(c, "fyprt_update_vertices", kNeedScene));
    if (vertex_count != c->vertexCount) return c->fail(FYPRT_EINVAL, "fyprt_update_vertices: vertex count differs from the uploaded scene");
    TRY(edit_check_state(c, "fyprt_update_vertices", kNeedDevice));
    TRY(edit_check_state(c, "fyprt_update_vertices", kNeedOwnLightTrees));
    TRY(edit_begin(c, kEditGeometry));
    const uint32_t nT = (uint32_t)(c->topoTris.size() / 4);
    temporal_edit_range(c, 0, nT);
    // the upload below is a blocking copy, which the non-blocking context stream does not order: the snapshot must have read dverts first
    if (c->dtSnapPending) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (upload(c, c->dverts.p, vertices, c->dverts.bytes())) return FYPRT_EHIP;
    c->hostVerts.assign(vertices, vertices + vertex_count); c->hostVertsStale = false;
    TRY(launch_refresh_triangles(c, 0, nT));
    TRY(run_refit(c));
    full_edit_stats(c);
    c->hostBvhStale = true;
    TRY(rebuild_light_trees(c, vertices));                      // every light tree, from the caller's array
    TRY(launch_light_records(c));
    HIPCHK(c, sync_all(c));
    return FYPRT_OK;
}

// Object-space vertices (Scene::vertices) and the meshes' vertex ranges, kept on the device so that a transform edit can be applied there.
int fyprt_set_object_vertices(fyprt_context* c, const fyprt_vertex* object_vertices, uint32_t vertex_count, const uint32_t* mesh_first_vertex) {
    if (!c || !object_vertices || !mesh_first_vertex) return FYPRT_EINVAL;
    TRY(edit_check_state(c, "fyprt_set_object_vertices", kNeedScene | kNeedDevice));
    if (vertex_count != c->vertexCount) return c->fail(FYPRT_EINVAL, "fyprt_set_object_vertices: vertex count differs from the uploaded scene");
    const uint32_t nM = (uint32_t)c->topoMeshes.size();
    for (uint32_t m = 0; m < nM; ++m) if (mesh_first_vertex[m] > mesh_first_vertex[m + 1] || mesh_first_vertex[m + 1] > vertex_count) return c->fail(FYPRT_EINVAL, "fyprt_set_object_vertices: mesh vertex ranges out of order / out of range");
    // every triangle of a mesh must index into that mesh's vertex range (the transform of one mesh must not move another mesh's triangles)
    for (uint32_t m = 0; m < nM; ++m)
        for (uint32_t t = c->topoMeshes[m].first_triangle; t < c->topoMeshes[m].first_triangle + c->topoMeshes[m].triangle_count; ++t)
            for (int k = 0; k < 3; ++k) { const uint32_t v = c->topoTris[(size_t)t * 4 + k]; if (v < mesh_first_vertex[m] || v >= mesh_first_vertex[m + 1]) return c->fail(FYPRT_EINVAL, "fyprt_set_object_vertices: triangle " + std::to_string(t) + " uses a vertex outside its mesh's range"); }
    HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c));
    c->drop_kept_primary();                    // the vertices the next transform edit starts from
    TRY(alloc_upload(c, c->objVerts, object_vertices, vertex_count));
    c->meshFirstVertex.assign(mesh_first_vertex, mesh_first_vertex + nM + 1);
    return FYPRT_OK;
}

// A transform edit of `count` meshes (SceneManager::PerformAllSceneUpdates with meshTransformToBeUpdated, SceneManager.cpp:24-66): 64
// bytes per mesh cross the bus; the world vertices are recomputed on the device (k_transform_vertices), per-triangle records, leaf
// triangles, tree boxes and light records refreshed there, and only the moved EMISSIVE meshes' light trees are rebuilt on the host
// (their vertices read back) + the small TLAS.  Same result as fyprt_update_vertices with host-computed world vertices.
// Tuning key 22 = 1: records and tree by the partial walk over the listed meshes (rt_partial.h) instead of the full passes.
int fyprt_update_transforms(fyprt_context* c, const uint32_t* mesh_indices, const float* matrices16, uint32_t count) {
    if (!c || (count && (!mesh_indices || !matrices16))) return FYPRT_EINVAL;
    TRY(edit_check_state(c, "fyprt_update_transforms", kNeedSceneAndRanges | kNeedOwnLightTrees));
    TRY(check_mesh_list(c, "fyprt_update_transforms", mesh_indices, count, nullptr));
    TRY(edit_begin(c, kEditGeometry));
    for (uint32_t k = 0; k < count; ++k) temporal_edit_range(c, c->topoMeshes[mesh_indices[k]].first_triangle, c->topoMeshes[mesh_indices[k]].triangle_count);
    std::vector<uint8_t> touched(c->topoMeshes.size(), 0);
    bool lightsMoved = false;
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t m = mesh_indices[k], first = c->meshFirstVertex[m], n = c->meshFirstVertex[m + 1] - first;
        Mat4 M; std::memcpy(M.m, matrices16 + (size_t)k * 16, 64);
        if (n) hipLaunchKernelGGL(k_transform_vertices, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, c->objVerts.p, c->dverts.p, first, n, M);
        if (is_emissive(c->topoMats[c->topoMeshes[m].material_index]) && n) {            // an emissive mesh moved: its light tree is rebuilt from its new vertices
            TRY(read_back_mesh_verts(c, m));
            touched[m] = 1; lightsMoved = true;
        }
    }
    HIPCHK(c, hipGetLastError());
    if (c->tuning[K_PARTIAL_REFIT]) {
        std::vector<uint8_t> listed; std::vector<uint32_t> distinct;              // a mesh may be listed twice: its last matrix holds, it is walked once
        TRY(check_mesh_list(c, "fyprt_update_transforms", mesh_indices, count, &listed, &distinct));
        TRY(run_partial_refit(c, distinct));
    } else {
        TRY(launch_refresh_triangles(c, 0, (uint32_t)(c->topoTris.size() / 4)));
        TRY(run_refit(c));
        full_edit_stats(c);
    }
    c->hostVertsStale = true;
    return finish_geometry_edit(c, touched.data(), lightsMoved, true);
}

// New world vertices for the listed meshes only: the state fyprt_update_vertices reaches with the full array (the given vertices in
// place, every other vertex as it is on the device), by the partial walk.  Only the listed ranges cross the bus.
int fyprt_update_mesh_vertices(fyprt_context* c, const uint32_t* mesh_indices, uint32_t mesh_count, const fyprt_vertex* vertices, uint32_t vertex_count) {
    if (!c) return FYPRT_EINVAL;
    if ((mesh_count && !mesh_indices) || (vertex_count && !vertices)) return c->fail(FYPRT_EINVAL, "fyprt_update_mesh_vertices: NULL array with a non-zero count");
    TRY(edit_check_state(c, "fyprt_update_mesh_vertices", kNeedScene | kNeedRanges | kNeedOwnLightTrees | kNeedDevice));
    std::vector<uint8_t> listed;
    TRY(check_mesh_list(c, "fyprt_update_mesh_vertices", mesh_indices, mesh_count, &listed));
    uint64_t sum = 0;
    for (uint32_t k = 0; k < mesh_count; ++k) sum += c->meshFirstVertex[mesh_indices[k] + 1] - c->meshFirstVertex[mesh_indices[k]];
    if (sum != vertex_count) return c->fail(FYPRT_EINVAL, "fyprt_update_mesh_vertices: vertex_count is not the sum of the listed meshes' vertex ranges");
    if (mesh_count == 0) return FYPRT_OK;
    TRY(edit_begin(c, kEditGeometry));
    for (uint32_t k = 0; k < mesh_count; ++k) temporal_edit_range(c, c->topoMeshes[mesh_indices[k]].first_triangle, c->topoMeshes[mesh_indices[k]].triangle_count);
    if (c->dtSnapPending) HIPCHK(c, hipStreamSynchronize(c->stream));          // blocking copies below: the snapshot must have read dverts first
    std::vector<uint8_t> touched(c->topoMeshes.size(), 0);
    bool lightsMoved = false;
    const fyprt_vertex* src = vertices;
    for (uint32_t k = 0; k < mesh_count; ++k) {
        const uint32_t m = mesh_indices[k], first = c->meshFirstVertex[m], n = c->meshFirstVertex[m + 1] - first;
        TRY(upload(c, c->dverts.p + first, src, (size_t)n * sizeof(fyprt_vertex)));
        if (n) std::memcpy(c->hostVerts.data() + first, src, (size_t)n * sizeof(fyprt_vertex));
        if (n && is_emissive(c->topoMats[c->topoMeshes[m].material_index])) { touched[m] = 1; lightsMoved = true; }
        src += n;
    }
    TRY(run_partial_refit(c, std::vector<uint32_t>(mesh_indices, mesh_indices + mesh_count)));
    return finish_geometry_edit(c, touched.data(), lightsMoved, false);
}

int fyprt_last_edit_stats(fyprt_context* c, fyprt_edit_stats* out) {
    if (!c || !out) return FYPRT_EINVAL;
    if (!c->haveEditStats) return c->fail(FYPRT_ESTATE, "fyprt_last_edit_stats before the first geometry edit");
    *out = c->editStats;
    return FYPRT_OK;
}

// The emissive list derived ON THE DEVICE from the per-material flags (rt_materials.h) over the triangles [first, nT): count per
// workgroup, scan, scatter in ascending triangle order.  `keep` = 0: the list is the range's (a material edit: first = 0) and c->emissive
// is sized to the count; otherwise the range's emitters follow the first `keep` entries of the list (an append).  `count`: the range's
// emitters, which come back in one 4-byte read.
static int derive_emissive_on_device(fyprt_context* c, const std::vector<char>& emissiveMat, uint32_t first, uint32_t nT, uint32_t keep, uint32_t* count) {
    const uint32_t nMat = (uint32_t)emissiveMat.size(), n = nT - first;
    *count = 0;
    if (n == 0 || nMat == 0) { if (!keep) c->emissive.release(); return FYPRT_OK; }
    const uint32_t groups = std::min<uint32_t>(kEmMaxGroups, (n + kEmMinChunk - 1u) / kEmMinChunk);
    const uint32_t perGroup = (((n + groups - 1u) / groups + kBlock - 1u) / kBlock) * kBlock;     // whole tiles, groups * perGroup >= n
    std::vector<uint32_t> flags(emissiveMat.begin(), emissiveMat.end());
    if (c->matFlags.n < nMat) HIPCHK(c, c->matFlags.alloc(nMat));
    if (c->emCounts.n < 2u * kEmMaxGroups + 1u) HIPCHK(c, c->emCounts.alloc(2u * kEmMaxGroups + 1u));
    TRY(upload(c, c->matFlags.p, flags.data(), (size_t)nMat * 4));
    uint32_t* counts = c->emCounts.p; uint32_t* offsets = c->emCounts.p + kEmMaxGroups;
    hipLaunchKernelGGL(k_emissive_count, dim3(groups), dim3(kBlock), 0, c->stream, c->triIdx.p, c->matFlags.p, nMat, first, nT, perGroup, counts);
    hipLaunchKernelGGL(k_emissive_scan, dim3(1), dim3(kBlock), 0, c->stream, counts, groups, offsets);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(count, offsets + groups, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (keep) TRY(grow_buffer(c, c->emissive, (size_t)keep + *count)); else HIPCHK(c, c->emissive.alloc(*count));
    if (*count) {
        hipLaunchKernelGGL(k_emissive_scatter, dim3(groups), dim3(kBlock), 0, c->stream, c->triIdx.p, c->matFlags.p, nMat, first, nT, perGroup, offsets, c->emissive.p + keep, *count);
        HIPCHK(c, hipGetLastError());
    }
    return FYPRT_OK;
}

// What a material edit means, worked out before anything changes: the packed table and which materials emit; the reassignment as (first
// triangle, count, material, mesh); does emission move, does the list stay; the meshes whose light tree changes, and does the set of lights
struct MaterialEdit {
    std::vector<float> mats; std::vector<char> emissiveMat; std::vector<uint4> ranges; std::vector<uint8_t> touched;
    bool emissionMoved = false, listSame = false, setChanged = false, anyTouched = false;
};
static MaterialEdit plan_material_edit(const fyprt_context* c, const fyprt_material* materials, uint32_t material_count, const uint32_t* mesh_indices, const int32_t* mesh_materials,
                                       uint32_t mesh_count, const uint32_t* emissive_triangles, uint32_t emissive_count) {
    MaterialEdit e;
    const uint32_t nM = (uint32_t)c->topoMeshes.size(), oldCount = (uint32_t)c->topoMats.size();
    pack_materials(materials, material_count, e.mats, e.emissiveMat);
    // Does the edit move any emission?  A material whose emission colour or power changed bit-wise, or a reassigned mesh that has
    // anything to do with an emitter (its old or new material, or the old material of any of its triangles).
    for (uint32_t i = 0; i < oldCount && !e.emissionMoved; ++i)
        e.emissionMoved = std::memcmp(materials[i].emission_color, c->topoMats[i].emission_color, 12) != 0 || std::memcmp(&materials[i].emission_power, &c->topoMats[i].emission_power, 4) != 0;
    // the reassignment, de-duplicated (the last entry of a mesh wins, as a sequence of edits would have it)
    if (mesh_count) {
        std::vector<int32_t> newMat(nM, -1);
        for (uint32_t k = 0; k < mesh_count; ++k) newMat[mesh_indices[k]] = mesh_materials[k];
        for (uint32_t k = 0; k < mesh_count; ++k) {
            const uint32_t m = mesh_indices[k];
            if (newMat[m] < 0) continue;                                     // an earlier entry of this mesh has been taken
            const fyprt_mesh& me = c->topoMeshes[m];
            e.ranges.push_back(make_uint4(me.first_triangle, me.triangle_count, (uint32_t)newMat[m], m));
            newMat[m] = -1;
        }
    }
    // light trees hang on the MESH's material (lighttree_build.cpp): which meshes change their tree, and does any mesh start or stop
    // being a light (then the node counts move and every tree is rebuilt)
    e.touched.assign(nM, 0); std::vector<uint8_t> reassigned(nM, 0);
    auto emissionBits = [](const fyprt_material& a, const fyprt_material& b) {
        return std::memcmp(a.emission_color, b.emission_color, 12) == 0 && std::memcmp(&a.emission_power, &b.emission_power, 4) == 0;
    };
    for (const uint4& r : e.ranges) {
        const fyprt_mesh& me = c->topoMeshes[r.w];
        const fyprt_material& was = c->topoMats[me.material_index]; const fyprt_material& is = materials[r.z];
        reassigned[r.w] = 1;
        bool emits = is_emissive(was) || e.emissiveMat[r.z];
        for (uint32_t t = me.first_triangle; t < me.first_triangle + me.triangle_count && !emits; ++t) emits = is_emissive(c->topoMats[c->topoTris[(size_t)t * 4 + 3]]);
        if (emits) e.emissionMoved = true;
        if (me.triangle_count && is_emissive(was) != (bool)e.emissiveMat[r.z]) e.setChanged = true;
        else if (e.emissiveMat[r.z] && !emissionBits(was, is)) { e.touched[r.w] = 1; e.anyTouched = true; }
    }
    // the emissive list stays as it is when it is derived as before and no emission moved, or handed over unchanged
    e.listSame = !e.emissionMoved;
    if (e.listSame) {
        if (emissive_triangles) e.listSame = c->emissiveExplicit && c->hostEmissive.size() == emissive_count && (emissive_count == 0 || std::memcmp(c->hostEmissive.data(), emissive_triangles, (size_t)emissive_count * 4) == 0);
        else e.listSame = !c->emissiveExplicit;
    }
    if (!e.listSame || e.emissionMoved) {
        for (uint32_t m = 0; m < nM; ++m) {
            if (reassigned[m] || c->topoMeshes[m].triangle_count == 0) continue;
            const uint32_t mi = (uint32_t)c->topoMeshes[m].material_index;             // < oldCount
            if (is_emissive(c->topoMats[mi]) != (bool)e.emissiveMat[mi]) e.setChanged = true;
            else if (e.emissiveMat[mi] && !emissionBits(c->topoMats[mi], materials[mi])) { e.touched[m] = 1; e.anyTouched = true; }
        }
    }
    return e;
}
// the reassigned ranges' triangles on the device (k_set_mesh_material: blockIdx.y = the range); the table is scratch the context keeps
static int launch_set_mesh_materials(fyprt_context* c, const std::vector<uint4>& ranges) {
    if (c->hostOnly || ranges.empty()) return FYPRT_OK;
    if (c->matRanges.n < ranges.size()) HIPCHK(c, c->matRanges.alloc(ranges.size()));
    TRY(upload(c, c->matRanges.p, ranges.data(), ranges.size() * sizeof(uint4)));
    for (size_t first = 0; first < ranges.size(); first += 65535u) {
        const uint32_t n = (uint32_t)std::min<size_t>(65535u, ranges.size() - first);
        uint32_t longest = 0; for (uint32_t k = 0; k < n; ++k) longest = std::max(longest, ranges[first + k].y);
        if (longest == 0) continue;
        const uint32_t gx = std::min<uint32_t>(64u, (longest + kBlock - 1u) / kBlock);
        hipLaunchKernelGGL(k_set_mesh_material, dim3(gx, n), dim3(kBlock), 0, c->stream, c->matRanges.p + first, c->triPos.p, c->triShade.p, c->triIdx.p, (uint32_t)(c->topoTris.size() / 4));
    }
    HIPCHK(c, hipGetLastError());
    return FYPRT_OK;
}

// A material edit (SceneManager::PerformAllSceneUpdates with materialsToUpdate / meshMatToBeUpdated, SceneManager.cpp:10-17, :69-85): the
// whole material table is replaced, the listed meshes (and all their triangles) get another material, the emissive list is the given one
// or derived again.  The context ends in the state fyprt_upload_scene reaches with the edited description — but the acceleration
// structure is not touched, and nothing per triangle crosses the bus: table, reassignment and the ordered compaction of the emissive
// list run on the device (rt_materials.h), the light records by their kernel, the light trees on the host.  An edit that moves no
// emission (albedo, roughness, metallic, texture switch) stops after table and reassignment.
int fyprt_update_materials(fyprt_context* c, const fyprt_material* materials, uint32_t material_count, const uint32_t* mesh_indices,
                           const int32_t* mesh_materials, uint32_t mesh_count, const uint32_t* emissive_triangles, uint32_t emissive_count) {
    if (!c) return FYPRT_EINVAL;
    if (!materials && material_count) return c->fail(FYPRT_EINVAL, "fyprt_update_materials: NULL materials with a non-zero count");
    if (mesh_count && (!mesh_indices || !mesh_materials)) return c->fail(FYPRT_EINVAL, "fyprt_update_materials: NULL mesh array with a non-zero count");
    const uint32_t nM = (uint32_t)c->topoMeshes.size(), nT = (uint32_t)(c->topoTris.size() / 4), oldCount = (uint32_t)c->topoMats.size();
    if (material_count < oldCount) return c->fail(FYPRT_EINVAL, "fyprt_update_materials: the material table must not shrink");
    TRY(check_mesh_list(c, "fyprt_update_materials", mesh_indices, mesh_count, nullptr));
    for (uint32_t k = 0; k < mesh_count; ++k) if (mesh_materials[k] < 0 || (uint32_t)mesh_materials[k] >= material_count) return c->fail(FYPRT_EINVAL, "fyprt_update_materials: material index out of range");
    if (emissive_triangles) for (uint32_t k = 0; k < emissive_count; ++k) if (emissive_triangles[k] >= nT) return c->fail(FYPRT_EINVAL, "fyprt_update_materials: emissive triangle index out of range");
    TRY(edit_check_state(c, "fyprt_update_materials", kNeedScene | kNeedOwnLightTrees));
    TRY(edit_begin(c, kEditShading));

    const MaterialEdit e = plan_material_edit(c, materials, material_count, mesh_indices, mesh_materials, mesh_count, emissive_triangles, emissive_count);
    // 1. the table
    if (material_count != oldCount) { HIPCHK(c, c->mats.alloc((size_t)material_count * 3, c->hostOnly)); c->dsc.mats = c->mats.p; }
    TRY(upload(c, c->mats.p, e.mats.data(), e.mats.size() * 4));
    c->topoMats.assign(materials, materials + material_count);
    // 2. the reassigned meshes: the host's copy of their ranges, their triangles on the device
    for (const uint4& r : e.ranges) {
        c->topoMeshes[r.w].material_index = (int32_t)r.z;
        for (uint32_t t = r.x; t < r.x + r.y; ++t) c->topoTris[(size_t)t * 4 + 3] = r.z;
    }
    TRY(launch_set_mesh_materials(c, e.ranges));
    if (e.listSame && !e.emissionMoved) {       // albedo, roughness, metallic, texture switch: no light changes
        if (!c->hostOnly) HIPCHK(c, sync_all(c));
        return FYPRT_OK;
    }
    // 3. the emissive list: handed over, or derived again from the materials that emit now
    uint32_t nE = 0;
    c->hostEmissive.clear();
    if (emissive_triangles) {
        c->hostEmissive.assign(emissive_triangles, emissive_triangles + emissive_count);
        TRY(alloc_upload(c, c->emissive, c->hostEmissive.data(), c->hostEmissive.size()));
        nE = emissive_count;
    } else if (c->hostOnly) {
        for (uint32_t i = 0; i < nT; ++i) if (e.emissiveMat[c->topoTris[(size_t)i * 4 + 3]]) c->hostEmissive.push_back(i);
        nE = (uint32_t)c->hostEmissive.size();
        HIPCHK(c, c->emissive.alloc(nE, true));
    } else TRY(derive_emissive_on_device(c, e.emissiveMat, 0, nT, 0, &nE));
    c->emissiveExplicit = emissive_triangles != nullptr;
    c->dsc.emissive = c->emissive.p; c->dsc.emissiveCount = nE;
    // 4. the light records (they carry the emission)
    HIPCHK(c, c->lightRecs.alloc((size_t)nE * 3, c->hostOnly));
    c->dsc.lightRecs = c->lightRecs.p;
    TRY(launch_light_records(c));
    // 5. the light trees, on the host.  The partial rebuild replaces a mesh's tree in place, which needs every mesh to keep its node
    // count: only when no mesh starts or stops being a light.  After device transform edits the host's vertices followed only the
    // meshes that were lights when they moved: what the build will read (the meshes that are lights NOW) comes back first.
    if (e.setChanged || e.anyTouched) {
        if (e.setChanged && c->hostVertsStale && !c->hostOnly && !c->meshFirstVertex.empty()) {
            for (uint32_t m = 0; m < nM; ++m) if (is_emissive(c->topoMats[c->topoMeshes[m].material_index])) TRY(read_back_mesh_verts(c, m));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        TRY(rebuild_light_trees(c, c->hostVerts.data(), e.setChanged ? nullptr : e.touched.data()));
    }
    if (!c->hostOnly) HIPCHK(c, sync_all(c));
    return FYPRT_OK;
}

// "Import Mesh" (WalnutApp.cpp:668-693 -> Scene::CreateNewMeshInScene, Scene.cpp:241-290, on Scene::AddNewMeshToScene, Scene.cpp:9-92):
// vertices, triangles and meshes are appended, nothing that exists moves.  The context ends in the state fyprt_upload_scene reaches
// with the combined description, except for the acceleration structure, which takes a sub-tree over the new triangles at its root
// (rt_graft.h).  Of the old scene nothing crosses the bus but the level grouping (4 bytes per node): the scene arrays grow in place
// or move device to device, the appended range goes through k_refresh_triangles, the emissive list is extended by the ordered
// compaction over the range, the light records are rebuilt by their kernel, and the host builds the new meshes' light trees + the TLAS.
int fyprt_append_meshes(fyprt_context* c, const fyprt_vertex* vertices, uint32_t vertex_count, const void* triangles, uint32_t triangle_count, uint32_t triangle_stride,
                        const fyprt_mesh* meshes, uint32_t mesh_count, const fyprt_vertex* object_vertices, const uint32_t* mesh_first_vertex) {
    if (!c) return FYPRT_EINVAL;
    if ((vertex_count && !vertices) || (triangle_count && !triangles) || (mesh_count && !meshes) || (object_vertices && !mesh_first_vertex))
        return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: NULL array with non-zero count");
    if (triangle_count && triangle_stride < 16) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: triangle stride below 16");
    const uint32_t V0 = c->vertexCount, T0 = (uint32_t)(c->topoTris.size() / 4), M0 = (uint32_t)c->topoMeshes.size(), nMat = (uint32_t)c->topoMats.size();
    const uint64_t V64 = (uint64_t)V0 + vertex_count, T64 = (uint64_t)T0 + triangle_count;
    if (V64 > 0xFFFFFFFFull || T64 > 0x3FFFFFFFull) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: too many vertices / triangles");
    const uint32_t V = (uint32_t)V64, T = (uint32_t)T64, M = M0 + mesh_count;
    const uint8_t* tb = (const uint8_t*)triangles;
    auto tri = [&](uint32_t i) { return reinterpret_cast<const uint32_t*>(tb + (size_t)i * triangle_stride); };
    for (uint32_t i = 0; i < triangle_count; ++i)
        if (tri(i)[0] >= V || tri(i)[1] >= V || tri(i)[2] >= V) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: triangle " + std::to_string(i) + " references a vertex out of range");
    for (uint32_t i = 0; i < triangle_count; ++i)
        if ((int32_t)tri(i)[3] < 0 || tri(i)[3] >= nMat) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: triangle " + std::to_string(i) + " references a material outside the table");
    for (uint32_t m = 0; m < mesh_count; ++m)
        if (meshes[m].material_index < 0 || (uint32_t)meshes[m].material_index >= nMat) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: mesh " + std::to_string(m) + " references a material outside the table");
    {
        uint64_t next = T0;
        for (uint32_t m = 0; m < mesh_count; ++m) {
            if (meshes[m].first_triangle != next) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: the meshes must partition the appended triangle range in order");
            next += meshes[m].triangle_count;
        }
        if (next != T64) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: the meshes must partition the appended triangle range in order");
    }
    if (object_vertices) {
        if (mesh_first_vertex[0] != V0 || mesh_first_vertex[mesh_count] != V) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: mesh vertex ranges must span the appended vertices");
        for (uint32_t m = 0; m < mesh_count; ++m) if (mesh_first_vertex[m] > mesh_first_vertex[m + 1]) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: mesh vertex ranges out of order");
        for (uint32_t m = 0; m < mesh_count; ++m)
            for (uint32_t t = meshes[m].first_triangle - T0; t < meshes[m].first_triangle - T0 + meshes[m].triangle_count; ++t)
                for (int k = 0; k < 3; ++k) if (tri(t)[k] < mesh_first_vertex[m] || tri(t)[k] >= mesh_first_vertex[m + 1]) return c->fail(FYPRT_EINVAL, "fyprt_append_meshes: triangle " + std::to_string(t) + " uses a vertex outside its mesh's range");
    }
    TRY(edit_check_state(c, "fyprt_append_meshes", kNeedScene | kNeedOwnLightTrees));
    if (triangle_count == 0 && mesh_count == 0) return FYPRT_OK;
    TRY(edit_begin(c, kEditTopology));

    // 1. the host's copies: vertices, topology.  The sub-tree's host builder and the new meshes' light trees read the vertices the new
    // triangles use: after device transform edits the old ones come back first if any is among them.
    bool usesOld = false;
    for (uint32_t i = 0; i < triangle_count && !usesOld; ++i) usesOld = tri(i)[0] < V0 || tri(i)[1] < V0 || tri(i)[2] < V0;
    if (usesOld) TRY(ensure_host_verts(c, V0));
    c->hostVerts.insert(c->hostVerts.end(), vertices, vertices + vertex_count);
    c->topoTris.resize((size_t)T * 4);
    for (uint32_t i = 0; i < triangle_count; ++i) std::memcpy(&c->topoTris[(size_t)(T0 + i) * 4], tri(i), 16);
    c->topoMeshes.insert(c->topoMeshes.end(), meshes, meshes + mesh_count);
    if (!c->meshMasks.empty()) { c->meshMasks.resize(M, 0xFFFFFFFFu); c->filterValid = false; }      // a new mesh is in every group (query filter)
    c->vertexCount = V; c->meshCount = M;
    // 2. the device's: vertices and triangle indices cross the bus, the per-triangle records are computed there
    static_assert(sizeof(DevVertex) == sizeof(fyprt_vertex), "vertex layout");
    TRY(grow_buffer(c, c->dverts, V)); TRY(grow_buffer(c, c->triIdx, T)); TRY(grow_buffer(c, c->triPos, (size_t)T * 3)); TRY(grow_buffer(c, c->triShade, (size_t)T * 4));
    if (!c->hostOnly) {
        TRY(upload(c, c->dverts.p + V0, vertices, (size_t)vertex_count * sizeof(fyprt_vertex)));
        TRY(upload(c, c->triIdx.p + T0, c->topoTris.data() + (size_t)T0 * 4, (size_t)triangle_count * 16));
        TRY(launch_refresh_triangles(c, T0, triangle_count));
    }
    // 3. object-space vertices: extended with the copy the context holds; without new ones the copy goes, as an upload drops it
    if (object_vertices && !c->meshFirstVertex.empty()) {
        TRY(grow_buffer(c, c->objVerts, V));
        TRY(upload(c, c->objVerts.p + V0, object_vertices, (size_t)vertex_count * sizeof(fyprt_vertex)));
        c->meshFirstVertex.insert(c->meshFirstVertex.end(), mesh_first_vertex + 1, mesh_first_vertex + mesh_count + 1);
    } else if (!object_vertices) { c->objVerts.release(); c->meshFirstVertex.clear(); }
    // 4. the acceleration structure: the graft, or the tree of the combined scene when the graft would be too deep / too large
    if (triangle_count) {
        TRY(graft_or_rebuild(c, "fyprt_append_meshes", vertices, vertex_count, T0, triangle_count, meshes, mesh_count, V0));
        c->havePlacement = true;
    }
    set_scene_triangles(c, T);
    DevScene& d = c->dsc;
    // 5. lights.  The emissive list: the old one followed by the appended triangles whose material emits, in ascending order
    std::vector<char> emissiveMat(nMat);
    for (uint32_t i = 0; i < nMat; ++i) emissiveMat[i] = is_emissive(c->topoMats[i]);
    std::vector<uint32_t> tail;
    for (uint32_t i = 0; i < triangle_count; ++i) if (emissiveMat[tri(i)[3]]) tail.push_back(T0 + i);
    const uint32_t nE0 = c->hostOnly ? (uint32_t)c->hostEmissive.size() : d.emissiveCount;
    if (c->hostEmissive.size() == nE0) c->hostEmissive.insert(c->hostEmissive.end(), tail.begin(), tail.end());   // (a device context keeps the copy of a list it was handed only)
    if (!tail.empty()) {
        const uint32_t nE = nE0 + (uint32_t)tail.size();
        if (c->hostOnly) HIPCHK(c, c->emissive.alloc(nE, true));
        else {
            uint32_t found = 0;
            TRY(derive_emissive_on_device(c, emissiveMat, T0, T, nE0, &found));
            if (found != tail.size()) return c->fail(FYPRT_EHIP, "fyprt_append_meshes: the device's emissive list disagrees with the host's");
        }
        d.emissive = c->emissive.p; d.emissiveCount = nE;
        HIPCHK(c, c->lightRecs.alloc((size_t)nE * 3, c->hostOnly));
        d.lightRecs = c->lightRecs.p;
        TRY(launch_light_records(c));
    }
    // ... and the light trees, which hang on the MESH's material: the new meshes' trees behind the old ones, then the TLAS
    {
        rth::LightTrees& lt = c->hostLt;
        std::vector<uint8_t> touched(M, 0);
        bool newLight = false;
        for (uint32_t m = M0; m < M; ++m) {
            const fyprt_mesh& me = c->topoMeshes[m];
            lt.first.push_back((uint32_t)lt.blas.size()); lt.count.push_back(0u); lt.root.push_back(~0u);
            if (!emissiveMat[me.material_index] || me.triangle_count == 0) continue;
            lt.blas.resize(lt.blas.size() + 2u * (size_t)me.triangle_count - 1u);         // a mesh's tree has 2n - 1 nodes
            touched[m] = 1; newLight = true;
        }
        if (newLight) TRY(rebuild_light_trees(c, c->hostVerts.data(), touched.data()));
        else if (!tail.empty()) TRY(upload_light_trees(c, T, M));                          // the emitter -> TLAS-leaf table covers the new triangles
        else TRY(extend_light_tables(c, T, M));                                            // no emitter came: the tables grow on the device
    }
    if (!c->hostOnly) HIPCHK(c, sync_all(c));
    return FYPRT_OK;
}

int fyprt_set_append_placement(fyprt_context* c, int mode) {
    if (!c) return FYPRT_EINVAL;
    if (mode != 0 && mode != 1) return c->fail(FYPRT_EINVAL, "fyprt_set_append_placement: mode must be 0 or 1");
    c->appendPlacement = mode;
    return FYPRT_OK;
}

int fyprt_last_append_placement(fyprt_context* c, fyprt_append_placement* out) {
    if (!c || !out) return FYPRT_EINVAL;
    if (!c->havePlacement) return c->fail(FYPRT_ESTATE, "fyprt_last_append_placement before the first append with triangles");
    *out = c->placement;
    return FYPRT_OK;
}

// Mesh removal (new, no reference counterpart): the listed meshes, their triangle ranges and the given vertex ranges leave the scene.  The
// context ends in the state fyprt_upload_scene reaches with the reduced description, except for the acceleration structure, which is the
// old tree pruned bottom-up (rt_prune.h).  Every array is compacted on the device into a buffer of the same capacity; 4 bytes per leaf
// record come back (the dead counts the host repeats the node pass with), tables, refit list and level grouping go up.
int fyprt_remove_meshes(fyprt_context* c, const uint32_t* mesh_indices, uint32_t mesh_count, const uint32_t* vertex_ranges) {
    if (!c) return FYPRT_EINVAL;
    if (mesh_count && !mesh_indices) return c->fail(FYPRT_EINVAL, "fyprt_remove_meshes: NULL mesh_indices with a non-zero count");
    const uint32_t T0 = (uint32_t)(c->topoTris.size() / 4), V0 = c->vertexCount;
    std::vector<uint8_t> gone;
    TRY(check_mesh_list(c, "fyprt_remove_meshes", mesh_indices, mesh_count, &gone));
    const bool copy = !c->meshFirstVertex.empty();
    std::vector<std::pair<uint32_t, uint32_t>> vr, tr;
    if (vertex_ranges) {
        for (uint32_t k = 0; k < mesh_count; ++k) {
            if ((uint64_t)vertex_ranges[2 * k] + vertex_ranges[2 * k + 1] > V0) return c->fail(FYPRT_EINVAL, "fyprt_remove_meshes: vertex range beyond the vertex count");
            if (vertex_ranges[2 * k + 1]) vr.push_back({vertex_ranges[2 * k], vertex_ranges[2 * k + 1]});
        }
        std::sort(vr.begin(), vr.end());
        for (size_t i = 1; i < vr.size(); ++i) if (vr[i - 1].first + vr[i - 1].second > vr[i].first) return c->fail(FYPRT_EINVAL, "fyprt_remove_meshes: vertex ranges overlap");
        if (copy) for (uint32_t k = 0; k < mesh_count; ++k) {
            const uint32_t m = mesh_indices[k];
            if (vertex_ranges[2 * k] != c->meshFirstVertex[m] || vertex_ranges[2 * k + 1] != c->meshFirstVertex[m + 1] - c->meshFirstVertex[m])
                return c->fail(FYPRT_EINVAL, "fyprt_remove_meshes: the vertex range of mesh " + std::to_string(m) + " is not the mesh's own");
        }
    } else if (copy) {
        for (uint32_t k = 0; k < mesh_count; ++k) { const uint32_t m = mesh_indices[k]; vr.push_back({c->meshFirstVertex[m], c->meshFirstVertex[m + 1] - c->meshFirstVertex[m]}); }
    }
    for (uint32_t k = 0; k < mesh_count; ++k) tr.push_back({c->topoMeshes[mesh_indices[k]].first_triangle, c->topoMeshes[mesh_indices[k]].triangle_count});
    PruneTable tris, verts;
    tris.build(tr); verts.build(vr);
    if (verts.removed) for (uint32_t t = 0; t < T0; ++t) {
        uint32_t shift;
        if (tris.dead(t, shift)) continue;
        for (int k = 0; k < 3; ++k) if (verts.dead(c->topoTris[(size_t)t * 4 + k], shift)) return c->fail(FYPRT_EINVAL, "fyprt_remove_meshes: surviving triangle " + std::to_string(t) + " uses a removed vertex");
    }
    TRY(edit_check_state(c, "fyprt_remove_meshes", kNeedScene | kNeedOwnLightTrees));
    if (mesh_count == 0) return FYPRT_OK;
    TRY(edit_begin(c, kEditTopology));
    return prune_remove(c, tris, verts, gone);
}

// Regraft (new, no reference counterpart): the listed meshes' leaf records leave the tree by the prune of a removal, then every listed
// mesh gets the graft of an append over its own triangle range.  Only the tree moves: no scene stream, light or frame state is touched.
// The body, after every check, all streams idle; `reports`: NULL or one entry per listed mesh, preset by the caller.
static int regraft_meshes(fyprt_context* c, const uint32_t* mesh_indices, uint32_t mesh_count, fyprt_append_placement* reports) {
    TRY(ensure_host_verts(c, c->vertexCount));                         // the builders and the placement rule read the meshes' world vertices
    // 1. the prune of a removal on the tree alone: no triangle leaves the scene, so no record is renumbered and no stream moves
    {
        std::vector<std::pair<uint32_t, uint32_t>> tr;
        for (uint32_t k = 0; k < mesh_count; ++k) tr.push_back({c->topoMeshes[mesh_indices[k]].first_triangle, c->topoMeshes[mesh_indices[k]].triangle_count});
        PruneTable tris; tris.build(tr);
        DevBuf<uint2> dTab; DevBuf<uint32_t> counts;                  // scratch of the prune, freed on every way out
        if (!c->hostOnly) { TRY(alloc_upload(c, dTab, tris.tab.data(), tris.tab.size())); HIPCHK(c, counts.alloc(2u * kEmMaxGroups + 1u)); }
        std::vector<uint32_t> refit, refitLevel;
        TRY(prune_tree(c, "fyprt_regraft_meshes", tris, false, dTab.p, counts, refit, refitLevel));
        TRY(prune_refit(c, refit, refitLevel));                       // (with the level grouping the placement search builds its parent links from)
    }
    // 2. one graft per listed mesh, in the order listed, as if the mesh had just been appended
    bool rebuilt = false;
    for (uint32_t k = 0; k < mesh_count; ++k) {
        const fyprt_mesh me = c->topoMeshes[mesh_indices[k]];
        if (!me.triangle_count) continue;
        if (!rebuilt) {
            // the device builders' Morton grid: the exact box of the mesh's triangles, handed over as its two corners
            const rth::HostBox box = tri_range_box(c, me.first_triangle, me.triangle_count);
            fyprt_vertex corner[2] = {};
            for (int a = 0; a < 3; ++a) { corner[0].position[a] = box.lo[a]; corner[1].position[a] = box.hi[a]; }
            TRY(graft_or_rebuild(c, "fyprt_regraft_meshes", corner, 2, me.first_triangle, me.triangle_count, &me, 1, 0u, &rebuilt));
            if (reports) reports[k] = c->placement;
        } else if (reports) {                                         // the rebuilt tree holds this mesh already
            reports[k].kind = 4u; reports[k].levels_before = reports[k].levels_after = c->hostBvh.levels;
        }
    }
    set_scene_tree(c);
    if (!c->hostOnly) HIPCHK(c, sync_all(c));
    return FYPRT_OK;
}

int fyprt_regraft_meshes(fyprt_context* c, const uint32_t* mesh_indices, uint32_t mesh_count, fyprt_append_placement* reports) {
    if (!c) return FYPRT_EINVAL;
    if (mesh_count && !mesh_indices) return c->fail(FYPRT_EINVAL, "fyprt_regraft_meshes: NULL mesh_indices with a non-zero count");
    std::vector<uint8_t> listed;
    TRY(check_mesh_list(c, "fyprt_regraft_meshes", mesh_indices, mesh_count, &listed));
    uint64_t moved = 0;
    for (uint32_t k = 0; k < mesh_count; ++k) moved += c->topoMeshes[mesh_indices[k]].triangle_count;
    TRY(edit_check_state(c, "fyprt_regraft_meshes", kNeedScene));
    if (mesh_count == 0) return FYPRT_OK;
    TRY(edit_begin(c, kEditTreeOnly));
    const fyprt_append_placement blank{(uint32_t)c->appendPlacement, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (reports) for (uint32_t k = 0; k < mesh_count; ++k) reports[k] = blank;
    if (!moved) return FYPRT_OK;
    // what the call leaves as it found it, whichever way it ends: the report of the last append, and the sizes of the kept scratch an append
    // or a placement search allocates (parent links, walk scratch, search result, graft list) — their contents describe the old tree and are
    // rebuilt by whoever needs them next, so only fyprt_live_device_bytes sees the difference
    const fyprt_append_placement saved = c->placement;
    DevBuf<uint32_t>* kept[] = {&c->nodeParent, &c->leafParent, &c->leafOfTri, &c->partialLists, &c->partialDirty, &c->partialCounters, &c->graftList};
    size_t keptSize[7]; for (int i = 0; i < 7; ++i) keptSize[i] = kept[i]->n;
    const size_t placeOutSize = c->placeOut.n;
    c->drop_kept_primary();                    // hits at equal distance go by the tree's order — also of a tree a failed call leaves half moved
    c->filterValid = false;                    // ... and so do the query filter's node and leaf words
    const int rc = regraft_meshes(c, mesh_indices, mesh_count, reports);
    c->placement = saved; c->linksValid = false;
    if (!c->hostOnly) {
        for (int i = 0; i < 7; ++i) if (kept[i]->n != keptSize[i]) HIPCHK(c, kept[i]->alloc(keptSize[i]));
        if (c->placeOut.n != placeOutSize) HIPCHK(c, c->placeOut.alloc(placeOutSize));
    }
    return rc;
}

// The surface-area cost of the tree as it is
int fyprt_tree_cost(fyprt_context* c, fyprt_tree_cost_sums* out) {
    if (!c || !out) return FYPRT_EINVAL;
    TRY(edit_check_state(c, "fyprt_tree_cost", kNeedScene));
    TRY(edit_begin(c, kEditTreeOnly));
    return tree_cost(c, out);
}

// "Import Texture" (WalnutApp.cpp:739-754 -> Scene::CreateNewTextureInScene, Scene.cpp:228-239): the new pixel arrays are uploaded and the
// table is extended; old pixel buffers stay where they are.
int fyprt_append_textures(fyprt_context* c, const fyprt_texture* textures, uint32_t count) {
    if (!c) return FYPRT_EINVAL;
    if (count && !textures) return c->fail(FYPRT_EINVAL, "fyprt_append_textures: NULL textures with a non-zero count");
    for (uint32_t i = 0; i < count; ++i) if (!textures[i].pixels || textures[i].width == 0 || textures[i].height == 0) return c->fail(FYPRT_EINVAL, "fyprt_append_textures: empty texture");
    if (!c->haveScene) return c->fail(FYPRT_ESTATE, "fyprt_append_textures before fyprt_upload_scene");
    if (count == 0) return FYPRT_OK;
    if (!c->hostOnly) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c)); }
    const uint32_t old = (uint32_t)c->texHost.size();
    // a material that already pointed at one of the new slots shaded as solid colour so far: the edit changes its pixels, as a material edit does
    for (const fyprt_material& m : c->topoMats)
        if ((m.is_use_albedo_map & 0xFFu) && m.albedo_map_index >= old && (uint64_t)m.albedo_map_index < (uint64_t)old + count) { c->frameComplete = false; c->drop_history(); }
    for (uint32_t i = 0; i < count; ++i) {
        const fyprt_texture& t = textures[i];
        c->texPixels.emplace_back();
        TRY(alloc_upload(c, c->texPixels.back(), t.pixels, (size_t)t.width * t.height));
        c->texHost.push_back(DevTexture{c->texPixels.back().p, t.width, t.height, 0});
    }
    TRY(alloc_upload(c, c->texTable, c->texHost.data(), c->texHost.size()));
    c->dsc.textures = c->texTable.p; c->dsc.textureCount = (uint32_t)c->texHost.size();
    return FYPRT_OK;
}

// The emissive-triangle list in effect (NULL `triangles` = query the count).
int fyprt_export_emissive(fyprt_context* c, uint32_t* triangles, uint32_t* count) {
    if (!c) return FYPRT_EINVAL;
    if (!c->haveScene) return c->fail(FYPRT_ESTATE, "fyprt_export_emissive before fyprt_upload_scene");
    const uint32_t n = c->hostOnly ? (uint32_t)c->hostEmissive.size() : c->dsc.emissiveCount;
    if (triangles && n) {
        if (c->hostOnly) std::memcpy(triangles, c->hostEmissive.data(), (size_t)n * 4);
        else {                                 // what the frames read
            HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c));
            HIPCHK(c, hipMemcpy(triangles, c->emissive.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
    }
    if (count) *count = n;
    return FYPRT_OK;
}

int fyprt_set_camera(fyprt_context* c, const fyprt_camera_desc* cam) {
    if (!c || !cam) return FYPRT_EINVAL;
    if (cam->viewport_width == 0 || cam->viewport_height == 0) return c->fail(FYPRT_EINVAL, "fyprt_set_camera: empty viewport");
    DevCamera& d = c->dcam;
    std::memcpy(&d.invProj, cam->inverse_projection, 64); std::memcpy(&d.invView, cam->inverse_view, 64);
    float pv[16]; matmul_cm(cam->prev_projection, cam->prev_view, pv);
    std::memcpy(&d.prevProjView, pv, 64);
    matmul_cm(cam->projection, cam->view, c->camPV);           // what a frame rendered with this camera leaves for fyprt_denoise_temporal
    d.position = f3{cam->position[0], cam->position[1], cam->position[2]};
    d.W = cam->viewport_width; d.H = cam->viewport_height;
    c->haveCamera = true;
    return FYPRT_OK;
}

// (Re)sizes the buffers of the wavefront path engine: `entries` live paths at most, `raysPer` rays per path and step,
// `stride` float4s of per-pixel state, `counters` list counters.  Grown on demand, kept between frames.
static int ensure_paths(fyprt_context* c, size_t entries, uint32_t raysPer, uint32_t stride, size_t counters) {
    const size_t npx = (size_t)c->W * c->H;
    if (c->wfRays[0].n < entries * raysPer * 3 || c->wfHits[0].n < entries * raysPer) {
        HIPCHK(c, sync_all(c));
        for (int k = 0; k < 2; ++k) { HIPCHK(c, c->wfRays[k].alloc(entries * raysPer * 3)); HIPCHK(c, c->wfHits[k].alloc(entries * raysPer)); }
    }
    if (c->wfState.n < npx * stride) { HIPCHK(c, sync_all(c)); HIPCHK(c, c->wfState.alloc(npx * stride)); }
    if (c->wfPixels.n < entries) { HIPCHK(c, sync_all(c)); HIPCHK(c, c->wfPixels.alloc(entries)); HIPCHK(c, c->wfPixels2.alloc(entries)); }
    if (c->wfCounters.n < counters) { HIPCHK(c, sync_all(c)); HIPCHK(c, c->wfCounters.alloc(counters)); }
    return FYPRT_OK;
}

extern "C++" {                                                   // (templates inside the C ABI file)
template <class CAM> using shade_kernel_t = void (*)(DevScene, CAM, DevFrame, DevSettings, PathIO);
template <class CAM> static shade_kernel_t<CAM> shade_kernel(int stage) {
    switch (stage) {
        case T_BRUTE: return k_shade<T_BRUTE, CAM>; case T_UNIFORM: return k_shade<T_UNIFORM, CAM>; case T_COSINE: return k_shade<T_COSINE, CAM>;
        case T_GGX: return k_shade<T_GGX, CAM>; case T_BRDF: return k_shade<T_BRDF, CAM>; case T_LIGHT: return k_shade<T_LIGHT, CAM>;
        case T_NEE: return k_shade<T_NEE, CAM>;
    }
    if constexpr (std::is_same<CAM, DevCamera>::value) return stage == T_GI1 ? k_shade<T_GI1> : k_shade<T_GI2>;      // (ReSTIR GI: frames only)
    return nullptr;
}

// One pass of the wavefront path engine over a list of live paths (rt_paths.h): per step one shade launch (NEE: + MIS and emit
// launches) and one trace launch.  Frames (CAM = DevCamera, the context's wf* buffers, counters at rayCounter + 8 x counterPart) and
// radiance queries (CAM = RaySource, the query's own buffers and counters) share it.  `blocking`: the caller synchronises anyway, so
// long sample x bounce products may poll the live-path count and stop early.  `launched` counts the kernel launches.
struct StageRun { int stage; uint32_t steps, raysPer, stride; const uint32_t* pixelList; uint32_t* cnt; uint32_t* heads; uint32_t* part2List; uint32_t* part2Count; int counterPart; uint32_t* misCounts; size_t maxEntries; };
struct StageBufs { float4* rays[2]; float4* hits[2]; float4* state; uint32_t* pixels; uint32_t* pixels2; unsigned long long* rayCounter; };
template <class CAM>
static int run_stage(fyprt_context* c, const StageRun& r, const StageBufs& b, const DevScene& sc, const CAM& cam, const DevFrame& fr, const DevSettings& st,
                     size_t ldsBytes, bool blocking, int* launched) {
    const shade_kernel_t<CAM> shade = shade_kernel<CAM>(r.stage);
    const dim3 block(kBlock);
    const dim3 shadeGrid((uint32_t)(c->numCUs * 8));
    const int occ = c->pathOcc.get(k_trace_rays<false>, ldsBytes, 4), perCU = c->tuning[K_WG_PER_CU] > 0 ? c->tuning[K_WG_PER_CU] : occ;
    // incoherent rays: leave the node loop once few lanes remain in it
    const DevScene tsc = secondary_scene(sc, (uint32_t)c->tuning[K_QUORUM_SECONDARY], b.rayCounter ? b.rayCounter + 8 * r.counterPart : nullptr);
    const bool simple = simple_ray_kernel(c);
    for (uint32_t it = 0; it <= r.steps; ++it) {
        PathIO io{};
        io.fusedOwner = kNotFused;
        io.pixelList = r.pixelList; io.raysIn = b.rays[it & 1u]; io.hitsIn = b.hits[it & 1u]; io.countIn = r.cnt + it;
        io.raysOut = b.rays[(it + 1u) & 1u]; io.countOut = r.cnt + it + 1; io.state = b.state; io.stateStride = r.stride;
        io.iteration = it; io.raysPer = r.raysPer; io.part2List = r.part2List; io.part2Count = r.part2Count;
        // NEE's MIS list reuses the primary kernel's pixel list, which only step 0 reads (and step 0 has no ray results, hence no MIS entries)
        io.misList = b.pixels; io.misCount = r.misCounts ? r.misCounts + it : nullptr;
        if (r.stage == T_GI2) {                                  // owner lists ping-pong between the Part-2 list's buffer and the (by now free) primary list's
            io.ownersIn = (it & 1u) ? b.pixels : b.pixels2; io.ownersOut = (it & 1u) ? b.pixels2 : b.pixels;
        }
        hipLaunchKernelGGL(shade, shadeGrid, block, 0, c->stream, sc, cam, fr, st, io);
        ++*launched;
        if (r.stage == T_NEE && it > 0u) {                       // NEE: emitter-hit MIS for the few paths that need it (may add to the pick list)
            hipLaunchKernelGGL(k_nee_mis<CAM>, dim3((uint32_t)c->numCUs), block, 0, c->stream, sc, cam, fr, st, (const uint32_t*)io.misList, (const uint32_t*)io.misCount,
                               b.state, r.stride, r.part2List, io.countOut);
            ++*launched;
        }
        if (it == r.steps) break;                                // the last step only consumes: every path has emitted all its rays
        if (r.stage == T_NEE) {                                  // light pick + ray construction for the listed paths
            hipLaunchKernelGGL(k_nee_emit, shadeGrid, block, 0, c->stream, sc, st, (const uint32_t*)r.part2List, (const uint32_t*)io.countOut, b.state, r.stride, io.raysOut, r.raysPer);
            ++*launched;
        }
        TraceQueue q{};
        q.rays = io.raysOut; q.hits = b.hits[(it + 1u) & 1u]; q.count = io.countOut; q.raysPer = r.raysPer; q.head = r.heads + it + 1;
        set_queue_params(c, q, K_REFILL_LANES);
        if (simple) {
            const uint32_t sg = (uint32_t)std::min<size_t>((size_t)c->numCUs * 16u, (r.maxEntries * r.raysPer + kBlock - 1) / kBlock);
            hipLaunchKernelGGL(tsc.rayCounter ? k_trace_rays_simple<true> : k_trace_rays_simple<false>, dim3(std::max(1u, sg)), block, ldsBytes, c->stream, tsc, q);
        }
        else hipLaunchKernelGGL(tsc.rayCounter ? k_trace_rays<true> : k_trace_rays<false>, dim3((uint32_t)(c->numCUs * perCU)), block, ldsBytes, c->stream, tsc, q);
        ++*launched;
        // long sample x bounce products: stop once no path is alive any more.  Only inside a blocking call (fyprt_render, fyprt_render_rays)
        // — an asynchronous call (fyprt_render_async, group / comm frames, fyprt_render_rays_device) must not wait on the device: there
        // the remaining steps are launched and find empty lists (every kernel of a step returns at once on a count of zero)
        if (blocking && r.steps > 8u && (it & 3u) == 3u) {
            uint32_t alive = 0;
            HIPCHK(c, hipMemcpyAsync(&alive, io.countOut, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (alive == 0u) break;
        }
    }
    return c->hip(hipGetLastError(), "path stage launch");
}
}  // extern "C++"

// The shape of a path technique's (0-6) sample: rays a pixel emits one after the other = trace passes `steps`, rays per path and step,
// float4s of per-path state, and L = the length of each of its counter arrays (list counts, queue heads, NEE: MIS counts)
struct PathShape { uint32_t steps, raysPer, stride; size_t L; };
static PathShape path_shape(int tech, const DevSettings& st) {
    const uint32_t nSamples = (tech == FYPRT_BRUTE_FORCE) ? 1u : st.sampleCount;
    const uint32_t steps = (tech == FYPRT_LIGHT_SOURCE_SAMPLING) ? nSamples : nSamples * st.maxBounces;
    return {steps, (tech == FYPRT_NEE && st.maxBounces != 1u) ? 2u : 1u, (tech == FYPRT_NEE) ? 6u : 2u, (size_t)steps + 2};
}
// ... and its stage over the `entries` paths the primary kernel listed in `pixels`; `counters`: 3 L zeroed words, NEE's pick list: `pixels2`
static StageRun path_stage(int tech, const PathShape& p, uint32_t* pixels, uint32_t* pixels2, uint32_t* counters, size_t entries) {
    return StageRun{tech, p.steps, p.raysPer, p.stride, pixels, counters, counters + p.L, tech == FYPRT_NEE ? pixels2 : nullptr, nullptr, 0, tech == FYPRT_NEE ? counters + 2 * p.L : nullptr, entries};
}

// The "previous normals" of a ReSTIR frame are the last ReSTIR frame's, whichever of the two techniques rendered it (the reference keeps
// one pair of normal buffers for both; rt_refit.h: k_sync_history_normals).  Called before Part 1 — by the multi-GPU layer before the
// halo rows' history is fetched from their owners, so that what travels is already in step.
static int sync_restir_normals(fyprt_context* c, int tech, hipStream_t stream) {
    if (c->lastRestir < 0 || c->lastRestir == tech || c->W == 0) { return FYPRT_OK; }
    const uint32_t npx = c->W * c->H;
    DIRec* records = c->dprevFlip ? c->dprevB.p : c->dprevA.p;            // the history the next ReSTIR DI frame reads
    f2* normals = c->normalFlip ? c->normalB.p : c->normalA.p;            // the previous normals the next ReSTIR GI frame reads
    hipLaunchKernelGGL(k_sync_history_normals, dim3((npx + 255u) / 256u), dim3(256), 0, stream, records, normals, npx, tech == FYPRT_RESTIR_DI ? 1 : 0);
    c->lastRestir = tech;
    return c->hip(hipGetLastError(), "k_sync_history_normals");
}

// ---- a frame's host path: check_frame, begin_frame, one function per technique family, end_frame.  FrameRun carries what they share.
// sc: the frame's own copy of c->dsc — the four per-launch fields are set here, never in the context; ldsBytes: traversal stack (+ top nodes) of its
// traversing launches; par: queue / event parity; wavefront: ReSTIR DI Part 2 over a task queue; overlap: pipelined over two streams; split: ... and the
// history-free half of Part 1 on a third; fs: where Part 1 (split: its history half) + setup go; grid: tiles of the context's rows; ev, ei: its slot of
// the timing ring, the next event to record; launches: the parts it reports (not its kernels); part1Only: phase 1 — Part 1 is enqueued, the frame stops there
struct FrameRun {
    fyprt_context* c; const fyprt_settings* s; int tech, phase; bool timed;
    DevSettings st; DevFrame fr; DevScene sc; size_t ldsBytes;
    int par; bool wavefront, overlap, split, striped; hipStream_t fs; dim3 grid;
    Event* ev; int ei, launches, stageLaunches; bool part1Only;
};
static bool stripes_set(const fyprt_context* c) { return c->stripeRows != 0 && c->stripeRows < c->H && c->stripeParts > 1; }
static dim3 tile_grid(const fyprt_context* c, uint32_t rowBegin, uint32_t rowEnd) {
    const uint32_t tilesX = (c->W + 15u) / 16u, tilesY = (rowEnd - rowBegin + 15u) / 16u;
    return dim3(c->tuning[K_TILE_ORDER] == 2 ? tilesX * ((tilesY + 7u) / 8u) * 8u : ((tilesX * tilesY + 7u) / 8u) * 8u);
}
static unsigned long long* frame_counters(const fyprt_context* c, int part) { return c->countRays ? c->rayCounter.p + 8 * part : nullptr; }   // of the frame's launch `part`
// Every refusal of a frame; nothing is enqueued or modified before it passes.
static int check_frame(fyprt_context* c, const fyprt_settings* s, int phase) {
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, "host-only context (device -1) cannot render");
    if (!c->haveScene || !c->haveCamera || c->W == 0) return c->fail(FYPRT_ESTATE, "fyprt_render: resize, upload_scene and set_camera must precede render");
    if (c->dcam.W != c->W || c->dcam.H != c->H) return c->fail(FYPRT_ESTATE, "fyprt_render: camera viewport differs from the render size");
    const int tech = s->technique; const bool restir = tech == FYPRT_RESTIR_DI || tech == FYPRT_RESTIR_GI;
    if (tech < 0 || tech > 8) return c->fail(FYPRT_EINVAL, "fyprt_render: unknown technique");
    if (phase != 0 && !restir) return c->fail(FYPRT_EINVAL, "fyprt_render_part: only the ReSTIR techniques have two parts");
    if (phase == 2 && !c->part1Pending) return c->fail(FYPRT_ESTATE, "fyprt_render_part(2) without a preceding part 1");
    if (phase != 2 && c->part1Pending) return c->fail(FYPRT_ESTATE, "a frame's part 1 is pending: call fyprt_render_part(ctx, settings, 2) first");
    if ((tech == FYPRT_LIGHT_SOURCE_SAMPLING || tech == FYPRT_NEE) && (c->dsc.emissiveCount == 0 || c->dsc.ltTlasCount == 0))
        return c->fail(FYPRT_ENOLIGHT, "fyprt_render: technique needs emissive triangles and a light tree");
    if (tech == FYPRT_RESTIR_DI && c->dsc.emissiveCount == 0) return c->fail(FYPRT_ENOLIGHT, "fyprt_render: ReSTIR DI needs emissive triangles");
    if (restir && stripes_set(c)) return c->fail(FYPRT_ESTATE, "ReSTIR frames need contiguous rows: clear fyprt_set_row_stripes first");
    return FYPRT_OK;
}
// The descriptors, the pipelining decision, the memsets a new frame starts with and its slot of the timing ring.
static int begin_frame(FrameRun& f) {
    fyprt_context* c = f.c; DevFrame& fr = f.fr;
    HIPCHK(c, hipSetDevice(c->device));
    f.st = dev_settings(c, f.s);
    fr.accum = c->accum.p; fr.image = c->externalImage ? c->externalImage : c->image.p; fr.payload = c->payload.p; fr.depth = c->depth.p;
    fr.normalPrev = c->normalFlip ? c->normalB.p : c->normalA.p; fr.normalCur = c->normalFlip ? c->normalA.p : c->normalB.p;
    fr.di = c->di.p; fr.diPrev = c->diPrev.p; fr.gi = c->gi.p; fr.giPrev = c->giPrev.p; fr.giHot = c->giHot.p;
    fr.drec = c->drec.p; fr.dprevRead = c->dprevFlip ? c->dprevB.p : c->dprevA.p; fr.dprevWrite = c->dprevFlip ? c->dprevA.p : c->dprevB.p;
    fr.W = c->W; fr.H = c->H; fr.frameIndex = c->frameIndex; fr.rowBegin = c->rowBegin; fr.rowEnd = c->rowEnd;
    fr.stripeRows = 0; fr.stripeParts = 1; fr.stripePart = 0; f.striped = stripes_set(c);
    fr.histBegin = (f.tech == FYPRT_RESTIR_GI) ? c->histGI[0] : c->histDI[0]; fr.histEnd = (f.tech == FYPRT_RESTIR_GI) ? c->histGI[1] : c->histDI[1];
    // The scene as the frame's first launches read it: counters of part 0; the node-loop quorum of the fused per-pixel kernels and of coherent primary rays (key 7:
    // 0 = auto — 16 for the light-tree kernels (their shadow rays: NEE 5.2 -> 4.95 ms), none elsewhere (path and ReSTIR GI kernels: neutral or slightly negative))
#ifdef RT_TOPCACHE
    const uint32_t topCount = (uint32_t)std::min<size_t>((size_t)std::max(0, c->tuning[K_TOP_NODES]), c->hostBvh.nodes.size());
#else
    const uint32_t topCount = 0u;              // tuning key 16 only acts in a -DRT_TOPCACHE build (rt_device.h: measured slower)
#endif
    const StackLds stack = stack_lds(c, topCount);
    f.sc = secondary_scene(c->dsc, (uint32_t)c->tuning[K_QUORUM_PRIMARY], frame_counters(c, 0));
    f.sc.stackBudget = stack.budget; f.sc.topCount = topCount; f.ldsBytes = stack.bytes;
    // Pipelining (tuning key 11): a wavefront ReSTIR DI frame runs Part 1 + setup on the front stream and the trace kernel on `stream`.  Nothing the
    // front part writes is read or written by a trace kernel (payload, records, history, depth, its own task queue — two queues alternate), and image +
    // accumulation are touched by trace kernels only (p1Mode 1), which stay in frame order on `stream`; so frame N+1's front part may run beside frame
    // N's trace kernel.  Any other frame runs on `stream` alone, after everything before it.
    f.par = (int)(c->frameSerial & 1ull); f.wavefront = f.tech == FYPRT_RESTIR_DI && c->tuning[K_DI_WAVEFRONT] == 1;
    f.overlap = f.wavefront && c->tuning[K_PIPELINE] != 0 && !c->countRays && f.phase == 0;
    f.fs = f.overlap ? c->front : c->stream;
    // Split Part 1 (tuning key 21, asynchronous pipelined frames): everything of Part 1 up to the candidate reservoir needs the scene, the camera, the
    // frame index and the seed only — k_di_part1_primary computes it on `prim` into the staging set of the frame's parity, which nothing else reads,
    // while the front stream is still busy with frame N's setup kernel (which writes the history Part 1 merges); k_di_part1_temporal on the front
    // stream does the rest, and writes every public buffer where k_di_part1 did.  The API calls that edit the scene or reallocate wait for all three
    // streams first (sync_all), so `prim` itself waits for one thing: the temporal kernel that read this staging set, two frames ago.
    f.split = f.overlap && c->tuning[K_DI_SPLIT] != 0 && !c->blockingCall;
    if (f.overlap) {
        HIPCHK(c, hipStreamWaitEvent(c->front, c->evDone[f.par], 0));                            // frame N-2 done: its queue is free
        if (!c->lastOverlapped) HIPCHK(c, hipStreamWaitEvent(c->front, c->evDone[f.par ^ 1], 0));   // frame N-1 ran on `stream` alone
    }
    if (f.split) HIPCHK(c, hipStreamWaitEvent(c->prim, c->evTemp[f.par], 0));
    c->frameComplete = false;                  // from the first enqueued work until the frame is enqueued to its end (fyprt_denoise)
    if (f.tech != FYPRT_RESTIR_DI) c->drop_kept_primary();   // k_primary, k_gi_primary and k_path_fused write the payload too, and keep nothing
    fr.tileOrder = (uint32_t)c->tuning[K_TILE_ORDER]; fr.p1Mode = f.wavefront ? 1u : 0u;
    f.grid = tile_grid(c, c->rowBegin, c->rowEnd); f.ev = c->ring[c->frameSerial % fyprt_context::kRing];
    if (f.phase == 2) { f.ei = 2; return FYPRT_OK; }          // part 1 recorded its start and its end
    std::memcpy(c->framePV, c->camPV, 64);     // the camera this frame is rendered with (fyprt_denoise_temporal)
    c->frameCam = c->dcam; c->frameSky = f.st.sky;   // ... and what fyprt_denoise_upscale traces and colours its hi-res primary rays with
    if (c->countRays) HIPCHK(c, hipMemsetAsync(c->rayCounter.p, 0, 256, c->stream));
    // frame 1 (or toAccumulate == false): the accumulator starts from zero (Renderer.cu:50-51) — on `stream`, which owns it (the whole buffer, as the
    // reference does, not just this context's rows: a band moved later with fyprt_set_rows must not find the sums of an earlier accumulation in its new rows)
    if (c->frameIndex == 1) HIPCHK(c, hipMemsetAsync(c->accum.p, 0, c->accum.bytes(), c->stream));
    if (f.timed) HIPCHK(c, hipEventRecord(f.ev[f.ei++], f.split ? c->prim.h : f.fs));
    return FYPRT_OK;
}
// One stage of the wavefront path engine (rt_paths.h) on the frame's scene, with the wf* buffers as ensure_paths left them
static int run_frame_stage(FrameRun& f, const StageRun& r) {
    fyprt_context* c = f.c;
    const StageBufs wf{{c->wfRays[0].p, c->wfRays[1].p}, {c->wfHits[0].p, c->wfHits[1].p}, c->wfState.p, c->wfPixels.p, c->wfPixels2.p, frame_counters(c, 0)};
    return run_stage(c, r, wf, f.sc, c->dcam, f.fr, f.st, f.ldsBytes, c->blockingCall, &f.stageLaunches);
}
// Techniques 0-6: the primary kernel, then per step one shade launch + one trace launch (run_stage) — or, small trees, the whole frame in one launch.
static int enqueue_path_frame(FrameRun& f) {
    fyprt_context* c = f.c; DevFrame& fr = f.fr; const int tech = f.tech;
    const PathShape p = path_shape(tech, f.st);
    dim3 pgrid = f.grid;
    if (f.striped) {                                           // k_primary maps the local rows [0, n) onto this context's stripes
        fr.stripeRows = c->stripeRows; fr.stripeParts = c->stripeParts; fr.stripePart = c->stripePart;
        fr.rowBegin = 0; fr.rowEnd = stripe_row_count(c->H, c->stripeRows, c->stripeParts, c->stripePart);
        pgrid = tile_grid(c, fr.rowBegin, fr.rowEnd);
    }
    const size_t entries = (size_t)(fr.rowEnd - fr.rowBegin) * c->W;
    TRY(ensure_paths(c, entries, p.raysPer, p.stride, 3 * p.L));
    HIPCHK(c, hipMemsetAsync(c->wfCounters.p, 0, 3 * p.L * sizeof(uint32_t), c->stream));
    f.launches = 1;                                            // (a frame reports its parts as launches, not its kernels)
    // small trees, techniques 0-5: the whole frame in one launch, one thread per pixel (rt_paths.h: k_path_fused; key 17: 0 = by tree size, 1 = never, 2 = always)
    const bool fused = tech != FYPRT_NEE && (c->tuning[K_FUSED_FRAME] == 2 || (c->tuning[K_FUSED_FRAME] == 0 && c->hostBvh.tris.size() < 65536u));
    if (fused) {
        PathIO io{};
        io.fusedOwner = kNotFused; io.raysIn = c->wfRays[0].p; io.raysOut = c->wfRays[0].p; io.hitsIn = c->wfHits[0].p; io.state = c->wfState.p; io.stateStride = p.stride; io.raysPer = 1u;
        static void (*const kFused[2][6])(DevScene, DevCamera, DevFrame, DevSettings, PathIO, uint32_t) = {{k_path_fused<T_BRUTE, false>, k_path_fused<T_UNIFORM, false>, k_path_fused<T_COSINE, false>, k_path_fused<T_GGX, false>, k_path_fused<T_BRDF, false>, k_path_fused<T_LIGHT, false>},
                                                    {k_path_fused<T_BRUTE, true>, k_path_fused<T_UNIFORM, true>, k_path_fused<T_COSINE, true>, k_path_fused<T_GGX, true>, k_path_fused<T_BRDF, true>, k_path_fused<T_LIGHT, true>}};
        hipLaunchKernelGGL(kFused[c->countRays ? 1 : 0][tech], pgrid, dim3(kBlock), f.ldsBytes, c->stream, f.sc, c->dcam, fr, f.st, io, p.steps);
        return FYPRT_OK;
    }
    hipLaunchKernelGGL(c->countRays ? k_primary<true> : k_primary<false>, pgrid, dim3(kBlock), f.ldsBytes, c->stream, f.sc, c->dcam, fr, f.st, c->wfPixels.p, c->wfCounters.p);
    return run_frame_stage(f, path_stage(tech, p, c->wfPixels.p, c->wfPixels2.p, c->wfCounters.p, entries));
}
// The rows Part 1 of a ReSTIR frame runs on, and its grid.  Halo rows: Part 1 recomputed on them (default), or — exchange mode — left to the band that
// owns them and copied in between the parts.  The reference's spatial-neighbour coordinate is computed in unsigned arithmetic (R.cu:1916-1917): an offset
// above the first row wraps and clamps to the LAST row.  A band that owns rows < radius therefore also needs Part 1 of row H-1 (one extra row of
// recompute) to stay bit-identical to a single-GPU frame.  It rides in the same launch as one more row of tiles (a separate one-row launch is all
// latency: ~0.09 ms on a 135-row band).
struct Part1Rows { uint32_t begin, end, extraRow; size_t pixels; dim3 grid; };
static Part1Rows part1_rows(const fyprt_context* c) {
    const uint32_t halo = (c->haloExchange || c->tuning[K_SKIP_HALO_PART1]) ? 0u : c->halo;
    const uint32_t b = (c->rowBegin > halo) ? c->rowBegin - halo : 0u, e = (c->rowEnd + halo < c->H) ? c->rowEnd + halo : c->H;
    const bool extra = halo > 0 && c->rowBegin < halo && e < c->H;
    return {b, e, extra ? c->H - 1u : 0xFFFFFFFFu, ((size_t)(e - b) + (extra ? 1u : 0u)) * c->W, tile_grid(c, b, extra ? e + 16u : e)};
}
// ReSTIR GI.  Part 1 = primary kernel + bounce-loop steps (they build the Part-2 list as paths complete); Part 2 = the neighbour loop over that
// list (wfPixels2, cnt2[0] = its length): as stages (tuning key 19 = 0) or in one launch.
static int enqueue_gi_frame(FrameRun& f) {
    fyprt_context* c = f.c; const Part1Rows p1 = part1_rows(c);
    const uint32_t steps1 = f.st.maxBounces, steps2 = f.st.useSpatial ? f.st.numNeighbors : 0u;
    const size_t L1 = (size_t)steps1 + 2, L2 = (size_t)steps2 + 2;
    TRY(ensure_paths(c, p1.pixels, 1, 5, 2 * L1 + 2 * L2));
    uint32_t* cnt1 = c->wfCounters.p; uint32_t* cnt2 = cnt1 + 2 * L1;
    if (f.phase != 2) {
        TRY(sync_restir_normals(c, f.tech, c->stream));   // the last ReSTIR frame was a DI frame: its normals (in the history records) are this frame's "previous normals"
        HIPCHK(c, hipMemsetAsync(cnt1, 0, (2 * L1 + 2 * L2) * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(c->countRays ? k_gi_primary<true> : k_gi_primary<false>, p1.grid, dim3(kBlock), f.ldsBytes, c->stream, f.sc, c->dcam, f.fr, f.st, p1.begin, p1.end, p1.extraRow, c->wfPixels.p, cnt1);
        TRY(run_frame_stage(f, StageRun{T_GI1, steps1, 1u, 5u, c->wfPixels.p, cnt1, cnt1 + L1, c->wfPixels2.p, cnt2, 0, nullptr, p1.pixels}));
        if (f.timed) HIPCHK(c, hipEventRecord(f.ev[f.ei++], c->stream));
        if (f.phase == 1) { f.part1Only = true; return c->hip(hipGetLastError(), "ReSTIR GI part 1"); }
    }
    const DevScene tsc = secondary_scene(f.sc, (uint32_t)c->tuning[K_QUORUM_SECONDARY], frame_counters(c, 1));      // of the one-launch forms
    if (c->tuning[K_GI2_MODE] == 2) {
        // one PERSISTENT launch (rt_paths.h: k_gi2_persistent): a lane owns a pixel of the list, lanes without a ray in flight are serviced together
        const int occ = c->gi2Occ.get(k_gi2_persistent<false>, f.ldsBytes, 3), perCU = c->tuning[K_WG_PER_CU] > 0 ? std::min(c->tuning[K_WG_PER_CU], occ) : occ;
        GI2Queue gq{c->wfPixels2.p, cnt2, cnt2 + L2 + 1};
        set_queue_params(c, gq, K_GI2_REFILL_LANES);
        hipLaunchKernelGGL(c->countRays ? k_gi2_persistent<true> : k_gi2_persistent<false>, dim3((uint32_t)(c->numCUs * perCU)), dim3(kBlock), f.ldsBytes, c->stream, tsc, c->dcam, f.fr, f.st, gq);
    } else if (c->tuning[K_GI2_MODE] == 1) {
        // one launch (rt_paths.h: k_gi2_fused): one thread per listed pixel for the whole neighbour loop, visibility rays traced in place
        const uint32_t fg = (uint32_t)std::max<size_t>(1, std::min<size_t>((size_t)c->numCUs * 64u, (p1.pixels + kBlock - 1) / kBlock));
        hipLaunchKernelGGL(c->countRays ? k_gi2_fused<true> : k_gi2_fused<false>, dim3(fg), dim3(kBlock), f.ldsBytes, c->stream, tsc, c->dcam, f.fr, f.st, (const uint32_t*)c->wfPixels2.p, (const uint32_t*)cnt2);
    } else TRY(run_frame_stage(f, StageRun{T_GI2, steps2, 1u, 5u, c->wfPixels2.p, cnt2, cnt2 + L2, nullptr, nullptr, 1, nullptr, p1.pixels}));
    f.launches = 2; c->normalFlip = !c->normalFlip; c->histGI[0] = c->rowBegin; c->histGI[1] = c->rowEnd;
    return FYPRT_OK;
}
// ReSTIR DI Part 2 as a wavefront: the setup kernel queues the frame's shadow rays as tasks (optionally sorted by light), one persistent
// kernel traces them.  Setup and sort go where Part 1 went (f.fs), the trace kernel on the context stream.
static int enqueue_di_wavefront_part2(FrameRun& f) {
    fyprt_context* c = f.c; const int par = f.par; const dim3 grid = f.grid; hipStream_t fs = f.fs;
    const dim3 block(kBlock);
    ShadowQueue q{};
    q.tasks = c->shadowTasks.p + (size_t)par * c->queueStride; q.rayless = q.tasks + c->queueStride; q.counters = c->queueCounters.p + 4 * par;
    set_queue_params(c, q, K_REFILL_LANES);
    const size_t sg = (size_t)par * c->sortGroups;
    q.sortMode = c->tuning[K_SORT_TASKS] ? 1u : 0u; q.numGroups = grid.x; q.counts = c->sortCounts.p + 2 * sg; q.bases = q.counts + c->sortGroups; q.keys = c->sortKeys.p + sg * 256u; q.hist = c->sortHist.p + sg * kSortBins;
    q.binOffset = c->sortOffset.p + sg * kSortBins; q.binTotal = c->sortTotal.p + (size_t)par * kSortBins; q.sorted = c->sortIndex.p + sg * 256u;
    HIPCHK(c, hipMemsetAsync(q.counters, 0, 16, fs));
    static void (*const kSetup[3])(DevScene, DevCamera, DevFrame, DevSettings, ShadowQueue) = {k_di_part2_setup<0>, k_di_part2_setup<1>, k_di_part2_setup<2>};
    hipLaunchKernelGGL(kSetup[c->tuning[K_SETUP_FETCH]], grid, block, 0, fs, f.sc, c->dcam, f.fr, f.st, q);
    if (q.sortMode) {
        hipLaunchKernelGGL(k_di_sort_scan, dim3(kSortBins), block, 0, fs, q);
        hipLaunchKernelGGL(k_di_sort_scatter, grid, block, 0, fs, q);
    }
    if (f.timed) HIPCHK(c, hipEventRecord(f.ev[f.ei++], fs));
    if (f.overlap) {                                   // the trace kernel waits for this frame's front part only
        HIPCHK(c, hipEventRecord(c->evFront[par], c->front));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->evFront[par], 0));
        if (f.timed) HIPCHK(c, hipEventRecord(f.ev[4], c->stream));      // start of the trace kernel on its own stream
    }
    f.sc.rayCounter = frame_counters(c, 2);
    int perCU = c->tuning[K_WG_PER_CU];
    if (perCU <= 0) {          // as many workgroups as registers + LDS let a CU hold (asked from the runtime once per stack size)
        perCU = c->traceOcc.get(k_di_part2_trace<false>, f.ldsBytes, 4);
        // pipelined frames: the persistent grid shares the chip with Part 1 + setup of the NEXT frame; with every slot a CU has (6 workgroups) those start late and run in
        // extra rounds — 4 per CU leave them room: an eighth of the frame (a multi-GPU band) renders in 0.228 instead of 0.252 ms, the whole frame in the same 0.888 ms (profiles/README.md r03)
        if (f.overlap && perCU > 4) perCU = 4;
    }
    // persistent grid: as many workgroups as the chip holds — but not more than the band has tasks for (one lane per task): a narrow
    // multi-GPU band would otherwise park idle workgroups on the LDS / wave slots the next frame's Part 1 is waiting for
    const uint32_t traceGrid = std::max(8u, std::min((uint32_t)(c->numCUs * perCU), grid.x));
    hipLaunchKernelGGL(c->countRays ? k_di_part2_trace<true> : k_di_part2_trace<false>, dim3(traceGrid), block, f.ldsBytes, c->stream, f.sc, f.fr, q);
#ifdef RT_DI_LEAF_STATS
    {   // test build only (rt_wavefront.h): the kinds of leaf phase the production kernel ran in this frame
        uint32_t kinds = 0;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(&kinds, q.counters + 3, sizeof kinds, hipMemcpyDeviceToHost));
        std::fprintf(stderr, "fyprt leaf phases: grid %u, rays %s, kinds 0x%x (1 one round, 2 over 64 pairs, 4 single-triangle leaves, 8 closest-mode lane)\n", traceGrid, c->countRays ? "counted" : "production", kinds);
    }
#endif
    f.launches = 3;
    return FYPRT_OK;
}
// Kept primary hits (fyprt_context::KeptPrimary).  May this frame read the payload instead of tracing it: it counts no rays, and the payload
// in place was traced for exactly its band and Part-1 rows with the five camera fields ray_direction and trace_ray read, byte for byte (compared
// here, at frame time: fyprt_set_camera with the same matrices, or with other prev_* matrices, keeps it; fyprt_set_rows, the halo mode
// and key 13 need no hook)
static bool kept_primary_usable(const fyprt_context* c, const Part1Rows& p1) {
    const fyprt_context::KeptPrimary& k = c->kept; const DevCamera& d = c->dcam;
    return k.valid && !c->countRays && c->tuning[K_KEEP_PRIMARY] != 0 && k.begin == p1.begin && k.end == p1.end && k.extraRow == p1.extraRow && k.rowBegin == c->rowBegin && k.rowEnd == c->rowEnd && k.W == d.W && k.H == d.H &&
           !std::memcmp(&k.invProj, &d.invProj, sizeof d.invProj) && !std::memcmp(&k.invView, &d.invView, sizeof d.invView) && !std::memcmp(&k.position, &d.position, sizeof d.position);
}
// ... and a frame that traced leaves it: `writer` is the stream whose last launch wrote c->payload
static int establish_kept_primary(fyprt_context* c, const Part1Rows& p1, hipStream_t writer) {
    fyprt_context::KeptPrimary& k = c->kept; const DevCamera& d = c->dcam;
    k.valid = true; k.begin = p1.begin; k.end = p1.end; k.extraRow = p1.extraRow; k.rowBegin = c->rowBegin; k.rowEnd = c->rowEnd; k.invProj = d.invProj; k.invView = d.invView; k.position = d.position; k.W = d.W; k.H = d.H; k.writer = writer;
    HIPCHK(c, hipEventRecord(c->evPayload, writer));
    return FYPRT_OK;
}
// ReSTIR DI.  Part 1: candidates + temporal reuse per pixel; Part 2: spatial reuse + shadow rays, as a wavefront (tuning key 1) or per pixel.
// Who touches c->payload in Part 1, and why no two of them meet:
//   a tracing frame  writes it in k_di_part1_temporal<false> on `front` (split) or in k_di_part1<.., false> on f.fs, and records evPayload behind it;
//   a kept frame     writes it nowhere and reads it in k_di_part1_primary<false, true> on `prim` and k_di_part1_temporal<true> on `front`, or in
//                    k_di_part1<false, true> on f.fs — each behind evPayload where the stream is not the writer's own.
//   A tracing split frame after kept ones writes on `front` behind its own evPrim, and `prim` runs in order: every earlier kept primary kernel
//   is done.  A tracing unsplit frame has no evPrim of its own and waits for both parities' — the later one covers every kept primary kernel.
//   The setup kernel and the denoisers read the payload as before (dn_call_done's dnDone wait stays: a tracing frame may follow any call).
static int enqueue_di_frame(FrameRun& f) {
    fyprt_context* c = f.c;
    if (f.phase != 2) {
        const Part1Rows p1 = part1_rows(c);
        const bool kept = kept_primary_usable(c, p1);
        if (kept) c->keptFrames++;
        if (f.split) {               // part 0 of the frame's timings: the primary kernel, between its own events on `prim`
            const size_t npx = (size_t)c->W * c->H;
            const DIStage sg{kept ? nullptr : c->stagePayload.p + (size_t)f.par * npx, c->stageRec.p + (size_t)f.par * npx};
            if (kept) {
                HIPCHK(c, hipStreamWaitEvent(c->prim, c->evPayload, 0));      // long signalled in steady state
                hipLaunchKernelGGL((k_di_part1_primary<false, true>), p1.grid, dim3(kBlock), 0, c->prim, f.sc, c->dcam, f.fr, f.st, p1.begin, p1.end, p1.extraRow, sg);
            } else hipLaunchKernelGGL((k_di_part1_primary<false, false>), p1.grid, dim3(kBlock), f.ldsBytes, c->prim, f.sc, c->dcam, f.fr, f.st, p1.begin, p1.end, p1.extraRow, sg);
            if (f.timed) HIPCHK(c, hipEventRecord(f.ev[f.ei++], c->prim));
            HIPCHK(c, hipEventRecord(c->evPrim[f.par], c->prim));
            HIPCHK(c, hipStreamWaitEvent(c->front, c->evPrim[f.par], 0));
            TRY(sync_restir_normals(c, f.tech, f.fs));
            if (f.timed) HIPCHK(c, hipEventRecord(f.ev[5], c->front));   // part 1: temporal + setup, from here to the event behind the setup kernel
            if (kept && c->kept.writer != c->front.h) HIPCHK(c, hipStreamWaitEvent(c->front, c->evPayload, 0));
            hipLaunchKernelGGL(kept ? k_di_part1_temporal<true> : k_di_part1_temporal<false>, p1.grid, dim3(kBlock), 0, c->front, f.sc, c->dcam, f.fr, f.st, p1.begin, p1.end, p1.extraRow, sg);
            HIPCHK(c, hipEventRecord(c->evTemp[f.par], c->front));
            if (!kept) TRY(establish_kept_primary(c, p1, c->front));
        } else {
            TRY(sync_restir_normals(c, f.tech, f.fs));   // the last ReSTIR frame was a GI frame: its normals are this frame's "previous normals"
            if (kept) {
                if (c->kept.writer != f.fs) HIPCHK(c, hipStreamWaitEvent(f.fs, c->evPayload, 0));
                hipLaunchKernelGGL((k_di_part1<false, true>), p1.grid, dim3(kBlock), 0, f.fs, f.sc, c->dcam, f.fr, f.st, p1.begin, p1.end, p1.extraRow);
            } else {
                for (int k = 0; k < 2; ++k) HIPCHK(c, hipStreamWaitEvent(f.fs, c->evPrim[k], 0));
                hipLaunchKernelGGL((c->countRays ? k_di_part1<true, false> : k_di_part1<false, false>), p1.grid, dim3(kBlock), f.ldsBytes, f.fs, f.sc, c->dcam, f.fr, f.st, p1.begin, p1.end, p1.extraRow);
                TRY(establish_kept_primary(c, p1, f.fs));
            }
            if (f.timed) HIPCHK(c, hipEventRecord(f.ev[f.ei++], f.fs));
        }
        if (f.phase == 1) { f.part1Only = true; return c->hip(hipGetLastError(), "ReSTIR DI part 1"); }
    }
    // shadow-ray kernels of Part 2: the secondary quorum (measured 0.85 -> 0.68 ms), counters of their own
    f.sc = secondary_scene(f.sc, (uint32_t)c->tuning[K_QUORUM_SECONDARY], frame_counters(c, 1)); f.launches = 2;
    if (f.wavefront) TRY(enqueue_di_wavefront_part2(f));
    else hipLaunchKernelGGL(c->countRays ? k_di_part2<true> : k_di_part2<false>, f.grid, dim3(kBlock), f.ldsBytes, c->stream, f.sc, c->dcam, f.fr, f.st);
    c->dprevFlip = !c->dprevFlip; c->histDI[0] = c->rowBegin; c->histDI[1] = c->rowEnd;
    return FYPRT_OK;
}
// The frame is enqueued to its end: its last timing event, evDone, the ring's and the context's bookkeeping.
static int end_frame(FrameRun& f) {
    fyprt_context* c = f.c; const unsigned long long slot = c->frameSerial % fyprt_context::kRing;
    HIPCHK(c, hipGetLastError());
    c->part1Pending = false;
    if (f.timed) HIPCHK(c, hipEventRecord(f.ev[f.ei++], c->stream));
    HIPCHK(c, hipEventRecord(c->evDone[f.par], c->stream));                // the frame is complete (and its task queue free again)
    c->lastOverlapped = f.overlap; c->lastLaunches = f.launches; c->lastTech = f.tech;
    if (f.tech == FYPRT_RESTIR_DI || f.tech == FYPRT_RESTIR_GI) c->lastRestir = f.tech;
    c->ringLaunches[slot] = f.timed ? f.launches : 0; c->ringSplit[slot] = f.split ? 2 : f.overlap ? 1 : 0;
    c->frameSerial++; c->frameComplete = true; c->lastFrameIndex = c->frameIndex;
    if (f.s->to_accumulate) c->frameIndex++; else c->frameIndex = 1;       // Renderer.cu:258-261
    return FYPRT_OK;
}
// phase: 0 = the whole frame; 1 = ReSTIR Part 1 only (nothing of the frame's bookkeeping advances); 2 = the rest of the frame that a
// phase-1 call started.  The split exists for the halo EXCHANGE of a multi-GPU frame (fyprt_multi.h): Part 1 on every band, the
// bands' Part-1 records of each other's halo rows copied across, Part 2 on every band.
static int enqueue_frame(fyprt_context* c, const fyprt_settings* s, bool timed, int phase = 0) {
    FrameRun f{}; f.c = c; f.s = s; f.tech = s->technique; f.phase = phase; f.timed = timed;
    int rc = check_frame(c, s, phase);
    if (rc == FYPRT_OK) rc = begin_frame(f);
    if (rc == FYPRT_OK) rc = f.tech == FYPRT_RESTIR_DI ? enqueue_di_frame(f) : f.tech == FYPRT_RESTIR_GI ? enqueue_gi_frame(f) : enqueue_path_frame(f);
    if (rc == FYPRT_OK) { if (f.part1Only) c->part1Pending = true; else rc = end_frame(f); }
    if (rc != FYPRT_OK && rc != FYPRT_ESTATE) c->part1Pending = false;      // a frame that failed half-way is abandoned, not left pending
    return rc;
}
// Time of part `k` of the frame in ring slot `slot`, between its timing events; the trace kernel of a pipelined frame has its own start event, and
// so has the front part (temporal + setup) of a frame whose Part 1 was split
static hipError_t part_elapsed(fyprt_context* c, unsigned long long slot, int k, float* ms) {
    const int mode = c->ringSplit[slot], start = (mode && k == 2) ? 4 : (mode == 2 && k == 1) ? 5 : k;
    return hipEventElapsedTime(ms, c->ring[slot][start], c->ring[slot][k + 1]);
}

int fyprt_render(fyprt_context* c, const fyprt_settings* s, fyprt_frame_stats* stats) {
    if (!c || !s) return FYPRT_EINVAL;
    c->blockingCall = true;
    int rc = enqueue_frame(c, s, true);
    c->blockingCall = false;
    if (rc != FYPRT_OK) return rc;
    HIPCHK(c, sync_all(c));                            // cudaDeviceSynchronize, Renderer.cu:237
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->launches = (uint32_t)c->lastLaunches;
        float total = 0.0f;
        for (int k = 0; k < c->lastLaunches; ++k) {
            float ms = 0.0f; (void)part_elapsed(c, (c->frameSerial - 1ull) % fyprt_context::kRing, k, &ms);
            stats->kernel_ms_part[k] = ms; total += ms;
        }
        stats->kernel_ms = total;
        if (c->countRays) {
            unsigned long long r[32] = {0}; (void)hipMemcpy(r, c->rayCounter.p, 256, hipMemcpyDeviceToHost);
            for (int k = 0; k < 4; ++k) add_ray_stats(stats, k, r + 8 * k);
        }
    }
    return FYPRT_OK;
}

int fyprt_render_async(fyprt_context* c, const fyprt_settings* s) { if (!c || !s) return FYPRT_EINVAL; return enqueue_frame(c, s, true); }

int fyprt_frame_timings(fyprt_context* c, uint32_t frames_back, float* kernel_ms_part4, uint32_t* launches) {
    if (!c || !kernel_ms_part4) return FYPRT_EINVAL;
    if (frames_back >= (uint32_t)fyprt_context::kRing || frames_back >= c->frameSerial) return c->fail(FYPRT_EINVAL, "fyprt_frame_timings: frame no longer in the ring");
    const unsigned long long slot = (c->frameSerial - 1ull - frames_back) % fyprt_context::kRing;
    const int n = c->ringLaunches[slot];
    for (int k = 0; k < 4; ++k) kernel_ms_part4[k] = 0.0f;
    for (int k = 0; k < n && k < 4; ++k) {
        float ms = 0.0f;
        const hipError_t e = part_elapsed(c, slot, k, &ms);
        if (e != hipSuccess) return c->hip(e, "hipEventElapsedTime (synchronize the context first)");
        kernel_ms_part4[k] = ms;
    }
    if (launches) *launches = (uint32_t)n;
    return FYPRT_OK;
}
int fyprt_synchronize(fyprt_context* c) { if (!c) return FYPRT_EINVAL; if (c->hostOnly) return FYPRT_OK; HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c)); return FYPRT_OK; }

int fyprt_readback(fyprt_context* c, uint32_t* rgba8, float* accum4) {
    if (!c) return FYPRT_EINVAL;
    if (c->hostOnly || c->W == 0) return c->fail(FYPRT_ESTATE, "fyprt_readback before fyprt_resize");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    const size_t off = (size_t)c->rowBegin * c->W, cnt = (size_t)(c->rowEnd - c->rowBegin) * c->W;
    const uint32_t* img = c->externalImage ? c->externalImage : c->image.p;
    if (rgba8) HIPCHK(c, hipMemcpy(rgba8 + off, img + off, cnt * 4, hipMemcpyDeviceToHost));
    if (accum4) HIPCHK(c, hipMemcpy(accum4 + off * 4, c->accum.p + off, cnt * 16, hipMemcpyDeviceToHost));
    return FYPRT_OK;
}

// The lean correctly rounded sqrt / reciprocal / reciprocal square root of rt_math.h against the compiler's sequences on all 2^32
// arguments each (a few milliseconds).  mismatches[3] / first_bad[3] in the order sqrt, 1/x, 1/sqrt(x); all zero on a sound build.
int fyprt_selftest_math(fyprt_context* c, uint64_t* mismatches3, uint32_t* first_bad3) {
    if (!c || !mismatches3) return FYPRT_EINVAL;
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, "fyprt_selftest_math needs a device");
    HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c));
    DevBuf<unsigned long long> counts; DevBuf<uint32_t> first;
    HIPCHK(c, counts.alloc(3)); HIPCHK(c, first.alloc(3));
    hipError_t e = hipMemsetAsync(counts.p, 0, 24, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(first.p, 0xFF, 12, c->stream);
    for (int w = 0; w < 3 && e == hipSuccess; ++w) { hipLaunchKernelGGL(k_math_selftest, dim3((uint32_t)c->numCUs * 16u), dim3(256), 0, c->stream, w, counts.p, first.p); e = hipGetLastError(); }
    unsigned long long hc[3] = {0, 0, 0}; uint32_t hf[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(hc, counts.p, 24, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hf, first.p, 12, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIPCHK(c, e);
    for (int w = 0; w < 3; ++w) { mismatches3[w] = hc[w]; if (first_bad3) first_bad3[w] = hf[w]; }
    return FYPRT_OK;
}

// One shading function (`probe`, enum fyprt_probe) evaluated on `count` caller-supplied argument records by the inline functions the frame
// kernels call (rt_probe.h); include/fyprt.h documents the records.  Touches no frame state: its buffers live for the call only.
int fyprt_selftest_functions(fyprt_context* c, int probe, const void* in, uint32_t count, void* out) {
    static_assert((int)P_COUNT == (int)FYPRT_PROBE_COUNT && (int)P_ASIN_KERNEL == (int)FYPRT_PROBE_ASIN_KERNEL, "enum fyprt_probe");
    if (!c) return FYPRT_EINVAL;
    if (probe < 0 || probe >= (int)P_COUNT) return c->fail(FYPRT_EINVAL, "fyprt_selftest_functions: unknown probe");
    if (count && (!in || !out)) return c->fail(FYPRT_EINVAL, "fyprt_selftest_functions: NULL records with a non-zero count");
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, "fyprt_selftest_functions needs a device");
    if (probe == (int)P_SAMPLE_ALBEDO && !c->haveScene) return c->fail(FYPRT_ESTATE, "fyprt_selftest_functions: the sample_albedo probe reads the uploaded scene's textures (before fyprt_upload_scene)");
    if (count == 0) return FYPRT_OK;
    HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c));
    const uint32_t inWords = kProbeIn[probe], outWords = kProbeOut[probe];
    DevBuf<uint32_t> din, dout;
    HIPCHK(c, din.alloc((size_t)count * inWords)); HIPCHK(c, dout.alloc((size_t)count * outWords));
    hipError_t e = hipMemcpyAsync(din.p, in, din.bytes(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const uint32_t blocks = std::min((count + (uint32_t)kBlock - 1u) / (uint32_t)kBlock, (uint32_t)c->numCUs * 16u);
        hipLaunchKernelGGL(k_probe_functions, dim3(blocks), dim3(kBlock), 0, c->stream, probe, c->dsc, din.p, inWords, dout.p, outWords, count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, dout.bytes(), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);      // also after a failed enqueue: the buffers are freed on return
    HIPCHK(c, e != hipSuccess ? e : es);
    return FYPRT_OK;
}

// MisUtils::ComputeMSE / ComputePSNR (MisUtils.cpp:118-157) of the frame on the device against a host reference image (the benchmark
// workflow of WalnutApp.cpp:826-876 without reading the frame back): RGB channels of the 8-bit images, this context's rows.
int fyprt_compare_image(fyprt_context* c, const uint32_t* reference_rgba8, int flip_reference_rows, double* mse, double* psnr) {
    if (!c || !reference_rgba8 || !mse) return FYPRT_EINVAL;
    if (c->hostOnly || c->W == 0) return c->fail(FYPRT_ESTATE, "fyprt_compare_image before fyprt_resize");
    HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c));
    const size_t n = (size_t)c->W * c->H;
    if (c->refImage.n != n) HIPCHK(c, c->refImage.alloc(n));
    TRY(upload(c, c->refImage.p, reference_rgba8, n * 4));
    HIPCHK(c, hipMemsetAsync(c->rayCounter.p + 31, 0, 8, c->stream));            // (the last, unused counter word serves as the accumulator)
    const uint32_t* img = c->externalImage ? c->externalImage : c->image.p;
    hipLaunchKernelGGL(k_image_sqdiff, dim3((uint32_t)c->numCUs * 4u), dim3(256), 0, c->stream, img, c->refImage.p, c->W, c->H, c->rowBegin, c->rowEnd, flip_reference_rows ? 1 : 0, c->rayCounter.p + 31);
    HIPCHK(c, hipGetLastError());
    unsigned long long tot = 0;
    HIPCHK(c, hipMemcpyAsync(&tot, c->rayCounter.p + 31, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *mse = (double)tot / ((double)((size_t)(c->rowEnd - c->rowBegin) * c->W) * 3.0);
    if (psnr) *psnr = (*mse == 0.0) ? (double)INFINITY : 10.0 * std::log10(255.0 * 255.0 / *mse);
    return FYPRT_OK;
}

int fyprt_image_device_ptr(fyprt_context* c, void** p) { if (!c || !p) return FYPRT_EINVAL; *p = c->externalImage ? (void*)c->externalImage : (void*)c->image.p; return FYPRT_OK; }
int fyprt_set_external_image(fyprt_context* c, void* p) { if (!c) return FYPRT_EINVAL; c->externalImage = (uint32_t*)p; return FYPRT_OK; }
int fyprt_stream(fyprt_context* c, void** s) { if (!c || !s) return FYPRT_EINVAL; *s = (void*)c->stream; return FYPRT_OK; }

int fyprt_read_buffer(fyprt_context* c, int which, void* dst, size_t bytes) {
    if (!c || !dst) return FYPRT_EINVAL;
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, "host-only context has no device buffers");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));
    const void* src = nullptr; size_t n = 0;
    switch (which) {
        case FYPRT_BUF_ACCUM: src = c->accum.p; n = c->accum.bytes(); break;
        case FYPRT_BUF_IMAGE: src = c->externalImage ? c->externalImage : c->image.p; n = c->image.bytes(); break;
        case FYPRT_BUF_PAYLOAD: src = c->payload.p; n = c->payload.bytes(); break;
        case FYPRT_BUF_DEPTH: src = c->depth.p; n = c->depth.bytes(); break;
        case FYPRT_BUF_NORMAL: src = c->normalFlip ? c->normalB.p : c->normalA.p; n = c->normalA.bytes(); break;   // after the flip "prev" = frame just rendered
        case FYPRT_BUF_DI_RESERVOIR: src = c->di.p; n = c->di.bytes(); break;
        case FYPRT_BUF_DI_PREV: src = c->diPrev.p; n = c->diPrev.bytes(); break;
        case FYPRT_BUF_GI_RESERVOIR: src = c->gi.p; n = c->gi.bytes(); break;
        case FYPRT_BUF_GI_PREV: src = c->giPrev.p; n = c->giPrev.bytes(); break;
        case FYPRT_BUF_ALBEDO:
            if (!c->albedoValid) return c->fail(FYPRT_ESTATE, "fyprt_read_buffer: FYPRT_BUF_ALBEDO is written by fyprt_denoise");
            src = c->dn.albedo.p; n = c->dn.albedo.bytes(); break;
        case FYPRT_BUF_TEMPORAL:
            if (!c->dtValid) return c->fail(FYPRT_ESTATE, "fyprt_read_buffer: FYPRT_BUF_TEMPORAL is written by fyprt_denoise_temporal");
            src = c->dt.hist[c->dtCur].p; n = c->dt.hist[c->dtCur].bytes(); break;
        case FYPRT_BUF_UPSCALE_GUIDE: case FYPRT_BUF_UPSCALE_ALBEDO:
            if (!c->upValid) return c->fail(FYPRT_ESTATE, "fyprt_read_buffer: FYPRT_BUF_UPSCALE_* are written by fyprt_denoise_upscale");
            src = which == FYPRT_BUF_UPSCALE_GUIDE ? c->up.guide.p : c->up.albedo.p;
            n = which == FYPRT_BUF_UPSCALE_GUIDE ? c->up.guide.bytes() : c->up.albedo.bytes(); break;
        default: return c->fail(FYPRT_EINVAL, "fyprt_read_buffer: unknown buffer");
    }
    if (which == FYPRT_BUF_GI_RESERVOIR || which == FYPRT_BUF_GI_PREV) {
        // the device keeps the 72-byte reservoirs padded to 80 aligned bytes (rt_device.h): hand out the reference layout
        const size_t npx = (size_t)c->W * c->H;
        std::vector<GIRes> rec(npx);
        HIPCHK(c, hipMemcpy(rec.data(), src, npx * sizeof(GIRes), hipMemcpyDeviceToHost));
        const size_t cnt = std::min(npx, bytes / kGIResBytes);
        for (size_t p = 0; p < cnt; ++p) std::memcpy((char*)dst + p * kGIResBytes, &rec[p], kGIResBytes);
        return FYPRT_OK;
    }
    if (c->lastTech == FYPRT_RESTIR_DI && (which == FYPRT_BUF_NORMAL || which == FYPRT_BUF_DI_RESERVOIR || which == FYPRT_BUF_DI_PREV)) {
        // ReSTIR DI keeps normal + reservoir packed in 32-byte records (DIRec); unpack into the reference layouts
        const size_t npx = (size_t)c->W * c->H;
        std::vector<DIRec> rec(npx);
        const DIRec* dsrc = (which == FYPRT_BUF_DI_PREV) ? (c->dprevFlip ? c->dprevB.p : c->dprevA.p) : c->drec.p;   // after the flip "read" = just written
        HIPCHK(c, hipMemcpy(rec.data(), dsrc, npx * sizeof(DIRec), hipMemcpyDeviceToHost));
        if (which == FYPRT_BUF_NORMAL) {
            std::vector<float> out(npx * 2);
            for (size_t p = 0; p < npx; ++p) { out[2 * p] = rec[p].nx; out[2 * p + 1] = rec[p].ny; }
            std::memcpy(dst, out.data(), std::min(bytes, out.size() * 4));
        } else {
            std::vector<DIRes> out(npx);
            for (size_t p = 0; p < npx; ++p) { out[p].index = rec[p].index; out[p].W = rec[p].W; out[p].pdf = rec[p].pdf; out[p].wSum = rec[p].wSum; out[p].M = rec[p].M; }
            std::memcpy(dst, out.data(), std::min(bytes, out.size() * sizeof(DIRes)));
        }
        return FYPRT_OK;
    }
    if (bytes > n) bytes = n;
    if (bytes) HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return FYPRT_OK;
}

int fyprt_reset_frame_index(fyprt_context* c) { if (!c) return FYPRT_EINVAL; c->frameIndex = 1; return FYPRT_OK; }
uint32_t fyprt_frame_index(const fyprt_context* c) { return c ? c->frameIndex : 0; }

int fyprt_export_bvh(fyprt_context* c, void* nodes64, uint32_t* node_count, void* tris48, uint32_t* tri_count, int32_t* root_ref, uint32_t* max_stack) {
    if (!c) return FYPRT_EINVAL;
    if (!c->haveScene) return c->fail(FYPRT_ESTATE, "fyprt_export_bvh before fyprt_upload_scene");
    if (c->hostBvhStale && !c->hostOnly) {              // the device refitted the tree: read it back
        HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c));
        TRY(download_nodes(c));
        if (!c->hostBvh.tris.empty()) HIPCHK(c, hipMemcpy(c->hostBvh.tris.data(), c->leafTris.p, c->hostBvh.tris.size() * 48, hipMemcpyDeviceToHost));
        c->hostBvhStale = false;
    }
    const rth::SceneBVH& b = c->hostBvh;
    if (nodes64) std::memcpy(nodes64, b.nodes.data(), b.nodes.size() * 64);
    if (tris48) std::memcpy(tris48, b.tris.data(), b.tris.size() * 48);
    if (node_count) *node_count = (uint32_t)b.nodes.size();
    if (tri_count) *tri_count = (uint32_t)b.tris.size();
    if (root_ref) *root_ref = b.rootRef;
    if (max_stack) *max_stack = b.levels;
    return FYPRT_OK;
}

int fyprt_export_lighttrees(fyprt_context* c, fyprt_lighttree_node* tlas, uint32_t* tlas_count, uint32_t* tlas_root, fyprt_lighttree_node* blas,
                            uint32_t* blas_total, uint32_t* blas_first, uint32_t* blas_count, uint32_t* blas_root) {
    if (!c) return FYPRT_EINVAL;
    if (!c->haveScene) return c->fail(FYPRT_ESTATE, "fyprt_export_lighttrees before fyprt_upload_scene");
    const rth::LightTrees& l = c->hostLt;
    if (tlas) std::memcpy(tlas, l.tlas.data(), l.tlas.size() * sizeof(fyprt_lighttree_node));
    if (blas) std::memcpy(blas, l.blas.data(), l.blas.size() * sizeof(fyprt_lighttree_node));
    if (tlas_count) *tlas_count = (uint32_t)l.tlas.size();
    if (tlas_root) *tlas_root = l.tlasRoot;
    if (blas_total) *blas_total = (uint32_t)l.blas.size();
    if (blas_first) std::memcpy(blas_first, l.first.data(), l.first.size() * 4);
    if (blas_count) std::memcpy(blas_count, l.count.data(), l.count.size() * 4);
    if (blas_root) std::memcpy(blas_root, l.root.data(), l.root.size() * 4);
    return FYPRT_OK;
}

int fyprt_get_tuning(fyprt_context* c, int key, int* value) {
    if (!c || !value || key < 0 || key >= K_COUNT) return FYPRT_EINVAL;
    *value = (key == K_STACK_BUDGET) ? stack_lds(c, 0u).budget : (key == K_WG_PER_CU && c->tuning[K_WG_PER_CU] <= 0) ? c->traceOcc.blocks : c->tuning[key];   // key 2: residency found at the last DI frame
    return FYPRT_OK;
}

int fyprt_set_tuning(fyprt_context* c, int key, int value) {
    if (!c || key < 0 || key >= K_COUNT) return FYPRT_EINVAL;
    // ranges: a value outside them could hang the persistent kernels (refill threshold above the wave size: no lane is ever
    // refilled) or index past a buffer, so it is refused here instead of trusted
    if (kTuning[key].max < 0) return c->fail(FYPRT_EINVAL, "fyprt_set_tuning: key " + std::to_string(key) + " is not assigned");
    if (value < 0 || value > kTuning[key].max)
        return c->fail(FYPRT_EINVAL, "fyprt_set_tuning: key " + std::to_string(key) + " accepts 0.." + std::to_string(kTuning[key].max));
    if (c->tuning[key] != value) c->drop_kept_primary();     // keys 7, 8 and 16 shape the traversal; no key changes in a still frame's steady state
    c->tuning[key] = value;
    return FYPRT_OK;
}

int fyprt_kept_primary_frames(fyprt_context* c, uint64_t* frames) { if (!c || !frames) return FYPRT_EINVAL; *frames = c->keptFrames; return FYPRT_OK; }
int fyprt_set_ray_counting(fyprt_context* c, int enabled) { if (!c) return FYPRT_EINVAL; c->countRays = enabled != 0; return FYPRT_OK; }

// The two parts of a ReSTIR frame as separate calls, for a host that moves the halo rows between the bands itself (part 1, then its
// own exchange of the buffers fyprt_multi.h lists, then part 2).  Asynchronous.
int fyprt_render_part(fyprt_context* c, const fyprt_settings* s, int part) {
    if (!c || !s || (part != 1 && part != 2)) return FYPRT_EINVAL;
    return enqueue_frame(c, s, true, part);
}

// ---- batched ray queries (rt_query.h).  A query reads the scene only and writes its own results and counters: no frame state moves.
static int check_query(fyprt_context* c, int query, const void* rays, uint32_t count, const void* results, bool device) {
    const char* who = device ? "fyprt_trace_rays_device" : "fyprt_trace_rays";
    if (!c) return FYPRT_EINVAL;
    if (query != FYPRT_QUERY_CLOSEST && query != FYPRT_QUERY_OCCLUDED) return c->fail(FYPRT_EINVAL, std::string(who) + ": unknown query kind");
    if (count && (!rays || !results)) return c->fail(FYPRT_EINVAL, std::string(who) + ": NULL rays / results with a non-zero count");
    if (device && (((uintptr_t)rays & 15u) || ((uintptr_t)results & 7u)))        // the kernels load rays as 16-byte quads, store 8-byte pairs
        return c->fail(FYPRT_EINVAL, std::string(who) + ": rays must be 16-byte and results 8-byte aligned");
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, std::string(who) + ": host-only context (device -1) cannot trace");
    if (!c->haveScene) return c->fail(FYPRT_ESTATE, std::string(who) + " before fyprt_upload_scene");
    return FYPRT_OK;
}
// `filterable`: a ray query proper, which the query filter applies to; the radiance queries' primary pass is not
static int enqueue_query(fyprt_context* c, int query, const float4* rays, uint32_t count, void* results, bool timed, bool filterable) {
    const int occluded = query == FYPRT_QUERY_OCCLUDED ? 1 : 0;
    static const QueryKernels<QueryRays> kQuery[2] = {query_kernels<ClosestLane>(), query_kernels<OccludedLane>()};
    QueryRays q{};
    q.rays = rays; q.results = results; q.count = count;
    // key 2 taken as it is, 4 workgroups per CU without an occupancy, the occupancy cached per kind
    return launch_query(c, c->rayQuery, occluded, q, kQuery[occluded], 0u, false, 4, timed, filterable);
}

int fyprt_trace_rays(fyprt_context* c, int query, const fyprt_ray* rays, uint32_t count, void* results, fyprt_frame_stats* stats) {
    TRY(check_query(c, query, rays, count, results, false));
    const HostQuery h{rays, 2, nullptr, results, (size_t)count * (query == FYPRT_QUERY_OCCLUDED ? 4u : 40u), nullptr, false};
    return run_host_query(c, c->rayQuery, h, count, stats, [&](const float4* in, const float4*, uint32_t* out, uint32_t*) {
        return enqueue_query(c, query, in, count, out, true, true); });
}

int fyprt_trace_rays_device(fyprt_context* c, int query, const void* rays, uint32_t count, void* results) {
    TRY(check_query(c, query, rays, count, results, true));
    if (count == 0) return FYPRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_query(c, query, static_cast<const float4*>(rays), count, results, false, true);
}

// ---- the list queries' entry points (ListQuery and its helpers, templates, stand before the extern "C" block)
int fyprt_trace_ray_hits(fyprt_context* c, const fyprt_ray* rays, const fyprt_ray_hit* after, uint32_t count, uint32_t max_hits, fyprt_ray_hit* hits,
                         uint32_t* hit_counts, fyprt_frame_stats* stats) {
    TRY(check_list_query(c, kRayHits, "fyprt_trace_ray_hits", rays, after, count, max_hits, hits, hit_counts, nullptr, false));
    return host_list_query(c, kRayHits, rays, after, count, max_hits, hits, hit_counts, nullptr, stats);
}
int fyprt_trace_ray_hits_device(fyprt_context* c, const void* rays, const void* after, uint32_t count, uint32_t max_hits, void* hits, void* hit_counts) {
    TRY(check_list_query(c, kRayHits, "fyprt_trace_ray_hits_device", rays, after, count, max_hits, hits, hit_counts, nullptr, true));
    return device_list_query(c, kRayHits, rays, after, count, max_hits, hits, hit_counts, nullptr);
}
int fyprt_nearest_points(fyprt_context* c, const fyprt_point* points, const fyprt_point_hit* after, uint32_t count, uint32_t max_hits, fyprt_point_hit* hits,
                         uint32_t* hit_counts, fyprt_frame_stats* stats) {
    TRY(check_list_query(c, kNearestPoints, "fyprt_nearest_points", points, after, count, max_hits, hits, hit_counts, nullptr, false));
    return host_list_query(c, kNearestPoints, points, after, count, max_hits, hits, hit_counts, nullptr, stats);
}
int fyprt_nearest_points_device(fyprt_context* c, const void* points, const void* after, uint32_t count, uint32_t max_hits, void* hits, void* hit_counts) {
    TRY(check_list_query(c, kNearestPoints, "fyprt_nearest_points_device", points, after, count, max_hits, hits, hit_counts, nullptr, true));
    return device_list_query(c, kNearestPoints, points, after, count, max_hits, hits, hit_counts, nullptr);
}

// ---- query filters (rt_filter.h): the mesh mask table and the query mask.  Host state only; the device data is built by the next
// filtered query (ensure_query_filter).  The table is replaced with the context stream idle: a build may still be copying the old one.
int fyprt_set_mesh_query_masks(fyprt_context* c, const uint32_t* masks, uint32_t mesh_count) {
    if (!c) return FYPRT_EINVAL;
    if ((masks == nullptr) != (mesh_count == 0)) return c->fail(FYPRT_EINVAL, "fyprt_set_mesh_query_masks: NULL masks with a non-zero count, or masks with count 0");
    if (!c->haveScene) return c->fail(FYPRT_ESTATE, "fyprt_set_mesh_query_masks before fyprt_upload_scene");
    if (mesh_count && mesh_count != (uint32_t)c->topoMeshes.size()) return c->fail(FYPRT_EINVAL, "fyprt_set_mesh_query_masks: mesh_count differs from the scene's mesh count");
    if (!c->hostOnly) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    c->meshMasks.assign(masks, masks + mesh_count);
    c->filterValid = false;
    if (!mesh_count) c->release_query_filter();
    return FYPRT_OK;
}
int fyprt_set_query_mask(fyprt_context* c, uint32_t query_mask) { if (!c) return FYPRT_EINVAL; c->queryMask = query_mask; return FYPRT_OK; }
int fyprt_get_query_filter(fyprt_context* c, uint32_t* masks, uint32_t* mesh_count, uint32_t* query_mask, uint64_t* builds) {
    if (!c || !mesh_count) return FYPRT_EINVAL;
    *mesh_count = (uint32_t)c->meshMasks.size();
    if (masks && !c->meshMasks.empty()) std::memcpy(masks, c->meshMasks.data(), c->meshMasks.size() * 4u);
    if (query_mask) *query_mask = c->queryMask;
    if (builds) *builds = c->filterBuilds;
    return FYPRT_OK;
}

// ---- box-overlap queries (rt_boxes.h): the list query whose entries are bare triangle indices, with a total beside the count
int fyprt_overlap_boxes(fyprt_context* c, const fyprt_box* boxes, const uint32_t* after, uint32_t count, uint32_t max_hits, uint32_t* triangles,
                        uint32_t* hit_counts, uint32_t* totals, fyprt_frame_stats* stats) {
    TRY(check_list_query(c, kOverlapBoxes, "fyprt_overlap_boxes", boxes, after, count, max_hits, triangles, hit_counts, totals, false));
    return host_list_query(c, kOverlapBoxes, boxes, after, count, max_hits, triangles, hit_counts, totals, stats);
}
int fyprt_overlap_boxes_device(fyprt_context* c, const void* boxes, const void* after, uint32_t count, uint32_t max_hits, void* triangles, void* hit_counts,
                               void* totals) {
    TRY(check_list_query(c, kOverlapBoxes, "fyprt_overlap_boxes_device", boxes, after, count, max_hits, triangles, hit_counts, totals, true));
    return device_list_query(c, kOverlapBoxes, boxes, after, count, max_hits, triangles, hit_counts, totals);
}

// ---- triangle-overlap queries (rt_triangles.h): the box query's walk and list around a triangle / triangle leaf test
int fyprt_overlap_triangles(fyprt_context* c, const fyprt_triangle* tris, const uint32_t* after, uint32_t count, uint32_t max_hits, uint32_t* triangles,
                            uint32_t* hit_counts, uint32_t* totals, fyprt_frame_stats* stats) {
    TRY(check_list_query(c, kOverlapTriangles, "fyprt_overlap_triangles", tris, after, count, max_hits, triangles, hit_counts, totals, false));
    return host_list_query(c, kOverlapTriangles, tris, after, count, max_hits, triangles, hit_counts, totals, stats);
}
int fyprt_overlap_triangles_device(fyprt_context* c, const void* tris, const void* after, uint32_t count, uint32_t max_hits, void* triangles, void* hit_counts,
                                   void* totals) {
    TRY(check_list_query(c, kOverlapTriangles, "fyprt_overlap_triangles_device", tris, after, count, max_hits, triangles, hit_counts, totals, true));
    return device_list_query(c, kOverlapTriangles, tris, after, count, max_hits, triangles, hit_counts, totals);
}

// ---- radiance queries (rt_query.h: k_render_rays_primary; rt_paths.h: the path stages with CAM = RaySource).  A frame's sample of
// techniques 0-6 for the caller's rays: the closest-hit query kernels trace the primary segments into the query's own payload records,
// k_render_rays_primary finishes what a frame's primary kernel finishes, run_stage runs the rest as it runs a frame's.  Everything it
// writes is its own (rr* buffers, the query counters): no frame state moves.
static int check_render_rays(fyprt_context* c, const fyprt_settings* s, uint32_t frameIndex, const void* rays, const void* indices, uint32_t count,
                             const void* radiance, const void* payloads, bool device) {
    const char* who = device ? "fyprt_render_rays_device" : "fyprt_render_rays";
    if (!c) return FYPRT_EINVAL;
    if (!s) return c->fail(FYPRT_EINVAL, std::string(who) + ": NULL settings");
    if (s->technique < 0 || s->technique > FYPRT_NEE) return c->fail(FYPRT_EINVAL, std::string(who) + ": techniques 0-6 only (ReSTIR is defined over screen-space neighbours and history)");
    if (frameIndex == 0) return c->fail(FYPRT_EINVAL, std::string(who) + ": frame_index must be >= 1");
    if (count && (!rays || !radiance)) return c->fail(FYPRT_EINVAL, std::string(who) + ": NULL rays / radiance with a non-zero count");
    if (device && (((uintptr_t)rays & 15u) || ((uintptr_t)radiance & 15u) || ((uintptr_t)payloads & 7u) || ((uintptr_t)indices & 3u)))
        return c->fail(FYPRT_EINVAL, std::string(who) + ": rays and radiance must be 16-byte, payloads 8-byte and indices 4-byte aligned");
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, std::string(who) + ": host-only context (device -1) cannot render");
    if (!c->haveScene) return c->fail(FYPRT_ESTATE, std::string(who) + " before fyprt_upload_scene");
    if ((s->technique == FYPRT_LIGHT_SOURCE_SAMPLING || s->technique == FYPRT_NEE) && (c->dsc.emissiveCount == 0 || c->dsc.ltTlasCount == 0))
        return c->fail(FYPRT_ENOLIGHT, std::string(who) + ": technique needs emissive triangles and a light tree");
    return FYPRT_OK;
}

// Enqueues one chunk (count <= FYPRT_RENDER_RAYS_CHUNK, device memory): primary pass, then the stages.  Buffers grow to the chunk and are kept.
static int enqueue_render_rays(fyprt_context* c, const fyprt_settings* s, uint32_t frameIndex, const float4* rays, const uint32_t* indices, uint32_t firstIndex,
                               uint32_t count, float4* radiance, void* payloads, hipMemcpyKind payloadKind, bool blocking, int* launched) {
    const int tech = s->technique;
    const DevSettings st = dev_settings(c, s);                   // as a frame's (techniques 0-6 read sky, bounces, samples and skipDeadRays only)
    const PathShape p = path_shape(tech, st);
    // buffers for the largest chunk so far, every technique (2 rays per entry, 6 quads of state); grown after the work that uses them
    if (c->rrPayload.n < count) {
        if (c->rrPayload.p) HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->rrPayload.alloc(count));
        for (int k = 0; k < 2; ++k) { HIPCHK(c, c->rrRays[k].alloc((size_t)count * 2 * 3)); HIPCHK(c, c->rrHits[k].alloc((size_t)count * 2)); }
        HIPCHK(c, c->rrState.alloc((size_t)count * 6)); HIPCHK(c, c->rrPixels.alloc(count)); HIPCHK(c, c->rrPixels2.alloc(count));
    }
    if (c->rrCounters.n < 3 * p.L) {
        if (c->rrCounters.p) HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, c->rrCounters.alloc(3 * p.L));
    }
    HIPCHK(c, hipMemsetAsync(c->rrCounters.p, 0, 3 * p.L * sizeof(uint32_t), c->stream));
    // primary segments: the closest-hit query (its own counters and queue head; ray counts of the whole call land there too)
    TRY(enqueue_query(c, FYPRT_QUERY_CLOSEST, rays, count, c->rrPayload.p, false, false));      // unfiltered: the query filter does not touch radiance queries
    ++*launched;
    const StackLds stack = stack_lds(c, 0u);
    DevScene qs = c->dsc; qs.stackBudget = stack.budget;        // (run_stage sets quorum and counters of its trace launches)
    DevFrame fr{};                                               // the step functions read the primary records and the frame index only
    fr.payload = c->rrPayload.p; fr.frameIndex = frameIndex; fr.W = 1u; fr.H = 1u;
    RaySource rs{rays, indices, firstIndex, radiance};
    const uint32_t pg = (uint32_t)std::max<size_t>(1, std::min<size_t>((size_t)c->numCUs * 16u, ((size_t)count + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(k_render_rays_primary, dim3(pg), dim3(kBlock), 0, c->stream, qs, rs, fr, st, count, c->rrPixels.p, c->rrCounters.p);
    ++*launched;
    HIPCHK(c, hipGetLastError());
    const StageBufs b{{c->rrRays[0].p, c->rrRays[1].p}, {c->rrHits[0].p, c->rrHits[1].p}, c->rrState.p, c->rrPixels.p, c->rrPixels2.p,
                      c->countRays ? c->rayQuery.counters.p : nullptr};
    TRY(run_stage(c, path_stage(tech, p, c->rrPixels.p, c->rrPixels2.p, c->rrCounters.p, count), b, qs, rs, fr, st, stack.bytes, blocking, launched));
    if (payloads) HIPCHK(c, hipMemcpyAsync(payloads, c->rrPayload.p, (size_t)count * sizeof(Payload), payloadKind, c->stream));
    return FYPRT_OK;
}

int fyprt_render_rays(fyprt_context* c, const fyprt_settings* s, uint32_t frame_index, const fyprt_ray* rays, const uint32_t* pixel_indices, uint32_t first_index,
                      uint32_t count, float* radiance4, void* payloads, fyprt_frame_stats* stats) {
    TRY(check_render_rays(c, s, frame_index, rays, pixel_indices, count, radiance4, payloads, false));
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (count == 0) return FYPRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (Event& e : c->rrEv) HIPCHK(c, create(e));
    const uint32_t chunkMax = std::min<uint32_t>(count, FYPRT_RENDER_RAYS_CHUNK);
    if (c->rrIn.n < (size_t)chunkMax * 2) { HIPCHK(c, c->rrIn.alloc((size_t)chunkMax * 2)); HIPCHK(c, c->rrOut.alloc(chunkMax)); }    // staging grows, is kept
    if (pixel_indices && c->rrIndices.n < chunkMax) HIPCHK(c, c->rrIndices.alloc(chunkMax));
    float ms = 0.0f; int launches = 0; unsigned long long totals[5] = {0, 0, 0, 0, 0};
    for (uint32_t base = 0; base < count; base += FYPRT_RENDER_RAYS_CHUNK) {
        const uint32_t n = std::min<uint32_t>(count - base, FYPRT_RENDER_RAYS_CHUNK);
        HIPCHK(c, hipMemcpyAsync(c->rrIn.p, rays + base, (size_t)n * sizeof(fyprt_ray), hipMemcpyHostToDevice, c->stream));
        if (pixel_indices) HIPCHK(c, hipMemcpyAsync(c->rrIndices.p, pixel_indices + base, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->rrEv[0], c->stream));
        TRY(enqueue_render_rays(c, s, frame_index, c->rrIn.p, pixel_indices ? c->rrIndices.p : nullptr, first_index + base, n, c->rrOut.p,
                                payloads ? static_cast<char*>(payloads) + (size_t)base * sizeof(Payload) : nullptr, hipMemcpyDeviceToHost, true, &launches));
        HIPCHK(c, hipEventRecord(c->rrEv[1], c->stream));
        HIPCHK(c, hipMemcpyAsync(radiance4 + (size_t)base * 4, c->rrOut.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float chunkMs = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&chunkMs, c->rrEv[0], c->rrEv[1]));
        ms += chunkMs;
        if (c->countRays) {
            unsigned long long r[5] = {0, 0, 0, 0, 0};
            HIPCHK(c, hipMemcpy(r, c->rayQuery.counters.p, sizeof r, hipMemcpyDeviceToHost));
            for (int k = 0; k < 5; ++k) totals[k] += r[k];
        }
    }
    if (stats) {
        stats->kernel_ms = ms; stats->kernel_ms_part[0] = ms; stats->launches = (uint32_t)launches;
        if (c->countRays) add_ray_stats(stats, 0, totals);
    }
    return FYPRT_OK;
}

int fyprt_render_rays_device(fyprt_context* c, const fyprt_settings* s, uint32_t frame_index, const void* rays, const uint32_t* pixel_indices, uint32_t first_index,
                             uint32_t count, void* radiance4, void* payloads) {
    TRY(check_render_rays(c, s, frame_index, rays, pixel_indices, count, radiance4, payloads, true));
    if (count == 0) return FYPRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int launches = 0;
    for (uint32_t base = 0; base < count; base += FYPRT_RENDER_RAYS_CHUNK) {
        const uint32_t n = std::min<uint32_t>(count - base, FYPRT_RENDER_RAYS_CHUNK);
        TRY(enqueue_render_rays(c, s, frame_index, static_cast<const float4*>(rays) + (size_t)base * 2, pixel_indices ? pixel_indices + base : nullptr,
                                first_index + base, n, static_cast<float4*>(radiance4) + base,
                                payloads ? static_cast<char*>(payloads) + (size_t)base * sizeof(Payload) : nullptr, hipMemcpyDeviceToDevice, false, &launches));
    }
    return FYPRT_OK;
}

// ---- denoiser (rt_denoise.h; the contract is include/fyprt.h's).  Reads the last frame's accumulation and payload, writes its own
// buffers and the caller's outputs: no frame state moves.
int fyprt_denoise_default_params(fyprt_denoise_params* out) {
    if (!out) return FYPRT_EINVAL;
    out->iterations = 5; out->sigma_luminance = 4.0f; out->sigma_plane = 0.01f; out->normal_power_log2 = 6; out->demodulate_albedo = 1;
    return FYPRT_OK;
}

// The checks of a denoise call in the header's order, in the pieces fyprt_group_denoise* (fyprt_multi.h) puts its own between:
// the parameters, the outputs, the frame.
static int check_denoise_params(fyprt_context* c, const char* who, const fyprt_denoise_params* p) {
    if (!p) return c->fail(FYPRT_EINVAL, std::string(who) + ": NULL params");
    if (p->iterations > 8u || p->normal_power_log2 > 7u || p->demodulate_albedo > 1u || !std::isfinite(p->sigma_luminance) ||
        !std::isfinite(p->sigma_plane) || !(p->sigma_plane > 0.0f))
        return c->fail(FYPRT_EINVAL, std::string(who) + ": iterations 0..8, normal_power_log2 0..7, demodulate_albedo 0 / 1, finite sigmas, sigma_plane > 0");
    return FYPRT_OK;
}
static int check_denoise_outputs(fyprt_context* c, const char* who, const void* rgba8, const void* radiance4, bool device) {
    if (device && (((uintptr_t)rgba8 & 3u) || ((uintptr_t)radiance4 & 15u)))
        return c->fail(FYPRT_EINVAL, std::string(who) + ": rgba8 must be 4-byte and radiance4 16-byte aligned");
    if (!rgba8 && !radiance4) return c->fail(FYPRT_EINVAL, std::string(who) + ": both outputs are NULL");
    return FYPRT_OK;
}
static int check_denoise_frame(fyprt_context* c, const char* who) {
    if (c->hostOnly) return c->fail(FYPRT_ESTATE, std::string(who) + ": host-only context (device -1) has no frame");
    if (c->W == 0 || !c->frameComplete || c->part1Pending)
        return c->fail(FYPRT_ESTATE, std::string(who) + ": no complete frame since the last fyprt_resize / fyprt_upload_scene / fyprt_update_vertices / fyprt_update_transforms");
    return FYPRT_OK;
}
static int check_denoise_rows(fyprt_context* c, const char* who) {
    if (c->comm || c->rowBegin != 0 || c->rowEnd != c->H || c->stripeRows != 0)
        return c->fail(FYPRT_ESTATE, std::string(who) + ": the context must render every row of the frame (no band, stripes, group or communicator)");
    return FYPRT_OK;
}
static int check_denoise(fyprt_context* c, const fyprt_denoise_params* p, const void* rgba8, const void* radiance4, bool device) {
    const char* who = device ? "fyprt_denoise_device" : "fyprt_denoise";
    if (!c) return FYPRT_EINVAL;
    TRY(check_denoise_params(c, who, p));
    TRY(check_denoise_outputs(c, who, rgba8, radiance4, device));
    TRY(check_denoise_frame(c, who));
    return check_denoise_rows(c, who);
}

extern "C++" {
// The iteration kernel of a step size: steps up to RT_DN_LDS_MAX_STEP run their LDS-staged instantiation, larger ones gather (<0>).
// `launch` is called with the instantiation's STEP as a std::integral_constant.
template <class F> static void for_dn_step(int step, F&& launch) {
    switch (step <= RT_DN_LDS_MAX_STEP ? step : 0) {
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 2: launch(std::integral_constant<int, 2>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        case 8: launch(std::integral_constant<int, 8>()); break;
        case 16: launch(std::integral_constant<int, 16>()); break;
        case 32: launch(std::integral_constant<int, 32>()); break;
        default: launch(std::integral_constant<int, 0>()); break;
    }
}

// The blocking form of a denoiser call: `n` output pixels staged on the device in outImg / outRad, `enqueue(rgba8, radiance4, &launches)`,
// copied back; the stats' parts are the times between the call's `nEv` timing events.
template <class Enqueue> static int staged_blocking(fyprt_context* c, size_t n, DevBuf<uint32_t>& outImg, DevBuf<float4>& outRad, uint32_t* rgba8, float* radiance4,
                                                    fyprt_frame_stats* stats, Event* ev, int nEv, Enqueue&& enqueue) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, sync_all(c));                           // as fyprt_readback: the last frame is complete on every stream
    for (int k = 0; k < nEv; ++k) HIPCHK(c, create(ev[k]));
    if (rgba8 && outImg.n != n) HIPCHK(c, outImg.alloc(n));
    if (radiance4 && outRad.n != n) HIPCHK(c, outRad.alloc(n));
    int launches = 0;
    TRY(enqueue(rgba8 ? outImg.p : nullptr, radiance4 ? outRad.p : nullptr, &launches));
    if (rgba8) HIPCHK(c, hipMemcpyAsync(rgba8, outImg.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (radiance4) HIPCHK(c, hipMemcpyAsync(radiance4, outRad.p, n * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (stats) {
        stats->launches = (uint32_t)launches;
        for (int k = 0; k + 1 < nEv; ++k) { HIPCHK(c, hipEventElapsedTime(&stats->kernel_ms_part[k], ev[k], ev[k + 1])); stats->kernel_ms += stats->kernel_ms_part[k]; }
    }
    return FYPRT_OK;
}
// ... of either denoiser at the rendered size: width x height pixels through the denoiser's own staging
template <class Enqueue> static int denoise_blocking(fyprt_context* c, uint32_t* rgba8, float* radiance4, fyprt_frame_stats* stats, Event* ev, int nEv, Enqueue&& enqueue) {
    return staged_blocking(c, (size_t)c->W * c->H, c->dn.outImg, c->dn.outRad, rgba8, radiance4, stats, ev, nEv, enqueue);
}
}  // extern "C++"

// ---- what fyprt_denoise*, fyprt_denoise_temporal* and fyprt_group_denoise* (fyprt_multi.h) enqueue with.
// Iteration k.  scaled: sigma_luminance / 2^k (spatial); otherwise sigma_luminance itself (temporal: the variance carries the scale).
// keep: the last iteration writes its colour buffer as every other one does, not the outputs.
static DnIter make_dn_iter(const fyprt_denoise_params& p, uint32_t k, bool scaled, bool keep) {
    return DnIter{1 << k, scaled ? p.sigma_luminance * (1.0f / (float)(1u << k)) : p.sigma_luminance, p.sigma_luminance > 0.0f ? 1u : 0u,
                  p.sigma_plane, p.normal_power_log2, (!keep && k + 1 == p.iterations) ? 1u : 0u};
}
// The full-size guide, albedo and ping-pong colour buffers of a context and its dnDone event; the frame descriptor over them.
static int ensure_dn_buffers(fyprt_context* c) {
    const size_t n = (size_t)c->W * c->H;
    if (c->dn.guide.n != 2 * n) {
        HIPCHK(c, c->dn.guide.alloc(2 * n)); HIPCHK(c, c->dn.albedo.alloc(n)); HIPCHK(c, c->dn.col[0].alloc(n)); HIPCHK(c, c->dn.col[1].alloc(n));
    }
    HIPCHK(c, create(c->dnDone, hipEventDisableTiming));
    return FYPRT_OK;
}
static DnFrame dn_frame(const fyprt_context* c, uint32_t demodulate, uint32_t* rgba8, float4* radiance4) {
    return DnFrame{c->W, c->H, (float)c->lastFrameIndex, demodulate, c->accum.p, c->dn.guide.p, c->dn.albedo.p, rgba8, radiance4};
}
static dim3 dn_pixel_grid(const DnFrame& fr, DnBand band) { return dim3((uint32_t)(((size_t)(band.rowEnd - band.rowBegin) * fr.W + 255u) / 256u)); }
// One launch each on the context stream, on the rows of `band` (the whole frame: {0, H}); prepare writes dn.col[0].
static void launch_dn_prepare(fyprt_context* c, const DnFrame& fr, DnBand band) {
    DevScene sc = c->dsc; sc.rayCounter = nullptr;
    hipLaunchKernelGGL(k_dn_prepare, dn_pixel_grid(fr, band), dim3(256), 0, c->stream, sc, fr, band, c->payload.p, c->dn.col[0].p);
}
static void launch_dn_iterate(fyprt_context* c, const DnFrame& fr, const DnIter& it, DnBand band, const float4* in, float4* out) {
    for_dn_step(it.step, [&](auto S) {
        constexpr int STEP = decltype(S)::value;
        hipLaunchKernelGGL(k_dn_iterate<STEP>, dim3(dn_grid<STEP>(fr.W, band.rowEnd - band.rowBegin)), dim3(256), 0, c->stream, fr, it, band, in, out);
    });
}
static void launch_dn_finish(fyprt_context* c, const DnFrame& fr, DnBand band, const float4* col) {
    hipLaunchKernelGGL(k_dn_finish, dn_pixel_grid(fr, band), dim3(256), 0, c->stream, fr, band, col);
}
// What every call ends with on a context, after its last kernel: dnDone — a pipelined ReSTIR DI frame enqueued next runs its Part 1 on
// the front stream, which overwrites the payload: after the denoiser.
static int dn_call_done(fyprt_context* c) {
    HIPCHK(c, hipEventRecord(c->dnDone, c->stream));
    if (c->front) HIPCHK(c, hipStreamWaitEvent(c->front, c->dnDone, 0));
    c->albedoValid = true;
    return FYPRT_OK;
}

// ---- A filter call is a list of steps, stated once per filter (spatial_steps, temporal_steps, upscale_steps) and run by filter_enqueue
// on one context or by group_filter_enqueue (fyprt_multi.h) on a group's bands.  A step pulls a stage of the group's plan, launches, or both.
struct XBuf { void* p; size_t bytesPerPixel; };
constexpr size_t kDnGuideBytes = 2 * sizeof(float4), kDnColourBytes = sizeof(float4), kDtHistoryBytes = 4 * sizeof(float4), kDtVarianceBytes = sizeof(float);
struct BandStep {
    int pulls;                                                        // the plan stage every band pulls before the launch, or -1,
    std::function<std::vector<XBuf>(fyprt_context*)> moved;           // and the buffers it moves: the receiver's and, in the same order, the owner's
    bool overwritesPulled;                                            // the launch overwrites rows the neighbours pulled earlier
    bool writesOutput;                                                // the launch writes the output rows
    std::function<bool(fyprt_context*, const DnFrame&, DnBand)> launch;      // on a band's rows, on its context's stream: whether a kernel was launched; empty: the step only pulls
    bool recordsDone;                                                 // `done` is recorded after the launch: a pull reads what it wrote
    int part;                                                         // the kernel_ms_part of a context's blocking call the launch counts in
};
// (a launch captures at most 16 bytes — the parameters by address: they outlive the list — so that no step allocates)
// The single-context runner: every launch of the list on the band [0, H) (a hi-res step scales it itself); what only concerns neighbours,
// the pulls and their events, is skipped.  ev: the blocking form's timing events and launch count, or null — ev[k] where part k begins, one more at the end.
static int filter_enqueue(fyprt_context* c, const std::vector<BandStep>& steps, uint32_t demodulate, uint32_t* rgba8, float4* radiance4, const Event* ev, int* launched) {
    const DnFrame fr = dn_frame(c, demodulate, rgba8, radiance4);
    int part = 0;
    if (ev) HIPCHK(c, hipEventRecord(ev[0], c->stream));
    for (const BandStep& st : steps) {
        if (!st.launch) continue;
        if (ev && st.part != part) HIPCHK(c, hipEventRecord(ev[part = st.part], c->stream));
        if (st.launch(c, fr, DnBand{0, c->H}) && launched) ++*launched;
    }
    HIPCHK(c, hipGetLastError());
    if (ev) HIPCHK(c, hipEventRecord(ev[part + 1], c->stream));
    return dn_call_done(c);
}
// What both denoisers start with: prepare on the band's rows (into dn.col[0]), then the guide records of the halo rows (stage 0) ...
static std::vector<BandStep> first_steps() {
    std::vector<BandStep> steps;
    steps.reserve(16);                                                // (the longest list: 8 iterations and 8 other steps)
    steps.push_back({-1, nullptr, false, false, [](fyprt_context* c, const DnFrame& fr, DnBand band) { launch_dn_prepare(c, fr, band); return true; }, true, 0});
    steps.push_back({0, [](fyprt_context* c) { return std::vector<XBuf>{{c->dn.guide.p, kDnGuideBytes}}; }, false, false, nullptr, false, 0});
    return steps;
}
// ... and, without iterations, end with: the finish kernel on the unfiltered colour dn.col[col]
static BandStep finish_step(int col, int part) {
    return {-1, nullptr, false, true, [col](fyprt_context* c, const DnFrame& fr, DnBand band) { launch_dn_finish(c, fr, band, c->dn.col[col].p); return true; }, true, part};
}

// The spatial filter (the group's plan: group_denoise_plan): prepare; the guides; per iteration k the colour halo it reads (stage 1 + k:
// dn.col[k & 1]) and the iteration dn.col[k & 1] -> dn.col[(k + 1) & 1]; without an iteration the finish kernel on dn.col[0].  Iteration 0
// waits for no puller: it writes dn.col[1], which nothing pulled yet.  Parts: prepare | the iterations or the finish kernel.
// keep (the low-res stage of the upscaler): the list stops before the output — the last iteration writes its colour buffer as every
// other one does (DnIter::last = 0), no finish kernel — and *keep is the index of the dn.col that holds e.
static std::vector<BandStep> spatial_steps(const fyprt_denoise_params& p, int* keep = nullptr) {
    std::vector<BandStep> steps = first_steps();
    const fyprt_denoise_params* pp = &p;
    const bool kept = keep != nullptr;
    for (uint32_t k = 0; k < p.iterations; ++k)
        steps.push_back({1 + (int)k, [k](fyprt_context* c) { return std::vector<XBuf>{{c->dn.col[k & 1u].p, kDnColourBytes}}; }, k > 0, !kept && k + 1 == p.iterations,
                         [pp, k, kept](fyprt_context* c, const DnFrame& fr, DnBand band) {
                             launch_dn_iterate(c, fr, make_dn_iter(*pp, k, true, kept), band, c->dn.col[k & 1u].p, c->dn.col[(k + 1u) & 1u].p);
                             return true;
                         }, true, 1});
    if (kept) *keep = (int)(p.iterations & 1u);
    else if (p.iterations == 0) steps.push_back(finish_step(0, 1));
    return steps;
}

// One spatial call on a context, outputs in device memory.  ev, launched: 3 timing events and the launch count of the blocking form, or null.
static int denoise_call(fyprt_context* c, const fyprt_denoise_params* p, uint32_t* rgba8, float4* radiance4, const Event* ev, int* launched) {
    TRY(ensure_dn_buffers(c));
    return filter_enqueue(c, spatial_steps(*p), p->demodulate_albedo, rgba8, radiance4, ev, launched);
}

int fyprt_denoise(fyprt_context* c, const fyprt_denoise_params* p, uint32_t* rgba8, float* radiance4, fyprt_frame_stats* stats) {
    TRY(check_denoise(c, p, rgba8, radiance4, false));
    return denoise_blocking(c, rgba8, radiance4, stats, c->dnEv, 3,      // parts: prepare, the iterations (or the finish kernel)
                            [&](uint32_t* img, float4* rad, int* launched) { return denoise_call(c, p, img, rad, c->dnEv, launched); });
}

int fyprt_denoise_device(fyprt_context* c, const fyprt_denoise_params* p, void* rgba8, void* radiance4) {
    TRY(check_denoise(c, p, rgba8, radiance4, true));
    HIPCHK(c, hipSetDevice(c->device));
    // every frame completes on the context stream (a pipelined frame's trace kernel waits there for its front part), so work enqueued on
    // it sees the last frame whole without a host wait
    return denoise_call(c, p, static_cast<uint32_t*>(rgba8), static_cast<float4*>(radiance4), nullptr, nullptr);
}

// ---- temporal denoiser (rt_temporal.h; the contract is include/fyprt.h's).  As the spatial one it reads the last frame's accumulation
// and payload and moves no frame state; what it keeps between calls is its own history.
int fyprt_denoise_temporal_default_params(fyprt_temporal_params* out) {
    if (!out) return FYPRT_EINVAL;
    fyprt_denoise_default_params(&out->spatial);
    out->history_limit = 32; out->normal_min = 0.9f; out->plane_max = 0.02f; out->feedback = 1;
    return FYPRT_OK;
}

// The temporal part of the parameters (the spatial part: check_denoise_params); fyprt_group_denoise_temporal* (fyprt_multi.h) shares it.
static int check_temporal_params(fyprt_context* c, const char* who, const fyprt_temporal_params* p) {
    if (!p) return c->fail(FYPRT_EINVAL, std::string(who) + ": NULL params");
    if (p->history_limit < 1u || p->history_limit > 256u || p->feedback > 1u || !std::isfinite(p->normal_min) || !std::isfinite(p->plane_max) ||
        !(p->plane_max > 0.0f))
        return c->fail(FYPRT_EINVAL, std::string(who) + ": history_limit 1..256, feedback 0 / 1, finite normal_min, finite plane_max > 0");
    return FYPRT_OK;
}
static int check_temporal(fyprt_context* c, const fyprt_temporal_params* p, const void* rgba8, const void* radiance4, bool device) {
    const char* who = device ? "fyprt_denoise_temporal_device" : "fyprt_denoise_temporal";
    if (!c) return FYPRT_EINVAL;
    TRY(check_temporal_params(c, who, p));
    const int rc = check_denoise(c, &p->spatial, rgba8, radiance4, device);
    if (rc != FYPRT_OK) c->err = std::string(who) + " (as fyprt_denoise): " + c->err;
    return rc;
}

// One iteration of the temporal form on the rows of `band`, on the context stream
static void launch_dt_iterate(fyprt_context* c, const DnFrame& fr, const DnIter& it, DnBand band, const float4* in, float4* out, const float* vin,
                              float* vout, float4* fb) {
    for_dn_step(it.step, [&](auto S) {
        constexpr int STEP = decltype(S)::value;
        hipLaunchKernelGGL(k_dt_iterate<STEP>, dim3(dn_grid<STEP>(fr.W, band.rowEnd - band.rowBegin)), dim3(256), 0, c->stream, fr, it, band, in, out, vin, vout, fb);
    });
}
// Object motion is at work in a call: there is a history to reproject, and a vertex snapshot with an edited range is pending.
static bool dt_motion_pending(const fyprt_context* c, bool history) { return history && c->dtSnapPending && c->dtEditHi > c->dtEditLo; }
// The moved flags of the edited range (only while dt_motion_pending), on the context stream
static void launch_dt_moved(fyprt_context* c) {
    const uint32_t count = c->dtEditHi - c->dtEditLo;
    hipLaunchKernelGGL(k_dt_moved, dim3((count + 255u) / 256u), dim3(256), 0, c->stream, c->dverts.p, c->dtSnap.p, c->triIdx.p, c->dtMoved.p, c->dtEditLo, count);
}
// The reprojection on the rows of `band`, its history taps within `window` (the whole frame: both {0, H}), in its motion form after
// launch_dt_moved: dn.col[0] and dt.hist[dtCur] -> dt.hist[dtCur ^ 1], dn.col[1], dt.var[0]
static void launch_dt_reproject(fyprt_context* c, const DnFrame& fr, const DtCall& tc, DnBand band, DnBand window, bool motion) {
    const dim3 grid(dt_reproject_grid(fr.W, band.rowEnd - band.rowBegin));
    const float4* histIn = c->dt.hist[c->dtCur].p; float4* histOut = c->dt.hist[c->dtCur ^ 1].p;
    if (motion) {
        const DtMotion mo{c->payload.p, c->dtMoved.p, c->triIdx.p, c->triPos.p, c->dtSnap.p};
        hipLaunchKernelGGL(k_dt_reproject_motion, grid, dim3(256), 0, c->stream, fr, tc, mo, band, window, c->dn.col[0].p, histIn, histOut, c->dn.col[1].p, c->dt.var[0].p);
    } else {
        hipLaunchKernelGGL(k_dt_reproject, grid, dim3(256), 0, c->stream, fr, tc, band, window, c->dn.col[0].p, histIn, histOut, c->dn.col[1].p, c->dt.var[0].p);
    }
}
// The history and variance buffers of a context (a new size drops the history)
static int ensure_dt_buffers(fyprt_context* c) {
    const size_t n = (size_t)c->W * c->H;
    if (c->dt.hist[0].n != 4 * n) {
        c->drop_history();
        for (int k = 0; k < 2; ++k) { HIPCHK(c, c->dt.hist[k].alloc(4 * n)); HIPCHK(c, c->dt.var[k].alloc(n)); }
    }
    return FYPRT_OK;
}

static DtCall make_dt_call(const fyprt_context* c, const fyprt_temporal_params& p, bool haveHistory) {
    DtCall tc{};
    std::memcpy(tc.m, c->dtPV, 64);
    tc.haveHistory = haveHistory ? 1u : 0u; tc.limit = (float)p.history_limit; tc.normalMin = p.normal_min; tc.planeMax = p.plane_max;
    tc.sigmaPlane = p.spatial.sigma_plane; tc.normalPow = p.spatial.normal_power_log2;
    return tc;
}

// The temporal filter (the group's plan: group_temporal_plan, without stage 2 while there is no history): prepare; the guides; the
// prepared colour the variance estimate reads (stage 1); with a history the moved flags of a pending edit — launched only while
// dt_motion_pending, and nothing pulls what they are, so no `done` — and the history window (stage 2: dt.hist[dtCur]); the reprojection,
// its taps within the band plus R rows either side, clipped to the frame (a context alone: R = H); per iteration k the colour and
// variance it reads (stage 3 + k) and the iteration, colour dn.col[1] -> [0] -> [1] ..., variance dt.var[0] -> [1] -> [0] ..., iteration 0
// feeding dt.hist[dtCur ^ 1] back; without an iteration the finish kernel on the integrated colour dn.col[1].  Every iteration waits
// for its pullers: iteration 0 overwrites the prepared colour of stage 1.  Parts: prepare | moved flags + reprojection | the iterations
// or the finish kernel.  keep: as spatial_steps' — the history advances as in any temporal call.  The callers advance the
// bookkeeping (dt_advance) once everything is enqueued: the launches read dtCur as it was.
static std::vector<BandStep> temporal_steps(const fyprt_temporal_params& p, bool history, uint32_t R, int* keep = nullptr) {
    std::vector<BandStep> steps = first_steps();
    const fyprt_temporal_params* pp = &p;
    const fyprt_denoise_params& sp = p.spatial;
    const bool kept = keep != nullptr;
    steps.push_back({1, [](fyprt_context* c) { return std::vector<XBuf>{{c->dn.col[0].p, kDnColourBytes}}; }, false, false, nullptr, false, 1});
    if (history) {
        steps.push_back({-1, nullptr, false, false, [](fyprt_context* c, const DnFrame&, DnBand) {
            if (!dt_motion_pending(c, true)) return false;
            launch_dt_moved(c);
            return true;
        }, false, 1});
        steps.push_back({2, [](fyprt_context* c) { return std::vector<XBuf>{{c->dt.hist[c->dtCur].p, kDtHistoryBytes}}; }, false, false, nullptr, false, 1});
    }
    steps.push_back({-1, nullptr, false, false, [pp, R, history](fyprt_context* c, const DnFrame& fr, DnBand band) {
        const DnBand window{band.rowBegin > R ? band.rowBegin - R : 0u, std::min(fr.H, band.rowEnd + R)};
        launch_dt_reproject(c, fr, make_dt_call(c, *pp, history), band, window, dt_motion_pending(c, history));
        return true;
    }, true, 1});
    for (uint32_t k = 0; k < sp.iterations; ++k)
        steps.push_back({3 + (int)k, [k](fyprt_context* c) { return std::vector<XBuf>{{c->dn.col[(k + 1u) & 1u].p, kDnColourBytes}, {c->dt.var[k & 1u].p, kDtVarianceBytes}}; },
                         true, !kept && k + 1 == sp.iterations,
                         [pp, k, kept](fyprt_context* c, const DnFrame& fr, DnBand band) {
                             launch_dt_iterate(c, fr, make_dn_iter(pp->spatial, k, false, kept), band, c->dn.col[(k + 1u) & 1u].p, c->dn.col[k & 1u].p, c->dt.var[k & 1u].p,
                                               c->dt.var[(k + 1u) & 1u].p, (k == 0 && pp->feedback) ? c->dt.hist[c->dtCur ^ 1].p : nullptr);
                             return true;
                         }, true, 2});
    if (kept) *keep = (int)((sp.iterations + 1u) & 1u);      // (iteration k writes col[k & 1]; none: the integrated colour in col[1])
    else if (sp.iterations == 0) steps.push_back(finish_step(1, 2));
    return steps;
}
// After a temporal list is enqueued: the history it wrote is the current one, written by `group` (0: by the context alone)
static void dt_advance(fyprt_context* c, uint64_t group) {
    c->dtCur ^= 1; c->dtValid = true; c->dtGroup = group; c->dtSnapPending = false; std::memcpy(c->dtPV, c->framePV, 64);
}

// One temporal call on a context, outputs in device memory.  ev, launched: 4 timing events and the launch count of the blocking form, or null.
static int temporal_call(fyprt_context* c, const fyprt_temporal_params* p, uint32_t* rgba8, float4* radiance4, const Event* ev, int* launched) {
    TRY(ensure_dt_buffers(c));
    if (c->dtGroup != 0) c->drop_history();      // a history a group wrote (fyprt_group_denoise_temporal*) covers the rows the context owned there
    TRY(ensure_dn_buffers(c));
    TRY(filter_enqueue(c, temporal_steps(*p, c->dtValid, c->H), p->spatial.demodulate_albedo, rgba8, radiance4, ev, launched));
    dt_advance(c, 0);
    return FYPRT_OK;
}

int fyprt_denoise_temporal(fyprt_context* c, const fyprt_temporal_params* p, uint32_t* rgba8, float* radiance4, fyprt_frame_stats* stats) {
    TRY(check_temporal(c, p, rgba8, radiance4, false));
    return denoise_blocking(c, rgba8, radiance4, stats, c->dtEv, 4,      // parts: prepare, reproject, iterations
                            [&](uint32_t* img, float4* rad, int* launched) { return temporal_call(c, p, img, rad, c->dtEv, launched); });
}

int fyprt_denoise_temporal_device(fyprt_context* c, const fyprt_temporal_params* p, void* rgba8, void* radiance4) {
    TRY(check_temporal(c, p, rgba8, radiance4, true));
    HIPCHK(c, hipSetDevice(c->device));
    return temporal_call(c, p, static_cast<uint32_t*>(rgba8), static_cast<float4*>(radiance4), nullptr, nullptr);
}

int fyprt_denoise_temporal_reset(fyprt_context* c) {
    if (!c) return FYPRT_EINVAL;
    c->drop_history();
    return FYPRT_OK;
}

int fyprt_denoise_temporal_set_motion(fyprt_context* c, int enabled) {
    if (!c) return FYPRT_EINVAL;
    if (enabled != 0 && enabled != 1) return c->fail(FYPRT_EINVAL, "fyprt_denoise_temporal_set_motion: enabled must be 0 or 1");
    if (c->dtMotion == (enabled == 1)) return FYPRT_OK;
    if (!c->hostOnly && c->dtSnap.p) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c)); }     // a call in flight may read the snapshot
    c->dtMotion = enabled == 1;
    c->drop_history(); c->release_snapshot();
    return FYPRT_OK;
}

// ---- upscaler (rt_upscale.h; the contract is include/fyprt.h's).  The low-res stage of either denoiser, hi-res primary rays, the resolve.
int fyprt_upscale_default_params(fyprt_upscale_params* out) {
    if (!out) return FYPRT_EINVAL;
    out->scale = 2; out->temporal = 0;
    return fyprt_denoise_temporal_default_params(&out->filter);
}

// The parameter cases of an upscale call in the header's order; fyprt_group_denoise_upscale* (fyprt_multi.h) shares them.
static int check_upscale_params(fyprt_context* c, const char* who, const fyprt_upscale_params* p) {
    if (!p) return c->fail(FYPRT_EINVAL, std::string(who) + ": NULL params");
    if (p->scale < 2u || p->scale > 4u || p->temporal > 1u) return c->fail(FYPRT_EINVAL, std::string(who) + ": scale 2..4, temporal 0 / 1");
    if (p->temporal) TRY(check_temporal_params(c, who, &p->filter));
    if ((uint64_t)c->W * p->scale * ((uint64_t)c->H * p->scale) > (1ull << 31))
        return c->fail(FYPRT_EINVAL, std::string(who) + ": scale*width x scale*height is beyond what fyprt_resize accepts");
    return check_denoise_params(c, who, &p->filter.spatial);
}
static int check_upscale(fyprt_context* c, const fyprt_upscale_params* p, const void* rgba8, const void* radiance4, bool device) {
    const char* who = device ? "fyprt_denoise_upscale_device" : "fyprt_denoise_upscale";
    if (!c) return FYPRT_EINVAL;
    TRY(check_upscale_params(c, who, p));
    TRY(check_denoise_outputs(c, who, rgba8, radiance4, device));
    TRY(check_denoise_frame(c, who));
    return check_denoise_rows(c, who);
}

// The hi-res buffers for scale s.  Another scale than the last call's: that call may still be writing the old ones on the context stream
static int ensure_up_buffers(fyprt_context* c, uint32_t s) {
    const size_t n = (size_t)c->W * s * ((size_t)c->H * s);
    if (c->upScale != s || c->up.albedo.n != n) {
        if (c->up.albedo.p) HIPCHK(c, hipStreamSynchronize(c->stream));
        c->release_upscale();
        HIPCHK(c, c->up.guide.alloc(2 * n)); HIPCHK(c, c->up.albedo.alloc(n));
        c->upScale = s;
    }
    return FYPRT_OK;
}

// One launch each on the context stream, on the hi-res rows of `band` (the whole frame: {0, s H}).  k_up_primary: the frame's camera on
// the hi-res viewport; the scene as a frame's primary rays read it (key 7's quorum, the tree's stack budget), no ray counters.
static void launch_up_primary(fyprt_context* c, uint32_t s, DnBand band) {
    DevCamera cam = c->frameCam; cam.W = c->W * s; cam.H = c->H * s;
    const StackLds stack = stack_lds(c, 0u);
    DevScene sc = secondary_scene(c->dsc, (uint32_t)c->tuning[K_QUORUM_PRIMARY], nullptr);
    sc.stackBudget = stack.budget; sc.topCount = 0u;
    const uint32_t order = (uint32_t)c->tuning[K_TILE_ORDER];
    hipLaunchKernelGGL(k_up_primary, dim3(up_primary_grid(cam.W, band.rowEnd - band.rowBegin, order)), dim3(kBlock), stack.bytes, c->stream, sc, cam, order, c->frameSky,
                       band, c->up.guide.p, c->up.albedo.p);
}
// k_up_resolve: e = the low-res colour buffer after the last iteration; rgba8 / radiance4 = where row 0 of the hi-res outputs is (or would be)
static void launch_up_resolve(fyprt_context* c, const fyprt_denoise_params& sp, uint32_t s, const float4* e, uint32_t* rgba8, float4* radiance4, DnBand band) {
    const UpFrame fr{c->W, c->H, (float)c->lastFrameIndex, sp.demodulate_albedo, sp.sigma_plane, sp.normal_power_log2, c->accum.p, c->dn.guide.p,
                     c->dn.albedo.p, e, c->up.guide.p, c->up.albedo.p, rgba8, radiance4};
    const dim3 rgrid(up_resolve_grid(c->W * s, band.rowEnd - band.rowBegin));
    switch (s) {
        case 2: hipLaunchKernelGGL(k_up_resolve<2>, rgrid, dim3(256), 0, c->stream, fr, band); break;
        case 3: hipLaunchKernelGGL(k_up_resolve<3>, rgrid, dim3(256), 0, c->stream, fr, band); break;
        default: hipLaunchKernelGGL(k_up_resolve<4>, rgrid, dim3(256), 0, c->stream, fr, band); break;
    }
}

// The upscaler at scale s: the low-res stage — either filter's list in its keep form, the colour e left in dn.col[col] —, then
//   k_up_primary on the band's hi-res rows.  It reads the scene and the frame's camera only, so it may stand anywhere before the
//   resolve; after the last iteration it runs, on a group, while the neighbour below finishes its last iteration, whose `done` the pull
//   after it waits for — the one wait of the call that nothing else of the band's own could fill.  primaryEarly (the group's
//   FYPRT_UP_PRIMARY_EARLY, fyprt_multi.h) puts it directly after prepare instead.  A launch-only step: it pulls nothing and records no
//   `done`, because nothing pulls from it;
//   then the pull of the plan's last stage (group_upscale_plan) — row e of dn.col[col], and its guide record where the plan has no
//   stage 0 (spatial without an iteration) — and k_up_resolve on the band's hi-res rows, which writes the output rows and records `done`.
// Parts: the low-res stage | k_up_primary | k_up_resolve.
static std::vector<BandStep> upscale_steps(const fyprt_upscale_params& p, bool history, uint32_t R, bool primaryEarly) {
    const fyprt_denoise_params* sp = &p.filter.spatial;
    const uint32_t s = p.scale;
    int col = 0;
    std::vector<BandStep> steps = p.temporal ? temporal_steps(p.filter, history, R, &col) : spatial_steps(*sp, &col);
    for (BandStep& st : steps) st.part = 0;
    const bool withGuide = !p.temporal && sp->iterations == 0;
    steps.insert(primaryEarly ? steps.begin() + 1 : steps.end(), BandStep{-1, nullptr, false, false, [s](fyprt_context* c, const DnFrame&, DnBand band) {
        launch_up_primary(c, s, DnBand{band.rowBegin * s, band.rowEnd * s});
        return true;
    }, false, 1});
    steps.push_back({(p.temporal ? 3 : 1) + (int)sp->iterations, [col, withGuide](fyprt_context* c) {
        std::vector<XBuf> v{{c->dn.col[col].p, kDnColourBytes}};
        if (withGuide) v.push_back({c->dn.guide.p, kDnGuideBytes});
        return v;
    }, false, true, [sp, s, col](fyprt_context* c, const DnFrame& fr, DnBand band) {
        launch_up_resolve(c, *sp, s, c->dn.col[col].p, fr.rgba8, fr.radiance4, DnBand{band.rowBegin * s, band.rowEnd * s});
        return true;
    }, true, 2});
    return steps;
}

// One upscale call on a context (after ensure_up_buffers), outputs in device memory.  ev, launched: 4 timing events and the launch count of the blocking form, or null.
static int upscale_call(fyprt_context* c, const fyprt_upscale_params* p, uint32_t* rgba8, float4* radiance4, const Event* ev, int* launched) {
    if (p->temporal) {
        TRY(ensure_dt_buffers(c));
        if (c->dtGroup != 0) c->drop_history();      // (as temporal_call)
    }
    TRY(ensure_dn_buffers(c));
    TRY(filter_enqueue(c, upscale_steps(*p, c->dtValid, c->H, false), p->filter.spatial.demodulate_albedo, rgba8, radiance4, ev, launched));
    if (p->temporal) dt_advance(c, 0);
    c->upValid = true;
    return FYPRT_OK;
}

int fyprt_denoise_upscale(fyprt_context* c, const fyprt_upscale_params* p, uint32_t* rgba8, float* radiance4, fyprt_frame_stats* stats) {
    TRY(check_upscale(c, p, rgba8, radiance4, false));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_up_buffers(c, p->scale));
    const size_t n = (size_t)c->W * p->scale * ((size_t)c->H * p->scale);
    return staged_blocking(c, n, c->up.outImg, c->up.outRad, rgba8, radiance4, stats, c->upEv, 4,      // parts: the low-res stage, the hi-res primary rays, the resolve
                           [&](uint32_t* img, float4* rad, int* launched) { return upscale_call(c, p, img, rad, c->upEv, launched); });
}

int fyprt_denoise_upscale_device(fyprt_context* c, const fyprt_upscale_params* p, void* rgba8, void* radiance4) {
    TRY(check_upscale(c, p, rgba8, radiance4, true));
    HIPCHK(c, hipSetDevice(c->device));
    TRY(ensure_up_buffers(c, p->scale));
    return upscale_call(c, p, static_cast<uint32_t*>(rgba8), static_cast<float4*>(radiance4), nullptr, nullptr);
}

#include "fyprt_multi.h"

}  // extern "C"
