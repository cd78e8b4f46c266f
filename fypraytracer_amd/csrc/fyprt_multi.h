// Multi-GPU layer of the C ABI (include/fyprt.h, "multi-GPU" section) — included at the end of fyprt.hip, inside extern "C".
//
// The frame is split into row bands, one context (one GPU) per band.  Two ways to get the ReSTIR
// records of the `radius` rows either side of a band ("halo") that Part 2's spatial reuse reads:
//   recompute (halo mode 0)  every band runs Part 1 on its halo rows too (fyprt_set_rows(..., halo)); no data crosses the fabric
//                            before the image gather; halo rows have no temporal history, so from frame 2 on pixels near a band
//                            border differ (unbiased) from a single-GPU frame;
//   exchange  (halo mode 1)  every band runs Part 1 on its own rows only; between Part 1 and Part 2 it receives the Part-1 records of
//                            its halo rows from the bands that own them, and before Part 1 their temporal history — 32 B per pixel
//                            and exchange for ReSTIR DI (1.8 MB per neighbour at 1080p), 96 B + 72 B for ReSTIR GI.  Every record is
//                            then computed once, by its owner, with its full history: a static-camera sequence is bit-identical to the
//                            single-GPU sequence on EVERY frame (tests/test_gpu_group.py), and Part 1 does 22 % less work at 8 bands.
//                            The history rows fetched are the spatial halo but at least two (temporal reuse without spatial reuse
//                            still reprojects onto the row above now and then), and a switch between the two ReSTIRs brings every
//                            band's "previous normals" in step BEFORE they travel (tests/test_gpu_group_sequences.py: 400 random
//                            sequences of techniques, settings, moved borders, restarts and interleave switches, all exact).
// Two transports under the same plan (`halo_plan`):
//   fyprt_group_*   one process, one context per GPU (what a C++ host such as the reference's application is): hipMemcpyPeerAsync
//                   between the contexts' buffers, ordered with events — no collective library at all;
//   fyprt_comm_*    one process per GPU (torch.distributed.run, MPI, ...): RCCL — grouped ncclSend / ncclRecv for the halos, grouped
//                   ncclBroadcast (one per band, in place in the full-size image) for the gather.  librccl.so.1 is opened on first use.
// fyprt_group_denoise* and fyprt_group_denoise_temporal* (below fyprt_group_synchronize): the a-trous and the temporal denoiser on the same
// bands, by the same peer copies and events — the filters' lists of steps (fyprt.hip) on one schedule, group_filter_enqueue.  The temporal history stays with
// the rows' owners, a band reads it inside its history window, and fyprt_group_set_rows moves it with the rows.
#include <dlfcn.h>

extern "C++" {
namespace {

struct RowSpan { uint32_t r0, r1; };
struct HaloXfer { int receiver, owner; uint32_t r0, r1; };

// every (receiver, owner, rows) transfer of one halo exchange, in the canonical order both ends of a pair derive independently
std::vector<HaloXfer> halo_plan(const std::vector<uint32_t>& bounds, uint32_t halo, uint32_t H, bool wrapRow) {
    std::vector<HaloXfer> plan;
    const int n = (int)bounds.size() - 1;
    for (int r = 0; r < n; ++r) {
        const uint32_t b = bounds[r], e = bounds[r + 1];
        if (b >= e) continue;
        const uint32_t lo = b > halo ? b - halo : 0u, hi = (e + halo < H) ? e + halo : H;
        std::vector<RowSpan> need;
        if (lo < b) need.push_back({lo, b});
        if (e < hi) need.push_back({e, hi});
        // the reference's unsigned neighbour wrap (R.cu:1916-1917): an offset above row 0 clamps to the LAST row
        if (wrapRow && b < halo && hi < H) need.push_back({H - 1u, H});
        for (const RowSpan& sp : need)
            for (int j = 0; j < n; ++j) {
                if (j == r) continue;
                const uint32_t a0 = std::max(sp.r0, bounds[j]), a1 = std::min(sp.r1, bounds[j + 1]);
                if (a0 < a1) plan.push_back({r, j, a0, a1});
            }
    }
    return plan;
}

// fyprt_group_denoise: every transfer of one call, in issue order.  Stage 0 = the guide records (32 B per pixel), halo 2^iterations rows
// (the farthest tap of any iteration: 2 * 2^(iterations-1)); stage 1 + k = the colour | luminance buffer iteration k reads (16 B per
// pixel), halo 2 * 2^k rows.  Clipped to the image, no wrap row; a halo higher than the neighbouring band has several owners.
struct DnXfer { int stage; HaloXfer x; };
std::vector<DnXfer> group_denoise_plan(const std::vector<uint32_t>& bounds, uint32_t H, uint32_t iterations) {
    std::vector<DnXfer> plan;
    if (iterations == 0) return plan;
    for (const HaloXfer& x : halo_plan(bounds, 1u << iterations, H, false)) plan.push_back({0, x});
    for (uint32_t k = 0; k < iterations; ++k)
        for (const HaloXfer& x : halo_plan(bounds, 2u << k, H, false)) plan.push_back({1 + (int)k, x});
    return plan;
}

// fyprt_group_denoise_temporal: every transfer of one call, in issue order, each sized by what the kernel after it reads.  Stage 0 = the
// guide records, max(2, 2^iterations) rows (the 5 x 5 variance estimate of k_dt_reproject reads 2 rows whatever the iterations); stage 1
// = the prepared colour e0 | L that estimate reads, 2 rows; stage 2 = the history records (64 B per pixel), min(historyRows, H) rows:
// the band's history window; stage 3 + k = the colour | luminance and the variance (4 B per pixel) iteration k reads, 2 * 2^k rows.
std::vector<DnXfer> group_temporal_plan(const std::vector<uint32_t>& bounds, uint32_t H, uint32_t iterations, uint32_t historyRows) {
    std::vector<DnXfer> plan;
    for (const HaloXfer& x : halo_plan(bounds, std::max(2u, 1u << iterations), H, false)) plan.push_back({0, x});
    for (const HaloXfer& x : halo_plan(bounds, 2u, H, false)) plan.push_back({1, x});
    for (const HaloXfer& x : halo_plan(bounds, std::min(historyRows, H), H, false)) plan.push_back({2, x});
    for (uint32_t k = 0; k < iterations; ++k)
        for (const HaloXfer& x : halo_plan(bounds, 2u << k, H, false)) plan.push_back({3 + (int)k, x});
    return plan;
}
// fyprt_group_denoise_upscale: the plan of its low-res stage, then one more stage, numbered after the last iteration's: every band but the
// last pulls the one low-res row below it, e_k, from its owner — the colour buffer that holds e after the last iteration (16 B per pixel).
// The resolve of the last s - 1 hi-res rows of a band taps that row.  Its guide record needs no entry: stage 0 already brings at least one
// guide row below the band (2^iterations >= 1 rows, temporal max(2, ...)) — except that the spatial plan has no stage 0 at all without an
// iteration, and the call then moves the guide record of the row with its colour (48 B per pixel; upscale_steps).
std::vector<DnXfer> group_upscale_plan(const std::vector<uint32_t>& bounds, uint32_t H, uint32_t iterations, bool temporal, uint32_t historyRows) {
    std::vector<DnXfer> plan = temporal ? group_temporal_plan(bounds, H, iterations, historyRows) : group_denoise_plan(bounds, H, iterations);
    const int n = (int)bounds.size() - 1, stage = (temporal ? 3 : 1) + (int)iterations;
    for (int k = 0; k + 1 < n; ++k) plan.push_back({stage, HaloXfer{k, k + 1, bounds[k + 1], bounds[k + 1] + 1u}});      // (no band is empty: row e_k is band k + 1's first)
    return plan;
}
// what crosses between Part 1 and Part 2 (kind 0) / before Part 1 (kind 1: temporal history), for the technique
std::vector<XBuf> exchange_buffers(fyprt_context* c, int tech, int kind) {
    std::vector<XBuf> v;
    if (tech == FYPRT_RESTIR_DI) {
        if (kind == 0) v.push_back({c->drec.p, sizeof(DIRec)});
        else v.push_back({c->dprevFlip ? (void*)c->dprevB.p : (void*)c->dprevA.p, sizeof(DIRec)});
    } else {
        if (kind == 0) {
            v.push_back({c->gi.p, sizeof(GIRes)}); v.push_back({c->giHot.p, 4 * sizeof(float4)});        // Part 2 reads a neighbour's 64-byte record; the reservoir only of the finally selected sample
            v.push_back({c->normalFlip ? (void*)c->normalA.p : (void*)c->normalB.p, sizeof(f2)});      // this frame's normals: next frame's history normals
        } else {
            v.push_back({c->giPrev.p, sizeof(GIRes)});
            v.push_back({c->normalFlip ? (void*)c->normalB.p : (void*)c->normalA.p, sizeof(f2)});      // the previous normals the history is tested against
        }
    }
    return v;
}
// what a row takes with it when it changes owner (fyprt_group_set_rows, fyprt_comm_set_rows): its accumulation — unless the last frame was
// interleaved: that accumulation lives in stripes, not in bands, and every context keeps its stripes — and its temporal history: the
// ReSTIR DI records, the ReSTIR GI reservoirs and the previous normals
std::vector<XBuf> row_buffers(fyprt_context* c, bool lastStriped) {
    std::vector<XBuf> v;
    if (!lastStriped) v.push_back({c->accum.p, sizeof(float4)});
    v.push_back({c->dprevFlip ? (void*)c->dprevB.p : (void*)c->dprevA.p, sizeof(DIRec)});
    v.push_back({c->giPrev.p, sizeof(GIRes)});
    v.push_back({c->normalFlip ? (void*)c->normalB.p : (void*)c->normalA.p, sizeof(f2)});
    return v;
}
// rows [r0, r1) of a full-size buffer (W pixels of bytesPerPixel a row) of context `o` into the same rows of context `c`'s, on `stream`
hipError_t copy_rows(const fyprt_context* c, void* dst, const fyprt_context* o, const void* src, uint32_t r0, uint32_t r1, uint32_t W, size_t bytesPerPixel, hipStream_t stream) {
    const size_t off = (size_t)r0 * W * bytesPerPixel;
    return hipMemcpyPeerAsync((char*)dst + off, c->device, (const char*)src + off, o->device, (size_t)(r1 - r0) * W * bytesPerPixel, stream);
}
// The check of a band table, for every entry that takes one: its ends are rows 0 and H, and no band is empty or out of order.  Each
// returns the text of what is wrong, or null; bad_bands looks at the ends first, then at every band, and says in `at` whose fault it is.
const char* bad_ends(const uint32_t* b, int n, uint32_t H) { return (b[0] != 0 || b[n] != H) ? ": the bands must partition rows 0..height" : nullptr; }
const char* bad_band(const uint32_t* b, int i) { return b[i] >= b[i + 1] ? ": empty or unordered band" : nullptr; }
const char* bad_bands(const uint32_t* b, int n, uint32_t H, int* at) {
    *at = 0;
    if (const char* t = bad_ends(b, n, H)) return t;
    for (; *at < n; ++*at) if (const char* t = bad_band(b, *at)) return t;
    return nullptr;
}
// What the three fyprt_group_denoise*_plan entries are: the check of the band table and the iterations, then `make(bounds)` as they hand
// a plan out — (stage, receiver, owner, first row, end row) per entry, up to `capacity` entries; returns the number of entries.
template <class Make> int export_checked_plan(const uint32_t* row_bounds, int n, uint32_t height, uint32_t iterations, uint32_t* out5, int capacity, Make&& make) {
    int at;
    if (!row_bounds || n <= 0 || iterations > 8u || bad_bands(row_bounds, n, height, &at)) return FYPRT_EINVAL;
    const std::vector<DnXfer> plan = make(std::vector<uint32_t>(row_bounds, row_bounds + n + 1));
    for (int k = 0; k < (int)plan.size() && k < capacity && out5; ++k) {
        const HaloXfer& x = plan[k].x;
        out5[5 * k] = (uint32_t)plan[k].stage; out5[5 * k + 1] = (uint32_t)x.receiver; out5[5 * k + 2] = (uint32_t)x.owner; out5[5 * k + 3] = x.r0; out5[5 * k + 4] = x.r1;
    }
    return (int)plan.size();
}
bool is_restir(const fyprt_settings* s) { return s->technique == FYPRT_RESTIR_DI || s->technique == FYPRT_RESTIR_GI; }
// stripes of part `part` of an interleaved split, as (first row, end row) — the same walk as stripe_row_count
template <class F> void for_each_stripe(uint32_t H, uint32_t stripe, uint32_t parts, uint32_t part, F&& f) {
    for (uint64_t r0 = (uint64_t)part * stripe; r0 < H; r0 += (uint64_t)parts * stripe) f((uint32_t)r0, (uint32_t)std::min<uint64_t>(r0 + stripe, H));
}
// rows around a band whose Part-1 records Part 2 reads (spatial reuse: the kernels' uint8 cast of the radius, R.cu:1897), and rows whose
// temporal history Part 1 may be reprojected onto: the spatial halo, at least kHistoryRows (a static camera reprojects a pixel onto
// itself or, by fp32 rounding of an exactly integral coordinate, onto its upper / left neighbour: Camera.cpp:143)
constexpr uint32_t kHistoryRows = 2;
uint32_t spatial_halo(const fyprt_settings* s, int n) { return (is_restir(s) && s->use_spatial_reuse && n > 1) ? ((uint32_t)s->spatial_neighbor_radius & 0xFFu) : 0u; }
uint32_t history_halo(const fyprt_settings* s, int n) { return (is_restir(s) && s->use_temporal_reuse && n > 1) ? std::max(spatial_halo(s, n), kHistoryRows) : 0u; }
void extend_history_rows(fyprt_context* c, int tech, uint32_t halo) {
    uint32_t* h = tech == FYPRT_RESTIR_DI ? c->histDI : c->histGI;
    h[0] = c->rowBegin > halo ? c->rowBegin - halo : 0u; h[1] = (c->rowEnd + halo < c->H) ? c->rowEnd + halo : c->H;
}

// ---- RCCL, opened lazily: a host that never calls fyprt_comm_* does not need the library
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr; int (*CommInitRank)(void**, int, ncclUniqueIdBytes, int) = nullptr; int (*CommDestroy)(void*) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr; int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr; int (*GroupEnd)() = nullptr; const char* (*GetErrorString)(int) = nullptr;
    std::string err;
    bool load() {
        if (lib) return true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (!lib) { err = std::string("cannot open librccl.so.1: ") + dlerror(); return false; }
        auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p) err = std::string("librccl lacks ") + n; return p; };
        GetUniqueId = (decltype(GetUniqueId))sym("ncclGetUniqueId"); CommInitRank = (decltype(CommInitRank))sym("ncclCommInitRank");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy"); Broadcast = (decltype(Broadcast))sym("ncclBroadcast");
        Send = (decltype(Send))sym("ncclSend"); Recv = (decltype(Recv))sym("ncclRecv"); GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd"); GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        if (!(GetUniqueId && CommInitRank && CommDestroy && Broadcast && Send && Recv && GroupStart && GroupEnd && GetErrorString)) { dlclose(lib); lib = nullptr; return false; }
        return true;
    }
} g_rccl;
constexpr int kNcclChar = 0;      // ncclInt8 / ncclChar: transfers are counted in bytes

// The point-to-point operations ONE rank issues inside one ncclGroupStart / ncclGroupEnd section, in issue order.  RCCL matches the
// sends and receives of a pair of ranks in the order each side issues them, so what has to hold — and what tests/test_multigpu_plan.py
// checks on the CPU for every pair, since more than one rank per device cannot run on the one-GPU box — is that rank a's sends to b
// and rank b's receives from a list the same byte counts in the same order.  Both functions are pure: (plan, rank) -> list.
struct CommOp { int recv, peer, buf; size_t offset, bytes; };
std::vector<CommOp> comm_exchange_ops(int rank, const std::vector<HaloXfer>& plan, const std::vector<size_t>& bytesPerPixel, uint32_t W) {
    std::vector<CommOp> ops;
    for (const HaloXfer& x : plan)
        for (size_t b = 0; b < bytesPerPixel.size(); ++b) {
            const size_t off = (size_t)x.r0 * W * bytesPerPixel[b], bytes = (size_t)(x.r1 - x.r0) * W * bytesPerPixel[b];
            if (x.receiver == rank) ops.push_back({1, x.owner, (int)b, off, bytes});
            else if (x.owner == rank) ops.push_back({0, x.receiver, (int)b, off, bytes});
        }
    return ops;
}
// rows that change owner when the band table `oldB` is replaced by `newB`: [r0, r1) owned by j so far, by k from now on
std::vector<CommOp> comm_set_rows_ops(int rank, const std::vector<uint32_t>& oldB, const std::vector<uint32_t>& newB, const std::vector<size_t>& bytesPerPixel, uint32_t W) {
    std::vector<CommOp> ops;
    const int n = (int)oldB.size() - 1;
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < n; ++j) {
            if (j == k) continue;
            const uint32_t r0 = std::max(newB[k], oldB[j]), r1 = std::min(newB[k + 1], oldB[j + 1]);
            if (r0 >= r1 || (rank != k && rank != j)) continue;
            for (size_t b = 0; b < bytesPerPixel.size(); ++b) {
                const size_t off = (size_t)r0 * W * bytesPerPixel[b], bytes = (size_t)(r1 - r0) * W * bytesPerPixel[b];
                ops.push_back({rank == k ? 1 : 0, rank == k ? j : k, (int)b, off, bytes});
            }
        }
    return ops;
}

}  // namespace
}  // extern "C++"

struct fyprt_group {
    std::vector<fyprt_context*> ctx; std::vector<uint32_t> bounds; int haloMode = 0;
    uint32_t stripeRows = 0, lastStripeRows = 0; bool lastStriped = false;      // interleaved split for the per-pixel techniques; whether (and with which stripes) the last frame used it
    struct BandEvents { Event p1, pulled, frame, sync; };      // per context: Part 1 done, halo pulled, frame done, history normals in step
    std::vector<BandEvents> ev; Event evGather; bool gatherPending = false; std::string err;
    // fyprt_group_denoise*, per context: its latest stage (prepare / an iteration) done, its latest halo pulled, the collect it ran as
    // root, the two timing events of the blocking entry; whether a call was enqueued before, and the root of the last one
    struct DenoiseEvents { Event done, pulled, collect, first, last; };
    std::vector<DenoiseEvents> dn; bool dnCalled = false; int dnRoot = -1;
    // fyprt_group_denoise_temporal*: the serial a member's history carries (fyprt_context::dtGroup) while this group wrote it
    uint64_t id = 0;
};
static uint64_t g_groupSerial = 0;
// The group holds a temporal history: every member's was written by this group's last temporal call (or moved by fyprt_group_set_rows
// since), for the same camera matrix.
static bool group_has_history(const fyprt_group* g) {
    const fyprt_context* c0 = g->ctx[0];
    for (const fyprt_context* c : g->ctx)
        if (!c->dtValid || c->dtGroup != g->id || c->dt.hist[0].n != 4 * (size_t)c->W * c->H || std::memcmp(c->dtPV, c0->dtPV, 64) != 0) return false;
    return true;
}

int fyprt_group_synchronize(fyprt_group* g);
#define NCCLCHK(c, call) do { const int _r = (call); if (_r != 0) return (c)->fail(FYPRT_EHIP, std::string(#call) + ": " + g_rccl.GetErrorString(_r)); } while (0)
// One group section: every operation of `ops` on the context's stream.  An error inside the section still closes it (an open group
// would swallow every later fyprt_comm_* call of this thread and the next synchronize would wait for ever).
static int comm_issue(fyprt_context* c, const std::vector<CommOp>& ops, const std::vector<void*>& base) {
    NCCLCHK(c, g_rccl.GroupStart());
    int bad = 0;
    for (const CommOp& o : ops) {
        char* p = (char*)base[(size_t)o.buf] + o.offset;
        const int e = o.recv ? g_rccl.Recv(p, o.bytes, kNcclChar, o.peer, c->comm, c->stream) : g_rccl.Send(p, o.bytes, kNcclChar, o.peer, c->comm, c->stream);
        if (e != 0) { bad = e; break; }
    }
    const int endRc = g_rccl.GroupEnd();
    if (bad != 0) return c->fail(FYPRT_EHIP, std::string("ncclSend / ncclRecv: ") + g_rccl.GetErrorString(bad));
    NCCLCHK(c, endRc);
    return FYPRT_OK;
}

// ------------------------------------------------------------------------------------------------ one process, one context per GPU
int fyprt_group_create(fyprt_context** ctxs, int n, const uint32_t* row_bounds, fyprt_group** out) {
    if (!ctxs || n <= 0 || !row_bounds || !out) return FYPRT_EINVAL;
    *out = nullptr;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i] || ctxs[i]->hostOnly || ctxs[i]->H == 0) return FYPRT_EINVAL;
        if (ctxs[i]->W != ctxs[0]->W || ctxs[i]->H != ctxs[0]->H) return ctxs[i]->fail(FYPRT_EINVAL, "fyprt_group_create: contexts differ in size");
        if (const char* bad = bad_band(row_bounds, i)) return ctxs[i]->fail(FYPRT_EINVAL, std::string("fyprt_group_create") + bad);
    }
    if (const char* bad = bad_ends(row_bounds, n, ctxs[0]->H)) return ctxs[0]->fail(FYPRT_EINVAL, std::string("fyprt_group_create") + bad);
    auto* g = new fyprt_group();
    g->ctx.assign(ctxs, ctxs + n); g->bounds.assign(row_bounds, row_bounds + n + 1);
    g->ev.resize(n); g->dn.resize(n); g->id = ++g_groupSerial;
    for (int i = 0; i < n; ++i) {
        (void)hipSetDevice(ctxs[i]->device);
        for (Event* e : {&g->ev[i].p1, &g->ev[i].pulled, &g->ev[i].frame, &g->ev[i].sync}) (void)create(*e, hipEventDisableTiming);
    }
    (void)hipSetDevice(ctxs[0]->device);
    (void)create(g->evGather, hipEventDisableTiming);
    *out = g;
    return FYPRT_OK;
}
void fyprt_group_destroy(fyprt_group* g) {
    if (!g) return;
    for (size_t i = 0; i < g->ctx.size(); ++i) {
        (void)hipSetDevice(g->ctx[i]->device); (void)sync_all(g->ctx[i]);
        g->ev[i] = fyprt_group::BandEvents();               // this band's events go while its device is current
        g->dn[i] = fyprt_group::DenoiseEvents();
        g->ctx[i]->haloExchange = false;
    }
    delete g;
}
// New band boundaries (e.g. from fyprt_balance_rows).  Rows that change owner take their accumulation and their temporal history
// (ReSTIR DI records, ReSTIR GI reservoirs + normals) with them — peer copies from the old owner, between two frames — so a sequence
// with moving borders stays what it was; and, while the group holds one, the temporal denoiser's history records.  Synchronises the group.
int fyprt_group_set_rows(fyprt_group* g, const uint32_t* row_bounds) {
    if (!g || !row_bounds) return FYPRT_EINVAL;
    const int n = (int)g->ctx.size();
    const uint32_t W = g->ctx[0]->W;
    int at;
    if (const char* bad = bad_bands(row_bounds, n, g->ctx[0]->H, &at)) return g->ctx[at]->fail(FYPRT_EINVAL, std::string("fyprt_group_set_rows") + bad);
    TRY(fyprt_group_synchronize(g));
    const bool history = group_has_history(g);
    auto moving = [&](fyprt_context* c) {                             // per context: the flips of its ping-pong buffers are its own
        std::vector<XBuf> v = row_buffers(c, g->lastStriped);
        if (history) v.push_back({c->dt.hist[c->dtCur].p, kDtHistoryBytes});
        return v;
    };
    for (int k = 0; k < n; ++k) {
        fyprt_context* c = g->ctx[k];
        HIPCHK(c, hipSetDevice(c->device));
        const std::vector<XBuf> mine = moving(c);
        for (int j = 0; j < n; ++j) {
            if (j == k) continue;
            const uint32_t r0 = std::max(row_bounds[k], g->bounds[j]), r1 = std::min(row_bounds[k + 1], g->bounds[j + 1]);
            if (r0 >= r1) continue;                                   // rows [r0, r1): owned by j so far, by k from now on
            const std::vector<XBuf> theirs = moving(g->ctx[j]);
            for (size_t b = 0; b < mine.size(); ++b) HIPCHK(c, copy_rows(c, mine[b].p, g->ctx[j], theirs[b].p, r0, r1, W, mine[b].bytesPerPixel, c->stream));
        }
    }
    TRY(fyprt_group_synchronize(g));
    g->bounds.assign(row_bounds, row_bounds + n + 1);
    for (int k = 0; k < n; ++k) {
        fyprt_context* c = g->ctx[k];
        c->histDI[0] = c->histGI[0] = row_bounds[k]; c->histDI[1] = c->histGI[1] = row_bounds[k + 1];
    }
    return FYPRT_OK;
}
int fyprt_group_set_halo_mode(fyprt_group* g, int mode) { if (!g || mode < 0 || mode > 1) return FYPRT_EINVAL; g->haloMode = mode; return FYPRT_OK; }
// Interleaved bands for the techniques without spatial reuse: context i renders the stripes of `stripe_rows` rows with
// index i modulo n — see fyprt_set_row_stripes.  ReSTIR frames keep the contiguous bands.  0 = contiguous bands for everything.
// A change takes effect with the next frame and, like a technique change in the reference (Renderer::ResetFrameIndex), wants the
// accumulation restarted: the rows a context has accumulated are the rows it rendered.
int fyprt_group_set_interleave(fyprt_group* g, uint32_t stripe_rows) {
    if (!g) return FYPRT_EINVAL;
    if (stripe_rows != 0 && (uint64_t)stripe_rows * g->ctx.size() > g->ctx[0]->H) return g->ctx[0]->fail(FYPRT_EINVAL, "fyprt_group_set_interleave: fewer stripes than contexts");
    g->stripeRows = stripe_rows;
    return FYPRT_OK;
}

// One frame on every band (asynchronous: returns when everything is enqueued; fyprt_group_synchronize / fyprt_synchronize wait).
int fyprt_group_render(fyprt_group* g, const fyprt_settings* s) {
    if (!g || !s) return FYPRT_EINVAL;
    const int n = (int)g->ctx.size();
    const uint32_t H = g->ctx[0]->H, W = g->ctx[0]->W;
    const uint32_t halo = spatial_halo(s, n), hhalo = history_halo(s, n);
    const bool exchange = g->haloMode == 1 && (halo > 0 || hhalo > 0);
    const bool striped = g->stripeRows != 0 && n > 1 && !is_restir(s);
    g->lastStriped = striped; g->lastStripeRows = g->stripeRows;
    for (int i = 0; i < n; ++i) {
        fyprt_context* c = g->ctx[i];
        c->rowBegin = g->bounds[i]; c->rowEnd = g->bounds[i + 1]; c->halo = halo; c->rowsSet = true; c->haloExchange = exchange;
        if (striped) TRY(fyprt_set_row_stripes(c, g->stripeRows, (uint32_t)n, (uint32_t)i));
        else c->stripeRows = 0;
        // the previous frame's gather still reads this band's image rows on the root's stream: the new frame's epilogues wait for it
        if (g->gatherPending) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamWaitEvent(c->stream, g->evGather, 0)); }
    }
    g->gatherPending = false;
    if (!exchange) {
        for (int i = 0; i < n; ++i) {
            fyprt_context* c = g->ctx[i];
            TRY(enqueue_frame(c, s, true));
            HIPCHK(c, hipEventRecord(g->ev[i].frame, c->stream));
        }
        return FYPRT_OK;
    }
    const std::vector<HaloXfer> plan = halo_plan(g->bounds, halo, H, true), hplan = halo_plan(g->bounds, hhalo, H, false);
    auto pull = [&](int i, const std::vector<HaloXfer>& pl, int kind, Event fyprt_group::BandEvents::*ready) -> int {
        fyprt_context* c = g->ctx[i];
        HIPCHK(c, hipSetDevice(c->device));
        const std::vector<XBuf> mine = exchange_buffers(c, s->technique, kind);
        for (const HaloXfer& x : pl) {
            if (x.receiver != i) continue;
            fyprt_context* o = g->ctx[x.owner];
            HIPCHK(c, hipStreamWaitEvent(c->stream, g->ev[x.owner].*ready, 0));
            if (kind == 1) HIPCHK(c, hipStreamWaitEvent(c->stream, g->ev[x.owner].sync, 0));      // the owner's history is in step with the technique
            const std::vector<XBuf> theirs = exchange_buffers(o, s->technique, kind);
            for (size_t b = 0; b < mine.size(); ++b) HIPCHK(c, copy_rows(c, mine[b].p, o, theirs[b].p, x.r0, x.r1, W, mine[b].bytesPerPixel, c->stream));
        }
        return FYPRT_OK;
    };
    // 0. a switch between the two ReSTIRs: every band brings its "previous normals" in step before anybody fetches them
    for (int i = 0; i < n; ++i) {
        fyprt_context* c = g->ctx[i];
        HIPCHK(c, hipSetDevice(c->device));
        TRY(sync_restir_normals(c, s->technique, c->stream));
        HIPCHK(c, hipEventRecord(g->ev[i].sync, c->stream));
    }
    // 1. temporal history of the halo rows, then Part 1 on the band's own rows
    for (int i = 0; i < n; ++i) {
        fyprt_context* c = g->ctx[i];
        HIPCHK(c, hipSetDevice(c->device));
        for (int j = 0; j < n; ++j) if (j != i) HIPCHK(c, hipStreamWaitEvent(c->stream, g->ev[j].pulled, 0));    // last frame's pulls FROM this band are done
        if (s->use_temporal_reuse) TRY(pull(i, hplan, 1, &fyprt_group::BandEvents::frame));
        extend_history_rows(c, s->technique, hhalo);
        TRY(enqueue_frame(c, s, true, 1));
        HIPCHK(c, hipEventRecord(g->ev[i].p1, c->stream));
    }
    // 2. the neighbours' Part-1 records of the halo rows, then Part 2
    for (int i = 0; i < n; ++i) {
        fyprt_context* c = g->ctx[i];
        TRY(pull(i, plan, 0, &fyprt_group::BandEvents::p1));
        HIPCHK(c, hipEventRecord(g->ev[i].pulled, c->stream));
    }
    for (int i = 0; i < n; ++i) {
        fyprt_context* c = g->ctx[i];
        HIPCHK(c, hipSetDevice(c->device));
        TRY(enqueue_frame(c, s, true, 2));
        HIPCHK(c, hipEventRecord(g->ev[i].frame, c->stream));
    }
    return FYPRT_OK;
}
// The bands' RGBA8 rows into the image of context `root` (the one that presents), on root's stream, after every band's frame.
int fyprt_group_gather(fyprt_group* g, int root) {
    if (!g || root < 0 || root >= (int)g->ctx.size()) return FYPRT_EINVAL;
    fyprt_context* r = g->ctx[root];
    HIPCHK(r, hipSetDevice(r->device));
    uint32_t* dst = r->externalImage ? r->externalImage : r->image.p;
    for (int i = 0; i < (int)g->ctx.size(); ++i) {
        if (i == root) continue;
        fyprt_context* c = g->ctx[i];
        HIPCHK(r, hipStreamWaitEvent(r->stream, g->ev[i].frame, 0));
        const uint32_t* src = c->externalImage ? c->externalImage : c->image.p;
        hipError_t e = hipSuccess;
        auto rows = [&](uint32_t r0, uint32_t r1) { if (e == hipSuccess) e = copy_rows(r, dst, c, src, r0, r1, r->W, sizeof(uint32_t), r->stream); };
        if (g->lastStriped) for_each_stripe(r->H, g->lastStripeRows, (uint32_t)g->ctx.size(), (uint32_t)i, rows);
        else rows(g->bounds[i], g->bounds[i + 1]);
        HIPCHK(r, e);
    }
    HIPCHK(r, hipEventRecord(g->evGather, r->stream));
    g->gatherPending = true;
    return FYPRT_OK;
}
int fyprt_group_synchronize(fyprt_group* g) {
    if (!g) return FYPRT_EINVAL;
    for (fyprt_context* c : g->ctx) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c)); }
    return FYPRT_OK;
}

// ---- fyprt_group_denoise*: the a-trous denoiser (rt_denoise.h) on the group's bands.  Every pixel is filtered by the context that owns
// its row, with its band as the kernels' DnBand; what a tap beyond the band reads was pulled from the row's owner into the same place of
// this context's full-size guide / colour buffers (group_denoise_plan).  The shared pixel code on the same inputs: the single-context
// call's bits.  Nothing but the denoiser's own buffers and the caller's outputs is written.
// everything fyprt_group_denoise* checks after the parameters, in the header's order (fyprt_group_denoise_temporal* shares it)
static int group_denoise_check_call(fyprt_group* g, const char* who, int root, const void* rgba8, const void* radiance4, bool device) {
    const int n = (int)g->ctx.size();
    if (root < 0 || root >= n) return g->ctx[0]->fail(FYPRT_EINVAL, std::string(who) + ": root out of range");
    TRY(check_denoise_outputs(g->ctx[root], who, rgba8, radiance4, device));
    for (int i = 0; i < n; ++i) TRY(check_denoise_frame(g->ctx[i], who));
    for (int i = 1; i < n; ++i)
        if (g->ctx[i]->lastFrameIndex != g->ctx[0]->lastFrameIndex) return g->ctx[i]->fail(FYPRT_ESTATE, std::string(who) + ": the members' last frames differ in frame index");
    if (g->lastStriped) return g->ctx[0]->fail(FYPRT_ESTATE, std::string(who) + ": the last group frame was striped (fyprt_group_set_interleave): the filter needs contiguous bands");
    for (int i = 0; i < n; ++i) {
        fyprt_context* c = g->ctx[i];
        if (c->rowBegin != g->bounds[i] || c->rowEnd != g->bounds[i + 1] || c->stripeRows != 0)
            return c->fail(FYPRT_ESTATE, std::string(who) + ": the member's rows are not its band of the group (fyprt_set_rows / fyprt_set_row_stripes behind the group)");
    }
    return FYPRT_OK;
}
static int group_denoise_check(fyprt_group* g, const fyprt_denoise_params* p, int root, const void* rgba8, const void* radiance4, bool device) {
    const char* who = device ? "fyprt_group_denoise_device" : "fyprt_group_denoise";
    if (!g) return FYPRT_EINVAL;
    TRY(check_denoise_params(g->ctx[0], who, p));
    return group_denoise_check_call(g, who, root, rgba8, radiance4, device);
}

// ---- group_filter_enqueue: one filter call on the group's bands, which both denoisers enqueue with.  A call is a plan — which rows a
// band pulls from which owner at which stage — and the filter's list of steps (BandStep, fyprt.hip); the engine below runs the steps in order, each on every band
// before the next on any (the waits of a step resolve to the records of the step before, so the host's issue order is part of it):
//   1. if the step's launch overwrites rows that neighbours pulled earlier: every band waits for the `pulled` of the bands that pull from it;
//   2. if the step pulls a plan stage: every band copies that stage's rows from their owners, after the owner's `done`, and records `pulled`
//      (also when it had nothing to pull);
//   3. if the step launches: every band launches and, unless the step says otherwise, records `done`.
// Around them: the members' buffers, events and output rows (a non-root band writes a staging buffer of its size; the kernels index the
// whole frame, so they get the address row 0 would have), the first work of the call, the end of a band, and the collect of the staging
// rows on root's stream.  No host wait but before a staging buffer is reallocated.  rgba8 / radiance4: device memory of root's GPU.
// Hazards, and the event that orders each:
//   read after write   a pull reads rows the owner's latest kernel wrote — the prepared colour and the guide records (prepare), the colour
//                      (and, temporal, the variance) the iteration before or the reprojection wrote, the history the call before wrote
//                      (which the owner's stream orders before its prepare): it waits for the owner's `done`, recorded after each of
//                      these launches.  A launch nothing pulls from (k_dt_moved) records none, and the `done` a pull after it waits
//                      for is the owner's latest earlier one;
//   write after read   an iteration writes the ping-pong buffers the iteration before read, which the neighbours pulled from one stage
//                      earlier (spatial: iteration k > 0 writes what stage k moved, and iteration 0 writes dn.col[1], which nothing pulled
//                      in this call; temporal: iteration k overwrites colour and variance of stage 3 + k - 1, and iteration 0 the
//                      prepared colour of stage 1): it waits for the last `pulled` of every band that pulls from this one, as recorded
//                      after that stage or a later one;
//   the history        ping-pongs per member: a temporal call writes dt.hist[dtCur ^ 1], the buffer the neighbours' stage 2 of the call
//                      before pulled from.  The first work of a call on a band waits for every other band's last `pulled` of the earlier
//                      call — recorded after that call's last stage, so after its stage 2 — which also covers the colour, variance and
//                      guide buffers;
//   across calls       a later call of either denoiser (or the same call of the next frame of a pipelined sequence) may be enqueued
//                      while neighbours still pull from this band: the first-work wait above; the kernel that writes the staging rows
//                      waits for the earlier root's `collect`, which may still read them; and the front stream waits for the band's last
//                      kernel before the next pipelined frame's Part 1 overwrites the payload (dn_call_done).
// The upscale call (fyprt_group_denoise_upscale*) runs on the same engine with an output scale s: the output rows of band [b, e) are the
// hi-res rows [s b, s e) at width s W, in the members' upscale staging (up.outImg / up.outRad) instead of the denoiser's — sizes, bias,
// collect and the blocking wrapper's staging all follow `scale`; with 1 everything is as above.  What its last stage adds:
//   read after write   the pull of row e reads the owner's colour buffer after its last iteration: the owner's `done`, which that iteration
//                      recorded — without an iteration the `done` of prepare (spatial: e0) or of the reprojection (temporal: the
//                      integrated colour).  k_up_primary records none and nothing pulls what it writes;
//   write after read   the next call's first kernel (prepare) may overwrite that buffer while a neighbour still pulls the row: the
//                      first-work wait on every other band's last `pulled`, which is now the one recorded after this stage.  Within the
//                      call nothing writes a colour buffer after the last iteration;
//   the staging        the resolve writes the band's hi-res staging rows, which the earlier root's `collect` may still read: the
//                      writesOutput wait, as for the low-res staging.  A staging or hi-res buffer reallocated for another scale is first
//                      waited for on the host (group_ensure_up_buffers).
// The first step must not pull: the first-work wait goes with its launch (both denoisers start with prepare).
static int group_filter_enqueue(fyprt_group* g, const std::vector<DnXfer>& plan, const std::vector<BandStep>& steps, uint32_t demodulate, int root,
                                uint32_t* rgba8, float4* radiance4, bool timed, uint32_t scale = 1u) {
    const int n = (int)g->ctx.size();
    const uint32_t W = g->ctx[0]->W, outW = W * scale;
    std::vector<char> pullsFrom((size_t)n * n, 0);                // [owner * n + receiver]
    for (const DnXfer& t : plan) pullsFrom[(size_t)t.x.owner * n + t.x.receiver] = 1;
    std::vector<DnFrame> frames(n); std::vector<DnBand> bands(n);
    for (int i = 0; i < n; ++i) {
        fyprt_context* c = g->ctx[i];
        HIPCHK(c, hipSetDevice(c->device));
        TRY(ensure_dn_buffers(c));
        fyprt_group::DenoiseEvents& e = g->dn[i];
        HIPCHK(c, create(e.done, hipEventDisableTiming)); HIPCHK(c, create(e.pulled, hipEventDisableTiming)); HIPCHK(c, create(e.collect, hipEventDisableTiming));
        if (timed) { HIPCHK(c, create(e.first)); HIPCHK(c, create(e.last)); }
        const uint32_t b = g->bounds[i], rows = g->bounds[i + 1] - b;
        bands[i] = DnBand{b, g->bounds[i + 1]};
        DnFrame& fr = frames[i];
        fr = dn_frame(c, demodulate, i == root ? rgba8 : nullptr, i == root ? radiance4 : nullptr);
        if (i == root) continue;
        // the band's output rows go to its staging (at least the band's size), biased to row 0.  A buffer the earlier root may still read
        // is not freed under it.
        DevBuf<uint32_t>& outImg = scale > 1u ? c->up.outImg : c->dn.outImg;
        DevBuf<float4>& outRad = scale > 1u ? c->up.outRad : c->dn.outRad;
        const size_t need = (size_t)rows * scale * outW, bias = (size_t)b * scale * outW;
        if ((rgba8 && outImg.n < need) || (radiance4 && outRad.n < need)) {
            if (g->dnRoot >= 0) HIPCHK(c, hipEventSynchronize(g->dn[g->dnRoot].collect));
            if (rgba8 && outImg.n < need) HIPCHK(c, outImg.alloc(need));
            if (radiance4 && outRad.n < need) HIPCHK(c, outRad.alloc(need));
        }
        if (rgba8) fr.rgba8 = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(outImg.p) - bias * sizeof(uint32_t));
        if (radiance4) fr.radiance4 = reinterpret_cast<float4*>(reinterpret_cast<uintptr_t>(outRad.p) - bias * sizeof(float4));
    }
    std::vector<std::vector<XBuf>> moved(n);
    for (const BandStep& st : steps) {
        if (st.overwritesPulled)                                  // every band that pulls from band i has pulled what it last asked for
            for (int i = 0; i < n; ++i) {
                fyprt_context* c = g->ctx[i];
                HIPCHK(c, hipSetDevice(c->device));
                for (int j = 0; j < n; ++j) if (pullsFrom[(size_t)i * n + j]) HIPCHK(c, hipStreamWaitEvent(c->stream, g->dn[j].pulled, 0));
            }
        if (st.pulls >= 0) {
            for (int i = 0; i < n; ++i) moved[i] = st.moved(g->ctx[i]);
            for (int i = 0; i < n; ++i) {
                fyprt_context* c = g->ctx[i];
                HIPCHK(c, hipSetDevice(c->device));
                for (const DnXfer& t : plan) {
                    if (t.stage != st.pulls || t.x.receiver != i) continue;
                    const int o = t.x.owner;
                    HIPCHK(c, hipStreamWaitEvent(c->stream, g->dn[o].done, 0));
                    for (size_t b = 0; b < moved[i].size(); ++b)
                        HIPCHK(c, copy_rows(c, moved[i][b].p, g->ctx[o], moved[o][b].p, t.x.r0, t.x.r1, W, moved[i][b].bytesPerPixel, c->stream));
                }
                HIPCHK(c, hipEventRecord(g->dn[i].pulled, c->stream));
            }
        }
        if (!st.launch) continue;
        for (int i = 0; i < n; ++i) {
            fyprt_context* c = g->ctx[i];
            HIPCHK(c, hipSetDevice(c->device));
            if (&st == &steps.front()) {                          // the first work of the call: after the earlier call's pulls from this band
                if (timed) HIPCHK(c, hipEventRecord(g->dn[i].first, c->stream));
                if (g->dnCalled) for (int j = 0; j < n; ++j) if (j != i) HIPCHK(c, hipStreamWaitEvent(c->stream, g->dn[j].pulled, 0));
            }
            // the earlier call's collect still reads this band's staging rows
            if (st.writesOutput && i != root && g->dnRoot >= 0) HIPCHK(c, hipStreamWaitEvent(c->stream, g->dn[g->dnRoot].collect, 0));
            st.launch(c, frames[i], bands[i]);
            HIPCHK(c, hipGetLastError());
            if (st.recordsDone) HIPCHK(c, hipEventRecord(g->dn[i].done, c->stream));
        }
    }
    for (int i = 0; i < n; ++i) {                                 // the end of a band
        fyprt_context* c = g->ctx[i];
        HIPCHK(c, hipSetDevice(c->device));
        if (timed) HIPCHK(c, hipEventRecord(g->dn[i].last, c->stream));
        TRY(dn_call_done(c));
    }
    // the other bands' output rows into the caller's buffers, on root's stream
    fyprt_context* r = g->ctx[root];
    HIPCHK(r, hipSetDevice(r->device));
    for (int i = 0; i < n; ++i) {
        if (i == root) continue;
        HIPCHK(r, hipStreamWaitEvent(r->stream, g->dn[i].done, 0));
        const uint32_t r0 = bands[i].rowBegin * scale, r1 = bands[i].rowEnd * scale;
        if (rgba8) HIPCHK(r, copy_rows(r, rgba8, g->ctx[i], frames[i].rgba8, r0, r1, outW, sizeof(uint32_t), r->stream));
        if (radiance4) HIPCHK(r, copy_rows(r, radiance4, g->ctx[i], frames[i].radiance4, r0, r1, outW, sizeof(float4), r->stream));
    }
    HIPCHK(r, hipEventRecord(g->dn[root].collect, r->stream));
    g->dnCalled = true; g->dnRoot = root;
    return FYPRT_OK;
}
// The blocking form of either group call, as denoise_blocking is of a context's: the group synchronised (the last frame is complete on
// every stream), the outputs staged at full size on member 0, `enqueue(rgba8, radiance4)` with member 0 as root and timed, copied back;
// band_ms from every member's timing events.  scale > 1 (the upscale call): scale*W x scale*H pixels through member 0's upscale staging,
// after `prepare` — the hi-res buffers of the members, which a change of scale drops together with that staging.
static int group_denoise_blocking(fyprt_group* g, uint32_t* rgba8, float* radiance4, float* band_ms, const std::function<int(uint32_t*, float4*)>& enqueue,
                                  uint32_t scale = 1u, const std::function<int()>& prepare = nullptr) {
    TRY(fyprt_group_synchronize(g));
    if (prepare) TRY(prepare());
    fyprt_context* r = g->ctx[0];
    HIPCHK(r, hipSetDevice(r->device));
    DevBuf<uint32_t>& outImg = scale > 1u ? r->up.outImg : r->dn.outImg;
    DevBuf<float4>& outRad = scale > 1u ? r->up.outRad : r->dn.outRad;
    const size_t npx = (size_t)r->W * scale * ((size_t)r->H * scale);
    if (rgba8 && outImg.n != npx) HIPCHK(r, outImg.alloc(npx));
    if (radiance4 && outRad.n != npx) HIPCHK(r, outRad.alloc(npx));
    TRY(enqueue(rgba8 ? outImg.p : nullptr, radiance4 ? outRad.p : nullptr));
    HIPCHK(r, hipSetDevice(r->device));
    if (rgba8) HIPCHK(r, hipMemcpyAsync(rgba8, outImg.p, npx * 4, hipMemcpyDeviceToHost, r->stream));
    if (radiance4) HIPCHK(r, hipMemcpyAsync(radiance4, outRad.p, npx * 16, hipMemcpyDeviceToHost, r->stream));
    HIPCHK(r, hipStreamSynchronize(r->stream));
    for (size_t i = 0; i < g->ctx.size(); ++i) {
        fyprt_context* c = g->ctx[i];
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipEventSynchronize(g->dn[i].last));
        if (band_ms) HIPCHK(c, hipEventElapsedTime(&band_ms[i], g->dn[i].first, g->dn[i].last));
    }
    return FYPRT_OK;
}

// The spatial call: the plan, the list (spatial_steps), the engine.  up: the call is the low-res stage of fyprt_group_denoise_upscale*
// (group_upscale_plan, upscale_steps), at its scale.
#ifndef FYPRT_UP_PRIMARY_EARLY
#define FYPRT_UP_PRIMARY_EARLY 0     // 1: a group's k_up_primary directly after prepare (the placement it was timed against); a context alone is not affected
#endif
static int group_spatial_call(fyprt_group* g, const fyprt_denoise_params* p, int root, uint32_t* rgba8, float4* radiance4, bool timed, const fyprt_upscale_params* up = nullptr) {
    const uint32_t H = g->ctx[0]->H;
    const std::vector<DnXfer> plan = up ? group_upscale_plan(g->bounds, H, p->iterations, false, 0u) : group_denoise_plan(g->bounds, H, p->iterations);
    const std::vector<BandStep> steps = up ? upscale_steps(*up, false, 0u, FYPRT_UP_PRIMARY_EARLY != 0) : spatial_steps(*p);
    return group_filter_enqueue(g, plan, steps, p->demodulate_albedo, root, rgba8, radiance4, timed, up ? up->scale : 1u);
}

int fyprt_group_denoise(fyprt_group* g, const fyprt_denoise_params* p, uint32_t* rgba8, float* radiance4, float* band_ms) {
    TRY(group_denoise_check(g, p, 0, rgba8, radiance4, false));
    return group_denoise_blocking(g, rgba8, radiance4, band_ms, [&](uint32_t* img, float4* rad) { return group_spatial_call(g, p, 0, img, rad, true); });
}

int fyprt_group_denoise_device(fyprt_group* g, const fyprt_denoise_params* p, int root, void* rgba8, void* radiance4) {
    TRY(group_denoise_check(g, p, root, rgba8, radiance4, true));
    return group_spatial_call(g, p, root, static_cast<uint32_t*>(rgba8), static_cast<float4*>(radiance4), false);
}

// The transfers of one fyprt_group_denoise* call in issue order: (stage, receiver, owner, first row, end row) per entry.
int fyprt_group_denoise_plan(const uint32_t* row_bounds, int n, uint32_t height, uint32_t iterations, uint32_t* out5, int capacity) {
    return export_checked_plan(row_bounds, n, height, iterations, out5, capacity, [&](const std::vector<uint32_t>& b) { return group_denoise_plan(b, height, iterations); });
}

// ---- fyprt_group_denoise_temporal*: the temporal denoiser (rt_temporal.h) on the group's bands, as fyprt_group_denoise* above: the band
// as the kernels' DnBand, its history window as the reprojection's second DnBand, and what a kernel reads beyond the band pulled from
// the rows' owners into the same place of this context's full-size buffers (group_temporal_plan).  Every member keeps the history of
// its own rows in its own ping-pong pair; dt.hist[dtCur] of a member also holds the window rows the last call pulled, which nothing
// reads again.
// the state cases a temporal call adds to group_denoise_check_call's (fyprt_group_denoise_upscale* with temporal = 1 shares them)
static int group_temporal_check_state(fyprt_group* g, const char* who) {
    fyprt_context* c0 = g->ctx[0];
    for (fyprt_context* c : g->ctx)
        if (std::memcmp(c->framePV, c0->framePV, 64) != 0) return c->fail(FYPRT_ESTATE, std::string(who) + ": the members' last frames differ in camera matrix");
    const bool history = group_has_history(g);
    for (fyprt_context* c : g->ctx)
        if (c->dtMotion != c0->dtMotion || (history && c->dtSnapPending != c0->dtSnapPending))
            return c->fail(FYPRT_ESTATE, std::string(who) + ": the members differ in motion mode (fyprt_denoise_temporal_set_motion) or in having a geometry edit pending");
    return FYPRT_OK;
}
static int group_temporal_check(fyprt_group* g, const fyprt_temporal_params* p, int root, const void* rgba8, const void* radiance4, bool device) {
    const char* who = device ? "fyprt_group_denoise_temporal_device" : "fyprt_group_denoise_temporal";
    if (!g) return FYPRT_EINVAL;
    fyprt_context* c0 = g->ctx[0];
    TRY(check_temporal_params(c0, who, p));
    TRY(check_denoise_params(c0, who, &p->spatial));
    TRY(group_denoise_check_call(g, who, root, rgba8, radiance4, device));
    return group_temporal_check_state(g, who);
}

// The temporal call: the members' buffers; the plan (without stage 2 while the group holds no history); the list (temporal_steps), a
// band's history window min(historyRows, H) rows either side of it; the engine; the members' bookkeeping, which advances only once
// everything is enqueued.  up: as group_spatial_call's.
static int group_temporal_call(fyprt_group* g, const fyprt_temporal_params* p, uint32_t historyRows, int root, uint32_t* rgba8, float4* radiance4, bool timed,
                               const fyprt_upscale_params* up = nullptr) {
    const uint32_t H = g->ctx[0]->H, R = std::min(historyRows, H), iterations = p->spatial.iterations;
    for (fyprt_context* c : g->ctx) { HIPCHK(c, hipSetDevice(c->device)); TRY(ensure_dt_buffers(c)); }      // (may drop the history)
    const bool history = group_has_history(g);
    std::vector<DnXfer> plan;
    for (const DnXfer& t : up ? group_upscale_plan(g->bounds, H, iterations, true, R) : group_temporal_plan(g->bounds, H, iterations, R))
        if (t.stage != 2 || history) plan.push_back(t);
    const std::vector<BandStep> steps = up ? upscale_steps(*up, history, R, FYPRT_UP_PRIMARY_EARLY != 0) : temporal_steps(*p, history, R);
    TRY(group_filter_enqueue(g, plan, steps, p->spatial.demodulate_albedo, root, rgba8, radiance4, timed, up ? up->scale : 1u));
    for (fyprt_context* c : g->ctx) dt_advance(c, g->id);
    return FYPRT_OK;
}
// A failed enqueue leaves some bands' new history written and others' not: the group's history is dropped instead.
static int group_temporal_call_or_drop(fyprt_group* g, const fyprt_temporal_params* p, uint32_t historyRows, int root, uint32_t* rgba8, float4* radiance4, bool timed,
                                       const fyprt_upscale_params* up = nullptr) {
    const int rc = group_temporal_call(g, p, historyRows, root, rgba8, radiance4, timed, up);
    if (rc != FYPRT_OK) for (fyprt_context* c : g->ctx) c->drop_history();
    return rc;
}

int fyprt_group_denoise_temporal(fyprt_group* g, const fyprt_temporal_params* p, uint32_t history_rows, uint32_t* rgba8, float* radiance4, float* band_ms) {
    TRY(group_temporal_check(g, p, 0, rgba8, radiance4, false));
    return group_denoise_blocking(g, rgba8, radiance4, band_ms, [&](uint32_t* img, float4* rad) { return group_temporal_call_or_drop(g, p, history_rows, 0, img, rad, true); });
}

int fyprt_group_denoise_temporal_device(fyprt_group* g, const fyprt_temporal_params* p, uint32_t history_rows, int root, void* rgba8, void* radiance4) {
    TRY(group_temporal_check(g, p, root, rgba8, radiance4, true));
    return group_temporal_call_or_drop(g, p, history_rows, root, static_cast<uint32_t*>(rgba8), static_cast<float4*>(radiance4), false);
}

int fyprt_group_denoise_temporal_reset(fyprt_group* g) {
    if (!g) return FYPRT_EINVAL;
    for (fyprt_context* c : g->ctx) c->drop_history();
    return FYPRT_OK;
}

// The transfers of one fyprt_group_denoise_temporal* call in issue order, entries as fyprt_group_denoise_plan's.
int fyprt_group_denoise_temporal_plan(const uint32_t* row_bounds, int n, uint32_t height, uint32_t iterations, uint32_t history_rows, uint32_t* out5, int capacity) {
    return export_checked_plan(row_bounds, n, height, iterations, out5, capacity, [&](const std::vector<uint32_t>& b) { return group_temporal_plan(b, height, iterations, history_rows); });
}

// ---- fyprt_group_denoise_upscale*: the guided upscaler (rt_upscale.h) on the group's bands.  The low-res stage is the group's (either call
// above in its keep form); band [b, e) then traces and resolves the hi-res rows [s b, s e) itself, after pulling the one low-res row below
// it.  The hi-res guide and albedo buffers are full size on every member (48 B per hi-res pixel), as every other group buffer is.
static int group_upscale_check(fyprt_group* g, const fyprt_upscale_params* p, int root, const void* rgba8, const void* radiance4, bool device) {
    const char* who = device ? "fyprt_group_denoise_upscale_device" : "fyprt_group_denoise_upscale";
    if (!g) return FYPRT_EINVAL;
    fyprt_context* c0 = g->ctx[0];
    TRY(check_upscale_params(c0, who, p));
    TRY(group_denoise_check_call(g, who, root, rgba8, radiance4, device));
    for (fyprt_context* c : g->ctx) {                         // the bands would otherwise trace different hi-res frames
        const DevCamera &a = c->frameCam, &b = c0->frameCam;
        if (std::memcmp(&a.invProj, &b.invProj, sizeof a.invProj) != 0 || std::memcmp(&a.invView, &b.invView, sizeof a.invView) != 0 ||
            std::memcmp(&a.position, &b.position, sizeof a.position) != 0 || std::memcmp(&c->frameSky, &c0->frameSky, sizeof c->frameSky) != 0)
            return c->fail(FYPRT_ESTATE, std::string(who) + ": the members' last frames differ in camera or sky colour");
    }
    return p->temporal ? group_temporal_check_state(g, who) : FYPRT_OK;
}
// The members' hi-res buffers for scale s.  Another scale drops a member's old ones together with its hi-res staging: the member's own
// stream may still write them (ensure_up_buffers waits for it), and the earlier root's collect may still read the staging.
static int group_ensure_up_buffers(fyprt_group* g, uint32_t s) {
    for (fyprt_context* c : g->ctx) {
        HIPCHK(c, hipSetDevice(c->device));
        if ((c->upScale != s || c->up.albedo.n != (size_t)c->W * s * ((size_t)c->H * s)) && (c->up.outImg.p || c->up.outRad.p) && g->dnRoot >= 0)
            HIPCHK(c, hipEventSynchronize(g->dn[g->dnRoot].collect));
        TRY(ensure_up_buffers(c, s));
    }
    return FYPRT_OK;
}
static int group_upscale_call(fyprt_group* g, const fyprt_upscale_params* p, uint32_t historyRows, int root, uint32_t* rgba8, float4* radiance4, bool timed) {
    const int rc = p->temporal ? group_temporal_call_or_drop(g, &p->filter, historyRows, root, rgba8, radiance4, timed, p)
                               : group_spatial_call(g, &p->filter.spatial, root, rgba8, radiance4, timed, p);
    if (rc == FYPRT_OK) for (fyprt_context* c : g->ctx) c->upValid = true;
    return rc;
}

int fyprt_group_denoise_upscale(fyprt_group* g, const fyprt_upscale_params* p, uint32_t history_rows, uint32_t* rgba8, float* radiance4, float* band_ms) {
    TRY(group_upscale_check(g, p, 0, rgba8, radiance4, false));
    return group_denoise_blocking(g, rgba8, radiance4, band_ms, [&](uint32_t* img, float4* rad) { return group_upscale_call(g, p, history_rows, 0, img, rad, true); },
                                  p->scale, [&]() { return group_ensure_up_buffers(g, p->scale); });
}

int fyprt_group_denoise_upscale_device(fyprt_group* g, const fyprt_upscale_params* p, uint32_t history_rows, int root, void* rgba8, void* radiance4) {
    TRY(group_upscale_check(g, p, root, rgba8, radiance4, true));
    TRY(group_ensure_up_buffers(g, p->scale));
    return group_upscale_call(g, p, history_rows, root, static_cast<uint32_t*>(rgba8), static_cast<float4*>(radiance4), false);
}

// The transfers of one fyprt_group_denoise_upscale* call in issue order, entries as fyprt_group_denoise_plan's.
int fyprt_group_denoise_upscale_plan(const uint32_t* row_bounds, int n, uint32_t height, uint32_t iterations, uint32_t temporal, uint32_t history_rows, uint32_t* out5,
                                     int capacity) {
    return export_checked_plan(row_bounds, n, height, iterations, out5, capacity,
                               [&](const std::vector<uint32_t>& b) { return group_upscale_plan(b, height, iterations, temporal != 0, history_rows); });
}

// Cost-balanced bands: new boundaries from the time each band took last frame, assuming a band's cost is spread evenly over its rows
// (piecewise-constant cost density), moved at most `max_shift` rows per boundary and frame, every band at least `min_rows` high.
int fyprt_balance_rows(const uint32_t* row_bounds, const float* band_ms, int n, uint32_t min_rows, uint32_t max_shift, uint32_t* new_bounds) {
    if (!row_bounds || !band_ms || !new_bounds || n <= 0) return FYPRT_EINVAL;
    const uint32_t H = row_bounds[n];
    double total = 0.0;
    for (int i = 0; i < n; ++i) { if (!(band_ms[i] > 0.0f) || row_bounds[i] >= row_bounds[i + 1]) return FYPRT_EINVAL; total += band_ms[i]; }
    new_bounds[0] = 0; new_bounds[n] = H;
    int band = 0; double before = 0.0;                       // cost of the bands entirely above the cursor
    for (int k = 1; k < n; ++k) {
        const double target = total * k / n;
        while (band < n - 1 && before + band_ms[band] < target) { before += band_ms[band]; ++band; }
        const double frac = (target - before) / band_ms[band];
        double row = row_bounds[band] + frac * (row_bounds[band + 1] - row_bounds[band]);
        const double lo = (double)row_bounds[k] - max_shift, hi = (double)row_bounds[k] + max_shift;
        row = std::min(std::max(row, lo), hi);
        uint32_t r = (uint32_t)std::max(0.0, row + 0.5);
        const uint32_t floor_ = new_bounds[k - 1] + min_rows, ceil_ = H - (uint32_t)(n - k) * min_rows;
        if (r < floor_) r = floor_;
        if (r > ceil_) r = ceil_;
        new_bounds[k] = r;
    }
    for (int k = 0; k < n; ++k) if (new_bounds[k] >= new_bounds[k + 1]) return FYPRT_EINVAL;      // min_rows x n exceeds the height
    return FYPRT_OK;
}

// Time of the last frame on this context (sum of its launches' hipEvent durations; synchronises the context).
int fyprt_last_frame_ms(fyprt_context* c, float* ms) {
    if (!c || !ms) return FYPRT_EINVAL;
    float part[4]; uint32_t n = 0;
    HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, sync_all(c));
    TRY(fyprt_frame_timings(c, 0, part, &n));
    *ms = part[0] + part[1] + part[2] + part[3];
    return FYPRT_OK;
}

// ------------------------------------------------------------------------------------------------ one process per GPU: RCCL
int fyprt_comm_unique_id(void* id128) {
    if (!id128) return FYPRT_EINVAL;
    if (!g_rccl.load()) { g_createError = g_rccl.err; return FYPRT_EHIP; }
    const int r = g_rccl.GetUniqueId(id128);
    if (r != 0) { g_createError = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return FYPRT_EHIP; }
    return FYPRT_OK;
}
int fyprt_comm_init_rank(fyprt_context* c, int world, int rank, const void* id128, const uint32_t* row_bounds) {
    if (!c || !id128 || !row_bounds || world <= 0 || rank < 0 || rank >= world) return FYPRT_EINVAL;
    if (c->hostOnly || c->H == 0) return c->fail(FYPRT_ESTATE, "fyprt_comm_init_rank: resize the context first");
    int at;
    if (const char* bad = bad_bands(row_bounds, world, c->H, &at)) return c->fail(FYPRT_EINVAL, std::string("fyprt_comm_init_rank") + bad);
    if (!g_rccl.load()) return c->fail(FYPRT_EHIP, g_rccl.err);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->comm) { (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
    ncclUniqueIdBytes id; std::memcpy(id.b, id128, 128);
    NCCLCHK(c, g_rccl.CommInitRank(&c->comm, world, id, rank));
    c->world = world; c->rank = rank; c->bounds.assign(row_bounds, row_bounds + world + 1);
    c->rowBegin = row_bounds[rank]; c->rowEnd = row_bounds[rank + 1]; c->rowsSet = true;
    return FYPRT_OK;
}
// New band boundaries for every rank (collective: every rank calls it with the same table, between two frames).  Rows that change
// owner take their accumulation and temporal history along (grouped ncclSend / ncclRecv), as fyprt_group_set_rows does with peer copies.
int fyprt_comm_set_rows(fyprt_context* c, const uint32_t* row_bounds) {
    if (!c || !row_bounds || !c->comm) return FYPRT_EINVAL;
    int at;
    if (const char* bad = bad_bands(row_bounds, c->world, c->H, &at)) return c->fail(FYPRT_EINVAL, std::string("fyprt_comm_set_rows") + bad);
    HIPCHK(c, hipSetDevice(c->device));
    // Between two frames for real: a pipelined ReSTIR DI frame still has Part 1 + setup of the NEXT frame in flight on the front stream,
    // and they read and write the very history rows that move here.  Everything of this context drains first, and the call returns only
    // once the rows have arrived — exactly what fyprt_group_set_rows does around its peer copies.
    HIPCHK(c, sync_all(c));
    std::vector<void*> base; std::vector<size_t> bpp;
    for (const XBuf& b : row_buffers(c, c->commLastStriped)) { base.push_back(b.p); bpp.push_back(b.bytesPerPixel); }
    TRY(comm_issue(c, comm_set_rows_ops(c->rank, c->bounds, std::vector<uint32_t>(row_bounds, row_bounds + c->world + 1), bpp, c->W), base));
    HIPCHK(c, sync_all(c));
    c->bounds.assign(row_bounds, row_bounds + c->world + 1);
    c->rowBegin = c->bounds[c->rank]; c->rowEnd = c->bounds[c->rank + 1];
    c->histDI[0] = c->histGI[0] = c->rowBegin; c->histDI[1] = c->histGI[1] = c->rowEnd;
    return FYPRT_OK;
}
int fyprt_comm_set_halo_mode(fyprt_context* c, int mode) { if (!c || mode < 0 || mode > 1) return FYPRT_EINVAL; c->commHaloMode = mode; return FYPRT_OK; }
// fyprt_group_set_interleave for one process per GPU (every rank calls it with the same value)
int fyprt_comm_set_interleave(fyprt_context* c, uint32_t stripe_rows) {
    if (!c || !c->comm) return FYPRT_EINVAL;
    if (stripe_rows != 0 && (uint64_t)stripe_rows * c->world > c->H) return c->fail(FYPRT_EINVAL, "fyprt_comm_set_interleave: fewer stripes than ranks");
    c->commStripeRows = stripe_rows;
    return FYPRT_OK;
}
void fyprt_comm_destroy(fyprt_context* c) { if (c && c->comm && g_rccl.lib) { (void)hipSetDevice(c->device); (void)sync_all(c); (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; c->haloExchange = false; } }

static int comm_exchange(fyprt_context* c, int tech, const std::vector<HaloXfer>& plan, int kind) {
    const std::vector<XBuf> bufs = exchange_buffers(c, tech, kind);
    std::vector<void*> base; std::vector<size_t> bpp;
    for (const XBuf& b : bufs) { base.push_back(b.p); bpp.push_back(b.bytesPerPixel); }
    return comm_issue(c, comm_exchange_ops(c->rank, plan, bpp, c->W), base);
}
// One frame of this rank's band (asynchronous).  Every rank of the communicator must call it with the same settings.
int fyprt_comm_render(fyprt_context* c, const fyprt_settings* s) {
    if (!c || !s) return FYPRT_EINVAL;
    if (!c->comm) return c->fail(FYPRT_ESTATE, "fyprt_comm_render before fyprt_comm_init_rank");
    const uint32_t halo = spatial_halo(s, c->world), hhalo = history_halo(s, c->world);
    const bool exchange = c->commHaloMode == 1 && (halo > 0 || hhalo > 0);
    c->rowBegin = c->bounds[c->rank]; c->rowEnd = c->bounds[c->rank + 1]; c->halo = halo; c->rowsSet = true; c->haloExchange = exchange;
    c->commLastStriped = c->commStripeRows != 0 && c->world > 1 && !is_restir(s); c->commLastStripeRows = c->commStripeRows;
    if (c->commLastStriped) TRY(fyprt_set_row_stripes(c, c->commStripeRows, (uint32_t)c->world, (uint32_t)c->rank));
    else c->stripeRows = 0;
    if (!exchange) return enqueue_frame(c, s, true);
    HIPCHK(c, hipSetDevice(c->device));
    TRY(sync_restir_normals(c, s->technique, c->stream));      // before the history travels
    if (s->use_temporal_reuse) TRY(comm_exchange(c, s->technique, halo_plan(c->bounds, hhalo, c->H, false), 1));
    extend_history_rows(c, s->technique, hhalo);
    TRY(enqueue_frame(c, s, true, 1));
    TRY(comm_exchange(c, s->technique, halo_plan(c->bounds, halo, c->H, true), 0));
    return enqueue_frame(c, s, true, 2);
}
// The image gather of the north-star design: every band's RGBA8 rows, in place in the full-size image (the context's own or the
// external one), one grouped ncclBroadcast per band on the context's stream.  root < 0: every rank ends up with the whole frame;
// root >= 0: only that rank does (ncclSend / ncclRecv).
int fyprt_comm_gather(fyprt_context* c, int root) {
    if (!c) return FYPRT_EINVAL;
    if (!c->comm) return c->fail(FYPRT_ESTATE, "fyprt_comm_gather before fyprt_comm_init_rank");
    if (root >= c->world) return c->fail(FYPRT_EINVAL, "fyprt_comm_gather: root out of range");
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t* img = c->externalImage ? c->externalImage : c->image.p;
    NCCLCHK(c, g_rccl.GroupStart());
    int bad = 0;
    for (int r = 0; r < c->world; ++r) {
        auto rows = [&](uint32_t r0, uint32_t r1) {
            uint32_t* band = img + (size_t)r0 * c->W;
            const size_t bytes = (size_t)(r1 - r0) * c->W * 4;
            int e = 0;
            if (root < 0) e = g_rccl.Broadcast(band, band, bytes, kNcclChar, r, c->comm, c->stream);
            else if (r != root) {
                if (c->rank == r) e = g_rccl.Send(band, bytes, kNcclChar, root, c->comm, c->stream);
                else if (c->rank == root) e = g_rccl.Recv(band, bytes, kNcclChar, r, c->comm, c->stream);
            }
            if (e != 0 && bad == 0) bad = e;
        };
        if (c->commLastStriped) for_each_stripe(c->H, c->commLastStripeRows, (uint32_t)c->world, (uint32_t)r, rows);      // one transfer per stripe, all in one group
        else rows(c->bounds[r], c->bounds[r + 1]);
    }
    const int endRc = g_rccl.GroupEnd();
    if (bad != 0) return c->fail(FYPRT_EHIP, std::string("fyprt_comm_gather: ") + g_rccl.GetErrorString(bad));
    NCCLCHK(c, endRc);
    return FYPRT_OK;
}

// Test hook: the transfer plan of a halo exchange (receiver, owner, first row, end row per entry); returns the number of entries.
int fyprt_halo_plan(const uint32_t* row_bounds, int n, uint32_t halo, uint32_t height, int wrap_row, uint32_t* out4, int capacity) {
    if (!row_bounds || n <= 0) return -1;
    const std::vector<HaloXfer> plan = halo_plan(std::vector<uint32_t>(row_bounds, row_bounds + n + 1), halo, height, wrap_row != 0);
    for (int k = 0; k < (int)plan.size() && k < capacity && out4; ++k) {
        out4[4 * k] = (uint32_t)plan[k].receiver; out4[4 * k + 1] = (uint32_t)plan[k].owner; out4[4 * k + 2] = plan[k].r0; out4[4 * k + 3] = plan[k].r1;
    }
    return (int)plan.size();
}

// Test hook: the point-to-point operations rank `rank` issues in one group section — kind 0: a halo exchange over `bounds` (halo rows,
// wrap row as fyprt_halo_plan); kind 1: fyprt_comm_set_rows from `bounds` to `new_bounds`.  out5 = (is_recv, peer, buffer, offset, bytes)
// per operation; returns the number of operations.  Pure host arithmetic: no device, no RCCL.
int fyprt_comm_ops(int kind, const uint32_t* bounds, const uint32_t* new_bounds, int n, uint32_t halo, uint32_t height, int wrap_row, uint32_t width,
                   int rank, const uint32_t* bytes_per_pixel, int nbuf, uint64_t* out5, int capacity) {
    if (!bounds || n <= 0 || rank < 0 || rank >= n || !bytes_per_pixel || nbuf <= 0 || (kind == 1 && !new_bounds)) return -1;
    const std::vector<uint32_t> b(bounds, bounds + n + 1);
    const std::vector<size_t> bpp(bytes_per_pixel, bytes_per_pixel + nbuf);
    const std::vector<CommOp> ops = kind == 0 ? comm_exchange_ops(rank, halo_plan(b, halo, height, wrap_row != 0), bpp, width)
                                               : comm_set_rows_ops(rank, b, std::vector<uint32_t>(new_bounds, new_bounds + n + 1), bpp, width);
    for (int k = 0; k < (int)ops.size() && k < capacity && out5; ++k) {
        out5[5 * k] = (uint64_t)ops[k].recv; out5[5 * k + 1] = (uint64_t)ops[k].peer; out5[5 * k + 2] = (uint64_t)ops[k].buf; out5[5 * k + 3] = ops[k].offset; out5[5 * k + 4] = ops[k].bytes;
    }
    return (int)ops.size();
}
