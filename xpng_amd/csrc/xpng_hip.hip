// xpng_hip.hip -- C-ABI of libxpng_hip.so (include/xpng_hip.h): context, launches, host-buffer wrappers.
// gfx950 only.  No CPU fallback: every compute entry point fails when HIP has no device.
#include "../../include/xpng_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "m1_decode.hpp"
#include "normalize.hpp"
#include "m1_encode.hpp"
#include "m2_decode.hpp"
#include "m2_encode.hpp"
#include "rans2.hpp"
#include "rans2_wide.hpp"
#include "rans1_wide.hpp"
#include "rans1_wide_dec.hpp"
#include "tile_container.hpp"
#include "top_class_cut.hpp"
#include "region.hpp"
#include "mixed.hpp"
#include "mixed_float.hpp"
#include "mixed_resize.hpp"
#include "mixed_resample.hpp"
#include "mixed_views.hpp"
#include "mixed_views_colour.hpp"
#include "mixed_views_cubic.hpp"
#include "mixed_views_blur.hpp"
#include "mixed_views_affine.hpp"
#include "mixed_views_tone.hpp"
#include "stage_from.hpp"

using namespace xpng;

static thread_local std::string g_err;
static int fail(const std::string &m) { g_err = m; return 1; }
#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(std::string(#call) + ": " + hipGetErrorString(e_));          \
    } while (0)

// One table of the context's workspace (WsTable, common.hpp): allocated, recorded and counted, or left alone when it exists.  The
// text of a failure is the one HIPCHK gave around the runtime's own allocation call with these arguments.
#define WS_GET(ptr, bytes)                                                                                                        \
    do {                                                                                                                         \
        if (hipError_t e_ = c->ws.get((void **)&(ptr), (bytes))) return fail(std::string("hipMalloc" "((void **)&" #ptr ", " #bytes "): ") + hipGetErrorString(e_)); \
    } while (0)

// extern "C" must not leak C++ exceptions (std::bad_alloc from a header that claims an absurd geometry)
#define XPNG_GUARDED(expr)                                               \
    try { return (expr); }                                               \
    catch (const std::bad_alloc &) { return fail("out of host memory"); } \
    catch (...) { return fail("unexpected C++ exception"); }

// A kernel that dereferences a device pointer nobody allocated does not fail - it FAULTS: the ROCm runtime's fault handler prints
// "Memory access fault by GPU node ..." and calls abort(), past every catch of the extern "C" entry points (that is what took
// the test process down in gpurun_out/r2_t14.log: a working tree in which the five symbol planes had just become lazily
// allocated and launch_transform, reached through the mode-2 encode, did not yet call ensure_planes).  So every launch
// sequence names the workspace buffers it is about to hand to kernels and refuses to launch when one of them is null.
#define XPNG_REQUIRE(...)                                                                                                    \
    do {                                                                                                                     \
        const void *rq_[] = {__VA_ARGS__};                                                                                   \
        for (const void *q_ : rq_)                                                                                           \
            if (!q_) return fail("internal error: a workspace buffer of this launch sequence was never allocated (one of: " #__VA_ARGS__ ")"); \
    } while (0)

// A pipelined caller keeps several contexts in flight, each on a stream of its own: with the runtime's default of 4 hardware queues
// those streams share queues, and kernels that share a queue run one after the other.  The runtime reads GPU_MAX_HW_QUEUES when it
// initialises - the first HIP call of the process - so the library asks for 32 when it is LOADED, unless the caller has chosen a
// value.  A process that has already initialised HIP before loading this library (any PyTorch process), or whose environment already
// sets the variable, keeps what it had: four queues are the common case, so the batched level-1 forms put every kernel of a call on
// the caller's ONE stream and launch the serial stages that may run beside each other as ranges of one grid (k_dec_serial,
// k_rans2_chain_all) - queue time is the step's bound there.  Only the narrow (single-image) RGBA decode and the
// level-2 decode still fork the context's side stream.  Nothing in the library reads the variable back: no code path depends on the
// queues being there.
__attribute__((constructor)) static void xpnghip_on_load(void) { (void)setenv("GPU_MAX_HW_QUEUES", "32", 0); }

extern "C" int xpnghip_abi_version(void) { return XPNGHIP_ABI_VERSION; }
extern "C" const char *xpnghip_last_error(void) { return g_err.c_str(); }
extern "C" int xpnghip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- tile table (reference compute_props_of_each_tile, libxpng.c:51-83) ---------------------------------
static void split_axis(uint64_t len, uint64_t base, uint64_t &count, uint64_t &first, uint64_t &second) {
    const uint64_t rem = len % base;
    count = len / base; first = base + rem; second = base;
    if (rem > base / 2) { count++; second = first / 2; first = second + (first & 1); }
}
// Tiles outside [r0, r1) get no plane / scratch space (a rank that encodes only its tile range of a large raster should
// not pay HBM for the rest); such a context can only be used on sub-ranges of [r0, r1).
static void build_tiles(uint64_t W, uint64_t H, std::vector<TileDesc> &out, uint64_t r0 = 0, uint64_t r1 = ~0ull) {
    uint64_t nx = 1, ny = 1, w0 = W, w1 = 0, bw = 0, h0 = H, h1 = 0, bh = 0;
    if (W * H > TILE_AREA) {
        if (W < 444) { bw = W; bh = TILE_AREA / W; }
        else if (H < 444) { bh = H; bw = TILE_AREA / H; }
        else bw = bh = 444;
        split_axis(W, bw, nx, w0, w1);
        split_axis(H, bh, ny, h0, h1);
    }
    out.clear();
    out.reserve(nx * ny);
    uint64_t pbase = 0, sbase = 0;
    for (uint64_t j = 0; j < ny; j++) {
        const uint64_t y = j == 0 ? 0 : (j == 1 ? h0 : h0 + h1 + (j - 2) * bh), th = j == 0 ? h0 : (j == 1 ? h1 : bh);
        for (uint64_t i = 0; i < nx; i++) {
            TileDesc t{};
            t.x = (uint32_t)(i == 0 ? 0 : (i == 1 ? w0 : w0 + w1 + (i - 2) * bw));
            t.w = (uint32_t)(i == 0 ? w0 : (i == 1 ? w1 : bw));
            t.y = (uint32_t)y; t.h = (uint32_t)th;
            t.n = t.w * t.h;
            t.pbase = pbase; t.sbase = sbase;
            const uint64_t idx = out.size();
            if (idx >= r0 && idx < r1) { pbase += rup(t.n + 192, 256); sbase += tile_scratch_bytes(t.n); }
            out.push_back(t);
        }
    }
}

struct xpnghip_ctx {
    int device = 0;
    uint64_t W = 0, H = 0;
    int pxsz = 0;
    uint32_t B = 1;    // images per launch (native batching: virtual tile = image * N + tile)
    uint64_t r0 = 0, r1 = 0;  // tile range this context has workspace for
    uint32_t spt = 0;  // streams per tile: 9 (+1 alpha)
    std::vector<TileDesc> tiles;  // the N tiles of ONE image (host copy); the device table has B * N entries
    uint64_t plane_img = 0, plane_stride = 0, scratch_img = 0;
    WsTable ws;  // every device allocation of the context, the decode workspace's and the host wrappers' included: ws.total is xpnghip_ctx_workspace_bytes
    TileDesc *d_tiles = nullptr;
    uint8_t *d_planes = nullptr, *d_scratch = nullptr;  // d_planes (4 or 5 symbol planes) and d_scratch (level-1 stream scratch = the decode's planes): allocated on first use
    uint32_t *d_sums = nullptr, *d_nlh = nullptr, *d_ctx_n = nullptr, *d_k_n = nullptr, *d_blk_sz = nullptr, *d_tile_sz = nullptr, *d_tile_hdr = nullptr;
    uint64_t *d_off = nullptr, *d_totals = nullptr, *d_dbg = nullptr;
    uint64_t *d_blob_len = nullptr;       // decode: B blob lengths
    uint32_t *d_status = nullptr;         // decode: bit 0 = some tile failed header validation
    std::vector<uint64_t> h_blob_len;
    const uint8_t **d_in_ptrs = nullptr;  // B raster (encode) / blob (decode) pointers
    uint8_t **d_out_ptrs = nullptr;       // B blob (encode) / raster (decode) pointers
    std::vector<const void *> h_in_ptrs;  // what d_in_ptrs / d_out_ptrs currently hold (skip the upload when unchanged)
    std::vector<void *> h_out_ptrs;
    // decode keeps its own pair of tables: a caller that alternates encode and decode on one context (a pipeline) would
    // otherwise re-upload, and synchronise its stream, on every call
    uint32_t *d_order = nullptr;          // tile indices of [r0, r1) by decreasing pixel count (TileSel::order)
    std::vector<uint32_t> order_n;        // ... and their pixel counts in that order (what top_class_cut reads)
    // ONE side stream per context, created by the first call that forks (dec_launch): the alpha branch of a narrow level-1 RGBA decode
    // and the big-alphabet chains of a level-2 decode run on it (DecodeWs::side borrows it).  The batched level-1 forms and every
    // encode stay on the caller's stream: every stream alive takes a share of the runtime's hardware queues
    hipStream_t side = nullptr;
    const uint8_t **d_dec_in_ptrs = nullptr;
    uint8_t **d_dec_out_ptrs = nullptr;
    std::vector<const void *> h_dec_in_ptrs;
    std::vector<void *> h_dec_out_ptrs;
    WPrep *d_wprep = nullptr;   // wide entropy stage: per (tile, stream) record, encoder tables, normalised frequencies
    uint8_t *d_wtab = nullptr;
    uint32_t nlh_slots = 0, nlh_generic = 0;  // records per tile in d_nlh (m1_encode.hpp); which transform form wrote them last
    uint16_t *d_wF = nullptr;
    // mode 2 (RGB slow level): allocated on first use
    bool m2_ready = false;                // ensure_m2 has allocated all of them and uploaded d_sbase2
    uint8_t *d_scratch2 = nullptr;
    uint64_t *d_sbase2 = nullptr;
    uint32_t *d_flags2 = nullptr, *d_stream_n2 = nullptr;
    M2Blk *d_blk2 = nullptr;
    M2Tile *d_mt2 = nullptr;
    M2DecTile *d_info2 = nullptr;
    uint16_t *d_tabs2 = nullptr;
    W1Prep *d_w1prep = nullptr;           // wide rANS v1 encode (rans1_wide.hpp): descriptors, encoder tables, frequencies
    uint8_t *d_w1tab = nullptr;
    uint16_t *d_w1F = nullptr;
    int stamps = 0;  // XPNG_STAMPS=1: chain kernels record s_memtime phase stamps (debug_fetch 40/41)
    uint64_t *h_total = nullptr;  // pinned, B entries
    hipStream_t stream = nullptr;
    // host-buffer wrappers keep their own device raster / blob buffers here (capacities in bytes; grown on demand, never per call)
    uint8_t *d_raster = nullptr, *d_blobs = nullptr, *d_blob_in = nullptr;
    uint64_t cap_raster = 0, cap_blobs = 0, cap_blob_in = 0;
    uint8_t *h_stage = nullptr;  // pinned host staging of a decoded band (wrappers.hpp: device -> pinned at link speed, pinned -> caller's raster by copy threads)
    uint64_t cap_stage = 0;
    uint64_t call = 0;  // id of the last host-wrapper call that used this context (wrappers.hpp: never evicted mid-call)
    DecodeWs dec;
    // region decode (region.hpp), allocated on first use: the staging raster (nimg x the largest tile-aligned bounding box of a
    // call; grown on demand), and one buffer with the work list (B * N entries) followed by B RegionCopy records
    uint8_t *d_region_stage = nullptr;
    uint64_t cap_region_stage = 0;
    uint8_t *d_region_meta = nullptr;
    std::vector<uint8_t> h_region_meta;  // what d_region_meta holds (skip the upload when unchanged)
    // mixed-size batch (xpnghip_ctx_create_mixed; mixed.hpp).  `tiles` is then the concatenation of the
    // B images' tile tables (M entries, img / pbase / sbase as on the device) and W = H = 0.  The constructor allocates what a
    // decode needs; the encode workspace follows with the first encode (ensure_mixed_encode)
    bool mixed = false;
    bool m_enc = false;                // the encode workspace exists (and d_scratch has the encode's share)
    uint64_t cap_scratch = 0;          // bytes of d_scratch
    std::vector<uint64_t> m_dims;      // B pairs {w, h}
    std::vector<uint32_t> m_first;     // B + 1 table indices: image i owns tiles [m_first[i], m_first[i + 1])
    std::vector<uint32_t> m_list;      // all M table indices by decreasing pixel count (the work list of every launch)
    uint64_t m_max_w = 0, m_max_h = 0;
    uint32_t *d_m_first = nullptr, *d_m_list = nullptr;  // the two on the device (one allocation: d_m_first)
    uint8_t *d_m_stage = nullptr;      // tight output form: staging raster at the widest image's pitch, allocated on first use
    uint64_t cap_m_stage = 0;
    // the record tables of the tight forms (mixed_records): B MixedLayout per direction - the caller's output buffers of a decode,
    // its input buffers of an encode.  A record holds the slot, the buffer, w and h: nothing that depends on the form of the call
    // (tight, layout word, dtype, constants - they only select the kernel), so the pointers are the whole cache key
    MixedLayout *d_m_out = nullptr, *d_m_in = nullptr;
    std::vector<const void *> h_m_out, h_m_in;  // the buffers the two tables hold (skip the upload when unchanged)
    ResizeRec *d_m_rect = nullptr;     // the rectangle table of a resized decode (mixed_resize.hpp): B records, uploaded by every call
    ResampleRec *d_m_rsmp = nullptr;   // ... and that of a resampled decode with filter 1 (mixed_resample.hpp), alike
    // a views decode (mixed_views.hpp): one record per view, grown when a call has more views than any before it, and the launch
    // list of the call (room for all M entries, so it never grows); both uploaded by every call
    ViewRec *d_m_views = nullptr;
    uint64_t cap_m_views = 0;          // records d_m_views has room for
    uint32_t *d_m_vlist = nullptr;
    // ... and, for a views call with colour matrices only (mixed_views_colour.hpp), one 48-byte matrix per view: grown, dropped
    // and uploaded as d_m_views is; a plain views call never allocates it
    ViewColour *d_m_vcolour = nullptr;
    uint64_t cap_m_vcolour = 0;        // matrices d_m_vcolour has room for
    // ... and, for a views call with views that blur or solarise only (mixed_views_blur.hpp), the fp32 planes of those views between
    // the two passes and one 160-byte record per such view: grown when a call needs more than any before it, dropped and uploaded as
    // d_m_views is; no other call allocates them
    float *d_m_bscratch = nullptr;
    uint64_t cap_m_bscratch = 0;       // bytes d_m_bscratch holds
    BlurRec *d_m_blur = nullptr;
    uint64_t cap_m_blur = 0;           // records d_m_blur has room for
    // ... and, for an affine views call only (mixed_views_affine.hpp), one 64-byte record per view in place of d_m_views: grown,
    // dropped and uploaded as d_m_views is; no other call allocates it
    AffineRec *d_m_affine = nullptr;
    uint64_t cap_m_affine = 0;         // records d_m_affine has room for
    // ... and, for a call with tone steps only (mixed_views_tone.hpp), one 48-byte record per view with a step and one statistics slot
    // per (such view, autocontrast or equalise step): grown and dropped as d_m_views is; the slots are zeroed on the stream by every call
    ToneRec *d_m_tone = nullptr;
    uint64_t cap_m_tone = 0;           // records d_m_tone has room for
    uint32_t *d_m_tstat = nullptr;
    uint64_t cap_m_tstat = 0;          // slots d_m_tstat has room for
    uint64_t last_tiles = 0;           // tile work items of the most recent decode launch (xpnghip_ctx_last_decode_tiles)
};

// the context's own stream, created when a call first needs it (the `stream == NULL` form of the device-resident entry points,
// and the host-buffer wrappers).  On failure nullptr, i.e. the legacy default stream: slower, still correct.
static hipStream_t ctx_stream(xpnghip_ctx *c) {
    if (!c->stream) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        if (hipSetDevice(c->device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) c->stream = nullptr;
        if (prev >= 0 && prev != c->device) (void)hipSetDevice(prev);
    }
    return c->stream;
}

extern "C" void xpnghip_ctx_destroy(xpnghip_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->ws.free_all();
    if (c->side) (void)hipStreamDestroy(c->side);
    decode_ws_free(c->dec);
    if (c->h_total) (void)hipHostFree(c->h_total);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// The encode workspace, the one statement of its 14 tables and their sizes: `entries` entries of the device tile table (B * N of an
// ordinary context, which allocates it when it is created; the M of a mixed one, which does with its first encode), `images` rasters
// per launch.  A table that exists is left alone.  Returns the name of the table whose allocation failed, or nullptr.
static const char *encode_tables(xpnghip_ctx *c, uint64_t entries, uint64_t images) {
    for (uint64_t i = c->r0; i < c->r1; i++) c->nlh_slots = std::max({c->nlh_slots, nlh_records(c->tiles[i].w, c->tiles[i].h, false), nlh_records(c->tiles[i].w, c->tiles[i].h, true)});
#define TABLE(ptr, bytes) {(void **)&c->ptr, (bytes), "c->" #ptr}
    const struct { void **slot; uint64_t bytes; const char *name; } tables[] = {
        TABLE(d_sums, entries * 16),
        TABLE(d_nlh, entries * c->nlh_slots * NLH_STRIDE * 4 + 64),  // nl histogram + last coded pixel of every transform workgroup (m1_encode.hpp)
        TABLE(d_ctx_n, entries * 9 * 4), TABLE(d_k_n, entries * 4), TABLE(d_blk_sz, entries * 10 * 4), TABLE(d_tile_sz, entries * 4),
        TABLE(d_tile_hdr, entries * 4), TABLE(d_off, (entries + images) * 8), TABLE(d_totals, images * 8), TABLE(d_wprep, entries * 10 * sizeof(WPrep)),
        TABLE(d_wtab, entries * WTAB_TILE_BYTES + 4096 + watab_bytes(entries)),  // per-tile tables, then the launch's interleaved alpha tables (rans2_wide.hpp)
        TABLE(d_wF, entries * 10 * 512), TABLE(d_in_ptrs, images * 8), TABLE(d_out_ptrs, images * 8)};
#undef TABLE
    for (const auto &t : tables) if (c->ws.get(t.slot, t.bytes) != hipSuccess) return t.name;
    return nullptr;
}

static int ctx_create_range_impl(xpnghip_ctx **out, int device, uint64_t w, uint64_t h, int pxsz, uint32_t batch, uint64_t r0, uint64_t r1);
extern "C" int xpnghip_ctx_create_range(xpnghip_ctx **out, int device, uint64_t w, uint64_t h, int pxsz, uint32_t batch,
                                        uint64_t r0, uint64_t r1) {
    XPNG_GUARDED(ctx_create_range_impl(out, device, w, h, pxsz, batch, r0, r1))
}
static int ctx_create_range_impl(xpnghip_ctx **out, int device, uint64_t w, uint64_t h, int pxsz, uint32_t batch, uint64_t r0, uint64_t r1) {
    if (!out || !w || !h || w > (1u << 24) || h > (1u << 24) || (pxsz != 3 && pxsz != 4) || batch < 1 || batch > 4096 || r0 >= r1) return fail("bad arguments");
    if (xpnghip_device_count() <= device || device < 0) return fail("no such HIP device (libxpng_hip has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    xpnghip_ctx *c = new xpnghip_ctx();
    c->device = device; c->W = w; c->H = h; c->pxsz = pxsz; c->spt = pxsz == 4 ? 10 : 9; c->B = batch;
    build_tiles(w, h, c->tiles, r0, r1);
    const uint64_t N = c->tiles.size(), VN = N * batch;
    c->r0 = r0; c->r1 = r1 < N ? r1 : N;
    const TileDesc &last = c->tiles[c->r1 - 1];
    c->plane_img = last.pbase + rup(last.n + 192, 256);
    c->scratch_img = last.sbase + tile_scratch_bytes(last.n);
    c->plane_stride = c->plane_img * batch;
    std::vector<TileDesc> all(VN);
    for (uint32_t b = 0; b < batch; b++)
        for (uint64_t i = 0; i < N; i++) {
            TileDesc t = c->tiles[i];
            t.img = b; t.pbase += b * c->plane_img; t.sbase += b * c->scratch_img;
            all[b * N + i] = t;
        }
#define ALLOC(ptr, bytes)                                                                          \
    do {                                                                                           \
        if (c->ws.get((void **)&(ptr), (bytes)) != hipSuccess) { xpnghip_ctx_destroy(c); return fail("hipMalloc failed for " #ptr); } \
    } while (0)
    ALLOC(c->d_tiles, VN * sizeof(TileDesc));
    // (the stream scratch - 7.5 B/px for a level-1 encode, 8 B/px as the decode's symbol / residual planes: one buffer of the larger
    //  size - and the symbol planes, 4 or 5 B/px, are allocated by the first call that needs them: ensure_scratch, ensure_planes)
    if (const char *name = encode_tables(c, VN, batch)) {
        xpnghip_ctx_destroy(c);
        return fail(std::string("hipMalloc failed for ") + name);
    }
#ifdef XPNG_PROBES
    ALLOC(c->d_dbg, VN * 10 * 8 * 8 * 2);  // phase stamps of the chain kernels (XPNG_STAMPS)
#endif
    ALLOC(c->d_blob_len, (uint64_t)batch * 8);
    ALLOC(c->d_status, 64);
    ALLOC(c->d_dec_in_ptrs, (uint64_t)batch * 8);
    ALLOC(c->d_dec_out_ptrs, (uint64_t)batch * 8);
    ALLOC(c->d_order, (c->r1 - c->r0) * 4);
#undef ALLOC
    {   // tiles of [r0, r1) by decreasing pixel count (stable: equal sizes stay in tile order)
        std::vector<uint32_t> ord;
        for (uint64_t i = c->r0; i < c->r1; i++) ord.push_back((uint32_t)i);
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return c->tiles[a].n > c->tiles[b].n; });
        if (hipMemcpy(c->d_order, ord.data(), ord.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { xpnghip_ctx_destroy(c); return fail("context setup failed"); }
        for (uint32_t i : ord) c->order_n.push_back(c->tiles[i].n);
    }
    c->stamps = c->d_dbg && probe_env("XPNG_STAMPS") != nullptr;  // (probe builds only)
#ifdef XPNG_PROBES
    {   // VALU burner (common.hpp)
        const uint32_t btr = (uint32_t)probe_pad("XPNG_BURN_TR"), bst = (uint32_t)probe_pad("XPNG_BURN_ST");
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_burn_tr), &btr, 4);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_burn_st), &bst, 4);
    }
#endif
    // (c->stream is created on first use, ctx_stream(): a caller that always passes its own stream never needs it, and every
    //  stream alive takes one of the runtime's hardware queues - with more streams than queues, streams share queues and serialise)
    if (hipHostMalloc((void **)&c->h_total, (uint64_t)batch * 8 + 64) != hipSuccess ||
        hipMemcpy(c->d_tiles, all.data(), VN * sizeof(TileDesc), hipMemcpyHostToDevice) != hipSuccess) {
        xpnghip_ctx_destroy(c);
        return fail("context setup failed");
    }
    *out = c;
    return 0;
}
extern "C" int xpnghip_ctx_create_batch(xpnghip_ctx **out, int device, uint64_t w, uint64_t h, int pxsz, uint32_t batch) {
    return xpnghip_ctx_create_range(out, device, w, h, pxsz, batch, 0, ~0ull);
}
extern "C" int xpnghip_ctx_create(xpnghip_ctx **out, int device, uint64_t w, uint64_t h, int pxsz) {
    return xpnghip_ctx_create_range(out, device, w, h, pxsz, 1, 0, ~0ull);
}

extern "C" uint64_t xpnghip_ctx_tile_count(const xpnghip_ctx *c) { return c ? c->tiles.size() : 0; }
extern "C" uint32_t xpnghip_ctx_batch(const xpnghip_ctx *c) { return c ? c->B : 0; }
extern "C" int xpnghip_ctx_tile(const xpnghip_ctx *c, uint64_t i, uint64_t xywh[4]) {
    if (!c || i >= c->tiles.size()) return 1;
    xywh[0] = c->tiles[i].x; xywh[1] = c->tiles[i].y; xywh[2] = c->tiles[i].w; xywh[3] = c->tiles[i].h;
    return 0;
}
extern "C" uint64_t xpnghip_ctx_blob_bound(const xpnghip_ctx *c, uint64_t t0, uint64_t t1) {
    uint64_t b = 0;
    for (uint64_t i = t0; c && i < t1 && i < c->tiles.size(); i++) b += (uint64_t)c->tiles[i].n * c->pxsz + 4;
    return b + 16;
}
extern "C" uint64_t xpnghip_ctx_workspace_bytes(const xpnghip_ctx *c) { return c ? c->ws.total : 0; }

static int check_range(const xpnghip_ctx *c, uint64_t t0, uint64_t t1) {
    if (!c) return fail("null context");
    if (c->mixed) return fail("a mixed context codes whole images only: use xpnghip_decode_mixed_device_batch / xpnghip_encode_varsize_device_batch (no tile ranges, no transform-only run)");
    if (t0 >= t1 || t1 > c->tiles.size()) return fail("bad tile range");
    if (t0 < c->r0 || t1 > c->r1) return fail("tile range outside the range this context was created for");
    return 0;
}

// upload the per-image pointer tables (only when they changed: the copy comes from pageable host memory)
static int set_ptrs(xpnghip_ctx *c, const void *const *in, void *const *outp, uint32_t nimg, hipStream_t s, bool dec = false) {
    if (nimg < 1 || nimg > c->B) return fail("batch size exceeds the context's batch");
    std::vector<const void *> &hin = dec ? c->h_dec_in_ptrs : c->h_in_ptrs;
    std::vector<void *> &hout = dec ? c->h_dec_out_ptrs : c->h_out_ptrs;
    bool same = hin.size() == nimg && hout.size() == nimg;
    for (uint32_t b = 0; same && b < nimg; b++) same = hin[b] == in[b] && hout[b] == outp[b];
    if (same) return 0;
    for (uint32_t b = 0; b < nimg; b++)
        if (((uintptr_t)(dec ? outp[b] : in[b]) & 15) || ((uintptr_t)(dec ? in[b] : outp[b]) & 3)) return fail("device buffers must be 16-byte aligned");
    HIPCHK(hipMemcpyAsync(dec ? c->d_dec_in_ptrs : c->d_in_ptrs, in, (uint64_t)nimg * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dec ? c->d_dec_out_ptrs : c->d_out_ptrs, outp, (uint64_t)nimg * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    hin.assign(in, in + nimg);
    hout.assign(outp, outp + nimg);
    return 0;
}

// the tile-major, size-sorted enumeration applies to launches over the context's whole tile range (XPNG_IMAGE_MAJOR=1: off)
static const uint32_t *order_for(const xpnghip_ctx *c, uint32_t t0, uint32_t t1) {
    return (t0 == c->r0 && t1 == c->r1 && !probe_env("XPNG_IMAGE_MAJOR")) ? c->d_order : nullptr;
}

// Level-1 stream scratch (k, block slots, context streams: 7.5 B/px, common.hpp) and the decode's symbol / residual planes
// (8 B/px: DecodeWs::arena) are ONE buffer: a context's encode intermediates are dead by the time the same context decodes.
// (A mixed context's scratch_img already spans its images, and it pays for the encode's share only from its first encode on.)
static uint64_t scratch_bytes(const xpnghip_ctx *c) {
    const uint64_t enc = c->mixed ? (c->m_enc ? c->scratch_img + 8192 : 0) : c->scratch_img * c->B + 8192, dec = 8 * c->plane_stride + (2u << 20);
    return enc > dec ? enc : dec;
}
static int ensure_scratch(xpnghip_ctx *c, hipStream_t s = nullptr) {
    const uint64_t bytes = scratch_bytes(c);
    if (c->d_scratch && c->cap_scratch >= bytes) return 0;
    if (c->d_scratch) {
        // a mixed context that decoded before its first encode, and whose encode streams need more than its decode planes (many
        // tiny images: a tile's stream scratch has ~6 KB of fixed room): once per context.  The decode places its planes again.
        // The context is a single-queue object: its earlier work is on the call's stream, its own stream or its side stream.
        // (hipFree itself may still wait for the device: xpng_hip.h says so.)
        for (hipStream_t q : {s, c->stream, c->side}) if (q) HIPCHK(hipStreamSynchronize(q));
        c->ws.drop((void **)&c->d_scratch); c->cap_scratch = 0;
        c->dec.arena = nullptr; c->dec.arena_bytes = 0; c->dec.cap_plane = 0;
    }
    WS_GET(c->d_scratch, bytes);
    c->cap_scratch = bytes;
    return 0;
}
static int ensure_arena(xpnghip_ctx *c) {
    if (c->dec.arena) return 0;
    if (ensure_scratch(c)) return 1;
    c->dec.arena = c->d_scratch; c->dec.arena_bytes = scratch_bytes(c);
    return 0;
}
// the symbol planes (nl, r, g, b, + alpha symbols for RGBA): allocated on first use
static int ensure_planes(xpnghip_ctx *c) {
    const uint64_t np = c->pxsz == 4 ? 5 : 4;  // nl, r, g, b (+ alpha symbols)
    WS_GET(c->d_planes, np * c->plane_stride + 8192);
    return 0;
}

// What an encode launch sequence enumerates.  An ordinary context: tiles [t0, t0 + cnt) of each of nimg rasters of ONE geometry,
// W * pxsz bytes per row.  A mixed context: its concatenated table as one image of M tiles (TileSel{0, M, M, 1}: vtile(j) is j or
// order[j], imglin() the table index, TileDesc::img finds the raster and the blob buffer), every raster at the call's one pitch.
struct EncSpan {
    uint32_t t0, cnt, N, nimg;   // the TileSel
    uint32_t images;             // rasters in, blob buffers and totals out
    uint64_t VN;                 // entries of the context's device tile table (what the per-tile arrays are sized from)
    uint64_t bpr, raster_bytes;  // row pitch; where the 16-byte loads of the strip transforms clamp (~0: the caller keeps 16 readable bytes behind every raster)
    const uint32_t *order;       // the size-sorted enumeration, for the kernels that use one
};
static EncSpan enc_span(const xpnghip_ctx *c, uint32_t nimg, uint32_t t0, uint32_t t1) {
    const uint64_t N = c->tiles.size();
    return EncSpan{t0, t1 - t0, (uint32_t)N, nimg, nimg, N * c->B, c->W * (uint64_t)c->pxsz, c->W * c->H * (uint64_t)c->pxsz, order_for(c, t0, t1)};
}
static EncSpan enc_span_mixed(const xpnghip_ctx *c, uint64_t bpr) {
    const uint32_t M = (uint32_t)c->tiles.size();
    return EncSpan{0, M, M, 1, c->B, M, bpr, ~0ull, probe_env("XPNG_IMAGE_MAJOR") ? nullptr : c->d_m_list};
}

// predictor chooser (pp_rgbx).  Launch only.
// (probe builds: occupancy throttles of the bandwidth kernels in the pipelined paths, bytes of unused dynamic LDS per workgroup)
template <int PXSZ>
static int launch_chooser(xpnghip_ctx *c, const EncSpan &e, hipStream_t s, size_t pad = 0) {
    const uint32_t t0 = e.t0, t1 = e.t0 + e.cnt, cnt = e.cnt, nimg = e.nimg, total = nimg * cnt;
    const TileSel sel{t0, cnt, e.N, nimg, nullptr};
    const uint64_t bpr = e.bpr;
    XPNG_REQUIRE(c->d_in_ptrs, c->d_tiles, c->d_sums);
    if (dbg_skip("chooser")) return 0;
    if (t0 == 0 && t1 == c->tiles.size()) HIPCHK(hipMemsetAsync(c->d_sums, 0, (uint64_t)nimg * sel.N * 16, s));
    else for (uint32_t b = 0; b < nimg; b++) HIPCHK(hipMemsetAsync(c->d_sums + ((uint64_t)b * sel.N + t0) * 4, 0, (uint64_t)cnt * 16, s));
    const uint32_t strips = 16;
    k_chooser<PXSZ><<<total * strips, 256, pad, s>>>(c->d_in_ptrs, bpr, c->d_tiles, sel, strips, c->d_sums);
    return 0;
}

// chooser + transform (BASELINE config 2).  Launch only; no sync.  d_in_ptrs already holds the raster pointers.
// hist: the transform also leaves the histogram of the nl plane in d_nlh (the stream lengths of the routing kernels come from it)
template <int PXSZ>
static int launch_transform(xpnghip_ctx *c, const EncSpan &e, hipStream_t s, size_t pad = 0, bool hist = false) {
    if (ensure_planes(c)) return 1;
    const uint32_t t0 = e.t0, t1 = e.t0 + e.cnt, cnt = e.cnt, nimg = e.nimg, total = nimg * cnt;
    // image-major here: these two kernels stream the rasters, and neighbouring workgroups on neighbouring rows of ONE raster
    // keep HBM pages open (measured with 64 distinct rasters: 2.25 ms per launch against 2.4-2.6 tile-major)
    const TileSel sel{t0, cnt, e.N, nimg, nullptr};
    const uint64_t bpr = e.bpr;
    uint32_t max_n = 0;
    for (uint32_t i = t0; i < t1; i++) max_n = c->tiles[i].n > max_n ? c->tiles[i].n : max_n;
    if (launch_chooser<PXSZ>(c, e, s, pad)) return 1;
    XPNG_REQUIRE(c->d_planes, c->d_nlh);
    uint32_t *nlh = hist ? c->d_nlh : nullptr;
    uint32_t max_w = 0, max_h = 0;
    for (uint32_t i = t0; i < t1; i++) { max_w = c->tiles[i].w > max_w ? c->tiles[i].w : max_w; max_h = c->tiles[i].h > max_h ? c->tiles[i].h : max_h; }
    if (PXSZ == 4 && max_w <= TR_MAXW && !probe_env("XPNG_GENERIC_TRANSFORM")) {
        const uint32_t spt_ = (max_h + TR_ROWS - 1) / TR_ROWS;
        if (!dbg_skip("transform")) k_m1_transform_rgba<<<(total * spt_ + 7) & ~7u, 256, pad, s>>>(c->d_in_ptrs, bpr, e.raster_bytes, c->d_tiles, sel, spt_, c->d_sums, c->d_planes, c->plane_stride, total * spt_, nlh, c->nlh_slots);
        c->nlh_generic = 0;
    } else if (PXSZ == 3 && max_w <= TR_MAXW && !probe_env("XPNG_GENERIC_TRANSFORM")) {
        const uint32_t spt_ = (max_h + TR_ROWS - 1) / TR_ROWS;
        k_m1_transform_rgb<<<(total * spt_ + 7) & ~7u, 256, pad, s>>>(c->d_in_ptrs, bpr, e.raster_bytes, c->d_tiles, sel, spt_, c->d_sums, c->d_planes, c->plane_stride, total * spt_, nlh, c->nlh_slots);
        c->nlh_generic = 0;
    } else {
        const uint32_t bpt = (max_n + 1024 * TG_REPS - 1) / (1024 * TG_REPS);
        k_m1_transform_generic<PXSZ><<<total * bpt, 256, 0, s>>>(c->d_in_ptrs, bpr, c->d_tiles, sel, bpt, c->d_sums, c->d_planes, c->plane_stride, nlh, c->nlh_slots);
        c->nlh_generic = 1;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int xpnghip_m1_transform_device_batch(xpnghip_ctx *c, const void *const *d_rasters, uint32_t nimg, uint64_t t0, uint64_t t1, void *stream) {
    if (check_range(c, t0, t1)) return 1;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    std::vector<void *> dummy(nimg, (void *)c->d_out_ptrs);  // no output buffers in this stage
    if (set_ptrs(c, d_rasters, dummy.data(), nimg, s)) return 1;
    const EncSpan e = enc_span(c, nimg, (uint32_t)t0, (uint32_t)t1);
    return c->pxsz == 4 ? launch_transform<4>(c, e, s, 0, true) : launch_transform<3>(c, e, s, 0, true);  // (with the nl histogram: the kernel the encode runs)
}
extern "C" int xpnghip_m1_transform_device(xpnghip_ctx *c, const void *d_raster, uint64_t t0, uint64_t t1, void *stream) {
    return xpnghip_m1_transform_device_batch(c, &d_raster, 1, t0, t1, stream);
}

template <int PXSZ>
static int launch_encode_m1(xpnghip_ctx *c, const EncSpan &e, hipStream_t s) {
    dbg_count_sequence();
    const uint32_t t0 = e.t0, t1 = e.t0 + e.cnt, cnt = e.cnt, nimg = e.nimg, total = nimg * cnt;
    const TileSel sel{t0, cnt, e.N, nimg, e.order};
    const uint64_t bpr = e.bpr;
    uint32_t max_w = 0;
    for (uint32_t i = t0; i < t1; i++) max_w = c->tiles[i].w > max_w ? c->tiles[i].w : max_w;
    const bool narrow = !wide_form((uint64_t)total * c->spt), small_wg = small_blocks((uint64_t)total * c->spt);
    static const size_t pad_tr = probe_pad("XPNG_PAD_TR"), pad_st = probe_pad("XPNG_PAD_ST"), pad_ga = probe_pad("XPNG_PAD_GA");
    if (ensure_planes(c) || ensure_scratch(c, s)) return 1;  // (before their address is taken below)
    XPNG_REQUIRE(c->d_planes, c->d_in_ptrs, c->d_out_ptrs, c->d_tiles, c->d_scratch, c->d_sums, c->d_ctx_n, c->d_k_n,
                 c->d_blk_sz, c->d_tile_sz, c->d_tile_hdr, c->d_off, c->d_totals, c->d_wprep, c->d_wtab, c->d_wF, c->h_total);
    const uint8_t *planesA = c->d_planes;
    uint8_t *const watab = c->d_wtab + ((e.VN * WTAB_TILE_BYTES + 4096 + 511) & ~511ull);
    // (A fused transform + routing kernel - no nl / r / g / b planes, 3.7 B/px less HBM traffic - existed through round 3 behind
    //  XPNG_FUSED: one long-lived 28 KB workgroup per tile, 12 % slower in the pipeline every time it was measured, and it cannot
    //  know the stream lengths before it routes.  Removed with the worst-case stream layout; git history has it.)
    if (launch_transform<PXSZ>(c, e, s, pad_tr, true)) return 1;
    // stream lengths (from the histogram of the nl plane the transform took as it wrote it) -> places of the nine context streams -> routing
    k_m1_lens<<<total, 64, 0, s>>>(c->d_nlh, c->nlh_slots, c->nlh_generic, c->d_tiles, sel, c->d_ctx_n);
    if (dbg_skip("streams")) {} else if (small_wg) k_m1_streams<PXSZ, 256><<<total, 256, pad_st, s>>>(c->d_in_ptrs, bpr, c->d_tiles, sel, c->d_planes, c->plane_stride, c->d_scratch, c->d_ctx_n, c->d_k_n);
    else k_m1_streams<PXSZ, 1024><<<total, 1024, 0, s>>>(c->d_in_ptrs, bpr, c->d_tiles, sel, c->d_planes, c->plane_stride, c->d_scratch, c->d_ctx_n, c->d_k_n);
    if (narrow) {
        // one wave per (tile, stream): fewer instructions per step (scalar cursors), best latency while every pair gets its own wave slot
        k_rans2_encode<<<total * c->spt, 64, 0, s>>>(c->d_tiles, sel, 0, c->spt, planesA, c->plane_stride, c->d_scratch, c->d_ctx_n, c->d_blk_sz, nullptr, c->stamps ? c->d_dbg : nullptr);
    } else {
        // every lane a chain: prep -> chains -> finish, all on the caller's stream.  ONE preparation launch over every stream of
        // every tile, and ONE chain launch whose grid holds the alpha class (RGBA) in front of the context classes
        // (k_rans2_chain_all, rans2_wide.hpp: why).  (Through round 4 the alpha streams were prepared and chained on a side stream
        // behind the transform, beside the routing kernel and the context chains.)
        // (Size classes of the alpha chains on a THIRD STREAM - 17 of 81 tiles' alpha streams a wavefront each, whole blocks by
        //  k_rans2_encode - lost in round 4: DESIGN.md 6, profiles/r04_experiments.txt.  The top class below is a range of the same
        //  grid: no stream, no event, the largest tile class only.)
        // (probe builds: a knocked-out preparation narrows the launch to the other class; a knocked-out chain class gets no workgroups)
        // The top class (top_class_cut.hpp): the alpha streams of the biggest tiles of a size-sorted launch - work items [0, n1) -
        // get a wavefront each in front of the wide alpha groups, which carry the work items from n1 on; k_rans2_prep leaves their
        // tables in the layout that role reads.  (probe builds: chain_a1 knocks the narrow role out, chain_a the wide one.)
        uint32_t n1 = PXSZ == 4 && e.order && !c->mixed && !probe_env("XPNG_NO_TOP_CLASS") ? top_class_cut(c->order_n.data(), (uint32_t)c->order_n.size(), nimg) * nimg : 0u;
        if (n1 >= total) n1 = 0;
        const uint32_t pa = PXSZ == 4 && !dbg_skip("prep_a") ? 1u : 0u, pc = dbg_skip("prep_c") ? 0u : 9u;
        if (pa + pc) k_rans2_prep<<<total * (pa + pc), 64, 0, s>>>(c->d_tiles, sel, pc ? 0 : 9, pa + pc, planesA, c->plane_stride, c->d_scratch, c->d_ctx_n, c->d_blk_sz, c->d_wprep, c->d_wtab, c->d_wF, n1, watab);
        const uint32_t n1groups = dbg_skip("chain_a1") ? 0u : n1;
        const uint32_t agroups = PXSZ == 4 && !dbg_skip("chain_a") ? (total - n1 + 31) / 32 : 0u, cgroups = dbg_skip("chain_c") ? 0u : ((total + 31) / 32) * 9;
        if (n1groups + agroups + cgroups) k_rans2_chain_all<<<n1groups + agroups + cgroups, 64, chain_all_lds_bytes() + probe_pad("XPNG_PAD_CHAIN"), s>>>(c->d_tiles, sel, total, planesA, c->plane_stride, c->d_scratch, c->d_ctx_n, c->d_wprep, c->d_wtab, watab, n1groups, agroups, n1);
        if (!dbg_skip("finish")) k_rans2_finish<<<total * c->spt, 64, 0, s>>>(c->d_tiles, sel, c->spt, planesA, c->plane_stride, c->d_scratch, c->d_ctx_n, c->d_blk_sz, c->d_wprep, c->d_wF);
    }
    k_tile_sizes<<<(total + 255) / 256, 256, 0, s>>>(c->d_tiles, sel, total, PXSZ, c->spt, c->d_sums, c->d_k_n, c->d_blk_sz, c->d_tile_sz, c->d_tile_hdr);
    if (c->mixed) k_tile_offsets_seg<<<e.images, 256, 0, s>>>(c->d_tile_sz, c->d_m_first, c->d_off, c->d_totals);  // (per image over its own span of the table)
    else k_tile_offsets<<<nimg, 256, 0, s>>>(c->d_tile_sz, cnt, c->d_off, c->d_totals);
    if (!dbg_skip("gather")) k_tile_gather<<<total, 256, pad_ga, s>>>(c->d_in_ptrs, bpr, PXSZ, c->d_tiles, sel, c->spt, c->d_scratch, c->d_k_n, c->d_ctx_n, c->d_blk_sz, c->d_tile_hdr, c->d_off, c->d_out_ptrs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_total, c->d_totals, (uint64_t)e.images * 8, hipMemcpyDeviceToHost, s));
    return 0;
}

static int ensure_m2(xpnghip_ctx *c) {
    if (c->m2_ready) return 0;  // (every table and the upload: a call after a failed attempt completes the group)
    const uint64_t N = c->tiles.size(), VN = c->mixed ? N : N * c->B;  // (a mixed context's table already holds every image)
    std::vector<uint64_t> sb(VN);
    uint64_t o = 0;
    for (uint64_t v = 0; v < VN; v++) { sb[v] = o; if (v % N >= c->r0 && v % N < c->r1) o += m2_tile_scratch(c->tiles[v % N].n); }
    // (d_flags2 and d_mt2 are the encode's: a mixed context allocates them with its first level-2 encode, launch_encode_m2)
    auto get = [&](void **p, uint64_t bytes) { return c->ws.get(p, bytes) == hipSuccess; };
    if (!get((void **)&c->d_scratch2, o + 8192) || !get((void **)&c->d_sbase2, VN * 8) || (!c->mixed && !get((void **)&c->d_flags2, VN * 4)) ||
        !get((void **)&c->d_stream_n2, VN * M2_SLOTS * 4) || !get((void **)&c->d_blk2, VN * M2_SLOTS * sizeof(M2Blk)) ||
        (!c->mixed && !get((void **)&c->d_mt2, VN * sizeof(M2Tile))) || !get((void **)&c->d_info2, VN * sizeof(M2DecTile)) ||
        !get((void **)&c->d_tabs2, VN * M2_SLOTS * 512))
        return fail("hipMalloc failed (mode-2 workspace)");
    HIPCHK(hipMemcpy(c->d_sbase2, sb.data(), VN * 8, hipMemcpyHostToDevice));
    c->m2_ready = true;
    return 0;
}

// mode 2: RGB only (libxpng.c:755 sends RGBA to mode 1 before the tile stage)
static int launch_encode_m2(xpnghip_ctx *c, const EncSpan &e, hipStream_t s) {
    if (ensure_m2(c)) return 1;
    const uint32_t t0 = e.t0, t1 = e.t0 + e.cnt, cnt = e.cnt, nimg = e.nimg, total = nimg * cnt;
    const TileSel sel{t0, cnt, e.N, nimg, nullptr};
    const uint64_t bpr = e.bpr, VN = e.VN;
    if (c->mixed && (c->ws.get((void **)&c->d_flags2, VN * 4) != hipSuccess || c->ws.get((void **)&c->d_mt2, VN * sizeof(M2Tile)) != hipSuccess))
        return fail("hipMalloc failed (mode-2 encode workspace)");
    uint32_t max_n = 0;
    for (uint32_t i = t0; i < t1; i++) max_n = c->tiles[i].n > max_n ? c->tiles[i].n : max_n;
    XPNG_REQUIRE(c->d_scratch2, c->d_sbase2, c->d_flags2, c->d_stream_n2, c->d_blk2, c->d_mt2, c->d_in_ptrs, c->d_out_ptrs, c->d_tiles, c->d_sums, c->d_tile_sz, c->d_off,
                 c->d_totals, c->h_total);
    HIPCHK(hipMemsetAsync(c->d_flags2, 0, VN * 4, s));
    HIPCHK(hipMemsetAsync(c->d_stream_n2, 0, VN * M2_SLOTS * 4, s));
    HIPCHK(hipMemsetAsync(c->d_blk2, 0, VN * M2_SLOTS * sizeof(M2Blk), s));
    k_m2_classify<<<total * 16, 256, 0, s>>>(c->d_in_ptrs, bpr, c->d_tiles, sel, 16, c->d_flags2);
    if (launch_transform<3>(c, e, s, 0, true)) return 1;  // chooser (PXSZ = 3, libxpng.c:663) + residual planes (allocates them on first use) + nl histogram
    XPNG_REQUIRE(c->d_planes);
    k_m2_count<<<total, 64, 0, s>>>(c->d_tiles, sel, c->d_flags2, c->d_nlh, c->nlh_slots, c->nlh_generic, c->d_stream_n2);  // stream lengths -> where every stream goes
    if (small_blocks((uint64_t)total * M2_STREAMS)) k_m2_streams<256><<<total, 256, 0, s>>>(c->d_tiles, sel, c->d_flags2, c->d_planes, c->plane_stride, c->d_scratch2, c->d_sbase2, c->d_stream_n2);
    else k_m2_streams<1024><<<total, 1024, 0, s>>>(c->d_tiles, sel, c->d_flags2, c->d_planes, c->plane_stride, c->d_scratch2, c->d_sbase2, c->d_stream_n2);
    const uint32_t gbpt = (max_n + 256 * M2_GRAY_REPS - 1) / (256 * M2_GRAY_REPS);
    k_m2_gray_syms<<<total * gbpt, 256, 0, s>>>(c->d_in_ptrs, bpr, c->d_tiles, sel, gbpt, c->d_flags2, c->d_scratch2, c->d_sbase2, c->d_stream_n2);
    if (!wide_form((uint64_t)total * M2_STREAMS)) {
        k_rans1_encode<<<total * M2_SLOTS, 64, 0, s>>>(c->d_tiles, sel, c->d_flags2, c->d_scratch2, c->d_sbase2, c->d_stream_n2, c->d_blk2);
    } else {  // every lane a chain: prep -> chains (small and big alphabets) -> finish
        if (c->ws.get((void **)&c->d_w1prep, VN * M2_SLOTS * sizeof(W1Prep)) != hipSuccess ||
            c->ws.get((void **)&c->d_w1tab, VN * M2_SLOTS * W1_TAB_BYTES) != hipSuccess ||
            c->ws.get((void **)&c->d_w1F, VN * M2_SLOTS * 512) != hipSuccess)
            return fail("hipMalloc failed (mode-2 wide encode workspace)");
        XPNG_REQUIRE(c->d_w1prep, c->d_w1tab, c->d_w1F);
        k_rans1_prep<<<total * M2_SLOTS, 64, 0, s>>>(c->d_tiles, sel, c->d_flags2, c->d_scratch2, c->d_sbase2, c->d_stream_n2, c->d_blk2, c->d_w1prep, c->d_w1tab, c->d_w1F);
        k_rans1_chain<true><<<((total + 15) / 16) * W1_BIG_SLOTS, 64, rans1_chain_lds_bytes<true>(), s>>>(c->d_tiles, sel, total, c->d_scratch2, c->d_sbase2, c->d_stream_n2, c->d_w1prep, c->d_w1tab);
        k_rans1_chain<false><<<((total + 31) / 32) * W1_SMALL_SLOTS, 64, rans1_chain_lds_bytes<false>(), s>>>(c->d_tiles, sel, total, c->d_scratch2, c->d_sbase2, c->d_stream_n2, c->d_w1prep, c->d_w1tab);
        k_rans1_finish<<<total * M2_SLOTS, 64, 0, s>>>(c->d_tiles, sel, c->d_scratch2, c->d_sbase2, c->d_stream_n2, c->d_blk2, c->d_w1prep, c->d_w1F);
    }
    k_m2_select<<<(total + 255) / 256, 256, 0, s>>>(c->d_tiles, sel, total, c->d_flags2, c->d_blk2, c->d_mt2, c->d_tile_sz);
    k_m2_bits<<<total, 256, 0, s>>>(c->d_in_ptrs, bpr, c->d_tiles, sel, c->d_mt2, c->d_blk2, c->d_scratch2, c->d_sbase2, c->d_stream_n2);
    if (c->mixed) k_tile_offsets_seg<<<e.images, 256, 0, s>>>(c->d_tile_sz, c->d_m_first, c->d_off, c->d_totals);
    else k_tile_offsets<<<nimg, 256, 0, s>>>(c->d_tile_sz, cnt, c->d_off, c->d_totals);
    k_m2_gather<<<total, 256, 0, s>>>(c->d_in_ptrs, bpr, c->d_tiles, sel, c->d_sums, c->d_mt2, c->d_blk2, c->d_scratch2, c->d_sbase2, c->d_off, c->d_out_ptrs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_total, c->d_totals, (uint64_t)e.images * 8, hipMemcpyDeviceToHost, s));
    return 0;
}

// The end of every encode call: the launch sequence of the mode and pixel size, and the blob lengths for a caller that waits for them.
static int enc_finish(xpnghip_ctx *c, int mode, const EncSpan &e, uint32_t nimg, uint64_t *blobs_len, hipStream_t s) {
    const int rc = mode == 2 ? launch_encode_m2(c, e, s) : c->pxsz == 4 ? launch_encode_m1<4>(c, e, s) : launch_encode_m1<3>(c, e, s);
    if (rc) return rc;
    if (blobs_len) {
        HIPCHK(hipStreamSynchronize(s));
        for (uint32_t b = 0; b < nimg; b++) blobs_len[b] = c->h_total[b];
    }
    return 0;
}
extern "C" int xpnghip_encode_device_batch(xpnghip_ctx *c, int mode, const void *const *d_rasters, uint32_t nimg, uint64_t t0,
                                           uint64_t t1, void *const *d_blobs, uint64_t *blobs_len, void *stream) {
    if (check_range(c, t0, t1)) return 1;
    if (mode != 1 && mode != 2) return fail("tile mode must be 1 or 2");
    if (mode == 2 && c->pxsz != 3) return fail("mode 2 codes RGB only (the driver sends RGBA to mode 1, libxpng.c:755)");
    if (c->pxsz == 4)
        for (uint64_t i = t0; i < t1; i++)
            if (c->tiles[i].w < 4 || c->tiles[i].h < 4) return fail("RGBA tile narrower than 4 px: undefined in the reference; store level 7");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    if (set_ptrs(c, d_rasters, d_blobs, nimg, s)) return 1;
    const EncSpan e = enc_span(c, nimg, (uint32_t)t0, (uint32_t)t1);
    return enc_finish(c, mode, e, nimg, blobs_len, s);
}
extern "C" int xpnghip_encode_device(xpnghip_ctx *c, int mode, const void *d_raster, uint64_t t0, uint64_t t1,
                                     void *d_blobs, uint64_t *blobs_len, void *stream) {
    return xpnghip_encode_device_batch(c, mode, &d_raster, 1, t0, t1, &d_blobs, blobs_len, stream);
}
extern "C" uint64_t xpnghip_ctx_last_blobs_len(xpnghip_ctx *c) { return c ? c->h_total[0] : 0; }
extern "C" uint64_t xpnghip_ctx_last_blobs_len_at(xpnghip_ctx *c, uint32_t img) { return c && img < c->B ? c->h_total[img] : 0; }

// What every decode launch sequence does before its kernels: pointer tables, blob lengths, status word, workspaces.
static int dec_prepare(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                       void *const *d_rasters, hipStream_t s) {
    if (set_ptrs(c, d_blobs, d_rasters, nimg, s, true)) return 1;
    if (!blobs_len) return fail("blob lengths are required (tile headers are validated against them)");
    if (c->h_blob_len.size() != nimg || memcmp(c->h_blob_len.data(), blobs_len, (size_t)nimg * 8) != 0) {
        HIPCHK(hipMemcpyAsync(c->d_blob_len, blobs_len, (uint64_t)nimg * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        c->h_blob_len.assign(blobs_len, blobs_len + nimg);
    }
    HIPCHK(hipMemsetAsync(c->d_status, 0, 4, s));
    if (ensure_arena(c)) return 1;
    XPNG_REQUIRE(c->d_dec_in_ptrs, c->d_dec_out_ptrs, c->d_blob_len, c->d_status, c->d_tiles, c->dec.arena);
    if (mode == 2) {
        if (ensure_m2(c)) return 1;
        XPNG_REQUIRE(c->d_info2, c->d_blk2, c->d_tabs2, c->d_scratch2, c->d_sbase2, c->d_stream_n2);
    }
    return 0;
}

// The one description of a decode launch (DecodeJob, m1_decode.hpp), and the launch.  The tile set is the range [t0, t1) of every
// image, or - a region decode - `list`: virtual tiles (image * N + tile), resident on the device as d_list, decoded into rasters W
// pixels wide.
static int dec_launch(xpnghip_ctx *c, int mode, uint32_t nimg, uint64_t W, const uint64_t *tile_off, hipStream_t s, uint32_t t0, uint32_t t1,
                      const std::vector<uint32_t> *list = nullptr, const uint32_t *d_list = nullptr, uint64_t bpr = 0) {
    const uint64_t N = c->tiles.size();
    DecodeJob j{};
    // (a mixed context: ONE table of N = M entries that already spans the images; the size walk follows img_first)
    if (c->mixed) { j.img_first = c->d_m_first; j.img_n = nimg; j.bpr = bpr; }
    j.B = c->mixed ? 1 : nimg; j.n_tiles = N; j.plane = c->plane_stride; j.W = W; j.pxsz = c->pxsz;
    j.min_w = ~0u;
    auto scan = [&](const TileDesc &t) { j.max_w = std::max(j.max_w, t.w); j.max_h = std::max(j.max_h, t.h); j.min_w = std::min(j.min_w, t.w); };
    if (list) for (uint32_t v : *list) scan(c->tiles[v % N]);
    else for (uint32_t i = t0; i < t1; i++) scan(c->tiles[i]);
    j.t0 = t0; j.t1 = t1;
    j.order = list ? nullptr : order_for(c, t0, t1);
    j.list = d_list; j.list_n = list ? (uint32_t)list->size() : 0u;
    j.tiles = c->d_tiles; j.blobs = c->d_dec_in_ptrs; j.blob_len = c->d_blob_len; j.rasters = c->d_dec_out_ptrs; j.status = c->d_status;
    j.tile_off = tile_off;
    j.s = s;
    c->last_tiles = j.total();
    j.stamps = c->stamps && !list ? c->d_dbg + N * c->B * 80 : nullptr;
    // the side stream, for the forms that fork one: level 2, and the narrow level-1 RGBA form (the wide form has no second stream)
    if (mode == 2 || (c->pxsz == 4 && !decode_m1_plan(j).wide)) {
        if (!c->side) HIPCHK(chain_stream_create(&c->side));
        c->dec.side = probe_env("XPNG_ONE_STREAM") ? s : c->side;  // (probe builds: every kernel of the context on the caller's stream)
    }
    if (mode == 2) return decode_m2_launch(c->dec, c->ws, j, M2DecBufs{c->d_info2, c->d_blk2, c->d_tabs2, c->d_scratch2, c->d_sbase2, c->d_stream_n2}, g_err);
    return decode_m1_launch(c->dec, c->ws, j, g_err);
}

extern "C" int xpnghip_decode_device_batch(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                           const uint64_t *tile_off, uint64_t t0, uint64_t t1, void *const *d_rasters, void *stream) {
    if (check_range(c, t0, t1)) return 1;
    if (mode != 1 && mode != 2) return fail("tile mode must be 1 or 2");
    if (mode == 2 && c->pxsz != 3) return fail("mode 2 codes RGB only");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    if (dec_prepare(c, mode, d_blobs, blobs_len, nimg, d_rasters, s)) return 1;
    return dec_launch(c, mode, nimg, c->W, tile_off, s, (uint32_t)t0, (uint32_t)t1);
}
extern "C" int xpnghip_decode_device(xpnghip_ctx *c, int mode, const void *d_blobs, uint64_t blobs_len,
                                     const uint64_t *tile_off, uint64_t t0, uint64_t t1, void *d_raster, void *stream) {
    return xpnghip_decode_device_batch(c, mode, &d_blobs, &blobs_len, 1, tile_off, t0, t1, &d_raster, stream);
}
// ---- region decode (region.hpp) ----------------------------------------------------------------
extern "C" int xpnghip_region_tiles(uint64_t w, uint64_t h, const uint64_t rect[4], uint32_t *tiles, int cap) {
    try {
        if (!w || !h || w > (1u << 24) || h > (1u << 24) || !rect || !region_valid(w, h, rect)) return -1;
        std::vector<TileDesc> all;
        build_tiles(w, h, all);
        std::vector<uint32_t> sel;
        region_select(all, rect, sel);
        if (cap < 0 || sel.size() > (size_t)cap || (!tiles && !sel.empty())) return -1;
        std::copy(sel.begin(), sel.end(), tiles);
        return (int)sel.size();
    } catch (...) { return -1; }
}

static int region_batch_impl(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                             const uint64_t *tile_off, const uint64_t *rects, void *const *d_outs, uint64_t out_bpr, void *stream) {
    // every argument is checked before anything reaches the device: a rejected call writes nothing
    if (!c) return fail("null context");
    if (c->mixed) return fail("region decode: a mixed context decodes whole images only (no crops)");
    if (mode != 1 && mode != 2) return fail("tile mode must be 1 or 2");
    if (mode == 2 && c->pxsz != 3) return fail("mode 2 codes RGB only");
    if (nimg < 1 || nimg > c->B) return fail("batch size exceeds the context's batch");
    if (c->r0 != 0 || c->r1 != c->tiles.size()) return fail("region decode needs a context over the whole tile table");
    if (!d_blobs || !blobs_len || !rects || !d_outs) return fail("null argument");
    const uint64_t N = c->tiles.size(), px = (uint64_t)c->pxsz;
    for (uint32_t i = 0; i < nimg; i++) {
        const uint64_t *r = rects + 4ull * i;
        if (!region_valid(c->W, c->H, r))
            return fail("bad region of image " + std::to_string(i) + ": {" + std::to_string(r[0]) + ", " + std::to_string(r[1]) + ", " + std::to_string(r[2]) + ", " +
                        std::to_string(r[3]) + "} is empty or leaves the " + std::to_string(c->W) + " x " + std::to_string(c->H) + " image");
        if (out_bpr < r[2] * px) return fail("out_bpr is smaller than a row of the region of image " + std::to_string(i));
        if (!d_outs[i]) return fail("null output buffer");
    }
    // the selected tiles of every image and their tile-aligned bounding boxes
    std::vector<uint32_t> list, sel;
    std::vector<uint64_t> box(4ull * nimg);  // X0, Y0, X1, Y1
    uint64_t bw = 0, bh = 0, max_rows = 0;
    for (uint32_t i = 0; i < nimg; i++) {
        region_select(c->tiles, rects + 4ull * i, sel);
        uint64_t *b = &box[4ull * i];
        b[0] = b[1] = ~0ull; b[2] = b[3] = 0;
        for (uint32_t t : sel) {
            const TileDesc &d = c->tiles[t];
            b[0] = std::min<uint64_t>(b[0], d.x); b[1] = std::min<uint64_t>(b[1], d.y);
            b[2] = std::max<uint64_t>(b[2], (uint64_t)d.x + d.w); b[3] = std::max<uint64_t>(b[3], (uint64_t)d.y + d.h);
            list.push_back((uint32_t)(i * N + t));
        }
        bw = std::max(bw, b[2] - b[0]); bh = std::max(bh, b[3] - b[1]);
        max_rows = std::max(max_rows, rects[4ull * i + 3]);
    }
    // biggest tiles first (equal sizes keep their order): neighbouring work items of the wide kernels get chains of equal length.
    // List launches run unsplit.
    std::stable_sort(list.begin(), list.end(), [&](uint32_t a, uint32_t b) { return c->tiles[a % N].n > c->tiles[b % N].n; });
    // staging: image i's box at pitch sbpr in slot i; its virtual base (base - Y0 * sbpr - X0 * pxsz) is 16-byte aligned, so every
    // pixel lands at the alignment it has in a whole raster of that pitch
    const uint64_t sbpr = bw * px, slot = rup(bh * sbpr + 16, 256);
    if (c->cap_region_stage < slot * nimg) {
        if (c->d_region_stage) {
            HIPCHK(hipSetDevice(c->device));
            HIPCHK(hipDeviceSynchronize());  // (an earlier call's kernels may still use the old buffer)
            c->ws.drop((void **)&c->d_region_stage); c->cap_region_stage = 0;
        }
        HIPCHK(hipSetDevice(c->device));
        WS_GET(c->d_region_stage, slot * nimg);
        c->cap_region_stage = slot * nimg;
    }
    if (!c->d_region_meta) {
        HIPCHK(hipSetDevice(c->device));
        const uint64_t bytes = rup((uint64_t)c->B * N * 4, 16) + (uint64_t)c->B * sizeof(RegionCopy);
        WS_GET(c->d_region_meta, bytes);
    }
    std::vector<void *> vbase(nimg);
    std::vector<RegionCopy> rc(nimg);
    for (uint32_t i = 0; i < nimg; i++) {
        const uint64_t *b = &box[4ull * i], *r = rects + 4ull * i;
        const uint64_t rel = b[1] * sbpr + b[0] * px, base = i * slot + (rel & 15);
        vbase[i] = c->d_region_stage + base - rel;
        rc[i] = RegionCopy{base + (r[1] - b[1]) * sbpr + (r[0] - b[0]) * px, (uint8_t *)d_outs[i], (uint32_t)(r[2] * px), (uint32_t)r[3]};
    }
    const uint64_t list_bytes = rup((uint64_t)list.size() * 4, 16);
    std::vector<uint8_t> meta(list_bytes + nimg * sizeof(RegionCopy), 0);
    memcpy(meta.data(), list.data(), list.size() * 4);
    memcpy(meta.data() + list_bytes, rc.data(), nimg * sizeof(RegionCopy));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    if (meta != c->h_region_meta) {  // (pageable host memory: the copy is staged synchronously anyway)
        c->h_region_meta.clear();
        HIPCHK(hipMemcpyAsync(c->d_region_meta, meta.data(), meta.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        c->h_region_meta.swap(meta);
    }
    const uint32_t *d_list = reinterpret_cast<const uint32_t *>(c->d_region_meta);
    const RegionCopy *d_rc = reinterpret_cast<const RegionCopy *>(c->d_region_meta + list_bytes);
    if (dec_prepare(c, mode, d_blobs, blobs_len, nimg, vbase.data(), s)) return 1;
    XPNG_REQUIRE(c->d_region_stage, c->d_region_meta);
    const int rc_launch = dec_launch(c, mode, nimg, bw, tile_off, s, 0, (uint32_t)N, &list, d_list);
    if (rc_launch) return rc_launch;
    k_region_copy<<<dim3((uint32_t)((max_rows + RC_ROWS - 1) / RC_ROWS), nimg), 256, 0, s>>>(d_rc, c->d_region_stage, sbpr, out_bpr);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int xpnghip_decode_region_device_batch(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                  const uint64_t *tile_off, const uint64_t *rects, void *const *d_outs, uint64_t out_bpr, void *stream) {
    XPNG_GUARDED(region_batch_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, rects, d_outs, out_bpr, stream))
}

// ---- mixed-size batch decode (mixed.hpp) ---------------------------------------------------------
static uint64_t tile_count_for(uint64_t W, uint64_t H);  // wrappers.hpp

static int ctx_create_mixed_impl(xpnghip_ctx **out, int device, const uint64_t *dims, uint32_t nimg, int pxsz) {
    if (!out || !dims || (pxsz != 3 && pxsz != 4)) return fail("bad arguments");
    if (nimg < 1 || nimg > 4096) return fail("a mixed context holds 1 .. 4096 images");
    uint64_t M = 0;
    for (uint32_t i = 0; i < nimg; i++) {
        const uint64_t w = dims[2ull * i], h = dims[2ull * i + 1];
        if (!w || !h || w > (1u << 24) || h > (1u << 24))
            return fail("bad size of image " + std::to_string(i) + ": " + std::to_string(w) + " x " + std::to_string(h) + " (each side must be 1 .. 16777216)");
        M += tile_count_for(w, h);
        if (M > 0xFFFFFFFFull) return fail("too many tiles: the concatenated tile table of a mixed context must fit in 32 bits");
    }
    if (xpnghip_device_count() <= device || device < 0) return fail("no such HIP device (libxpng_hip has no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    xpnghip_ctx *c = new xpnghip_ctx();
    c->device = device; c->pxsz = pxsz; c->spt = pxsz == 4 ? 10 : 9; c->B = nimg; c->mixed = true;
    c->m_dims.assign(dims, dims + 2ull * nimg);
    c->m_first.resize((size_t)nimg + 1);
    c->tiles.reserve(M);
    std::vector<TileDesc> one;
    uint64_t pbase = 0, sbase = 0;
    for (uint32_t i = 0; i < nimg; i++) {
        build_tiles(dims[2ull * i], dims[2ull * i + 1], one);
        c->m_first[i] = (uint32_t)c->tiles.size();
        const TileDesc &last = one.back();
        const uint64_t plane_i = last.pbase + rup(last.n + 192, 256), scratch_i = last.sbase + tile_scratch_bytes(last.n);
        for (TileDesc t : one) { t.img = i; t.pbase += pbase; t.sbase += sbase; c->tiles.push_back(t); }
        pbase += plane_i; sbase += scratch_i;  // (continue across images, as b * plane_img and b * scratch_img do in a uniform batch)
        c->m_max_w = std::max(c->m_max_w, dims[2ull * i]); c->m_max_h = std::max(c->m_max_h, dims[2ull * i + 1]);
    }
    c->m_first[nimg] = (uint32_t)M;
    c->r0 = 0; c->r1 = M;
    c->plane_img = c->plane_stride = pbase;  // the symbol / residual planes of the WHOLE batch (the decode arena is 8 of them)
    c->scratch_img = sbase;
    c->m_list.resize(M);
    for (uint64_t i = 0; i < M; i++) c->m_list[i] = (uint32_t)i;
    // biggest tiles first (equal sizes keep table order): neighbouring work items of the wide kernels get chains of equal length
    std::stable_sort(c->m_list.begin(), c->m_list.end(), [&](uint32_t a, uint32_t b) { return c->tiles[a].n > c->tiles[b].n; });
    const uint64_t first_bytes = rup(((uint64_t)nimg + 1) * 4, 16);
    std::vector<uint8_t> meta(first_bytes + M * 4, 0);
    memcpy(meta.data(), c->m_first.data(), ((size_t)nimg + 1) * 4);
    memcpy(meta.data() + first_bytes, c->m_list.data(), M * 4);
    auto alloc = [&](void **p, uint64_t bytes) { return c->ws.get(p, bytes) == hipSuccess; };
    // what a decode needs, sized from M and nimg; planes / arena, decode tables and level-2 tables follow on first use (ensure_arena,
    // decode_ws_prepare, ensure_m2), sized from M and the summed plane lengths too.  The encode workspace: ensure_mixed_encode.
    if (!alloc((void **)&c->d_tiles, M * sizeof(TileDesc)) || !alloc((void **)&c->d_blob_len, (uint64_t)nimg * 8) || !alloc((void **)&c->d_status, 64) ||
        !alloc((void **)&c->d_dec_in_ptrs, (uint64_t)nimg * 8) || !alloc((void **)&c->d_dec_out_ptrs, (uint64_t)nimg * 8) ||
        !alloc((void **)&c->d_m_first, meta.size()) || hipHostMalloc((void **)&c->h_total, (uint64_t)nimg * 8 + 64) != hipSuccess ||
        hipMemcpy(c->d_tiles, c->tiles.data(), M * sizeof(TileDesc), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_m_first, meta.data(), meta.size(), hipMemcpyHostToDevice) != hipSuccess) {
        xpnghip_ctx_destroy(c);
        return fail("mixed context setup failed (hipMalloc / upload)");
    }
    memset(c->h_total, 0, (size_t)nimg * 8 + 64);
    c->d_m_list = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(c->d_m_first) + first_bytes);
    *out = c;
    return 0;
}
extern "C" int xpnghip_ctx_create_mixed(xpnghip_ctx **out, int device, const uint64_t *dims, uint32_t nimg, int pxsz) {
    XPNG_GUARDED(ctx_create_mixed_impl(out, device, dims, nimg, pxsz))
}
extern "C" uint64_t xpnghip_ctx_mixed_first_tile(const xpnghip_ctx *c, uint32_t image) {
    return c && c->mixed && image < c->m_first.size() ? c->m_first[image] : ~0ull;
}

// ---- layouts of the caller's buffers (XPNGHIP_LAYOUT_*; mixed.hpp) --------------------------------
extern "C" int xpnghip_layout_channels(uint32_t layout, int pxsz) {
    const uint32_t ch = (layout >> 8) & 0xFu;
    if ((layout & ~(XPNGHIP_LAYOUT_PLANAR | XPNGHIP_LAYOUT_BGR | 0xF00u)) || (ch != 0 && ch != 3 && ch != 4) || (pxsz != 3 && pxsz != 4)) return -1;
    return ch ? (int)ch : pxsz;
}
static std::string layout_hex(uint32_t layout) {
    char b[16];
    snprintf(b, sizeof b, "0x%x", layout);
    return b;
}
// The per-image records of a tight call, either direction and every form: image i's slot, its buffer and its size.  `table` and
// `cache` are the context's pair for the direction; the table is allocated on first use and uploaded when the buffers changed.
static int mixed_records(xpnghip_ctx *c, MixedLayout *&table, std::vector<const void *> &cache, const std::vector<uint64_t> &slot,
                         const void *const *bufs, hipStream_t s) {
    const uint32_t nimg = c->B;
    WS_GET(table, (uint64_t)nimg * sizeof(MixedLayout));
    if (cache.size() == nimg && std::equal(cache.begin(), cache.end(), bufs)) return 0;
    std::vector<MixedLayout> ml(nimg);
    for (uint32_t i = 0; i < nimg; i++)
        ml[i] = MixedLayout{slot[i], (uint8_t *)const_cast<void *>(bufs[i]), (uint32_t)c->m_dims[2ull * i], (uint32_t)c->m_dims[2ull * i + 1]};
    cache.clear();  // (a failed upload must not leave a cache that claims the table is current)
    HIPCHK(hipMemcpyAsync(table, ml.data(), (uint64_t)nimg * sizeof(MixedLayout), hipMemcpyHostToDevice, s));  // (pageable host memory: the copy is staged synchronously anyway)
    HIPCHK(hipStreamSynchronize(s));
    cache.assign(bufs, bufs + nimg);
    return 0;
}
// The compile-time form of a copy-out / staging kernel from the run-time words of a call: each of these hands its callable a
// value whose TYPE carries the choice (3 | 4, planar or not, the element type), and the one place that names a kernel nests them.
template <class F> static void with_3or4(int n, F f) { if (n == 3) f(std::integral_constant<int, 3>{}); else f(std::integral_constant<int, 4>{}); }
template <class F> static void with_planar(uint32_t layout, F f) { if (layout & XPNGHIP_LAYOUT_PLANAR) f(std::true_type{}); else f(std::false_type{}); }
static dim3 mixed_grid(const xpnghip_ctx *c, uint64_t rows) { return dim3((uint32_t)((rows + MC_ROWS - 1) / MC_ROWS), c->B); }
// ---- float layouts (XPNGHIP_DTYPE_*; mixed_float.hpp) -----------------------------------------------------
extern "C" int xpnghip_dtype_bytes(uint32_t dtype) {
    return dtype == XPNGHIP_DTYPE_F16 || dtype == XPNGHIP_DTYPE_BF16 ? 2 : dtype == XPNGHIP_DTYPE_F32 ? 4 : -1;
}
// fp32 -> the bits of the nearest f16 / bf16, ties to even, on the host (what v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32 give on the device)
static uint16_t f16_bits_rne(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (a > 0x7F800000u ? 0x200u : 0));  // inf, NaN
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // >= 65520 rounds to inf
    if (a < 0x33000001u) return (uint16_t)sign;               // <= 2^-25 rounds to zero (the tie 2^-25 goes to even 0)
    const int32_t e = (int32_t)(a >> 23) - 127;
    uint32_t m = (a & 0x7FFFFFu) | 0x800000u, shift = e < -14 ? (uint32_t)(13 + (-14 - e)) : 13u;  // bits that fall off the f16 mantissa
    const uint32_t q = m >> shift, rest = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    uint32_t h = e < -14 ? q : (((uint32_t)(e + 15) << 10) + (q - 0x400u));  // subnormal: no hidden bit, exponent field 0
    if (rest > half || (rest == half && (h & 1))) h++;  // (a carry out of the mantissa runs into the exponent, as it should)
    return (uint16_t)(sign | h);
}
static uint16_t bf16_bits_rne(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x40u);  // NaN stays NaN
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1)) >> 16);
}
static bool float_consts(int C, const float *scale, const float *bias, FloatConsts &k, std::string &why) {
    for (int c = 0; c < 4; c++) {
        k.scale[c] = scale && c < C ? scale[c] : 1.0f;
        k.bias[c] = bias && c < C ? bias[c] : 0.0f;
        if (!std::isfinite(k.scale[c]) || !std::isfinite(k.bias[c])) {
            const bool sc = !std::isfinite(k.scale[c]);
            char b[64];
            snprintf(b, sizeof b, "%s[%d] is %g", sc ? "scale" : "bias", c, (double)(sc ? k.scale[c] : k.bias[c]));
            why = std::string(b) + ": the constants must be finite";
            return false;
        }
    }
    return true;
}
extern "C" int xpnghip_float_table(uint32_t dtype, int C, const float *scale, const float *bias, void *table) {
    const int es = xpnghip_dtype_bytes(dtype);
    if (es < 0) return fail("bad dtype " + std::to_string(dtype) + " (XPNGHIP_DTYPE_F16 = 1, _BF16 = 2, _F32 = 3)"), -1;
    if (C < 1 || C > 4) return fail("xpnghip_float_table: C is " + std::to_string(C) + ", not 1 .. 4"), -1;
    if (!scale || !bias || !table) return fail("xpnghip_float_table: null argument"), -1;
    FloatConsts k;
    std::string why;
    if (!float_consts(C, scale, bias, k, why)) return fail(why), -1;
    for (int c = 0; c < C; c++)
        for (int v = 0; v < 256; v++) {
            const float y = fmaf((float)v, k.scale[c], k.bias[c]);
            if (dtype == XPNGHIP_DTYPE_F32) reinterpret_cast<float *>(table)[c * 256 + v] = y;
            else reinterpret_cast<uint16_t *>(table)[c * 256 + v] = dtype == XPNGHIP_DTYPE_F16 ? f16_bits_rne(y) : bf16_bits_rne(y);
        }
    return 0;
}
// what the float form of the decode adds to the arguments of the layout form
struct FloatCall {
    uint32_t dtype;
    const float *scale, *bias;
};
template <class F> static void with_float(uint32_t dtype, F f) {
    if (dtype == XPNGHIP_DTYPE_F16) f(f16_t{}); else if (dtype == XPNGHIP_DTYPE_BF16) f(bf16_t{}); else f(float{});
}

// ---- crop, resize and flip in the copy-out (mixed_resize.hpp) ------------------------------------------------
// what the resized form of the decode adds to the arguments of the float form
struct ResizeCall {
    const uint64_t *rects;
    const uint8_t *flips;
    uint32_t out_w, out_h;
    uint32_t filter = XPNGHIP_FILTER_BILINEAR;  // (xpnghip_decode_varsize_device_batch_resampled: DESIGN.md 19)
};
static bool resize_size_ok(uint32_t out_w, uint32_t out_h, std::string &why) {
    if (out_w >= 1 && out_w <= 16384 && out_h >= 1 && out_h <= 16384) return true;
    why = "bad output size " + std::to_string(out_w) + " x " + std::to_string(out_h) + " (out_w and out_h must each be 1 .. 16384)";
    return false;
}
// the record of one image: rect == NULL is the whole W x H image.  false, with the reason, for a rectangle that is empty or leaves
// the image and for a flip byte other than 0 or 1
static bool resize_record(uint64_t W, uint64_t H, const uint64_t *rect, uint32_t flip, uint32_t out_w, uint32_t out_h, ResizeRec &z, std::string &why) {
    const uint64_t whole[4] = {0, 0, W, H}, *r = rect ? rect : whole;
    if (!region_valid(W, H, r)) {
        why = "bad rectangle {" + std::to_string(r[0]) + ", " + std::to_string(r[1]) + ", " + std::to_string(r[2]) + ", " + std::to_string(r[3]) +
              "}: it is empty or leaves the " + std::to_string(W) + " x " + std::to_string(H) + " image";
        return false;
    }
    if (flip > 1) {
        why = "bad flip " + std::to_string(flip) + " (a flip is 0 or 1)";
        return false;
    }
    // one IEEE fp32 division each (both operands are below 2^24 + 1: exact as floats)
    z = ResizeRec{(uint32_t)r[0], (uint32_t)r[1], (uint32_t)r[2], (uint32_t)r[3], (float)r[2] / (float)out_w, (float)r[3] / (float)out_h, flip, 0};
    return true;
}
// The twin of k_mixed_resize_as_float on the host: the same operations in the same order.  Every multiplication of the rule is
// inside an explicit fmaf(), and contraction is off for this function on top of that.
static ResizeTap resize_tap_host(uint32_t u, float k, uint32_t n) {
#pragma clang fp contract(off)
    const float c = (float)u + 0.5f;
    const float f = fmaf(c, k, -0.5f);
    const float s = f > 0.0f ? f : 0.0f;
    const uint32_t t = (uint32_t)s;
    ResizeTap r;
    r.i0 = t < n - 1 ? t : n - 1;
    r.i1 = r.i0 + 1 < n - 1 ? r.i0 + 1 : n - 1;
    r.l = s - (float)r.i0;
    return r;
}
// the checks of the two host twins (`fn` names the entry point in the texts): the channels, the constants and the record of the call
static int resize_host_args(const char *fn, int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w,
                            uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias, const void *out, int &C, FloatConsts &k,
                            ResizeRec &z) {
    C = xpnghip_layout_channels(layout, pxsz);
    if (pxsz != 3 && pxsz != 4) return fail(std::string(fn) + ": pxsz is " + std::to_string(pxsz) + ", not 3 or 4");
    if (C < 0) return fail("bad layout word " + layout_hex(layout) + " (XPNGHIP_LAYOUT_PLANAR | XPNGHIP_LAYOUT_BGR | channels 0, 3 or 4 in bits 8..11)");
    const int es = xpnghip_dtype_bytes(dtype);
    if (es < 0) return fail("bad dtype " + std::to_string(dtype) + " (XPNGHIP_DTYPE_F16 = 1, _BF16 = 2, _F32 = 3)");
    std::string why;
    if (!float_consts(C, scale, bias, k, why)) return fail(why);
    if (!raster || !out) return fail(std::string(fn) + ": null raster or output buffer");
    if ((uintptr_t)out & (uintptr_t)(es - 1)) {
        char b[32];
        snprintf(b, sizeof b, "%p", out);
        return fail("output buffer " + std::string(b) + " is not aligned to its " + std::to_string(es) + "-byte elements");
    }
    if (!w || !h || w > (1u << 24) || h > (1u << 24)) return fail("bad image size " + std::to_string(w) + " x " + std::to_string(h) + " (each side must be 1 .. 16777216)");
    if (!resize_size_ok(out_w, out_h, why)) return fail(why);
    if (!resize_record(w, h, rect, (uint32_t)flip, out_w, out_h, z, why)) return fail(why);
    return 0;
}
static int resize_host_impl(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w, uint32_t out_h,
                            uint32_t layout, uint32_t dtype, const float *scale, const float *bias, void *out) {
#pragma clang fp contract(off)
    int C;
    FloatConsts k;
    ResizeRec z;
    if (resize_host_args("xpnghip_resize_host", pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, out, C, k, z)) return 1;
    const bool planar = layout & XPNGHIP_LAYOUT_PLANAR, bgr = layout & XPNGHIP_LAYOUT_BGR;
    std::vector<ResizeTap> tx(out_w);
    for (uint32_t ox = 0; ox < out_w; ox++) tx[ox] = resize_tap_host(z.flip ? out_w - 1 - ox : ox, z.kx, z.rw);
    for (uint32_t oy = 0; oy < out_h; oy++) {
        const ResizeTap ty = resize_tap_host(oy, z.ky, z.rh);
        const uint8_t *s0 = raster + ((uint64_t)(z.ry + ty.i0) * w + z.rx) * pxsz, *s1 = raster + ((uint64_t)(z.ry + ty.i1) * w + z.rx) * pxsz;
        for (uint32_t ox = 0; ox < out_w; ox++)
            for (int c = 0; c < C; c++) {
                float v = 255.0f;  // the alpha an RGB raster does not store
                if (!(pxsz == 3 && c == 3)) {
                    const uint32_t sc = bgr && c < 3 ? 2 - c : c, o0 = tx[ox].i0 * pxsz + sc, o1 = tx[ox].i1 * pxsz + sc;
                    const float p00 = (float)s0[o0], p01 = (float)s0[o1], p10 = (float)s1[o0], p11 = (float)s1[o1];
                    const float d0 = p01 - p00, d1 = p11 - p10;
                    const float a = fmaf(tx[ox].l, d0, p00), b = fmaf(tx[ox].l, d1, p10);
                    const float d = b - a;
                    v = fmaf(ty.l, d, a);
                }
                const float y = fmaf(v, k.scale[c], k.bias[c]);
                const uint64_t e = planar ? ((uint64_t)c * out_h + oy) * out_w + ox : ((uint64_t)oy * out_w + ox) * C + c;
                if (dtype == XPNGHIP_DTYPE_F32) reinterpret_cast<float *>(out)[e] = y;
                else reinterpret_cast<uint16_t *>(out)[e] = dtype == XPNGHIP_DTYPE_F16 ? f16_bits_rne(y) : bf16_bits_rne(y);
            }
    }
    return 0;
}
extern "C" int xpnghip_resize_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w, uint32_t out_h,
                                   uint32_t layout, uint32_t dtype, const float *scale, const float *bias, void *out) {
    XPNG_GUARDED(resize_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, out))
}
// ---- the antialiased downscale (mixed_resample.hpp) -------------------------------------------------------------
static bool resample_filter_ok(uint32_t filter, std::string &why) {
    if (filter <= XPNGHIP_FILTER_TRIANGLE_AA) return true;
    why = "bad filter " + std::to_string(filter) + " (XPNGHIP_FILTER_BILINEAR = 0, XPNGHIP_FILTER_TRIANGLE_AA = 1)";
    return false;
}
// the record of filter 1 from the resized call's: the inverses are one IEEE fp32 division each
static ResampleRec resample_record(const ResizeRec &z) {
    return ResampleRec{z.rx, z.ry, z.rw, z.rh, z.kx, z.ky, 1.0f / z.kx, 1.0f / z.ky, z.flip, {0, 0, 0}};
}
// The twin of k_mixed_resample_as_float on the host: the same operations in the same order, every multiplication inside an
// explicit fmaf(), contraction off on top of that.  One axis of the rule for output index u: the two taps (aa false) or the window.
struct ResampleAxis {
    bool aa;
    ResizeTap t;
    uint32_t j0, j1;
    float f;
};
static ResampleAxis resample_axis_host(uint32_t u, float k, uint32_t n) {
#pragma clang fp contract(off)
    ResampleAxis a{};
    a.aa = k > 1.0f;
    if (!a.aa) {
        a.t = resize_tap_host(u, k, n);
        return a;
    }
    const float c = (float)u + 0.5f;
    a.f = fmaf(c, k, -0.5f);
    const float lo = a.f - k, hi = a.f + k;
    a.j0 = lo > 0.0f ? (uint32_t)lo : 0u;
    const uint32_t t = (uint32_t)hi;
    a.j1 = t < n - 1 ? t : n - 1;
    return a;
}
// the axis operation over q(0 .. n-1); *bad is set where W is not positive (the rule's argument says never)
template <class Q> static float resample_axis_apply(const ResampleAxis &a, float ik, Q q, bool *bad) {
#pragma clang fp contract(off)
    if (!a.aa) {
        const float q0 = q(a.t.i0), q1 = q(a.t.i1);
        const float d = q1 - q0;
        return fmaf(a.t.l, d, q0);
    }
    float W = 0.0f, A = 0.0f;
    for (uint32_t j = a.j0; j <= a.j1; j++) {
        const float d = fabsf((float)j - a.f);
        float w = fmaf(-d, ik, 1.0f);
        if (!(w > 0.0f)) w = 0.0f;
        W = W + w;
        A = fmaf(w, q(j), A);
    }
    if (!(W > 0.0f)) *bad = true;
    return A / W;
}
// What the twins of the views kernels share behind a pixel's resampled values (mixed_views_pixel.hpp), contraction off as in the
// twins themselves.  The three rows of a view's colour matrix and the clamp: t[k] from v = R, G, B
static void colour_rows_host(const float *colour, const float *v, float *t) {
#pragma clang fp contract(off)
    for (int q = 0; q < 3; q++) {
        const float *m = colour + 4 * q;
        const float a = fmaf(m[2], v[2], m[3]);
        const float b = fmaf(m[1], v[1], a);
        const float x = fmaf(m[0], v[0], b);
        t[q] = x < 0.0f ? 0.0f : x > 255.0f ? 255.0f : x;
    }
}
// the element of a buffer of `dtype`
static void host_put(void *out, uint32_t dtype, uint64_t e, float y) {
    if (dtype == XPNGHIP_DTYPE_F32) reinterpret_cast<float *>(out)[e] = y;
    else reinterpret_cast<uint16_t *>(out)[e] = dtype == XPNGHIP_DTYPE_F16 ? f16_bits_rne(y) : bf16_bits_rne(y);
}
// a twin's output: C channels of w x h elements of `dtype`, planar or interleaved (a twin that collects its values first, so that
// a failing call writes nothing, points this at fp32 values and narrows them behind its checks)
struct HostOut {
    void *out;
    uint32_t dtype;
    bool planar;
    int C;
    uint32_t w, h;
};
// value v of channel position c of output pixel (ox, oy): the constants, the element's index, the element
static void host_element(const HostOut &o, const FloatConsts &k, uint32_t ox, uint32_t oy, int c, float v) {
#pragma clang fp contract(off)
    const float y = fmaf(v, k.scale[c], k.bias[c]);
    host_put(o.out, o.dtype, o.planar ? ((uint64_t)c * o.h + oy) * o.w + ox : ((uint64_t)oy * o.w + ox) * o.C + c, y);
}
static int resample_host_impl(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w, uint32_t out_h,
                              uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, void *out) {
#pragma clang fp contract(off)
    std::string why;
    if (!resample_filter_ok(filter, why)) return fail(why);
    // filter 0 is the resized twin itself, whole
    if (filter == XPNGHIP_FILTER_BILINEAR) return resize_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, out);
    int C;
    FloatConsts k;
    ResizeRec z0;
    if (resize_host_args("xpnghip_resample_host", pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, out, C, k, z0)) return 1;
    const ResampleRec z = resample_record(z0);
    const bool planar = layout & XPNGHIP_LAYOUT_PLANAR, bgr = layout & XPNGHIP_LAYOUT_BGR;
    std::vector<ResampleAxis> ax(out_w), ay(out_h);
    for (uint32_t ox = 0; ox < out_w; ox++) ax[ox] = resample_axis_host(z.flip ? out_w - 1 - ox : ox, z.kx, z.rw);
    for (uint32_t oy = 0; oy < out_h; oy++) ay[oy] = resample_axis_host(oy, z.ky, z.rh);
    // the values first, the elements after them: a call that fails writes nothing
    std::vector<float> ys((uint64_t)C * out_h * out_w);
    const HostOut yo{ys.data(), XPNGHIP_DTYPE_F32, planar, C, out_w, out_h};
    bool bad = false;
    for (uint32_t oy = 0; oy < out_h; oy++)
        for (uint32_t ox = 0; ox < out_w; ox++)
            for (int c = 0; c < C; c++) {
                float v = 255.0f;  // the alpha an RGB raster does not store
                if (!(pxsz == 3 && c == 3)) {
                    const uint32_t sc = bgr && c < 3 ? 2 - c : c;
                    auto H = [&](uint32_t s) {
                        const uint8_t *p = raster + ((uint64_t)(z.ry + s) * w + z.rx) * pxsz + sc;
                        return resample_axis_apply(ax[ox], z.ikx, [&](uint32_t j) { return (float)p[(uint64_t)j * pxsz]; }, &bad);
                    };
                    v = resample_axis_apply(ay[oy], z.iky, H, &bad);
                }
                host_element(yo, k, ox, oy, c, v);
            }
    if (bad) return fail("internal error: a window of the triangle filter has no weight");  // (W > 0 always: DESIGN.md 19)
    for (uint64_t e = 0; e < ys.size(); e++) host_put(out, dtype, e, ys[e]);
    return 0;
}
extern "C" int xpnghip_resample_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w, uint32_t out_h,
                                     uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, void *out) {
    XPNG_GUARDED(resample_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, filter, out))
}
// ---- a colour matrix behind the resampling (mixed_views_colour.hpp) ---------------------------------------------
// every entry finite and |m| <= 65536: no intermediate of the rule overflows and no NaN arises.  `who` names the view in a device call
static bool colour_matrix_ok(const float *m, const std::string &who, std::string &why) {
    for (int e = 0; e < 12; e++) {
        if (std::isfinite(m[e]) && fabsf(m[e]) <= 65536.0f) continue;
        char b[48];
        snprintf(b, sizeof b, "%g", (double)m[e]);
        why = "bad colour matrix" + who + ": entry [" + std::to_string(e / 4) + "][" + std::to_string(e % 4) + "] is " + b + " (every entry must be finite and at most 65536 in magnitude)";
        return false;
    }
    return true;
}
// The twin of k_mixed_views_colour on the host: the resampled twin's operations for the bytes of a pixel, then the matrix, the clamp
// and the constants, every multiplication inside an explicit fmaf(), contraction off on top of that.
static int resample_colour_host_impl(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w, uint32_t out_h,
                                     uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *colour, void *out) {
#pragma clang fp contract(off)
    if (!colour) return resample_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, filter, out);
    std::string why;
    if (!resample_filter_ok(filter, why)) return fail(why);
    int C;
    FloatConsts k;
    ResizeRec z0;
    if (resize_host_args("xpnghip_resample_colour_host", pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, out, C, k, z0)) return 1;
    if (!colour_matrix_ok(colour, "", why)) return fail(why);
    const ResampleRec z = resample_record(z0);
    const bool planar = layout & XPNGHIP_LAYOUT_PLANAR, bgr = layout & XPNGHIP_LAYOUT_BGR;
    // filter 0: the two taps on both axes whatever the ratio
    auto axis = [&](uint32_t u, float kk, uint32_t n) {
        if (filter) return resample_axis_host(u, kk, n);
        ResampleAxis a{};
        a.t = resize_tap_host(u, kk, n);
        return a;
    };
    std::vector<ResampleAxis> ax(out_w), ay(out_h);
    for (uint32_t ox = 0; ox < out_w; ox++) ax[ox] = axis(z.flip ? out_w - 1 - ox : ox, z.kx, z.rw);
    for (uint32_t oy = 0; oy < out_h; oy++) ay[oy] = axis(oy, z.ky, z.rh);
    // the values first, the elements after them: a call that fails writes nothing
    std::vector<float> ys((uint64_t)C * out_h * out_w);
    const HostOut yo{ys.data(), XPNGHIP_DTYPE_F32, planar, C, out_w, out_h};
    bool bad = false;
    for (uint32_t oy = 0; oy < out_h; oy++)
        for (uint32_t ox = 0; ox < out_w; ox++) {
            float v[4] = {0.0f, 0.0f, 0.0f, 255.0f};  // R, G, B of the file and its alpha (255: the alpha an RGB raster does not store)
            for (int sc = 0; sc < (pxsz == 4 && C == 4 ? 4 : 3); sc++) {
                auto H = [&](uint32_t s) {
                    const uint8_t *p = raster + ((uint64_t)(z.ry + s) * w + z.rx) * pxsz + sc;
                    return resample_axis_apply(ax[ox], z.ikx, [&](uint32_t j) { return (float)p[(uint64_t)j * pxsz]; }, &bad);
                };
                v[sc] = resample_axis_apply(ay[oy], z.iky, H, &bad);
            }
            float t[3];
            colour_rows_host(colour, v, t);
            for (int c = 0; c < C; c++) host_element(yo, k, ox, oy, c, c == 3 ? v[3] : t[bgr ? 2 - c : c]);
        }
    if (bad) return fail("internal error: a window of the triangle filter has no weight");  // (W > 0 always: DESIGN.md 19)
    for (uint64_t e = 0; e < ys.size(); e++) host_put(out, dtype, e, ys[e]);
    return 0;
}
extern "C" int xpnghip_resample_colour_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w,
                                            uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter,
                                            const float *colour, void *out) {
    XPNG_GUARDED(resample_colour_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, filter, colour, out))
}
// ---- the antialiased bicubic of a views call (mixed_views_cubic.hpp) --------------------------------------------
// One axis of the cubic rule for output index u: the window and the centre; `is` is the inverse of the stretch
struct CubicAxis {
    uint32_t j0, j1;
    float f;
};
static CubicAxis cubic_axis_host(uint32_t u, float k, uint32_t n) {
#pragma clang fp contract(off)
    CubicAxis a{};
    const float c = (float)u + 0.5f;
    a.f = fmaf(c, k, -0.5f);
    const float s = k > 1.0f ? k : 1.0f;
    const float r = s + s;
    const float lo = a.f - r, hi = a.f + r;
    a.j0 = lo > 0.0f ? (uint32_t)lo : 0u;
    const uint32_t t = (uint32_t)hi;
    a.j1 = t < n - 1 ? t : n - 1;
    return a;
}
// the axis operation over q(0 .. n-1); *bad is set where W is not positive (the rule's argument says never)
template <class Q> static float cubic_axis_apply(const CubicAxis &a, float is, Q q, bool *bad) {
#pragma clang fp contract(off)
    float W = 0.0f, A = 0.0f;
    for (uint32_t j = a.j0; j <= a.j1; j++) {
        const float d = fabsf((float)j - a.f);
        const float t = fmaf(d, is, 0.0f);
        float w = 0.0f;
        if (t < 1.0f) w = fmaf(fmaf(fmaf(1.5f, t, -2.5f), t, 0.0f), t, 1.0f);
        else if (t < 2.0f) w = fmaf(fmaf(fmaf(-0.5f, t, 2.5f), t, -4.0f), t, 2.0f);
        W = W + w;
        A = fmaf(w, q(j), A);
    }
    if (!(W > 0.0f)) *bad = true;
    return A / W;
}
// The twin of k_mixed_views_cubic on the host: the same operations in the same order, every multiplication inside an explicit
// fmaf(), contraction off on top of that.  It IS the rule of the cubic views call.
static int resample_cubic_host_impl(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w, uint32_t out_h,
                                    uint32_t layout, uint32_t dtype, const float *scale, const float *bias, const float *colour, void *out) {
#pragma clang fp contract(off)
    std::string why;
    int C;
    FloatConsts k;
    ResizeRec z0;
    if (resize_host_args("xpnghip_resample_cubic_host", pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, out, C, k, z0)) return 1;
    if (colour && !colour_matrix_ok(colour, "", why)) return fail(why);
    const ResampleRec z = resample_record(z0);
    const bool planar = layout & XPNGHIP_LAYOUT_PLANAR, bgr = layout & XPNGHIP_LAYOUT_BGR;
    const float isx = z.kx > 1.0f ? z.ikx : 1.0f, isy = z.ky > 1.0f ? z.iky : 1.0f;
    std::vector<CubicAxis> ax(out_w), ay(out_h);
    for (uint32_t ox = 0; ox < out_w; ox++) ax[ox] = cubic_axis_host(z.flip ? out_w - 1 - ox : ox, z.kx, z.rw);
    for (uint32_t oy = 0; oy < out_h; oy++) ay[oy] = cubic_axis_host(oy, z.ky, z.rh);
    // the values first, the elements after them: a call that fails writes nothing
    std::vector<float> ys((uint64_t)C * out_h * out_w);
    const HostOut yo{ys.data(), XPNGHIP_DTYPE_F32, planar, C, out_w, out_h};
    bool bad = false;
    for (uint32_t oy = 0; oy < out_h; oy++)
        for (uint32_t ox = 0; ox < out_w; ox++) {
            float v[4] = {0.0f, 0.0f, 0.0f, 255.0f};  // R, G, B of the file and its alpha (255: the alpha an RGB raster does not store)
            for (int sc = 0; sc < (pxsz == 4 && C == 4 ? 4 : 3); sc++) {
                auto H = [&](uint32_t s) {
                    const uint8_t *p = raster + ((uint64_t)(z.ry + s) * w + z.rx) * pxsz + sc;
                    return cubic_axis_apply(ax[ox], isx, [&](uint32_t j) { return (float)p[(uint64_t)j * pxsz]; }, &bad);
                };
                const float x = cubic_axis_apply(ay[oy], isy, H, &bad);
                v[sc] = x < 0.0f ? 0.0f : x > 255.0f ? 255.0f : x;  // a cubic overshoots: the clamp a uint8 pipeline applies
            }
            float t[3] = {v[0], v[1], v[2]};
            if (colour) colour_rows_host(colour, v, t);
            for (int c = 0; c < C; c++) host_element(yo, k, ox, oy, c, c == 3 ? v[3] : t[bgr ? 2 - c : c]);
        }
    if (bad) return fail("internal error: a window of the cubic filter has no weight");  // (W > 0 always: DESIGN.md 22)
    for (uint64_t e = 0; e < ys.size(); e++) host_put(out, dtype, e, ys[e]);
    return 0;
}
extern "C" int xpnghip_resample_cubic_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w,
                                           uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias, const float *colour,
                                           void *out) {
    XPNG_GUARDED(resample_cubic_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, colour, out))
}
// ---- Gaussian blur and solarise behind the resampling (mixed_views_blur.hpp) ------------------------------------
// the third filter word: the two entry points of the blur alone take it
static bool blur_filter_ok(uint32_t filter, std::string &why) {
    if (filter <= XPNGHIP_FILTER_CUBIC_AA) return true;
    why = "bad filter " + std::to_string(filter) + " (XPNGHIP_FILTER_BILINEAR = 0, XPNGHIP_FILTER_TRIANGLE_AA = 1, XPNGHIP_FILTER_CUBIC_AA = 2)";
    return false;
}
static std::string blur_num(float v) {
    char b[48];
    snprintf(b, sizeof b, "%g", (double)v);
    return b;
}
// sigma and radius of a record or of xpnghip_blur_weights.  `who` names the view in a device call
static bool blur_sigma_ok(float sigma, uint32_t radius, const std::string &who, std::string &why) {
    if (radius > BLUR_RMAX) { why = "bad blur" + who + ": radius is " + std::to_string(radius) + ", not 0 .. 31"; return false; }
    if (radius == 0 && !(sigma == 0.0f)) { why = "bad blur" + who + ": sigma is " + blur_num(sigma) + " with radius 0 (no blur: sigma must be 0)"; return false; }
    if (radius > 0 && !(std::isfinite(sigma) && sigma >= 0.0009765625f && sigma <= 1024.0f)) {
        why = "bad blur" + who + ": sigma is " + blur_num(sigma) + " (with radius > 0 it must be finite and lie in 2^-10 .. 1024)";
        return false;
    }
    return true;
}
// a whole record against the output size of its view
static bool blur_record_ok(const xpnghip_view_blur &b, uint32_t out_w, uint32_t out_h, const std::string &who, std::string &why) {
    if (!blur_sigma_ok(b.sigma, b.radius, who, why)) return false;
    if (b.radius >= out_w || b.radius >= out_h) {
        why = "bad blur" + who + ": radius " + std::to_string(b.radius) + " does not lie below both sides of the " + std::to_string(out_w) + " x " + std::to_string(out_h) +
              " output (the border is a reflection)";
        return false;
    }
    if (!(b.solarise == 256.0f || (b.solarise >= 0.0f && b.solarise <= 255.0f))) {
        why = "bad blur" + who + ": solarise is " + blur_num(b.solarise) + " (a threshold of 0 .. 255, or exactly 256 for none)";
        return false;
    }
    if (b.reserved) { why = "bad blur" + who + ": reserved is " + std::to_string(b.reserved) + ", not 0"; return false; }
    return true;
}
static bool blur_off(const xpnghip_view_blur &b) { return b.radius == 0 && b.solarise == 256.0f; }
// the weights of a checked (sigma, radius): the one statement (include/xpng_hip.h)
static void blur_weights(float sigma, uint32_t radius, float *w) {
    if (!radius) { w[0] = 1.0f; return; }
    const double s = (double)sigma;
    double g[BLUR_RMAX + 1], t = 0.0;
    for (uint32_t d = 0; d <= radius; d++) g[d] = exp(-(double)(d * d) / (2.0 * s * s));
    for (uint32_t d = 1; d <= radius; d++) t += g[d];
    const double S = g[0] + 2.0 * t;
    for (uint32_t d = 0; d <= radius; d++) w[d] = (float)(g[d] / S);
}
extern "C" int xpnghip_blur_weights(float sigma, uint32_t radius, float *w) {
    std::string why;
    if (!blur_sigma_ok(sigma, radius, "", why)) return fail(why);
    if (!w) return fail("xpnghip_blur_weights: w is NULL");
    blur_weights(sigma, radius, w);
    return 0;
}
// The twin of the two passes on the host: the intermediate from the host rule of the filter, then k_mixed_views_blur's operations
// in its order, every multiplication inside an explicit fmaf(), contraction off on top of that.  It IS the rule of the blur call.
static int resample_blur_host_impl(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w, uint32_t out_h,
                                   uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *colour,
                                   const xpnghip_view_blur *blur, void *out) {
#pragma clang fp contract(off)
    std::string why;
    if (!blur_filter_ok(filter, why)) return fail(why);
    int C;
    FloatConsts k;
    ResizeRec z0;
    if (resize_host_args("xpnghip_resample_blur_host", pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, out, C, k, z0)) return 1;
    if (colour && !colour_matrix_ok(colour, "", why)) return fail(why);
    const xpnghip_view_blur b = blur ? *blur : xpnghip_view_blur{0.0f, 0u, 256.0f, 0u};
    if (!blur_record_ok(b, out_w, out_h, "", why)) return fail(why);
    // T: C planes of fp32 in byte units, from the host rule of the filter
    const uint64_t plane = (uint64_t)out_h * out_w;
    std::vector<float> T((uint64_t)C * plane);
    const float one[4] = {1.0f, 1.0f, 1.0f, 1.0f}, zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t tl = XPNGHIP_LAYOUT_PLANAR | ((uint32_t)C << 8);
    if (filter == XPNGHIP_FILTER_CUBIC_AA ? resample_cubic_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, tl, XPNGHIP_DTYPE_F32, one, zero, colour, T.data())
                                          : resample_colour_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, tl, XPNGHIP_DTYPE_F32, one, zero, filter, colour, T.data()))
        return 1;
    const uint32_t R = b.radius;
    if (R) {
        float wt[BLUR_RMAX + 1];
        blur_weights(b.sigma, R, wt);
        auto refl = [](int64_t i, int64_t n) { return (uint64_t)(i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i); };
        std::vector<float> Hh(plane);
        for (int q = 0; q < 3; q++) {
            float *p = T.data() + q * plane;
            for (uint32_t y = 0; y < out_h; y++)
                for (uint32_t x = 0; x < out_w; x++) {
                    const float *row = p + (uint64_t)y * out_w;
                    float A = 0.0f;
                    for (uint32_t d = R; d >= 1; d--) {
                        const float s = row[refl((int64_t)x - d, out_w)] + row[refl((int64_t)x + d, out_w)];
                        A = fmaf(wt[d], s, A);
                    }
                    Hh[(uint64_t)y * out_w + x] = fmaf(wt[0], row[x], A);
                }
            for (uint32_t y = 0; y < out_h; y++)
                for (uint32_t x = 0; x < out_w; x++) {
                    float A = 0.0f;
                    for (uint32_t d = R; d >= 1; d--) {
                        const float s = Hh[refl((int64_t)y - d, out_h) * out_w + x] + Hh[refl((int64_t)y + d, out_h) * out_w + x];
                        A = fmaf(wt[d], s, A);
                    }
                    A = fmaf(wt[0], Hh[(uint64_t)y * out_w + x], A);
                    p[(uint64_t)y * out_w + x] = A < 0.0f ? 0.0f : A > 255.0f ? 255.0f : A;
                }
        }
    }
    const bool planar = layout & XPNGHIP_LAYOUT_PLANAR, bgr = layout & XPNGHIP_LAYOUT_BGR, sol = b.solarise < 256.0f;
    const HostOut ho{out, dtype, planar, C, out_w, out_h};
    for (uint32_t oy = 0; oy < out_h; oy++)
        for (uint32_t ox = 0; ox < out_w; ox++)
            for (int c = 0; c < C; c++) {
                float v = T[(uint64_t)(c == 3 ? 3 : bgr ? 2 - c : c) * plane + (uint64_t)oy * out_w + ox];
                if (c < 3 && sol && v >= b.solarise) v = 255.0f - v;
                host_element(ho, k, ox, oy, c, v);
            }
    return 0;
}
extern "C" int xpnghip_resample_blur_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w,
                                          uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter,
                                          const float *colour, const xpnghip_view_blur *blur, void *out) {
    XPNG_GUARDED(resample_blur_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, filter, colour, blur, out))
}
// ---- an affine map per view (mixed_views_affine.hpp) -----------------------------------------------------------
// the filter words of the affine entry points: bilinear or nearest, nothing else
static bool affine_filter_ok(uint32_t filter, std::string &why) {
    if (filter == XPNGHIP_FILTER_BILINEAR || filter == XPNGHIP_FILTER_NEAREST) return true;
    why = "bad filter " + std::to_string(filter) + " (an affine call takes XPNGHIP_FILTER_BILINEAR = 0 or XPNGHIP_FILTER_NEAREST = 3)";
    return false;
}
static bool affine_fill_ok(const float *fill, std::string &why) {
    for (int e = 0; fill && e < 4; e++) {
        if (std::isfinite(fill[e]) && fill[e] >= 0.0f && fill[e] <= 255.0f) continue;
        why = "bad fill: entry " + std::to_string(e) + " is " + blur_num(fill[e]) + " (R, G, B, A in byte units: each must be finite and lie in 0 .. 255)";
        return false;
    }
    return true;
}
// The matrix of a view against its output size, and its footprint {x, y, w, h} in pixels of the W x H image ({0, 0, 0, 0}: empty).
// The entry bounds: |m| times the extent it multiplies - out_w in the first column, out_h in the second, 1 in the third - is at
// most 2^18, so every coordinate of the view and every intermediate of the rule stays below 2^20 in magnitude.
// The corners in double from the fp32 entries; the map is affine, so the extremes are there.  `who` names the view in a device call
static bool affine_footprint(uint64_t W, uint64_t H, const float *m, uint32_t ow, uint32_t oh, const std::string &who, uint64_t *rect, std::string &why) {
    for (int e = 0; e < 6; e++) {
        const uint32_t n = e % 3 == 0 ? ow : e % 3 == 1 ? oh : 1u;
        if (std::isfinite(m[e]) && fabs((double)m[e]) * n <= 262144.0) continue;
        why = "bad affine matrix" + who + ": entry [" + std::to_string(e / 3) + "][" + std::to_string(e % 3) + "] is " + blur_num(m[e]) +
              " (every entry must be finite, and its magnitude times " + (e % 3 == 0 ? "out_w" : e % 3 == 1 ? "out_h" : "1") + " = " + std::to_string(n) + " at most 262144)";
        return false;
    }
    double lo[2] = {0, 0}, hi[2] = {0, 0};
    for (int a = 0; a < 2; a++)
        for (int q = 0; q < 4; q++) {
            const double X = (q & 1 ? (double)(ow - 1) : 0.0) + 0.5, Y = (q & 2 ? (double)(oh - 1) : 0.0) + 0.5;
            const double s = (double)m[3 * a] * X + (double)m[3 * a + 1] * Y + (double)m[3 * a + 2] - 0.5;
            if (!q || s < lo[a]) lo[a] = s;
            if (!q || s > hi[a]) hi[a] = s;
        }
    const int64_t x0 = std::max<int64_t>((int64_t)floor(lo[0]) - 1, 0), x1 = std::min<int64_t>((int64_t)floor(hi[0]) + 2, (int64_t)W - 1);
    const int64_t y0 = std::max<int64_t>((int64_t)floor(lo[1]) - 1, 0), y1 = std::min<int64_t>((int64_t)floor(hi[1]) + 2, (int64_t)H - 1);
    const bool empty = x0 > x1 || y0 > y1;
    rect[0] = empty ? 0 : (uint64_t)x0; rect[1] = empty ? 0 : (uint64_t)y0;
    rect[2] = empty ? 0 : (uint64_t)(x1 - x0 + 1); rect[3] = empty ? 0 : (uint64_t)(y1 - y0 + 1);
    return true;
}
extern "C" int xpnghip_affine_footprint(uint64_t w, uint64_t h, const float *affine, uint32_t out_w, uint32_t out_h, uint64_t *rect) {
    std::string why;
    if (!affine || !rect) return fail("xpnghip_affine_footprint: null matrix or rectangle");
    if (!w || !h || w > (1u << 24) || h > (1u << 24)) return fail("bad image size " + std::to_string(w) + " x " + std::to_string(h) + " (each side must be 1 .. 16777216)");
    if (!resize_size_ok(out_w, out_h, why)) return fail(why);
    uint64_t r[4];
    if (!affine_footprint(w, h, affine, out_w, out_h, "", r, why)) return fail(why);
    memcpy(rect, r, sizeof r);
    return 0;
}
// The twin of k_mixed_views_affine on the host: the same operations in the same order, every multiplication inside an explicit
// fmaf(), contraction off on top of that.  It IS the rule of the affine views call.
static int resample_affine_host_impl(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const float *affine, uint32_t out_w, uint32_t out_h,
                                     uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *fill,
                                     const float *colour, void *out) {
#pragma clang fp contract(off)
    std::string why;
    if (!affine_filter_ok(filter, why)) return fail(why);
    int C;
    FloatConsts k;
    ResizeRec z0;
    if (resize_host_args("xpnghip_resample_affine_host", pxsz, raster, w, h, nullptr, 0, out_w, out_h, layout, dtype, scale, bias, out, C, k, z0)) return 1;
    if (!affine) return fail("xpnghip_resample_affine_host: null matrix");
    uint64_t F[4];
    if (!affine_footprint(w, h, affine, out_w, out_h, "", F, why)) return fail(why);
    if (!affine_fill_ok(fill, why)) return fail(why);
    if (colour && !colour_matrix_ok(colour, "", why)) return fail(why);
    const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f}, *fl = fill ? fill : zero, *m = affine;
    const bool planar = layout & XPNGHIP_LAYOUT_PLANAR, bgr = layout & XPNGHIP_LAYOUT_BGR;
    const int NS = pxsz == 4 && C == 4 ? 4 : 3;
    const HostOut ho{out, dtype, planar, C, out_w, out_h};
    const int64_t fx0 = (int64_t)F[0], fy0 = (int64_t)F[1], fx1 = fx0 + (int64_t)F[2], fy1 = fy0 + (int64_t)F[3];
    auto q = [&](int64_t j, int64_t i, int sc) {
        if (j < fx0 || j >= fx1 || i < fy0 || i >= fy1) return fl[sc];
        return (float)raster[((uint64_t)i * w + (uint64_t)j) * pxsz + sc];
    };
    for (uint32_t oy = 0; oy < out_h; oy++)
        for (uint32_t ox = 0; ox < out_w; ox++) {
            const float X = (float)ox + 0.5f, Y = (float)oy + 0.5f;
            const float ax = fmaf(m[1], Y, m[2]), ay = fmaf(m[4], Y, m[5]);
            const float bx = fmaf(m[0], X, ax), by = fmaf(m[3], X, ay);
            const float sx = bx - 0.5f, sy = by - 0.5f;
            float v[4] = {0.0f, 0.0f, 0.0f, 255.0f};  // R, G, B of the file and its alpha (255: the alpha an RGB raster does not store)
            if (filter == XPNGHIP_FILTER_NEAREST) {
                const int64_t j = (int64_t)rintf(sx), i = (int64_t)rintf(sy);  // (ties to even: the default rounding mode)
                for (int sc = 0; sc < NS; sc++) v[sc] = q(j, i, sc);
            } else {
                const float x0 = floorf(sx), y0 = floorf(sy);
                const float lx = sx - x0, ly = sy - y0;
                const int64_t j = (int64_t)x0, i = (int64_t)y0;
                for (int sc = 0; sc < NS; sc++) {
                    const float q00 = q(j, i, sc), q10 = q(j + 1, i, sc), q01 = q(j, i + 1, sc), q11 = q(j + 1, i + 1, sc);
                    const float d0 = q10 - q00, d1 = q11 - q01;
                    const float t = fmaf(lx, d0, q00), u = fmaf(lx, d1, q01);
                    const float d = u - t;
                    v[sc] = fmaf(ly, d, t);
                }
            }
            float t[3] = {v[0], v[1], v[2]};
            if (colour) colour_rows_host(colour, v, t);
            for (int c = 0; c < C; c++) host_element(ho, k, ox, oy, c, c == 3 ? v[3] : t[bgr ? 2 - c : c]);
        }
    return 0;
}
extern "C" int xpnghip_resample_affine_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const float *affine, uint32_t out_w, uint32_t out_h,
                                            uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *fill,
                                            const float *colour, void *out) {
    XPNG_GUARDED(resample_affine_host_impl(pxsz, raster, w, h, affine, out_w, out_h, layout, dtype, scale, bias, filter, fill, colour, out))
}
// ---- tone steps behind the blur call or the affine call (mixed_views_tone.hpp) ----------------------------------
static const char *const TONE_NAMES[6] = {"none", "autocontrast", "equalise", "posterise", "solarise", "invert"};
// a whole record.  `who` names the view in a device call
static bool tone_record_ok(const xpnghip_view_tone &t, const std::string &who, std::string &why) {
    bool ended = false;
    for (int i = 0; i < 4; i++) {
        const uint32_t op = t.op[i];
        const float a = t.arg[i];
        const std::string at = "bad tone" + who + ", step " + std::to_string(i) + ": ";
        if (op > XPNGHIP_TONE_INVERT) { why = at + "op is " + std::to_string(op) + ", not 0 .. 5"; return false; }
        if (op != XPNGHIP_TONE_NONE && ended) { why = at + TONE_NAMES[op] + " follows a step that is NONE (steps are contiguous from index 0)"; return false; }
        if (op == XPNGHIP_TONE_NONE) ended = true;
        if (op == XPNGHIP_TONE_POSTERISE) {
            if (!(a >= 0.0f && a <= 8.0f && a == floorf(a))) { why = at + "posterise bits are " + blur_num(a) + ", not an integer in 0 .. 8"; return false; }
        } else if (op == XPNGHIP_TONE_SOLARISE) {
            if (!(a >= 0.0f && a <= 255.0f)) { why = at + "solarise threshold is " + blur_num(a) + " (it must be finite and lie in 0 .. 255)"; return false; }
        } else if (!(a == 0.0f)) {
            why = at + "arg is " + blur_num(a) + " on " + TONE_NAMES[op] + ", which takes none (it must be 0)";
            return false;
        }
    }
    return true;
}
static bool tone_off(const xpnghip_view_tone &t) { return t.op[0] == XPNGHIP_TONE_NONE; }  // (of a checked record)
// The steps of a checked record on the three colour planes of T (planes of N floats back to back), in the header's words: it IS
// the rule of the tone calls.  Contraction off; the product of autocontrast is an operation of its own.
static void tone_planes_host(float *T, uint64_t N, const xpnghip_view_tone &t) {
#pragma clang fp contract(off)
    for (int q = 0; q < 3; q++) {
        float *p = T + (uint64_t)q * N;
        for (uint64_t i = 0; i < N; i++) p[i] = p[i] > 0.0f ? (p[i] > 255.0f ? 255.0f : p[i]) : 0.0f;
        for (int si = 0; si < 4 && t.op[si] != XPNGHIP_TONE_NONE; si++) {
            const float a = t.arg[si];
            switch (t.op[si]) {
            case XPNGHIP_TONE_AUTOCONTRAST: {
                float lo = p[0], hi = p[0];
                for (uint64_t i = 1; i < N; i++) { lo = p[i] < lo ? p[i] : lo; hi = p[i] > hi ? p[i] : hi; }
                if (hi == lo) break;
                const float d = hi - lo;
                const float s = 255.0f / d;
                if (std::isinf(s)) break;  // (d below about 7.5e-37: s is infinite and the plane stays as it is)
                for (uint64_t i = 0; i < N; i++) {
                    const float e = p[i] - lo;
                    const float x = e * s;
                    p[i] = x > 255.0f ? 255.0f : x;
                }
                break;
            }
            case XPNGHIP_TONE_EQUALISE: {
                uint64_t hst[256] = {};
                for (uint64_t i = 0; i < N; i++) hst[(uint32_t)rintf(p[i])]++;
                int last = 255;
                while (!hst[last]) last--;
                const uint64_t step = (N - hst[last]) / 255;
                if (!step) break;
                float lut[256];
                uint64_t sum = step / 2;
                for (int n = 0; n < 256; n++) { lut[n] = (float)std::min<uint64_t>(255, sum / step); sum += hst[n]; }
                for (uint64_t i = 0; i < N; i++) p[i] = lut[(uint32_t)rintf(p[i])];
                break;
            }
            case XPNGHIP_TONE_POSTERISE: {
                const float m = (float)(1u << (8u - (uint32_t)a));
                for (uint64_t i = 0; i < N; i++) p[i] = p[i] - fmodf(p[i], m);
                break;
            }
            case XPNGHIP_TONE_SOLARISE:
                for (uint64_t i = 0; i < N; i++) p[i] = p[i] >= a ? 255.0f - p[i] : p[i];
                break;
            default:  // invert
                for (uint64_t i = 0; i < N; i++) p[i] = 255.0f - p[i];
            }
        }
    }
}
// what the two host rules share: `under` writes the underlying call's values as C fp32 planes (identity constants, no BGR exchange)
// - its own checks included -, the steps run on them, and the caller's constants, colour order, layout and dtype come last
template <class F> static int tone_host_tail(int C, const FloatConsts &k, uint32_t out_w, uint32_t out_h, uint32_t layout, uint32_t dtype, const xpnghip_view_tone &tone,
                                              void *out, F under) {
    const uint64_t plane = (uint64_t)out_h * out_w;
    std::vector<float> T((uint64_t)C * plane);
    const float one[4] = {1.0f, 1.0f, 1.0f, 1.0f}, zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (under(XPNGHIP_LAYOUT_PLANAR | ((uint32_t)C << 8), one, zero, T.data())) return 1;
    tone_planes_host(T.data(), plane, tone);
    const bool planar = layout & XPNGHIP_LAYOUT_PLANAR, bgr = layout & XPNGHIP_LAYOUT_BGR;
    const HostOut ho{out, dtype, planar, C, out_w, out_h};
    for (uint32_t oy = 0; oy < out_h; oy++)
        for (uint32_t ox = 0; ox < out_w; ox++)
            for (int c = 0; c < C; c++) host_element(ho, k, ox, oy, c, T[(uint64_t)(c == 3 ? 3 : bgr ? 2 - c : c) * plane + (uint64_t)oy * out_w + ox]);
    return 0;
}
static int resample_tone_host_impl(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w, uint32_t out_h,
                                   uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *colour,
                                   const xpnghip_view_blur *blur, const xpnghip_view_tone *tone, void *out) {
    std::string why;
    if (tone && !tone_record_ok(*tone, "", why)) return fail(why);
    if (!tone || tone_off(*tone)) return resample_blur_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, filter, colour, blur, out);
    if (!blur_filter_ok(filter, why)) return fail(why);
    int C;
    FloatConsts k;
    ResizeRec z0;
    if (resize_host_args("xpnghip_resample_tone_host", pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, out, C, k, z0)) return 1;
    return tone_host_tail(C, k, out_w, out_h, layout, dtype, *tone, out, [&](uint32_t tl, const float *one, const float *zero, float *T) {
        return resample_blur_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, tl, XPNGHIP_DTYPE_F32, one, zero, filter, colour, blur, T);
    });
}
extern "C" int xpnghip_resample_tone_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const uint64_t *rect, int flip, uint32_t out_w,
                                          uint32_t out_h, uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter,
                                          const float *colour, const xpnghip_view_blur *blur, const xpnghip_view_tone *tone, void *out) {
    XPNG_GUARDED(resample_tone_host_impl(pxsz, raster, w, h, rect, flip, out_w, out_h, layout, dtype, scale, bias, filter, colour, blur, tone, out))
}
static int resample_affine_tone_host_impl(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const float *affine, uint32_t out_w, uint32_t out_h,
                                          uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *fill,
                                          const float *colour, const xpnghip_view_tone *tone, void *out) {
    std::string why;
    if (tone && !tone_record_ok(*tone, "", why)) return fail(why);
    if (!tone || tone_off(*tone)) return resample_affine_host_impl(pxsz, raster, w, h, affine, out_w, out_h, layout, dtype, scale, bias, filter, fill, colour, out);
    if (!affine_filter_ok(filter, why)) return fail(why);
    int C;
    FloatConsts k;
    ResizeRec z0;
    if (resize_host_args("xpnghip_resample_affine_tone_host", pxsz, raster, w, h, nullptr, 0, out_w, out_h, layout, dtype, scale, bias, out, C, k, z0)) return 1;
    return tone_host_tail(C, k, out_w, out_h, layout, dtype, *tone, out, [&](uint32_t tl, const float *one, const float *zero, float *T) {
        return resample_affine_host_impl(pxsz, raster, w, h, affine, out_w, out_h, tl, XPNGHIP_DTYPE_F32, one, zero, filter, fill, colour, T);
    });
}
extern "C" int xpnghip_resample_affine_tone_host(int pxsz, const uint8_t *raster, uint64_t w, uint64_t h, const float *affine, uint32_t out_w, uint32_t out_h,
                                                 uint32_t layout, uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *fill,
                                                 const float *colour, const xpnghip_view_tone *tone, void *out) {
    XPNG_GUARDED(resample_affine_tone_host_impl(pxsz, raster, w, h, affine, out_w, out_h, layout, dtype, scale, bias, filter, fill, colour, tone, out))
}
// ---- staging from tensors (stage_from.hpp) ---------------------------------------------------------------------
// the layout word of a call whose channel count is per image: the PLANAR and BGR bits and nothing else
static bool stage_layout_ok(uint32_t layout, std::string &why) {
    if (!(layout & ~(XPNGHIP_LAYOUT_PLANAR | XPNGHIP_LAYOUT_BGR))) return true;
    why = "bad layout word " + layout_hex(layout) + " (XPNGHIP_LAYOUT_PLANAR | XPNGHIP_LAYOUT_BGR only: the channel count is an argument of its own)";
    return false;
}
// dtype 0 (uint8) takes no constants; 1 .. 3 as in the float call
static bool stage_dtype_ok(uint32_t dtype, const float *scale, const float *bias, std::string &why) {
    if (dtype > XPNGHIP_DTYPE_F32) { why = "bad dtype " + std::to_string(dtype) + " (0 = uint8, XPNGHIP_DTYPE_F16 = 1, _BF16 = 2, _F32 = 3)"; return false; }
    if (dtype == 0 && (scale || bias)) { why = std::string(scale ? "scale" : "bias") + " given with dtype 0: a uint8 buffer is stored as it is"; return false; }
    return true;
}
// the bits of an f16 widened to fp32: exact, subnormals kept (what v_cvt_f32_f16 gives on the device)
static float f16_bits_to_f32(uint16_t hb) {
    const uint32_t sign = (uint32_t)(hb & 0x8000u) << 16, e = (hb >> 10) & 0x1Fu, m = hb & 0x3FFu;
    uint32_t x;
    if (e == 0x1F) x = sign | 0x7F800000u | (m << 13);
    else if (e) x = sign | ((e + 112u) << 23) | (m << 13);
    else if (!m) x = sign;
    else {  // subnormal: m * 2^-24
        uint32_t k = m, sh = 0;
        while (!(k & 0x400u)) { k <<= 1; sh++; }
        x = sign | ((113u - sh) << 23) | ((k & 0x3FFu) << 13);
    }
    float f;
    memcpy(&f, &x, 4);
    return f;
}
// The twin of k_images_stage_from's arithmetic on the host: the same operations in the same order, the multiply-add an explicit
// fmaf(), contraction off on top of that.
static uint8_t quantize_one_host(uint32_t dtype, const uint8_t *p, float s, float b) {
#pragma clang fp contract(off)
    float x;
    if (dtype == XPNGHIP_DTYPE_F32) memcpy(&x, p, 4);
    else {
        uint16_t hb;
        memcpy(&hb, p, 2);
        if (dtype == XPNGHIP_DTYPE_F16) x = f16_bits_to_f32(hb);
        else { const uint32_t w = (uint32_t)hb << 16; memcpy(&x, &w, 4); }
    }
    const float y = fmaf(x, s, b);
    if (!(y > 0.0f)) return 0;  // NaN, -0, -inf
    if (y >= 255.0f) return 255;
    return (uint8_t)nearbyintf(y);  // (the default rounding mode: half to even)
}
static int quantize_host_impl(uint32_t layout, uint32_t dtype, int C, const void *src, uint64_t npx, const float *scale, const float *bias, uint8_t *out) {
    std::string why;
    if (!stage_layout_ok(layout, why)) return fail(why);
    if (!stage_dtype_ok(dtype, scale, bias, why)) return fail(why);
    if (C != 3 && C != 4) return fail("xpnghip_quantize_host: C is " + std::to_string(C) + ", not 3 or 4");
    FloatConsts k;
    if (!float_consts(C, scale, bias, k, why)) return fail(why);
    if (!src || !out) return fail("xpnghip_quantize_host: null source or output buffer");
    if (npx > (1ull << 48)) return fail("xpnghip_quantize_host: npx is " + std::to_string(npx) + ", more than 2^48");
    const bool planar = layout & XPNGHIP_LAYOUT_PLANAR, bgr = layout & XPNGHIP_LAYOUT_BGR;
    const uint64_t es = dtype ? (uint64_t)xpnghip_dtype_bytes(dtype) : 1;
    const uint8_t *s = static_cast<const uint8_t *>(src);
    for (uint64_t p = 0; p < npx; p++)
        for (int c = 0; c < C; c++) {
            const int cc = bgr && c < 3 ? 2 - c : c;  // the channel's position in the caller's buffer
            const uint64_t e = planar ? (uint64_t)cc * npx + p : p * C + cc;
            out[p * C + c] = dtype ? quantize_one_host(dtype, s + e * es, k.scale[cc], k.bias[cc]) : s[e];
        }
    return 0;
}
extern "C" int xpnghip_quantize_host(uint32_t layout, uint32_t dtype, int C, const void *src, uint64_t npx, const float *scale, const float *bias, uint8_t *out) {
    XPNG_GUARDED(quantize_host_impl(layout, dtype, C, src, npx, scale, bias, out))
}
// one launch for the images of C channels of a staged batch
template <int C>
static void launch_stage_from(const ImgRec *rec, const uint8_t *const *srcs, dim3 grid, uint32_t layout, uint32_t dtype, const FloatConsts &k, hipStream_t s) {
    const uint32_t bgr = layout & XPNGHIP_LAYOUT_BGR;
    with_planar(layout, [&](auto PL) {
        constexpr bool P = decltype(PL)::value;
        if (dtype == 0) k_images_stage_from<C, P, uint8_t><<<grid, 256, 0, s>>>(rec, srcs, bgr, k);
        else with_float(dtype, [&](auto t) { k_images_stage_from<C, P, decltype(t)><<<grid, 256, 0, s>>>(rec, srcs, bgr, k); });
    });
}
// The rectangle table of a resized call: allocated on first use, uploaded by EVERY call (rectangles change with every batch, so
// there is nothing to cache).  The records are in pageable host memory that dies with this call, so the stream is synchronised
// behind the copy.  The copy is queued before the decode's own kernels, so that wait covers only what the caller had queued on the
// stream earlier, never this call's work.
static int resize_records(xpnghip_ctx *c, const std::vector<ResizeRec> &recs, hipStream_t s) {
    const uint64_t bytes = (uint64_t)c->B * sizeof(ResizeRec);
    WS_GET(c->d_m_rect, bytes);
    HIPCHK(hipMemcpyAsync(c->d_m_rect, recs.data(), bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}
// ... and the table of a resampled call with filter 1, in its place and by the same protocol
static int resample_records(xpnghip_ctx *c, const std::vector<ResizeRec> &recs, hipStream_t s) {
    std::vector<ResampleRec> rr(recs.size());
    for (size_t i = 0; i < recs.size(); i++) rr[i] = resample_record(recs[i]);
    const uint64_t bytes = (uint64_t)c->B * sizeof(ResampleRec);
    WS_GET(c->d_m_rsmp, bytes);
    HIPCHK(hipMemcpyAsync(c->d_m_rsmp, rr.data(), bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// The staging raster of the tight forms (decode: reconstruct into it, k_mixed_copy out of it; encode: k_mixed_pack into it, the
// kernels read it): image i's h_i rows at the pitch bpr in slot[i], every slot 256-byte aligned, 256 spare bytes behind the last.
// ONE layout and one buffer for both directions; allocated by the first tight call, never shrunk.
static int mixed_stage_slots(xpnghip_ctx *c, uint64_t bpr, std::vector<uint64_t> &slot) {
    const uint32_t nimg = c->B;
    slot.assign((size_t)nimg + 1, 0);
    for (uint32_t i = 0; i < nimg; i++) slot[i + 1] = slot[i] + rup(c->m_dims[2ull * i + 1] * bpr, 256);
    const uint64_t need = slot[nimg] + 256;
    if (c->cap_m_stage >= need) return 0;
    if (c->d_m_stage) return fail("internal error: the staging raster of a mixed context was allocated for another layout");  // (bpr is a function of the context: this cannot happen)
    WS_GET(c->d_m_stage, need);
    c->cap_m_stage = need;
    return 0;
}

// What every decode call of a mixed context checks first, in this order: the context, the layout word (`layout` == NULL: the file's
// own form), the dtype and the constants of a float call (`fc` == NULL: bytes), the mode, the number of images, the arrays.  Gives
// the channels and the element size of the caller's buffers and the constants.
static int mixed_decode_args(const xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg, void *const *d_outs,
                             const uint32_t *layout, const FloatCall *fc, int &C, int &es, FloatConsts &fk) {
    if (!c) return fail("null context");
    if (!c->mixed) return fail("not a mixed context (xpnghip_ctx_create_mixed)");
    C = layout ? xpnghip_layout_channels(*layout, c->pxsz) : c->pxsz;
    if (C < 0) return fail("bad layout word " + layout_hex(*layout) + " (XPNGHIP_LAYOUT_PLANAR | XPNGHIP_LAYOUT_BGR | channels 0, 3 or 4 in bits 8..11)");
    es = fc ? xpnghip_dtype_bytes(fc->dtype) : 1;
    if (es < 0)
        return fail("bad dtype " + std::to_string(fc->dtype) + " (XPNGHIP_DTYPE_F16 = 1, _BF16 = 2, _F32 = 3; uint8 buffers are written by xpnghip_decode_varsize_device_batch_as)");
    if (fc) {
        std::string why;
        if (!float_consts(C, fc->scale, fc->bias, fk, why)) return fail(why);
    }
    if (mode != 1 && mode != 2) return fail("tile mode must be 1 or 2");
    if (mode == 2 && c->pxsz != 3) return fail("mode 2 codes RGB only");
    if (nimg != c->B) return fail("nimg is " + std::to_string(nimg) + ", the mixed context holds " + std::to_string(c->B) + " images");
    if (!d_blobs || !blobs_len || !d_outs) return fail("null argument");
    return 0;
}

// `layout` != NULL: the call of xpnghip_decode_varsize_device_batch_as (out_bpr == 0: its buffers are tight); `fc` != NULL beside
// it: the call of xpnghip_decode_varsize_device_batch_as_float (its buffers hold elements of fc->dtype); `rz` != NULL beside both:
// the call of xpnghip_decode_varsize_device_batch_resized (every buffer holds C * rz->out_h * rz->out_w such elements), or with
// rz->filter that of xpnghip_decode_varsize_device_batch_resampled
static int decode_mixed_batch_impl(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                   const uint64_t *tile_off, void *const *d_outs, uint64_t out_bpr, void *stream, const uint32_t *layout = nullptr,
                                   const FloatCall *fc = nullptr, const ResizeCall *rz = nullptr) {
    // every argument is checked before anything reaches the device: a rejected call writes nothing
    int C, es;
    FloatConsts fk{};
    if (mixed_decode_args(c, mode, d_blobs, blobs_len, nimg, d_outs, layout, fc, C, es, fk)) return 1;
    // (interleaved, the file's colour order and channel count: the tight form itself, k_mixed_copy and its records)
    const bool as = !fc && layout && ((*layout & (XPNGHIP_LAYOUT_PLANAR | XPNGHIP_LAYOUT_BGR)) || C != c->pxsz);
    const uint64_t px = (uint64_t)c->pxsz, widest = c->m_max_w * px;
    if (out_bpr && out_bpr < widest)
        return fail("out_bpr " + std::to_string(out_bpr) + " is smaller than the widest row of the batch (" + std::to_string(widest) + " bytes)");
    std::vector<ResizeRec> recs;
    if (rz) {
        std::string why;
        if (!resample_filter_ok(rz->filter, why)) return fail(why);
        if (!resize_size_ok(rz->out_w, rz->out_h, why)) return fail(why);
        recs.resize(nimg);
        for (uint32_t i = 0; i < nimg; i++)
            if (!resize_record(c->m_dims[2ull * i], c->m_dims[2ull * i + 1], rz->rects ? rz->rects + 4ull * i : nullptr, rz->flips ? rz->flips[i] : 0u,
                               rz->out_w, rz->out_h, recs[i], why))
                return fail(why + " (image " + std::to_string(i) + ")");
    }
    for (uint32_t i = 0; i < nimg; i++) {
        if (!d_blobs[i] || !d_outs[i]) return fail("null blob or output buffer of image " + std::to_string(i));
        if (((uintptr_t)d_blobs[i] & 3) || (out_bpr && ((uintptr_t)d_outs[i] & 15))) return fail("device buffers must be 16-byte aligned");
        if ((uintptr_t)d_outs[i] & (uintptr_t)(es - 1)) {
            char b[32];
            snprintf(b, sizeof b, "%p", d_outs[i]);
            return fail("output buffer " + std::string(b) + " of image " + std::to_string(i) + " is not aligned to its " + std::to_string(es) + "-byte elements");
        }
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    const uint64_t bpr = out_bpr ? out_bpr : rup(widest, 16);  // (staging rows start 16-byte aligned: the recon kernels take any pitch)
    std::vector<void *> base(d_outs, d_outs + nimg);
    if (!out_bpr) {
        // tight rasters: reconstruct into a staging raster at the widest image's pitch, rounded up to 16 bytes (image i: h_i rows,
        // its slot 256-byte aligned), then k_mixed_copy moves every image out at its own pitch
        std::vector<uint64_t> slot;
        if (mixed_stage_slots(c, bpr, slot)) return 1;
        if (mixed_records(c, c->d_m_out, c->h_m_out, slot, d_outs, s)) return 1;
        if (rz && (rz->filter == XPNGHIP_FILTER_TRIANGLE_AA ? resample_records(c, recs, s) : resize_records(c, recs, s))) return 1;
        for (uint32_t i = 0; i < nimg; i++) base[i] = c->d_m_stage + slot[i];
    }
    if (dec_prepare(c, mode, d_blobs, blobs_len, nimg, base.data(), s)) return 1;
    XPNG_REQUIRE(c->d_m_first, c->d_m_list);
    const int rc = dec_launch(c, mode, nimg, c->m_max_w, tile_off, s, 0, (uint32_t)c->tiles.size(), &c->m_list, c->d_m_list, bpr);
    if (rc) return rc;
    if (rz || fc || as) {
        XPNG_REQUIRE(c->d_m_stage, c->d_m_out);
        const bool aa = rz && rz->filter == XPNGHIP_FILTER_TRIANGLE_AA;
        if (rz) XPNG_REQUIRE(aa ? (const void *)c->d_m_rsmp : (const void *)c->d_m_rect);
        const uint32_t bgr = *layout & XPNGHIP_LAYOUT_BGR;
        with_3or4(c->pxsz, [&](auto PXc) { with_3or4(C, [&](auto Cc) { with_planar(*layout, [&](auto PL) {
            constexpr int PX = decltype(PXc)::value, CH = decltype(Cc)::value;
            constexpr bool P = decltype(PL)::value;
            if (aa) {
                with_float(fc->dtype, [&](auto t) {
                    k_mixed_resample_as_float<PX, CH, P, decltype(t)><<<mixed_grid(c, rz->out_h), 256, 0, s>>>(c->d_m_out, c->d_m_rsmp, c->d_m_stage, bpr, bgr, rz->out_w, rz->out_h, fk);
                });
            } else if (rz) {
                with_float(fc->dtype, [&](auto t) {
                    k_mixed_resize_as_float<PX, CH, P, decltype(t)><<<mixed_grid(c, rz->out_h), 256, 0, s>>>(c->d_m_out, c->d_m_rect, c->d_m_stage, bpr, bgr, rz->out_w, rz->out_h, fk);
                });
            } else if (fc) {
                with_float(fc->dtype, [&](auto t) {
                    k_mixed_copy_as_float<PX, CH, P, decltype(t)><<<mixed_grid(c, c->m_max_h), 256, 0, s>>>(c->d_m_out, c->d_m_stage, bpr, bgr, fk);
                });
            } else k_mixed_copy_as<PX, CH, P><<<mixed_grid(c, c->m_max_h), 256, 0, s>>>(c->d_m_out, c->d_m_stage, bpr, bgr);
        }); }); });
        HIPCHK(hipGetLastError());
    } else if (!out_bpr) {
        XPNG_REQUIRE(c->d_m_stage, c->d_m_out);
        k_mixed_copy<<<mixed_grid(c, c->m_max_h), 256, 0, s>>>(c->d_m_out, c->d_m_stage, bpr, (uint32_t)px);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
extern "C" int xpnghip_decode_mixed_device_batch(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                 const uint64_t *tile_off, void *const *d_outs, uint64_t out_bpr, void *stream) {
    XPNG_GUARDED(decode_mixed_batch_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, d_outs, out_bpr, stream))
}
extern "C" int xpnghip_decode_varsize_device_batch_as(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                      const uint64_t *tile_off, void *const *d_outs, uint32_t layout, void *stream) {
    XPNG_GUARDED(decode_mixed_batch_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, d_outs, 0, stream, &layout))
}
extern "C" int xpnghip_decode_varsize_device_batch_as_float(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                            const uint64_t *tile_off, void *const *d_outs, uint32_t layout, uint32_t dtype,
                                                            const float *scale, const float *bias, void *stream) {
    const FloatCall fc{dtype, scale, bias};
    XPNG_GUARDED(decode_mixed_batch_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, d_outs, 0, stream, &layout, &fc))
}
extern "C" int xpnghip_decode_varsize_device_batch_resized(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                           const uint64_t *tile_off, void *const *d_outs, uint32_t layout, uint32_t dtype,
                                                           const float *scale, const float *bias, const uint64_t *rects, const uint8_t *flips,
                                                           uint32_t out_w, uint32_t out_h, void *stream) {
    const FloatCall fc{dtype, scale, bias};
    const ResizeCall rz{rects, flips, out_w, out_h};
    XPNG_GUARDED(decode_mixed_batch_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, d_outs, 0, stream, &layout, &fc, &rz))
}
extern "C" int xpnghip_decode_varsize_device_batch_resampled(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                             const uint64_t *tile_off, void *const *d_outs, uint32_t layout, uint32_t dtype,
                                                             const float *scale, const float *bias, const uint64_t *rects, const uint8_t *flips,
                                                             uint32_t out_w, uint32_t out_h, uint32_t filter, void *stream) {
    const FloatCall fc{dtype, scale, bias};
    const ResizeCall rz{rects, flips, out_w, out_h, filter};
    XPNG_GUARDED(decode_mixed_batch_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, d_outs, 0, stream, &layout, &fc, &rz))
}

// ---- several views per image, only the tiles they touch (mixed_views.hpp) -----------------------------------------
// what the two entry points below check alike: the number of views, the image of every view and its rectangle (NULL: whole images)
static bool view_args_ok(const uint64_t *dims, uint32_t nimg, uint32_t nviews, const uint32_t *view_image, const uint64_t *rects, std::string &why) {
    if (nviews < 1 || nviews > 65535) { why = "nviews is " + std::to_string(nviews) + ", not 1 .. 65535"; return false; }
    if (!view_image && nviews != nimg) {
        why = "view_image is NULL (the identity) but nviews is " + std::to_string(nviews) + " and nimg " + std::to_string(nimg);
        return false;
    }
    for (uint32_t v = 0; v < nviews; v++) {
        const uint32_t i = view_image ? view_image[v] : v;
        if (i >= nimg) { why = "view_image[" + std::to_string(v) + "] is " + std::to_string(i) + ", the batch holds " + std::to_string(nimg) + " images"; return false; }
        if (!rects) continue;
        const uint64_t W = dims[2ull * i], H = dims[2ull * i + 1], *r = rects + 4ull * v;
        if (!region_valid(W, H, r)) {
            why = "bad rectangle {" + std::to_string(r[0]) + ", " + std::to_string(r[1]) + ", " + std::to_string(r[2]) + ", " + std::to_string(r[3]) +
                  "}: it is empty or leaves the " + std::to_string(W) + " x " + std::to_string(H) + " image (view " + std::to_string(v) + ", image " + std::to_string(i) + ")";
            return false;
        }
    }
    return true;
}
// The launch list of a views call: `sorted` - every index of the concatenated table `tiles` by decreasing pixel count, equal sizes in
// table order; image i owns [first[i], first[i + 1]) - without the tiles that no view of their image touches (region_select's
// test).  The arguments have passed view_args_ok.
static void view_select(const std::vector<TileDesc> &tiles, const std::vector<uint32_t> &first, const std::vector<uint32_t> &sorted, const uint64_t *dims,
                        uint32_t nviews, const uint32_t *view_image, const uint64_t *rects, std::vector<uint32_t> &out) {
    std::vector<uint8_t> keep(tiles.size(), 0);
    std::vector<TileDesc> one;
    std::vector<uint32_t> sel;
    for (uint32_t v = 0; v < nviews; v++) {
        const uint32_t i = view_image ? view_image[v] : v;
        const uint64_t whole[4] = {0, 0, dims[2ull * i], dims[2ull * i + 1]};
        if (rects && !(rects[4ull * v + 2] && rects[4ull * v + 3])) continue;  // (an affine view's empty footprint selects nothing; a rectangle of the other calls is never empty: view_args_ok)
        one.assign(tiles.begin() + first[i], tiles.begin() + first[i + 1]);
        region_select(one, rects ? rects + 4ull * v : whole, sel);
        for (uint32_t t : sel) keep[first[i] + t] = 1;
    }
    out.clear();
    for (uint32_t t : sorted) if (keep[t]) out.push_back(t);
}
// the launch list over images of `dims`; `affines` (with out_sizes) replaces the rectangles by the footprints of the views
static int64_t view_tiles_impl(const uint64_t *dims, uint32_t nimg, uint32_t nviews, const uint32_t *view_image, const uint64_t *rects,
                               const float *affines, const uint32_t *out_sizes, uint32_t *tiles, uint64_t cap) {
    try {
        if (!dims || nimg < 1 || nimg > 4096) return -1;
        for (uint32_t i = 0; i < 2 * nimg; i++) if (!dims[i] || dims[i] > (1u << 24)) return -1;
        std::string why;
        if (!view_args_ok(dims, nimg, nviews, view_image, rects, why)) return -1;
        std::vector<uint64_t> foot;
        if (affines) {
            if (!out_sizes) return -1;
            foot.resize(4ull * nviews);
            for (uint32_t v = 0; v < nviews; v++) {
                const uint32_t i = view_image ? view_image[v] : v;
                if (!resize_size_ok(out_sizes[2ull * v], out_sizes[2ull * v + 1], why)) return -1;
                if (!affine_footprint(dims[2ull * i], dims[2ull * i + 1], affines + 6ull * v, out_sizes[2ull * v], out_sizes[2ull * v + 1], "", &foot[4ull * v], why)) return -1;
            }
            rects = foot.data();
        }
        // the concatenated table and its size-sorted list, as xpnghip_ctx_create_mixed builds them
        std::vector<TileDesc> all, one;
        std::vector<uint32_t> first((size_t)nimg + 1);
        for (uint32_t i = 0; i < nimg; i++) {
            build_tiles(dims[2ull * i], dims[2ull * i + 1], one);
            first[i] = (uint32_t)all.size();
            all.insert(all.end(), one.begin(), one.end());
            if (all.size() > 0xFFFFFFFFull) return -1;
        }
        first[nimg] = (uint32_t)all.size();
        std::vector<uint32_t> sorted(all.size()), list;
        for (size_t i = 0; i < all.size(); i++) sorted[i] = (uint32_t)i;
        std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return all[a].n > all[b].n; });
        view_select(all, first, sorted, dims, nviews, view_image, rects, list);
        if (list.size() > cap || !tiles) return -1;
        std::copy(list.begin(), list.end(), tiles);
        return (int64_t)list.size();
    } catch (...) { return -1; }
}
extern "C" int64_t xpnghip_view_tiles(const uint64_t *dims, uint32_t nimg, uint32_t nviews, const uint32_t *view_image, const uint64_t *rects,
                                      uint32_t *tiles, uint64_t cap) {
    return view_tiles_impl(dims, nimg, nviews, view_image, rects, nullptr, nullptr, tiles, cap);
}
extern "C" int64_t xpnghip_affine_view_tiles(const uint64_t *dims, uint32_t nimg, uint32_t nviews, const uint32_t *view_image, const float *affines,
                                             const uint32_t *out_sizes, uint32_t *tiles, uint64_t cap) {
    if (!affines) return -1;
    return view_tiles_impl(dims, nimg, nviews, view_image, nullptr, affines, out_sizes, tiles, cap);
}
extern "C" uint64_t xpnghip_ctx_last_decode_tiles(const xpnghip_ctx *c) { return c ? c->last_tiles : 0; }

// A grow-on-demand table of the views calls: `cap` is what ptr has room for, `need` what this call asks for, both in the table's
// own unit.  A table that is too small is dropped and allocated anew.  An earlier call's copy-out may still read the old one - the
// context's work is on these streams - so they are synchronised first, and only when there is an old table.
#define VIEWS_TABLE(ptr, cap, need, bytes)                                                                 \
    do {                                                                                                  \
        if ((cap) < (need)) {                                                                             \
            if (ptr)                                                                                      \
                for (hipStream_t q : {s, c->stream, c->side}) if (q) HIPCHK(hipStreamSynchronize(q));     \
            c->ws.drop((void **)&(ptr)); (cap) = 0;                                                       \
            WS_GET(ptr, bytes);                                                                           \
            (cap) = (need);                                                                               \
        }                                                                                                 \
    } while (0)
// What the seven views entry points differ in, filled by field name: the rectangles and flips (NULL: whole images, no flip), the
// filter word, the colour matrices (nviews * 12 floats; NULL: none), whether the call takes the cubic rule (it has no filter word
// then), the blur records (NULL: none) and, where `affine` is set, nviews * 6 floats and the fill (NULL: zeros) in place of
// rectangles and flips; the tone records (NULL: none) of the two tone calls
struct ViewsCall {
    const uint64_t *rects = nullptr;
    const uint8_t *flips = nullptr;
    uint32_t filter = 0;
    const float *colours = nullptr;
    bool cubic = false;
    const xpnghip_view_blur *blurs = nullptr;
    bool affine = false;
    const float *affines = nullptr, *fill = nullptr;
    const xpnghip_view_tone *tones = nullptr;
};
static int decode_views_impl(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg, const uint64_t *tile_off,
                             uint32_t nviews, const uint32_t *view_image, void *const *d_outs, const uint32_t *out_sizes, uint32_t layout,
                             uint32_t dtype, const float *scale, const float *bias, void *stream, const ViewsCall &vc) {
    // every argument is checked before anything reaches the device: a rejected call writes nothing
    int C, es;
    FloatConsts fk{};
    const FloatCall fc{dtype, scale, bias};
    if (mixed_decode_args(c, mode, d_blobs, blobs_len, nimg, d_outs, &layout, &fc, C, es, fk)) return 1;  // (everything the float call refuses)
    std::string why;
    const float *colours = vc.colours;  // (re-pointed below at the partitioned copy of a call with second-pass views)
    if (vc.affine ? !affine_filter_ok(vc.filter, why) : !vc.cubic && !resample_filter_ok(vc.filter, why)) return fail(why);  // (the cubic call has no filter word)
    if (!out_sizes) return fail("out_sizes is NULL: a views call needs the pair {out_w, out_h} of every view");
    if (vc.affine && !vc.affines) return fail("affines is NULL: an affine views call needs the six floats of every view");
    if (!view_args_ok(c->m_dims.data(), nimg, nviews, view_image, vc.rects, why)) return fail(why);
    // an affine call has no rectangles and no flips: its matrices and its fill are checked in their place, and the footprints of
    // its views are the rectangles of the selection
    std::vector<AffineRec> arecs(vc.affine ? nviews : 0);
    std::vector<uint64_t> foot(vc.affine ? 4ull * nviews : 0);
    AffineFill afill{};
    if (vc.affine) {
        if (!affine_fill_ok(vc.fill, why)) return fail(why);
        for (int e = 0; vc.fill && e < 4; e++) afill.v[e] = vc.fill[e];
    }
    const uint64_t px = (uint64_t)c->pxsz, bpr = rup(c->m_max_w * px, 16);
    std::vector<uint64_t> slot((size_t)nimg + 1, 0);  // (mixed_stage_slots' layout: the refusals below come before anything is allocated)
    for (uint32_t i = 0; i < nimg; i++) slot[i + 1] = slot[i] + rup(c->m_dims[2ull * i + 1] * bpr, 256);
    std::vector<ViewRec> recs(nviews);
    uint32_t max_oh = 0;
    for (uint32_t v = 0; v < nviews; v++) {
        const uint32_t i = view_image ? view_image[v] : v, ow = out_sizes[2ull * v], oh = out_sizes[2ull * v + 1];
        const std::string who = " (view " + std::to_string(v) + ", image " + std::to_string(i) + ")";
        ResizeRec z;
        if (!resize_size_ok(ow, oh, why)) return fail(why + who);
        if (vc.affine) {
            if (!affine_footprint(c->m_dims[2ull * i], c->m_dims[2ull * i + 1], vc.affines + 6ull * v, ow, oh, " of view " + std::to_string(v), &foot[4ull * v], why)) return fail(why);
        } else if (!resize_record(c->m_dims[2ull * i], c->m_dims[2ull * i + 1], vc.rects ? vc.rects + 4ull * v : nullptr, vc.flips ? vc.flips[v] : 0u, ow, oh, z, why)) return fail(why + who);
        if (!d_outs[v]) return fail("null output buffer of view " + std::to_string(v));
        if ((uintptr_t)d_outs[v] & (uintptr_t)(es - 1)) {
            char b[32];
            snprintf(b, sizeof b, "%p", d_outs[v]);
            return fail("output buffer " + std::string(b) + " of view " + std::to_string(v) + " is not aligned to its " + std::to_string(es) + "-byte elements");
        }
        if (vc.affine) {
            max_oh = std::max(max_oh, oh);
            const float *m = vc.affines + 6ull * v;
            const uint64_t *f = &foot[4ull * v];
            arecs[v] = AffineRec{slot[i], (uint8_t *)d_outs[v], {m[0], m[1], m[2], m[3], m[4], m[5]}, ow, oh,
                                 (int32_t)f[0], (int32_t)f[1], (int32_t)(f[0] + f[2]), (int32_t)(f[1] + f[3])};
            continue;
        }
        const ResampleRec q = resample_record(z);  // (the four ratios exactly as the resized and the resampled calls compute them)
        recs[v] = ViewRec{slot[i], (uint8_t *)d_outs[v], q.rx, q.ry, q.rw, q.rh, ow, oh, q.kx, q.ky, q.ikx, q.iky, q.flip, 0};
        max_oh = std::max(max_oh, oh);
    }
    for (uint32_t i = 0; i < nimg; i++) {
        if (!d_blobs[i]) return fail("null blob of image " + std::to_string(i));
        if ((uintptr_t)d_blobs[i] & 3) return fail("device buffers must be 16-byte aligned");
    }
    for (uint32_t v = 0; colours && v < nviews; v++)
        if (!colour_matrix_ok(colours + 12ull * v, " of view " + std::to_string(v), why)) return fail(why);
    // the views that blur or solarise take two passes (mixed_views_blur.hpp): the tables are partitioned, plain views first, and each
    // copy-out launch gets its part by pointer offset.  Without such a view nothing below differs from the underlying call
    std::vector<uint32_t> order(nviews);
    for (uint32_t v = 0; v < nviews; v++) order[v] = v;
    // A view with a tone step (mixed_views_tone.hpp) is a second-pass view too: its first pass goes into the scratch as well; where it
    // also blurs, k_mixed_views_blur writes fp32 planes into a SECOND slice (a blur cannot work in place: the `mid` records, behind
    // the others in the blur table); the steps rewrite the last slice in place, and the view's record of the last launch is all off
    uint32_t nplain = nviews, max_oh2 = 0, max_tiles2 = 0, max_tiles_mid = 0, max_chunks = 0, nslots = 0;
    std::vector<BlurRec> brecs, mid;
    std::vector<uint64_t> first_dst, mid_dst;  // where a second-pass view's first pass and a mid record's planes go, in floats of the scratch
    std::vector<ToneRec> trecs;
    std::vector<ViewColour> pcol;
    uint64_t scratch_floats = 0;
    const xpnghip_view_blur blur_none{0.0f, 0u, 256.0f, 0u};
    auto blurred = [&](uint32_t v) { return vc.blurs && !blur_off(vc.blurs[v]); };
    auto toned = [&](uint32_t v) { return vc.tones && !tone_off(vc.tones[v]); };
    auto is_plain = [&](uint32_t v) { return !blurred(v) && !toned(v); };
    if (vc.blurs || vc.tones) {
        for (uint32_t v = 0; vc.blurs && v < nviews; v++)
            if (!blur_record_ok(vc.blurs[v], recs[v].ow, recs[v].oh, " of view " + std::to_string(v), why)) return fail(why);
        for (uint32_t v = 0; vc.tones && v < nviews; v++)
            if (!tone_record_ok(vc.tones[v], " of view " + std::to_string(v), why)) return fail(why);
        std::stable_partition(order.begin(), order.end(), is_plain);
        nplain = 0;
        while (nplain < nviews && is_plain(order[nplain])) nplain++;
    }
    if (nplain < nviews) {
        if (vc.affine) {
            std::vector<AffineRec> part(nviews);
            for (uint32_t i = 0; i < nviews; i++) part[i] = arecs[order[i]];
            arecs.swap(part);
        } else {
            std::vector<ViewRec> part(nviews);
            for (uint32_t i = 0; i < nviews; i++) part[i] = recs[order[i]];
            recs.swap(part);
        }
        if (colours) {
            pcol.resize(nviews);
            for (uint32_t i = 0; i < nviews; i++) memcpy(pcol[i].m, colours + 12ull * order[i], sizeof(ViewColour));
            colours = pcol[0].m;
        }
        max_oh = 0;
        for (uint32_t i = 0; i < nplain; i++) max_oh = std::max(max_oh, out_sizes[2ull * order[i] + 1]);
        brecs.resize(nviews - nplain);
        for (uint32_t i = nplain; i < nviews; i++) {
            const uint32_t v = order[i], ow = out_sizes[2ull * v], oh = out_sizes[2ull * v + 1];
            BlurRec &b = brecs[i - nplain];
            const xpnghip_view_blur &q = blurred(v) ? vc.blurs[v] : blur_none;
            const uint64_t slice = rup((uint64_t)C * oh * ow * 4, 256) / 4;  // (the slice's own planes, rounded up to 256 bytes)
            const uint32_t tiles = ((ow + BLUR_TW - 1) / BLUR_TW) * ((oh + BLUR_TH - 1) / BLUR_TH);
            b = BlurRec{scratch_floats, (uint8_t *)d_outs[v], ow, oh, q.radius, q.solarise, {}};
            blur_weights(q.sigma, q.radius, b.w);
            first_dst.push_back(scratch_floats);
            scratch_floats += slice;
            max_oh2 = std::max(max_oh2, oh);
            max_tiles2 = std::max(max_tiles2, tiles);
            if (!toned(v)) continue;
            if (blurred(v)) {  // the blur moves to a mid record, the last launch's record reads the second slice
                mid.push_back(b);
                mid_dst.push_back(scratch_floats);
                max_tiles_mid = std::max(max_tiles_mid, tiles);
                b = BlurRec{scratch_floats, (uint8_t *)d_outs[v], ow, oh, 0u, 256.0f, {1.0f}};
                scratch_floats += slice;
            }
            const xpnghip_view_tone &t = vc.tones[v];
            ToneRec tr{b.src, oh * ow, {t.op[0], t.op[1], t.op[2], t.op[3]}, {}, {}};
            for (int si = 0; si < 4; si++) {
                tr.arg[si] = t.op[si] == XPNGHIP_TONE_POSTERISE ? (float)(1u << (8u - (uint32_t)t.arg[si])) : t.arg[si];
                if (t.op[si] == XPNGHIP_TONE_AUTOCONTRAST || t.op[si] == XPNGHIP_TONE_EQUALISE) tr.slot[si] = nslots++;
            }
            trecs.push_back(tr);
            max_chunks = std::max(max_chunks, (3u * oh * ow + TONE_CHUNK - 1) / TONE_CHUNK);
        }
    }
    std::vector<uint32_t> list;
    view_select(c->tiles, c->m_first, c->m_list, c->m_dims.data(), nviews, view_image, vc.affine ? foot.data() : vc.rects, list);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    if (mixed_stage_slots(c, bpr, slot)) return 1;
    // (the affine call has a record table of its own and never touches d_m_views)
    if (vc.affine) VIEWS_TABLE(c->d_m_affine, c->cap_m_affine, nviews, (uint64_t)nviews * sizeof(AffineRec));
    else VIEWS_TABLE(c->d_m_views, c->cap_m_views, nviews, (uint64_t)nviews * sizeof(ViewRec));
    WS_GET(c->d_m_vlist, (uint64_t)c->tiles.size() * 4);
    if (colours) VIEWS_TABLE(c->d_m_vcolour, c->cap_m_vcolour, nviews, (uint64_t)nviews * sizeof(ViewColour));
    if (!brecs.empty()) {
        VIEWS_TABLE(c->d_m_bscratch, c->cap_m_bscratch, scratch_floats * 4, scratch_floats * 4);
        VIEWS_TABLE(c->d_m_blur, c->cap_m_blur, brecs.size() + mid.size(), (uint64_t)(brecs.size() + mid.size()) * sizeof(BlurRec));
        // the first pass of these views writes their slices of the scratch
        for (uint32_t i = nplain; i < nviews; i++) {
            uint8_t *dst = (uint8_t *)(c->d_m_bscratch + first_dst[i - nplain]);
            if (vc.affine) arecs[i].buf = dst;
            else recs[i].buf = dst;
        }
        HIPCHK(hipMemcpyAsync(c->d_m_blur, brecs.data(), (uint64_t)brecs.size() * sizeof(BlurRec), hipMemcpyHostToDevice, s));
    }
    if (!mid.empty()) {  // (behind the records of the last launch, in the same table)
        for (size_t i = 0; i < mid.size(); i++) mid[i].buf = (uint8_t *)(c->d_m_bscratch + mid_dst[i]);
        HIPCHK(hipMemcpyAsync(c->d_m_blur + brecs.size(), mid.data(), (uint64_t)mid.size() * sizeof(BlurRec), hipMemcpyHostToDevice, s));
    }
    if (!trecs.empty()) {
        VIEWS_TABLE(c->d_m_tone, c->cap_m_tone, trecs.size(), (uint64_t)trecs.size() * sizeof(ToneRec));
        HIPCHK(hipMemcpyAsync(c->d_m_tone, trecs.data(), (uint64_t)trecs.size() * sizeof(ToneRec), hipMemcpyHostToDevice, s));
        if (nslots) {  // every slot starts from zero in every call: counts, hi and the complement of lo all grow
            VIEWS_TABLE(c->d_m_tstat, c->cap_m_tstat, nslots, (uint64_t)nslots * TONE_SLOT_WORDS * 4);
            HIPCHK(hipMemsetAsync(c->d_m_tstat, 0, (uint64_t)nslots * TONE_SLOT_WORDS * 4, s));
        }
    }
    // the resized call's protocol: both tables are in pageable host memory that ends with this call, so the stream is synchronised
    // once behind the two copies - queued before the decode's own kernels, so the wait never covers this call's work
    if (vc.affine) HIPCHK(hipMemcpyAsync(c->d_m_affine, arecs.data(), (uint64_t)nviews * sizeof(AffineRec), hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemcpyAsync(c->d_m_views, recs.data(), (uint64_t)nviews * sizeof(ViewRec), hipMemcpyHostToDevice, s));
    if (!list.empty()) HIPCHK(hipMemcpyAsync(c->d_m_vlist, list.data(), (uint64_t)list.size() * 4, hipMemcpyHostToDevice, s));
    if (colours) HIPCHK(hipMemcpyAsync(c->d_m_vcolour, colours, (uint64_t)nviews * sizeof(ViewColour), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    XPNG_REQUIRE(c->d_m_first, c->d_m_stage, vc.affine ? (const void *)c->d_m_affine : (const void *)c->d_m_views, c->d_m_vlist);
    if (list.empty()) {
        // an affine call whose views all lie outside their images (every other views call selects a tile: its rectangles are not
        // empty): nothing is decoded, the status is clear and the copy-out below writes the fill
        XPNG_REQUIRE(c->d_status);
        HIPCHK(hipMemsetAsync(c->d_status, 0, 4, s));
        c->last_tiles = 0;
    } else {
        std::vector<void *> base(nimg);
        for (uint32_t i = 0; i < nimg; i++) base[i] = c->d_m_stage + slot[i];
        if (dec_prepare(c, mode, d_blobs, blobs_len, nimg, base.data(), s)) return 1;
        const int rc = dec_launch(c, mode, nimg, c->m_max_w, tile_off, s, 0, (uint32_t)c->tiles.size(), &list, c->d_m_vlist, bpr);
        if (rc) return rc;
    }
    const uint32_t bgr = layout & XPNGHIP_LAYOUT_BGR;
    const dim3 grid((max_oh + MC_ROWS - 1) / MC_ROWS, nplain);
    if (colours) XPNG_REQUIRE(c->d_m_vcolour);
    const ViewColour *vm = colours ? c->d_m_vcolour : nullptr;
    const uint32_t n2 = nviews - nplain;
    const FloatConsts ident{{1.0f, 1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
    if (vc.affine) {  // one kernel for every view: a matrix carries the crop, the size and the mirror
        const dim3 agrid((max_oh + AF_ROWS - 1) / AF_ROWS, nplain);
        if (nplain) with_3or4(c->pxsz, [&](auto PXc) { with_3or4(C, [&](auto Cc) { with_planar(layout, [&](auto PL) { with_float(dtype, [&](auto t) {
            constexpr int PXv = decltype(PXc)::value, Cv = decltype(Cc)::value;
            constexpr bool PLv = decltype(PL)::value;
#ifdef XPNG_PROBES
            // the lane-mapping study (tools/views_affine_timing.py): the siblings' mapping, one output row per wave pass
            if (probe_env("XPNG_AFFINE_ROW_MAP")) { k_mixed_views_affine<PXv, Cv, PLv, decltype(t), 1><<<agrid, 256, 0, s>>>(c->d_m_affine, vm, c->d_m_stage, bpr, bgr, vc.filter, afill, fk); return; }
#endif
            k_mixed_views_affine<PXv, Cv, PLv, decltype(t)><<<agrid, 256, 0, s>>>(c->d_m_affine, vm, c->d_m_stage, bpr, bgr, vc.filter, afill, fk);
        }); }); }); });
        HIPCHK(hipGetLastError());
        if (!n2) return 0;
        // the views with tone steps: the same kernel as <PX, C, planar, float> with no BGR exchange and identity constants into the scratch
        const dim3 agrid1((max_oh2 + AF_ROWS - 1) / AF_ROWS, n2);
        with_3or4(c->pxsz, [&](auto PXc) { with_3or4(C, [&](auto Cc) {
            k_mixed_views_affine<decltype(PXc)::value, decltype(Cc)::value, true, float><<<agrid1, 256, 0, s>>>(c->d_m_affine + nplain, vm ? vm + nplain : nullptr, c->d_m_stage, bpr, 0u, vc.filter, afill, ident);
        }); });
        HIPCHK(hipGetLastError());
    }
    // the copy-out kernel of this call's filter over the records vr (their matrices mats, or none) into buffers of layout PL and
    // element t, as with_planar and with_float hand them over
    auto copy_out = [&](dim3 g, const ViewRec *vr, const ViewColour *mats, auto PL, auto t, uint32_t bgr_, const FloatConsts &k) {
        with_3or4(c->pxsz, [&](auto PXc) { with_3or4(C, [&](auto Cc) {
            constexpr int PXv = decltype(PXc)::value, Cv = decltype(Cc)::value;
            constexpr bool PLv = decltype(PL)::value;
            if (vc.cubic) k_mixed_views_cubic<PXv, Cv, PLv, decltype(t)><<<g, 256, 0, s>>>(vr, mats, c->d_m_stage, bpr, bgr_, k);
            else if (mats) k_mixed_views_colour<PXv, Cv, PLv, decltype(t)><<<g, 256, 0, s>>>(vr, mats, c->d_m_stage, bpr, bgr_, vc.filter, k);
            else k_mixed_views_as_float<PXv, Cv, PLv, decltype(t)><<<g, 256, 0, s>>>(vr, c->d_m_stage, bpr, bgr_, vc.filter, k);
        }); });
    };
    if (!vc.affine && nplain) with_planar(layout, [&](auto PL) { with_float(dtype, [&](auto t) { copy_out(grid, c->d_m_views, vm, PL, t, bgr, fk); }); });
    HIPCHK(hipGetLastError());
    if (brecs.empty()) return 0;
    // the two passes of the views that blur or solarise: the copy-out kernel of the filter as <PX, C, planar, float> with no BGR
    // exchange and identity constants into the scratch, then k_mixed_views_blur into the caller's layout and dtype
    XPNG_REQUIRE(c->d_m_bscratch, c->d_m_blur);
    const dim3 grid1((max_oh2 + MC_ROWS - 1) / MC_ROWS, n2), grid2(max_tiles2, n2);
    if (!vc.affine) copy_out(grid1, c->d_m_views + nplain, vm ? vm + nplain : nullptr, std::true_type{}, float{}, 0u, ident);
    HIPCHK(hipGetLastError());
    if (!trecs.empty()) {
        // the views with tone steps (mixed_views_tone.hpp): where such a view blurs, its blur as fp32 planes into its second slice;
        // then per step index that some view uses a statistics launch - only where some view's step there is autocontrast or
        // equalise - and an apply launch, in place
        XPNG_REQUIRE(c->d_m_tone);
        if (!mid.empty()) {
            with_3or4(C, [&](auto Cc) {
                k_mixed_views_blur<decltype(Cc)::value, true, float><<<dim3(max_tiles_mid, (uint32_t)mid.size()), 256, 0, s>>>(c->d_m_blur + brecs.size(), c->d_m_bscratch, 0u, ident);
            });
            HIPCHK(hipGetLastError());
        }
        const dim3 tgrid(max_chunks, (uint32_t)trecs.size());
        for (uint32_t si = 0; si < 4; si++) {
            bool any = false, stat = false;
            for (const ToneRec &t : trecs) {
                any |= t.op[si] != TONE_NONE;
                stat |= t.op[si] == TONE_AUTOCONTRAST || t.op[si] == TONE_EQUALISE;
            }
            if (!any) break;  // (steps are contiguous: nobody has a later one)
            if (stat) {
                XPNG_REQUIRE(c->d_m_tstat);
                k_mixed_views_tone_stats<<<tgrid, 256, 0, s>>>(c->d_m_tone, c->d_m_bscratch, c->d_m_tstat, si);
            }
            k_mixed_views_tone_apply<<<tgrid, 256, 0, s>>>(c->d_m_tone, c->d_m_bscratch, c->d_m_tstat, si);
            HIPCHK(hipGetLastError());
        }
    }
    with_3or4(C, [&](auto Cc) { with_planar(layout, [&](auto PL) { with_float(dtype, [&](auto t) {
        k_mixed_views_blur<decltype(Cc)::value, decltype(PL)::value, decltype(t)><<<grid2, 256, 0, s>>>(c->d_m_blur, c->d_m_bscratch, bgr, fk);
    }); }); });
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int xpnghip_decode_varsize_device_batch_views(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                         const uint64_t *tile_off, uint32_t nviews, const uint32_t *view_image, void *const *d_outs,
                                                         const uint32_t *out_sizes, const uint64_t *rects, const uint8_t *flips, uint32_t layout,
                                                         uint32_t dtype, const float *scale, const float *bias, uint32_t filter, void *stream) {
    ViewsCall vc;
    vc.rects = rects; vc.flips = flips; vc.filter = filter;
    XPNG_GUARDED(decode_views_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, nviews, view_image, d_outs, out_sizes, layout, dtype, scale, bias, stream, vc))
}
extern "C" int xpnghip_decode_varsize_device_batch_views_colour(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                                const uint64_t *tile_off, uint32_t nviews, const uint32_t *view_image, void *const *d_outs,
                                                                const uint32_t *out_sizes, const uint64_t *rects, const uint8_t *flips, uint32_t layout,
                                                                uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *colours,
                                                                void *stream) {
    ViewsCall vc;
    vc.rects = rects; vc.flips = flips; vc.filter = filter; vc.colours = colours;
    XPNG_GUARDED(decode_views_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, nviews, view_image, d_outs, out_sizes, layout, dtype, scale, bias, stream, vc))
}
// the views-colour call without a filter word: always the cubic rule (mixed_views_cubic.hpp)
extern "C" int xpnghip_decode_varsize_device_batch_views_cubic(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                               const uint64_t *tile_off, uint32_t nviews, const uint32_t *view_image, void *const *d_outs,
                                                               const uint32_t *out_sizes, const uint64_t *rects, const uint8_t *flips, uint32_t layout,
                                                               uint32_t dtype, const float *scale, const float *bias, const float *colours, void *stream) {
    ViewsCall vc;
    vc.rects = rects; vc.flips = flips; vc.colours = colours; vc.cubic = true;
    XPNG_GUARDED(decode_views_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, nviews, view_image, d_outs, out_sizes, layout, dtype, scale, bias, stream, vc))
}
// the views-colour call plus one blur record per view (mixed_views_blur.hpp); filter 2 is the cubic rule, blurs == NULL the
// underlying call itself
extern "C" int xpnghip_decode_varsize_device_batch_views_blur(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                              const uint64_t *tile_off, uint32_t nviews, const uint32_t *view_image, void *const *d_outs,
                                                              const uint32_t *out_sizes, const uint64_t *rects, const uint8_t *flips, uint32_t layout,
                                                              uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *colours,
                                                              const xpnghip_view_blur *blurs, void *stream) {
    std::string why;
    if (!blur_filter_ok(filter, why)) return fail(why);
    ViewsCall vc;
    vc.rects = rects; vc.flips = flips; vc.colours = colours; vc.blurs = blurs;
    vc.cubic = filter == XPNGHIP_FILTER_CUBIC_AA;
    vc.filter = vc.cubic ? 0 : filter;
    XPNG_GUARDED(decode_views_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, nviews, view_image, d_outs, out_sizes, layout, dtype, scale, bias, stream, vc))
}
// the views-colour call with a matrix per view in place of its rectangle and flip, and one fill (mixed_views_affine.hpp)
extern "C" int xpnghip_decode_varsize_device_batch_views_affine(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                                const uint64_t *tile_off, uint32_t nviews, const uint32_t *view_image, void *const *d_outs,
                                                                const uint32_t *out_sizes, const float *affines, const float *fill, uint32_t layout,
                                                                uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *colours,
                                                                void *stream) {
    ViewsCall vc;
    vc.filter = filter; vc.colours = colours; vc.affine = true; vc.affines = affines; vc.fill = fill;
    XPNG_GUARDED(decode_views_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, nviews, view_image, d_outs, out_sizes, layout, dtype, scale, bias, stream, vc))
}
// the blur call and the affine call plus one tone record per view (mixed_views_tone.hpp); tones == NULL is the underlying call itself
extern "C" int xpnghip_decode_varsize_device_batch_views_tone(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                              const uint64_t *tile_off, uint32_t nviews, const uint32_t *view_image, void *const *d_outs,
                                                              const uint32_t *out_sizes, const uint64_t *rects, const uint8_t *flips, uint32_t layout,
                                                              uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *colours,
                                                              const xpnghip_view_blur *blurs, const xpnghip_view_tone *tones, void *stream) {
    std::string why;
    if (!blur_filter_ok(filter, why)) return fail(why);
    ViewsCall vc;
    vc.rects = rects; vc.flips = flips; vc.colours = colours; vc.blurs = blurs; vc.tones = tones;
    vc.cubic = filter == XPNGHIP_FILTER_CUBIC_AA;
    vc.filter = vc.cubic ? 0 : filter;
    XPNG_GUARDED(decode_views_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, nviews, view_image, d_outs, out_sizes, layout, dtype, scale, bias, stream, vc))
}
extern "C" int xpnghip_decode_varsize_device_batch_views_affine_tone(xpnghip_ctx *c, int mode, const void *const *d_blobs, const uint64_t *blobs_len, uint32_t nimg,
                                                                     const uint64_t *tile_off, uint32_t nviews, const uint32_t *view_image, void *const *d_outs,
                                                                     const uint32_t *out_sizes, const float *affines, const float *fill, uint32_t layout,
                                                                     uint32_t dtype, const float *scale, const float *bias, uint32_t filter, const float *colours,
                                                                     const xpnghip_view_tone *tones, void *stream) {
    ViewsCall vc;
    vc.filter = filter; vc.colours = colours; vc.affine = true; vc.affines = affines; vc.fill = fill; vc.tones = tones;
    XPNG_GUARDED(decode_views_impl(c, mode, d_blobs, blobs_len, nimg, tile_off, nviews, view_image, d_outs, out_sizes, layout, dtype, scale, bias, stream, vc))
}

// ---- mixed-size batch encode (mixed.hpp) ---------------------------------------------------------
// The encode workspace of a mixed context, allocated by its first encode: what ctx_create_range_impl allocates for an ordinary
// context, sized from M (the concatenated table) and nimg.  The planes, the stream scratch and the level-2 buffers follow in the
// launch sequences (ensure_planes, ensure_scratch, ensure_m2 / launch_encode_m2).
static int ensure_mixed_encode(xpnghip_ctx *c) {
    if (c->m_enc) return 0;
    if (encode_tables(c, c->tiles.size(), c->B)) return fail("hipMalloc failed (encode workspace of a mixed context)");
    c->m_enc = true;  // (from here on scratch_bytes() includes the encode's share)
    return 0;
}

// `layout` != NULL: the call of xpnghip_encode_varsize_device_batch_from (in_bpr == 0: its buffers are tight)
static int encode_varsize_impl(xpnghip_ctx *c, int mode, const void *const *d_rasters, uint64_t in_bpr, uint32_t nimg, void *const *d_blobs,
                               uint64_t *blobs_len, void *stream, const uint32_t *layout = nullptr) {
    // every argument is checked before anything reaches the device: a rejected call writes nothing
    if (!c) return fail("null context");
    if (!c->mixed) return fail("not a mixed context (xpnghip_ctx_create_mixed)");
    const int C = layout ? xpnghip_layout_channels(*layout, c->pxsz) : c->pxsz;
    if (C < 0) return fail("bad layout word " + layout_hex(*layout) + " (XPNGHIP_LAYOUT_PLANAR | XPNGHIP_LAYOUT_BGR | channels 0, 3 or 4 in bits 8..11)");
    if (C != c->pxsz)
        return fail("the layout has " + std::to_string(C) + " channels, the context " + std::to_string(c->pxsz) + " bytes per pixel: a lossless encoder does not drop or invent a channel");
    // (interleaved in the file's colour order: the tight form itself, k_mixed_pack and its records)
    const bool from = layout && (*layout & (XPNGHIP_LAYOUT_PLANAR | XPNGHIP_LAYOUT_BGR));
    if (mode != 1 && mode != 2) return fail("tile mode must be 1 or 2");
    if (mode == 2 && c->pxsz != 3) return fail("mode 2 codes RGB only (the driver sends RGBA to mode 1, libxpng.c:755)");
    if (nimg != c->B) return fail("nimg is " + std::to_string(nimg) + ", the mixed context holds " + std::to_string(c->B) + " images");
    if (!d_rasters || !d_blobs) return fail("null argument");
    const uint64_t px = (uint64_t)c->pxsz, widest = c->m_max_w * px;
    if (in_bpr && in_bpr < widest)
        return fail("in_bpr " + std::to_string(in_bpr) + " is smaller than the widest row of the batch (" + std::to_string(widest) + " bytes)");
    for (uint32_t i = 0; i < nimg; i++) {
        if (!d_rasters[i] || !d_blobs[i]) return fail("null raster or blob buffer of image " + std::to_string(i));
        if ((uintptr_t)d_blobs[i] & 3) return fail("blob buffer of image " + std::to_string(i) + " must be 4-byte aligned");
        if (in_bpr && ((uintptr_t)d_rasters[i] & 15)) return fail("padded raster of image " + std::to_string(i) + " must be 16-byte aligned");
        if (c->pxsz == 4 && (c->m_dims[2ull * i] < 4 || c->m_dims[2ull * i + 1] < 4))
            return fail("RGBA image " + std::to_string(i) + " is narrower than 4 px: undefined in the reference; store level 7");
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    if (ensure_mixed_encode(c)) return 1;
    const uint64_t bpr = in_bpr ? in_bpr : rup(widest, 16);
    std::vector<const void *> base(d_rasters, d_rasters + nimg);
    if (!in_bpr) {
        // tight rasters: k_mixed_pack brings every image into the staging raster at the widest image's pitch, rounded up to 16 bytes
        // (image i: h_i rows, its slot 256-byte aligned - the buffer, and the layout, of the tight decode), and the kernels read that
        std::vector<uint64_t> slot;
        if (mixed_stage_slots(c, bpr, slot)) return 1;
        if (mixed_records(c, c->d_m_in, c->h_m_in, slot, d_rasters, s)) return 1;
        for (uint32_t i = 0; i < nimg; i++) base[i] = c->d_m_stage + slot[i];
    }
    if (set_ptrs(c, base.data(), d_blobs, nimg, s)) return 1;
    XPNG_REQUIRE(c->d_m_first, c->d_m_list);
    if (from) {
        XPNG_REQUIRE(c->d_m_stage, c->d_m_in);
        const uint32_t bgr = *layout & XPNGHIP_LAYOUT_BGR;
        with_3or4(c->pxsz, [&](auto PXc) { with_planar(*layout, [&](auto PL) {
            k_mixed_pack_from<decltype(PXc)::value, decltype(PL)::value><<<mixed_grid(c, c->m_max_h), 256, 0, s>>>(c->d_m_in, c->d_m_stage, bpr, bgr);
        }); });
        HIPCHK(hipGetLastError());
    } else if (!in_bpr) {
        XPNG_REQUIRE(c->d_m_stage, c->d_m_in);
        k_mixed_pack<<<mixed_grid(c, c->m_max_h), 256, 0, s>>>(c->d_m_in, c->d_m_stage, bpr, (uint32_t)px);
        HIPCHK(hipGetLastError());
    }
    const EncSpan e = enc_span_mixed(c, bpr);
    return enc_finish(c, mode, e, nimg, blobs_len, s);
}
extern "C" int xpnghip_encode_varsize_device_batch(xpnghip_ctx *c, int mode, const void *const *d_rasters, uint64_t in_bpr, uint32_t nimg,
                                                   void *const *d_blobs, uint64_t *blobs_len, void *stream) {
    XPNG_GUARDED(encode_varsize_impl(c, mode, d_rasters, in_bpr, nimg, d_blobs, blobs_len, stream))
}
extern "C" int xpnghip_encode_varsize_device_batch_from(xpnghip_ctx *c, int mode, const void *const *d_rasters, uint32_t layout, uint32_t nimg,
                                                        void *const *d_blobs, uint64_t *blobs_len, void *stream) {
    XPNG_GUARDED(encode_varsize_impl(c, mode, d_rasters, 0, nimg, d_blobs, blobs_len, stream, &layout))
}

// Synchronises `stream` and reports the last decode: 0 = every tile header was consistent, 1 = at least one tile was
// rejected (its pixels were left untouched), -1 = HIP error.
extern "C" int xpnghip_ctx_decode_status(xpnghip_ctx *c, void *stream) {
    if (!c) return -1;
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    // (on the call's own stream, into pinned memory: a plain hipMemcpy runs on the null stream, which waits for every blocking
    //  stream of the device - a caller with several contexts in flight would wait for all of them here, as the pipeline shards of
    //  xpnghip_decode_tiles did: the two early shards "finished" when the last one did)
    volatile uint32_t *hv = reinterpret_cast<volatile uint32_t *>(c->h_total + c->B);  // (h_total has 64 spare bytes behind its B entries)
    if (hipSetDevice(c->device) != hipSuccess || hipMemcpyAsync((void *)hv, c->d_status, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) return -1;
    return (int)(*hv & 1);
}

#include "wrappers.hpp"

// ---- introspection for parity tests ----------------------------------------------------------------------
// wave probe (common.hpp): register a device buffer of `cap` WaveProbe records (nullptr: off); the count so far
#ifdef XPNG_PROBES
extern "C" int xpnghip_debug_probe(void *d_buf, uint32_t cap) {
    WaveProbe *p = (WaveProbe *)d_buf;
    const uint32_t zero = 0;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_probe_buf), &p, sizeof(p)));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_probe_cap), &cap, sizeof(cap)));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_probe_n), &zero, sizeof(zero)));
    return 0;
}
extern "C" int64_t xpnghip_debug_probe_count(void) {
    uint32_t n = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_probe_n), sizeof(n)) != hipSuccess) return -1;
    return n;
}
extern "C" int xpnghip_probes_built(void) { return 1; }
#else
extern "C" int xpnghip_debug_probe(void *, uint32_t) { return fail("the wave probe exists only in libxpng_hip_probes.so (make probes)"); }
extern "C" int64_t xpnghip_debug_probe_count(void) { return -1; }
extern "C" int xpnghip_probes_built(void) { return 0; }
#endif

extern "C" int64_t xpnghip_debug_fetch(xpnghip_ctx *c, int what, uint64_t tile, void *out, uint64_t cap) {
    if (!c || c->mixed || tile >= c->tiles.size() || !out) return -1;  // (the introspection is the ordinary context's)
    if (hipSetDevice(c->device) != hipSuccess || (c->stream && hipStreamSynchronize(c->stream) != hipSuccess)) return -1;  // (debug_fetch follows a call that synchronised its stream or used this one)
    const TileDesc &t = c->tiles[tile];
    const uint8_t *src = nullptr;
    uint64_t bytes = 0;
    uint32_t tmp[16];
    auto d2h = [&](void *dst, const void *s, uint64_t b) { return hipMemcpy(dst, s, b, hipMemcpyDeviceToHost) == hipSuccess; };
    if (what == 0) {
        if (!d2h(tmp, c->d_sums + tile * 4, 16)) return -1;
        int m = 0; uint32_t r = tmp[0];
        for (int k = 1; k < 4; k++) if (tmp[k] < r) { m = k; r = tmp[k]; }
        uint8_t pr = (t.w < 4 || t.h < 4) ? 0 : (uint8_t)((c->pxsz & 4) | m);
        if (cap < 1) return -1;
        *(uint8_t *)out = pr;
        return 1;
    } else if (what >= 1 && what <= 5) {
        if (!c->d_planes || (what == 5 && c->pxsz != 4)) return -1;  // the five planes exist after xpnghip_m1_transform_device (config-2 entry) or a mode-2 encode
        src = c->d_planes + (uint64_t)(what - 1) * c->plane_stride + t.pbase; bytes = t.n;
    } else if (what >= 10 && what <= 29 && !c->d_scratch) {
        return -1;  // no level-1 encode has run on this context
    } else if (what >= 10 && what <= 18) {
        if (!d2h(tmp, c->d_ctx_n + tile * 9, 36)) return -1;
        src = c->d_scratch + t.sbase + off_ctx(t.n, tmp, what - 10); bytes = tmp[what - 10];
    } else if (what == 19) {
        if (!d2h(tmp, c->d_k_n + tile, 4)) return -1;
        src = c->d_scratch + t.sbase + off_kw(t.n); bytes = 4ull * tmp[0];
    } else if (what >= 20 && what <= 29) {
        if ((uint32_t)(what - 20) >= c->spt) return 0;
        uint32_t cn[9];
        if (!d2h(cn, c->d_ctx_n + tile * 9, 36) || !d2h(tmp, c->d_blk_sz + tile * 10, 40)) return -1;
        src = c->d_scratch + t.sbase + off_blk(t.n, cn, what - 20); bytes = tmp[what - 20];
    } else if (what == 40 || what == 41) {
        if (!c->d_dbg) return -1;  // phase stamps exist in probe builds only
        src = (const uint8_t *)(c->d_dbg + ((what - 40) * c->tiles.size() * c->B + tile) * 80); bytes = 640;
    } else if (what == 30) {
        src = (const uint8_t *)(c->d_sums + tile * 4); bytes = 16;
    } else return -1;
    if (bytes > cap) return -1;
    if (bytes && !d2h(out, src, bytes)) return -1;
    return (int64_t)bytes;
}
