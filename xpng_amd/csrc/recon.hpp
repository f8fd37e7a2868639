// recon.hpp -- the last stage of every decode, both levels: pixels from the residual plane.
//
// Reference path restated: m1d_* (libxpng.c:796-830) behind dec_1_th, DEC / DEC4 (901-914) behind dec_2_th.  A tile record (DecTile,
// M2DecTile) is read once, by its recon_head overload; the uncoded kinds are filled by recon_fill; a coded tile runs one of three forms
// over the pixel rule recon_px / recon_px_band:
//
//   k_dec_recon       one workgroup per tile, one row per thread on an anti-diagonal: recon_free (waves hand rows over through LDS
//                     and progress counters, tiles up to 1024 rows whose rows fit the LDS) or recon_wavefront (barrier per step)
//   k_dec_recon_band  one wavefront per tile sweeping 64-row bands (recon_band_core): what a batch uses
//
// recon_geometry chooses among them and recon_launch launches.
#pragma once
#include "common.hpp"
#include "rans_dec.hpp"  // DecTile, TILE_BAD, ld32u

namespace xpng {

// What a reconstruction kernel needs from a tile's record.
enum ReconFill : uint32_t { RF_CODED, RF_ROWS, RF_GRAY, RF_COLOUR, RF_SKIP };
struct ReconHead {
    const uint8_t *src;  // uncoded kinds: what to fill from
    ReconFill fill;      // coded / raw rows / raw gray (level 2) / one colour (level 2) / skip: the tile failed validation
    uint32_t first;      // coded: the tile's first pixel
    int predmode;        // coded: 0 = average (p2a), 1 = gradient (p3a), 2 = left (p1x), 3 = up (p1y) for interior pixels
};
// (The order of the statements in a recon_head - every field set where the parent kernels computed it, early returns - is what keeps
//  the band kernel's code next to its predecessor's: profiles/device_code_recon.txt.)
template <int PXSZ>
__device__ __forceinline__ ReconHead recon_head(const DecTile *d) {
    ReconHead h{};
    const uint32_t type = d->type;
    h.fill = RF_SKIP;
    if (type == TILE_BAD) return h;
    h.fill = RF_ROWS;  // raw rows (libxpng.c:846)
    h.src = d->blob + 4;
    if (type == 0) return h;
    h.fill = RF_CODED;
    const uint32_t kw0 = ld32u(d->blob + 8);  // first pixel from the head of k (libxpng.c:850): bytes MSB-first
    h.first = ((kw0 >> 24) & 255u) | (((kw0 >> 16) & 255u) << 8) | (((kw0 >> 8) & 255u) << 16) | (PXSZ == 4 ? (kw0 & 255u) << 24 : 0u);
    h.predmode = (int)((type >> 1) & 1);
    return h;
}
// the uncoded kinds, by `nthreads` threads of which this one is `tid`
template <int PXSZ>
__device__ __forceinline__ void recon_fill(const ReconHead &h, const TileDesc &t, uint8_t *dst, uint64_t bpr, uint32_t tid,
                                           uint32_t nthreads) {
    const uint64_t row = (uint64_t)t.w * PXSZ;
    for (uint64_t b = tid; b < row * t.h; b += nthreads) {
        const uint64_t y = b / row, o = b - y * row;
        dst[y * bpr + o] = h.fill == RF_ROWS ? h.src[b] : h.fill == RF_GRAY ? h.src[y * t.w + o / PXSZ] : h.src[o % PXSZ];
    }
}

// --------------------------------------------------------------------------------------------------
// The pixel rule (libxpng.c:798-813), once per representation.  rw = packed residual word of the pixel (r | g<<8 | b<<16 | coded<<24:
// the top byte is the pixel's alpha for RGBA - non-zero exactly when coded - and 1 for RGB); L, U, UL = the reconstructed
// neighbours; interior pixels predict by predmode, row 0 always from the left and column 0 from above; `first` = the tile's first pixel.
__device__ __forceinline__ uint32_t swar_add8(uint32_t a, uint32_t b) {  // per-byte a + b (mod 256)
    return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
}
// Byte-parallel: all four channels move through one register (v_lerp_u8 average, 16-bit-lane gradient, byte-parallel add).
// predmode is wave-uniform, grad = (predmode == 1) hoisted by the caller.  Modes 2 and 3 occur in gray tiles of level 2 only
// (libxpng.c:890-895).
__device__ __forceinline__ uint32_t recon_px_band(uint32_t rw, uint32_t prev, uint32_t nU, uint32_t nUL, int predmode, bool grad, int32_t x,
                                                  uint32_t y, uint32_t first) {
    uint32_t pred;
    if (!grad) pred = __builtin_amdgcn_lerp(prev, nU, 0x01010101u);  // per byte (L + U + 1) >> 1
    else {
        const uint32_t Le = prev & 0x00FF00FFu, Ue = nU & 0x00FF00FFu, ULe = nUL & 0x00FF00FFu;
        const uint32_t pe = ((times3(Le + Ue) + 0x04020402u - 2u * ULe) >> 2) & 0x00FF00FFu;
        const int lg = (int)((prev >> 8) & 255u), ug = (int)((nU >> 8) & 255u), ulg = (int)((nUL >> 8) & 255u);
        pred = pe | (((uint32_t)(((int)times3((uint32_t)(lg + ug)) - 2 * ulg + 2) >> 2) & 255u) << 8);
    }
    pred = predmode == 2 ? prev : pred;
    pred = predmode == 3 ? nU : pred;
    pred = y == 0 ? prev : pred;   // row 0 predicts from the left,
    pred = x == 0 ? nU : pred;     // column 0 from above (libxpng.c:805-810)
    uint32_t px = (swar_add8(rw, pred) & 0x00FFFFFFu) | (rw & 0xFF000000u);  // alpha travels in the residual word
    px = (rw >> 24) ? px : 0u;     // alpha == 0: the whole pixel is 0 (libxpng.c:802)
    px = (y | (uint32_t)x) == 0 ? first : px;
    return px;
}
// Scalar, a channel at a time.
template <int PXSZ>
__device__ __forceinline__ uint32_t recon_px(uint32_t rw, uint32_t L, uint32_t U, uint32_t UL, int32_t x, uint32_t y, int predmode,
                                             uint32_t first) {
    if ((y | (uint32_t)x) == 0) return first;
    uint32_t px = 0;
    if ((rw >> 24) != 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int l = (L >> (8 * c)) & 255, u = (U >> (8 * c)) & 255, ul = (UL >> (8 * c)) & 255;
            int pred;
            if (y == 0) pred = l;
            else if (x == 0) pred = u;
            else pred = predmode == 0 ? pred_avg(l, u) : predmode == 1 ? pred_grad(l, u, ul) : predmode == 2 ? l : u;
            px |= (((rw >> (8 * c)) + (uint32_t)pred) & 255u) << (8 * c);
        }
    }
    if (PXSZ == 4) px |= rw & 0xFF000000u;  // alpha travels in the residual word; alpha == 0 -> whole pixel 0 (libxpng.c:802)
    return px;
}
// (end of the pixel rules: tests/test_recon_pixel_host.py runs the text from swar_add8 to here on the host)

// --------------------------------------------------------------------------------------------------
// Coded tiles: pixel (x,y) needs reconstructed L, U, UL, so rows advance as an anti-diagonal wavefront: thread r handles row
// yb+r and, at step s, column s-r.  Its U is what thread r-1 produced one step earlier (LDS, double-buffered by step parity),
// its UL is its previous U, its L its own previous output.  Tiles taller than 1024 rows run in bands; a band's first row reads
// U from the raster.  rs[i] = packed residual word of pixel i.
template <int PXSZ>
__device__ inline void recon_wavefront(const TileDesc &t, uint8_t *__restrict__ dst, uint64_t bpr,
                                       const uint32_t *__restrict__ rs, uint32_t first, int predmode, uint32_t (*s_row)[1024]) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t yb = 0; yb < t.h; yb += 1024) {
        const uint32_t rows = (t.h - yb) < 1024u ? (t.h - yb) : 1024u;
        const uint32_t y = yb + tid;
        const bool active = tid < rows;
        uint32_t L = 0, U = 0, UL = 0;
        const uint32_t steps = t.w + rows - 1;
        uint32_t nres = 0;  // residual word prefetched for the next step of this thread
        if (active && tid == 0) nres = rs[(uint64_t)y * t.w];
        for (uint32_t s = 0; s < steps; s++) {
            const int32_t x = (int32_t)s - (int32_t)tid;
            const bool on = active && x >= 0 && x < (int32_t)t.w;
            // U for this step: previous row's output at column x
            uint32_t Unew = 0;
            if (on && y > 0) {
                if (tid > 0) Unew = s_row[(s + 1) & 1][tid - 1];  // written at step s-1
                else Unew = load_px<PXSZ>(dst + (uint64_t)(y - 1) * bpr + (uint64_t)x * PXSZ);  // band seam: from the raster
            }
            if (on) {
                UL = U; U = Unew;
                const uint32_t outpx = recon_px<PXSZ>(nres, L, U, UL, x, y, predmode, first);
                L = outpx;
                uint8_t *o = dst + (uint64_t)y * bpr + (uint64_t)x * PXSZ;
                if (PXSZ == 4) *reinterpret_cast<uint32_t *>(o) = outpx;
                else { o[0] = (uint8_t)outpx; o[1] = (uint8_t)(outpx >> 8); o[2] = (uint8_t)(outpx >> 16); }
                s_row[s & 1][tid] = outpx;
            }
            // prefetch the residual of the next step (column x+1 of this row)
            const int32_t xn = x + 1;
            if (active && xn >= 0 && xn < (int32_t)t.w) nres = rs[(uint64_t)y * t.w + (uint32_t)xn];
            __syncthreads();
        }
        __syncthreads();  // the band's last row is in the raster (global) before the next band reads it
        __threadfence_block();
    }
}

// Barrier-free form of the wavefront (tiles up to 1024 rows).  Wave w owns rows 64w..64w+63, lane l handles column s - l at
// its own step s; no workgroup barrier: a wave only waits for the wave above through a progress counter in LDS.
//   * U (row above, same column) is what lane l-1 produced one step earlier: one DPP wave_shr, no LDS;
//   * lane 0 takes U from the boundary row of the wave above, which that wave's last lane streams into an LDS row buffer
//     (64 columns are fetched at a time and handed out with v_readlane);
//   * residual words are prefetched 4 steps ahead into rotating registers.
// dynamic LDS: nw * ew dwords of boundary rows + 16 progress counters.
template <int PXSZ>
__device__ inline void recon_free(const TileDesc &t, uint8_t *__restrict__ dst, uint64_t bpr, const uint32_t *__restrict__ rs,
                                  uint32_t first, int predmode, uint32_t *edge, uint32_t ew, uint32_t *prog) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t nw = (t.h + 63) >> 6;
    if (tid < 16) prog[tid] = 0;
    __syncthreads();
    if (w >= nw) return;
    const uint32_t y = 64 * w + lane;
    const bool active = y < t.h;
    const uint32_t *rsrow = rs + (uint64_t)(active ? y : 0) * t.w;
    uint8_t *drow = dst + (uint64_t)(active ? y : 0) * bpr;
    const uint32_t S = t.w + 63;  // steps of this wave
    uint32_t *my_edge = edge + w * ew;
    const uint32_t *up_edge = edge + (w ? w - 1 : 0) * ew;
    const bool writer = lane == 63 && w + 1 < nw;  // (the last lane of a non-final wave is always an existing row)
    uint32_t prev = 0, U = 0, UL = 0, ev = 0;
    auto fetch = [&](uint32_t s) -> uint32_t {  // residual word this lane needs at step s
        const int32_t x = (int32_t)s - (int32_t)lane;
        return (active && x >= 0 && x < (int32_t)t.w) ? rsrow[x] : 0u;
    };
    uint32_t r0 = fetch(0), r1 = fetch(1), r2 = fetch(2), r3 = fetch(3);
    auto step = [&](uint32_t s, uint32_t rw) {
        if (w > 0 && (s & 63u) == 0 && s < t.w) {  // uniform: next 64 columns of the boundary row above
            const uint32_t need = s + 64 < t.w ? s + 64 : t.w;
            while (__hip_atomic_load(&prog[w - 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < need) __builtin_amdgcn_s_sleep(2);
            ev = s + lane < t.w ? up_edge[s + lane] : 0u;
        }
        // previous-step output of the lane above (lane 0: boundary row of the wave above)
        uint32_t Unew = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)prev, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)ev, (int)(s & 63u));
        if (lane == 0) Unew = e0;
        const int32_t x = (int32_t)s - (int32_t)lane;
        const bool on = active && x >= 0 && x < (int32_t)t.w;
        if (on) {
            UL = U; U = Unew;
            const uint32_t outpx = recon_px<PXSZ>(rw, prev, U, UL, x, y, predmode, first);
            uint8_t *o = drow + (uint64_t)x * PXSZ;
            if (PXSZ == 4) *reinterpret_cast<uint32_t *>(o) = outpx;
            else { o[0] = (uint8_t)outpx; o[1] = (uint8_t)(outpx >> 8); o[2] = (uint8_t)(outpx >> 16); }
            if (writer) {
                my_edge[x] = outpx;
                if ((x & 15) == 15 || x + 1 == (int32_t)t.w) __hip_atomic_store(&prog[w], (uint32_t)x + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            prev = outpx;
        }
    };
    uint32_t s = 0;
    for (; s + 4 <= S; s += 4) {
        uint32_t c0 = r0; r0 = fetch(s + 4); step(s, c0);
        uint32_t c1 = r1; r1 = fetch(s + 5); step(s + 1, c1);
        uint32_t c2 = r2; r2 = fetch(s + 6); step(s + 2, c2);
        uint32_t c3 = r3; r3 = fetch(s + 7); step(s + 3, c3);
    }
    if (s < S) { step(s, r0); s++; }
    if (s < S) { step(s, r1); s++; }
    if (s < S) { step(s, r2); s++; }
}

template <int PXSZ, class Info>
__global__ __launch_bounds__(1024) void k_dec_recon(const Info *__restrict__ info, const TileDesc *__restrict__ tiles, TileSel sel,
                                                    const uint32_t *__restrict__ resid, uint8_t *const *__restrict__ rasters,
                                                    uint64_t bpr, uint32_t free_ew) {
    bw_prio();
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const ReconHead h = recon_head<PXSZ>(info + j);
    if (h.fill == RF_SKIP) return;
    const TileDesc t = tiles[vtile(sel, j)];
    uint8_t *dst = rasters[t.img] + (uint64_t)t.y * bpr + (uint64_t)t.x * PXSZ;
    if (h.fill != RF_CODED) { recon_fill<PXSZ>(h, t, dst, bpr, tid, blockDim.x); return; }
    if (free_ew) {
        extern __shared__ uint32_t dyn_lds[];
        recon_free<PXSZ>(t, dst, bpr, resid + t.pbase, h.first, h.predmode, dyn_lds + 16, free_ew, dyn_lds);
    } else {
        __shared__ uint32_t s_row[2][1024];
        recon_wavefront<PXSZ>(t, dst, bpr, resid + t.pbase, h.first, h.predmode, s_row);
    }
}

// --------------------------------------------------------------------------------------------------
// Reconstruction for large batches: ONE wavefront per tile (k_dec_recon spreads a tile over up to 9 waves that hand rows
// to each other through LDS and progress counters: right for one image, but with thousands of tiles in flight the
// per-step hand-over latency, not the arithmetic, sets the pace).  The tile is swept in bands of 64 rows; lane r owns row
// yb + r and at step s reconstructs column s - r, so its U is what lane r-1 produced one step earlier (DPP wave_shr:1),
// its UL its previous U and its L its own previous output: no LDS, no synchronisation inside a band.  Lane 63 leaves its
// row in a seam buffer for lane 0 of the next band.  All four channels move through one register (v_lerp_u8 average,
// 16-bit-lane gradient, byte-parallel add); residual words arrive as one 16-byte load per lane every 4 steps and pixels
// leave as one 16-byte store (single dwords at the two ends of a row).
constexpr uint32_t RB_MAXW = 2048;  // seam buffer, pixels
// Row staging through LDS.  A lane's row moves between HBM and the wave in whole, 64-byte-aligned 16-word chunks - four
// back-to-back 16-byte requests per lane for ONE chunk of its own row, once per 16 steps - instead of one 16-byte piece every
// 4 steps: with thousands of waves x 64 rows in flight the pieces of a line used to arrive microseconds apart, L2 had dropped the
// line in between, and the kernel moved 2.2-2.4x its algorithmic bytes (profiles/r02_pmc_step_mem.json: 21.9 B/px against 8).
// Each lane owns a two-chunk ring per direction (the lane skew makes the word a lane needs at a step lane-dependent, which LDS
// addressing absorbs): residual words [0,32) + a 4-word mirror of words 0-3, so that a lane's unaligned 4-word read never
// wraps; pixels [0,32) + a 4-word spill zone behind them for the 4-word write that straddles the ring's end.
constexpr uint32_t RB_RING = 36;                       // words per lane and direction (a stride of 9 x 16 bytes: conflict-free b128)
constexpr uint32_t RB_STAGE_WORDS = 64 * RB_RING * 2;  // LDS words in front of the seam row
constexpr size_t RB_LDS_BYTES(uint32_t max_w) { return (size_t)RB_STAGE_WORDS * 4 + (size_t)max_w * 4 + 256; }
template <int PXSZ>
__device__ __forceinline__ void recon_band_core(const TileDesc &t, uint8_t *__restrict__ dst, uint64_t bpr, const uint32_t *__restrict__ rs,
                                                uint32_t first, int predmode, uint32_t *stage, uint32_t *seam, uint32_t dbgflags) {
    const uint32_t lane = threadIdx.x & 63;
    const bool grad = predmode == 1;
    const int32_t w = (int32_t)t.w;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x4_a4r __attribute__((ext_vector_type(4), aligned(4)));
    uint32_t *rin = stage + lane * RB_RING, *rout = stage + 64 * RB_RING + lane * RB_RING;
    for (uint32_t yb = 0; yb < t.h; yb += 64) {
        const uint32_t y = yb + lane;
        const bool active = y < t.h;
        // (a lane without a row reads the tile's last row again and stores nothing)
        const uint32_t *rsrow = rs + (uint64_t)(active ? y : t.h - 1) * t.w;
        uint8_t *drow = dst + (uint64_t)(active ? y : 0) * bpr;
        // positions: p = x + a counts words from the 64-byte boundary in front of the row's first residual word (chunk c = words
        // [16c, 16c+16), chunks 0..Lc hold the row; at most 15 words in front of / behind the row are read: the neighbouring rows
        // of the tile, or the slack around the residual plane); po = x + ao the same for the pixels of the raster row
        const int32_t a = (int32_t)(((uintptr_t)rsrow >> 2) & 15u);
        const u32x4 *rsal = reinterpret_cast<const u32x4 *>(rsrow - a);
        const int32_t Lc = (a + w - 1) >> 4;
        const int32_t ao = PXSZ == 4 ? (int32_t)(((uintptr_t)drow >> 2) & 15u) : 0;
        uint8_t *dal = drow - 4 * ao;
        const int32_t olo = active ? ao : 0, ohi = active ? ao + w : 0;  // valid pixel positions of this lane
        const uint32_t pho = (uint32_t)(ao - (int32_t)lane) & 3u;      // every 4-word pixel write of this lane starts at po = pho (mod 4)
        // RGB [r3]: the same staging in BYTE positions (a pixel is 3 bytes at any alignment): pb = 3 x + ab counts bytes from the
        // 64-byte boundary in front of the row's first byte; four pixels are one unaligned 12-byte LDS write into the lane's 128-byte
        // ring (a write that crosses its end continues in the 16-byte spill zone and is taken back when ring chunk 0 is flushed);
        // a 64-byte chunk leaves as four aligned 16-byte stores once a block (48 bytes) has completed it; only the partial
        // granules at the two ends of a row fall back to dword / byte stores.  (Round 2 stored every group as 12 bytes at its own
        // address: 64 rows x 12 bytes per wave instruction.)
        const int32_t ab = PXSZ == 3 ? (int32_t)((uintptr_t)drow & 63u) : 0;
        uint8_t *dalb = drow - ab;
        const int32_t blo = active ? ab : 0, bhi = active ? ab + 3 * w : 0;  // valid byte positions of this lane
        int32_t pb0 = ab - 3 * (int32_t)lane;                           // byte position of the block's first pixel
        int32_t flc = pb0 >> 6;                                          // next chunk to flush
        uint32_t sp_n = 0;                                               // bytes of ring chunk 0 that sit in the spill zone
        const uint32_t S = t.w + 63;
        uint32_t prev = 0, U = 0, ev = 0;
#define XPNG_RB_CLAMP(c) ((c) < 0 ? 0 : (c) > Lc ? Lc : (c))
#define XPNG_RB_LOAD(G, c) { const u32x4 *cp_ = rsal + 4 * XPNG_RB_CLAMP(c); G[0] = cp_[0]; G[1] = cp_[1]; G[2] = cp_[2]; G[3] = cp_[3]; }
#define XPNG_RB_PUT(G, c) { const uint32_t sl_ = (uint32_t)XPNG_RB_CLAMP(c) & 1u; u32x4 *rp_ = reinterpret_cast<u32x4 *>(rin + 16 * sl_); \
                            rp_[0] = G[0]; rp_[1] = G[1]; rp_[2] = G[2]; rp_[3] = G[3]; if (sl_ == 0) *reinterpret_cast<u32x4 *>(rin + 32) = G[0]; }
        int32_t p0 = a - (int32_t)lane, po0 = ao - (int32_t)lane;  // positions of this lane at the first step of the block
        u32x4 G[4];
        XPNG_RB_LOAD(G, p0 >> 4);
        XPNG_RB_PUT(G, p0 >> 4);
        XPNG_RB_LOAD(G, (p0 >> 4) + 1);
        for (uint32_t s0 = 0; s0 < S; s0 += 16, p0 += 16, po0 += 16, pb0 += 48) {
            // block of 16 steps: the chunk requested a block ago lands in the ring, the next one is requested, and the block's 16
            // residual words come out of the ring (they lie in chunks p0 >> 4 and (p0 >> 4) + 1)
            XPNG_RB_PUT(G, (p0 >> 4) + 1);
            XPNG_RB_LOAD(G, (p0 >> 4) + 2);
            u32x4 cur[4];
#pragma unroll
            for (int q = 0; q < 4; q++) cur[q] = *reinterpret_cast<const u32x4_a4r *>(rin + ((uint32_t)(p0 + 4 * q) & 31u));
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const uint32_t s = s0 + 4 * q;
            if (yb > 0 && (s & 63u) == 0 && (int32_t)s < w) ev = (int32_t)(s + lane) < w ? seam[s + lane] : 0u;  // next 64 columns of the row above the band
            const uint32_t rwv[4] = {cur[q].x, cur[q].y, cur[q].z, cur[q].w};
            uint32_t o[4];
            const int32_t x0 = (int32_t)s - (int32_t)lane;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                // previous-step output of the lane above (lane 0: the seam row)
                uint32_t Unew = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)prev, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
                const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)ev, (int)((s + k) & 63u));
                Unew = lane == 0 ? e0 : Unew;
                const int32_t x = x0 + k;
                const bool on = active && x >= 0 && x < w;
                const uint32_t px = recon_px_band(rwv[k], prev, Unew, U, predmode, grad, x, y, first);
                if (on) { U = Unew; prev = px; }
                o[k] = px;
                if (lane == 63 && on) seam[x] = px;  // (a full band: lane 63 is an existing row)
            }
            if (PXSZ == 4) {
                // four pixels into the lane's ring (words past 31: the spill zone, taken back when chunk 0 of the ring is flushed)
                *reinterpret_cast<u32x4_a4r *>(rout + ((uint32_t)(po0 + 4 * q) & 31u)) = u32x4_a4r{o[0], o[1], o[2], o[3]};
            } else {
                // RGB: the (marker) top byte of a pixel word is dropped; four pixels are 12 consecutive bytes at any alignment
                typedef uint32_t u32x3_a1 __attribute__((ext_vector_type(3), aligned(1)));
                const uint32_t q0 = o[0] & 0xFFFFFFu, q1 = o[1] & 0xFFFFFFu, q2 = o[2] & 0xFFFFFFu, q3 = o[3] & 0xFFFFFFu;
                const uint32_t ob = (uint32_t)(pb0 + 12 * q) & 127u;
                *reinterpret_cast<u32x3_a1 *>(reinterpret_cast<uint8_t *>(rout) + ob) = u32x3_a1{q0 | (q1 << 24), (q1 >> 8) | (q2 << 16), (q2 >> 16) | (q3 << 8)};
                sp_n = ob > 116u ? ob - 116u : sp_n;
            }
          }
            if (PXSZ == 3) {
#define XPNG_RB_FLUSH3()                                                                                                                \
                {                                                                                                                       \
                    const u32x4 *fp = reinterpret_cast<const u32x4 *>(rout + 16 * ((uint32_t)flc & 1u));                                \
                    u32x4 v[4] = {fp[0], fp[1], fp[2], fp[3]};                                                                          \
                    if (((uint32_t)flc & 1u) == 0) {                                                                                    \
                        const u32x4 sp = *reinterpret_cast<const u32x4 *>(rout + 32);                                                   \
                        const uint32_t spw[3] = {sp.x, sp.y, sp.z};                                                                     \
                        uint32_t vw[3] = {v[0].x, v[0].y, v[0].z};                                                                      \
                        _Pragma("unroll") for (int j = 0; j < 3; j++) {                                                                 \
                            const int32_t nb = (int32_t)sp_n - 4 * j;                                                                   \
                            const uint32_t m = nb >= 4 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : (1u << (8 * nb)) - 1u);                          \
                            vw[j] = (spw[j] & m) | (vw[j] & ~m);                                                                        \
                        }                                                                                                               \
                        v[0].x = vw[0]; v[0].y = vw[1]; v[0].z = vw[2];                                                                 \
                        sp_n = 0;                                                                                                       \
                    }                                                                                                                   \
                    _Pragma("unroll") for (int g = 0; g < 4; g++) {                                                                     \
                        const int32_t lo = flc * 64 + 16 * g;                                                                           \
                        if (lo >= blo && lo + 16 <= bhi) *reinterpret_cast<u32x4 *>(dalb + lo) = v[g];                                  \
                        else if (lo + 16 > blo && lo < bhi) {                                                                           \
                            const uint32_t vv[4] = {v[g].x, v[g].y, v[g].z, v[g].w};                                                    \
                            _Pragma("unroll") for (int k = 0; k < 4; k++) {                                                             \
                                const int32_t dlo = lo + 4 * k;                                                                         \
                                if (dlo >= blo && dlo + 4 <= bhi) *reinterpret_cast<uint32_t *>(dalb + dlo) = vv[k];                    \
                                else if (dlo + 4 > blo && dlo < bhi) {                                                                  \
                                    _Pragma("unroll") for (int b = 0; b < 4; b++)                                                       \
                                        if (dlo + b >= blo && dlo + b < bhi) dalb[dlo + b] = (uint8_t)(vv[k] >> (8 * b));               \
                                }                                                                                                       \
                            }                                                                                                           \
                        }                                                                                                               \
                    }                                                                                                                   \
                    flc++;                                                                                                              \
                }
                if (64 * (flc + 1) <= pb0 + 48) XPNG_RB_FLUSH3()  // (a block writes 48 bytes: it completes at most one chunk)
            }
            if (PXSZ == 4) {
                // the pixel chunk this block completed (the one holding the block's first position) leaves as four 16-byte stores
#define XPNG_RB_FLUSH(fc_)                                                                                                              \
                {                                                                                                                       \
                    const int32_t fc = (fc_);                                                                                           \
                    const u32x4 *fp = reinterpret_cast<const u32x4 *>(rout + 16 * ((uint32_t)fc & 1u));                                 \
                    u32x4 v[4] = {fp[0], fp[1], fp[2], fp[3]};                                                                          \
                    if (((uint32_t)fc & 1u) == 0) {                                                                                     \
                        const u32x4 sp = *reinterpret_cast<const u32x4 *>(rout + 32);                                                   \
                        v[0].x = pho > 0 ? sp.x : v[0].x; v[0].y = pho > 1 ? sp.y : v[0].y; v[0].z = pho > 2 ? sp.z : v[0].z;           \
                    }                                                                                                                   \
                    if (!(dbgflags & 1)) {                                                                                              \
                        _Pragma("unroll") for (int q = 0; q < 4; q++) {                                                                 \
                            const int32_t pq = fc * 16 + 4 * q;                                                                         \
                            if (pq >= olo && pq + 4 <= ohi) *reinterpret_cast<u32x4 *>(dal + 4ll * pq) = v[q];                          \
                            else if (pq + 4 > olo && pq < ohi) {                                                                        \
                                const uint32_t vv[4] = {v[q].x, v[q].y, v[q].z, v[q].w};                                                \
                                _Pragma("unroll") for (int k = 0; k < 4; k++)                                                           \
                                    if (pq + k >= olo && pq + k < ohi) *reinterpret_cast<uint32_t *>(dal + 4ll * (pq + k)) = vv[k];     \
                            }                                                                                                           \
                        }                                                                                                               \
                    }                                                                                                                   \
                }
                XPNG_RB_FLUSH(po0 >> 4)
            }
        }
        if (PXSZ == 4) XPNG_RB_FLUSH(po0 >> 4)  // (po0 was advanced past the last block: its chunk holds the tail of the row, if anything)
        if (PXSZ == 3) {
            // the tail of the row: every position up to the last block's end has been written; at most two chunks are still in the ring
            if (64 * flc < bhi) XPNG_RB_FLUSH3()
            if (64 * flc < bhi) XPNG_RB_FLUSH3()
        }
#undef XPNG_RB_FLUSH3
#undef XPNG_RB_FLUSH
#undef XPNG_RB_CLAMP
#undef XPNG_RB_LOAD
#undef XPNG_RB_PUT
    }
}

template <int PXSZ, class Info>
__global__ __launch_bounds__(64) void k_dec_recon_band(const Info *__restrict__ info, const TileDesc *__restrict__ tiles, TileSel sel,
                                                       const uint32_t *__restrict__ resid, uint8_t *const *__restrict__ rasters,
                                                       uint64_t bpr, uint32_t dbgflags, uint32_t j0, uint32_t j1) {
    bw_prio();
    extern __shared__ uint32_t rb_lds[];  // the lanes' staging rings, then one row of the widest tile of the launch (bottom row of the band above)
    uint32_t *seam = rb_lds + RB_STAGE_WORDS;
    const uint32_t lane = threadIdx.x & 63;
    // work items [j0, j1), one wave each; a launch with fewer workgroups than items walks them with a grid stride (recon_grid)
    for (uint32_t j = j0 + blockIdx.x; j < j1; j += gridDim.x) {
        const ReconHead h = recon_head<PXSZ>(info + j);
        if (h.fill == RF_SKIP) continue;
        const TileDesc t = tiles[vtile(sel, j)];
        uint8_t *dst = rasters[t.img] + (uint64_t)t.y * bpr + (uint64_t)t.x * PXSZ;
        if (h.fill != RF_CODED) { recon_fill<PXSZ>(h, t, dst, bpr, lane, 64); continue; }
        recon_band_core<PXSZ>(t, dst, bpr, resid + t.pbase, h.first, h.predmode, rb_lds, seam, dbgflags);
    }
}

// (Round 3 built the residual extraction INTO this kernel - a lane cutting its row's residuals out of k from per-row cursors,
// no residual plane, no k_dec_resid - and measured it: bit-exact, 13.3 instead of 15.7 ms of kernel time per step, the same
// 37-38 Gpx/s, and 66.7 instead of 46.3 B/px of HBM traffic (profiles/r03_pmc_step_mem_fold_experiment.json): 64 rows x three
// variable-rate streams per wave cannot be fetched in whole 64-byte sectors without ~32 KB of LDS rings per wave, and anything less
// re-fetches every sector once per block because L2 does not keep it for the microsecond between two blocks.  k_dec_resid reads
// the same streams in raster order, perfectly coalesced; the 4 B/px residual plane is the price of that.  Not kept)

// workgroups of a band-reconstruction launch over n work items (probe builds: XPNG_RECON_CAP)
inline uint32_t recon_grid(uint32_t n) {
    const char *e = probe_env("XPNG_RECON_CAP");
    const uint32_t cap = e ? (uint32_t)atoi(e) : 0u;
    return cap && cap < n ? cap : n;
}

// The form a decode's reconstruction takes and the geometry of its launch, for tiles up to max_w x max_h; wide = the decode has
// enough tiles in flight for the wide entropy path (wide_form, common.hpp).
struct ReconPlan {
    bool band;         // k_dec_recon_band; otherwise k_dec_recon
    uint32_t free_ew;  // k_dec_recon: columns of a boundary row of recon_free; 0 = recon_wavefront, the barrier form
    uint32_t threads, lds;
    uint32_t nostore;  // probe builds (XPNG_DBG_NOSTORE): the band form stores no pixels; 0 in the release library
};
inline ReconPlan recon_geometry(uint32_t max_w, uint32_t max_h, bool wide) {
    ReconPlan p{};
    if (wide && max_w <= RB_MAXW && !probe_env("XPNG_WAVEFRONT_RECON")) {
        // (probe builds, XPNG_RECON_LDS_PAD: bytes of unused LDS per workgroup.  The band form's scattered 16-byte loads and stores fill
        //  the memory pipeline's queues and the chain kernels of the other pipeline slots then wait for their words: DESIGN.md 6)
        p.band = true; p.threads = 64; p.lds = (uint32_t)(RB_LDS_BYTES(max_w) + probe_pad("XPNG_RECON_LDS_PAD"));
        p.nostore = probe_env("XPNG_DBG_NOSTORE") ? 1u : 0u;
        return p;
    }
    const uint32_t nw = (max_h + 63) / 64;
    p.threads = 1024;
    if (probe_env("XPNG_BARRIER_RECON") || max_h > 1024 || (uint64_t)nw * max_w * 4 + 64 > 60000) return p;
    p.free_ew = max_w; p.threads = nw * 64; p.lds = nw * max_w * 4 + 64;
    return p;
}

// Reconstruct work items [first, first + n) of `info` on stream st.
template <int PXSZ, class Info>
inline void recon_launch(const ReconPlan &p, const Info *info, const TileDesc *tiles, const TileSel &sel, const uint32_t *resid,
                         uint8_t *const *rasters, uint64_t bpr, uint32_t first, uint32_t n, hipStream_t st) {
    if (p.band) k_dec_recon_band<PXSZ, Info><<<recon_grid(n), p.threads, p.lds, st>>>(info, tiles, sel, resid, rasters, bpr, p.nostore, first, first + n);
    else k_dec_recon<PXSZ, Info><<<n, p.threads, p.lds, st>>>(info, tiles, sel, resid, rasters, bpr, p.free_ew);  // (only the band form takes a sub-range: first == 0)
}

}  // namespace xpng
