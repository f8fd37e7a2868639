// The four validators of the decode - k_dec_parse, k_dec_offsets, k_dec_offsets_mixed (m1_decode.hpp) and k_m2_dec_parse
// (m2_decode.hpp) - run on the host over the hostile tiles of tests/_hostile.py (CASE_FILE, written by tests/test_dec_parse_host.py).
// KERNEL_TEXT is the kernels' text with the records and helpers they name, cut out of the product headers; this program adds the
// shims of bw_prio, atomicOr, bit_width and ld32u.  ld32u does what the product's does - an unaligned load becomes two aligned
// dword reads - and CHECKS each of them: a read must lie inside one of the byte ranges the launch may read (a tile's
// [blob, blob + avail), rounded out to aligned dwords).  Every blob sits at the end of a heap block of exactly that rounded size, at
// each of the four byte phases, so the sanitizer sees what the check sees.
//
// Checked: the verdict of every case against the one its rules give; bit 0 of *status and the TILE_BAD / M2_KIND_BAD mark; the reads of
// accepted AND rejected cases; the record of every accepted case against the contract its consumers rely on (contract_m1,
// contract_m2: one clause per consumer); the three selection forms and the mixed one on 2 images x 3 tiles with one bad tile; both
// size walks on intact and broken chains.  Prints `cases: N` and ends with `errors: 0`; CASE_FILE.verdicts gets one line per case.
#include "kernel_host.hpp"
#include <string>
#define __host__

// ---- shims
struct Range { const uint8_t *lo, *hi; };
static std::vector<Range> g_may_read;
static const char *g_what = "";
static long g_reads = 0;
static uint32_t rd_dword(const uint32_t *q) {
    const uint8_t *p = (const uint8_t *)q;
    g_reads++;
    for (const Range &r : g_may_read) if (p >= r.lo && p + 4 <= r.hi) { uint32_t v; memcpy(&v, p, 4); return v; }
    if (errors < 20) printf("read outside the tile's bytes: %s\n", g_what);
    errors++;
    return 0;
}
static uint32_t ld32u(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3) * 8;
    const uint32_t lo = rd_dword(q);
    if (sh == 0) return lo;
    return (lo >> sh) | (rd_dword(q + 1) << (32 - sh));
}
static void bw_prio() {}
static uint32_t atomicOr(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o | v; return o; }
static int bit_width(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

namespace P {
#include KERNEL_TEXT
}
using P::DecTile; using P::M2DecTile; using P::M2Blk; using P::TileDesc; using P::TileSel;
using P::M2_SLOTS; using P::TILE_BAD; using P::M2_KIND_BAD;

// ---- the case file
struct Case { uint32_t base, mode, pxsz, n, w, avail, expect; std::vector<uint8_t> bytes; std::string name; };
static std::vector<Case> g_cases;
static void load_cases(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { printf("no case file %s\n", path); exit(2); }
    auto u = [&] { uint32_t v = 0; if (fread(&v, 4, 1, f) != 1) { puts("short case file"); exit(2); } return v; };
    auto bytes = [&](uint32_t n) { std::vector<uint8_t> b(n); if (n && fread(b.data(), 1, n, f) != n) { puts("short case file"); exit(2); } return b; };
    std::vector<std::vector<uint8_t>> bases(u());
    for (auto &b : bases) b = bytes(u());
    g_cases.resize(u());
    for (Case &c : g_cases) {
        c.base = u(); c.mode = u(); c.pxsz = u(); c.n = u(); c.w = u(); c.avail = u(); c.expect = u();
        const uint32_t np = u();
        c.bytes = bases[c.base];
        c.bytes.resize(c.avail, 0x5A);
        for (uint32_t i = 0; i < np; i++) { const uint32_t o = u(), l = u(); auto p = bytes(l); if (o + l > c.avail) { puts("patch outside the case"); exit(2); } if (l) memcpy(c.bytes.data() + o, p.data(), l); }
        auto nm = bytes(u());
        c.name.assign(nm.begin(), nm.end());
    }
    fclose(f);
}

// a blob at byte phase `ph` at the end of a heap block of exactly the dwords it touches
struct Placed {
    uint8_t *block; const uint8_t *blob; uint32_t avail;
    Placed(const uint8_t *src, uint32_t n, uint32_t ph) : avail(n) {
        block = (uint8_t *)malloc(rup(ph + n, 4) ? rup(ph + n, 4) : 1);
        memset(block, 0xC3, rup(ph + n, 4));
        if (n) memcpy(block + ph, src, n);
        blob = block + ph;
    }
    Range range() const { const uintptr_t a = (uintptr_t)blob; return {(const uint8_t *)(a & ~(uintptr_t)3), (const uint8_t *)((a + avail + 3) & ~(uintptr_t)3)}; }
    ~Placed() { free(block); }
    Placed(const Placed &) = delete;
};

static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
#define REQUIRE(cond, clause) do { if (!(cond)) { if (errors < 20) printf("contract: %s: %s\n", clause, name); errors++; return; } } while (0)

// ---- what the consumers of an accepted DecTile rely on
static void contract_m1(const DecTile &d, const uint8_t *blob, uint32_t avail, uint32_t n, int pxsz, const char *name) {
    const uint32_t L = rd32(blob) & 0xFFFFFF, ty = blob[3];
    REQUIRE(L <= avail, "the tile lies inside the bytes that exist");
    REQUIRE(d.blob == blob && d.type == ty, "record names the tile");
    if (ty == 0) { REQUIRE(L == n * (uint32_t)pxsz + 4, "k_dec_recon (RF_ROWS): n * pxsz raw bytes behind the word"); return; }
    REQUIRE(d.kbytes >= 4 && d.kbytes % 4 == 0 && 8 + (uint64_t)d.kbytes <= L, "k_dec_resid / recon_head: the k words [8, 8 + kbytes) inside the tile, the first pixel's word among them");
    const int spt = pxsz == 4 ? 10 : 9;
    uint64_t prev_end = 8 + (uint64_t)d.kbytes, sum = 0, prev_ctx_end = 0;
    for (int c = 0; c < spt; c++) {
        const uint64_t o = d.blk_off[c];
        REQUIRE(o >= prev_end && o + 4 <= L, "rans2_decode_stream: the block's first word inside the tile, blocks in order");
        const uint32_t h0 = rd32(blob + o), bt = h0 >> 24, sz = bt ? h0 & 0xFFFFFF : 4;
        REQUIRE(bt <= 4 && o + sz <= L, "rans2_decode_stream: the block [blk_off, blk_off + size) inside the tile");
        prev_end = o + sz;
        if (bt == 0) REQUIRE(d.blk_n[c] == 0, "k_dec_walk: an empty block has no symbols");
        else {
            REQUIRE(sz >= 8 && sz % 4 == 0, "rans2_dec_freqs / rans2_dec_plain: read whole dwords below the block's end");
            const uint32_t h1 = rd32(blob + o + 4), m = h1 & 0xFFFFFF, v2 = h1 >> 24;
            REQUIRE(d.blk_n[c] == m, "k_dec_walk / k_dec_alpha: blk_n is the header's count (the stream decoders re-read it)");
            if (bt == 2) REQUIRE(v2 >= 1 && v2 <= 8 && 8 + 4 * (((uint64_t)m * v2 + 31) >> 5) <= sz, "rans2_dec_plain: in + 8 + 4 ceil(n v2 / 32) inside the block, 1..8 bits");
            if (bt >= 3) {
                REQUIRE(sz >= 12, "rans2_decode_stream: the third header word");
                const uint32_t h2 = rd32(blob + o + 8), toff = h2 & 0xFFFFFF, pb = h2 >> 24;
                const int64_t table = 8 + 4 * (int64_t)toff, nw = (table - 16 - 12) >> 2;
                REQUIRE(v2 + 2 <= 256, "rans2_dec_freqs: N = v2 + 2 entries of Fs[260] / fc[256]");
                REQUIRE(pb >= 10 && pb <= 15, "rans2_decode_stream: coarse[1 << (15 - 3)], 16-bit cumulative counts");
                REQUIRE(nw >= 0 && table - 16 >= 12, "k_rans2_dec_prep / rans2_decode_stream: nw = (table - 16 - words) >> 2 >= 0, the states behind the header");
                REQUIRE(table < (int64_t)sz, "rans2_dec_freqs: the table starts inside the block");
            }
        }
        if (c < 9) {
            REQUIRE(d.ctx_start[c] % 16 == 0 && d.ctx_start[c] >= prev_ctx_end, "ctx_walk_salu: queue starts 16-byte aligned and increasing");
            REQUIRE((uint64_t)d.ctx_start[c] + d.blk_n[c] <= rup((uint64_t)n + 192, 256), "rans2_decode_stream: pbase + ctx_start[c] + blk_n[c] inside the tile's share of the symbol plane");
            prev_ctx_end = (uint64_t)d.ctx_start[c] + d.blk_n[c];
            sum += d.blk_n[c];
        } else REQUIRE(d.blk_n[9] <= n - 1, "k_dec_alpha: at most n - 1 alpha symbols behind asym + pbase");
    }
    REQUIRE(d.ctx_start[9] == sum && sum <= n - 1, "k_dec_walk: ctx_start[9] = the nine counts together <= n - 1 steps of the chain");
}

// MSB-first bits of b, 0 behind its end: this program's own reader
static uint32_t b_bits(const uint8_t *bw, uint64_t pos, uint32_t c, uint64_t endbit) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < c; i++, pos++) {
        uint32_t bit = 0;
        if ((pos & ~31ull) < endbit) { const uint32_t w = rd32(bw + (pos >> 5) * 4); bit = (w >> (31 - (pos & 31))) & 1; }
        v = (v << 1) | bit;
    }
    return v;
}

// ---- what the consumers of an accepted M2DecTile / M2Blk / stream_n / table rely on
static void contract_m2(const M2DecTile &d, const M2Blk *mb, const uint32_t *sn, const uint16_t *tabs, const uint8_t *blob, uint32_t avail,
                        uint32_t n, const char *name) {
    const uint32_t L = rd32(blob) & 0xFFFFFF, ty = blob[3];
    REQUIRE(L <= avail, "the tile lies inside the bytes that exist");
    REQUIRE(d.blob == blob, "record names the tile");
    for (uint32_t s = 0; s < M2_SLOTS; s++) REQUIRE(sn[s] != 0xDEADBEEFu, "m2_off_stream: all 21 stream_n entries of the tile are written");
    const uint32_t kind = ty == 0 ? 0 : ty == 255 ? 4 : (ty >> 4) == 2 ? ((ty & 8) ? 3 : 2) : 1;
    REQUIRE(d.kind == kind, "recon_head: kind from the type byte");
    if (kind == 0) REQUIRE(L == 3 * n + 4, "recon (RF_ROWS): 3 n raw bytes");
    if (kind == 3) REQUIRE(L == n + 4, "recon (RF_GRAY): n raw bytes");
    if (kind == 4) REQUIRE(L == 8, "recon (RF_COLOUR): one pixel behind the word");
    if (kind != 1 && kind != 2) { for (uint32_t s = 0; s < M2_SLOTS; s++) REQUIRE(sn[s] == 0, "a tile without streams has none"); return; }
    REQUIRE(d.m == (ty & 3), "recon_head / k_m2_dec_resid: predictor bits");
    REQUIRE(d.bsz >= 8 && d.bsz % 4 == 0 && 4 + (uint64_t)d.bsz <= L && d.bsz == rd32(blob + 4), "recon_head / bits_at: b = [8, 4 + bsz) inside the tile, whole words, the first pixel's word among them");
    const uint8_t *bw = blob + 8;
    const uint64_t endbit = (uint64_t)(d.bsz - 4) * 8, region = P::m2_streams_region(n);
    uint64_t pos = kind == 1 ? 24 : 8, o = 4 + (uint64_t)d.bsz, coded = 0, room = 0;
    const uint32_t s0 = kind == 1 ? 0 : 17, s1 = kind == 1 ? 17 : 18;
    for (uint32_t s = 0; s < M2_SLOTS; s++) if (s < s0 || s >= s1) REQUIRE(sn[s] == 0, "m2_off_stream: absent streams count 0");
    for (uint32_t s = s0; s < s1; s++) {
        REQUIRE(mb[s].cnt == o && o + 4 <= L, "k_rans1_decode: blkp = blob + cnt, the block's word inside the tile");
        const uint32_t h = rd32(blob + o), bt = h >> 24, sz = h & 0xFFFFFF, Nnom = P::m2_nominal(s), pb = s >= 17 ? 15 : 14;
        REQUIRE(bt <= 4 && mb[s].type == bt && sz >= 4 && o + sz <= L, "k_rans1_decode: the block [cnt, cnt + size) inside the tile");
        uint32_t m = 0;
        if (bt) {
            REQUIRE(sz >= 8, "k_rans1_decode: the symbol count word");
            const uint32_t w1 = rd32(blob + o + 4);
            m = bt == 1 ? w1 & 0xFFFFFF : w1;
            if (bt == 1) REQUIRE(mb[s].pbits == (w1 >> 24), "rans1_dec_plain: the single symbol");
            if (bt == 2) { REQUIRE(mb[s].pbits == pos, "rans1_dec_plain: the raw symbols' bit offset in b"); pos += (uint64_t)m * (uint32_t)bit_width(Nnom - 1); }
            if (bt >= 3) {
                REQUIRE(sz >= 24, "k_rans1_decode / k_rans1_dec_prep: two states at +8 and +16, nw = (size - 24) >> 2 >= 0");
                const uint16_t *F = tabs + (uint64_t)s * 256;
                for (uint32_t i = 0; i < Nnom; i++) {
                    uint32_t f;
                    const uint64_t at = pos;
                    if (bt == 3) { f = b_bits(bw, pos, pb, endbit); pos += pb; }
                    else if (b_bits(bw, pos, 1, endbit)) { f = b_bits(bw, pos + 1, pb, endbit); pos += pb + 1; }
                    else { f = 0; pos += 1; }
                    REQUIRE(F[i] == f, "rans_dec_cum: the table entries are b's fields");
                    if (at >= endbit) REQUIRE(F[i] == 0, "rans_dec_cum: the entries behind endbit are 0");
                }
            }
        }
        REQUIRE(mb[s].n == m && sn[s] == m, "k_rans1_decode / m2_off_stream: M2Blk.n and stream_n are the header's count");
        room += P::m2_slot(m);
        REQUIRE(P::m2_off_stream(n, sn, s) + sn[s] <= region && room <= region, "k_rans1_decode: m2_off_stream(s) + stream_n[s] inside m2_streams_region(n)");
        REQUIRE(m <= ((s >= 11 && s < 17) ? 3 * n : n), "k_m2_dec_resid: a stream within its cap");
        if (s < 9) coded += m;
        o += sz;
    }
    REQUIRE(d.coded == coded && coded <= n - 1, "k_m2_dec_walk: coded = the nine counts together <= n - 1 steps of the chain");
}

// ---- one case, one phase: the launch of one tile
static FILE *g_verdicts;
static void run_case(const Case &c, uint32_t ph) {
    Placed pl(c.bytes.data(), c.avail, ph);
    g_may_read = {pl.range()};
    g_what = c.name.c_str();
    const uint8_t *blobs[1] = {pl.blob};
    const uint64_t off[1] = {0}, blob_len[1] = {c.avail};
    const uint32_t h = c.n / c.w;
    const TileDesc tiles[1] = {{0, 0, c.w, h, c.n, 0, 0, 0}};
    const TileSel sel{0, 1, 1, 1, nullptr};
    uint32_t status = 0;
    bool accepted;
    if (c.mode == 1) {
        DecTile info[1];
        memset(info, 0xCD, sizeof info);
        launch(1, 1, [&] { P::k_dec_parse(blobs, off, blob_len, 1, 1, c.pxsz == 4 ? 10 : 9, (int)c.pxsz, tiles, sel, info, &status); });
        accepted = info[0].type != TILE_BAD;
        if (accepted) contract_m1(info[0], pl.blob, c.avail, c.n, (int)c.pxsz, g_what);
    } else {
        M2DecTile info[1];
        memset(info, 0xCD, sizeof info);
        std::vector<M2Blk> blk(M2_SLOTS, M2Blk{0, 0, 0, 0});  // (decode_m2_launch clears the block records)
        std::vector<uint16_t> tabs(M2_SLOTS * 256, 0x7E7E);
        std::vector<uint32_t> sn(M2_SLOTS, 0xDEADBEEFu);
        launch(1, 1, [&] { P::k_m2_dec_parse(blobs, off, blob_len, 1, 1, tiles, sel, info, blk.data(), tabs.data(), sn.data(), &status); });
        accepted = info[0].kind != M2_KIND_BAD;
        for (uint32_t s = 0; s < M2_SLOTS; s++) if (sn[s] == 0xDEADBEEFu) { bad("stream_n entry never written", s, 0); break; }
        if (accepted) contract_m2(info[0], blk.data(), sn.data(), tabs.data(), pl.blob, c.avail, c.n, g_what);
    }
    if ((status & 1u) != (accepted ? 0u : 1u) || (status & ~1u)) { if (errors < 20) printf("status %u beside the tile's mark: %s\n", status, g_what); errors++; }
    if (accepted != (c.expect == 1)) { if (errors < 20) printf("verdict %s, the rules say %s: %s (phase %u)\n", accepted ? "accept" : "reject", c.expect ? "accept" : "reject", g_what, ph); errors++; }
    if (ph == 0 && g_verdicts) fprintf(g_verdicts, "%d %s\n", accepted ? 1 : 0, g_what);
}

// ---- 2 images x 3 tiles, one bad tile, in the three selection forms and the mixed form
static void selection_forms(uint32_t mode, uint32_t pxsz) {
    const Case *base = nullptr;
    for (const Case &c : g_cases)
        if (c.mode == mode && c.pxsz == pxsz && c.expect == 1 && c.avail == (rd32(c.bytes.data()) & 0xFFFFFF) && c.bytes[3] != 0 && c.bytes[3] != 255 && c.avail > 64) { base = &c; break; }
    if (!base) { bad("no base tile for the selection forms", mode, pxsz); return; }
    const uint32_t L = base->avail, N = 3, NI = 2, bad_img = 1, bad_tile = 1;
    std::vector<uint8_t> img[2];
    for (uint32_t i = 0; i < NI; i++) {
        for (uint32_t t = 0; t < N; t++) img[i].insert(img[i].end(), base->bytes.begin(), base->bytes.end());
        if (i == bad_img) img[i][bad_tile * L + 3] = 0x7F;  // a type byte both parsers reject; the size word stays
    }
    Placed p0(img[0].data(), 3 * L, 1), p1(img[1].data(), 3 * L, 3);
    const uint8_t *blobs[2] = {p0.blob, p1.blob};
    const uint64_t blob_len[2] = {3ull * L, 3ull * L};
    g_may_read = {p0.range(), p1.range()};
    const uint32_t h = base->n / base->w;
    // tile tables: per image N entries; the mixed form's is the concatenation with nimg = 1
    std::vector<TileDesc> tiles;
    for (uint32_t i = 0; i < NI; i++) for (uint32_t t = 0; t < N; t++) tiles.push_back({0, 0, base->w, h, base->n, i, 0, 0});
    static const uint32_t order[3] = {2, 0, 1}, list[4] = {5, 0, 4, 2}, all[6] = {3, 1, 5, 0, 4, 2}, first[3] = {0, 3, 6};
    struct Form { const char *what; TileSel sel; uint32_t total; bool full_off; } forms[4] = {
        {"range t0 = 1", {1, 2, N, NI, nullptr}, 4, false},
        {"order", {0, 3, N, NI, order}, 6, false},
        {"list", {0, 4, N, NI, nullptr, list}, 4, true},
        {"mixed", {0, 6, 6, 1, nullptr, all}, 6, true},
    };
    for (const Form &f : forms) {
        g_what = f.what;
        const TileSel &sel = f.sel;
        // off[]: indexed as imglin says (per image cnt entries from t0, or - list forms - the whole table); the other entries are poison
        std::vector<uint64_t> off(NI * N, ~0ull);
        if (f.full_off) {
            if (sel.nimg == 1) launch(1, 1, [&] { P::k_dec_offsets_mixed(blobs, blob_len, first, NI, off.data()); });
            else launch(1, 1, [&] { P::k_dec_offsets(blobs, blob_len, N, NI, off.data()); });
            for (uint32_t i = 0; i < NI * N; i++) if (off[i] != (uint64_t)(i % N) * L) bad("size walk of an intact image", i, (long)off[i]);
        } else for (uint32_t i = 0; i < NI; i++) for (uint32_t k = 0; k < sel.cnt; k++) off[i * sel.cnt + k] = (uint64_t)(sel.t0 + k) * L;
        uint32_t status = 0;
        std::vector<DecTile> i1(f.total);
        std::vector<M2DecTile> i2(f.total);
        std::vector<M2Blk> blk(NI * N * M2_SLOTS, M2Blk{0, 0, 0, 0});
        std::vector<uint16_t> tabs((size_t)NI * N * M2_SLOTS * 256, 0);
        std::vector<uint32_t> sn(NI * N * M2_SLOTS, 0xDEADBEEFu);
        memset(i1.data(), 0xCD, i1.size() * sizeof(DecTile));
        memset(i2.data(), 0xCD, i2.size() * sizeof(M2DecTile));
        if (mode == 1) launch(1, 1, [&] { P::k_dec_parse(blobs, off.data(), blob_len, sel.cnt, f.total, pxsz == 4 ? 10 : 9, (int)pxsz, tiles.data(), sel, i1.data(), &status); });
        else launch(1, 1, [&] { P::k_m2_dec_parse(blobs, off.data(), blob_len, sel.cnt, f.total, tiles.data(), sel, i2.data(), blk.data(), tabs.data(), sn.data(), &status); });
        uint32_t marked = 0, has_bad = 0;
        std::vector<bool> touched(NI * N, false);
        for (uint32_t j = 0; j < f.total; j++) {
            // this program's own statement of the three enumerations
            uint32_t im, t;
            if (sel.list) { im = sel.list[j] / N; t = sel.list[j] % N; }
            else if (sel.order) { im = j % NI; t = order[j / NI]; }
            else { im = j / sel.cnt; t = sel.t0 + j % sel.cnt; }
            const uint32_t vt = im * N + t;
            touched[vt] = true;
            const uint8_t *want = blobs[im] + (uint64_t)t * L;
            const bool is_bad = im == bad_img && t == bad_tile;
            has_bad += is_bad;
            const bool got_bad = mode == 1 ? i1[j].type == TILE_BAD : i2[j].kind == M2_KIND_BAD;
            marked += got_bad;
            if ((mode == 1 ? i1[j].blob : i2[j].blob) != want) bad("record of work item names another tile's bytes", j, vt);
            if (got_bad != is_bad) bad("the launch marks the wrong tile", j, vt);
            if (!got_bad) {
                if (mode == 1) contract_m1(i1[j], want, L, base->n, (int)pxsz, f.what);
                else contract_m2(i2[j], blk.data() + (size_t)vt * M2_SLOTS, sn.data() + (size_t)vt * M2_SLOTS, tabs.data() + (size_t)vt * M2_SLOTS * 256, want, L, base->n, f.what);
            }
        }
        if (marked != has_bad || status != (has_bad ? 1u : 0u)) bad("marks / status of the launch", marked, status);
        if (mode == 2) for (uint32_t vt = 0; vt < NI * N; vt++) if (!touched[vt] && sn[vt * M2_SLOTS] != 0xDEADBEEFu) bad("stream_n of a tile outside the launch written", vt, 0);
    }
}

// ---- the size walks
static void size_walks() {
    struct Chain { const char *what; std::vector<uint32_t> sizes; int brk; uint32_t cut; };  // brk: index of the first tile whose word breaks the walk (-1: none); cut: bytes kept (0: all)
    const std::vector<Chain> chains = {
        {"intact", {40, 8, 52, 7, 100}, -1, 0},
        {"ends one byte inside a size word", {40, 8, 52, 7, 100}, 3, 40 + 8 + 52 + 1},
        {"ends inside a size word", {40, 8, 52, 7, 100}, 3, 40 + 8 + 52 + 2},
        {"ends one byte short of a size word", {40, 8, 52, 7, 100}, 3, 40 + 8 + 52 + 3},
        {"ends before a size word", {40, 8, 52, 7, 100}, 3, 40 + 8 + 52},
        {"size 0", {40, 8, 0, 7, 100}, 2, 0},
        {"size beyond the buffer", {40, 8, 0xFFFFFF, 7, 100}, 2, 0},
        {"size one byte beyond the buffer", {40, 8, 52, 7, 101}, 4, 40 + 8 + 52 + 7 + 100},
        {"size lands exactly on L", {40, 8, 52, 7, 100}, -1, 0},
        {"size lands exactly on L early", {40, 8, 52}, -1, 0},
    };
    const uint32_t cnt = 6;
    for (uint32_t ph = 0; ph < 4; ph++) {
        std::vector<Placed *> pl;
        std::vector<const uint8_t *> blobs;
        std::vector<uint64_t> lens;
        std::vector<std::vector<uint64_t>> want;
        g_may_read.clear();
        for (const Chain &c : chains) {
            std::vector<uint8_t> b;
            std::vector<uint64_t> starts;
            for (size_t i = 0; i < c.sizes.size(); i++) {
                starts.push_back(b.size());
                const uint32_t s = c.sizes[i], room = s == 0 || s > 4096 ? 12 : s;
                const uint32_t word = s | 0x12000000u;  // (a type byte above the size: the walk takes the low 24 bits)
                for (uint32_t k = 0; k < room; k++) b.push_back(k < 4 ? (uint8_t)(word >> (8 * k)) : 0x99);
            }
            if (c.cut) b.resize(c.cut);
            const uint64_t L = b.size();
            std::vector<uint64_t> w(cnt);
            for (uint32_t i = 0; i < cnt; i++) {
                const bool before = c.brk < 0 ? i < c.sizes.size() : (int)i <= c.brk;
                w[i] = before ? starts[i] : L;
                if (c.brk < 0 && i >= c.sizes.size()) w[i] = L;
            }
            want.push_back(w);
            pl.push_back(new Placed(b.data(), (uint32_t)L, (ph + (uint32_t)pl.size()) & 3));
            blobs.push_back(pl.back()->blob); lens.push_back(L);
            g_may_read.push_back(pl.back()->range());
        }
        const uint32_t NI = (uint32_t)chains.size();
        auto check = [&](const char *form, const uint64_t *off, uint32_t b) {
            g_what = chains[b].what;
            for (uint32_t i = 0; i < cnt; i++) {
                if (off[i] != want[b][i]) { if (errors < 20) printf("%s walk, %s: off[%u] = %lld, not %lld\n", form, g_what, i, (long long)off[i], (long long)want[b][i]); errors++; }
                if (off[i] > lens[b] || (i && off[i] < off[i - 1])) { if (errors < 20) printf("%s walk, %s: off[] beyond L or not monotonic\n", form, g_what); errors++; }
            }
        };
        g_what = "batched size walk";
        std::vector<uint64_t> off(NI * cnt + 2, 0xABABABABABABABABull);
        launch(1, 1, [&] { P::k_dec_offsets(blobs.data(), lens.data(), cnt, NI, off.data() + 1); });
        for (uint32_t b = 0; b < NI; b++) check("batched", off.data() + 1 + b * cnt, b);
        if (off[0] != 0xABABABABABABABABull || off[NI * cnt + 1] != 0xABABABABABABABABull) bad("batched walk wrote outside its table", 0, 0);
        // mixed: every image with its own number of tiles (the chain's, or cnt), one image per launch: nothing of another image moves
        std::vector<uint32_t> first(NI + 1, 0);
        for (uint32_t b = 0; b < NI; b++) first[b + 1] = first[b] + cnt;
        std::vector<uint64_t> moff(first[NI], 0xABABABABABABABABull);
        for (uint32_t b = 0; b < NI; b++) {
            const std::vector<uint64_t> before = moff;
            g_what = chains[b].what;
            launch(1, 1, [&] { P::k_dec_offsets_mixed(blobs.data() + b, lens.data() + b, first.data() + b, 1, moff.data()); });
            check("mixed", moff.data() + first[b], b);
            for (uint32_t i = 0; i < first[NI]; i++) if ((i < first[b] || i >= first[b + 1]) && moff[i] != before[i]) bad("mixed walk moved another image's entry", b, i);
        }
        g_what = "mixed size walk of all images";
        std::vector<uint64_t> mall(first[NI], 0);
        launch(1, 1, [&] { P::k_dec_offsets_mixed(blobs.data(), lens.data(), first.data(), NI, mall.data()); });
        if (mall != moff) bad("mixed walk of all images differs from the walks one by one", 0, 0);
        for (Placed *p : pl) delete p;
    }
}

int main() {
    load_cases(CASE_FILE);
    g_verdicts = fopen(CASE_FILE ".verdicts", "w");
    long runs = 0;
    for (const Case &c : g_cases) for (uint32_t ph = 0; ph < 4; ph++, runs++) run_case(c, ph);
    if (g_verdicts) fclose(g_verdicts);
#ifndef VERDICTS_ONLY
    selection_forms(1, 3); selection_forms(1, 4); selection_forms(2, 3);
    size_walks();
#endif
    printf("cases: %zu runs: %ld checked reads: %ld\nerrors: %d\n", g_cases.size(), runs, g_reads, errors);
    return errors != 0;
}
