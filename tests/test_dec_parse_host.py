"""CPU: the four validators of the decode - k_dec_parse, k_dec_offsets, k_dec_offsets_mixed (m1_decode.hpp), k_m2_dec_parse
(m2_decode.hpp) - run on the host over crafted and boundary-mutated tile headers.

Every later decode kernel takes the records these four write on faith, so they alone stand between a file's bytes and an out-of-range
address.  Their text, with the records and helpers they name, is cut out of the product headers and compiled with
-fsanitize=address,undefined into tests/dec_parse_host.cpp, a stand-alone program; tests/_hostile.py makes the cases (every header
field of oracle-written tiny tiles at 0, 1, min - 1, min, value - 1, value, value + 1, max, max + 1, all ones; the compound cases one
edit cannot reach) and the verdict of each from rules written from the format.  The program checks, at the four byte phases of a blob
at the end of an exact-size heap block: verdict == rule, status bit 0 and the TILE_BAD / M2_KIND_BAD mark, every read of the parsers
inside the bytes that exist (rejected cases too), the record of every accepted case against the consumers' contract (contract_m1,
contract_m2), one bad tile among 2 x 3 in the range / order / list / mixed selection forms, and both size walks on intact and broken
chains.  The rejected cases of tests/test_hostile_tiles.py (the device test) run here too.

THE TESTS BITE: every conjunct of the two `ok` chains and of the walks was deleted or moved by one on a scratch copy; the case that
then fails (`read` = the parser read bytes that do not exist, `contract` = an accepted record broke a consumer's clause; otherwise
the verdict differs from the rule):
  k_dec_parse
    avail >= 4                     photo4x4/avail=3 (read)
    L <= avail                     photo64x64/L=6113 (contract)
    raw: L == n pxsz + 4           photo4x4/L=0 (as <=), photo4x4/L=53 in front of 8 more bytes (as >=)
    L >= 12                        deleted: coded tile L=4 in 4 bytes (read); as >= 7: coded tile L=7 in 7 bytes (read).  8 .. 12 give the
                                   same verdicts: ksz >= 8 and 4 + ksz <= L imply L >= 12; the conjunct guards the read of ksz
    (type >> 4) == 1               photo64x64/type=1
    ksz >= 8                       ksz=4: no k word (contract)
    (ksz & 3) == 0                 ksz=10 over 1 words
    4 + ksz <= L                   REDUNDANT: o = 4 + ksz (64 bits) and block 0's o + 4 <= L imply it; a tile has at least 9 blocks
    o + 4 <= L                     tile and buffer end 1 bytes inside the last block word (read)
    ty <= 4                        photo64x64/blk2.type=5
    sz >= 8 (ty != 0)              flat64x64/blk8.type=1 (read)
    (sz & 3) == 0                  steered64x64/blk6.size=219
    o + sz <= L                    photo64x64/L=6111
    ty 2: v2 >= 1, v2 <= 8         photo64x64/blk0.v2=0, gray16x3/blk4.v2=9
    ty 2: 8 + 4 ceil(n v2/32) <= sz  photo64x64/blk0.v2=8
    ty >= 3: sz >= 32              deleted: last block type 3 of 8 bytes (read).  28 .. 32 give the same verdicts: toff >= 5,
                                   8 + 4 toff < sz and sz % 4 == 0 imply sz >= 32; the conjunct guards the read of the third word
    ty >= 3: v2 <= 254             photo64x64/blk2.v2=255
    pb >= 10, pb <= 15             photo64x64/blk2.pb=9, blk2.pb=16
    toff >= 5                      photo64x64/blk2.toff=4 (nw would wrap)
    8 + 4 toff < sz                photo64x64/blk2.toff=21
    coded <= n - 1                 photo64x64/blk0.n=11
    blk_n[9] <= n - 1              m1.4.photo64x64/alpha9.n=4096
  k_m2_dec_parse
    avail >= 4                     photo4x4/avail=3 (read)
    L <= avail                     photo64x64/L=5981
    L >= 5                         REDUNDANT: every kind has its own bound (3 n + 4, 8, n + 4, L >= 8) and an unknown kind fails
    kind 0: L == 3 n + 4           photo4x4/L=5 (as <=), photo4x4/L=53 in front of 8 more bytes (as >=)
    kind 4: L == 8                 photo4x4/kind=255 (as >= 7), flat4x4/L=5 (as <=)
    kind 3: L == n + 4             flat4x4/kind=43 (as <=), photo4x4/kind=43 (as >=)
    else ok = false                photo64x64/kind=1
    L >= 8                         kind 0x10 L=5 n=1 in 5 bytes (read); as >= 7: kind 0x10 L=7 n=1 in 7 bytes (read)
    bsz >= 8                       gray bsz=4 (contract)
    (bsz & 3) == 0                 gray b of 5 bytes, a block behind it
    4 + bsz + 4 <= L               REDUNDANT: the first block's o + 4 <= L implies it, but for bsz = 2^32 - 4, where the 32-bit o wraps to 0
                                   and the "block word" read there is the tile's own, whose type >= 0x10 fails type <= 4 (case bsz=0xfffffffc)
    o + 4 <= L                     ramp20x12/blk15.size=5 (read)
    type <= 4                      photo64x64/blk2.type=5
    bsize >= 4 / 8                 ramp20x12/blk16.size=3, photo64x64/blk14.type=1
    o + bsize <= L                 photo64x64/L=5979
    type >= 3: bsize >= 24         gray64x64/blk17.size=23
    nsym <= ncap                   gray64x64/blk17.nsym=4097
    room <= m2_streams_region(n)   stream slots sum to the region and one slot
    coded <= n - 1                 photo64x64/blk0.nsym=11
  k_dec_offsets / k_dec_offsets_mixed
    o + 4 <= L                     chain "ends one byte short of a size word" (read)
    sz != 0                        chain "ends inside a size word" (off[] stops moving)
    o + sz <= L                    chain "size one byte beyond the buffer" (off[5] = 208 > L)
No accepted case broke the contract: the parsers needed no change."""
import collections

import _hostile as H
from _kit import po  # noqa: F401  (fixture)


def test_decode_validators_on_hostile_headers(tmp_path, po):
    cs = H.build(po)
    names = [c.name for c in cs.cases]
    assert len(set(names)) == len(names)
    seen = collections.defaultdict(set)
    for c in cs.cases:
        seen[c.field].add(c.verdict)
    # both verdicts for every edited field - but a block's single symbol (mode 2: a byte of its own) has no illegal value: all accepted
    assert seen.pop("m2.blk.sym") == {H.ACCEPT}
    assert all(v == {H.ACCEPT, H.REJECT} for v in seen.values()), {f: v for f, v in seen.items() if len(v) < 2}
    assert {f.split(".", 1)[1] for f in seen if f.startswith("m1.")} >= {"L", "type", "ksz", "blk.type", "blk.size", "blk.n", "blk.v2", "blk.toff", "blk.pb",
                                                                       "alpha.type", "alpha.size", "alpha.n", "alpha.v2", "alpha.toff", "alpha.pb", "avail"}
    assert {f.split(".", 1)[1] for f in seen if f.startswith("m2.")} >= {"L", "kind", "bsz", "blk.type", "blk.size", "blk.nsym", "avail"}
    # the device test's cases go through the same program: what it sends to a GPU is rejected here first
    dev = []
    for mode, pxsz in H.FORMATS:
        picked = H.device_cases(po, mode, pxsz)[-1]
        assert 10 <= len(picked) <= 15 and all(c.verdict == H.REJECT for c in picked)
        dev += picked
    r, verdicts, n = H.run_parsers_on_host(tmp_path, cs, cs.cases + dev)
    print(r.stdout.strip().splitlines()[-2])
    assert n == len(cs.cases) + len(dev) and n > 5000             # the floor is the count generated; thousands, not a guess
    assert int(r.stdout.split("cases: ")[1].split()[0]) >= n
    for c in cs.cases + dev:
        assert verdicts[c.name] == (c.verdict == H.ACCEPT), c.name
