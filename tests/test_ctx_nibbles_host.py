"""CPU: the four-bit context queues of the wide level-1 decode (xpng_amd/csrc/rans_dec.hpp, the ctxn_* helpers) run on the host.

The helpers' text is cut out of rans_dec.hpp and compiled into tests/ctx_nibbles_host.cpp, a stand-alone program.

1. Pack, merge and unpack against the layout's restatement (symbol i = nibble i & 1, low first, of byte i >> 1; symbols above 8 are
   stored as 9): ctxn_byte as rans2_dec_plain and the flush of rans2_decode_stream use it; the chain's register gather, its merge of
   the pair's dwords, its rule for inactive steps, unstored blocks and the odd tail, inside wavefronts 0, 1 and 3 blocks longer than
   the stream; the walk's head arithmetic.  Queue lengths 0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65 and a few more, so that the
   odd tail falls into either dword of its block and into a block of its own.
2. A model of k_dec_walk_wide's service rule on one lane for a window of four and of two chunks (one chunk requested per queue and
   service, landed at the next if its slot is free, the head one dword ahead): one queue on every step, two queues alternating, runs
   that end at every offset of a chunk, queues empty from the start, random bursts.  No head may take a window dword that has not
   landed, and the sequence must be that of the direct walk nl = *cx[nl]++.

The window size the product builds (WALK_WIDE_WCH, m1_decode.hpp) must pass 2.  Four chunks do; two chunks do not (a queue popped on
every step outruns them: the window then has to hold 32 symbols and the dword behind them from any position, 40 symbols, and two
chunks hold as few as 33), which is why the four-chunk window is the one that is built."""
import re

import _kit as K


def test_context_nibble_helpers_and_walk_window_model_on_the_host(tmp_path):
    text = K.cut("rans_dec.hpp", "constexpr uint32_t CTXN_CHUNK", "// (end of the nibble pieces", last=False)
    for name in ("ctxn_clamp", "ctxn_byte", "ctxn_gather", "ctxn_merge", "ctxn_sym", "ctxn_pop", "ctxn_cross", "ctxn_dword", "ctxn_chunk"):
        assert "uint32_t %s(" % name in text or "bool %s(" % name in text, name
    assert "asm" not in text and "address_space" not in text
    wch = int(re.search(r"constexpr uint32_t WALK_WIDE_WCH = (\d+);", K.cut("m1_decode.hpp", "constexpr uint32_t WALK_WIDE_WCH")).group(1))
    r = K.run_kernels_on_host(tmp_path, "ctx_nibbles_host", {"KERNEL_TEXT": text}, flags=("-DSHIPPED_WCH=%d" % wch,),
                              sanitize=("-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"), timeout=120)
    print(r.stdout)
    assert "window of %d chunks: 0 violations" % wch in r.stdout
    assert "cases: " in r.stdout and int(r.stdout.split("cases: ")[1].split()[0]) > 100000
