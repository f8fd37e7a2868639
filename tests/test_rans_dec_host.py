"""CPU: the symbol look-up and the state update of the rANS decoders (xpng_amd/csrc/rans_dec.hpp) run on the host.

The text of pick32, rans_dec_owner (the search that fills every coarse table of the four decoders, and resolves a slot where there is
no table), wd_reg9 (the register search of the wide chains' small layout) and wd_advance (their 64x32 state update) is cut out of
rans_dec.hpp and compiled into tests/rans_dec_host.cpp, a stand-alone program with shims for v_alignbit_b32 and the 24-bit multiply.
It compares them with a plain restatement of decompress_block (libxpng.c:283-296: cum2sym[], state = F (state >> pb) + slot - cum):
wd_reg9 and rans_dec_owner on every slot of tables with 2 .. 9 symbols at pb 10, 11, 12 and 14 - flat, one dominant symbol, a
zero-frequency symbol at every position, symbol 8 alone behind zeros, random splits with random zeros; the counts behind N hold 2^pb as
the kernels load them -, rans_dec_owner also on 256 symbols at pb 15 with runs of zeros; wd_advance at pb 10 .. 15 on the states 2^31,
2^32 - 1, 2^32, 2^63 - 1 and 4096 random ones, F in {1, 2, 2^pb - 1, 2^pb} (2^pb: the identity entry of an idle lane), off in
{0, F - 1}, with need == (result < 2^31).  Two counts swapped in wd_reg9's tree, or `<=` turned into `<` in rans_dec_owner's search,
fail here without a GPU (both checked)."""
import _kit as K


def test_rans_decode_lookup_and_state_update_on_the_host(tmp_path):
    text = K.cut("rans_dec.hpp", "__device__ __forceinline__ uint32_t pick32", "// (end of the host-run pieces", last=False)
    assert "uint32_t rans_dec_owner(" in text and "uint32_t wd_reg9(" in text and "bool wd_advance(" in text
    assert "asm" not in text and "address_space" not in text
    r = K.run_kernels_on_host(tmp_path, "rans_dec_host", {"KERNEL_TEXT": text},
                              sanitize=("-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"), timeout=120)
    assert "cases: " in r.stdout and int(r.stdout.split("cases: ")[1].split()[0]) > 1000000
