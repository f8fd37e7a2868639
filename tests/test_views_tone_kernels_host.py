"""CPU: the two kernels of the tone steps of a views call (xpng_amd/csrc/mixed_views_tone.hpp k_mixed_views_tone_stats and
k_mixed_views_tone_apply) run on the host.

Their text is cut out of the header and compiled into tests/views_tone_kernels_host.cpp, a stand-alone program with its own main and
with shims for the device operations (the scratch reads and writes, the LDS and global atomics, the wave exchange, the barrier, the
division), built with contraction off and with a statically linked AddressSanitizer where the toolchain has one; nothing sanitised
is loaded into Python.  The kernels have barriers and an exchange between lanes, so the program runs a block's threads as fibers and
checks that every live thread of a block stops at each of them or none does.  It runs every thread of every block of both kernels,
step index after step index, over views of 1 x 1, 1 x 300, 300 x 1, 15 x 16, 16 x 16, 63 / 64 / 65 by 15 / 16 / 17, 130 x 40 and
300 x 200 with one to four steps, and checks every float against the program's own plain loop, that no scratch access leaves the
colour planes of the view whose block made it, that 16-byte accesses are aligned, and that no statistics access leaves the slot of
that view and step."""
import _kit as K


def test_views_tone_kernels_on_the_host(tmp_path):
    text = K.cut("mixed_views_tone.hpp", "constexpr uint32_t TONE_NONE = 0")
    assert "k_mixed_views_tone_stats" in text and "k_mixed_views_tone_apply" in text and "struct ToneRec {" in text
    assert "asm" not in text and "address_space" not in text
    # every access to the scratch and to the slots, every atomic, the exchange, the barrier and the division is a named operation
    for op in ("tone_ld(const", "tone_st(float", "tone_ld4(const", "tone_st4(float", "tone_lds_add(uint32_t", "tone_stat_ld(const", "tone_stat_add(uint32_t",
               "tone_stat_max(uint32_t", "tone_xor(uint32_t", "tone_sync() {", "tone_div(float", "__syncthreads", "atomicAdd", "atomicMax", "__shfl", "__fdiv"):
        assert op not in text, op
    r = K.run_kernels_on_host(tmp_path, "views_tone_kernels_host", {"KERNEL_TEXT": text}, flags=("-ffp-contract=off",))
    assert "views: 36" in r.stdout
