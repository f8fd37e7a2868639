"""CPU: the staging copy kernels (xpng_amd/csrc/mixed.hpp k_mixed_copy, k_mixed_pack, k_mixed_copy_as, k_mixed_pack_from) run on the host.

Their text is cut out of mixed.hpp and compiled into tests/layout_kernels_host.cpp, a stand-alone program with shims for the three
device operations they use, built with a statically linked AddressSanitizer where the toolchain has one.  It runs every thread of
every block one after another for both pixel sizes, the tight pair, all 12 layouts out of a staging raster and the 4 + 4 layouts into it, on widths 1 .. 9 (every alignment of a row and of a
plane row), wider rows than a wave covers and several images per launch in both orders, and checks every byte: the values, the
sentinels around every caller's buffer, the untouched padding of the staging rows, and that ld32u reads only aligned dwords that
hold a byte of the buffer it is reading."""
import _kit as K


def test_layout_kernels_on_the_host(tmp_path):
    text = K.cut("mixed.hpp", "struct MixedLayout {")
    assert all(k in text for k in ("k_mixed_copy(", "k_mixed_pack(", "k_mixed_copy_as(", "k_mixed_pack_from("))
    K.run_kernels_on_host(tmp_path, "layout_kernels_host", {"KERNEL_TEXT": text})
