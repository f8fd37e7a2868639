"""CPU: the float copy-out kernel (xpng_amd/csrc/mixed_float.hpp k_mixed_copy_as_float) run on the host.

Its text is cut out of mixed_float.hpp and compiled into tests/float_kernels_host.cpp, a stand-alone program with shims for the
device operations the kernel uses (its loads, stores, v_perm, v_alignbyte, the fp32 multiply-add and the two narrowing
conversions), built with a statically linked AddressSanitizer where the toolchain has one.  It runs every thread of every block one
after another for both pixel sizes, all 12 layouts and the three element types on widths 1 .. 17 (every start of a row and of a
plane row modulo 16 bytes, rows shorter than one 16-byte store), rows wider than one pass of a wave and several images per launch
in both orders, and checks every element against fmaf() and the program's own round-to-nearest-even conversions, the sentinels
around every buffer, that every store is aligned and inside a buffer, and that no staging read reaches more than 7 bytes behind the
pixels of its row."""
import _kit as K


def test_float_kernels_on_the_host(tmp_path):
    text = K.cut("mixed_float.hpp", "struct FloatConsts {")
    assert "k_mixed_copy_as_float" in text and "asm" not in text and "address_space" not in text
    K.run_kernels_on_host(tmp_path, "float_kernels_host", {"TYPES_TEXT": K.product_types("layout", "dw"), "KERNEL_TEXT": text})
