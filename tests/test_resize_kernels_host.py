"""CPU: the resize copy-out kernel (xpng_amd/csrc/mixed_resize.hpp k_mixed_resize_as_float) run on the host.

Its text, and in front of it the text of mixed_float.hpp whose named operations it reuses, is cut out of the headers and compiled
into tests/resize_kernels_host.cpp, a stand-alone program with shims for the device operations (loads, stores, the fp32
multiply-add, the two narrowing conversions), built with contraction off and with a statically linked AddressSanitizer where the
toolchain has one.  It runs every thread of every block one after another for both pixel sizes, all 12 layouts and the three
element types: source widths 1 .. 17 and heights 1 .. 3 plus larger images, output widths 1 .. 17 (every start of a row and of a
plane row modulo 16 bytes), an output row wider than one pass of a wave, whole-image, last-pixel, last-column, last-row and
output-sized rectangles with both flips.  It checks every element against the program's own plain statement of the rule, the
sentinels around every buffer, that every store is aligned and inside a buffer, that no staging read reaches more than 7 bytes
behind the pixels of its row - and that none leaves the image's rectangle."""
import _kit as K


def test_resize_kernels_on_the_host(tmp_path):
    ftext = K.cut("mixed_float.hpp", "struct FloatConsts {")
    text = K.cut("mixed_resize.hpp", "struct ResizeRec {")
    assert "k_mixed_resize_as_float" in text and "asm" not in text and "address_space" not in text
    K.run_kernels_on_host(tmp_path, "resize_kernels_host", {"TYPES_TEXT": K.product_types("layout", "dw"), "FLOAT_TEXT": ftext, "KERNEL_TEXT": text},
                          flags=("-ffp-contract=off",))
