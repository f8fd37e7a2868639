"""CPU: the resample copy-out kernel (xpng_amd/csrc/mixed_resample.hpp k_mixed_resample_as_float) run on the host.

Its text, and in front of it the texts of mixed_float.hpp and mixed_resize.hpp whose named operations it reuses, is cut out of the
headers and compiled into tests/resample_kernels_host.cpp, a stand-alone program with shims for the device operations (loads,
stores, the fp32 multiply-add, the two narrowing conversions), built with contraction off and with a statically linked
AddressSanitizer where the toolchain has one.  It runs every thread of every block one after another for all 24 instances: source
widths 1 .. 17 and heights 1 .. 3 plus larger images, output widths 1 .. 17, so ratios on both sides of 1 on each axis, alone and
mixed; whole-image, last-pixel, last-column, last-row and output-sized rectangles and rectangles strictly inside the image, with
both flips.  It checks every element against the program's own plain statement of the rule, the sentinels around every buffer, that
every store is aligned and inside a buffer - and that no staging read leaves the image's rectangle."""
import _kit as K


def test_resample_kernels_on_the_host(tmp_path):
    ftext = K.cut("mixed_float.hpp", "struct FloatConsts {")
    rtext = K.cut("mixed_resize.hpp", "struct ResizeRec {")
    text = K.cut("mixed_resample.hpp", "struct ResampleRec {")
    assert "k_mixed_resample_as_float" in text and "asm" not in text and "address_space" not in text
    K.run_kernels_on_host(tmp_path, "resample_kernels_host",
                          {"TYPES_TEXT": K.product_types("layout", "dw"), "FLOAT_TEXT": ftext, "RESIZE_TEXT": rtext, "KERNEL_TEXT": text},
                          flags=("-ffp-contract=off",))
