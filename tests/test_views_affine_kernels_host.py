"""CPU: the copy-out kernel of an affine views call (xpng_amd/csrc/mixed_views_affine.hpp k_mixed_views_affine) run on the host.

Its text, and in front of it the texts of mixed_float.hpp, of the end of a pixel and the row writers of mixed_views_pixel.hpp and of
the matrix record of mixed_views_colour.hpp whose named operations it reuses, is cut out of the headers and compiled into tests/views_affine_kernels_host.cpp, a stand-alone program with its own main
and with shims for the device operations (loads, stores, the fp32 multiply-add, the two narrowing conversions), built with
contraction off and with a statically linked AddressSanitizer where the toolchain has one; nothing sanitised is loaded into
Python.  It runs every thread of every block one after another for all 24 instances, both filters and both lane mappings.  A launch
holds more views than images: rotations, a shear, a quarter turn, a mirror, a view partly outside its image, one whose footprint
is empty, views of different heights.  It checks every element against the program's own plain statement of the rule, the sentinels
around every buffer, that every store is aligned and inside the buffer of the view whose block made it - and that no staging read
leaves the footprint of that view."""
import _kit as K


def test_views_affine_kernels_on_the_host(tmp_path):
    ftext = K.cut("mixed_float.hpp", "struct FloatConsts {")
    ptext = K.cut("mixed_views_pixel.hpp", "// one colour through a row of the matrix and the clamp")
    ctext = K.cut("mixed_views_colour.hpp", "struct ViewColour {", "// grid (", last=False)
    text = K.cut("mixed_views_affine.hpp", "struct AffineRec {")
    assert "k_mixed_views_affine" in text and "asm" not in text and "address_space" not in text
    assert "static_assert(sizeof(AffineRec) == 64" in text and "colour_row(const float" in ptext and "k_mixed_views_colour" not in ctext
    assert "row_wide(uint8_t" in ptext and "static_assert(sizeof(ViewColour) == 48" in ctext
    assert "asm" not in ptext and "address_space" not in ptext and "__global__" not in ptext
    # the kernel restates none of the named operations and records it reuses
    for op in ("fma_f32(float v", "pick4(const", "store1(uint8_t", "out_st128(uint8_t", "stage_ld8(const", "float_chunk(const", "struct ViewColour",
               "colour_row(const", "pixel_finish(const float", "pixel_store(uint8_t", "row_narrow(uint8_t", "row_wide(uint8_t"):
        assert op not in text
    K.run_kernels_on_host(tmp_path, "views_affine_kernels_host",
                          {"TYPES_TEXT": K.product_types("layout", "dw"), "FLOAT_TEXT": ftext, "PIXEL_TEXT": ptext, "COLOUR_TEXT": ctext, "KERNEL_TEXT": text},
                          flags=("-ffp-contract=off",))
