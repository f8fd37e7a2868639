"""CPU: the copy-out kernel of a views call with a colour matrix per view (xpng_amd/csrc/mixed_views_colour.hpp
k_mixed_views_colour) run on the host.

Its text, and in front of it the texts of mixed_float.hpp, mixed_resize.hpp, mixed_resample.hpp, the record of mixed_views.hpp and
the end of a pixel and the row writers of mixed_views_pixel.hpp whose named operations it reuses, is cut out of the headers and compiled into tests/views_colour_kernels_host.cpp, a stand-alone
program with its own main and with shims for the device operations (loads, stores, the fp32 multiply-add, the two narrowing
conversions), built with contraction off and with a statically linked AddressSanitizer where the toolchain has one; nothing
sanitised is loaded into Python.  It runs every thread of every block one after another for all 24 instances and both filters.  A
launch holds more views than images, as the views kernel's program does, and every view has a matrix of its own: the identity, a
non-symmetric permutation, gray, one that leaves 0 .. 255 on both sides, a dense one.  It checks every element against the
program's own plain statement of the rule, the sentinels around every buffer, that every store is aligned and inside the buffer of the view whose block made it - and that no
staging read leaves the rectangle of that view."""
import _kit as K


def test_views_colour_kernels_on_the_host(tmp_path):
    ftext = K.cut("mixed_float.hpp", "struct FloatConsts {")
    rtext = K.cut("mixed_resize.hpp", "struct ResizeRec {")
    stext = K.cut("mixed_resample.hpp", "struct ResampleRec {")
    vtext = K.cut("mixed_views.hpp", "struct ViewRec {", "// grid (", last=False)
    ptext = K.cut("mixed_views_pixel.hpp", "// one colour through a row of the matrix and the clamp")
    text = K.cut("mixed_views_colour.hpp", "struct ViewColour {")
    assert "k_mixed_views_colour" in text and "asm" not in text and "address_space" not in text
    assert "static_assert(sizeof(ViewRec) == 64" in vtext and "colour_row(const float *m" in ptext and "row_wide(uint8_t" in ptext
    assert "asm" not in ptext and "address_space" not in ptext and "__global__" not in ptext
    # the kernel restates none of the named operations and records it reuses
    for op in ("resize_tap(uint32_t u", "resample_win(uint32_t u", "resample_weight(uint32_t j", "resample_div(float a", "fma_f32(float v",
               "pick4(const", "store1(uint8_t", "out_st128(uint8_t", "stage_ld8(const", "float_chunk(const", "struct ViewRec",
               "colour_row(const float", "pixel_finish(const float", "pixel_store(uint8_t", "row_narrow(uint8_t", "row_wide(uint8_t"):
        assert op not in text
    K.run_kernels_on_host(tmp_path, "views_colour_kernels_host",
                          {"TYPES_TEXT": K.product_types("layout", "dw"), "FLOAT_TEXT": ftext, "RESIZE_TEXT": rtext, "RESAMPLE_TEXT": stext,
                           "VIEWS_TEXT": vtext, "PIXEL_TEXT": ptext, "KERNEL_TEXT": text},
                          flags=("-ffp-contract=off",))
