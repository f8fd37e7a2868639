"""CPU: the copy-out kernel of a cubic views call (xpng_amd/csrc/mixed_views_cubic.hpp k_mixed_views_cubic) run on the host.

Its text, and in front of it the texts of mixed_float.hpp, the window and the division of mixed_resample.hpp, the record of mixed_views.hpp, the
end of a pixel and the row writers of mixed_views_pixel.hpp and the matrix record of mixed_views_colour.hpp whose named operations it reuses, is cut out of the headers and compiled
into tests/views_cubic_kernels_host.cpp, a stand-alone program with its own main and with shims for the device operations (loads,
stores, the fp32 multiply-add, the two narrowing conversions), built with contraction off and with a statically linked
AddressSanitizer where the toolchain has one; nothing sanitised is loaded into Python.  It runs every thread of every block one
after another for all 24 instances, with a matrix per view and with a null matrix table, over the view programs of the views
kernels' host runs: more views than images, widths shifted by 0 .. 7, wide rows, one-pixel views.  It checks every element against
the program's own plain statement of the rule, the sentinels around every buffer, that every store is aligned and inside the buffer
of the view whose block made it - and that no staging read leaves the rectangle of that view."""
import _kit as K


def test_views_cubic_kernels_on_the_host(tmp_path):
    ftext = K.cut("mixed_float.hpp", "struct FloatConsts {")
    stext = K.cut("mixed_resample.hpp", "struct ResampleRec {", "// grid (", last=False)
    vtext = K.cut("mixed_views.hpp", "struct ViewRec {", "// grid (", last=False)
    ptext = K.cut("mixed_views_pixel.hpp", "// one colour through a row of the matrix and the clamp")
    ctext = K.cut("mixed_views_colour.hpp", "struct ViewColour {", "// grid (", last=False)
    text = K.cut("mixed_views_cubic.hpp", "// the window of one axis")
    assert "k_mixed_views_cubic" in text and "cubic_win(uint32_t u" in text and "cubic_weight(uint32_t j" in text
    assert "asm" not in text and "address_space" not in text
    assert "static_assert(sizeof(ViewRec) == 64" in vtext and "colour_row(const float *m" in ptext and "resample_div(float a" in stext
    assert "row_narrow(uint8_t" in ptext and "static_assert(sizeof(ViewColour) == 48" in ctext
    assert "asm" not in ptext and "address_space" not in ptext and "__global__" not in ptext
    # the kernel restates none of the named operations and records it reuses
    for op in ("resize_tap(uint32_t u", "resample_win(uint32_t u", "resample_weight(uint32_t j", "resample_div(float a", "fma_f32(float v",
               "pick4(const", "store1(uint8_t", "out_st128(uint8_t", "stage_ld8(const", "stage_ld32(const", "float_chunk(const", "struct ViewRec", "struct ViewColour",
               "struct ResampleWin", "colour_row(const", "pixel_finish(const float", "pixel_store(uint8_t", "row_narrow(uint8_t", "row_wide(uint8_t"):
        assert op not in text
    K.run_kernels_on_host(tmp_path, "views_cubic_kernels_host",
                          {"TYPES_TEXT": K.product_types("layout", "dw"), "FLOAT_TEXT": ftext, "RESAMPLE_TEXT": stext,
                           "VIEWS_TEXT": vtext, "PIXEL_TEXT": ptext, "COLOUR_TEXT": ctext, "KERNEL_TEXT": text},
                          flags=("-ffp-contract=off",))
