"""CPU: the views copy-out kernel (xpng_amd/csrc/mixed_views.hpp k_mixed_views_as_float) run on the host.

Its text, and in front of it the texts of mixed_float.hpp, mixed_resize.hpp and mixed_resample.hpp whose named operations it
reuses, is cut out of the headers and compiled into tests/views_kernels_host.cpp, a stand-alone program with its own main and
with shims for the device operations (loads, stores, the fp32 multiply-add, the two narrowing conversions), built with contraction
off and with a statically linked AddressSanitizer where the toolchain has one; nothing sanitised is loaded into Python.  It runs
every thread of every block one after another for all 24 instances and both filters.  A launch holds more views than images: views
whose sizes differ, so blocks of short views exit; two and three views of one image with overlapping rectangles; an image without
a view; ratios on both sides of 1 on each axis; both flips; rectangles at the image's edges; output widths that start rows at
every multiple of the element size modulo 16.  It checks every element against the program's own plain statement of the rule, the
sentinels around every buffer, that every store is aligned and inside a buffer - and that no staging read leaves the rectangle of
the view whose block made it."""
import _kit as K


def test_views_kernels_on_the_host(tmp_path):
    ftext = K.cut("mixed_float.hpp", "struct FloatConsts {")
    rtext = K.cut("mixed_resize.hpp", "struct ResizeRec {")
    stext = K.cut("mixed_resample.hpp", "struct ResampleRec {")
    text = K.cut("mixed_views.hpp", "struct ViewRec {")
    assert "k_mixed_views_as_float" in text and "asm" not in text and "address_space" not in text
    # the kernel restates none of the named operations it reuses
    for op in ("resize_tap(uint32_t u", "resample_win(uint32_t u", "resample_weight(uint32_t j", "fma_f32(float v", "float_chunk(const"):
        assert op not in text
    K.run_kernels_on_host(tmp_path, "views_kernels_host",
                          {"TYPES_TEXT": K.product_types("layout", "dw"), "FLOAT_TEXT": ftext, "RESIZE_TEXT": rtext, "RESAMPLE_TEXT": stext,
                           "KERNEL_TEXT": text},
                          flags=("-ffp-contract=off",))
