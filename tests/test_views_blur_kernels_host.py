"""CPU: the second-pass kernel of a blur views call (xpng_amd/csrc/mixed_views_blur.hpp k_mixed_views_blur) run on the host.

Its text, and in front of it the texts of mixed_float.hpp and of mixed_views_pixel.hpp (its pixel_store) whose named operations it reuses, is cut out of the headers and compiled
into tests/views_blur_kernels_host.cpp, a stand-alone program with its own main and with shims for the device operations (the
scratch reads, the stores, the fp32 multiply-add, the two narrowing conversions, the barrier), built with contraction off and with
a statically linked AddressSanitizer where the toolchain has one; nothing sanitised is loaded into Python.  The kernel has
barriers, so the program runs a block's threads as fibers and checks that a barrier is reached by all live threads of a block or by
none.  It runs every thread of every block for all 12 instances, with and without the BGR exchange, over views of every radius in
{0, 1, 11, 31} whose widths come from {R + 1, 63, 64, 65, 130} and heights from {R + 1, 15, 16, 17, 40}.  It checks every element
against the program's own plain loop, the sentinels around every buffer, that every store is aligned and inside the buffer of the
view whose block made it - and that no scratch read leaves the slice of that view."""
import _kit as K


def test_views_blur_kernels_on_the_host(tmp_path):
    ftext = K.cut("mixed_float.hpp", "struct FloatConsts {")
    ptext = K.cut("mixed_views_pixel.hpp", "// one colour through a row of the matrix and the clamp")
    text = K.cut("mixed_views_blur.hpp", "// the tile of one workgroup")
    assert "k_mixed_views_blur" in text and "struct BlurRec {" in text and "blur_refl(int32_t i" in text
    assert "asm" not in text and "address_space" not in text
    assert "pixel_store(uint8_t" in ptext and "asm" not in ptext and "address_space" not in ptext and "__global__" not in ptext
    # the kernel restates none of the named operations it reuses, and every read of the scratch and every barrier is a named one
    for op in ("fma_f32(float v", "pick4(const", "store1(uint8_t", "scratch_ld(const", "blur_sync() {", "__syncthreads", "struct FloatConsts",
               "pixel_finish(const float", "pixel_store(uint8_t", "row_narrow(uint8_t", "row_wide(uint8_t"):
        assert op not in text
    r = K.run_kernels_on_host(tmp_path, "views_blur_kernels_host",
                              {"TYPES_TEXT": K.product_types("layout", "dw"), "FLOAT_TEXT": ftext, "PIXEL_TEXT": ptext, "KERNEL_TEXT": text},
                              flags=("-ffp-contract=off",))
    assert "views: " in r.stdout
