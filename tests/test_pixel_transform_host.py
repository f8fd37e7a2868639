"""CPU: the byte-parallel per-pixel transform of the encode (xpng_amd/csrc/m1_encode.hpp m1_pixel_interior) run on the host.

Its text - swar_sub8, swar_zigzag8 and m1_pixel_interior - is cut out of m1_encode.hpp and compiled into
tests/pixel_transform_host.cpp, a stand-alone program with shims for v_lerp_u8 and the multiply-by-3 instruction, which compares it
with a plain scalar restatement of libxpng.c:497-513 on every (L, U, UL) out of 16 values per channel (both ends and the middle of
the byte range, where the damped gradient leaves 0..255), a different triple in each channel, for the four predictors, column 0 and
interior pixels, and transparent, nearly transparent and opaque alpha.  A lost bias, a wrong shift or a carry between the 16-bit
lanes of the gradient fails here without a GPU (dropping the `+ 0x04020402u` bias: checked, it fails)."""
import _kit as K


def test_interior_pixel_transform_on_the_host(tmp_path):
    text = K.cut("m1_encode.hpp", "__device__ __forceinline__ uint32_t swar_sub8", "// four interior RGB pixels", last=False)
    assert "m1_pixel_interior" in text and "0x04020402u" in text and "asm" not in text
    r = K.run_kernels_on_host(tmp_path, "pixel_transform_host", {"KERNEL_TEXT": text},
                              sanitize=("-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"), timeout=120)
    assert "runs: 6291456" in r.stdout
