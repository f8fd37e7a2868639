"""CPU: the per-pixel rule of the decode's reconstruction (xpng_amd/csrc/recon.hpp recon_px_band, recon_px) run on the host.

Its text - swar_add8, the byte-parallel recon_px_band of the band form and the scalar recon_px of the other two forms - is cut out of
recon.hpp (and pred_avg / pred_grad, which recon_px calls, out of common.hpp) and compiled into tests/recon_pixel_host.cpp, a
stand-alone program with shims for v_lerp_u8 and the multiply-by-3 instruction.  It compares recon_px_band, recon_px<3> and recon_px<4>
with a plain scalar restatement of libxpng.c:798-813 on every (L, U, UL) out of 16 values per channel (both ends and the middle of the
byte range, where the damped gradient leaves 0..255), a different triple in each channel, for the four predictor modes, row 0,
column 0, the tile's first pixel and interior pixels, and a marker byte of 0, 1 and 255.  A lost bias, a wrong shift or a carry
between the 16-bit lanes of the gradient fails here without a GPU (dropping the `+ 0x04020402u` bias: checked, it fails)."""
import _kit as K


def test_reconstruction_pixel_rule_on_the_host(tmp_path):
    preds = K.cut("common.hpp", "__device__ __forceinline__ int pred_avg", "\n\n", last=False)
    text = K.cut("recon.hpp", "__device__ __forceinline__ uint32_t swar_add8", "// (end of the pixel rules", last=False)
    assert "pred_grad" in preds and "recon_px_band" in text and "uint32_t recon_px(" in text and "0x04020402u" in text
    assert "asm" not in preds + text
    r = K.run_kernels_on_host(tmp_path, "recon_pixel_host", {"KERNEL_TEXT": preds + "\n" + text},
                              sanitize=("-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"), timeout=120)
    assert "runs: 3145728" in r.stdout
