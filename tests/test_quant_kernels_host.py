"""CPU: the staging kernel of the tensor store (xpng_amd/csrc/stage_from.hpp k_images_stage_from) run on the host.

Its text is cut out of stage_from.hpp and compiled into tests/quant_kernels_host.cpp, a stand-alone program with shims for the
device operations the kernel uses (its loads, stores, v_alignbyte, the widening of f16 and bf16, the fp32 multiply-add and the
quantisation), built with a statically linked AddressSanitizer where the toolchain has one.  It runs every thread of every block
one after another for all 16 instances and both colour orders on npx = 1 .. 9 with the source at every element offset 0 .. 7 of a
sentinel-framed arena, on a size above one grid pass and on several images per launch that mix 3 and 4 channels, and checks every
byte against the rule computed with fmaf(), that every store is dword-aligned (the tail: single bytes) and inside the image's slot,
that no read leaves the aligned dwords the buffer occupies, and the sentinels."""
import _kit as K


def test_quant_kernels_on_the_host(tmp_path):
    text = K.cut("stage_from.hpp", "// ---- staging from tensors")
    assert "k_images_stage_from" in text and "asm" not in text and "address_space" not in text
    K.run_kernels_on_host(tmp_path, "quant_kernels_host", {"TYPES_TEXT": K.product_types("float"), "KERNEL_TEXT": text})
