"""CPU: the staging kernel of the tensor store (xpng_amd/csrc/stage_from.hpp k_images_stage_from) run on the host.

Its text is cut out of stage_from.hpp and compiled into tests/quant_kernels_host.cpp, a stand-alone program with shims for the
device operations the kernel uses (its loads, stores, v_alignbyte, the widening of f16 and bf16, the fp32 multiply-add and the
quantisation), built with a statically linked AddressSanitizer where the toolchain has one.  It runs every thread of every block
one after another for all 16 instances and both colour orders on npx = 1 .. 9 with the source at every element offset 0 .. 7 of a
sentinel-framed arena, on a size above one grid pass and on several images per launch that mix 3 and 4 channels, and checks every
byte against the rule computed with fmaf(), that every store is dword-aligned (the tail: single bytes) and inside the image's slot,
that no read leaves the aligned dwords the buffer occupies, and the sentinels."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quant_kernels_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the host run of the staging kernel")
    src = open(os.path.join(ROOT, "xpng_amd", "csrc", "stage_from.hpp")).read()
    a, b = src.index("// ---- staging from tensors"), src.rindex("}  // namespace xpng")
    text = src[a:b]
    assert "k_images_stage_from" in text and "asm" not in text and "address_space" not in text
    inc = tmp_path / "quant_kernels.inc"
    inc.write_text(text)
    exe = tmp_path / "quant_kernels_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", '-DKERNEL_TEXT="%s"' % inc,
           os.path.join(ROOT, "tests", "quant_kernels_host.cpp"), "-o", str(exe)]
    # the sanitizer's runtime is linked statically, so the program runs in whatever environment the suite runs in; where the
    # toolchain has no static runtime the program is built plain and its own range checks and sentinels are what is checked
    if subprocess.run(cmd + ["-fsanitize=address", "-static-libasan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("errors: 0"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
