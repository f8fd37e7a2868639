"""CPU: the float copy-out kernel (xpng_amd/csrc/mixed_float.hpp k_mixed_copy_as_float) run on the host.

Its text is cut out of mixed_float.hpp and compiled into tests/float_kernels_host.cpp, a stand-alone program with shims for the
device operations the kernel uses (its loads, stores, v_perm, v_alignbyte, the fp32 multiply-add and the two narrowing
conversions), built with a statically linked AddressSanitizer where the toolchain has one.  It runs every thread of every block one
after another for both pixel sizes, all 12 layouts and the three element types on widths 1 .. 17 (every start of a row and of a
plane row modulo 16 bytes, rows shorter than one 16-byte store), rows wider than one pass of a wave and several images per launch
in both orders, and checks every element against fmaf() and the program's own round-to-nearest-even conversions, the sentinels
around every buffer, that every store is aligned and inside a buffer, and that no staging read reaches more than 7 bytes behind the
pixels of its row."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float_kernels_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the host run of the float kernels")
    src = open(os.path.join(ROOT, "xpng_amd", "csrc", "mixed_float.hpp")).read()
    a, b = src.index("struct FloatConsts {"), src.rindex("}  // namespace xpng")
    text = src[a:b]
    assert "k_mixed_copy_as_float" in text and "asm" not in text and "address_space" not in text
    inc = tmp_path / "float_kernels.inc"
    inc.write_text(text)
    exe = tmp_path / "float_kernels_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", '-DKERNEL_TEXT="%s"' % inc,
           os.path.join(ROOT, "tests", "float_kernels_host.cpp"), "-o", str(exe)]
    # the sanitizer's runtime is linked statically, so the program runs in whatever environment the suite runs in; where the
    # toolchain has no static runtime the program is built plain and its own range checks and sentinels are what is checked
    if subprocess.run(cmd + ["-fsanitize=address", "-static-libasan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("errors: 0"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
