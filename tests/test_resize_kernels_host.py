"""CPU: the resize copy-out kernel (xpng_amd/csrc/mixed_resize.hpp k_mixed_resize_as_float) run on the host.

Its text, and in front of it the text of mixed_float.hpp whose named operations it reuses, is cut out of the headers and compiled
into tests/resize_kernels_host.cpp, a stand-alone program with shims for the device operations (loads, stores, the fp32
multiply-add, the two narrowing conversions), built with contraction off and with a statically linked AddressSanitizer where the
toolchain has one.  It runs every thread of every block one after another for both pixel sizes, all 12 layouts and the three
element types: source widths 1 .. 17 and heights 1 .. 3 plus larger images, output widths 1 .. 17 (every start of a row and of a
plane row modulo 16 bytes), an output row wider than one pass of a wave, whole-image, last-pixel, last-column, last-row and
output-sized rectangles with both flips.  It checks every element against the program's own plain statement of the rule, the
sentinels around every buffer, that every store is aligned and inside a buffer, that no staging read reaches more than 7 bytes
behind the pixels of its row - and that none leaves the image's rectangle."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resize_kernels_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the host run of the resize kernels")
    src = open(os.path.join(ROOT, "xpng_amd", "csrc", "mixed_float.hpp")).read()
    ftext = src[src.index("struct FloatConsts {"):src.rindex("}  // namespace xpng")]
    src = open(os.path.join(ROOT, "xpng_amd", "csrc", "mixed_resize.hpp")).read()
    text = src[src.index("struct ResizeRec {"):src.rindex("}  // namespace xpng")]
    assert "k_mixed_resize_as_float" in text and "asm" not in text and "address_space" not in text
    finc, inc = tmp_path / "float_kernels.inc", tmp_path / "resize_kernels.inc"
    finc.write_text(ftext)
    inc.write_text(text)
    exe = tmp_path / "resize_kernels_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", '-DFLOAT_TEXT="%s"' % finc, '-DKERNEL_TEXT="%s"' % inc,
           os.path.join(ROOT, "tests", "resize_kernels_host.cpp"), "-o", str(exe)]
    # the sanitizer's runtime is linked statically, so the program runs in whatever environment the suite runs in; where the
    # toolchain has no static runtime the program is built plain and its own range checks and sentinels are what is checked
    if subprocess.run(cmd + ["-fsanitize=address", "-static-libasan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("errors: 0"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
