"""CPU: the staging copy kernels (xpng_amd/csrc/mixed.hpp k_mixed_copy, k_mixed_pack, k_mixed_copy_as, k_mixed_pack_from) run on the host.

Their text is cut out of mixed.hpp and compiled into tests/layout_kernels_host.cpp, a stand-alone program with shims for the three
device operations they use, built with a statically linked AddressSanitizer where the toolchain has one.  It runs every thread of
every block one after another for both pixel sizes, the tight pair, all 12 layouts out of a staging raster and the 4 + 4 layouts into it, on widths 1 .. 9 (every alignment of a row and of a
plane row), wider rows than a wave covers and several images per launch in both orders, and checks every byte: the values, the
sentinels around every caller's buffer, the untouched padding of the staging rows, and that ld32u reads only aligned dwords that
hold a byte of the buffer it is reading."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_kernels_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the host run of the layout kernels")
    src = open(os.path.join(ROOT, "xpng_amd", "csrc", "mixed.hpp")).read()
    a, b = src.index("struct MixedLayout {"), src.rindex("}  // namespace xpng")
    text = src[a:b]
    assert all(k in text for k in ("k_mixed_copy(", "k_mixed_pack(", "k_mixed_copy_as(", "k_mixed_pack_from("))
    inc = tmp_path / "layout_kernels.inc"
    inc.write_text(text)
    exe = tmp_path / "layout_kernels_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", '-DKERNEL_TEXT="%s"' % inc,
           os.path.join(ROOT, "tests", "layout_kernels_host.cpp"), "-o", str(exe)]
    # the sanitizer's runtime is linked statically, so the program runs in whatever environment the suite runs in; where the
    # toolchain has no static runtime the program is built plain and its own range checks and sentinels are what is checked
    if subprocess.run(cmd + ["-fsanitize=address", "-static-libasan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("errors: 0"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
