"""CPU: the byte-parallel per-pixel transform of the encode (xpng_amd/csrc/m1_encode.hpp m1_pixel_interior) run on the host.

Its text - swar_sub8, swar_zigzag8 and m1_pixel_interior - is cut out of m1_encode.hpp and compiled into
tests/pixel_transform_host.cpp, a stand-alone program with shims for v_lerp_u8 and the multiply-by-3 instruction, which compares it
with a plain scalar restatement of libxpng.c:497-513 on every (L, U, UL) out of 16 values per channel (both ends and the middle of
the byte range, where the damped gradient leaves 0..255), a different triple in each channel, for the four predictors, column 0 and
interior pixels, and transparent, nearly transparent and opaque alpha.  A lost bias, a wrong shift or a carry between the 16-bit
lanes of the gradient fails here without a GPU (dropping the `+ 0x04020402u` bias: checked, it fails)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_interior_pixel_transform_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the host run of the pixel transform")
    src = open(os.path.join(ROOT, "xpng_amd", "csrc", "m1_encode.hpp")).read()
    a, b = src.index("__device__ __forceinline__ uint32_t swar_sub8"), src.index("// four interior RGB pixels")
    text = src[a:b]
    assert "m1_pixel_interior" in text and "0x04020402u" in text and "asm" not in text
    inc = tmp_path / "pixel_transform.inc"
    inc.write_text(text)
    exe = tmp_path / "pixel_transform_host"
    cmd = [cxx, "-std=c++17", "-O1", "-g", '-DKERNEL_TEXT="%s"' % inc, os.path.join(ROOT, "tests", "pixel_transform_host.cpp"), "-o", str(exe)]
    # (statically linked sanitizer runtimes where the toolchain has them: the program then runs in whatever environment the suite runs in)
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("errors: 0"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "runs: 6291456" in r.stdout
