"""What the test modules share, one copy of each: the module fixtures (built, po, gpu), the reading of a header and of a shared
object's symbols, the upload and the tile offsets of a mixed batch, the checker's rearrangement of a raster into a layout, its
float table and constants, the sentinel arena the GPU tests write into, and the build-and-run of the host-run kernel programs
(tests/*_host.cpp with tests/kernel_host.hpp).  Imported like tests/_resize.py and tests/_quant.py; a fixture is imported by name
into the module that uses it."""
import ctypes as C
import ctypes.util
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32 = 1, 2, 3                                          # include/xpng_hip.h XPNGHIP_DTYPE_*
DTYPES = [F16, BF16, F32]
ES = {F16: 2, BF16: 2, F32: 4}
BITS = {F16: np.uint16, BF16: np.uint16, F32: np.uint32}
FORMATS = [(1, False), (2, False), (1, True)]                     # (tile mode, alpha)
SENTINEL = 0xA5
LEAD, GUARD = 64, 256                                             # an arena's buffer i starts LEAD + a phase into its region; GUARD bytes behind it
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
libm.fmaf.restype = C.c_float
libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


# ---- fixtures ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def built():
    api.build_native(("hip", "host"))


@pytest.fixture(scope="module", autouse=True)
def built_with_probes():
    api.build_native(("hip", "probes", "host"))


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def gpu():
    import torch
    import xpng_amd
    if not torch.cuda.is_available() or xpng_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the product has no CPU fallback")
    return xpng_amd


# ---- headers, symbols, bytes ------------------------------------------------------------------------------------------
def declared(header, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"\w*)\s*\(", txt)))


def exported(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def md5(b):
    return hashlib.md5(b).hexdigest()


# ---- a mixed batch on the device --------------------------------------------------------------------------------------
def _upload(blobs):
    import torch
    return [torch.from_numpy(np.frombuffer(b + b"\0" * 64, dtype=np.uint8).copy()).cuda() for b in blobs]


def _offsets(blobs, ctx):
    offs = []
    for i, b in enumerate(blobs):
        off, end = api.walk_tile_offsets(b, ctx.first_tile[i + 1] - ctx.first_tile[i])
        assert end == len(b)
        offs.append(off)
    return offs


def _torch_dtype(dtype):
    import torch
    return {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}[dtype]


def _bits(t, dtype):
    """a torch tensor of a float dtype as the numpy array of its bit patterns"""
    import torch
    t = t.cpu().contiguous()
    return t.view(torch.int16 if ES[dtype] == 2 else torch.int32).numpy().view(BITS[dtype])


class Arena:
    """one sentinel-filled device tensor holding a region per image: LEAD + es * (i % phases) sentinel bytes (with 8 phases the
    buffers start at every multiple of the element size modulo 16), room for `sizes[i]` bytes - holding fill[i] where a fill is
    given - and GUARD sentinel bytes"""

    def __init__(self, sizes, es=1, phases=8, fill=None):
        import torch
        self.sizes, self.off, total = sizes, [], 0
        for i, n in enumerate(sizes):
            self.off.append(total + LEAD + es * (i % phases))
            total += -(-(LEAD + phases * es + n + GUARD) // 16) * 16
        self.host0 = np.full(total, SENTINEL, np.uint8)
        if fill is not None:
            for o, n, data in zip(self.off, sizes, fill):
                self.host0[o:o + n] = np.frombuffer(data, np.uint8) if isinstance(data, bytes) else data.reshape(-1)
        self.t = torch.from_numpy(self.host0.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptrs = [self.t.data_ptr() + o for o in self.off]

    def refill(self):
        self.t.fill_(SENTINEL)

    def fetch(self, sizes=None):
        """the first sizes[i] bytes of every image (all of them by default), after checking that every other byte still holds the
        sentinel"""
        import torch
        torch.cuda.synchronize()
        got = self.t.cpu().numpy()
        sizes = sizes or self.sizes
        mask = np.ones(got.size, bool)
        for o, n in zip(self.off, sizes):
            mask[o:o + n] = False
        assert (got[mask] == SENTINEL).all(), "a byte before or behind an image was written"
        return [got[o:o + n] for o, n in zip(self.off, sizes)]

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(self.t.cpu().numpy(), self.host0)


# ---- the checker of the layouts and of the float call -----------------------------------------------------------------
def arrange(r, planar, bgr, ch):
    """(h, w, 3|4) in the file's form -> the bytes of a buffer of that layout: the checker's rearrangement"""
    px = r.shape[2]
    if ch == 4 and px == 3:
        r = np.concatenate([r, np.full(r.shape[:2] + (1,), 255, np.uint8)], axis=2)
    elif ch == 3 and px == 4:
        r = r[..., :3]
    if bgr:
        r = r[..., [2, 1, 0] + ([3] if r.shape[2] == 4 else [])]
    return np.ascontiguousarray(r.transpose(2, 0, 1) if planar else r)


def f32_of(x):
    """a Python double rounded once to fp32 (and back to a Python float)"""
    return float(np.float32(x))


def consts_from(mean, std):
    """load_files' formula: scale = float32(1 / (255 std)), bias = float32(-mean / std), in Python doubles rounded once"""
    return [f32_of(1.0 / (255.0 * s)) for s in std], [f32_of(-m / s) for m, s in zip(mean, std)]


def probes(dtype):
    """two scales whose products with v = 1 and v = 2 are exact ties of the narrow type, one rounding down to even, one up"""
    return (257.0 / 256.0, 259.0 / 256.0) if dtype == BF16 else (2049.0 / 2048.0, 2051.0 / 2048.0)


def mixed_consts(dtype):
    """four different (scale, bias) pairs, one per channel position: ImageNet's on 0 and 2, the rounding probes on 1 and 3"""
    s, b = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    p = probes(dtype)
    return [s[0], p[0], s[2], p[1]], [b[0], 0.0, b[2], 0.0]


def table(dtype, scale, bias):
    """(C, 256) bit patterns of the expected elements: libm's fmaf, then numpy's / torch's round-to-nearest-even narrowing"""
    import torch
    y = np.array([[libm.fmaf(float(v), s, b) for v in range(256)] for s, b in zip(scale, bias)], dtype=np.float32)
    if dtype == F32:
        return y.view(np.uint32)
    if dtype == F16:
        with np.errstate(over="ignore"):
            return y.astype(np.float16).view(np.uint16)
    return torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def expect(r, planar, bgr, ch, tab):
    """the bit patterns of the float buffer of raster r: tab[c][byte] at every element"""
    a = arrange(r, planar, bgr, ch)
    out = np.empty(a.shape, tab.dtype)
    for c in range(ch):
        if planar:
            out[c] = tab[c][a[c]]
        else:
            out[..., c] = tab[c][a[..., c]]
    return out


# ---- kernels run on the host ------------------------------------------------------------------------------------------
def cut(header, start, end="}  // namespace xpng", last=True):
    """the text of xpng_amd/csrc/<header> from the first `start` up to the last (or, last=False, the next) `end`"""
    src = open(os.path.join(ROOT, "xpng_amd", "csrc", header)).read()
    a = src.index(start)
    return src[a:src.rindex(end) if last else src.index(end, a)]


def product_types(*names):
    """the product's own declarations that the host programs name, as text cut out of its headers: 'layout' = MixedLayout and
    MC_ROWS (mixed.hpp), 'dw' = Dw4 and Dw3, 'float' = FloatConsts, the element types and pick4 (mixed_float.hpp)"""
    parts = {
        "layout": lambda: cut("mixed.hpp", "struct MixedLayout {", "// grid (", last=False),
        "dw": lambda: cut("mixed.hpp", "struct __attribute__((aligned(4))) Dw4 {", "};", last=False) + "};\n" +
        cut("mixed_float.hpp", "struct __attribute__((aligned(4))) Dw3 {", "};", last=False) + "};\n",
        "float": lambda: cut("mixed_float.hpp", "struct FloatConsts {", "// byte i of x as a float", last=False),
    }
    text = "\n".join(parts[n]() for n in names)
    assert "asm" not in text and "address_space" not in text
    return text


def run_kernels_on_host(tmp_path, program, segments, flags=(), sanitize=("-fsanitize=address", "-static-libasan"), timeout=300):
    """Compile tests/<program>.cpp with every text of `segments` ({macro: text}) written to a file that the macro names, run it and
    check that it ends with `errors: 0`.  Returns the finished process."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler for the host run of " + program)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", *flags]
    for macro, text in segments.items():
        inc = tmp_path / (macro.lower() + ".inc")
        inc.write_text(text)
        cmd.append('-D%s="%s"' % (macro, inc))
    exe = tmp_path / program
    cmd += [os.path.join(ROOT, "tests", program + ".cpp"), "-o", str(exe)]
    # the sanitizer's runtime is linked statically, so the program runs in whatever environment the suite runs in; where the
    # toolchain has no static runtime the program is built plain and its own range checks and sentinels are what is checked
    if subprocess.run(cmd + list(sanitize), capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("errors: 0"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r
