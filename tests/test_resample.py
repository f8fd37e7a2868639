"""Antialiased downscale in the resized copy-out of a mixed-size decode (include/xpng_hip.h
xpnghip_decode_varsize_device_batch_resampled, xpnghip_resample_host, XPNGHIP_FILTER_*; xpng_amd/tensors.py load_files antialias;
DESIGN.md 19).

The checker is tests/_resample.py: the rule in numpy with the C library's fmaf, independent of the code under test.  Every
comparison with the library is on the bits.
CPU: the symbols; xpnghip_resample_host with filter 1 against the checker for every layout word x dtype on RGB and RGBA rasters, and
with filter 0 against xpnghip_resize_host; the three consequences of the rule (no ratio above 1: filter 0's bits; the flip mirror;
no tap outside the rectangle); a rectangle that shrinks in one direction and grows in the other; the rule against torch's
F.interpolate(antialias=True); refusals; load_files(size=..., antialias=True) on the host-answered kinds.
GPU (-m gpu): filter 1 into every layout word x dtype x format on batches with the edge rectangles, inside sentinel-filled buffers;
filter 0 against decode_batch_resized; filter 1 against filter 0 where no axis shrinks; the device call against api.resample_host;
NULL rects / flips, both size walks, rectangles that change between two calls on one pointer array, the workspace, a rejected tile,
misuse; load_files(size=..., antialias=True, stack=True) on reference-written goldens."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _kit import (BF16, BITS, DTYPES, ES, F16, F32, FORMATS, IMAGENET_MEAN, IMAGENET_STD, Arena, _bits, _offsets, _torch_dtype, _upload,
                  built, consts_from, f32_of, gpu, mixed_consts, po)
from _resample import Resampled
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_decode_varsize_device_batch_resampled", "xpnghip_resample_host"]
WORDS = [api.layout(planar=p, bgr=b, channels=c) for c in (0, 3, 4) for p in (False, True) for b in (False, True)]
AA = api.FILTER_TRIANGLE_AA
GPU_SIZES = [(3, 5), (37, 29)]                                    # (OW, OH): rows narrower than one 16-byte store; an odd width
# one rectangle per image: the whole image, 1 x 1 at the last pixel, the last column, a whole image that shrinks, the last row, an
# upscale (smaller than either output), the mixed-branch 9 x 200 across the 444-px tile boundary of the 889-wide image, a downscale
# across that boundary, the strong downscale 90 x 1000 and a rectangle strictly inside its image
RGB_DIMS = [(3, 3), (17, 4), (17, 4), (64, 64), (64, 64), (445, 444), (889, 445), (889, 445), (100, 1100), (100, 1100)]
RGB_RECTS = [(0, 0, 3, 3), (16, 3, 1, 1), (16, 0, 1, 4), (0, 0, 64, 64), (0, 63, 64, 1), (10, 20, 2, 3), (440, 100, 9, 200),
             (400, 50, 80, 300), (3, 50, 90, 1000), (20, 30, 60, 500)]
RGBA_DIMS = [(4, 4), (17, 4), (64, 64), (64, 64), (445, 444), (889, 445), (889, 445), (100, 1100)]
RGBA_RECTS = [(0, 0, 4, 4), (16, 3, 1, 1), (63, 0, 1, 64), (0, 63, 64, 1), (430, 431, 2, 4), (440, 0, 9, 200), (400, 50, 80, 300),
              (3, 50, 90, 1000)]


def _lib(r, rect, flip, OW, OH, word, dtype, scale, bias, filter=AA):
    ch = (word >> 8) or r.shape[2]
    raw = api.resample_host(r, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip, filter=filter)
    shape = (ch, OH, OW) if word & 1 else (OH, OW, ch)
    return np.frombuffer(raw, BITS[dtype]).reshape(shape)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_resample_symbols_are_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xpng_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(xpnghip_\w*)\s*\(", txt))
    assert set(NEW) <= names and set(NEW) <= set(api.HIP_SYMBOLS)
    assert re.search(r"#define\s+XPNGHIP_FILTER_BILINEAR\s+0u?\b", txt) and re.search(r"#define\s+XPNGHIP_FILTER_TRIANGLE_AA\s+1u?\b", txt)
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.HIP_SO], text=True)
    assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    import xpng_amd
    for name in ("resample_host", "FILTER_BILINEAR", "FILTER_TRIANGLE_AA"):
        assert name in xpng_amd.__all__ and hasattr(xpng_amd, name)
    assert (api.FILTER_BILINEAR, api.FILTER_TRIANGLE_AA) == (0, 1)
    assert hasattr(api.MixedContext, "decode_batch_resampled")
    assert api.hip_lib().xpnghip_abi_version() == 2


HOST_RASTERS = [(1, 1), (2, 1), (1, 2), (3, 3), (17, 4), (45, 31), (130, 9)]
HOST_SIZES = [(1, 1), (3, 5), (8, 8), (37, 29)]                   # (OW, OH)


def _host_rects(w, h, OW, OH):
    rects = [None, (w - 1, h - 1, 1, 1), (w - 1, 0, 1, h)]       # whole, 1 x 1 at the last pixel, the rightmost column
    if w >= OW and h >= OH:
        rects.append((w - OW, h - OH, OW, OH))                    # of the output's size
    if w >= 5 and h >= 5:
        rects.append((2, 2, w - 4, h - 4))                        # strictly inside: 2 px of other pixels on every side
    return rects


@pytest.mark.parametrize("px", [3, 4])
def test_resample_host_equals_the_checker(px):
    """Filter 1: every layout word x dtype, four different (scale, bias) pairs, on the bits - a tap outside the rectangle would show
    on the rectangles strictly inside their raster (consequence c).  With it filter 0 against xpnghip_resize_host, the mirror
    (consequence b) and, wherever both ratios are <= 1, filter 1 against filter 0 (consequence a)."""
    rng = np.random.default_rng(200 + px)
    inside = same = 0
    for (w, h) in HOST_RASTERS:
        r = rng.integers(0, 256, (h, w, px), dtype=np.uint8)
        for (OW, OH) in HOST_SIZES:
            for rect in _host_rects(w, h, OW, OH):
                want = [Resampled(r, rect, flip, OH, OW) for flip in (False, True)]
                rw, rh = rect[2:] if rect else (w, h)
                inside += rect is not None and rect[:2] == (2, 2)
                for dtype in DTYPES:
                    scale, bias = mixed_consts(dtype)
                    for word in WORDS:
                        ch = (word >> 8) or px
                        got = [_lib(r, rect, flip, OW, OH, word, dtype, scale, bias) for flip in (False, True)]
                        for flip in (0, 1):
                            exp = want[flip].bits(word, dtype, scale, bias)
                            assert got[flip].shape == exp.shape and np.array_equal(got[flip], exp), \
                                (px, (w, h), (OW, OH), rect, flip, dtype, hex(word), np.argwhere(got[flip] != exp)[:4])
                        ax = 2 if word & 1 else 1
                        assert np.array_equal(got[1], np.flip(got[0], axis=ax)), ("mirror", (w, h), (OW, OH), rect, dtype, hex(word))
                        old = np.frombuffer(api.resize_host(r, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=True), BITS[dtype])
                        zero = _lib(r, rect, True, OW, OH, word, dtype, scale, bias, filter=api.FILTER_BILINEAR)
                        assert np.array_equal(zero.reshape(-1), old), ("filter 0", (w, h), (OW, OH), rect, dtype, hex(word))
                        if rw <= OW and rh <= OH:
                            assert np.array_equal(got[1], zero), ("no ratio above 1", (w, h), (OW, OH), rect, dtype, hex(word))
                            same += 1
                        elif rw > 2 * OW and rh > 2 * OH and w > 3:
                            assert not np.array_equal(got[1], zero)   # (random bytes: the filters do differ where both axes shrink)
    assert inside >= 8 and same >= 36 * 20


def test_mixed_branches():
    """A 9 x 200 rectangle to 37 x 29: x grows (two taps), y shrinks (the triangle); and its transpose."""
    rng = np.random.default_rng(9)
    for (w, h, rect, OW, OH) in [(13, 204, (2, 2, 9, 200), 37, 29), (204, 13, (2, 2, 200, 9), 29, 37)]:
        r = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        for flip in (False, True):
            z = Resampled(r, rect, flip, OH, OW)
            for dtype in DTYPES:
                scale, bias = mixed_consts(dtype)
                for word in WORDS:
                    got = _lib(r, rect, flip, OW, OH, word, dtype, scale, bias)
                    assert np.array_equal(got, z.bits(word, dtype, scale, bias)), ((w, h), flip, dtype, hex(word))
            zero = _lib(r, rect, flip, OW, OH, 0, F32, *mixed_consts(F32), filter=api.FILTER_BILINEAR)
            assert not np.array_equal(zero, _lib(r, rect, flip, OW, OH, 0, F32, *mixed_consts(F32)))


TORCH_SHAPES = [(7, 9, 3, 5), (17, 33, 4, 7), (64, 64, 5, 5), (100, 37, 37, 29), (445, 300, 3, 5), (33, 65, 32, 64), (50, 50, 50, 20),
                (20, 50, 40, 7), (2, 1000, 1, 3), (129, 131, 7, 128)]    # (h, w, OH, OW)


def test_rule_against_torch_interpolate_antialias():
    """The checker (f32, scale 1, bias 0) against torch's CPU F.interpolate(bilinear, align_corners=False, antialias=True) of the
    cropped fp32 raster.  torch normalises the weights of a window first and sums weighted taps, the rule divides the weighted sum
    by the sum of the weights at the end, so the two differ in the last bits: with this checker the largest difference over these
    shapes was 1.22e-4 in byte units (2^-13, on 2 x 1000 -> 1 x 3: up to 667 taps in a row).  The bound is 2^-10: 8x that,
    rounded up to a power of two, for another vector path of another torch build (the margin of test_rule_against_torch_interpolate);
    a wrong window, weight or half-pixel convention is off by whole grey levels on random bytes."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(7)
    worst = 0.0
    for (h, w, OH, OW) in TORCH_SHAPES:
        r = rng.integers(0, 256, (h + 3, w + 2, 3), dtype=np.uint8)
        rect = (2, 1, w, h)
        v = Resampled(r, rect, False, OH, OW).v
        crop = torch.from_numpy(r[1:1 + h, 2:2 + w].astype(np.float32)).permute(2, 0, 1)[None]
        t = F.interpolate(crop, size=(OH, OW), mode="bilinear", align_corners=False, antialias=True)[0].permute(1, 2, 0).numpy()
        d = float(np.abs(t.astype(np.float64) - v.astype(np.float64)).max())
        print("rule vs torch antialias", (h, w, OH, OW), d)
        worst = max(worst, d)
        assert d <= 2.0 ** -10, ((h, w, OH, OW), d)
    print("rule vs torch antialias, worst", worst)


def test_resample_host_refusals():
    lib = api.hip_lib()
    r = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    out = np.full(4 * 4 * 4 * 4 + 4, 0x5A5A5A5A, np.uint32)
    one, zero = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0)
    u64 = C.c_uint64

    def call(pxsz=3, raster=r.ctypes.data, w=7, h=5, rect=None, flip=0, ow=4, oh=4, layout=0, dtype=F32, scale=one, bias=zero, filter=AA, o=None):
        ra = None if rect is None else (u64 * 4)(*rect)
        return lib.xpnghip_resample_host(pxsz, raster, w, h, ra, flip, ow, oh, layout, dtype, scale, bias, filter, out.ctypes.data if o is None else o)

    def refused(words, **kw):
        for f in ([AA, api.FILTER_BILINEAR] if "filter" not in kw else [kw.pop("filter")]):
            assert call(filter=f, **kw) != 0, kw
            assert all(w in api._err() for w in words), (words, api._err())

    assert call() == 0
    out[:] = 0x5A5A5A5A
    refused(["filter 2", "XPNGHIP_FILTER_TRIANGLE_AA"], filter=2)
    refused(["filter 4294967295"], filter=0xFFFFFFFF)
    refused(["{0, 0, 0, 3}", "7 x 5"], rect=(0, 0, 0, 3))           # zero size
    refused(["{2, 0, 6, 1}", "7 x 5"], rect=(2, 0, 6, 1))           # x + w > W
    refused(["{0, 5, 1, 1}"], rect=(0, 5, 1, 1))
    refused(["4 x 0", "16384"], oh=0)
    refused(["0 x 4"], ow=0)
    refused(["16385 x 4"], ow=16385)
    refused(["4 x 16385"], oh=16385)
    refused(["flip 2"], flip=2)
    refused(["dtype 0"], dtype=0)
    refused(["dtype 4"], dtype=4)
    refused(["layout", "0x4"], layout=0x004)
    refused(["layout", "0x500"], layout=0x500)
    refused(["scale[1]", "nan"], scale=(C.c_float * 4)(1, float("nan"), 1, 1))
    refused(["bias[2]", "inf"], bias=(C.c_float * 4)(0, 0, float("inf"), 0))
    refused(["null"], raster=None)
    refused(["null"], o=0)
    refused(["aligned", "%x" % (out.ctypes.data + 2)], o=out.ctypes.data + 2)          # f32 at 2 mod 4
    refused(["aligned"], o=out.ctypes.data + 1, dtype=F16)
    refused(["pxsz is 5"], pxsz=5)
    refused(["0 x 5"], w=0)
    assert (out == 0x5A5A5A5A).all()                                # a refused call writes nothing
    assert call(o=out.ctypes.data + 2, dtype=BF16) == 0             # (2 mod 4 is fine for a 2-byte element)
    with pytest.raises(api.XpngError) as e:
        api.resample_host(r, (4, 4), 0, F32, rect=(0, 0, 8, 1))
    assert "{0, 0, 8, 1}" in str(e.value)
    with pytest.raises(api.XpngError) as e:
        api.resample_host(r, (4, 4), 0, F32, filter=3)
    assert "filter 3" in str(e.value)
    # the device entry point refuses a NULL context like its siblings
    p1, n1 = (C.c_void_p * 1)(0), (u64 * 1)(0)
    assert lib.xpnghip_decode_varsize_device_batch_resampled(None, 1, p1, n1, 1, None, p1, 0, F16, None, None, None, None, 4, 4, AA, None) != 0
    assert "null context" in api._err()


def _host_files(po, tmp_path):
    """two oracle-written level-7 files and the committed 11-byte single-colour golden, with the oracle's decode of each"""
    from xpng_amd.synth import synth_raster
    paths = []
    for (w, h, alpha) in [(25, 37, False), (39, 16, True)]:
        p = tmp_path / f"l7_{w}x{h}_{int(alpha)}.xpng"
        p.write_bytes(po.encode_image(7, synth_raster("noise" if alpha else "photo", w, h, alpha, seed=w)))
        paths.append(str(p))
    single = os.path.join(GOLD, "imgfull_30d5c8.L2.xpng")
    assert os.path.getsize(single) == 11
    paths.insert(1, single)
    return paths, [po.decode_image(open(p, "rb").read()) for p in paths]


def test_load_files_antialias_answers_host_kinds_without_a_gpu(po, tmp_path):
    import torch
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    assert [r.shape for r in want] == [(37, 25, 3), (1000, 1000, 3), (16, 39, 4)]
    crops, flips = [(1, 2, 23, 34), (100, 200, 300, 150), (2, 0, 37, 5)], [True, False, True]     # the last one shrinks in x and grows in y
    mean, std = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)
    OH, OW = 6, 5
    zs = [Resampled(r, c, f, OH, OW) for r, c, f in zip(want, crops, flips)]
    for dtype in DTYPES:
        for ch in (3, 4):
            scale, bias = consts_from(mean[:ch], std[:ch])
            for lay, bgr in (("chw", False), ("hwc", True)):
                word = api.layout(planar=lay == "chw", bgr=bgr, channels=ch)
                kw = dict(layout=lay, channels=ch, bgr=bgr, device="cpu", dtype=_torch_dtype(dtype), mean=mean[:ch], std=std[:ch],
                          size=(OH, OW), crops=crops, flips=flips)
                got = tensors.load_files(paths, antialias=True, **kw)
                whole = tensors.load_files(paths, stack=True, antialias=True, **kw)
                plain = tensors.load_files(paths, **kw)
                assert isinstance(got, list) and len(got) == 3 and isinstance(whole, torch.Tensor) and whole.is_contiguous()
                assert tuple(whole.shape) == (3,) + ((ch, OH, OW) if lay == "chw" else (OH, OW, ch)) and whole.dtype == _torch_dtype(dtype)
                for i, (g, z) in enumerate(zip(got, zs)):
                    exp = z.bits(word, dtype, scale, bias)
                    assert g.device.type == "cpu" and g.is_contiguous() and tuple(g.shape) == exp.shape
                    assert np.array_equal(_bits(g, dtype), exp), (dtype, ch, lay, bgr, i)
                    assert np.array_equal(_bits(whole[i], dtype), exp), ("stack", dtype, ch, lay, bgr, i)
                # antialias=False is today's path: the resized call's bits, and they differ on the two patterned files
                for i in (0, 2):
                    raw = api.resize_host(want[i], (OH, OW), word, dtype, scale, bias, rect=crops[i], flip=flips[i])
                    assert np.array_equal(_bits(plain[i], dtype).reshape(-1), np.frombuffer(raw, BITS[dtype]))
                    assert not np.array_equal(_bits(plain[i], dtype), _bits(got[i], dtype))
    # channels None keeps each file's own count; no crops and no flips: every whole image
    got = tensors.load_files(paths[::2], device="cpu", dtype=torch.float32, size=(4, 3), antialias=True)
    for g, r in zip(got, want[::2]):
        px = r.shape[2]
        exp = Resampled(r, None, False, 4, 3).bits(api.layout(planar=True), F32, [f32_of(1 / 255.0)] * px, [0.0] * px)
        assert tuple(g.shape) == (px, 4, 3) and np.array_equal(_bits(g, F32), exp)
    # misuse
    for bad in (dict(antialias=True),                                                      # without size
                dict(antialias=True, dtype=torch.float16),
                dict(antialias=True, crops=crops), dict(antialias=True, size=(4, 4)),      # uint8
                dict(antialias=True, dtype=torch.float16, size=(0, 4)),
                dict(antialias=True, dtype=torch.float16, size=(4, 4), crops=[(0, 0, 26, 1), None, None]),     # leaves the 25 x 37 image
                dict(antialias=True, dtype=torch.float16, size=(4, 4), stack=True)):                            # channels None: 3 and 4 do not stack
        with pytest.raises(api.XpngError):
            tensors.load_files(paths, device="cpu", **bad)
    with pytest.raises(api.XpngError) as e:
        tensors.load_files(paths, device="cpu", dtype=torch.float16, antialias=True)
    assert "antialias" in str(e.value) and "size" in str(e.value)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches(po):
    """per (mode, alpha): dims, rectangles, the rasters and the oracle's tile blobs - computed once, never changed"""
    from xpng_amd.synth import synth_raster
    kinds = ["photo", "noise", "gray", "flat"]
    out = {}
    for mode, alpha in FORMATS:
        dims, rects = (RGBA_DIMS, RGBA_RECTS) if alpha else (RGB_DIMS, RGB_RECTS)
        assert len(dims) == len(rects) and all(x + w <= W and y + h <= H for (W, H), (x, y, w, h) in zip(dims, rects))
        rasters = [synth_raster(kinds[(i + 1) % 4], w, h, alpha, seed=i + 1) for i, (w, h) in enumerate(dims)]
        blobs = [po.encode_tiles(mode, r) for r in rasters]
        out[(mode, alpha)] = (dims, rects, rasters, blobs)
    return out


_CHECK = {}


def checked(key, i, raster, rect, flip, OW, OH):
    """the checker's v for (image, rectangle, flip, size), computed once for all layout words and dtypes"""
    k = (key, i, rect, bool(flip), OW, OH)
    if k not in _CHECK:
        _CHECK[k] = Resampled(raster, rect, bool(flip), OH, OW)
    return _CHECK[k]


def _decode(ctx, mode, d_b, lens, word, dtype, size, scale, bias, rects, flips, filter=AA, offs=None, expect_status=0, arena=None):
    """the images' elements as bit patterns, flat; size = (OW, OH); filter None: the resized call"""
    ch = api.layout_channels(word, ctx.pxsz)
    ar = arena or Arena([ES[dtype] * ch * size[0] * size[1]] * ctx.nimg, ES[dtype])
    args = (mode, [t.data_ptr() for t in d_b], lens, ar.ptrs, word, dtype, (size[1], size[0]), scale and scale[:ch], bias and bias[:ch])
    if filter is None:
        ctx.decode_batch_resized(*args, rects=rects, flips=flips, tile_offs=offs)
    else:
        ctx.decode_batch_resampled(*args, rects=rects, flips=flips, filter=filter, tile_offs=offs)
    assert ctx.decode_status() == expect_status
    return [g.view(BITS[dtype]) for g in ar.fetch()]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_decode_resampled_into_every_layout(gpu, batches, mode, alpha, dtype):
    """Filter 1: all 12 layout words x both output sizes, four different (scale, bias) pairs, the edge rectangles, alternating
    flips, every output at LEAD + es * (i % 8) inside a sentinel-filled region: the checker's bits and intact sentinels.  Then, on
    the same context, filter 0 against decode_batch_resized and the device call against api.resample_host of the rasters."""
    dims, rects, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    flips = [i % 2 for i in range(len(dims))]
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for (OW, OH) in GPU_SIZES:
            for word in WORDS:
                got = _decode(ctx, mode, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips)
                for i, (g, r) in enumerate(zip(got, rasters)):
                    w = checked((mode, alpha), i, r, rects[i], flips[i], OW, OH).bits(word, dtype, scale, bias).reshape(-1)
                    assert np.array_equal(g, w), (hex(word), dtype, (OW, OH), i, dims[i], rects[i], np.argwhere(g != w)[:4].ravel())
        OW, OH = GPU_SIZES[1]
        for word in (api.layout(planar=True, bgr=True, channels=7 - px), api.layout(channels=px)):
            ch = api.layout_channels(word, px)
            zero = _decode(ctx, mode, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips, filter=api.FILTER_BILINEAR)
            old = _decode(ctx, mode, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips, filter=None)
            one = _decode(ctx, mode, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips)
            for i, r in enumerate(rasters):
                assert np.array_equal(zero[i], old[i]), ("filter 0", hex(word), dtype, i)
                host = api.resample_host(r, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rects[i], flip=flips[i])
                assert np.array_equal(one[i], np.frombuffer(host, BITS[dtype])), ("host twin", hex(word), dtype, i)
            assert any(not np.array_equal(a, b) for a, b in zip(zero, one))
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [False, True])
def test_filter_1_is_filter_0_where_no_axis_shrinks(gpu, batches, alpha):
    """Rectangles no larger than the output in either direction (the identity crop among them, one across the tile boundary):
    filter 1 gives bit for bit what filter 0 gives, which is what decode_batch_resized gives."""
    dims, _, rasters, blobs = batches[(1, alpha)]
    px = 4 if alpha else 3
    OW, OH = GPU_SIZES[1]
    sizes = [(min(w, OW - (i // 2) % 3), min(h, OH - i % 3)) for i, (w, h) in enumerate(dims)]
    rects = [((w - rw) // 2, (h - rh) // 3, rw, rh) for (w, h), (rw, rh) in zip(dims, sizes)]
    assert all(rw <= OW and rh <= OH for (_, _, rw, rh) in rects) and any(r[2:] == (OW, OH) for r in rects)
    k = len(dims) - 1 - dims[::-1].index((889, 445))
    assert rects[k][0] < 444 < rects[k][0] + rects[k][2]          # across the tile boundary
    flips = [(i // 2) % 2 for i in range(len(dims))]
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for dtype in DTYPES:
            scale, bias = mixed_consts(dtype)
            for word in WORDS:
                one = _decode(ctx, 1, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips)
                zero = _decode(ctx, 1, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips, filter=api.FILTER_BILINEAR)
                old = _decode(ctx, 1, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips, filter=None)
                for i in range(len(dims)):
                    assert np.array_equal(one[i], zero[i]) and np.array_equal(zero[i], old[i]), (hex(word), dtype, i, dims[i], rects[i])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_null_rects_size_walks_changing_rectangles_and_the_workspace(gpu, po):
    """One pointer array, four calls: rectangles, then none (every whole image, no flip), then the first again with the host's
    size walk, then other rectangles.  The workspace grows by the 48-byte record table of filter 1 and by nothing else."""
    from xpng_amd.synth import synth_raster
    dims = [(17, 4), (64, 64), (130, 90), (100, 110), (5, 7)]
    rasters = [synth_raster(["photo", "noise", "gray"][i % 3], w, h, False, seed=i + 40) for i, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(1, r) for r in rasters]
    r1 = [(0, 0, 17, 4), (3, 4, 50, 55), (10, 10, 110, 70), (0, 0, 100, 110), (1, 2, 3, 4)]
    r2 = [(1, 1, 15, 2), (0, 0, 64, 64), (100, 0, 30, 90), (40, 50, 60, 60), (0, 0, 5, 7)]
    flips = [1, 0, 1, 0, 1]
    OW, OH = 21, 13
    dtype, word = F16, api.layout(planar=True, bgr=True, channels=4)
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(dims, 3)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        full = Arena([2 * 4 * w * h for (w, h) in dims], 2)
        ctx.decode_batch_as_float(1, [t.data_ptr() for t in d_b], lens, full.ptrs, word, dtype, scale, bias)
        assert ctx.decode_status() == 0
        ws = ctx.workspace_bytes()
        ar = Arena([2 * 4 * OW * OH] * len(dims), 2)
        a = _decode(ctx, 1, d_b, lens, word, dtype, (OW, OH), scale, bias, r1, flips, arena=ar)
        assert ctx.workspace_bytes() - ws == 48 * len(dims)        # the record table, once; no second staging raster
        ar.refill()
        b = _decode(ctx, 1, d_b, lens, word, dtype, (OW, OH), scale, bias, None, None, arena=ar)
        ar.refill()
        c = _decode(ctx, 1, d_b, lens, word, dtype, (OW, OH), scale, bias, r1, flips, offs=_offsets(blobs, ctx), arena=ar)
        ar.refill()
        d = _decode(ctx, 1, d_b, lens, word, dtype, (OW, OH), scale, bias, r2, flips, arena=ar)
        assert ctx.workspace_bytes() - ws == 48 * len(dims)
        for i, r in enumerate(rasters):
            wa = Resampled(r, r1[i], flips[i], OH, OW).bits(word, dtype, scale, bias).reshape(-1)
            wb = Resampled(r, None, False, OH, OW).bits(word, dtype, scale, bias).reshape(-1)
            wd = Resampled(r, r2[i], flips[i], OH, OW).bits(word, dtype, scale, bias).reshape(-1)
            assert np.array_equal(a[i], wa) and np.array_equal(b[i], wb) and np.array_equal(c[i], wa) and np.array_equal(d[i], wd), i
        assert any(not np.array_equal(x, y) for x, y in zip(a, b)) and any(not np.array_equal(x, y) for x, y in zip(a, d))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_rejected_tile_and_misuse_of_the_resampled_call(gpu, po):
    """One tile of one image gets type byte 0x7F: the launch reports 1, every element with no tap inside that tile is exact, and
    so is every other image.  Misuse is refused before device work: the error names the value and no byte of the arena changes."""
    from xpng_amd.synth import synth_raster
    dims = [(300, 200), (889, 445), (100, 100), (64, 70)]
    rasters = [synth_raster("photo", w, h, True, seed=s + 1) for s, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(1, r) for r in rasters]
    scale, bias = mixed_consts(F16)
    OW, OH = GPU_SIZES[1]
    rects, flips = [(0, 0, 300, 200), (400, 100, 80, 300), (50, 50, 50, 50), (0, 0, 64, 70)], [0, 1, 0, 1]
    word = api.layout(planar=True, channels=3)
    ctx = gpu.MixedContext(dims, 4)
    try:
        k = 1
        offs = _offsets(blobs, ctx)
        tx, ty, tw, th = ctx.tile(ctx.first_tile[k] + 1)           # the image's second tile: the right half of its top row
        assert tx >= 440 and ty == 0 and tx < 480 < tx + tw
        bad = bytearray(blobs[k])
        bad[offs[k][1] + 3] = 0x7F                                 # top byte of the tile's first little-endian word
        bb = blobs[:k] + [bytes(bad)] + blobs[k + 1:]
        got = _decode(ctx, 1, _upload(bb), [len(b) for b in bb], word, F16, (OW, OH), scale, bias, rects, flips, expect_status=1)
        clean = 0
        for i, (g, r) in enumerate(zip(got, rasters)):
            z = Resampled(r, rects[i], flips[i], OH, OW)
            w = z.bits(word, F16, scale, bias)
            g = g.reshape(w.shape)
            if i == k:
                xa, xb, ya, yb = z.span                             # relative to the rectangle, inclusive
                hitx = (rects[i][0] + xb >= tx) & (rects[i][0] + xa < tx + tw)
                hity = (rects[i][1] + yb >= ty) & (rects[i][1] + ya < ty + th)
                hit = hity[:, None] & hitx[None, :]
                assert hit.any() and not hit.all()
                clean = int((~hit).sum())
                assert np.array_equal(g[:, ~hit], w[:, ~hit])
            else:
                assert np.array_equal(g, w), i
        assert clean > 100
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        outs = Arena([4 * 4 * OW * OH] * 4, 4)

        def refused(words, **kw):
            a = dict(mode=1, d_blobs=ins, lens=lens, d_outs=outs.ptrs, layout=word, dtype=F16, size=(OH, OW), rects=rects, flips=flips, filter=AA)
            a.update(kw)
            with pytest.raises(gpu.XpngError) as e:
                ctx.decode_batch_resampled(**a)
            assert all(w in str(e.value) for w in words), (words, str(e.value))
            assert outs.untouched(), words

        refused(["filter 2", "XPNGHIP_FILTER_TRIANGLE_AA"], filter=2)
        refused(["filter 255"], filter=255)
        refused(["{0, 0, 0, 5}", "image 2", "100 x 100"], rects=rects[:2] + [(0, 0, 0, 5)] + rects[3:])
        refused(["{60, 0, 5, 5}", "image 3", "64 x 70"], rects=rects[:3] + [(60, 0, 5, 5)])
        refused(["37 x 0"], size=(0, OW))
        refused(["16385 x 29"], size=(OH, 16385))
        refused(["flip 2", "image 1"], flips=[0, 2, 0, 1])
        refused(["dtype 0"], dtype=0)
        refused(["layout", "0x500"], layout=0x500)
        refused(["scale[1]", "nan"], scale=[1.0, float("nan"), 1.0])
        refused(["null"], d_outs=[outs.ptrs[0], 0, outs.ptrs[2], outs.ptrs[3]])
        odd = [outs.ptrs[0], outs.ptrs[1] + 1, outs.ptrs[2], outs.ptrs[3]]
        refused(["aligned", "%x" % odd[1], "image 1"], d_outs=odd)
        refused(["nimg"], d_blobs=ins[:2], lens=lens[:2], d_outs=outs.ptrs[:2], rects=rects[:2], flips=flips[:2])
        # the context still works after all that
        for i, (g, r) in enumerate(zip(_decode(ctx, 1, d_b, lens, word, F16, (OW, OH), scale, bias, rects, flips), rasters)):
            assert np.array_equal(g, Resampled(r, rects[i], flips[i], OH, OW).bits(word, F16, scale, bias).reshape(-1)), i
    finally:
        ctx.close()


@pytest.mark.gpu
def test_load_files_antialias_and_stack_on_goldens(gpu, manifest):
    """load_files(size=(32, 48), antialias=True, stack=True) on committed reference-written goldens of different sizes, levels and
    channel counts: one tensor, every slice the checker's bits of api.load of the file with its rectangle and flip."""
    import torch
    from xpng_amd import tensors
    names = ["crop_evil", "crop_olaf", "img_juicy", "img_pigz-logo", "special_opaque_alpha"]
    files = sorted({manifest[n][lv]["file"] for n in names for lv in ("L1", "L2")})
    paths = [os.path.join(GOLD, f) for f in files]
    want = [gpu.load(p) for p in paths]
    assert len({r.shape for r in want}) >= 3 and {r.shape[2] for r in want} == {3, 4}
    dims = [(r.shape[1], r.shape[0]) for r in want]
    crops = tensors.random_resized_crops(dims, generator=torch.Generator().manual_seed(3))
    crops[0] = None
    flips = [i % 2 == 1 for i in range(len(paths))]
    assert any((c[2] if c else w) > 48 and (c[3] if c else h) > 32 for c, (w, h) in zip(crops, dims))   # (some do shrink)
    scale, bias = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    OH, OW = 32, 48
    zs = [Resampled(r, c, f, OH, OW) for r, c, f in zip(want, crops, flips)]
    for lay, bgr, dtype in (("chw", False, F16), ("hwc", True, F32)):
        t = tensors.load_files(paths, layout=lay, channels=3, bgr=bgr, dtype=_torch_dtype(dtype), mean=IMAGENET_MEAN, std=IMAGENET_STD,
                               size=(OH, OW), crops=crops, flips=flips, stack=True, antialias=True)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == _torch_dtype(dtype)
        assert tuple(t.shape) == (len(paths),) + ((3, OH, OW) if lay == "chw" else (OH, OW, 3))
        word = api.layout(planar=lay == "chw", bgr=bgr, channels=3)
        for i, z in enumerate(zs):
            assert np.array_equal(_bits(t[i], dtype), z.bits(word, dtype, scale, bias)), (lay, i, paths[i])
    lst = tensors.load_files(paths[:3], channels=3, dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, size=(OH, OW), antialias=True)
    assert isinstance(lst, list) and all(tuple(g.shape) == (3, OH, OW) and g.is_cuda for g in lst)
    for i, g in enumerate(lst):
        assert np.array_equal(_bits(g, F16), Resampled(want[i], None, False, OH, OW).bits(api.layout(planar=True, channels=3), F16, scale, bias)), i
