"""Crop, resize and flip in the copy-out of a mixed-size decode (include/xpng_hip.h xpnghip_decode_varsize_device_batch_resized,
xpnghip_resize_host; xpng_amd/tensors.py load_files size / crops / flips, random_resized_crops).

The checker is tests/_resize.py: the rule in numpy with the C library's fmaf, independent of the code under test.  Every comparison
with the library is on the bits.
CPU: the symbols; xpnghip_resize_host against the checker for every layout word x dtype on RGB and RGBA rasters; the identity
property (a rectangle of the output's size is the float table's lookup of the cropped bytes) and the flip mirror; the rule against
torch's F.interpolate; refusals; load_files(size=...) on the host-answered kinds; random_resized_crops.
GPU (-m gpu): every layout word x dtype x format on batches with the edge rectangles, inside sentinel-filled buffers; the identity
call against the float call on the same context; NULL rects / flips, both size walks, rectangles that change between two calls on
one pointer array, the workspace, a rejected tile, misuse; load_files(size=..., stack=True) on reference-written goldens."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _kit import (BF16, BITS, DTYPES, ES, F16, F32, FORMATS, IMAGENET_MEAN, IMAGENET_STD, Arena, _bits, _offsets, _torch_dtype, _upload,
                  arrange, built, consts_from, f32_of, gpu, mixed_consts, po)
from _resize import Resized
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_decode_varsize_device_batch_resized", "xpnghip_resize_host"]
WORDS = [api.layout(planar=p, bgr=b, channels=c) for c in (0, 3, 4) for p in (False, True) for b in (False, True)]
RGB_DIMS = [(1, 1), (2, 1), (1, 2), (3, 3), (17, 4), (64, 64), (445, 444), (889, 445), (100, 1100)]
RGBA_DIMS = [(4, 4), (5, 7), (13, 4), (64, 64), (445, 444), (889, 445)]
GPU_SIZES = [(3, 5), (37, 29)]                                    # (OW, OH): rows narrower than one 16-byte store; an odd width
# one rectangle per image: whole, 1 x 1 at the last pixel, the last column, the last row, across the 444-px tile boundary of the
# 889-wide image, an upscale (a rectangle smaller than either output) and downscales
RGB_RECTS = [(0, 0, 1, 1), (1, 0, 1, 1), (0, 0, 1, 2), (2, 0, 1, 3), (0, 3, 17, 1), (10, 20, 2, 3), (0, 0, 445, 444), (440, 100, 9, 200),
             (3, 50, 90, 1000)]
RGBA_RECTS = [(0, 0, 4, 4), (4, 6, 1, 1), (12, 0, 1, 4), (0, 63, 64, 1), (430, 431, 2, 4), (440, 0, 9, 445)]


def _lib_resize(r, rect, flip, OW, OH, word, dtype, scale, bias):
    ch = (word >> 8) or r.shape[2]
    raw = api.resize_host(r, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip)
    shape = (ch, OH, OW) if word & 1 else (OH, OW, ch)
    return np.frombuffer(raw, BITS[dtype]).reshape(shape)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_resize_symbols_are_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xpng_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(xpnghip_\w*)\s*\(", txt))
    assert set(NEW) <= names and set(NEW) <= set(api.HIP_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.HIP_SO], text=True)
    assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    import xpng_amd
    assert "resize_host" in xpng_amd.__all__ and hasattr(xpng_amd, "resize_host")
    assert hasattr(api.MixedContext, "decode_batch_resized")
    assert api.hip_lib().xpnghip_abi_version() == 2
    from xpng_amd import tensors
    assert hasattr(tensors, "random_resized_crops")


HOST_RASTERS = [(1, 1), (2, 1), (1, 2), (3, 3), (17, 4), (45, 31)]
HOST_SIZES = [(1, 1), (3, 5), (8, 8), (37, 29)]                   # (OW, OH)


def _host_rects(w, h, OW, OH):
    rects = [None, (w - 1, h - 1, 1, 1), (w - 1, 0, 1, h)]       # whole, 1 x 1 at the last pixel, the rightmost column
    if w >= OW and h >= OH:
        rects.append((w - OW, h - OH, OW, OH))                    # of the output's size
    return rects


@pytest.mark.parametrize("px", [3, 4])
def test_resize_host_equals_the_checker(px):
    """Every layout word x dtype, four different (scale, bias) pairs, on the bits; with it the identity property (a rectangle of
    the output's size gives the float table's lookup of the cropped bytes) and the mirror property of the library's own outputs."""
    rng = np.random.default_rng(100 + px)
    identities = 0
    for (w, h) in HOST_RASTERS:
        r = rng.integers(0, 256, (h, w, px), dtype=np.uint8)
        for (OW, OH) in HOST_SIZES:
            for rect in _host_rects(w, h, OW, OH):
                want = [Resized(r, rect, flip, OH, OW) for flip in (False, True)]
                for dtype in DTYPES:
                    scale, bias = mixed_consts(dtype)
                    for word in WORDS:
                        got = [_lib_resize(r, rect, flip, OW, OH, word, dtype, scale, bias) for flip in (False, True)]
                        for flip in (0, 1):
                            exp = want[flip].bits(word, dtype, scale, bias)
                            assert got[flip].shape == exp.shape and np.array_equal(got[flip], exp), \
                                (px, (w, h), (OW, OH), rect, flip, dtype, hex(word), np.argwhere(got[flip] != exp)[:4])
                        ax = 2 if word & 1 else 1
                        assert np.array_equal(got[1], np.flip(got[0], axis=ax)), ("mirror", (w, h), (OW, OH), rect, dtype, hex(word))
                        if rect is not None and rect[2:] == (OW, OH):
                            ch = (word >> 8) or px
                            tab = np.frombuffer(api.float_table(dtype, scale[:ch], bias[:ch]), BITS[dtype]).reshape(ch, 256)
                            a = arrange(r[rect[1]:rect[1] + OH, rect[0]:rect[0] + OW], bool(word & 1), bool(word & 2), ch)
                            look = np.stack([tab[c][a[c] if word & 1 else a[..., c]] for c in range(ch)], axis=0 if word & 1 else 2)
                            assert np.array_equal(got[0], look), ("identity", (w, h), rect, dtype, hex(word))
                            identities += 1
    assert identities >= 36 * 5


TORCH_SHAPES = [(1, 1, 3, 5), (2, 3, 7, 7), (17, 4, 8, 8), (45, 31, 29, 37), (444, 445, 37, 29), (100, 1100, 33, 31), (5, 7, 64, 63),
                (889, 445, 224, 224)]                               # (h, w, OH, OW)


def test_rule_against_torch_interpolate():
    """The checker (f32, scale 1, bias 0) against torch's CPU F.interpolate(bilinear, align_corners=False, antialias=False) of the
    cropped fp32 raster.  torch sums four weighted taps where the rule nests three FMAs, so the two differ in the last bits: with
    a prototype of the rule the largest difference over these shapes was 2^-15 in byte units (2 ulp at 255).  The bound is 2^-12:
    8x that for another vector path of another torch build; a wrong tap or a wrong half-pixel convention is off by whole grey
    levels on random bytes."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(7)
    worst = 0.0
    for (h, w, OH, OW) in TORCH_SHAPES:
        r = rng.integers(0, 256, (h + 3, w + 2, 3), dtype=np.uint8)
        rect = (2, 1, w, h)
        v = Resized(r, rect, False, OH, OW).v
        crop = torch.from_numpy(r[1:1 + h, 2:2 + w].astype(np.float32)).permute(2, 0, 1)[None]
        t = F.interpolate(crop, size=(OH, OW), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy()
        d = float(np.abs(t.astype(np.float64) - v.astype(np.float64)).max())
        print("rule vs torch", (h, w, OH, OW), d)
        worst = max(worst, d)
        assert d <= 2.0 ** -12, ((h, w, OH, OW), d)
    print("rule vs torch, worst", worst)


def test_resize_host_refusals():
    lib = api.hip_lib()
    r = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    out = np.full(4 * 4 * 4 * 4 + 4, 0x5A5A5A5A, np.uint32)
    one, zero = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0)
    u64 = C.c_uint64

    def call(pxsz=3, raster=r.ctypes.data, w=7, h=5, rect=None, flip=0, ow=4, oh=4, layout=0, dtype=F32, scale=one, bias=zero, o=None):
        ra = None if rect is None else (u64 * 4)(*rect)
        return lib.xpnghip_resize_host(pxsz, raster, w, h, ra, flip, ow, oh, layout, dtype, scale, bias, out.ctypes.data if o is None else o)

    def refused(words, **kw):
        assert call(**kw) != 0, kw
        assert all(w in api._err() for w in words), (words, api._err())

    assert call() == 0
    out[:] = 0x5A5A5A5A
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
        api.resize_host(r, (4, 4), 0, F32, rect=(0, 0, 8, 1))
    assert "{0, 0, 8, 1}" in str(e.value)
    # the device entry point refuses a NULL context like its siblings
    p1, n1 = (C.c_void_p * 1)(0), (u64 * 1)(0)
    assert lib.xpnghip_decode_varsize_device_batch_resized(None, 1, p1, n1, 1, None, p1, 0, F16, None, None, None, None, 4, 4, None) != 0
    assert "null context" in api._err()


def _host_files(po, tmp_path):
    """two oracle-written level-7 files and the committed 11-byte single-colour golden, with the oracle's decode of each (as
    tests/test_float_layouts.py builds them)"""
    from xpng_amd.synth import synth_raster
    paths = []
    for (w, h, alpha) in [(5, 7, False), (9, 6, True)]:
        p = tmp_path / f"l7_{w}x{h}_{int(alpha)}.xpng"
        p.write_bytes(po.encode_image(7, synth_raster("noise" if alpha else "photo", w, h, alpha, seed=w)))
        paths.append(str(p))
    single = os.path.join(GOLD, "imgfull_30d5c8.L2.xpng")
    assert os.path.getsize(single) == 11
    paths.insert(1, single)
    return paths, [po.decode_image(open(p, "rb").read()) for p in paths]


def test_load_files_size_answers_host_kinds_without_a_gpu(po, tmp_path):
    import torch
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    assert [r.shape for r in want] == [(7, 5, 3), (1000, 1000, 3), (6, 9, 4)]
    crops, flips = [(1, 2, 3, 4), None, (2, 0, 7, 5)], [True, False, True]
    mean, std = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)
    OH, OW = 6, 5
    zs = [Resized(r, c, f, OH, OW) for r, c, f in zip(want, crops, flips)]
    for dtype in DTYPES:
        for ch in (3, 4):
            scale, bias = consts_from(mean[:ch], std[:ch])
            for lay in ("chw", "hwc"):
                for bgr in (False, True):
                    word = api.layout(planar=lay == "chw", bgr=bgr, channels=ch)
                    kw = dict(layout=lay, channels=ch, bgr=bgr, device="cpu", dtype=_torch_dtype(dtype), mean=mean[:ch], std=std[:ch],
                              size=(OH, OW), crops=crops, flips=flips)
                    got = tensors.load_files(paths, **kw)
                    whole = tensors.load_files(paths, stack=True, **kw)
                    assert isinstance(got, list) and len(got) == 3 and isinstance(whole, torch.Tensor) and whole.is_contiguous()
                    assert tuple(whole.shape) == (3,) + ((ch, OH, OW) if lay == "chw" else (OH, OW, ch)) and whole.dtype == _torch_dtype(dtype)
                    for i, (g, z) in enumerate(zip(got, zs)):
                        exp = z.bits(word, dtype, scale, bias)
                        assert g.device.type == "cpu" and g.is_contiguous() and tuple(g.shape) == exp.shape
                        assert np.array_equal(_bits(g, dtype), exp), (dtype, ch, lay, bgr, i)
                        assert np.array_equal(_bits(whole[i], dtype), exp), ("stack", dtype, ch, lay, bgr, i)
    # channels None keeps each file's own count; no crops and no flips: every whole image
    got = tensors.load_files(paths, device="cpu", dtype=torch.float32, size=(4, 3))
    for g, r in zip(got, want):
        px = r.shape[2]
        exp = Resized(r, None, False, 4, 3).bits(api.layout(planar=True), F32, [f32_of(1 / 255.0)] * px, [0.0] * px)
        assert tuple(g.shape) == (px, 4, 3) and np.array_equal(_bits(g, F32), exp)
    # misuse
    for bad in (dict(size=(4, 4)),                                               # uint8
                dict(crops=crops), dict(flips=flips),                             # without size
                dict(dtype=torch.float16, size=(4, 4), crops=crops[:2]), dict(dtype=torch.float16, size=(4, 4), flips=flips + [False]),
                dict(dtype=torch.float16, size=(0, 4)), dict(dtype=torch.float16, size=(4, 16385)), dict(dtype=torch.float16, size=4),
                dict(dtype=torch.float16, size=(4, 4), crops=[(0, 0, 6, 1), None, None]),          # leaves the 5 x 7 image
                dict(dtype=torch.float16, size=(4, 4), stack=True)):                                 # channels None: 3 and 4 do not stack
        with pytest.raises(api.XpngError):
            tensors.load_files(paths, device="cpu", **bad)
    with pytest.raises(api.XpngError) as e:
        tensors.load_files(paths, device="cpu", size=(4, 4))
    assert "float dtype" in str(e.value)
    # size=None is today's path
    for g, r in zip(tensors.load_files(paths, layout="hwc", device="cpu"), want):
        assert g.dtype == torch.uint8 and np.array_equal(g.numpy(), r)


def test_random_resized_crops():
    import math
    import torch
    from xpng_amd import tensors
    rng = np.random.default_rng(5)
    dims = [(int(w), int(h)) for w, h in rng.integers(1, 2049, (200, 2))] + [(1, 1), (1, 2048), (2048, 1), (3, 2)]
    for scale, ratio in (((0.08, 1.0), (3 / 4, 4 / 3)), ((0.5, 0.6), (1.9, 2.0))):
        a = tensors.random_resized_crops(dims, scale, ratio, generator=torch.Generator().manual_seed(11))
        b = tensors.random_resized_crops(dims, scale, ratio, generator=torch.Generator().manual_seed(11))
        c = tensors.random_resized_crops(dims, scale, ratio, generator=torch.Generator().manual_seed(12))
        assert a == b and a != c and len(a) == len(dims)
        fallbacks = 0
        for (W, H), (x, y, w, h) in zip(dims, a):
            assert all(isinstance(v, int) for v in (x, y, w, h))
            assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H, ((W, H), (x, y, w, h))
            # w and h are roundings of real numbers whose product and quotient lie in the ranges: each is within 0.5 of them
            in_area = (w - 0.5) * (h - 0.5) <= scale[1] * W * H and (w + 0.5) * (h + 0.5) >= scale[0] * W * H
            in_ratio = (w - 0.5) / (h + 0.5) <= ratio[1] and (w + 0.5) / max(h - 0.5, 1e-9) >= ratio[0]
            if not (in_area and in_ratio):
                assert (x, y, w, h) == tensors.centre_crop(W, H, ratio), ((W, H), (x, y, w, h))
                fallbacks += 1
        assert fallbacks < len(dims)
    assert tensors.centre_crop(100, 1000) == (0, 433, 100, 133) and tensors.centre_crop(1000, 100) == (433, 0, 133, 100)
    assert tensors.centre_crop(100, 100) == (0, 0, 100, 100) and math.isclose(100 / 133, 0.75, rel_tol=0.01)


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
        _CHECK[k] = Resized(raster, rect, bool(flip), OH, OW)
    return _CHECK[k]


def _decode_resized(ctx, mode, d_b, lens, word, dtype, size, scale, bias, rects, flips, offs=None, expect_status=0, arena=None):
    """the images' elements as bit patterns, flat; size = (OW, OH)"""
    ch = api.layout_channels(word, ctx.pxsz)
    ar = arena or Arena([ES[dtype] * ch * size[0] * size[1]] * ctx.nimg, ES[dtype])
    ctx.decode_batch_resized(mode, [t.data_ptr() for t in d_b], lens, ar.ptrs, word, dtype, (size[1], size[0]), scale and scale[:ch], bias and bias[:ch],
                             rects=rects, flips=flips, tile_offs=offs)
    assert ctx.decode_status() == expect_status
    return [g.view(BITS[dtype]) for g in ar.fetch()]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_decode_resized_into_every_layout(gpu, batches, mode, alpha, dtype):
    """All 12 layout words x both output sizes, four different (scale, bias) pairs, the edge rectangles, alternating flips, every
    output at LEAD + es * (i % 8) inside a sentinel-filled region: the checker's bits and intact sentinels.  Then NULL rects and
    flips, both size walks, and two calls back to back on one pointer array with different rectangles."""
    dims, rects, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    flips = [i % 2 for i in range(len(dims))]
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for (OW, OH) in GPU_SIZES:
            for word in WORDS:
                got = _decode_resized(ctx, mode, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips)
                for i, (g, r) in enumerate(zip(got, rasters)):
                    w = checked((mode, alpha), i, r, rects[i], flips[i], OW, OH).bits(word, dtype, scale, bias).reshape(-1)
                    assert np.array_equal(g, w), (hex(word), dtype, (OW, OH), i, dims[i], rects[i], np.argwhere(g != w)[:4].ravel())
        OW, OH = GPU_SIZES[1]
        word = api.layout(planar=True, bgr=True, channels=7 - px)
        ch = 7 - px
        # one pointer array, three calls: the rectangles above, then none (every whole image, no flip), then the first again
        ar = Arena([ES[dtype] * ch * OW * OH] * len(dims), ES[dtype])
        a = _decode_resized(ctx, mode, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips, arena=ar)
        ar.refill()
        b = _decode_resized(ctx, mode, d_b, lens, word, dtype, (OW, OH), scale, bias, None, None, arena=ar)
        ar.refill()
        c = _decode_resized(ctx, mode, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips, _offsets(blobs, ctx), arena=ar)
        for i, r in enumerate(rasters):
            wa = checked((mode, alpha), i, r, rects[i], flips[i], OW, OH).bits(word, dtype, scale, bias).reshape(-1)
            wb = checked((mode, alpha), i, r, None, 0, OW, OH).bits(word, dtype, scale, bias).reshape(-1)
            assert np.array_equal(a[i], wa) and np.array_equal(b[i], wb) and np.array_equal(c[i], wa), (dtype, i)
        assert any(not np.array_equal(x, y) for x, y in zip(a, b))      # (the two rectangle sets do differ)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [False, True])
def test_identity_rectangles_equal_the_float_call(gpu, batches, alpha):
    """Rectangles of the output's size: the elements are bit for bit the slices of decode_batch_as_float on the same context, and
    a flip is their mirror.  The float call comes first: the resized call after it adds no workspace beyond its record table."""
    dims, _, rasters, blobs = batches[(1, alpha)]
    px = 4 if alpha else 3
    OW, OH = GPU_SIZES[1]
    big = [i for i, (w, h) in enumerate(dims) if w >= OW and h >= OH]
    assert len(big) >= 3
    rects = [((w - OW) // 2 + i, (h - OH) // 3, OW, OH) if i in big else (0, 0, w, h) for i, (w, h) in enumerate(dims)]
    assert rects[dims.index((889, 445))][0] < 444 < rects[dims.index((889, 445))][0] + OW     # across the tile boundary
    flips = [(i // 2) % 2 for i in range(len(dims))]
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for dtype in DTYPES:
            scale, bias = mixed_consts(dtype)
            for word in WORDS:
                ch = api.layout_channels(word, px)
                full = Arena([ES[dtype] * ch * w * h for (w, h) in dims], ES[dtype])
                ctx.decode_batch_as_float(1, [t.data_ptr() for t in d_b], lens, full.ptrs, word, dtype, scale[:ch], bias[:ch])
                assert ctx.decode_status() == 0
                ref = [g.view(BITS[dtype]) for g in full.fetch()]
                ws = ctx.workspace_bytes()
                got = _decode_resized(ctx, 1, d_b, lens, word, dtype, (OW, OH), scale, bias, rects, flips)
                assert 0 <= ctx.workspace_bytes() - ws <= 4096           # the record table, once; no second staging raster
                for i in big:
                    (w, h), (x, y, _, _) = dims[i], rects[i]
                    if word & 1:
                        want = ref[i].reshape(ch, h, w)[:, y:y + OH, x:x + OW]
                        want = want[:, :, ::-1] if flips[i] else want
                    else:
                        want = ref[i].reshape(h, w, ch)[y:y + OH, x:x + OW]
                        want = want[:, ::-1] if flips[i] else want
                    assert np.array_equal(got[i], np.ascontiguousarray(want).reshape(-1)), (hex(word), dtype, i, dims[i])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_rejected_tile_and_misuse_of_the_resized_call(gpu, po):
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
        got = _decode_resized(ctx, 1, _upload(bb), [len(b) for b in bb], word, F16, (OW, OH), scale, bias, rects, flips, expect_status=1)
        clean = 0
        for i, (g, r) in enumerate(zip(got, rasters)):
            z = Resized(r, rects[i], flips[i], OH, OW)
            w = z.bits(word, F16, scale, bias)
            g = g.reshape(w.shape)
            if i == k:
                x0, x1, y0, y1 = z.taps                            # relative to the rectangle
                inx = lambda v: (rects[i][0] + v >= tx) & (rects[i][0] + v < tx + tw)      # noqa: E731
                iny = lambda v: (rects[i][1] + v >= ty) & (rects[i][1] + v < ty + th)      # noqa: E731
                hit = (iny(y0) | iny(y1))[:, None] & (inx(x0) | inx(x1))[None, :]
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
            a = dict(mode=1, d_blobs=ins, lens=lens, d_outs=outs.ptrs, layout=word, dtype=F16, size=(OH, OW), rects=rects, flips=flips)
            a.update(kw)
            with pytest.raises(gpu.XpngError) as e:
                ctx.decode_batch_resized(**a)
            assert all(w in str(e.value) for w in words), (words, str(e.value))
            assert outs.untouched(), words

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
        for i, (g, r) in enumerate(zip(_decode_resized(ctx, 1, d_b, lens, word, F16, (OW, OH), scale, bias, rects, flips), rasters)):
            assert np.array_equal(g, Resized(r, rects[i], flips[i], OH, OW).bits(word, F16, scale, bias).reshape(-1)), i
    finally:
        ctx.close()


@pytest.mark.gpu
def test_load_files_size_and_stack_on_goldens(gpu, manifest):
    """load_files(size=..., stack=True) on committed reference-written goldens of different sizes, levels and channel counts: one
    tensor, every slice the checker's bits of api.load of the file with its rectangle and flip."""
    import torch
    from xpng_amd import tensors
    names = ["crop_evil", "crop_olaf", "img_juicy", "img_pigz-logo", "imgfull_pe4en_k", "special_opaque_alpha"]
    files = sorted({manifest[n][lv]["file"] for n in names for lv in ("L1", "L2")})
    paths = [os.path.join(GOLD, f) for f in files]
    want = [gpu.load(p) for p in paths]
    assert len({r.shape for r in want}) >= 3 and {r.shape[2] for r in want} == {3, 4}
    dims = [(r.shape[1], r.shape[0]) for r in want]
    crops = tensors.random_resized_crops(dims, generator=torch.Generator().manual_seed(3))
    crops[0] = None
    flips = [i % 2 == 1 for i in range(len(paths))]
    scale, bias = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    OH, OW = 24, 21
    for lay, bgr, dtype in (("chw", False, F16), ("hwc", True, F32)):
        t = tensors.load_files(paths, layout=lay, channels=3, bgr=bgr, dtype=_torch_dtype(dtype), mean=IMAGENET_MEAN, std=IMAGENET_STD,
                               size=(OH, OW), crops=crops, flips=flips, stack=True)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == _torch_dtype(dtype)
        assert tuple(t.shape) == (len(paths),) + ((3, OH, OW) if lay == "chw" else (OH, OW, 3))
        word = api.layout(planar=lay == "chw", bgr=bgr, channels=3)
        for i, r in enumerate(want):
            exp = Resized(r, crops[i], flips[i], OH, OW).bits(word, dtype, scale, bias)
            assert np.array_equal(_bits(t[i], dtype), exp), (lay, i, paths[i])
    lst = tensors.load_files(paths[:3], channels=3, dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, size=(OH, OW))
    assert isinstance(lst, list) and all(tuple(g.shape) == (3, OH, OW) and g.is_cuda for g in lst)
    for i, g in enumerate(lst):
        assert np.array_equal(_bits(g, F16), Resized(want[i], None, False, OH, OW).bits(api.layout(planar=True, channels=3), F16, scale, bias)), i
