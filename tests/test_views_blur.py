"""Gaussian blur and solarise per view in a views decode (include/xpng_hip.h xpnghip_blur_weights, xpnghip_resample_blur_host,
xpnghip_decode_varsize_device_batch_views_blur; xpng_amd/tensors.py load_views(blur=, solarise=), random_gaussian_blur,
random_solarise).

CPU: the symbols; the weights against the float64 formula; the host rule against the independent checker (tests/_blur.py) on the
bits; the consequences the header states; solarise; the clamp; the rule against torch's reflect pad and depthwise conv2d in float64;
every refusal; load_views on host-answered files without a GPU.  GPU: every view of a device call against the host rule on the
bits."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import _blur
from _blur import Blurred
from _kit import (BF16, BITS, DTYPES, ES, F16, F32, FORMATS, IMAGENET_MEAN, IMAGENET_STD, Arena, _bits, _offsets, _torch_dtype, _upload, built,
                  consts_from, declared, exported, gpu, mixed_consts, po)
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_blur_weights", "xpnghip_resample_blur_host", "xpnghip_decode_varsize_device_batch_views_blur"]
WORDS = [api.layout(planar=p, bgr=b, channels=c) for c in (0, 3, 4) for p in (False, True) for b in (False, True)]
PERM = [0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0]                       # R <- B, G <- R, B <- G: not symmetric, so a transposed index shows
RANGE = [3, -2, 0.5, -300, -2, 3, 0, 300, 1, 1, -2, 40]            # leaves 0 .. 255 on both sides
DENSE = [0.70710678, -0.31830989, 0.57721566, 12.345678, 0.14142135, 1.6180339, -0.69314718, -7.3890561, -0.43429448, 0.26179939, 1.2020569,
         31.415926]
OFF = (0.0, 0, None)                                               # the record that is all off


def _lib(r, rect, flip, OW, OH, word, dtype, scale, bias, filt, colour=None, blur=None):
    ch = (word >> 8) or r.shape[2]
    raw = api.resample_blur_host(r, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip, filter=filt, colour=colour, blur=blur)
    shape = (ch, OH, OW) if word & 1 else (OH, OW, ch)
    return np.frombuffer(raw, BITS[dtype]).reshape(shape)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_blur_symbols_are_declared_listed_and_exported():
    assert set(NEW) <= set(declared("xpng_hip.h", "xpnghip_")) and set(NEW) <= set(api.HIP_SYMBOLS) and set(NEW) <= exported(api.HIP_SO)
    assert api.hip_lib().xpnghip_abi_version() == 2
    import xpng_amd
    from xpng_amd import tensors
    for name in ("blur_weights", "resample_blur_host", "FILTER_CUBIC_AA"):
        assert name in xpng_amd.__all__ and hasattr(xpng_amd, name)
    assert xpng_amd.FILTER_CUBIC_AA == 2 and callable(api.MixedContext.decode_batch_views_blur)
    assert callable(tensors.random_gaussian_blur) and callable(tensors.random_solarise)
    assert C.sizeof(api.ViewBlur) == 16
    hdr = open(os.path.join(ROOT, "include", "xpng_hip.h")).read()
    assert "#define XPNGHIP_FILTER_CUBIC_AA 2u" in hdr
    assert "typedef struct { float sigma; uint32_t radius; float solarise; uint32_t reserved; } xpnghip_view_blur;" in hdr


def test_blur_weights_equal_the_float64_formula():
    """bit for bit; the kernel is symmetric by construction - one w[d] serves both taps at distance d"""
    for sigma in (2.0 ** -10, 0.1, 0.5, 2.0, 10.0, 1024.0):
        for R in (1, 2, 11, 31):
            w = api.blur_weights(sigma, R)
            assert w.dtype == np.float32 and w.shape == (R + 1,)
            assert np.array_equal(w.view(np.uint32), _blur.weights(sigma, R).view(np.uint32)), (sigma, R)
            assert (w >= 0).all() and (np.diff(w) <= 0).all()
            assert abs(float(w[0]) + 2.0 * float(w[1:].astype(np.float64).sum()) - 1.0) < 1e-6
    assert api.blur_weights(0.1, 2)[0] == np.float32(1.0)
    assert np.array_equal(api.blur_weights(0.0, 0), np.ones(1, np.float32))
    for sigma, R, word in ((1.0, 32, "radius is 32"), (0.0, 1, "sigma is 0"), (1.0, 0, "radius 0"), (float("nan"), 3, "nan"), (float("inf"), 3, "inf"),
                           (2.0 ** -11, 3, "2^-10"), (1025.0, 3, "1025")):
        with pytest.raises(api.XpngError) as e:
            api.blur_weights(sigma, R)
        assert word in str(e.value), str(e.value)


HOST_RASTERS = [(3, 3), (17, 4), (45, 31), (130, 9)]               # (w, h)
# (sigma, radius, threshold) with the smallest output that holds it, (OW, OH) = (R + 1, R + 1), and a larger one
RECORDS = [(0.5, 1, None), (2.0, 2, 128.0), (10.0, 11, None), (1024.0, 31, 0.0), (0.0, 0, 255.0), (2.0 ** -10, 1, 100.5), (3.0, 5, 255.0), None]


def test_resample_blur_host_equals_the_checker():
    """The library's host rule against tests/_blur.py on the bits: filters 0, 1 and 2, with and without a matrix, both pixel sizes,
    whole rasters and rectangles, both flips, outputs from (R + 1) x (R + 1) up, and - turning over the cases - every layout word
    with every dtype."""
    rng = np.random.default_rng(23)
    k = 0
    seen = set()
    for (w, h) in HOST_RASTERS:
        for px in (3, 4):
            r = rng.integers(0, 256, (h, w, px), dtype=np.uint8)
            for filt in (0, 1, 2):
                colour = [None, DENSE, RANGE, PERM][(k + filt) % 4]
                rect = None if k % 3 else (1, 0, w - 2, h - 1)
                flip = bool(k % 2)
                for rec in (RECORDS[k % 8], RECORDS[(k + 3) % 8], RECORDS[(k + 5) % 8]):
                    R = rec[1] if rec else 0
                    for (OW, OH) in ((R + 1, R + 1), (R + 6, R + 2)):
                        b = Blurred(r, rect, flip, OH, OW, filt, colour, rec)
                        for _ in range(3):
                            word, dtype = WORDS[k % 12], DTYPES[(k // 12) % 3]
                            k += 5                                  # (5 is coprime to 36: the pairs turn over)
                            seen.add((word, dtype))
                            scale, bias = mixed_consts(dtype)
                            got = _lib(r, rect, flip, OW, OH, word, dtype, scale, bias, filt, colour, rec)
                            exp = b.bits(word, dtype, scale, bias)
                            assert got.shape == exp.shape and np.array_equal(got, exp), ((w, h), px, filt, colour, rect, flip, rec, (OW, OH), hex(word), dtype)
                k += 1
    assert len(seen) == 36


def test_consequences_all_off_and_flip():
    rng = np.random.default_rng(5)
    r = rng.integers(0, 256, (31, 45, 4), dtype=np.uint8)
    rect = (2, 3, 40, 25)
    for filt in (0, 1, 2):
        for colour in (None, DENSE):
            for word, dtype in ((WORDS[3], F16), (WORDS[8], BF16), (WORDS[5], F32)):
                scale, bias = mixed_consts(dtype)
                ch = (word >> 8) or 4
                # (a) all off, as a record and as None: the bits of the plain call
                if filt == 2:
                    plain = api.resample_cubic_host(r, (13, 17), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=True, colour=colour)
                else:
                    plain = api.resample_colour_host(r, (13, 17), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=True, filter=filt, colour=colour)
                for blur in (None, OFF):
                    got = api.resample_blur_host(r, (13, 17), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=True, filter=filt, colour=colour, blur=blur)
                    assert got == plain, (filt, hex(word), dtype, blur)
                # (b) a flip is a mirror on the bits
                for blur in ((2.5, 7, None), (0.7, 2, 128.0), (0.0, 0, 60.0)):
                    a = _lib(r, rect, False, 17, 13, word, dtype, scale, bias, filt, colour, blur)
                    b = _lib(r, rect, True, 17, 13, word, dtype, scale, bias, filt, colour, blur)
                    assert np.array_equal(b, a[:, :, ::-1] if word & 1 else a[:, ::-1, :]), (filt, hex(word), dtype, blur)
                    assert not np.array_equal(a, b)


def test_solarise_thresholds_and_alpha():
    rng = np.random.default_rng(9)
    r = rng.integers(0, 256, (9, 11, 4), dtype=np.uint8)
    word = api.layout(planar=True, channels=4)
    one, zero = [1.0] * 4, [0.0] * 4
    base = _lib(r, None, False, 11, 9, word, F32, one, zero, 0).view(np.float32)   # a rectangle of the output's size: the bytes themselves
    assert np.array_equal(base, r.transpose(2, 0, 1).astype(np.float32))
    for thr in (0.0, 128.0, 255.0):
        got = _lib(r, None, False, 11, 9, word, F32, one, zero, 0, blur=(0.0, 0, thr)).view(np.float32)
        exp = base.copy()
        exp[:3] = np.where(base[:3] >= thr, 255.0 - base[:3], base[:3])
        assert np.array_equal(got, exp), thr
        assert np.array_equal(got[3], base[3])                     # alpha is not solarised
    assert (_lib(r, None, False, 11, 9, word, F32, one, zero, 0, blur=(0.0, 0, 0.0)).view(np.float32)[:3] == 255.0 - base[:3]).all()
    # ... and not blurred either, while the colours are
    got = _lib(r, None, False, 11, 9, word, F32, one, zero, 0, blur=(2.0, 4, None)).view(np.float32)
    assert np.array_equal(got[3], base[3]) and not np.array_equal(got[:3], base[:3])
    assert np.array_equal(got, Blurred(r, None, False, 9, 11, 0, None, (2.0, 4, None)).bits(word, F32, one, zero).view(np.float32))


def test_the_clamp_is_exercised():
    """The weights are rounded one by one, so their sum can pass 1 by a few units in the last place: a white raster then blurs to
    more than 255 and the clamp brings it back.  (T is not negative and no weight is, so the lower end cannot be passed.)"""
    r = np.full((12, 12, 3), 255, np.uint8)
    word = api.layout(planar=True, channels=3)
    over = 0
    for sigma, R in ((0.8, 2), (1.0, 3), (1.3, 4), (2.0, 6), (2.7, 8), (3.1, 9), (4.0, 11)):
        b = Blurred(r, None, False, 12, 12, 0, None, (sigma, R, None))
        got = _lib(r, None, False, 12, 12, word, F32, [1.0] * 3, [0.0] * 3, 0, blur=(sigma, R, None)).view(np.float32)
        assert np.array_equal(got, b.bits(word, F32, [1.0] * 3, [0.0] * 3).view(np.float32)) and got.max() <= 255.0
        if b.raw.max() > 255.0:
            over += 1
            assert got.max() == 255.0
    assert over, "no case of this list passes 255 before the clamp"


TORCH_CASES = [((45, 31), (29, 37), 1, (2.0, 11)), ((130, 9), (12, 12), 2, (0.1, 2)), ((17, 4), (32, 32), 0, (10.0, 31)), ((45, 31), (40, 64), 2, (1.3, 4)),
               ((130, 9), (23, 24), 1, (2.0, 11)), ((45, 31), (6, 7), 0, (0.5, 1)), ((45, 31), (33, 35), 2, (1024.0, 31))]
# measured here on the CPU over TORCH_CASES: the largest difference is 3.22e-5 of a byte step (sigma 1024, 63 taps); four times that
# is 1.29e-4 and the next power of two above it 2^-12 = 2.44e-4.  The margin covers the fp32 order of accumulation on other inputs
TORCH_BOUND = 2.0 ** -12


def test_rule_against_torch_reflect_pad_and_conv2d():
    """The blur of the checker's T against torch on the CPU in float64: F.pad(mode="reflect") and a depthwise conv2d with weights
    built the torchvision way (linspace, exp(-0.5 (x / sigma)^2), normalise), clamped to 0 .. 255."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(11)
    worst = 0.0
    for ((w, h), (OH, OW), filt, (sigma, R)) in TORCH_CASES:
        r = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b = Blurred(r, None, False, OH, OW, filt, None, (sigma, R, None))
        ks = 2 * R + 1
        x = torch.linspace(-R, R, ks, dtype=torch.float64)
        pdf = torch.exp(-0.5 * (x / float(np.float32(sigma))).pow(2))
        k1 = pdf / pdf.sum()
        k2 = (k1[:, None] * k1[None, :]).expand(3, 1, ks, ks)
        T = torch.from_numpy(b.T.astype(np.float64)).permute(2, 0, 1)[None]
        t = F.conv2d(F.pad(T, [R, R, R, R], mode="reflect"), k2, groups=3).clamp(0.0, 255.0)[0].permute(1, 2, 0).numpy()
        d = float(np.abs(t - b.v.astype(np.float64)).max())
        print("blur rule vs torch", (w, h), (OH, OW), filt, (sigma, R), d)
        worst = max(worst, d)
        assert d <= TORCH_BOUND, ((w, h), (OH, OW), filt, (sigma, R), d)
    print("blur rule vs torch, worst", worst)


def test_resample_blur_host_refusals():
    lib = api.hip_lib()
    r = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    out = np.full(4 * 4 * 4 * 4 + 4, 0x5A5A5A5A, np.uint32)
    one, zero = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0)
    u64 = C.c_uint64

    def call(pxsz=3, raster=r.ctypes.data, w=7, h=5, rect=None, flip=0, ow=4, oh=4, layout=0, dtype=F32, scale=one, bias=zero, filt=1, colour=None,
             blur=(1.0, 2, 256.0, 0), o=None):
        ra = None if rect is None else (u64 * 4)(*rect)
        cm = None if colour is None else (C.c_float * 12)(*colour)
        br = None if blur is None else C.byref(api.ViewBlur(*blur))
        return lib.xpnghip_resample_blur_host(pxsz, raster, w, h, ra, flip, ow, oh, layout, dtype, scale, bias, filt, cm, br, out.ctypes.data if o is None else o)

    def refused(words, **kw):
        for filt in (0, 1, 2):
            for colour in (None, DENSE):
                a = dict(filt=filt, colour=colour)
                a.update(kw)
                assert call(**a) != 0, kw
                msg = api._err()
                assert all(w in msg for w in words), (words, msg)

    for filt in (0, 1, 2):
        assert call(filt=filt) == 0 and call(filt=filt, colour=DENSE) == 0 and call(filt=filt, blur=None) == 0
    out[:] = 0x5A5A5A5A
    # the record: every field by its name
    refused(["radius is 32", "0 .. 31"], blur=(1.0, 32, 256.0, 0), ow=64, oh=64)
    refused(["radius 4", "4 x 5"], blur=(1.0, 4, 256.0, 0), oh=5)
    refused(["radius 4", "5 x 4"], blur=(1.0, 4, 256.0, 0), ow=5)
    refused(["sigma is 1", "radius 0"], blur=(1.0, 0, 256.0, 0))
    refused(["sigma is 0", "2^-10"], blur=(0.0, 1, 256.0, 0))
    refused(["sigma is nan"], blur=(float("nan"), 1, 256.0, 0))
    refused(["sigma is inf"], blur=(float("inf"), 1, 256.0, 0))
    refused(["sigma is 1025"], blur=(1025.0, 1, 256.0, 0))
    refused(["sigma is 0.000488281"], blur=(2.0 ** -11, 1, 256.0, 0))
    refused(["solarise is 255.5"], blur=(1.0, 1, 255.5, 0))
    refused(["solarise is 257"], blur=(0.0, 0, 257.0, 0))
    refused(["solarise is -1"], blur=(0.0, 0, -1.0, 0))
    refused(["solarise is nan"], blur=(1.0, 1, float("nan"), 0))
    refused(["reserved is 7"], blur=(1.0, 1, 256.0, 7))
    refused(["filter 3", "XPNGHIP_FILTER_CUBIC_AA"], filt=3)
    # everything the underlying call refuses
    refused(["{0, 0, 0, 3}", "7 x 5"], rect=(0, 0, 0, 3))
    refused(["{2, 0, 6, 1}", "7 x 5"], rect=(2, 0, 6, 1))
    refused(["4 x 0", "16384"], oh=0)
    refused(["16385 x 4"], ow=16385)
    refused(["flip 2"], flip=2)
    refused(["dtype 0"], dtype=0)
    refused(["dtype 4"], dtype=4)
    refused(["layout", "0x4"], layout=0x004)
    refused(["layout", "0x500"], layout=0x500)
    refused(["scale[1]", "nan"], scale=(C.c_float * 4)(1, float("nan"), 1, 1))
    refused(["bias[2]", "inf"], bias=(C.c_float * 4)(0, 0, float("inf"), 0))
    refused(["null"], raster=None)
    refused(["null"], o=0)
    refused(["aligned", "%x" % (out.ctypes.data + 2)], o=out.ctypes.data + 2)
    refused(["aligned"], o=out.ctypes.data + 1, dtype=F16)
    refused(["pxsz is 5"], pxsz=5)
    refused(["0 x 5"], w=0)
    m = list(DENSE)
    m[6] = float("nan")
    for filt in (0, 1, 2):
        assert call(filt=filt, colour=m) != 0 and "[1][2]" in api._err() and "colour" in api._err()
    assert (out == 0x5A5A5A5A).all()                                # a refused call writes nothing
    with pytest.raises(api.XpngError) as e:
        api.resample_blur_host(r, (4, 4), 0, F32, blur=(1.0, 4, None))
    assert "radius 4" in str(e.value)
    for bad in ((1.0,), "blur", (1.0, "x", None)):
        with pytest.raises(api.XpngError) as e:
            api.resample_blur_host(r, (4, 4), 0, F32, blur=bad)
        assert "blur is None or" in str(e.value)
    # the device entry point refuses a filter above 2 and a NULL context like its siblings
    p1, n1 = (C.c_void_p * 1)(0), (u64 * 1)(0)
    args = (None, 1, p1, n1, 1, None, 1, None, p1, (C.c_uint32 * 2)(4, 4), None, None, 0, F16, None, None)
    assert lib.xpnghip_decode_varsize_device_batch_views_blur(*args, 3, None, None, None) != 0 and "filter 3" in api._err()
    assert lib.xpnghip_decode_varsize_device_batch_views_blur(*args, 2, None, None, None) != 0 and "null context" in api._err()
    # the entry points with a filter word keep their domain
    for fn in (api.resample_host, api.resample_colour_host):
        with pytest.raises(api.XpngError) as e:
            fn(r, (4, 4), 0, F32, filter=2)
        assert "filter 2" in str(e.value) and "XPNGHIP_FILTER_TRIANGLE_AA" in str(e.value) and "CUBIC" not in str(e.value)


def _host_files(po, tmp_path):
    """two oracle-written level-7 files and the committed 11-byte single-colour golden, with the oracle's decode of each"""
    from xpng_amd.synth import synth_raster
    paths = []
    for (w, h, alpha) in [(25, 37, False), (39, 16, True)]:
        p = tmp_path / f"l7_{w}x{h}.xpng"
        p.write_bytes(po.encode_image(7, synth_raster("noise" if w > 30 else "photo", w, h, alpha, seed=w)))
        paths.append(str(p))
    single = os.path.join(GOLD, "imgfull_30d5c8.L2.xpng")
    assert os.path.getsize(single) == 11
    paths.insert(1, single)
    return paths, [po.decode_image(open(p, "rb").read()) for p in paths]


def test_load_views_blur_and_solarise_answer_host_kinds_without_a_gpu(po, tmp_path):
    import torch
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    views = [(0, (1, 2, 23, 34), True), (2, None, False), (0, None, False), (1, (100, 200, 300, 150), False), (2, (3, 1, 35, 5), True),
             (0, (23, 35, 1, 1), False)]
    sizes = [(6, 5), (3, 7), (40, 30), (12, 12), (9, 4), (1, 1)]   # (OH, OW): per-view sizes
    cols = [PERM, None, RANGE, None, np.asarray(DENSE).reshape(3, 4), None]
    blur = [(1.5, 5), None, (2.0, 23), (0.3, 3), None, None]
    sol = [None, 128, 100.5, None, None, None]
    recs = [(1.5, 2, None), (0.0, 0, 128.0), (2.0, 11, 100.5), (0.3, 1, None), None, None]
    mean, std = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)
    ident = list(api.COLOUR_IDENTITY)
    for dtype in DTYPES:
        for ch, lay, bgr, interp in ((3, "chw", False, "bicubic"), (4, "hwc", True, "bilinear")):
            scale, bias = consts_from(mean[:ch], std[:ch])
            word = api.layout(planar=lay == "chw", bgr=bgr, channels=ch)
            kw = dict(layout=lay, channels=ch, bgr=bgr, device="cpu", dtype=_torch_dtype(dtype), mean=mean[:ch], std=std[:ch], interpolation=interp)
            filt = 2 if interp == "bicubic" else 1
            got = tensors.load_views(paths, views, sizes, colour=cols, blur=blur, solarise=sol, **kw)
            nocol = tensors.load_views(paths, views, sizes, blur=blur, **kw)
            plain = tensors.load_views(paths, views, sizes, colour=cols, **kw)
            for v, ((i, rect, flip), (oh, ow)) in enumerate(zip(views, sizes)):
                exp = Blurred(want[i], rect, flip, oh, ow, filt, cols[v] if cols[v] is not None else ident, recs[v]).bits(word, dtype, scale, bias)
                g = got[v]
                assert g.device.type == "cpu" and g.is_contiguous() and g.dtype == _torch_dtype(dtype) and tuple(g.shape) == exp.shape
                assert np.array_equal(_bits(g, dtype), exp), (dtype, ch, lay, v)
                rec = recs[v] and (recs[v][0], recs[v][1], None)
                assert np.array_equal(_bits(nocol[v], dtype), Blurred(want[i], rect, flip, oh, ow, filt, None, rec).bits(word, dtype, scale, bias)), (dtype, ch, lay, v)
                if recs[v] is None:
                    assert torch.equal(g, plain[v])
            assert not torch.equal(got[0], plain[0]) and not torch.equal(got[2], plain[2])
    o1 = [torch.zeros((3, 4, 4), dtype=torch.float16)]
    for kw, word in ((dict(blur=[(1.0, 4)]), "odd"), (dict(blur=[(1.0, 65)]), "3 .. 63"), (dict(blur=[(1.0, 9)]), "radius 4"), (dict(blur=[None, None]), "2 entries"),
                     (dict(solarise=[256]), "0 .. 255"), (dict(solarise=[-1]), "0 .. 255"), (dict(blur=[3.0]), "(sigma, kernel_size)"),
                     (dict(blur=[(0.0, 3)]), "sigma is 0")):
        with pytest.raises(api.XpngError) as e:
            tensors.load_views(paths, [(0, None, False)], (4, 4), out=o1, device="cpu", **kw)
        assert word in str(e.value), (kw, str(e.value))
    assert float(o1[0].abs().sum()) == 0.0
    # the two drawing functions: reproducible, the shapes load_views takes
    g = torch.Generator().manual_seed(3)
    a = tensors.random_gaussian_blur(200, generator=g)
    s = tensors.random_solarise(200, generator=g)
    g = torch.Generator().manual_seed(3)
    assert a == tensors.random_gaussian_blur(200, generator=g) and s == tensors.random_solarise(200, generator=g)
    on = [x for x in a if x is not None]
    assert 60 < len(on) < 140 and all(0.1 <= sg <= 2.0 and ks == 23 for (sg, ks) in on)
    assert 15 < sum(x is not None for x in s) < 70 and all(x in (None, 128.0) for x in s)
    assert tensors.random_gaussian_blur(3, p=0.0) == [None] * 3 and all(x is not None for x in tensors.random_gaussian_blur(3, p=1.0))
    for bad in (dict(kernel_size=4), dict(kernel_size=65), dict(sigma=(0.0, 1.0)), dict(sigma=(2.0, 1.0)), dict(p=1.5)):
        with pytest.raises(api.XpngError):
            tensors.random_gaussian_blur(2, **bad)
    for bad in (dict(threshold=256), dict(p=-0.1)):
        with pytest.raises(api.XpngError):
            tensors.random_solarise(2, **bad)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
# tests/test_cubic.py's batches: the 889-wide image has a tile boundary inside the rectangles across x = 444
RGB_DIMS = [(3, 3), (17, 4), (64, 64), (445, 444), (889, 445), (100, 1100)]
RGBA_DIMS = [(4, 4), (17, 4), (64, 64), (445, 444), (889, 445), (100, 1100)]
# ((OW, OH), record): the sizes of the kernel's host run - R + 1, 63, 64, 65, 130 wide and R + 1, 15, 16, 17, 40 high, every edge of
# the 64 x 16 tile from both sides - with plain, blurred, solarise-only and blurred-and-solarised views side by side
SHAPES = [((37, 29), None), ((2, 2), (0.5, 1, None)), ((63, 15), (2.0, 11, 128.0)), ((3, 5), None), ((64, 16), (1.0, 1, None)), ((65, 17), (0.0, 0, 128.0)),
          ((130, 40), (9.5, 31, None)), ((12, 12), (3.7, 11, 200.0)), ((32, 32), (1024.0, 31, 0.0)), ((130, 17), (0.3, 1, 255.0)), ((1, 1), (0.0, 0, 0.0)),
          ((63, 40), (2.0, 11, None)), ((65, 15), OFF), ((64, 32), (20.0, 31, 100.5))]


def _views(dims, p):
    """(image, rectangle, flip, (OW, OH), record) of pass p: tests/test_cubic.py's rectangles - edges, one pixel, across the tile
    boundary, strong downscales; more views than images; several of one image overlap; image 3 (pass 0) or image 0 (pass 1) has
    none - with the shapes above turning over the views."""
    w0, h0 = dims[0]
    views = [(0, (0, 0, w0, h0)), (0, (w0 - 1, h0 - 1, 1, 1)), (1, (16, 3, 1, 1)), (1, (16, 0, 1, 4)), (1, (0, 0, 17, 4)),
             (2, (0, 0, 64, 64)), (2, (0, 63, 64, 1)), (2, (2, 2, 60, 60)), (2, (10, 20, 37, 29)), (2, (27, 35, 37, 29)),
             (3, (10, 20, 2, 3)), (3, (200, 140, 245, 304)),
             (4, (440, 100, 9, 200)), (4, (400, 50, 80, 300)), (5, (3, 50, 90, 1000)), (5, (20, 30, 60, 500))]
    views = [v for v in views if v[0] != (3, 0)[p]]
    return [(i, rect, (k // 2) % 2) + SHAPES[(k + 5 * p) % len(SHAPES)] for k, (i, rect) in enumerate(views)]


def view_args(views):
    return [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [(v[3][1], v[3][0]) for v in views], [v[4] for v in views]


@pytest.fixture(scope="module")
def batches(po):
    """per (mode, alpha): the dims, the rasters and the oracle's tile blobs - computed once, never changed"""
    from xpng_amd.synth import synth_raster
    kinds = ["photo", "noise", "gray", "noise"]
    out = {}
    for mode, alpha in FORMATS:
        dims = RGBA_DIMS if alpha else RGB_DIMS
        rasters = [synth_raster(kinds[(i + 1) % 4], w, h, alpha, seed=i + 31) for i, (w, h) in enumerate(dims)]
        out[(mode, alpha)] = (dims, rasters, [po.encode_tiles(mode, r) for r in rasters])
    return out


def run_blur(ctx, mode, d_b, lens, views, word, dtype, scale, bias, filt, colours=None, offs=None, arena=None, blurs="views"):
    """the views' elements as bit patterns, flat, out of a sentinel-filled arena whose every other byte is checked.  Buffer i starts
    i % 8 elements into its 16-byte aligned region: every start of a row modulo 16 bytes, odd element offsets among them."""
    ch = api.layout_channels(word, ctx.pxsz)
    vi, rects, flips, sizes, recs = view_args(views)
    ar = arena or Arena([ES[dtype] * ch * oh * ow for (oh, ow) in sizes], ES[dtype])
    ctx.decode_batch_views_blur(mode, [t.data_ptr() for t in d_b], lens, vi, ar.ptrs, word, dtype, sizes, scale[:ch], bias[:ch], rects=rects, flips=flips,
                                filter=filt, colours=colours, tile_offs=offs, blurs=recs if blurs == "views" else blurs)
    assert ctx.decode_status() == 0
    return [g.view(BITS[dtype]).copy() for g in ar.fetch()]


def host_rule(raster, view, col, word, dtype, scale, bias, filt):
    i, rect, flip, (OW, OH), rec = view
    ch = api.layout_channels(word, raster.shape[2])
    return np.frombuffer(api.resample_blur_host(raster, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=bool(flip), filter=filt, colour=col,
                                                blur=rec), BITS[dtype])


@pytest.mark.gpu
def test_one_blurred_view_in_one_tile_of_a_two_tile_image(gpu, po):
    """The smallest case: the lower tile of a 200 x 2000 image alone."""
    from xpng_amd.synth import synth_raster
    r = synth_raster("photo", 200, 2000, False, seed=5)
    blob = po.encode_tiles(1, r)
    ctx = gpu.MixedContext([(200, 2000)], 3)
    try:
        assert ctx.n_tiles == 2 and ctx.tile(1) == (0, 1015, 200, 985)
        word = api.layout(planar=True, channels=3)
        scale, bias = mixed_consts(F16)
        d_b = _upload([blob])
        for filt, col, rec in ((2, None, (2.0, 11, None)), (1, PERM, (0.7, 3, 128.0)), (0, None, (0.0, 0, 100.0))):
            views = [(0, (0, 1100, 200, 800), 0, (37, 29), rec)]
            got = run_blur(ctx, 1, d_b, [len(blob)], views, word, F16, scale, bias, filt, colours=col and [col])
            assert ctx.last_decode_tiles() == 1
            assert np.array_equal(got[0], host_rule(r, views[0], col, word, F16, scale, bias, filt)), (filt, rec)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_views_blur_bits(gpu, batches, mode, alpha, dtype, filt):
    """Every element of every view equals api.resample_blur_host and every sentinel is intact, for all 12 layout words (interleaved
    and planar, BGR, C 3 and 4), with and without matrices, in calls that mix plain, blurred, solarise-only and blurred-and-solarised
    views of radii 0, 1, 11 and 31; the launch held exactly the tiles of api.view_tiles."""
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for wi, word in enumerate(WORDS):
            p, with_cols = (wi + filt) % 2, (wi // 2 + filt) % 2 == 1
            views = _views(dims, p)
            vi, rects, _, _, recs = view_args(views)
            assert len(views) > len(dims) and (3, 0)[p] not in vi and {r and r[1] for r in recs} >= {None, 0, 1, 11, 31}
            sel = api.view_tiles(dims, vi, rects)
            colours = [[PERM, RANGE, DENSE, None][(v + wi) % 4] for v in range(len(views))] if with_cols else None
            got = run_blur(ctx, mode, d_b, lens, views, word, dtype, scale, bias, filt, colours=colours)
            assert ctx.last_decode_tiles() == len(sel) < ctx.n_tiles
            for v, view in enumerate(views):
                col = (colours[v] or list(api.COLOUR_IDENTITY)) if colours else None
                w = host_rule(rasters[view[0]], view, col, word, dtype, scale, bias, filt)
                assert np.array_equal(got[v], w), (hex(word), dtype, filt, p, v, view, with_cols, np.argwhere(got[v] != w)[:4].ravel())
    finally:
        ctx.close()


@pytest.mark.gpu
def test_blur_off_is_the_underlying_call_and_the_workspace(gpu, po):
    """blurs=None and all-off records give the bytes of the underlying call and allocate nothing beyond it.  The first call with
    second-pass views grows the workspace by the scratch (C * oh * ow floats per such view, each slice rounded up to 256 bytes) and
    160 bytes per such view; a smaller call after it grows nothing; two calls in a row with different views and sizes each get
    their own bits."""
    from xpng_amd.synth import synth_raster
    dims = [(17, 4), (64, 64), (130, 90), (100, 110), (5, 7)]
    rasters = [synth_raster(["photo", "noise", "gray"][i % 3], w, h, False, seed=i + 40) for i, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(1, r) for r in rasters]
    r1 = [(0, 0, 17, 4), (3, 4, 50, 55), (10, 10, 110, 70), (0, 0, 100, 110), (1, 2, 3, 4)]
    flips = [1, 0, 1, 0, 1]
    dtype, word = F16, api.layout(planar=True, bgr=True, channels=4)
    scale, bias = mixed_consts(dtype)
    ctx = gpu.MixedContext(dims, 3)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        ident = list(range(len(dims)))
        n = len(dims)

        def under(filt, cols, sizes, ar):
            ar.refill()
            kw = dict(rects=r1, flips=flips, colours=cols)
            if filt == 2:
                ctx.decode_batch_views_cubic(1, ins, lens, ident, ar.ptrs, word, dtype, sizes, scale, bias, **kw)
            else:
                ctx.decode_batch_views(1, ins, lens, ident, ar.ptrs, word, dtype, sizes, scale, bias, filter=filt, **kw)
            assert ctx.decode_status() == 0
            return [g.copy() for g in ar.fetch()]

        def blur(filt, cols, sizes, ar, blurs):
            ar.refill()
            ctx.decode_batch_views_blur(1, ins, lens, ident, ar.ptrs, word, dtype, sizes, scale, bias, rects=r1, flips=flips, filter=filt, colours=cols, blurs=blurs)
            assert ctx.decode_status() == 0
            return [g.copy() for g in ar.fetch()]

        s1 = [(13, 21)] * n
        ar = Arena([2 * 4 * oh * ow for (oh, ow) in s1], 2)
        for filt in (0, 1, 2):
            for cols in (None, [DENSE] * n):
                want = under(filt, cols, s1, ar)
                ws = ctx.workspace_bytes()
                for blurs in (None, [None] * n, [OFF] * n):
                    got = blur(filt, cols, s1, ar, blurs)
                    assert all(np.array_equal(a, b) for a, b in zip(got, want)), (filt, cols is None, blurs)
                    assert ctx.workspace_bytes() == ws
        ws = ctx.workspace_bytes()
        # the first call with second-pass views: views 1, 2 and 4 of five
        recs_a = [None, (2.0, 5, None), (0.0, 0, 128.0), OFF, (1.0, 3, 64.0)]
        got_a = blur(2, None, s1, ar, recs_a)
        slice_a = -(-(4 * 13 * 21 * 4) // 256) * 256
        assert ctx.workspace_bytes() - ws == 3 * slice_a + 3 * 160
        # other sizes, other views, less scratch: nothing grows, and every view gets its own bits
        s2 = [(7, 9), (16, 64), (9, 7), (17, 33), (12, 12)]
        ar2 = Arena([2 * 4 * oh * ow for (oh, ow) in s2], 2)
        recs_b = [(0.5, 1, None), None, (3.0, 6, 0.0), (0.0, 0, 255.0), None]
        got_b = blur(1, [PERM] * n, s2, ar2, recs_b)
        got_a2 = blur(2, None, s1, ar, recs_a)
        assert ctx.workspace_bytes() - ws == 3 * slice_a + 3 * 160
        for i, r in enumerate(rasters):
            a = np.frombuffer(api.resample_blur_host(r, s1[i], word, dtype, scale, bias, rect=r1[i], flip=bool(flips[i]), filter=2, blur=recs_a[i]), np.uint8)
            b = np.frombuffer(api.resample_blur_host(r, s2[i], word, dtype, scale, bias, rect=r1[i], flip=bool(flips[i]), filter=1, colour=PERM, blur=recs_b[i]), np.uint8)
            assert np.array_equal(got_a[i], a) and np.array_equal(got_a2[i], a) and np.array_equal(got_b[i], b), i
        # a call that needs more grows it once more, and it stays
        s3 = [(40, 130)] * n
        ar3 = Arena([2 * 4 * oh * ow for (oh, ow) in s3], 2)
        recs_c = [(2.0, 11, None)] * n
        got_c = blur(0, None, s3, ar3, recs_c)
        slice_c = -(-(4 * 40 * 130 * 4) // 256) * 256
        assert ctx.workspace_bytes() - ws == n * slice_c + n * 160
        blur(2, None, s1, ar, recs_a)
        assert ctx.workspace_bytes() - ws == n * slice_c + n * 160
        for i, r in enumerate(rasters):
            c = np.frombuffer(api.resample_blur_host(r, s3[i], word, dtype, scale, bias, rect=r1[i], flip=bool(flips[i]), filter=0, blur=recs_c[i]), np.uint8)
            assert np.array_equal(got_c[i], c), i
    finally:
        ctx.close()


@pytest.mark.gpu
def test_blur_device_refusals_leave_the_sentinels(gpu, batches):
    dims, rasters, blobs = batches[(1, True)]
    word = api.layout(planar=True, channels=3)
    scale, bias = mixed_consts(F16)
    views = _views(dims, 1)
    ctx = gpu.MixedContext(dims, 4)
    try:
        vi, rects, flips, sizes, recs = view_args(views)
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        outs = Arena([4 * 4 * oh * ow for (oh, ow) in sizes], 4)
        ws = ctx.workspace_bytes()
        n = len(views)

        def refused(words, **kw):
            a = dict(mode=1, d_blobs=ins, lens=lens, view_image=vi, d_outs=outs.ptrs, layout=word, dtype=F16, sizes=sizes, scale=scale[:3], bias=bias[:3],
                     rects=rects, flips=flips, filter=2, blurs=recs)
            a.update(kw)
            for cols in (None, [DENSE] * n):
                with pytest.raises(gpu.XpngError) as e:
                    ctx.decode_batch_views_blur(colours=cols, **a)
                assert all(w in str(e.value) for w in words), (words, str(e.value))
                assert outs.untouched(), words

        def rec_at(v, rec):
            return recs[:v] + [rec] + recs[v + 1:]

        k = next(v for v, s in enumerate(sizes) if s == (29, 37))
        refused(["view %d" % k, "radius is 32"], blurs=rec_at(k, api.ViewBlur(1.0, 32, 256.0, 0)))
        refused(["view %d" % k, "radius 29", "37 x 29"], blurs=rec_at(k, (1.0, 29, None)))
        refused(["view %d" % k, "sigma is 0"], blurs=rec_at(k, (0.0, 2, None)))
        refused(["view %d" % k, "sigma is 3", "radius 0"], blurs=rec_at(k, (3.0, 0, 10.0)))
        refused(["view %d" % k, "sigma is nan"], blurs=rec_at(k, (float("nan"), 2, None)))
        refused(["view %d" % k, "sigma is 2048"], blurs=rec_at(k, (2048.0, 2, None)))
        refused(["view %d" % k, "solarise is 300"], blurs=rec_at(k, (1.0, 2, 300.0)))
        refused(["view %d" % k, "solarise is nan"], blurs=rec_at(k, (1.0, 2, float("nan"))))
        refused(["view %d" % k, "reserved is 1"], blurs=rec_at(k, api.ViewBlur(1.0, 2, 256.0, 1)))
        refused(["filter 3"], filter=3)
        refused(["blurs has 2 entries"], blurs=recs[:2])
        # everything the underlying call refuses
        refused(["view_image[2]", "is 6", "6 images"], view_image=vi[:2] + [6] + vi[3:])
        refused(["{0, 0, 18, 4}", "17 x 4"], rects=[r if i != 1 else (0, 0, 18, 4) for i, r in zip(vi, rects)])
        refused(["16385 x 29", "view 5"], sizes=sizes[:5] + [(29, 16385)] + sizes[6:])
        refused(["flip 2", "view 1"], flips=[0, 2] + flips[2:])
        refused(["out_sizes is NULL"], sizes=None)
        refused(["null", "view 1"], d_outs=[outs.ptrs[0], 0] + outs.ptrs[2:])
        refused(["dtype 4"], dtype=4)
        refused(["layout", "0x500"], layout=0x500)
        refused(["scale[1]", "nan"], scale=[1.0, float("nan"), 1.0])
        refused(["mode 2", "RGB"], mode=2)
        refused(["null blob", "image 1"], d_blobs=[ins[0], 0] + ins[2:])
        assert outs.untouched() and ctx.workspace_bytes() == ws     # nothing was allocated for a refused call
        # the other views calls keep the filter's domain
        with pytest.raises(gpu.XpngError) as e:
            ctx.decode_batch_views(1, ins, lens, vi, outs.ptrs, word, F16, sizes, scale[:3], bias[:3], rects=rects, flips=flips, filter=2)
        assert "filter 2" in str(e.value) and outs.untouched()
        # the context still works after all that
        got = run_blur(ctx, 1, d_b, lens, views, word, F16, scale, bias, 2)
        for v, view in enumerate(views):
            assert np.array_equal(got[v], host_rule(rasters[view[0]], view, None, word, F16, scale, bias, 2)), v
    finally:
        ctx.close()


@pytest.mark.gpu
def test_load_views_blur_on_goldens(gpu):
    """Two views per reference-written file with random_colour_jitter matrices, random_gaussian_blur and random_solarise entries:
    every view equals api.resample_blur_host of api.load of its file, with both interpolations."""
    import torch
    from xpng_amd import tensors
    paths = sorted(p for p in glob.glob(os.path.join(GOLD, "imgfull_*.xpng")) if 11 < os.path.getsize(p) < 200000)[:6]
    assert len(paths) == 6
    want = [gpu.load(p) for p in paths]
    dims = [(r.shape[1], r.shape[0]) for r in want]
    g = torch.Generator().manual_seed(22)
    used = [0, 1, 2, 3, 5]                                          # file 4 has no view
    big_r = tensors.random_resized_crops([dims[i] for i in used], generator=g)
    small_r = tensors.random_resized_crops([dims[i] for i in used], scale=(0.05, 0.14), generator=g)
    views = [(i, r, k % 2 == 1) for k, (i, r) in enumerate(zip(used, big_r))] + [(i, r, k % 2 == 0) for k, (i, r) in enumerate(zip(used, small_r))]
    cols = tensors.random_colour_jitter(len(views), p=0.9, gray_p=0.3, generator=g)
    blur = tensors.random_gaussian_blur(len(views), kernel_size=23, p=0.6, generator=g)
    sol = tensors.random_solarise(len(views), p=0.4, generator=g)
    blur[0], sol[0], blur[1], sol[1], blur[2], sol[2] = (1.7, 23), 128.0, None, None, None, 128.0
    scale, bias = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    for lay, bgr, dtype, interp in (("chw", False, F16, "bicubic"), ("hwc", True, F32, "bilinear"), ("chw", True, BF16, "bicubic")):
        kw = dict(layout=lay, channels=3, bgr=bgr, dtype=_torch_dtype(dtype), mean=IMAGENET_MEAN, std=IMAGENET_STD, interpolation=interp)
        whole = tensors.load_views(paths, views, (32, 48), stack=True, colour=cols, blur=blur, solarise=sol, **kw)
        assert whole.is_cuda and tuple(whole.shape) == (10,) + ((3, 32, 48) if lay == "chw" else (32, 48, 3))
        word = api.layout(planar=lay == "chw", bgr=bgr, channels=3)
        for v, (i, rect, flip) in enumerate(views):
            rec = None if blur[v] is None and sol[v] is None else ((blur[v][0], blur[v][1] // 2) if blur[v] else (0.0, 0)) + (sol[v],)
            raw = api.resample_blur_host(want[i], (32, 48), word, dtype, scale, bias, rect=rect, flip=flip, filter=2 if interp == "bicubic" else 1,
                                         colour=cols[v], blur=rec)
            assert np.array_equal(_bits(whole[v], dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), (lay, v, paths[i], rect)
        plain = tensors.load_views(paths, views, (32, 48), stack=True, colour=cols, **kw)
        assert torch.equal(plain[1], whole[1]) and not torch.equal(plain[0], whole[0]) and not torch.equal(plain[2], whole[2])
