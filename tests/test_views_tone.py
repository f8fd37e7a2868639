"""Autocontrast, equalise, posterise, solarise and invert per view in a views decode (include/xpng_hip.h xpnghip_view_tone,
xpnghip_resample_tone_host, xpnghip_resample_affine_tone_host, xpnghip_decode_varsize_device_batch_views_tone,
xpnghip_decode_varsize_device_batch_views_affine_tone; xpng_amd/tensors.py load_views(tone=), random_tone).

CPU: the symbols; both host rules against the independent checker (tests/_tone.py) on the bits, over the sizes, step lists and
planes that take every branch of the rule; equalise, posterise, solarise and invert against PIL; autocontrast against its float64
statement; every refusal; load_views on host-answered files without a GPU; random_tone.  GPU: every view of both device calls
against the checker's bits."""
import ctypes as C
import glob
import itertools
import os

import numpy as np
import pytest

import _tone
from _kit import (BF16, BITS, DTYPES, ES, F16, F32, FORMATS, IMAGENET_MEAN, IMAGENET_STD, Arena, _bits, _torch_dtype, _upload, consts_from, declared, exported,
                  gpu, mixed_consts, po)
from _tone import AUTOCONTRAST, EQUALISE, INVERT, NONE, POSTERISE, SOLARISE, AffineToned, Toned
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_resample_tone_host", "xpnghip_resample_affine_tone_host", "xpnghip_decode_varsize_device_batch_views_tone",
       "xpnghip_decode_varsize_device_batch_views_affine_tone"]
WORDS = [api.layout(planar=p, bgr=b, channels=c) for c in (0, 3, 4) for p in (False, True) for b in (False, True)]
PERM = [0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0]
RANGE = [3, -2, 0.5, -300, -2, 3, 0, 300, 1, 1, -2, 40]            # leaves 0 .. 255 on both sides: the entry clamp is taken
DENSE = [0.70710678, -0.31830989, 0.57721566, 12.345678, 0.14142135, 1.6180339, -0.69314718, -7.3890561, -0.43429448, 0.26179939, 1.2020569,
         31.415926]
AC, EQ, INV = (AUTOCONTRAST, 0.0), (EQUALISE, 0.0), (INVERT, 0.0)
SINGLES = [AC, EQ, (POSTERISE, 3.0), (SOLARISE, 128.0), INV]
# each op alone, every ordered pair, a four-step list, posterise with 0, 1, 4 and 8 bits, solarise at 0, 100.5 and 255
STEP_LISTS = ([[s] for s in SINGLES] + [list(p) for p in itertools.product(SINGLES, repeat=2)] + [[EQ, (SOLARISE, 100.5), AC, (POSTERISE, 2.0)]] +
              [[(POSTERISE, float(k))] for k in (0, 1, 4, 8)] + [[(SOLARISE, t)] for t in (0.0, 100.5, 255.0)])
# (OW, OH): degenerate axes; 240 pixels (equalise's step is 0); 256 pixels; every edge of the blur kernel's 64 x 16 tile; several tiles
WARP = [0.9, 0.35, -3.0, -0.3, 0.95, 2.0]                          # a rotation with a shear: fill in the corners
SIZES = [(1, 1), (1, 300), (300, 1), (15, 16), (16, 16)] + [(w, h) for w in (63, 64, 65) for h in (15, 16, 17)] + [(130, 40)]


def _shape(word, px, OW, OH):
    ch = (word >> 8) or px
    return (ch, OH, OW) if word & 1 else (OH, OW, ch)


def _lib(r, rect, flip, OW, OH, word, dtype, scale, bias, filt, colour=None, blur=None, tone=None):
    ch = (word >> 8) or r.shape[2]
    raw = api.resample_tone_host(r, (OH, OW), word, dtype, scale[:ch], bias[:ch], rect=rect, flip=flip, filter=filt, colour=colour, blur=blur, tone=tone)
    return np.frombuffer(raw, BITS[dtype]).reshape(_shape(word, r.shape[2], OW, OH))


def _lib_affine(r, m, OW, OH, word, dtype, scale, bias, filt, fill=None, colour=None, tone=None):
    ch = (word >> 8) or r.shape[2]
    raw = api.resample_affine_tone_host(r, (OH, OW), m, word, dtype, scale[:ch], bias[:ch], filter=filt, fill=fill, colour=colour, tone=tone)
    return np.frombuffer(raw, BITS[dtype]).reshape(_shape(word, r.shape[2], OW, OH))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_tone_symbols_are_declared_listed_and_exported():
    assert set(NEW) <= set(declared("xpng_hip.h", "xpnghip_")) and set(NEW) <= set(api.HIP_SYMBOLS) and set(NEW) <= exported(api.HIP_SO)
    assert api.hip_lib().xpnghip_abi_version() == 2
    import xpng_amd
    from xpng_amd import tensors
    for name in ("ViewTone", "resample_tone_host", "resample_affine_tone_host", "TONE_NONE", "TONE_AUTOCONTRAST", "TONE_EQUALISE", "TONE_POSTERISE",
                 "TONE_SOLARISE", "TONE_INVERT"):
        assert name in xpng_amd.__all__ and hasattr(xpng_amd, name)
    assert (api.TONE_NONE, api.TONE_AUTOCONTRAST, api.TONE_EQUALISE, api.TONE_POSTERISE, api.TONE_SOLARISE, api.TONE_INVERT) == (0, 1, 2, 3, 4, 5)
    assert (NONE, AUTOCONTRAST, EQUALISE, POSTERISE, SOLARISE, INVERT) == (0, 1, 2, 3, 4, 5)
    assert callable(api.MixedContext.decode_batch_views_tone) and callable(api.MixedContext.decode_batch_views_affine_tone) and callable(tensors.random_tone)
    assert C.sizeof(api.ViewTone) == 20
    hdr = open(os.path.join(ROOT, "include", "xpng_hip.h")).read()
    for line in ("typedef struct { uint8_t op[4]; float arg[4]; } xpnghip_view_tone;   /* 20 bytes */",
                 "#define XPNGHIP_TONE_NONE 0u          /* arg 0 */",
                 "#define XPNGHIP_TONE_AUTOCONTRAST 1u  /* arg 0 */",
                 "#define XPNGHIP_TONE_EQUALISE 2u      /* arg 0 */",
                 "#define XPNGHIP_TONE_POSTERISE 3u     /* arg = bits, an integer 0 .. 8 */",
                 "#define XPNGHIP_TONE_SOLARISE 4u      /* arg = threshold, 0 .. 255 */",
                 "#define XPNGHIP_TONE_INVERT 5u        /* arg 0 */"):
        assert line in hdr, line
    assert "#define XPNGHIP_ABI_VERSION 2 " in hdr


def _identity_raster(rng, OW, OH):
    """a raster of the output's size, so that filter 0 hands over the file's bytes: R random in 10 .. 200 except its LAST pixel, the
    plane's only 255; G constant (hi == lo); B two-valued; alpha random"""
    r = np.empty((OH, OW, 4), np.uint8)
    r[..., 0] = rng.integers(10, 201, (OH, OW))
    r[-1, -1, 0] = 255
    r[..., 1] = 77
    r[..., 2] = np.where(rng.integers(0, 2, (OH, OW)) == 1, 30, 201)
    r[..., 3] = rng.integers(0, 256, (OH, OW))
    return r


def test_both_host_rules_equal_the_checker():
    """Per size four sources of planes - the file's own bytes (a constant plane, a two-valued plane, a plane whose only extreme is its
    last pixel; at 16 x 16 a plane with most pixels in its highest bin), a triangle resample through a matrix that leaves 0 .. 255
    on both sides, a cubic resample behind a blur record, an affine warp with fill - and per source EVERY step list; the layout
    words and dtypes turn over the cases."""
    rng = np.random.default_rng(41)
    k, seen, clamped, step0 = 0, set(), 0, 0
    for (OW, OH) in SIZES:
        ident = _identity_raster(rng, OW, OH)
        if (OW, OH) == (16, 16):
            ident[..., 0] = 255                                     # 250 pixels in the highest bin: step = (256 - 250) / 255 = 0
            ident[0, :6, 0] = [0, 50, 100, 150, 200, 250]
        big = rng.integers(0, 256, (OH + 5, OW + 7, 3), dtype=np.uint8)
        R, afilt = min(2, OW - 1, OH - 1), 3 * (k % 2)
        sources = [Toned(ident, None, False, OH, OW, 0),
                   Toned(big, (1, 2, OW + 5, OH + 2), True, OH, OW, 1, RANGE),
                   Toned(big, None, False, OH, OW, 2, DENSE, (1.5, R, 100.5) if R else (0.0, 0, 100.5)),
                   AffineToned(ident, WARP, OH, OW, afilt, [10, 200.5, 30, 40], PERM)]
        clamped += int((sources[1].under[..., :3] == 0).any() and (sources[1].under[..., :3] == 255).any())
        for si, src in enumerate(sources):
            for steps in STEP_LISTS:
                src.retone(steps)
                word, dtype = WORDS[k % 12], DTYPES[(k // 12) % 3]
                k += 5
                seen.add((word, dtype))
                scale, bias = mixed_consts(dtype)
                if si == 0:
                    got = _lib(ident, None, False, OW, OH, word, dtype, scale, bias, 0, tone=steps)
                    if steps == [EQ] and OW * OH <= 256:
                        assert np.array_equal(src.v, src.under)     # step == 0: the plane is unchanged
                        step0 += 1
                elif si == 1:
                    got = _lib(big, (1, 2, OW + 5, OH + 2), True, OW, OH, word, dtype, scale, bias, 1, RANGE, None, steps)
                elif si == 2:
                    got = _lib(big, None, False, OW, OH, word, dtype, scale, bias, 2, DENSE, (1.5, R, 100.5) if R else (0.0, 0, 100.5), steps)
                else:
                    got = _lib_affine(ident, WARP, OW, OH, word, dtype, scale, bias, afilt, [10, 200.5, 30, 40], PERM, steps)
                exp = src.bits(word, dtype, scale, bias)
                assert got.shape == exp.shape and np.array_equal(got, exp), ((OW, OH), si, steps, hex(word), dtype)
        k += 1
    assert len(seen) == 36 and clamped >= 10 and step0 == 3            # 1 x 1, 15 x 16 and 16 x 16


def test_none_and_all_none_are_the_underlying_rules():
    rng = np.random.default_rng(3)
    r = rng.integers(0, 256, (31, 45, 4), dtype=np.uint8)
    m = [1.1, 0.2, -4.0, -0.2, 1.05, 3.0]
    for word, dtype in ((WORDS[3], F16), (WORDS[8], BF16), (WORDS[5], F32)):
        scale, bias = mixed_consts(dtype)
        ch = (word >> 8) or 4
        for filt in (0, 1, 2):
            plain = api.resample_blur_host(r, (13, 17), word, dtype, scale[:ch], bias[:ch], rect=(2, 3, 40, 25), flip=True, filter=filt, colour=DENSE, blur=(1.0, 2, 90.0))
            for tone in (None, [], [(NONE, 0.0)] * 4):
                assert api.resample_tone_host(r, (13, 17), word, dtype, scale[:ch], bias[:ch], rect=(2, 3, 40, 25), flip=True, filter=filt, colour=DENSE,
                                              blur=(1.0, 2, 90.0), tone=tone) == plain
        for filt in (0, 3):
            plain = api.resample_affine_host(r, (13, 17), m, word, dtype, scale[:ch], bias[:ch], filter=filt, fill=[1, 2, 3, 4], colour=DENSE)
            for tone in (None, [], [(NONE, 0.0)] * 4):
                assert api.resample_affine_tone_host(r, (13, 17), m, word, dtype, scale[:ch], bias[:ch], filter=filt, fill=[1, 2, 3, 4], colour=DENSE, tone=tone) == plain
    # alpha passes through untouched, and the fill takes part in the statistics
    word = api.layout(planar=True, channels=4)
    one, zero = [1.0] * 4, [0.0] * 4
    base = _lib(r, None, False, 45, 31, word, F32, one, zero, 0).view(np.float32)
    got = _lib(r, None, False, 45, 31, word, F32, one, zero, 0, tone=[EQ, INV, AC]).view(np.float32)
    assert np.array_equal(got[3], base[3]) and not np.array_equal(got[:3], base[:3])
    dark = np.full((9, 9, 3), 100, np.uint8)
    out = _lib_affine(dark, [1, 0, -2, 0, 1, 0], 9, 9, api.layout(planar=True, channels=3), F32, one, zero, 0, fill=[200, 200, 200, 0], tone=[AC]).view(np.float32)
    assert out.min() == 0.0 and out.max() == 255.0                  # without the fill the plane would be constant and stay 100


def test_integer_steps_equal_pil():
    """On an identity resample the planes are the file's bytes: equalise, posterise, solarise and invert, and pairs of them, equal
    PIL's ImageOps per band, value for value."""
    from PIL import Image, ImageOps
    rng = np.random.default_rng(17)
    ops = {"eq": (EQ, ImageOps.equalize), "inv": (INV, ImageOps.invert)}
    for kbits in range(1, 9):
        ops["post%d" % kbits] = ((POSTERISE, float(kbits)), lambda im, kbits=kbits: ImageOps.posterize(im, kbits))
    for thr in (0, 77, 128, 255):
        ops["sol%d" % thr] = ((SOLARISE, float(thr)), lambda im, thr=thr: ImageOps.solarize(im, thr))
    names = sorted(ops)
    lists = [[n] for n in names] + [[a, b] for a in ("eq", "inv", "post3", "sol128", "post8", "sol77") for b in ("eq", "inv", "post2", "sol128")]
    word = api.layout(planar=True, channels=3)
    for (w, h), kind in (((69, 41), "uniform"), ((64, 16), "narrow"), ((33, 50), "gauss"), ((16, 15), "uniform"), ((40, 40), "four"), ((1, 1), "uniform"), ((300, 1), "narrow")):
        if kind == "uniform":
            r = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif kind == "narrow":
            r = rng.integers(90, 131, (h, w, 3), dtype=np.uint8)
        elif kind == "gauss":
            r = np.clip(rng.normal(120, 30, (h, w, 3)), 0, 255).astype(np.uint8)
        else:
            r = rng.choice(np.array([3, 80, 81, 250], np.uint8), (h, w, 3))
        for lst in lists:
            got = _lib(r, None, False, w, h, word, F32, [1.0] * 3, [0.0] * 3, 0, tone=[ops[n][0] for n in lst]).view(np.float32)
            for band in range(3):
                im = Image.fromarray(np.ascontiguousarray(r[..., band]), "L")
                for n in lst:
                    im = ops[n][1](im)
                assert np.array_equal(got[band], np.asarray(im).astype(np.float32)), ((w, h), kind, lst, band)


# measured here on the CPU over the cases below, on the values the LIBRARY's rule writes (xpnghip_resample_tone_host, f32 planes,
# identity constants): the largest difference between its autocontrast and the float64 statement (x - lo) * 255 / (hi - lo) is
# 2.01e-5 of a byte step; four times that is 8.03e-5 and the next power of two above it 2^-13 = 1.22e-4.
# The margin covers the fp32 rounding of s on other inputs
AUTOCONTRAST_BOUND = 2.0 ** -13


def test_autocontrast_against_its_float64_statement():
    rng = np.random.default_rng(29)
    worst = 0.0
    word = api.layout(planar=True, channels=3)
    one, zero = [1.0] * 3, [0.0] * 3
    for (w, h), (OW, OH), filt, colour in (((45, 31), (29, 37), 1, None), ((130, 9), (12, 12), 2, DENSE), ((17, 4), (32, 32), 0, None), ((45, 31), (64, 40), 2, RANGE),
                                           ((64, 64), (64, 64), 0, None), ((130, 90), (23, 24), 1, PERM), ((9, 9), (130, 40), 0, DENSE)):
        r = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if (w, h) == (64, 64):
            r = (r // 3 + 60).astype(np.uint8)
        under = _lib(r, None, False, OW, OH, word, F32, one, zero, filt, colour, None, None).view(np.float32)
        got = _lib(r, None, False, OW, OH, word, F32, one, zero, filt, colour, None, [AC]).view(np.float32)
        for q in range(3):
            x = np.clip(under[q].astype(np.float64), 0.0, 255.0)
            lo, hi = x.min(), x.max()
            assert hi > lo
            d = float(np.abs((x - lo) * 255.0 / (hi - lo) - got[q].astype(np.float64)).max())
            print("autocontrast vs float64", (w, h), (OW, OH), filt, q, d)
            worst = max(worst, d)
            assert d <= AUTOCONTRAST_BOUND, ((w, h), (OW, OH), filt, q, d)
            assert got[q].min() == 0.0 and got[q].max() <= 255.0
    print("autocontrast vs float64, worst", worst)


def test_autocontrast_with_an_infinite_scale_leaves_the_plane():
    """A colour matrix may shrink a plane until 255.0f / (hi - lo) overflows: the plane is then unchanged, no NaN is made, and a
    following equalise sees finite values.  Library and checker agree on the bits."""
    rng = np.random.default_rng(2)
    r = rng.integers(10, 31, (9, 11, 3), dtype=np.uint8)          # a range of at most 20 bytes, times 2e-38: below 7.5e-37
    tiny = [2e-38, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    word = api.layout(planar=True, channels=3)
    one, zero = [1.0] * 3, [0.0] * 3
    under = _lib(r, None, False, 11, 9, word, F32, one, zero, 0, tiny).view(np.float32)
    assert 0.0 < under[0].max() - under[0].min() < 7.5e-37
    for steps in ([AC], [AC, EQ], [AC, INV, AC], [EQ, AC, EQ, AC]):
        got = _lib(r, None, False, 11, 9, word, F32, one, zero, 0, tiny, None, steps)
        exp = Toned(r, None, False, 9, 11, 0, tiny, None, steps).bits(word, F32, one, zero)
        assert np.array_equal(got, exp), steps
        assert np.isfinite(got.view(np.float32)).all()
    got = _lib(r, None, False, 11, 9, word, F32, one, zero, 0, tiny, None, [AC]).view(np.float32)
    assert np.array_equal(got[0], under[0]) and got[1].min() == 0.0 and got[1].max() == 255.0


BAD_TONES = [([(6, 0.0)], ["step 0", "op is 6"]), ([AC, (255, 0.0)], ["step 1", "op is 255"]),
             ([AC, (NONE, 0.0), INV], ["step 2", "invert follows", "NONE"]), ([(NONE, 0.0), EQ], ["step 1", "equalise follows"]),
             ([(AUTOCONTRAST, 1.0)], ["step 0", "arg is 1", "autocontrast"]), ([EQ, (EQUALISE, -2.0)], ["step 1", "arg is -2", "equalise"]),
             ([(INVERT, float("nan"))], ["step 0", "arg is nan", "invert"]), ([INV, (NONE, 3.0)], ["step 1", "arg is 3", "none"]),
             ([(POSTERISE, 9.0)], ["step 0", "bits are 9", "0 .. 8"]), ([(POSTERISE, 2.5)], ["step 0", "bits are 2.5"]),
             ([AC, EQ, INV, (POSTERISE, -1.0)], ["step 3", "bits are -1"]), ([(POSTERISE, float("nan"))], ["step 0", "bits are nan"]),
             ([(SOLARISE, 255.5)], ["step 0", "threshold is 255.5"]), ([INV, (SOLARISE, -0.5)], ["step 1", "threshold is -0.5"]),
             ([(SOLARISE, float("nan"))], ["threshold is nan"]), ([(SOLARISE, float("inf"))], ["threshold is inf"])]


def test_host_rule_refusals():
    lib = api.hip_lib()
    r = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    out = np.full(4 * 4 * 4 * 4 + 4, 0x5A5A5A5A, np.uint32)
    one, zero = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0)
    u64 = C.c_uint64
    good = api._tone_record("t", [EQ, AC])

    def call(pxsz=3, raster=r.ctypes.data, w=7, h=5, rect=None, flip=0, ow=4, oh=4, layout=0, dtype=F32, scale=one, bias=zero, filt=1, colour=None,
             blur=(1.0, 2, 256.0, 0), tone=good, o=None, affine=False):
        ra = None if rect is None else (u64 * 4)(*rect)
        cm = None if colour is None else (C.c_float * 12)(*colour)
        br = None if blur is None else C.byref(api.ViewBlur(*blur))
        tr = None if tone is None else C.byref(tone)
        dst = out.ctypes.data if o is None else o
        if affine:
            return lib.xpnghip_resample_affine_tone_host(pxsz, raster, w, h, (C.c_float * 6)(1, 0, 0, 0, 1, 0), ow, oh, layout, dtype, scale, bias, 3 if filt == 1 else filt,
                                                         None, cm, tr, dst)
        return lib.xpnghip_resample_tone_host(pxsz, raster, w, h, ra, flip, ow, oh, layout, dtype, scale, bias, filt, cm, br, tr, dst)

    def refused(words, both=True, **kw):
        for affine in ((False, True) if both else (False,)):
            assert call(affine=affine, **kw) != 0, kw
            msg = api._err()
            assert all(w in msg for w in words), (words, msg)

    assert call() == 0 and call(affine=True) == 0 and call(tone=None) == 0
    out[:] = 0x5A5A5A5A
    for steps, words in BAD_TONES:
        refused(["bad tone"] + words, tone=api._tone_record("t", steps))
    # everything the underlying calls refuse, with a tone record that has steps
    refused(["filter 4"], filt=4)
    refused(["radius 4", "4 x 4"], both=False, blur=(1.0, 4, 256.0, 0))
    refused(["{0, 0, 0, 3}", "7 x 5"], both=False, rect=(0, 0, 0, 3))
    refused(["flip 2"], both=False, flip=2)
    refused(["4 x 0", "16384"], oh=0)
    refused(["dtype 4"], dtype=4)
    refused(["layout", "0x500"], layout=0x500)
    refused(["scale[1]", "nan"], scale=(C.c_float * 4)(1, float("nan"), 1, 1))
    refused(["null"], raster=None)
    refused(["null"], o=0)
    refused(["aligned"], o=out.ctypes.data + 2)
    refused(["pxsz is 5"], pxsz=5)
    mbad = list(DENSE)
    mbad[6] = float("nan")
    refused(["[1][2]", "colour"], colour=mbad)
    assert (out == 0x5A5A5A5A).all()                                # a refused call writes nothing
    for bad in ("autocontrast", [(1, 0.0)] * 5, [(1, "x")], 7):
        with pytest.raises(api.XpngError) as e:
            api.resample_tone_host(r, (4, 4), 0, F32, tone=bad)
        assert "tone entry" in str(e.value)
    # the device entry points refuse a bad filter and a NULL context like their siblings
    p1, n1 = (C.c_void_p * 1)(0), (u64 * 1)(0)
    args = (None, 1, p1, n1, 1, None, 1, None, p1, (C.c_uint32 * 2)(4, 4), None, None, 0, F16, None, None)
    assert lib.xpnghip_decode_varsize_device_batch_views_tone(*args, 3, None, None, None, None) != 0 and "filter 3" in api._err()
    assert lib.xpnghip_decode_varsize_device_batch_views_tone(*args, 2, None, None, None, None) != 0 and "null context" in api._err()
    assert lib.xpnghip_decode_varsize_device_batch_views_affine_tone(*args, 0, None, None, None) != 0 and "null context" in api._err()


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


NAMED = [["equalise", ("solarise", 100.5)], None, ["autocontrast"], [("posterise", 3), "equalise", "invert", "autocontrast"], ["invert"], [("posterise", 0)]]
NAMED_STEPS = [[EQ, (SOLARISE, 100.5)], None, [AC], [(POSTERISE, 3.0), EQ, INV, AC], [INV], [(POSTERISE, 0.0)]]


def test_load_views_tone_answers_host_kinds_without_a_gpu(po, tmp_path):
    import torch
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    views = [(0, (1, 2, 23, 34), True), (2, None, False), (0, None, False), (1, (100, 200, 300, 150), False), (2, (3, 1, 35, 5), True),
             (0, (23, 35, 1, 1), False)]
    sizes = [(6, 5), (3, 7), (40, 30), (12, 12), (9, 4), (1, 1)]   # (OH, OW): per-view sizes
    cols = [PERM, None, RANGE, None, np.asarray(DENSE).reshape(3, 4), None]
    blur = [(1.5, 5), None, (2.0, 23), None, None, None]
    sol = [None, 128, None, None, None, None]
    recs = [(1.5, 2, None), (0.0, 0, 128.0), (2.0, 11, None), None, None, None]
    mean, std = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)
    ident = list(api.COLOUR_IDENTITY)
    for dtype in DTYPES:
        for ch, lay, bgr, interp in ((3, "chw", False, "bicubic"), (4, "hwc", True, "bilinear")):
            scale, bias = consts_from(mean[:ch], std[:ch])
            word = api.layout(planar=lay == "chw", bgr=bgr, channels=ch)
            kw = dict(layout=lay, channels=ch, bgr=bgr, device="cpu", dtype=_torch_dtype(dtype), mean=mean[:ch], std=std[:ch], interpolation=interp)
            filt = 2 if interp == "bicubic" else 1
            got = tensors.load_views(paths, views, sizes, colour=cols, blur=blur, solarise=sol, tone=NAMED, **kw)
            plain = tensors.load_views(paths, views, sizes, colour=cols, blur=blur, solarise=sol, **kw)
            for v, ((i, rect, flip), (oh, ow)) in enumerate(zip(views, sizes)):
                exp = Toned(want[i], rect, flip, oh, ow, filt, cols[v] if cols[v] is not None else ident, recs[v], NAMED_STEPS[v]).bits(word, dtype, scale, bias)
                g = got[v]
                assert g.device.type == "cpu" and g.is_contiguous() and g.dtype == _torch_dtype(dtype) and tuple(g.shape) == exp.shape
                assert np.array_equal(_bits(g, dtype), exp), (dtype, ch, lay, v)
            assert torch.equal(got[1], plain[1]) and not torch.equal(got[0], plain[0]) and not torch.equal(got[2], plain[2])
            # with affine=: views without a rectangle
            aviews = [(0, None, False), (2, None, False), (1, None, False)]
            mats = [tensors.affine_matrix((0, 0, 25, 37), (20, 16), angle=30.0), None, tensors.affine_matrix((0, 0, 400, 300), (20, 16), angle=-10.0, scale=0.5)]
            tl = [[("posterise", 2), "autocontrast"], ["equalise", ("solarise", 64)], None]
            ts = [[(POSTERISE, 2.0), AC], [EQ, (SOLARISE, 64.0)], None]
            akw = dict(kw, interpolation="bilinear", antialias=False)
            got = tensors.load_views(paths, aviews, (20, 16), affine=mats, fill=[9, 100, 200, 50], tone=tl, **akw)
            for v, (i, _, _) in enumerate(aviews):
                m = mats[v] if mats[v] is not None else tensors.affine_matrix((0, 0, want[i].shape[1], want[i].shape[0]), (20, 16))
                exp = AffineToned(want[i], m, 20, 16, 0, [9, 100, 200, 50], None, ts[v]).bits(word, dtype, scale, bias)
                assert np.array_equal(_bits(got[v], dtype), exp), (dtype, ch, lay, v)
    o1 = [torch.zeros((3, 4, 4), dtype=torch.float16)]
    for tone, word in (([["sharpen"]], "a step is"), ([[("posterise", 9)]], "0 .. 8"), ([[("posterise", 2.5)]], "integer"), ([[("solarise", 256)]], "0 .. 255"),
                       ([["invert"] * 5], "at most four"), ([None, None], "2 entries"), (["invert"], "not one step"), ([[("invert", 1)]], "takes no argument"),
                       ([["posterise"]], "needs a number"), ([[("solarise", "x")]], "needs a number")):
        with pytest.raises(api.XpngError) as e:
            tensors.load_views(paths, [(0, None, False)], (4, 4), out=o1, device="cpu", tone=tone)
        assert word in str(e.value), (tone, str(e.value))
    assert float(o1[0].abs().sum()) == 0.0


def test_random_tone():
    import torch
    from xpng_amd import tensors
    g = torch.Generator().manual_seed(5)
    a = tensors.random_tone(300, generator=g)
    g = torch.Generator().manual_seed(5)
    assert a == tensors.random_tone(300, generator=g)
    # entry k depends on row k of the one draw alone: a shorter list is a prefix, and p only removes steps
    g = torch.Generator().manual_seed(5)
    half = tensors.random_tone(300, p=0.5, generator=g)
    g = torch.Generator().manual_seed(5)
    u = torch.rand((300, 2, 2), dtype=torch.float64, generator=g)
    names = ("autocontrast", "equalise", "posterise", "solarise")
    for k in range(300):
        full = [names[min(int(float(u[k, j, 0]) * 4), 3)] for j in range(2)]
        assert [s if isinstance(s, str) else s[0] for s in a[k]] == full
        kept = [full[j] for j in range(2) if float(u[k, j, 1]) < 0.5]
        assert [s if isinstance(s, str) else s[0] for s in (half[k] or [])] == kept
    flat = [s for e in a for s in e]
    assert {s if isinstance(s, str) else s[0] for s in flat} == set(names)
    # RandAugment's table: magnitude 9 of 31 bins
    assert ("posterise", 8 - round(9 * 4 / 30)) in flat and ("posterise", 7) in flat
    assert ("solarise", 255.0 * (1.0 - 9 / 30)) in flat
    for mag, bits, thr in ((0, 8, 255.0), (30, 4, 0.0), (15, 6, 127.5)):
        e = tensors.random_tone(50, ops=("posterise", "solarise"), magnitude=mag, generator=torch.Generator().manual_seed(1))
        assert {s for x in e for s in x} == {("posterise", bits), ("solarise", thr)}
    assert tensors.random_tone(3, p=0.0) == [None] * 3 and tensors.random_tone(2, num_ops=0) == [None] * 2
    assert all(len(e) == 4 for e in tensors.random_tone(5, num_ops=4, ops=("invert",)))
    for bad in (dict(num_ops=5), dict(ops=("sharpen",)), dict(ops=()), dict(magnitude=31), dict(magnitude=-1), dict(p=1.5), dict(num_magnitude_bins=1)):
        with pytest.raises(api.XpngError):
            tensors.random_tone(2, **bad)
    # what load_views takes
    for e in a[:20]:
        assert tensors._tone_steps("t", e) is not None


# ---- GPU ----------------------------------------------------------------------------------------------------------------
# tests/test_cubic.py's batches - the 889-wide image has a tile boundary inside the rectangles across x = 444 - plus one crafted
# 70 x 50 image: 3 * 3500 floats are one whole chunk of 8192 and a partial one, and the blue plane's extremes (0 and 255) and its
# fullest bin (200) lie only in the partial chunk
RGB_DIMS = [(3, 3), (17, 4), (64, 64), (445, 444), (889, 445), (100, 1100), (70, 50)]
RGBA_DIMS = [(4, 4), (17, 4), (64, 64), (445, 444), (889, 445), (100, 1100), (70, 50)]
CHUNK = 8192
FOUR = [EQ, (SOLARISE, 100.5), AC, (POSTERISE, 2.0)]               # two statistics steps, at indices 0 and 2
# (image, rectangle, flip, (OW, OH), blur record, steps): plain, blur-only, tone-only and blur-and-tone views side by side; 1 x 1 and
# 1 x 300; 65 x 17; 300 x 200 (23 chunks merge into one slot); the crafted image at its own size; four steps beside one step
TONE_VIEWS = [(0, None, 0, (37, 29), None, None),
              (1, (0, 0, 17, 4), 1, (12, 12), (3.7, 11, 200.0), None),
              (2, (2, 2, 60, 60), 0, (65, 17), None, [AC]),
              (2, (10, 20, 37, 29), 1, (63, 15), (2.0, 11, 128.0), [EQ]),
              (1, (16, 3, 1, 1), 0, (1, 1), None, [EQ, AC]),
              (4, (440, 100, 9, 200), 1, (1, 300), None, [AC, INV]),
              (4, (300, 100, 300, 200), 0, (300, 200), None, FOUR),
              (6, None, 0, (70, 50), None, [AC, EQ]),
              (6, None, 1, (70, 50), (0.0, 0, 90.0), [EQ, AC, INV]),
              (5, (3, 50, 90, 1000), 0, (64, 16), (1.0, 1, None), [(POSTERISE, 3.0)]),
              (3, (200, 140, 245, 304), 1, (130, 40), (9.5, 31, None), [INV, EQ, (SOLARISE, 0.0), EQ]),
              (5, (20, 30, 60, 500), 0, (3, 5), None, None),
              (4, (400, 50, 80, 300), 1, (64, 32), None, [(SOLARISE, 255.0)])]
# (image, matrix, (OW, OH), steps): a view wholly outside its image (all fill), fill in the corners of the others
AFFINE_VIEWS = [(2, [0.9, 0.35, -3.0, -0.3, 0.95, 2.0], (37, 29), None),
                (2, [1.0, 0.0, 500.0, 0.0, 1.0, 500.0], (20, 10), [AC, EQ]),
                (4, [0.8, 0.6, 250.0, -0.6, 0.8, 200.0], (300, 200), FOUR),
                (1, [1.0, 0.0, 16.0, 0.0, 1.0, 3.0], (1, 1), [EQ]),
                (3, [0.0, -1.0, 300.0, 1.0, 0.0, 100.0], (65, 17), [AC]),
                (6, [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], (70, 50), [AC, EQ]),
                (6, [1.1, 0.2, -8.0, -0.2, 1.1, 4.0], (70, 50), [EQ, INV, AC, (POSTERISE, 4.0)]),
                (5, [2.0, 0.0, -20.0, 0.0, 2.5, -30.0], (1, 300), [(SOLARISE, 128.0), AC]),
                (0, [0.1, 0.0, 0.0, 0.0, 0.1, 0.0], (16, 16), None),
                (4, [1.0, 0.0, 440.0, 0.0, 1.0, 100.0], (63, 40), [(POSTERISE, 1.0)])]
FILL = [10.0, 200.5, 30.0, 40.0]


def _crafted(alpha):
    rng = np.random.default_rng(77)
    r = rng.integers(50, 151, (50, 70, 4 if alpha else 3)).astype(np.uint8)
    blue = r[..., 2].reshape(-1)
    first = CHUNK - 2 * 3500                                        # the blue pixels of the first chunk
    assert 0 < first < 3500
    blue[first + 10:] = 200
    blue[-3], blue[-2] = 0, 255
    return r


@pytest.fixture(scope="module")
def batches(po):
    """per (mode, alpha): the dims, the rasters and the oracle's tile blobs - computed once, never changed"""
    from xpng_amd.synth import synth_raster
    kinds = ["photo", "noise", "gray", "noise"]
    out = {}
    for mode, alpha in FORMATS:
        dims = RGBA_DIMS if alpha else RGB_DIMS
        rasters = [synth_raster(kinds[(i + 1) % 4], w, h, alpha, seed=i + 31) for i, (w, h) in enumerate(dims[:-1])] + [_crafted(alpha)]
        out[(mode, alpha)] = (dims, rasters, [po.encode_tiles(mode, r) for r in rasters])
    return out


_REFS = {}


def _reference(key, make):
    """a checker object per (call, alpha, filter, view, matrix): computed once, shared by the cases, its steps never changed"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _colours(n, on):
    return [[PERM, RANGE, DENSE, None][v % 4] for v in range(n)] if on else None


def _fetch(ar, dtype):
    return [g.view(BITS[dtype]).copy() for g in ar.fetch()]


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_views_tone_bits(gpu, batches, mode, alpha, dtype, filt):
    """Every element of every view equals the checker and every sentinel is intact, for all 12 layout words, in one call that mixes
    plain, blur-only, tone-only and blur-and-tone views with one to four steps."""
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    views = TONE_VIEWS
    n = len(views)
    colours = _colours(n, (filt + alpha) % 2 == 1)
    refs = []
    for v, (i, rect, flip, (OW, OH), rec, steps) in enumerate(views):
        col = (colours[v] or list(api.COLOUR_IDENTITY)) if colours else None
        refs.append(_reference(("tone", alpha, filt, v), lambda: Toned(rasters[i], rect, bool(flip), OH, OW, filt, col, rec, steps)))
    assert not np.array_equal(refs[7].under[..., 2], refs[7].v[..., 2])
    sizes = [(v[3][1], v[3][0]) for v in views]
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for word in WORDS:
            ch = api.layout_channels(word, px)
            ar = Arena([ES[dtype] * ch * oh * ow for (oh, ow) in sizes], ES[dtype])
            ctx.decode_batch_views_tone(mode, [t.data_ptr() for t in d_b], lens, [v[0] for v in views], ar.ptrs, word, dtype, sizes, scale[:ch], bias[:ch],
                                        rects=[v[1] or (0, 0) + dims[v[0]] for v in views], flips=[v[2] for v in views], filter=filt, colours=colours,
                                        blurs=[v[4] for v in views], tones=[v[5] for v in views])
            assert ctx.decode_status() == 0
            got = _fetch(ar, dtype)
            for v in range(n):
                w = refs[v].bits(word, dtype, scale, bias).reshape(-1)
                assert np.array_equal(got[v], w), (hex(word), dtype, filt, v, views[v], np.argwhere(got[v] != w)[:4].ravel())
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [0, 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_views_affine_tone_bits(gpu, batches, mode, alpha, dtype, filt):
    """The same for the affine call: a view wholly outside its image is all fill, and the fill takes part in the statistics."""
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    views = AFFINE_VIEWS
    n = len(views)
    colours = _colours(n, (filt + alpha) % 2 == 0)
    refs = []
    for v, (i, m, (OW, OH), steps) in enumerate(views):
        col = (colours[v] or list(api.COLOUR_IDENTITY)) if colours else None
        refs.append(_reference(("affine", alpha, filt, v), lambda: AffineToned(rasters[i], m, OH, OW, filt, FILL, col, steps)))
    assert refs[1].foot == (0, 0, 0, 0)
    sizes = [(v[2][1], v[2][0]) for v in views]
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for word in WORDS:
            ch = api.layout_channels(word, px)
            ar = Arena([ES[dtype] * ch * oh * ow for (oh, ow) in sizes], ES[dtype])
            ctx.decode_batch_views_affine_tone(mode, [t.data_ptr() for t in d_b], lens, [v[0] for v in views], ar.ptrs, word, dtype, sizes, [v[1] for v in views],
                                               scale[:ch], bias[:ch], filter=filt, fill=FILL, colours=colours, tones=[v[3] for v in views])
            assert ctx.decode_status() == 0
            got = _fetch(ar, dtype)
            for v in range(n):
                w = refs[v].bits(word, dtype, scale, bias).reshape(-1)
                assert np.array_equal(got[v], w), (hex(word), dtype, filt, v, views[v], np.argwhere(got[v] != w)[:4].ravel())
    finally:
        ctx.close()


SLOT_BYTES, TONE_REC_BYTES, BLUR_REC_BYTES = 3 * 258 * 4, 48, 160


def _slice(ch, oh, ow):
    return -(-(ch * oh * ow * 4) // 256) * 256


@pytest.mark.gpu
def test_tones_off_are_the_underlying_calls_and_the_workspace(gpu, po):
    """tones=None and records that are all NONE give the underlying calls' bytes and allocate nothing; the first tone call grows the
    workspace by exactly the bytes INTEGRATION.md B14 states; a second call with fewer tone views gets its own statistics."""
    from xpng_amd.synth import synth_raster
    dims = [(17, 4), (64, 64), (130, 90), (100, 110), (5, 7)]
    rasters = [synth_raster(["photo", "noise", "gray"][i % 3], w, h, False, seed=i + 40) for i, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(1, r) for r in rasters]
    r1 = [(0, 0, 17, 4), (3, 4, 50, 55), (10, 10, 110, 70), (0, 0, 100, 110), (1, 2, 3, 4)]
    flips = [1, 0, 1, 0, 1]
    mats = [[1.0, 0.1, -1.0, -0.1, 1.0, 0.5]] * 5
    dtype, word = F16, api.layout(planar=True, bgr=True, channels=4)
    scale, bias = mixed_consts(dtype)
    n = len(dims)
    s1 = [(13, 21)] * n
    recs = [None, (2.0, 5, None), (0.0, 0, 128.0), None, (1.0, 3, 64.0)]
    for affine in (False, True):
        ctx = gpu.MixedContext(dims, 3)
        try:
            d_b, lens = _upload(blobs), [len(b) for b in blobs]
            ins = [t.data_ptr() for t in d_b]
            ident = list(range(n))
            ar = Arena([2 * 4 * oh * ow for (oh, ow) in s1], 2)

            def call(tones, under=False, blurs=recs, filt=2):
                ar.refill()
                if affine:
                    f = 3 if filt == 2 else 0
                    if under:
                        ctx.decode_batch_views_affine(1, ins, lens, ident, ar.ptrs, word, dtype, s1, mats, scale, bias, filter=f, fill=FILL, colours=[DENSE] * n)
                    else:
                        ctx.decode_batch_views_affine_tone(1, ins, lens, ident, ar.ptrs, word, dtype, s1, mats, scale, bias, filter=f, fill=FILL, colours=[DENSE] * n, tones=tones)
                elif under:
                    ctx.decode_batch_views_blur(1, ins, lens, ident, ar.ptrs, word, dtype, s1, scale, bias, rects=r1, flips=flips, filter=filt, blurs=blurs)
                else:
                    ctx.decode_batch_views_tone(1, ins, lens, ident, ar.ptrs, word, dtype, s1, scale, bias, rects=r1, flips=flips, filter=filt, blurs=blurs, tones=tones)
                assert ctx.decode_status() == 0
                return [g.copy() for g in ar.fetch()]

            def rule(i, tone, filt=2):
                if affine:
                    raw = api.resample_affine_tone_host(rasters[i], s1[i], mats[i], word, dtype, scale, bias, filter=3 if filt == 2 else 0, fill=FILL, colour=DENSE, tone=tone)
                else:
                    raw = api.resample_tone_host(rasters[i], s1[i], word, dtype, scale, bias, rect=r1[i], flip=bool(flips[i]), filter=filt, blur=recs[i], tone=tone)
                return np.frombuffer(raw, np.uint8)

            for filt in (0, 2):
                want = call(None, under=True, filt=filt)
                ws = ctx.workspace_bytes()
                for tones in (None, [None] * n, [[(NONE, 0.0)] * 4] * n):
                    got = call(tones, filt=filt)
                    assert all(np.array_equal(a, b) for a, b in zip(got, want)), (affine, filt, tones)
                    assert ctx.workspace_bytes() == ws
            # the first tone call: tone views 0 (plain before), 1 (blurs too: a second slice and a mid record) and 4; view 2 is blur-only
            t_a = [[AC], [EQ, INV, AC], None, None, [(POSTERISE, 2.0), (SOLARISE, 77.0)]]
            got_a = call(t_a)
            sl = _slice(4, 13, 21)
            if affine:
                grow = 3 * sl + 3 * BLUR_REC_BYTES + 3 * TONE_REC_BYTES + 3 * SLOT_BYTES
            else:
                # the blur call above already holds 3 slices and 3 records: views 0, 1, 2, 4 are second-pass views now, views 1 and 4 blur and tone
                before = 3 * sl + 3 * BLUR_REC_BYTES
                grow = (4 + 2) * sl + (4 + 2) * BLUR_REC_BYTES + 3 * TONE_REC_BYTES + 3 * SLOT_BYTES - before
            assert ctx.workspace_bytes() - ws == grow, (affine, ctx.workspace_bytes() - ws, grow)
            for i in range(n):
                assert np.array_equal(got_a[i], rule(i, t_a[i])), (affine, i)
            # fewer tone views, other steps in the same slots: the statistics of the first call must be gone
            t_b = [None, [AC], None, None, [EQ]]
            got_b = call(t_b)
            assert ctx.workspace_bytes() - ws == grow
            for i in range(n):
                assert np.array_equal(got_b[i], rule(i, t_b[i])), (affine, i)
            got_a2 = call(t_a)
            assert all(np.array_equal(a, b) for a, b in zip(got_a, got_a2)) and ctx.workspace_bytes() - ws == grow
        finally:
            ctx.close()


@pytest.mark.gpu
def test_tone_device_refusals_leave_the_sentinels(gpu, batches):
    dims, rasters, blobs = batches[(1, True)]
    word = api.layout(planar=True, channels=3)
    scale, bias = mixed_consts(F16)
    views = TONE_VIEWS
    n = len(views)
    sizes = [(v[3][1], v[3][0]) for v in views]
    ctx = gpu.MixedContext(dims, 4)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        outs = Arena([4 * 4 * oh * ow for (oh, ow) in sizes], 4)
        ws = ctx.workspace_bytes()
        tones = [v[5] for v in views]
        a = dict(mode=1, d_blobs=ins, lens=lens, view_image=[v[0] for v in views], d_outs=outs.ptrs, layout=word, dtype=F16, sizes=sizes, scale=scale[:3],
                 bias=bias[:3])
        blur_kw = dict(rects=[v[1] or (0, 0) + dims[v[0]] for v in views], flips=[v[2] for v in views], filter=2, blurs=[v[4] for v in views])
        aff_kw = dict(matrices=[[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * n, filter=0, fill=FILL)

        def refused(words, affine=(False, True), **kw):
            for af in affine:
                b = dict(a, **(aff_kw if af else blur_kw))
                b.update(tones=tones)
                b.update(kw)
                with pytest.raises(gpu.XpngError) as e:
                    (ctx.decode_batch_views_affine_tone if af else ctx.decode_batch_views_tone)(**b)
                assert all(w in str(e.value) for w in words), (words, str(e.value))
                assert outs.untouched(), words

        for k, (steps, words) in enumerate(BAD_TONES):
            v = k % n
            refused(["bad tone", "view %d" % v] + words, tones=tones[:v] + [steps] + tones[v + 1:])
        refused(["tones has 2 entries"], tones=tones[:2])
        # everything the underlying calls refuse
        refused(["filter 3"], affine=(False,), filter=3)
        refused(["filter 1"], affine=(True,), filter=1)
        refused(["view 2", "radius 29"], affine=(False,), blurs=[None, None, (1.0, 29, None)] + [None] * (n - 3))
        refused(["bad fill", "entry 1"], affine=(True,), fill=[0, 300, 0, 0])
        refused(["view 3", "affine matrix"], affine=(True,), matrices=[[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * 3 + [[float("nan"), 0, 0, 0, 1, 0]] + [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * (n - 4))
        refused(["view_image[2]", "is 9"], view_image=a["view_image"][:2] + [9] + a["view_image"][3:])
        refused(["16385 x 29", "view 5"], sizes=sizes[:5] + [(29, 16385)] + sizes[6:])
        refused(["out_sizes is NULL"], sizes=None)
        refused(["null", "view 1"], d_outs=[outs.ptrs[0], 0] + outs.ptrs[2:])
        refused(["dtype 4"], dtype=4)
        refused(["layout", "0x500"], layout=0x500)
        refused(["scale[1]", "nan"], scale=[1.0, float("nan"), 1.0])
        refused(["mode 2", "RGB"], mode=2)
        refused(["null blob", "image 1"], d_blobs=[ins[0], 0] + ins[2:])
        assert outs.untouched() and ctx.workspace_bytes() == ws     # nothing was allocated for a refused call
        # the context still works after all that
        ctx.decode_batch_views_tone(**dict(a, **blur_kw), tones=tones)
        assert ctx.decode_status() == 0
        got = outs.fetch()
        for v in (2, 6, 10):
            i, rect, flip, (OW, OH), rec, steps = views[v]
            raw = api.resample_tone_host(rasters[i], (OH, OW), word, F16, scale[:3], bias[:3], rect=rect, flip=bool(flip), filter=2, blur=rec, tone=steps)
            assert np.array_equal(got[v][:len(raw)], np.frombuffer(raw, np.uint8)), v
    finally:
        ctx.close()


@pytest.mark.gpu
def test_load_views_tone_on_goldens(gpu, po, tmp_path):
    """Two views per reference-written file, mixed with a level-7 file, with random_tone lists beside blur=, solarise= and colour=:
    with out=, with stack=True, and with affine=; every view equals the host rule of api.load of its file."""
    import torch
    from xpng_amd import tensors
    from xpng_amd.synth import synth_raster
    paths = sorted(p for p in glob.glob(os.path.join(GOLD, "imgfull_*.xpng")) if 11 < os.path.getsize(p) < 200000)[:5]
    assert len(paths) == 5
    l7 = tmp_path / "l7.xpng"
    l7.write_bytes(po.encode_image(7, synth_raster("photo", 60, 45, False, seed=2)))
    paths.append(str(l7))
    want = [gpu.load(p) for p in paths]
    dims = [(r.shape[1], r.shape[0]) for r in want]
    g = torch.Generator().manual_seed(31)
    used = [0, 1, 2, 3, 5]                                          # file 4 has no view; file 5 is answered by the host rule
    big_r = tensors.random_resized_crops([dims[i] for i in used], generator=g)
    small_r = tensors.random_resized_crops([dims[i] for i in used], scale=(0.05, 0.14), generator=g)
    views = [(i, r, k % 2 == 1) for k, (i, r) in enumerate(zip(used, big_r))] + [(i, r, k % 2 == 0) for k, (i, r) in enumerate(zip(used, small_r))]
    V = len(views)
    cols = tensors.random_colour_jitter(V, p=0.9, gray_p=0.3, generator=g)
    blur = tensors.random_gaussian_blur(V, kernel_size=23, p=0.5, generator=g)
    sol = tensors.random_solarise(V, p=0.3, generator=g)
    tone = tensors.random_tone(V, num_ops=2, p=0.8, generator=g)
    tone[0], tone[1], blur[0], blur[1] = ["equalise", ("solarise", 100.5)], None, (1.7, 23), None
    steps = [tensors._tone_steps("t", t) for t in tone]
    scale, bias = consts_from(IMAGENET_MEAN, IMAGENET_STD)
    for lay, bgr, dtype, interp, how in (("chw", False, F16, "bicubic", "stack"), ("hwc", True, F32, "bilinear", "out")):
        kw = dict(layout=lay, channels=3, bgr=bgr, dtype=_torch_dtype(dtype), mean=IMAGENET_MEAN, std=IMAGENET_STD, interpolation=interp)
        shape = (3, 32, 48) if lay == "chw" else (32, 48, 3)
        if how == "stack":
            whole = tensors.load_views(paths, views, (32, 48), stack=True, colour=cols, blur=blur, solarise=sol, tone=tone, **kw)
            assert whole.is_cuda and tuple(whole.shape) == (V,) + shape
        else:
            whole = torch.zeros((V,) + shape, dtype=_torch_dtype(dtype), device="cuda")
            res = tensors.load_views(paths, views, (32, 48), out=list(whole.unbind(0)), colour=cols, blur=blur, solarise=sol, tone=tone, **kw)
            assert all(a.data_ptr() == b.data_ptr() for a, b in zip(res, whole.unbind(0)))
        word = api.layout(planar=lay == "chw", bgr=bgr, channels=3)
        for v, (i, rect, flip) in enumerate(views):
            rec = None if blur[v] is None and sol[v] is None else ((blur[v][0], blur[v][1] // 2) if blur[v] else (0.0, 0)) + (sol[v],)
            raw = api.resample_tone_host(want[i], (32, 48), word, dtype, scale, bias, rect=rect, flip=flip, filter=2 if interp == "bicubic" else 1,
                                         colour=cols[v], blur=rec, tone=steps[v])
            assert np.array_equal(_bits(whole[v], dtype).reshape(-1), np.frombuffer(raw, BITS[dtype])), (lay, v, paths[i], rect)
        plain = tensors.load_views(paths, views, (32, 48), stack=True, colour=cols, blur=blur, solarise=sol, **kw)
        # (a view whose steps change nothing is possible - a flat, dark crop under equalise and solarise -, so: some view with steps)
        assert torch.equal(plain[1], whole[1]) and any(not torch.equal(plain[v], whole[v]) for v in range(V) if steps[v])
    # AutoAugment's (Posterise, Rotate) and (Equalise, Solarise) through affine= + tone=
    aviews = [(i, None, False) for i in used]
    mats = [tensors.affine_matrix((0, 0) + dims[i], (32, 48), angle=[30.0, 0.0, -45.0, 90.0, 12.0][k]) for k, i in enumerate(used)]
    atone = [[("posterise", 4)], ["equalise", ("solarise", 128)], None, ["autocontrast"], ["invert", "equalise"]]
    asteps = [tensors._tone_steps("t", t) for t in atone]
    got = tensors.load_views(paths, aviews, (32, 48), affine=mats, fill=128, tone=atone, antialias=False, dtype=torch.float32, mean=IMAGENET_MEAN,
                             std=IMAGENET_STD, channels=3)
    word = api.layout(planar=True, channels=3)
    for v, (i, _, _) in enumerate(aviews):
        raw = api.resample_affine_tone_host(want[i], (32, 48), mats[v], word, F32, scale, bias, filter=0, fill=128, tone=asteps[v])
        assert np.array_equal(_bits(got[v], F32).reshape(-1), np.frombuffer(raw, BITS[F32])), (v, paths[i])
