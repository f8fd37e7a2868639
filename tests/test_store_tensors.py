"""Float and uint8 device tensors -> .xpng files through one staged batch: xpnghip_images_begin_device, xpnghip_quantize_host,
xpng_store_tensors, api.StagedImages.from_device and tensors.store_files (include/xpng_hip.h "staged batch from device tensors",
include/xpng_store_tensors.h).

The checker is tests/_quant.py: the quantisation rule in numpy with libm's fmaf, and the oracle's normalize_RGBA and encode_image
behind it.  CPU: the symbols, xpnghip_quantize_host on the bytes over every tie, the special values and all 65536 f16 and bf16
patterns, the refusals, the round trip of api.float_table, and store_files at level 7 on CPU tensors.  GPU: the staged rasters, the
files at every level, the round trip through load_files, and the order behind a side stream."""
import os
import re

import numpy as np
import pytest

from _kit import built_with_probes as built, declared, exported, gpu, po
import _quant as Q
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CONST_SETS = {"imagenet": IMAGENET, "unit": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), "half": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))}
# four different pairs, one per channel position of the caller's buffer; position 3 (alpha) passes 0 and 255 through
MIXED = ([0.5, 2.0, 1.0, 1.0], [0.5, -3.0, 0.25, 0.0])
WORDS = [0, Q.PLANAR, Q.BGR, Q.PLANAR | Q.BGR]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_listed_and_exported():
    new = ["xpnghip_images_begin_device", "xpnghip_quantize_host"]
    assert set(new) <= set(declared("xpng_hip.h", "xpnghip_")) and set(new) <= set(api.HIP_SYMBOLS)
    for so in (api.HIP_SO, api.PROBES_SO):
        assert set(new) <= exported(so), so
    assert declared("xpng_store_tensors.h", "xpng_") == api.HOST_STORE_TENSORS_SYMBOLS == ["xpng_store_tensors"]
    assert "xpng_store_tensors" in exported(api.HOST_SO) and "xpng_store_tensors" not in api.HOST_SYMBOLS
    assert "xpng_store_tensors" not in declared("xpng.h", "xpng_")
    assert api.hip_lib().xpnghip_abi_version() == 2
    import xpng_amd
    from xpng_amd import tensors
    for name in ("quantize_host", "store_tensors"):
        assert name in xpng_amd.__all__ and hasattr(xpng_amd, name)
    assert hasattr(api.StagedImages, "from_device") and hasattr(tensors, "store_files")


def _f32_bits(vals):
    return np.array(vals, dtype=np.float32).view(np.uint32)


def _value_bits(dtype):
    """the bit patterns every (layout, order, C) of a dtype is checked on"""
    if dtype == Q.U8:
        return np.arange(256, dtype=np.uint8)
    if dtype in (Q.F16, Q.BF16):
        return np.arange(65536, dtype=np.uint16)                     # every pattern: all ties, specials and subnormals the type has
    ties = np.arange(255, dtype=np.float32) + np.float32(0.5)
    edge = []
    for v in (0.0, 0.5, 1.5, 254.5, 255.0):                          # within 1 ulp of 0, of 255 and of three ties
        v = np.float32(v)
        edge += [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, -1e30, 1e30, 1e-45, -1e-45, 1e-39, 3.4e38, -3.4e38, 256.0, 1000.0, -1.0]
    ints = np.arange(-2, 258, dtype=np.float32)
    rng = np.random.RandomState(7)
    rand = (rng.rand(3000) * 300 - 20).astype(np.float32)
    bits = np.concatenate([_f32_bits(ties), _f32_bits(edge), _f32_bits(special), _f32_bits(ints), _f32_bits(rand),
                           np.array([0x7FC00001, 0xFFC00000, 0x7F800001, 0x00000001, 0x80000001, 0x007FFFFF], np.uint32)])   # NaNs, subnormals
    return bits


def _buffer(bits, C, word):
    """a tight buffer of C * npx elements in the layout: position cc of pixel p holds bits[(p + 7919 cc) % n]"""
    n = bits.size
    npx = n + 3                                                      # (npx & 3 differs from 0 for every set)
    cols = [bits[(np.arange(npx) + 7919 * cc) % n] for cc in range(C)]
    chan = np.stack(cols, axis=0)                                    # [position in the caller's buffer][pixel]
    return np.ascontiguousarray(chan if word & Q.PLANAR else chan.T), npx


@pytest.mark.parametrize("dtype", Q.DTYPES)
def test_quantize_host_equals_the_checker_on_the_bytes(dtype):
    """xpnghip_quantize_host against tests/_quant.py for both layouts x RGB/BGR x C 3/4: constants 1 and 0 (every representable
    value as itself), four different pairs (which position a constant belongs to), integers + 0.5 (every tie k + 0.5, k = 0 .. 254,
    in every dtype) and, for f16, scale 2^24 on the subnormals."""
    bits = _value_bits(dtype)
    runs = [(None, None)]
    if dtype != Q.U8:
        runs.append(MIXED)
        runs.append(([1.0] * 4, [0.5, 0.5, 0.5, 0.5]))
    if dtype == Q.F16:
        runs.append(([float(2 ** 24)] * 4, [0.0, 0.5, 0.0, 0.5]))
    luts = {}

    def lut(sc, bi):
        """the rule over the value set for one pair of constants, computed once"""
        if (sc, bi) not in luts:
            luts[(sc, bi)] = Q.quantize(Q.widen(bits, dtype), sc, bi)
        return luts[(sc, bi)]

    n = bits.size
    for scale, bias in runs:
        for word in WORDS:
            for C in (3, 4):
                buf, npx = _buffer(bits, C, word)
                got = api.quantize_host(buf, npx, C, word, dtype, scale, bias)
                want = np.empty((npx, C), np.uint8)
                for c in range(C):
                    cc = Q.caller_pos(c, word & Q.BGR)
                    idx = (np.arange(npx) + 7919 * cc) % n
                    want[:, c] = bits[idx] if dtype == Q.U8 else lut(scale[cc] if scale else 1.0, bias[cc] if bias else 0.0)[idx]
                bad = np.argwhere(got != want)
                assert bad.size == 0, (dtype, word, C, scale, bias, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
                if C == 3 and scale is None:                         # the checker's own walk of a layout gives the same
                    m = min(npx, 2048)
                    assert np.array_equal(Q.stage(buf[..., :m] if word & Q.PLANAR else buf[:m], m, C, word, dtype), want[:m])
    # the ties themselves, spelled out: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254, and the special values
    if dtype != Q.U8:
        k = np.arange(255, dtype=np.float32)
        x = {Q.F32: k.view(np.uint32), Q.F16: k.astype(np.float16).view(np.uint16), Q.BF16: (k.view(np.uint32) >> 16).astype(np.uint16)}[dtype]
        assert np.array_equal(Q.widen(x, dtype), k)                  # (0 .. 254 are exact in every dtype)
        x3 = np.ascontiguousarray(np.stack([x, x, x], axis=1))
        got = api.quantize_host(x3, 255, 3, 0, dtype, [1.0] * 4, [0.5] * 4)[:, 0]
        want = np.array([2 * ((i + 1) // 2) for i in range(255)], dtype=np.uint8)          # i + 0.5 rounds to the even neighbour
        assert np.array_equal(got, want) and want[0] == 0 and want[1] == 2 and want[2] == 2 and want[254] == 254
        sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1e30, 1e30, 255.0, 256.0, 0.25, -0.25, 3.0], dtype=np.float32)
        with np.errstate(over="ignore"):
            spb = {Q.F32: sp.view(np.uint32), Q.F16: sp.astype(np.float16).view(np.uint16), Q.BF16: (sp.view(np.uint32) >> 16).astype(np.uint16)}[dtype]
        got = api.quantize_host(np.ascontiguousarray(spb.reshape(4, 3)), 4, 3, 0, dtype).reshape(-1)
        assert got.tolist() == [0, 0, 255, 0, 0, 0, 255, 255, 255, 0, 0, 3], got.tolist()
    if dtype == Q.F16:                                               # the subnormals m * 2^-24 under 2^24 are the integers m
        m = np.arange(1, 1024, dtype=np.uint16)
        m3 = np.ascontiguousarray(np.stack([m, m, m], axis=1))
        got = api.quantize_host(m3, 1023, 3, 0, Q.F16, [float(2 ** 24)] * 4, None)[:, 0]
        assert np.array_equal(got, np.minimum(np.arange(1, 1024), 255).astype(np.uint8))


def test_quantize_host_and_begin_device_refuse_bad_arguments():
    x = np.zeros(12, np.float32)
    ok = api.quantize_host(x, 4, 3, 0, Q.F32)
    assert ok.shape == (4, 3) and not ok.any()
    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(layout=0, dtype=Q.U8, scale=[1.0] * 4), "dtype 0"),                    # constants with uint8
        (dict(layout=0, dtype=Q.U8, bias=[0.0] * 4), "dtype 0"),
        (dict(layout=0, dtype=Q.F32, scale=[1.0, inf, 1.0, 1.0]), "scale[1]"),      # a non-finite constant
        (dict(layout=0, dtype=Q.F32, bias=[0.0, 0.0, nan, 0.0]), "bias[2]"),
        (dict(layout=0x300, dtype=Q.F32), "0x300"),                                 # a channel field in the layout word
        (dict(layout=0x401, dtype=Q.F32), "0x401"),
        (dict(layout=0x004, dtype=Q.F32), "0x4"),                                   # an unknown bit
        (dict(layout=0, dtype=4), "dtype 4"),
        (dict(layout=0, dtype=99), "dtype 99"),
    ]
    for kw, word in cases:
        src = np.zeros(12, np.uint8) if kw["dtype"] == Q.U8 else x
        with pytest.raises(api.XpngError, match=re.escape(word)):
            api.quantize_host(src, 4, 3, kw["layout"], kw["dtype"], kw.get("scale"), kw.get("bias"))
        with pytest.raises(api.XpngError, match=re.escape(word)):
            api.StagedImages.from_device([0x10000], [(2, 2)], [3], kw["layout"], kw["dtype"], kw.get("scale"), kw.get("bias"))
    with pytest.raises(api.XpngError, match="C is 2"):
        api.quantize_host(np.zeros(8, np.float32), 4, 2, 0, Q.F32)
    with pytest.raises(api.XpngError, match="null"):
        api.quantize_host(0, 4, 3, 0, Q.F32)                         # a NULL source
    L = api.hip_lib()
    assert L.xpnghip_quantize_host(0, Q.F32, 3, x.ctypes.data, 4, None, None, None) != 0 and "null" in api._err()
    # the device call: everything below is refused before a device is looked for
    for ptrs, dims, ch, dt, word in [
        ([0], [(2, 2)], [3], Q.F16, "null buffer of image 0"),
        ([0x10000, 0x10001], [(2, 2), (2, 2)], [3, 3], Q.F16, "image 1 is not aligned to its 2-byte"),
        ([0x10002], [(2, 2)], [3], Q.F32, "not aligned to its 4-byte"),
        ([0x10000], [(0, 2)], [3], Q.F32, "0 x 2"),
        ([0x10000], [(2, (1 << 24) + 1)], [3], Q.F32, "2 x 16777217"),
        ([0x10000], [(2, 2)], [5], Q.F32, "5 channels"),
        ([0x10000], [(2, 2)], [2], Q.U8, "2 channels"),
    ]:
        with pytest.raises(api.XpngError, match=re.escape(word)):
            api.StagedImages.from_device(ptrs, dims, ch, 0, dt)
    for n in (0, 4097):
        with pytest.raises(api.XpngError, match="1 .. 4096"):
            api.StagedImages.from_device([0x10000] * n, [(2, 2)] * n, [3] * n, 0, Q.U8)
    with pytest.raises(api.XpngError, match="no usable HIP device"):
        api.StagedImages.from_device([0x10000], [(2, 2)], [3], 0, Q.U8, device=api.device_count())
    h = api.C.c_void_p(0x1234)                                        # *h is NULL after a refused call
    assert L.xpnghip_images_begin_device(api.C.byref(h), 0, 0, None, None, None, 0, 0, None, None, None, None) != 0 and not h


@pytest.mark.parametrize("dtype", [Q.F16, Q.BF16, Q.F32])
@pytest.mark.parametrize("name", sorted(CONST_SETS))
def test_float_table_round_trips_through_the_inverse_constants(name, dtype):
    """The 256 outputs of api.float_table for each channel, quantised with store_files' inverse constants, give back 0 .. 255:
    what load_files returns, store_files stores as the file's bytes.  All nine (set, dtype) pairs hold with the real fmaf."""
    mean, std = CONST_SETS[name]
    fwd_s = [float(np.float32(1.0 / (255.0 * s))) for s in std]
    fwd_b = [float(np.float32(-m / s)) for m, s in zip(mean, std)]
    table = np.frombuffer(api.float_table(dtype, fwd_s, fwd_b), dtype=Q.BITS[dtype]).reshape(3, 256)
    scale, bias = Q.inverse_consts(mean, std)
    got = api.quantize_host(np.ascontiguousarray(table), 256, 3, Q.PLANAR, dtype, scale, bias)
    want = Q.stage(table, 256, 3, Q.PLANAR, dtype, scale, bias)
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)), (name, dtype)


def _torch_of(bits, dtype):
    """a numpy array of bit patterns as a torch tensor of the dtype (same shape)"""
    import torch
    if dtype == Q.U8:
        return torch.from_numpy(bits.copy())
    if dtype == Q.F32:
        return torch.from_numpy(bits.view(np.float32).copy())
    t = torch.from_numpy(bits.view(np.int16).copy())
    return t.view(torch.float16 if dtype == Q.F16 else torch.bfloat16)


def _elements(r, dtype, scale, bias, seed):
    """element bit patterns, file order (h, w, C), that quantise near the uint8 raster r: x = (v + jitter - bias) / scale in float64,
    rounded to the dtype (seed None: no jitter).  What they quantise TO is the checker's business; the alpha channel (scale 1,
    bias 0) comes out exact."""
    if dtype == Q.U8:
        return r.copy()
    rng = np.random.RandomState(seed)
    C = r.shape[2]
    x = np.empty(r.shape, np.float64)
    for c in range(C):
        jit = (rng.randint(-2, 3, r.shape[:2]) * 0.25) if c < 3 and seed is not None else 0.0   # quarter steps: exact ties happen
        x[..., c] = (r[..., c] + jit - bias[c]) / scale[c]
    x32 = x.astype(np.float32)
    if dtype == Q.F32:
        return x32.view(np.uint32)
    if dtype == Q.F16:
        return x32.astype(np.float16).view(np.uint16)
    import torch
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_store_files_level_7_on_cpu_tensors(po, tmp_path):
    """CPU tensors at level 7 need no device: the files equal api.store(7, checker's raster); an opaque RGBA tensor becomes an
    RGB file and hidden colours are zeroed; every misuse raises XpngError and writes nothing."""
    import torch
    from xpng_amd import tensors as T
    from xpng_amd.synth import special_cases, synth_raster
    sp = dict(special_cases())
    base = [synth_raster("photo", 37, 21, False), synth_raster("photo", 5, 3, True), sp["opaque_alpha"], sp["hidden_colour"], synth_raster("photo", 1, 1, True)]
    for dtype, tdt in [(Q.U8, torch.uint8), (Q.F16, torch.float16), (Q.BF16, torch.bfloat16), (Q.F32, torch.float32)]:
        for layout, bgr in [("chw", False), ("hwc", True)]:
            word = (Q.PLANAR if layout == "chw" else 0) | (Q.BGR if bgr else 0)
            paths, want = [], []
            for i, r in enumerate(base):                             # (one call per tensor: a per-channel mean fits one channel count)
                h, w, C = r.shape
                mean, std = list(IMAGENET[0]) + [0.0] * (C - 3), list(IMAGENET[1]) + [1.0] * (C - 3)   # C values: alpha passes through
                scale, bias = (None, None) if dtype == Q.U8 else Q.inverse_consts(mean, std)
                # the constants belong to positions of the CALLER's buffer: build the elements in that order
                rc = r[..., [Q.caller_pos(c, bgr) for c in range(C)]]
                el = _elements(rc, dtype, scale, bias, i)            # (h, w, C) in the caller's channel order
                buf = np.ascontiguousarray(el.transpose(2, 0, 1) if layout == "chw" else el)
                t = _torch_of(buf, dtype)
                assert t.dtype == tdt
                q = Q.stage(buf, h * w, C, word, dtype, scale, bias).reshape(h, w, C)
                p, one = str(tmp_path / f"c{dtype}{layout}{i}.xpng"), str(tmp_path / "one.xpng")
                T.store_files([t], [p], level=7, layout=layout, bgr=bgr, **({} if dtype == Q.U8 else dict(mean=mean, std=std)))
                api.store(7, q, one)
                assert open(p, "rb").read() == open(one, "rb").read() == po.encode_image(7, q), (dtype, layout, i)
                paths.append(p); want.append(q)
            assert api.load(paths[2]).shape[2] == 3                  # opaque RGBA -> RGB
            hid = api.load(paths[3])
            assert hid.shape[2] == 4 and not hid[hid[..., 3] == 0].any() and want[3][want[3][..., 3] == 0].any()   # hidden colours zeroed
    # a list of mixed sizes and channel counts in one call, and a stacked tensor
    rs = [base[0], base[1]]
    ts = [torch.from_numpy(np.ascontiguousarray(r.transpose(2, 0, 1))) for r in rs]
    paths = [str(tmp_path / f"m{i}.xpng") for i in range(2)]
    T.store_files(ts, paths, level=7)
    assert [open(p, "rb").read() for p in paths] == [po.encode_image(7, r) for r in rs]
    stack = torch.rand(3, 6, 5, 4)                                   # (N, h, w, C) floats in 0 .. 1
    paths = [str(tmp_path / f"s{i}.xpng") for i in range(3)]
    T.store_files(stack, paths, level=7, layout="hwc")
    for i, p in enumerate(paths):
        bits = stack[i].numpy().view(np.uint32)
        r = Q.stage(bits, 30, 4, 0, Q.F32, [255.0] * 4, [0.0] * 4).reshape(6, 5, 4)
        assert open(p, "rb").read() == po.encode_image(7, r)
    # misuse
    good = torch.zeros(3, 4, 4, dtype=torch.uint8)
    p1 = str(tmp_path / "never.xpng")
    bad = [
        (dict(tensors=[good, good.to(torch.float32)], paths=[p1, p1]), "dtype"),
        (dict(tensors=[torch.zeros(3, 4, 8, dtype=torch.uint8)[:, :, ::2]], paths=[p1]), "not contiguous"),
        (dict(tensors=[torch.zeros(2, 4, 4, dtype=torch.uint8)], paths=[p1]), "2 channels"),
        (dict(tensors=[good], paths=[p1], mean=[0.5, 0.5, 0.5]), "mean and std need a float dtype"),
        (dict(tensors=[good], paths=[p1], level=1), "level 7 only"),
        (dict(tensors=[good, good], paths=[p1]), "2 tensors and 1 paths"),
        (dict(tensors=[good.to(torch.float64)], paths=[p1]), "float64"),
        (dict(tensors=[good.to(torch.float32)], paths=[p1], mean=[0.5, 0.5]), "mean has 2 values"),
        (dict(tensors=[good], paths=[p1], level=3), "level"),
        (dict(tensors=[good], paths=[p1], layout="nchw"), "layout"),
        (dict(tensors=[], paths=[]), "empty"),
    ]
    for kw, word in bad:
        kw.setdefault("level", 7)
        with pytest.raises(api.XpngError, match=re.escape(word)):
            T.store_files(**kw)
    assert not os.path.exists(p1)


# ---- GPU ------------------------------------------------------------------------------------------------------------
_RASTERS = {}


def _rasters():
    """the twelve images of the staged-batch tests, as the uint8 rasters the elements are built around: every npx & 3, the
    smallest RGBA the codec takes (4 x 4), an RGBA narrower than 4 px (-> level 7), one tile, two tiles; RGB, opaque RGBA, RGBA
    with colours hidden under alpha 0, translucent RGBA"""
    if not _RASTERS:
        from xpng_amd.synth import synth_raster

        def rgba(w, h, kind, seed):
            r = synth_raster("photo", w, h, True, seed=seed)
            if kind == "opaque":
                r[..., 3] = 255
            elif kind == "hidden":
                r[..., 3] = 255
                r[::3, 1::2, 3] = 0                                  # alpha 0 over colours that stay what they are
            else:
                r[..., 3] = np.where(r[..., 3] == 0, 7, r[..., 3])   # translucent, nothing hidden
                r[0, 0, 3] = 128
            return r

        items = [("rgb_1x1", synth_raster("photo", 1, 1, False)), ("rgb_2x1", synth_raster("photo", 2, 1, False)),
                 ("rgb_3x3", synth_raster("photo", 3, 3, False)), ("rgb_5x1", synth_raster("photo", 5, 1, False)),
                 ("rgba_4x4_translucent", rgba(4, 4, "translucent", 1)), ("rgba_3x5_hidden", rgba(3, 5, "hidden", 2)),
                 ("rgb_67x33", synth_raster("photo", 67, 33, False)), ("rgba_67x33_opaque", rgba(67, 33, "opaque", 3)),
                 ("rgba_300x200_hidden", rgba(300, 200, "hidden", 4)), ("rgb_300x200", synth_raster("photo", 300, 200, False, seed=5)),
                 ("rgb_889x445", synth_raster("photo", 889, 445, False, seed=6)), ("rgba_889x445_translucent", rgba(889, 445, "translucent", 7))]
        _RASTERS["items"] = [(n, np.ascontiguousarray(r)) for n, r in items]
    return _RASTERS["items"]


_CASES = {}


def _case(po, dtype, word, extra=()):
    """(names, buffers of bit patterns in the layout, dims, channels, scale, bias, checker's rasters, normalised rasters) of the
    twelve images (+ extra) for a dtype and a layout word; the elements are computed once per dtype and order"""
    key = (dtype, word, len(extra))
    if key in _CASES:
        return _CASES[key]
    scale, bias = (None, None) if dtype == Q.U8 else MIXED
    bgr = bool(word & Q.BGR)
    names, bufs, dims, chans, want, norm = [], [], [], [], [], []
    for i, (name, r) in enumerate(list(_rasters()) + list(extra)):
        h, w, C = r.shape
        ekey = ("el", dtype, bgr, name)
        if ekey not in _CASES:
            rc = r[..., [Q.caller_pos(c, bgr) for c in range(C)]]    # the caller's channel order: that is where a constant belongs
            el = _elements(rc, dtype, scale or [1.0] * 4, bias or [0.0] * 4, 100 + i if i < 12 else None)   # (an extra image: no jitter)
            if dtype != Q.U8 and h * w >= 300 * 200 and C == 3:     # special values among the colours of the large RGB images
                sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, -1e30, 6e-8, -6e-8, 254.5, 0.5, 1.5], dtype=np.float32)
                with np.errstate(over="ignore"):
                    spb = {Q.F32: sp.view(np.uint32), Q.F16: sp.astype(np.float16).view(np.uint16), Q.BF16: (sp.view(np.uint32) >> 16).astype(np.uint16)}[dtype]
                flat = el.reshape(-1)
                flat[5:5 + 3 * spb.size:3] = spb
                flat[flat.size - 40:flat.size - 40 + spb.size] = spb
            _CASES[ekey] = el
        el = _CASES[ekey]
        buf = np.ascontiguousarray(el.transpose(2, 0, 1) if word & Q.PLANAR else el)
        q = Q.stage(buf, h * w, C, word, dtype, scale, bias).reshape(h, w, C)
        names.append(name); bufs.append(buf); dims.append((w, h)); chans.append(C); want.append(q)
        norm.append(po.normalize_rgba(q) if C == 4 else q)
    _CASES[key] = (names, bufs, dims, chans, scale, bias, want, norm)
    return _CASES[key]


class _Arena:
    """one device tensor of bytes holding every buffer at a 16-byte boundary plus 0, 1 or 3 ELEMENTS, sentinels around them"""

    def __init__(self, bufs, es):
        import torch
        self.off, total = [], 64
        for i, b in enumerate(bufs):
            self.off.append(total + es * (0, 1, 3)[i % 3])
            total += -(-(b.nbytes + 3 * es + 64) // 16) * 16
        host = np.full(total, 0xA5, np.uint8)
        for o, b in zip(self.off, bufs):
            host[o:o + b.nbytes] = b.reshape(-1).view(np.uint8)
        self.host = host
        self.t = torch.from_numpy(host.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptrs = [self.t.data_ptr() + o for o in self.off]

    def unchanged(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(self.t.cpu().numpy(), self.host)


@pytest.mark.gpu
@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("dtype", Q.DTYPES)
def test_begin_device_stages_what_the_checker_quantises(gpu, po, dtype, word):
    """StagedImages.from_device + fetch over one handle of twelve images at element offsets 0, 1 and 3 of one arena: pxsz_out and
    every normalised raster equal the oracle's normalize_RGBA of the checker's quantised raster; the caller's buffers and the bytes
    around them are not written."""
    names, bufs, dims, chans, scale, bias, want, norm = _case(po, dtype, word)
    assert len(names) == 12 and {(w * h) & 3 for (w, h) in dims} == {0, 1, 2, 3}
    assert [n.shape[2] for n in norm] == [3, 3, 3, 3, 4, 4, 3, 3, 4, 3, 3, 4]      # (opaque RGBA -> RGB; the others keep alpha)
    assert any((q[q[..., 3] == 0][:, :3] != 0).any() for q in want if q.shape[2] == 4)   # some colour IS hidden before normalisation
    arena = _Arena(bufs, Q.ES[dtype])
    st = api.StagedImages.from_device(arena.ptrs, dims, chans, word, dtype, scale, bias)
    try:
        assert st.pxsz == [n.shape[2] for n in norm]
        for i, n in enumerate(norm):
            got = st.fetch(i)
            assert got.shape == n.shape and np.array_equal(got, n), (names[i], np.argwhere(got != n)[:4].tolist())
        single = st.single_colour()
        assert single == [bool((n.reshape(-1, n.shape[2]) == n.reshape(-1, n.shape[2])[0]).all()) for n in norm]
    finally:
        st.end()
    assert arena.unchanged()


def _device_tensors(bufs, dtype, shapes):
    """the buffers as torch tensors on the device: slices of one arena tensor of the dtype at element offsets 0, 1 and 3"""
    import torch
    total, offs = 0, []
    for i, b in enumerate(bufs):
        offs.append(total + (0, 1, 3)[i % 3])
        total += -(-(b.size + 3) // 8) * 8
    host = np.zeros(total, Q.BITS[dtype])
    for o, b in zip(offs, bufs):
        host[o:o + b.size] = b.reshape(-1)
    arena = _torch_of(host, dtype).cuda()
    return [arena[o:o + b.size].view(shape) for o, b, shape in zip(offs, bufs, shapes)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,layout,bgr", [(Q.F16, "chw", False), (Q.U8, "hwc", True), (Q.BF16, "hwc", False), (Q.F32, "chw", True)])
def test_store_files_equals_store_batch_on_the_checkers_rasters(gpu, po, tmp_path, dtype, layout, bgr):
    """tensors.store_files at levels 1, 2 and 7 over the twelve images and a single-colour 40 x 30 (level 2: the 11-byte file):
    every file is byte for byte the one api.store_batch writes for the checker's quantised raster, and what the oracle's
    encode_image gives (but for the RGBA narrower than 4 px below level 7, undefined in the reference)."""
    from xpng_amd import tensors as T
    flat = np.empty((30, 40, 3), np.uint8)
    flat[...] = (17, 130, 250)
    word = (Q.PLANAR if layout == "chw" else 0) | (Q.BGR if bgr else 0)
    names, bufs, dims, chans, scale, bias, want, norm = _case(po, dtype, word, extra=[("flat_40x30", flat)])
    if dtype != Q.U8:                                                # store_files' constants are 255 std and 255 mean: MIXED as mean and std
        std, mean = [s / 255.0 for s in scale], [b / 255.0 for b in bias]
        assert Q.inverse_consts(mean, std) == (scale, bias)
    assert (want[-1] == want[-1][0, 0]).all()                        # (still one colour after the quantisation)
    shapes = [(C, h, w) if layout == "chw" else (h, w, C) for (w, h), C in zip(dims, chans)]
    ts = _device_tensors(bufs, dtype, shapes)
    for level in (1, 2, 7):
        paths = [str(tmp_path / f"t{level}_{i}.xpng") for i in range(len(ts))]
        refs = [str(tmp_path / f"r{level}_{i}.xpng") for i in range(len(ts))]
        # (a per-channel mean serves one channel count: the RGB and the RGBA tensors go in two calls)
        for C in (3, 4):
            sel = [i for i, c in enumerate(chans) if c == C]
            kw = {} if dtype == Q.U8 else dict(mean=mean[:C], std=std[:C])
            T.store_files([ts[i] for i in sel], [paths[i] for i in sel], level=level, layout=layout, bgr=bgr, **kw)
        api.store_batch(level, want, refs)
        for name, q, p, r in zip(names, want, paths, refs):
            got = open(p, "rb").read()
            assert got == open(r, "rb").read(), (level, name, "store_batch")
            if name != "rgba_3x5_hidden" or level == 7:
                assert got == po.encode_image(level, q), (level, name, "oracle")
        if level == 2:
            assert os.path.getsize(paths[-1]) == 11
        if level != 7:
            assert open(paths[5], "rb").read()[3] == 7               # RGBA narrower than 4 px: stored at level 7
        back = api.load_batch(paths)
        for name, n, b in zip(names, norm, back):
            assert b.shape == n.shape and np.array_equal(b, n), (level, name)


def _corpus_three(manifest):
    from conftest import corpus_entries
    ents = [(n, e) for n, e in corpus_entries(manifest) if e["ch"] == 3 and e["w"] * e["h"] <= 700_000]
    assert len(ents) >= 3
    return ents[:3]


@pytest.mark.gpu
def test_store_files_on_corpus_goldens(gpu, po, manifest, tmp_path):
    """Three images of the reference's corpus as f16 planar tensors in 0 .. 1 and as uint8 interleaved BGR tensors: the level-1
    files are the reference-written goldens themselves."""
    import torch
    from conftest import corpus_raster
    from xpng_amd import tensors as T
    ents = _corpus_three(manifest)
    rasters = [corpus_raster(e) for _, e in ents]
    golden = [open(os.path.join(GOLD, e["L1"]["file"]), "rb").read() for _, e in ents]
    paths = [str(tmp_path / f"g{i}.xpng") for i in range(3)]
    f16 = [(torch.from_numpy(r).cuda().permute(2, 0, 1).to(torch.float32) / 255.0).to(torch.float16).contiguous() for r in rasters]
    T.store_files(f16, paths, level=1)                               # v / 255 in f16, times 255: back within 0.07 of v
    assert [open(p, "rb").read() for p in paths] == golden
    bgr = [torch.from_numpy(np.ascontiguousarray(r[..., ::-1])).cuda() for r in rasters]
    T.store_files(bgr, paths, level=1, layout="hwc", bgr=True)
    assert [open(p, "rb").read() for p in paths] == golden


@pytest.mark.gpu
def test_load_files_and_store_files_round_trip(gpu, po, manifest, tmp_path):
    """load_files(f16, ImageNet mean / std) -> store_files(same mean / std) -> files that decode to the goldens' rasters; with
    dtype uint8 the files re-stored at their own level are byte for byte what api.store writes."""
    import torch
    from conftest import corpus_raster
    from xpng_amd import tensors as T
    ents = _corpus_three(manifest)
    rasters = [corpus_raster(e) for _, e in ents]
    mean, std = IMAGENET
    for level in (1, 2):
        src = [os.path.join(GOLD, e["L%d" % level]["file"]) for _, e in ents]
        out = [str(tmp_path / f"rt{level}_{i}.xpng") for i in range(3)]
        ts = T.load_files(src, dtype=torch.float16, mean=mean, std=std)
        T.store_files(ts, out, level=level, mean=mean, std=std)
        for p, r in zip(out, rasters):
            assert np.array_equal(api.load(p), r), (level, p)
        t8 = T.load_files(src, layout="hwc")
        T.store_files(t8, out, level=level, layout="hwc")
        for p, r in zip(out, rasters):
            one = str(tmp_path / "one.xpng")
            api.store(level, r, one)
            assert open(p, "rb").read() == open(one, "rb").read(), (level, p)


@pytest.mark.gpu
def test_store_files_runs_behind_the_current_stream_and_a_refused_call_leaves_nothing(gpu, po, tmp_path):
    """A tensor filled by a kernel queued on a side stream, which the current stream waits for, is read after that kernel; a
    refused call writes no file and hands back no handle."""
    import torch
    from xpng_amd import tensors as T
    from xpng_amd.synth import synth_raster
    r = synth_raster("photo", 640, 480, False, seed=9)
    src = torch.from_numpy(r).cuda().permute(2, 0, 1).contiguous()
    big = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")  # work that keeps the side stream busy in front of the fill
    t = torch.full((3, 480, 640), 77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(8):
            big.add_(1.0)
        t.copy_(src)                                                 # the fill, queued behind them on the side stream
    torch.cuda.current_stream().wait_stream(side)
    p = str(tmp_path / "side.xpng")
    T.store_files([t], [p], level=1, mean=0.0, std=1.0 / 255.0)      # scale 1: the tensor holds 0 .. 255
    assert np.array_equal(api.load(p), r)
    # refused calls
    never = [str(tmp_path / "never0.xpng"), str(tmp_path / "never1.xpng")]
    h16 = torch.zeros(2 * 3 * 4 * 4 + 8, dtype=torch.float16, device="cuda")
    good, odd = h16.data_ptr(), h16.data_ptr() + 96 + 1
    with pytest.raises(api.XpngError, match="not aligned"):
        api.store_tensors(1, [good, odd], [(4, 4), (4, 4)], [3, 3], 0, Q.F16, never)
    with pytest.raises(api.XpngError, match="scale"):
        api.store_tensors(1, [good, good + 96], [(4, 4), (4, 4)], [3, 3], 0, Q.F16, never, scale=[1.0, float("nan"), 1.0, 1.0])
    with pytest.raises(api.XpngError, match="0x300"):
        api.store_tensors(1, [good, good + 96], [(4, 4), (4, 4)], [3, 3], 0x300, Q.F16, never)
    with pytest.raises(api.XpngError):
        api.store_tensors(1, [good, 0], [(4, 4), (4, 4)], [3, 3], 0, Q.F16, never)
    with pytest.raises(api.XpngError, match="not contiguous"):
        T.store_files([torch.zeros(3, 4, 8, device="cuda")[:, :, ::2]], never[:1])
    with pytest.raises(api.XpngError, match="level 7 only"):
        T.store_files([torch.zeros(3, 4, 4)], never[:1], level=1)
    assert not any(os.path.exists(q) for q in never)
    L, h = api.hip_lib(), api.C.c_void_p(0x1234)
    ptrs, flat, ch = api._tensor_args([good, odd], [(4, 4), (4, 4)], [3, 3])
    assert L.xpnghip_images_begin_device(api.C.byref(h), 0, 2, ptrs, flat, ch, 0, Q.F16, None, None, None, (api.C.c_uint8 * 2)()) != 0 and not h
