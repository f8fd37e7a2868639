"""Float layouts: decode a mixed-size batch straight into normalised f16 / bf16 / f32 buffers (include/xpng_hip.h XPNGHIP_DTYPE_*,
xpnghip_decode_varsize_device_batch_as_float, xpnghip_float_table; xpng_amd/tensors.py load_files dtype / mean / std / stack).

The rule: element = (T) fmaf((float)byte, scale[c], bias[c]), T rounded to nearest even, c the channel's position in the caller's
buffer.  The checker is independent of the code under test: a 256-entry table per (dtype, scale, bias, c) made with the C library's
fmaf through ctypes and numpy's astype(float16) / torch's CPU .to(bfloat16), indexed by the oracle's raster after the numpy
rearrangement of tests/_kit.py (arrange; table and expect are there too).  Every comparison is on the bits.
CPU: the symbols, xpnghip_dtype_bytes, xpnghip_float_table against the checker (1/255, ImageNet, exact rounding ties, f16
subnormals, overflow to inf) and its refusals, load_files on the host-answered kinds in every layout and dtype, stack, misuse.
GPU (-m gpu): every layout word x dtype on batches whose widths put every row and plane-row start at every multiple of the
element size modulo 16 bytes, inside sentinel-filled buffers; the uint8 layout call as a second reference; a rejected tile and
misuse; load_files on reference-written goldens."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _kit import (built, Arena, arrange, BF16, BITS, _bits, consts_from, DTYPES, ES, expect, F16, F32, f32_of, FORMATS, gpu,
                  IMAGENET_MEAN, IMAGENET_STD, mixed_consts, _offsets, po, table, _torch_dtype, _upload)
from xpng_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ["xpnghip_dtype_bytes", "xpnghip_float_table", "xpnghip_decode_varsize_device_batch_as_float"]
COMMON_DIMS = [(17, 4), (64, 64), (445, 444), (889, 445), (100, 1100), (701, 300)]
RGB_DIMS = [(w, h) for w in range(1, 18) for h in range(1, 4)] + COMMON_DIMS
RGBA_DIMS = [(4, 4), (5, 7), (6, 5), (7, 4), (9, 5), (13, 4)] + COMMON_DIMS
WORDS = [api.layout(planar=p, bgr=b, channels=c) for c in (0, 3, 4) for p in (False, True) for b in (False, True)]


# ---- the checker ------------------------------------------------------------------------------------------------------
def expect_word(r, word, tab):
    return expect(r, bool(word & 1), bool(word & 2), (word >> 8) or r.shape[2], tab)


def lib_table(dtype, scale, bias):
    raw = api.float_table(dtype, scale, bias)
    return np.frombuffer(raw, BITS[dtype]).reshape(len(scale), 256)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_float_symbols_are_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xpng_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(xpnghip_\w*)\s*\(", txt))
    assert set(NEW) <= names and set(NEW) <= set(api.HIP_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.HIP_SO], text=True)
    assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for macro, value in (("F16", 1), ("BF16", 2), ("F32", 3)):
        assert re.search(r"#define\s+XPNGHIP_DTYPE_%s\s+%du" % (macro, value), txt), macro
        assert getattr(api, "DTYPE_" + macro) == value
    assert not [n for n in NEW if "mixed" in n]
    assert "xpnghip_decode_varsize_device_batch_as_float" not in open(os.path.join(ROOT, "include", "xpng_batch.h")).read()
    import xpng_amd
    for name in ("DTYPE_F16", "DTYPE_BF16", "DTYPE_F32", "dtype_bytes", "float_table"):
        assert name in xpng_amd.__all__ and hasattr(xpng_amd, name)
    assert hasattr(api.MixedContext, "decode_batch_as_float")
    assert api.hip_lib().xpnghip_abi_version() == 2


def test_dtype_bytes():
    lib = api.hip_lib()
    assert [lib.xpnghip_dtype_bytes(d) for d in (1, 2, 3)] == [2, 2, 4] == [api.dtype_bytes(d) for d in (1, 2, 3)]
    for bad in (0, 4, 0x80000000):
        assert lib.xpnghip_dtype_bytes(bad) == -1
        with pytest.raises(api.XpngError):
            api.dtype_bytes(bad)


CONSTANT_SETS = {
    "unit": ([f32_of(1.0 / 255.0)] * 4, [0.0] * 4),
    "imagenet": consts_from(IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)),
    "ties_f16": ([2049.0 / 2048.0, 2051.0 / 2048.0], [0.0, 0.0]),
    "ties_bf16": ([257.0 / 256.0, 259.0 / 256.0], [0.0, 0.0]),
    "subnormal": ([2.0 ** -20], [0.0]),
    "overflow": ([300.0, -300.0], [0.0, 0.0]),
}


@pytest.mark.parametrize("name", sorted(CONSTANT_SETS))
def test_float_table_equals_the_checker(name):
    scale, bias = CONSTANT_SETS[name]
    for dtype in DTYPES:
        want, got = table(dtype, scale, bias), lib_table(dtype, scale, bias)
        assert got.shape == want.shape and np.array_equal(got, want), (name, dtype, np.argwhere(got != want)[:4])
    # what the sets are there for, on the checker's own tables
    if name == "ties_f16":
        t = table(F16, scale, bias).view(np.float16)
        assert (t[0][1], t[0][2], t[1][1], t[1][2]) == (1.0, 2.0, np.float16(1.002), np.float16(2.004))
        assert t[1][1].view(np.uint16) == 0x3C02 and t[0][1].view(np.uint16) == 0x3C00
    if name == "ties_bf16":
        t = table(BF16, scale, bias)
        assert (t[0][1], t[1][1]) == (0x3F80, 0x3F82)
    if name == "subnormal":
        t = table(F16, scale, bias)
        assert ((t[0][1:64] & 0x7C00) == 0).all() and (t[0][1:] != 0).any()                 # exponent field 0: subnormal, not flushed
    if name == "overflow":
        t = table(F16, scale, bias)
        assert t[0][255] == 0x7C00 and t[1][255] == 0xFC00 and t[0][200] != 0x7C00
    if name == "imagenet":                                          # "one FMA", not "multiply, then add": the two differ in f32
        s, b = scale, bias
        mul_add = np.array([[np.float32(np.float32(v) * np.float32(s[c])) + np.float32(b[c]) for v in range(256)] for c in range(3)], np.float32)
        assert (mul_add.view(np.uint32) != table(F32, s[:3], b[:3])).sum() > 50


def test_float_table_refusals():
    lib = api.hip_lib()
    buf = C.create_string_buffer(4 * 256 * 4)
    one, zero = (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0)
    assert lib.xpnghip_float_table(F32, 4, one, zero, buf) == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.xpnghip_float_table(F16, 3, (C.c_float * 4)(1, bad, 1, 1), zero, buf) == -1
        assert lib.xpnghip_float_table(F16, 3, one, (C.c_float * 4)(0, 0, bad, 0), buf) == -1
        with pytest.raises(api.XpngError):
            api.float_table(F16, [1.0, bad], [0.0, 0.0])
    for badC in (0, 5, -1):
        assert lib.xpnghip_float_table(F16, badC, one, zero, buf) == -1
    for dt in (0, 4):
        assert lib.xpnghip_float_table(dt, 3, one, zero, buf) == -1
    assert lib.xpnghip_float_table(F16, 3, None, zero, buf) == -1
    assert lib.xpnghip_float_table(F16, 3, one, None, buf) == -1
    assert lib.xpnghip_float_table(F16, 3, one, zero, None) == -1
    assert np.array_equal(np.frombuffer(buf.raw, np.float32), np.tile(np.arange(256, dtype=np.float32), 4))   # a refused call writes nothing


def test_null_context_is_refused_by_the_float_entry_point():
    lib = api.hip_lib()
    one, n = (C.c_void_p * 1)(0), (C.c_uint64 * 1)(0)
    assert lib.xpnghip_decode_varsize_device_batch_as_float(None, 1, one, n, 1, None, one, 0, F16, None, None, None) != 0
    assert "null context" in api._err()


def _host_files(po, tmp_path):
    """two oracle-written level-7 files and the committed 11-byte single-colour golden, with the oracle's decode of each (as
    tests/test_layouts.py builds them)"""
    from xpng_amd.synth import synth_raster
    paths = []
    for (w, h, alpha) in [(5, 7, False), (3, 3, True)]:
        p = tmp_path / f"l7_{w}x{h}_{int(alpha)}.xpng"
        p.write_bytes(po.encode_image(7, synth_raster("noise" if alpha else "photo", w, h, alpha, seed=w)))
        paths.append(str(p))
    single = os.path.join(GOLD, "imgfull_30d5c8.L2.xpng")
    assert os.path.getsize(single) == 11
    paths.insert(1, single)
    return paths, [po.decode_image(open(p, "rb").read()) for p in paths]


def test_load_files_float_answers_host_kinds_without_a_gpu(po, tmp_path):
    from xpng_amd import tensors
    paths, want = _host_files(po, tmp_path)
    assert [r.shape for r in want] == [(7, 5, 3), (1000, 1000, 3), (3, 3, 4)]
    mean, std = IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)
    for dtype in DTYPES:
        for ch in (None, 3, 4):
            n = ch or 4
            tabs = {c: table(dtype, *consts_from(mean[:c], std[:c])) for c in (3, 4)}
            for lay in ("hwc", "chw"):
                for bgr in (False, True):
                    if ch is None:                               # the files' own counts differ: a scalar mean / std serves both
                        kw = dict(mean=0.25, std=0.5)
                        tabs = {c: table(dtype, *consts_from([0.25] * c, [0.5] * c)) for c in (3, 4)}
                    else:
                        kw = dict(mean=mean[:n], std=std[:n])
                    got = tensors.load_files(paths, layout=lay, channels=ch, bgr=bgr, device="cpu", dtype=_torch_dtype(dtype), stack=False, **kw)
                    assert isinstance(got, list) and len(got) == len(paths)
                    for g, r in zip(got, want):
                        c = ch or r.shape[2]
                        w = expect(r, lay == "chw", bgr, c, tabs[c])
                        assert g.device.type == "cpu" and g.dtype == _torch_dtype(dtype) and g.is_contiguous() and tuple(g.shape) == w.shape, (lay, ch, bgr)
                        assert np.array_equal(_bits(g, dtype), w), (dtype, lay, ch, bgr, r.shape)
    # the defaults: mean 0, std 1 is v / 255 as one FMA with scale float32(1 / 255)
    got = tensors.load_files(paths[:1], device="cpu", dtype=_torch_dtype(F32))
    assert np.array_equal(_bits(got[0], F32), expect(want[0], True, False, 3, table(F32, [f32_of(1 / 255.0)] * 3, [0.0] * 3)))
    # uint8 stays what it was
    import torch
    got = tensors.load_files(paths, layout="hwc", device="cpu")
    for g, r in zip(got, want):
        assert g.dtype == torch.uint8 and np.array_equal(g.numpy(), r)


def test_load_files_stack_and_misuse_without_a_gpu(po, tmp_path):
    import torch
    from xpng_amd import tensors
    from xpng_amd.synth import synth_raster
    paths, rasters = [], []
    for k, alpha in enumerate((False, True)):
        r = synth_raster("noise", 6, 5, alpha, seed=k + 3)
        p = tmp_path / f"s{k}.xpng"
        p.write_bytes(po.encode_image(7, r))
        paths.append(str(p))
        rasters.append(po.decode_image(p.read_bytes()))
    assert [r.shape[2] for r in rasters] == [3, 4]
    t = tensors.load_files(paths, channels=3, device="cpu", dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, stack=True)
    tab = table(F16, *consts_from(IMAGENET_MEAN, IMAGENET_STD))
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (2, 3, 5, 6) and t.is_contiguous() and t.dtype == torch.float16
    for i, r in enumerate(rasters):
        assert np.array_equal(_bits(t[i], F16), expect(r, True, False, 3, tab)), i
    u = tensors.load_files(paths, layout="hwc", channels=4, bgr=True, device="cpu", stack=True)      # uint8 stacks too
    assert tuple(u.shape) == (2, 5, 6, 4) and u.dtype == torch.uint8 and u.is_contiguous()
    for i, r in enumerate(rasters):
        assert np.array_equal(u[i].numpy(), arrange(r, False, True, 4)), i
    other = tmp_path / "other.xpng"
    other.write_bytes(po.encode_image(7, synth_raster("noise", 6, 4, False, seed=9)))
    with pytest.raises(api.XpngError) as e:
        tensors.load_files(paths + [str(other)], channels=3, device="cpu", stack=True)
    assert "other.xpng" in str(e.value)
    with pytest.raises(api.XpngError):                              # channels None: an RGB and an RGBA file do not stack
        tensors.load_files(paths, device="cpu", stack=True)
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, device="cpu", mean=0.5)
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, device="cpu", std=[1, 1, 1])
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, channels=3, device="cpu", dtype=torch.float16, std=0)
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, channels=3, device="cpu", dtype=torch.float16, std=[0.5, 0.0, 0.5])
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, channels=3, device="cpu", dtype=torch.float16, mean=[0.5, 0.5])
    with pytest.raises(api.XpngError):
        tensors.load_files(paths, channels=3, device="cpu", dtype=torch.float64)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches(po):
    """per (mode, alpha): dims, the rasters and the oracle's tile blobs - computed once, never changed"""
    from xpng_amd.synth import synth_raster
    kinds = ["photo", "noise", "gray", "flat"]
    out = {}
    for mode, alpha in FORMATS:
        dims = RGBA_DIMS if alpha else RGB_DIMS
        rasters = [synth_raster(kinds[i % 4], w, h, alpha, seed=i + 1) for i, (w, h) in enumerate(dims)]
        # the value coverage the comparisons rest on: every table entry of every colour channel is used
        for c in range(3):
            assert len(np.unique(np.concatenate([r[..., c].ravel() for r in rasters]))) == 256, (mode, alpha, c)
        if alpha:
            a = np.unique(np.concatenate([r[..., 3].ravel() for r in rasters]))
            assert a[0] == 0 and a[-1] == 255 and len(a) >= 100
        blobs = [po.encode_tiles(mode, r) for r in rasters]
        for r, b, (w, h) in zip(rasters[-3:], blobs[-3:], dims[-3:]):
            assert np.array_equal(po.decode_tiles(mode, b, w, h, r.shape[2]), r)
        out[(mode, alpha)] = (dims, rasters, blobs)
    return out


def _decode_float(ctx, mode, d_b, lens, word, dtype, scale, bias, offs=None, expect_status=0, arena=None):
    """the images' elements as bit patterns, flat"""
    ch = api.layout_channels(word, ctx.pxsz)
    sizes = [ES[dtype] * ch * w * h for (w, h) in ctx.dims]
    ar = arena or Arena(sizes, ES[dtype])
    ctx.decode_batch_as_float(mode, [t.data_ptr() for t in d_b], lens, ar.ptrs, word, dtype, scale and scale[:ch], bias and bias[:ch], tile_offs=offs)
    assert ctx.decode_status() == expect_status
    return [g.view(BITS[dtype]) for g in ar.fetch(sizes)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,alpha", FORMATS)
def test_decode_into_every_float_layout(gpu, batches, mode, alpha, dtype):
    """All 12 layout words with four different (scale, bias) pairs per channel position: the image's elements are the checker's
    table entries of the rearranged oracle raster, every sentinel byte before and behind is intact; the workspace does not grow
    with the word; both size walks agree; two dtypes back to back on the same pointers."""
    import torch
    dims, rasters, blobs = batches[(mode, alpha)]
    px = 4 if alpha else 3
    scale, bias = mixed_consts(dtype)
    tab = table(dtype, scale, bias)
    ctx = gpu.MixedContext(dims, px)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ws0 = None
        for word in WORDS:
            got = _decode_float(ctx, mode, d_b, lens, word, dtype, scale, bias)
            for i, (g, r) in enumerate(zip(got, rasters)):
                w = expect_word(r, word, tab).reshape(-1)
                assert np.array_equal(g, w), (hex(word), dtype, i, dims[i], np.argwhere(g != w)[:4].ravel())
            ws0 = ws0 or ctx.workspace_bytes()
        assert abs(ctx.workspace_bytes() - ws0) <= 4096               # no second staging raster, whatever the layout
        # host-given offsets against the device-side walk
        word = api.layout(planar=True, bgr=True, channels=7 - px)
        for a, b in zip(_decode_float(ctx, mode, d_b, lens, word, dtype, scale, bias, _offsets(blobs, ctx)),
                        _decode_float(ctx, mode, d_b, lens, word, dtype, scale, bias)):
            assert np.array_equal(a, b)
        # two dtypes, back to back, on the same output pointers: the buffers have room for f32, the narrow call leaves the rest
        ar = Arena([4 * 4 * w * h for (w, h) in dims], 4)
        word = api.layout(planar=dtype != F32, bgr=True, channels=4)
        for dt in (F32, F16 if dtype == F32 else dtype):
            ar.refill()
            s2, b2 = mixed_consts(dt)
            t2 = table(dt, s2, b2)
            for i, (g, r) in enumerate(zip(_decode_float(ctx, mode, d_b, lens, word, dt, s2, b2, arena=ar), rasters)):
                assert np.array_equal(g, expect_word(r, word, t2).reshape(-1)), (hex(word), dt, i)
        torch.cuda.synchronize()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_float_matches_uint8_layout_call(gpu, batches):
    """scale 1, bias 0, f32: the float call gives the uint8 layout call's bytes converted by numpy, for every word."""
    dims, rasters, blobs = batches[(1, True)]
    ctx = gpu.MixedContext(dims, 4)
    try:
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        for word in WORDS:
            ch = api.layout_channels(word, 4)
            u8 = Arena([ch * w * h for (w, h) in dims], 1)
            ctx.decode_batch_as(1, [t.data_ptr() for t in d_b], lens, u8.ptrs, word)
            assert ctx.decode_status() == 0
            got = _decode_float(ctx, 1, d_b, lens, word, F32, [1.0] * 4, [0.0] * 4)
            none = _decode_float(ctx, 1, d_b, lens, word, F32, None, None) if word == WORDS[0] else got   # NULL = ones / zeros
            for i, (a, b, c) in enumerate(zip(u8.fetch(), got, none)):
                assert np.array_equal(a.astype(np.float32).view(np.uint32), b) and np.array_equal(b, c), (hex(word), i)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_rejected_tile_and_misuse(gpu, po):
    """One tile of one image gets type byte 0x7F: the launch reports 1 and every other image is exact.  Misuse is refused before
    device work: the error names the value and no byte of the arena changes."""
    from xpng_amd.synth import synth_raster
    lib = api.hip_lib()
    dims = [(300, 200), (889, 445), (100, 100), (64, 70)]
    rasters = [synth_raster("photo", w, h, True, seed=s + 1) for s, (w, h) in enumerate(dims)]
    blobs = [po.encode_tiles(1, r) for r in rasters]
    scale, bias = mixed_consts(F16)
    tab = table(F16, scale, bias)
    ctx = gpu.MixedContext(dims, 4)
    try:
        k = 1
        offs = _offsets(blobs, ctx)
        bad = bytearray(blobs[k])
        bad[offs[k][1] + 3] = 0x7F                               # top byte of the tile's first little-endian word
        bb = blobs[:k] + [bytes(bad)] + blobs[k + 1:]
        word = api.layout(planar=True, channels=3)
        got = _decode_float(ctx, 1, _upload(bb), [len(b) for b in bb], word, F16, scale, bias, expect_status=1)
        for i, (g, r) in enumerate(zip(got, rasters)):
            if i != k:
                assert np.array_equal(g, expect_word(r, word, tab).reshape(-1)), i
        d_b, lens = _upload(blobs), [len(b) for b in blobs]
        ins = [t.data_ptr() for t in d_b]
        outs = Arena([4 * 4 * w * h for (w, h) in dims], 4)
        assert all(p % 4 == 0 for p in outs.ptrs)

        def refused(words, fn):
            with pytest.raises(gpu.XpngError) as e:
                fn()
            assert all(w in str(e.value) for w in words), (words, str(e.value))
            assert outs.untouched(), words

        odd = [outs.ptrs[0], outs.ptrs[1] + 1, outs.ptrs[2], outs.ptrs[3]]
        refused(["aligned", "%x" % odd[1], "image 1"], lambda: ctx.decode_batch_as_float(1, ins, lens, odd, word, F16))
        two = [outs.ptrs[0], outs.ptrs[1], outs.ptrs[2] + 2, outs.ptrs[3]]
        refused(["aligned", "%x" % two[2], "image 2"], lambda: ctx.decode_batch_as_float(1, ins, lens, two, word, F32))
        ctx.decode_batch_as_float(1, ins, lens, two, word, BF16)      # (2 mod 4 is fine for a 2-byte element)
        assert ctx.decode_status() == 0
        outs.refill()
        refused(["dtype 0", "xpnghip_decode_varsize_device_batch_as"], lambda: ctx.decode_batch_as_float(1, ins, lens, outs.ptrs, word, 0))
        refused(["dtype 4"], lambda: ctx.decode_batch_as_float(1, ins, lens, outs.ptrs, word, 4))
        refused(["scale[1]", "nan"], lambda: ctx.decode_batch_as_float(1, ins, lens, outs.ptrs, word, F16, [1.0, float("nan"), 1.0]))
        refused(["bias[2]", "inf"], lambda: ctx.decode_batch_as_float(1, ins, lens, outs.ptrs, word, F16, None, [0.0, 0.0, float("inf")]))
        for badword in (0x004, 0x500, 0x1000):
            refused(["layout", "%#x" % badword], lambda: ctx.decode_batch_as_float(1, ins, lens, outs.ptrs, badword, F16))
        refused(["nimg"], lambda: ctx.decode_batch_as_float(1, ins[:2], lens[:2], outs.ptrs[:2], word, F16))
        refused(["null"], lambda: ctx.decode_batch_as_float(1, ins, lens, [outs.ptrs[0], 0, outs.ptrs[2], outs.ptrs[3]], word, F16))
        plain = gpu.Context(300, 200, 4)
        try:
            vp, u64 = C.c_void_p, C.c_uint64
            one_in, one_out, one_len = (vp * 1)(ins[0]), (vp * 1)(outs.ptrs[0]), (u64 * 1)(lens[0])
            assert lib.xpnghip_decode_varsize_device_batch_as_float(plain._h, 1, one_in, one_len, 1, None, one_out, word, F16, None, None, None) != 0
            assert "mixed context" in api._err()
        finally:
            plain.close()
        assert outs.untouched()
        # the context still works after all that
        for g, r in zip(_decode_float(ctx, 1, d_b, lens, word, F16, scale, bias), rasters):
            assert np.array_equal(g, expect_word(r, word, tab).reshape(-1))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_load_files_float_on_goldens(gpu, manifest):
    """load_files on committed reference-written goldens of level 1 and level 2, float16 with ImageNet mean / std, planar,
    channels=3, against the checker applied to api.load of each file; then stack=True on an RGB and an RGBA golden of one size."""
    import torch
    from xpng_amd import tensors
    names = ["crop_evil", "crop_olaf", "img_juicy", "img_pigz-logo", "imgfull_pe4en_k", "special_opaque_alpha"]
    files = sorted({manifest[n][lv]["file"] for n in names for lv in ("L1", "L2")})
    paths = [os.path.join(GOLD, f) for f in files]
    heads = [open(p, "rb").read(8) for p in paths]
    assert {(h[3], h[7] & 1) for h in heads} >= {(1, 0), (1, 1), (2, 0)}
    tab = table(F16, *consts_from(IMAGENET_MEAN, IMAGENET_STD))
    want = [gpu.load(p) for p in paths]
    got = tensors.load_files(paths, layout="chw", channels=3, dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD)
    assert len(got) == len(paths)
    for p, g, r in zip(paths, got, want):
        assert g.is_cuda and g.dtype == torch.float16 and g.is_contiguous() and tuple(g.shape) == (3,) + r.shape[:2], p
        assert np.array_equal(_bits(g, F16), expect(r, True, False, 3, tab)), p
    pair = [os.path.join(GOLD, manifest[n]["L1"]["file"]) for n in ("synth_photo_64x64_rgb", "synth_photo_64x64_rgba")]
    pw = [gpu.load(p) for p in pair]
    assert [r.shape for r in pw] == [(64, 64, 3), (64, 64, 4)]
    t = tensors.load_files(pair, layout="chw", channels=3, dtype=torch.float16, mean=IMAGENET_MEAN, std=IMAGENET_STD, stack=True)
    assert t.is_cuda and tuple(t.shape) == (2, 3, 64, 64) and t.is_contiguous() and t.dtype == torch.float16
    for i, r in enumerate(pw):
        assert np.array_equal(_bits(t[i], F16), expect(r, True, False, 3, tab)), i
    u = tensors.load_files(pair, layout="hwc", channels=4, stack=True)                         # uint8, interleaved, stacked
    assert tuple(u.shape) == (2, 64, 64, 4) and u.dtype == torch.uint8
    for i, r in enumerate(pw):
        assert np.array_equal(u[i].cpu().numpy(), arrange(r, False, False, 4)), i
